"""The update tail through its own entry points, against the float64 restatements of tests/adam_reference.py:
  bdof_adam_step / bdof_adam_step_slab  (k_adam, adam_voxel: regulariser gradient, Adam, finite-support mask, clip),
  bdof_regularizer_value                (k_reg_value),
  bdof_mask_shrink                      (k_mask_shrink) and FullfieldSolver.shrink_wrap on top of it.
The one-pass tail, the sharded and the slab-wise solvers are held bit for bit to bdof_adam_step elsewhere (test_gpu_fused_tail.py,
test_gpu_dist.py); this file is what holds adam_voxel itself to the mathematics.

Every output lies between sentinel guards (Guarded of test_gpu_gradient_gathers.py); delta and beta are drawn independently, each
with its own zeros (and its own negative entries where the clip is off), so that no kernel can read one for the other unseen.

Exact cases.  x_old, g and the prior m are integers in [-4, 4], the prior v integers in [0, 8], g_scale = 0.5, alpha_d = 8,
alpha_b = 16, gamma = 1, b1 = 0.5, b2 = 0.25: every intermediate of m and v is a dyadic number of a few bits, so neither the
order nor the fusion of the operations can change it and the device must return the float64 reference's m and v exactly
(np.array_equal; that the reference survives float32 is asserted on the host).  x_new (lr = 0.5, eps = 1, i_batch = 1) is held
to the bound.  Outside a slab x_new keeps its sentinels and m, v their priors; the union of two slab calls is the whole call
bit for bit.

Bounded cases run at the magnitudes of production; every element of x_new, m and v is compared against a bound derived, not
measured, from the kernel's arithmetic; adam_step_reference forms it next to the reference and the docstring of
tests/adam_reference.py carries the derivation line by line.  In short, with u = 2^-24 and the float64 constants:
  the build (-O3, no fast-math flag) may contract any a * b + c into a fused multiply-add, which rounds once where the pair rounds
  twice — the unfused count below covers either —, and keeps sqrtf and the float32 division correctly rounded: u each;
  gradient   gd = g g_scale + alpha sgn(x) + gamma T (T: the exact integer sum of the stencil signs), A = the sum of the three
             magnitudes: the float32 constants g_scale, alpha, gamma (u A) and two products and two sums (<= 3 u A):  E_g = 4 u A;
  m' = (1 - b1) gd + b1 m: E_m = (1 - b1) E_g + 3 u ((1 - b1) |gd| + b1 |m|) — the float32 1 - b1 and b1 of adam_args, two products, one
             sum; the cancellation of the two terms is charged to their magnitudes;
  v' = ((1 - b2) gd) gd + b2 v: E_v = (1 - b2) (2 |gd| E_g + E_g^2) + 4 u (1 - b2) gd^2 + 3 u b2 v;
  bias corrections (float32 reciprocals of float64 1 - b^(i + 1)): E_mh = E_m / bc1 + 2 u |mh|, E_vh = E_v / bc2 + 2 u vh;
  s = sqrt(vh): E_s = min(sqrt(E_vh), E_vh / s) + u s;  d = s + eps: E_d = E_s + u eps + u d;  q = lr mh: E_q = lr E_mh + 2 u |q|;
  r = q / d: E_r = (E_q + |r| E_d) / (d - E_d) + u |r|;  the final subtraction x' = x - r: E_x = E_r + u |x'|; mask in {0, 0.5, 1}: exact;
  clip: no two numbers move apart.  No element is excluded.
The bounds are capped by 1e-5 lr, 8 u ((1 - b1) A + b1 |m|) and 16 u ((1 - b2) A^2 + b2 |v|); the caps are conditions, asserted on
the host before each comparison.  Each step's reference starts from the state downloaded from the device, so errors do not
compound.

Every test prints what it measured before it asserts; MEASUREMENTS.md section 7 quotes the ratios."""
import ctypes

import numpy as np
import pytest

import adam_reference as ar
import test_gpu_gradient_gathers as gg

pytestmark = pytest.mark.gpu

HIP_ATTRIBUTE_MULTIPROCESSOR_COUNT = 63          # hipDeviceAttributeMultiprocessorCount (hip_runtime_api.h)


class Device(object):
    """A configured context (bdof_regularizer_value needs its partial sums) and the three entry points as the callables the case
    drivers of adam_reference take."""

    def __init__(self):
        import __graft_entry__ as entry
        entry.build()
        from beyond_dof_amd import _lib
        from beyond_dof_amd.engine import MultisliceEngine
        self.eng = MultisliceEngine(64, 64, 2, 1, with_grad=False)
        self.ctx, self.lib, self.h = self.eng.ctx, self.eng.lib, self.eng.h
        self.up = lambda a: _lib.DeviceBuffer.from_host(self.ctx, np.ascontiguousarray(a))

    def compute_units(self):
        """of the ctx's device, asked of the HIP runtime the library has loaded"""
        paths = sorted(set(line.split()[-1] for line in open('/proc/self/maps') if 'libamdhip64' in line))
        n = ctypes.c_int(0)
        for path in paths:                # (a process that imported torch holds a second runtime, which sees no device)
            if ctypes.CDLL(path).hipDeviceGetAttribute(ctypes.byref(n), HIP_ATTRIBUTE_MULTIPROCESSOR_COUNT, self.ctx.device) == 0:
                break
        assert 16 <= n.value <= 1024, (paths, n.value)
        return n.value

    def step(self, x_old, g, m0, v0, mask, x_new_prior, x0, nx, g_scale, alpha_d, alpha_b, gamma, lr, b1, b2, eps, i_batch, clip):
        NXv, NZv, NYv = x_old.shape[:3]
        xo, gb = self.up(x_old.astype(np.float32)), self.up(g.astype(np.float32))
        mk = None if mask is None else self.up(mask.astype(np.float32))
        out = [gg.Guarded(self.ctx, np.asarray(a, dtype=np.float32)) for a in (x_new_prior, m0, v0)]
        args = (self.h, xo.ptr, out[0].ptr, gb.ptr, out[1].ptr, out[2].ptr, None if mk is None else mk.ptr, NXv, NZv, NYv,
                g_scale, alpha_d, alpha_b, gamma, lr, b1, b2, eps, i_batch, clip)
        if (x0, nx) == (0, NXv):
            self.ctx.check(self.lib.bdof_adam_step(*args))
        else:
            self.ctx.check(self.lib.bdof_adam_step_slab(*(args + (x0, nx))))
        self.ctx.sync()
        return tuple(o.download() for o in out)                       # (download() checks the guards)

    def reg(self, x):
        sums = (ctypes.c_double * 3)()
        buf = self.up(x.astype(np.float32))
        self.ctx.check(self.lib.bdof_regularizer_value(self.h, buf.ptr, x.shape[0], x.shape[1], x.shape[2], sums))
        return np.array(sums[:])

    def shrink(self, x, mask, thresh):
        xb, mb = gg.Guarded(self.ctx, x.astype(np.float32)), gg.Guarded(self.ctx, mask.astype(np.float32))
        self.ctx.check(self.lib.bdof_mask_shrink(self.h, xb.ptr, mb.ptr, len(mask), thresh))
        self.ctx.sync()
        assert np.array_equal(xb.download().view(np.uint32), x.astype(np.float32).view(np.uint32)), 'x was written'
        return mb.download()


@pytest.fixture(scope='module')
def dev():
    return Device()


# ================================================================================================================================
# bdof_adam_step, bdof_adam_step_slab
# ================================================================================================================================
@pytest.mark.parametrize('shape', ar.EXACT_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_adam_exact(dev, shape):
    """integer data: m and v equal the float64 reference's, x_new inside its bound; with and without the stencil, mask and clip"""
    for variant in ar.EXACT_VARIANTS:
        r = ar.run_exact(dev.step, shape, variant)
        print('exact', shape, variant, ': largest x_new error / bound', r['x'])


@pytest.mark.parametrize('shape', ar.SHAPES_3, ids=lambda s: 'x'.join(map(str, s)))
def test_adam_slabs(dev, shape):
    """every split point, nx = 0, the single planes at both ends: nothing outside the slab moves, the union is the whole call"""
    print('slabs', shape, ': largest x_new error / bound', ar.run_slabs(dev.step, shape))


def test_adam_grid_stride(dev):
    """more voxels than 16 workgroups of 256 per compute unit, no multiple of 8: k_adam's per-XCD chunks stride"""
    print('grid stride: largest x_new error / bound', ar.run_strided(dev.step, dev.compute_units()))


@pytest.mark.parametrize('case', list(ar.BOUNDED_CASES))
def test_adam_bounded(dev, case):
    """production magnitudes, i_batch 0, 1, 2, 3, 500: every element of x_new, m, v inside the derived bound"""
    print('bounded', case, ': largest error / bound', ar.run_bounded(dev.step, case))


# ================================================================================================================================
# bdof_regularizer_value
# ================================================================================================================================
@pytest.mark.parametrize('shape', ar.EXACT_SHAPES + [ar.STRIDED_SHAPE], ids=lambda s: 'x'.join(map(str, s)))
def test_regularizer_value_exact(dev, shape):
    """integer data, independent components: the three sums are the float64 reference's"""
    if shape == ar.STRIDED_SHAPE:
        n, n_cu = int(np.prod(shape)), dev.compute_units()
        print('k_reg_value launches at most', 2 * (16 * n_cu + 64) // 3, 'workgroups of 256 for', n, 'voxels')
        assert n > 2 * (16 * n_cu + 64) // 3 * 256
    ar.run_reg(dev.reg, shape)


def test_regularizer_value_production_magnitudes(dev):
    print('regulariser value: largest error / bound', ar.run_reg(dev.reg, ar.BOUNDED_SHAPE, production=True))


# ================================================================================================================================
# bdof_mask_shrink
# ================================================================================================================================
@pytest.mark.parametrize('thresh', ar.SHRINK_THRESHOLDS)
@pytest.mark.parametrize('n', ar.SHRINK_NS + (int(np.prod(ar.STRIDED_SHAPE)),))
def test_mask_shrink(dev, n, thresh):
    """delta at, just above and just below the threshold, 0, negative, inf, NaN; beta on the other side for two voxels of three"""
    ar.run_shrink(dev.shrink, n, thresh)


def test_shrink_wrap_solver():
    """set_mask + shrink_wrap on a volume of three extents, in the solver's (Y, X, Z) order"""
    from beyond_dof_amd.solver import FullfieldSolver
    Y, X, Z = 12, 10, 8
    thresh = 1e-15
    x, mask = ar.shrink_data(Y * X * Z, thresh, seed=8)
    x = np.where(np.isfinite(x), x, np.float32(2e-6))                       # (the solver makes the volume's modulation table from it)
    od, ob, mask = x[:, 0].reshape(Y, X, Z), x[:, 1].reshape(Y, X, Z), mask.reshape(Y, X, Z)
    with np.errstate(invalid='ignore'):
        assert 3 * np.count_nonzero((od > np.float32(thresh)) != (ob > np.float32(thresh))) >= od.size
    s = FullfieldSolver(Y, X, Z, 2, 1, 5000., 1e-7)
    s.set_volume(od, ob)
    s.set_mask(mask)
    s.shrink_wrap(thresh)
    s.ctx.sync()
    got = s.mask.download().transpose(2, 0, 1)                              # [X][Z][Y] -> (Y, X, Z)
    want = np.where(od > np.float32(thresh), mask, np.float32(0))
    print('shrink_wrap', (Y, X, Z), ': kept', np.count_nonzero(want), 'zeroed', np.count_nonzero((want == 0) & (mask != 0)),
          'elements off', np.count_nonzero(got != want))
    assert np.any(want != mask) and np.array_equal(got, want)
    d, b = s.get_volume()
    assert np.array_equal(d, od) and np.array_equal(b, ob)
