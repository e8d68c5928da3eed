"""Host-only restatements of the update tail (csrc/bdof_kernels.h: adam_voxel / k_adam, k_reg_value, k_mask_shrink; their host
code bdof_adam_step_slab, bdof_regularizer_value, bdof_mask_shrink in csrc/bdof_capi.hip), the error bounds the device is held
to, and the comparisons and case drivers that tests/test_gpu_update_tail.py (device) and tests/test_adam_reference.py (float32
emulation, with and without planted errors) both run.

Three things per operation:
  *_reference   float64, written from the formulas of oracle/bdof_oracle.py (regularizer_grad, apply_gradient_adam,
                regularizer) in the device's [X][Z][Y] layout of (delta, beta) pairs, with np.roll for the periodic stencil;
                next to every result it returns the per-element bound derived below.
  *_float32     the kernel's arithmetic restated operation by operation in numpy float32 (every operation rounds, nothing is
                fused), with the kernel's own flat-index split and neighbour addressing; `plant` names one deliberate error.
  check_*       the comparisons; run_* the cases (data, calls, comparisons) for a `step` / `shrink` / `reg` callable that is
                either the device or the emulation.

The bound (u = 2^-24, the unit round-off of float32 round-to-nearest; all constants below are the float64 ones)
---------------------------------------------------------------------------------------------------------------
The library is built with -O3 and no fast-math flag: hipcc then contracts a * b + c into one fused multiply-add where it likes
(-ffp-contract=fast is its default for device code) and keeps sqrtf and the float32 division correctly rounded (its default
-fhip-fp32-correctly-rounded-divide-sqrt): one rounding of relative size u each.  A fused multiply-add rounds once where the
unfused pair rounds twice, so counting the unfused roundings covers either contraction.  No quantity below underflows (asserted
on the host: every non-zero product is above 2^-120), so every rounding is relative.

Gradient.  gd = g g_scale + alpha sgn(x) + gamma T, T the integer sum of the six stencil signs (exact on the device: the sign
of a float32 difference is the sign of the exact difference; sgn and the integer sum are exact).  With
A = |g g_scale| + |alpha sgn x| + |gamma T|, the sum of the magnitudes of the terms:
  each term carries one float32 constant (g_scale, alpha, gamma: c_float arguments)                 u A
  the product g g_scale, the sum with alpha sgn(x) (alpha * {-1, 0, 1} is exact), the product gamma T,
  the last sum: u |g g_scale| + u (|g g_scale| + |alpha|) + u |gamma T| + u A                    <= 3 u A
      E_g = 4 u A          (beta has no TV term: fewer roundings, the same bound)
First moment.  m' = (1 - b1) gd + b1 m, a = (1 - b1) |gd|, b = b1 |m|: the constants 1 - b1 and b1 as adam_args rounds them
to float32 (u (a + b)), two products (u a + u b), the sum (u (a + b)); the cancellation of the two terms is thereby charged
to their magnitudes, not to |m'|:
      E_m = (1 - b1) E_g + 3 u (a + b)                         <= 7 u ((1 - b1) A + b1 |m|), under the cap of 8 u (...)
Second moment.  v' = ((1 - b2) gd) gd + b2 v, a = (1 - b2) gd^2, b = b2 v: the square inherits 2 |gd| E_g + E_g^2; constants
u (a + b); three products u a + u a + u b; the sum u (a + b):
      E_v = (1 - b2) (2 |gd| E_g + E_g^2) + 4 u a + 3 u b      <= (12 u + 16 u^2) (1 - b2) A^2 + 3 u b2 v, cap 16 u (...)
Step.  mh = m' / bc1, vh = v' / bc2 (bc = 1 - b^(i_batch + 1) formed in float64, its reciprocal rounded to float32):
      E_mh = E_m / bc1 + 2 u |mh|,  E_vh = E_v / bc2 + 2 u vh        (constant, product)
  s = sqrt(vh): |sqrt(a) - sqrt(b)| = |a - b| / (sqrt a + sqrt b) <= min(sqrt|a - b|, |a - b| / sqrt b), plus sqrtf's rounding:
      E_s = min(sqrt(E_vh), E_vh / s) + u (s + that)
  d = s + eps:  E_d = E_s + u eps (the constant) + u (d + E_s + u eps) (the sum);   d_lo = d - E_d > 0 (asserted)
  q = lr mh:    E_q = lr E_mh + 2 u (|q| + lr E_mh)                  (constant, product)
  r = q / d:    E_r = (E_q + |r| E_d) / d_lo, then the division's rounding u (|r| + E_r)
  x' = x - r:   E_x = E_r + u (|x - r| + E_r)                        (the final subtraction)
The mask multiplies by 0, 1 or 0.5 (exact): E_x |mask|.  The clip max(., 0) moves no two numbers apart: E_x stands.
All three bounds get a factor 1 + 2^-10 for the second-order terms left out and the float64 reference's own rounding.
Outside the slab [x0, x0 + nx) nothing may change: bound 0.

Caps (conditions on the bound, asserted before every comparison so that a bound cannot hide a failure):
  x_new <= 1e-5 lr;   m <= 8 u ((1 - b1) A + b1 |m|);   v <= 16 u ((1 - b2) A^2 + b2 |v|).

Regulariser value.  k_reg_value forms |delta|, |beta| exactly, the stencil differences in float32 (one rounding, u per term),
and adds everything in float64 in a fixed tree over n voxels: TV <= (u + n 2^-53) sum|term|, the L1 sums <= n 2^-53 sum.
"""
import math
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24
SLACK = 1 + 2.0 ** -10
NO_UNDERFLOW = 2.0 ** -120
SENTINEL = -777.25                 # tests/test_gpu_gradient_gathers.py's: what an output holds before the call
f32, f64 = np.float32, np.float64

SHAPES_3 = [(5, 3, 7), (9, 4, 6)]                                     # (NXv, NZv, NYv): three different extents
EXACT_SHAPES = SHAPES_3 + [(1, 4, 5), (4, 1, 5), (4, 5, 1),            # an extent of 1 on each axis: the stencil meets itself
                           (2, 3, 5), (3, 2, 5), (3, 5, 2),            # an extent of 2: both neighbours are the same voxel
                           (1, 1, 1)]
STRIDED_SHAPE = (33, 180, 181)                                        # 1 075 140 voxels (= 4 mod 8) > 16 * 256 CUs * 256
EXACT = dict(g_scale=0.5, alpha_d=8., alpha_b=16., gamma=1., lr=0.5, b1=0.5, b2=0.25, eps=1., i_batch=1, clip=1)
EXACT_VARIANTS = {
    'tv_mask_clip': dict(gamma=1., mask=True, clip=1),
    'gamma0': dict(gamma=0., mask=True, clip=1),                       # the branch that skips the stencil
    'no_mask_no_clip': dict(gamma=1., mask=False, clip=0),             # negative results survive
    'mask_no_clip': dict(gamma=1., mask=True, clip=0),
}
BOUNDED_SHAPE = SHAPES_3[1]
I_BATCHES = (0, 1, 2, 3, 500)
PRODUCTION = dict(g_scale=0.5, alpha_d=1.5e-8, alpha_b=1.5e-9, lr=1e-7, eps=1e-8)
BOUNDED_CASES = dict(
    [('g{:g}_gamma{:g}'.format(s, gm), dict(sigma=s, gamma=gm, b1=0.9, b2=0.999, mask=True, clip=1))
     for s in (1e-4, 1e-8, 1.) for gm in (1e-9, 1e-11)] +
    [('g1e-08_gamma1e-09_b0.8_0.99', dict(sigma=1e-8, gamma=1e-9, b1=0.8, b2=0.99, mask=True, clip=1)),
     ('g0.0001_gamma1e-09_no_mask_no_clip', dict(sigma=1e-4, gamma=1e-9, b1=0.9, b2=0.999, mask=False, clip=0))])
SHRINK_NS = (1, 255, 256, 257)
SHRINK_THRESHOLDS = (float(f32(1e-15)), 0., 0.5)


# ================================================================================================================================
# bdof_adam_step_slab
# ================================================================================================================================
def adam_constants(b1, b2, i_batch):
    """What adam_args (csrc/bdof_capi.hip) makes of the float32 b1, b2 it is handed: the 7-digit decimal the caller meant, and
    the bias corrections 1 - b^(i_batch + 1), all float64."""
    b1d, b2d = round(float(f32(b1)) * 1e7) / 1e7, round(float(f32(b2)) * 1e7) / 1e7
    return b1d, b2d, 1.0 - b1d ** (i_batch + 1), 1.0 - b2d ** (i_batch + 1)


def _tv_signs(d):
    """T: for every axis sgn(c - previous) - sgn(next - c), periodic (oracle total_variation_3d_grad)"""
    t = np.zeros_like(d)
    for ax in range(3):
        t += np.sign(d - np.roll(d, 1, axis=ax)) - np.sign(np.roll(d, -1, axis=ax) - d)
    return t


def adam_step_reference(x_old, g, m0, v0, mask, x_new_prior, g_scale, alpha_d, alpha_b, gamma, lr, b1, b2, eps, i_batch, clip,
                        x0=0, nx=None):
    """One call of bdof_adam_step_slab in float64.  x_old, g, m0, v0, x_new_prior: (NXv, NZv, NYv, 2); mask (NXv, NZv, NYv) or
    None.  Returns x_new, m, v (outside the slab: the priors), their bounds bx, bm, bv and the caps cap_x, cap_m, cap_v."""
    x, g, m0, v0 = (np.asarray(a, dtype=f64) for a in (x_old, g, m0, v0))
    NXv = x.shape[0]
    nx = NXv - x0 if nx is None else nx
    b1d, b2d, bc1, bc2 = adam_constants(b1, b2, i_batch)
    t_data = g * g_scale
    t_l1 = np.array([alpha_d, alpha_b]) * np.sign(x)
    t_tv = np.zeros_like(x)
    if gamma != 0:
        t_tv[..., 0] = gamma * _tv_signs(x[..., 0])
    gd = t_data + t_l1 + t_tv
    A = np.abs(t_data) + np.abs(t_l1) + np.abs(t_tv)
    m = (1 - b1d) * gd + b1d * m0
    v = (1 - b2d) * gd ** 2 + b2d * v0
    mh, vh = m / bc1, v / bc2
    s = np.sqrt(vh)
    d = s + eps
    q = lr * mh
    r = q / d
    pre = x - r
    mk = np.ones(x.shape[:3]) if mask is None else np.asarray(mask, dtype=f64)
    xn = pre * mk[..., None]
    if clip:
        xn = np.maximum(xn, 0.)
    # ---- the bounds of the module docstring -----------------------------------------------------------------------------
    for prod in ((1 - b1d) * np.abs(gd), b1d * np.abs(m0), (1 - b2d) * gd ** 2, b2d * v0, vh, np.abs(q), np.abs(t_data)):
        assert not np.any((prod != 0) & (prod < NO_UNDERFLOW)), 'a product would underflow in float32: the bound does not cover it'
    Eg = 4 * U * A
    am, bm_ = (1 - b1d) * np.abs(gd), b1d * np.abs(m0)
    Em = (1 - b1d) * Eg + 3 * U * (am + bm_)
    av, bv_ = (1 - b2d) * gd ** 2, b2d * v0
    Ev = (1 - b2d) * (2 * np.abs(gd) * Eg + Eg ** 2) + 4 * U * av + 3 * U * bv_
    Emh = Em / bc1 + 2 * U * np.abs(mh)
    Evh = Ev / bc2 + 2 * U * vh
    with np.errstate(divide='ignore', invalid='ignore'):
        Es = np.where(s > 0, np.minimum(np.sqrt(Evh), Evh / s), np.sqrt(Evh))
    Es = Es + U * (s + Es)
    Ed = Es + U * eps + U * (d + Es + U * eps)
    d_lo = d - Ed
    assert np.all(d_lo > 0)
    Eq = lr * Emh + 2 * U * (np.abs(q) + lr * Emh)
    Er = (Eq + np.abs(r) * Ed) / d_lo
    Er = Er + U * (np.abs(r) + Er)
    Ex = (Er + U * (np.abs(pre) + Er)) * np.abs(mk)[..., None]
    bx, bm, bv = Ex * SLACK, Em * SLACK, Ev * SLACK
    cap_x = np.full(x.shape, 1e-5 * lr)
    cap_m = 8 * U * ((1 - b1d) * A + b1d * np.abs(m0))
    cap_v = 16 * U * ((1 - b2d) * A ** 2 + b2d * np.abs(v0))
    # ---- the slab range ---------------------------------------------------------------------------------------------------
    out = np.ones(NXv, dtype=bool)
    out[x0:x0 + nx] = False
    xn[out], m[out], v[out] = np.asarray(x_new_prior, dtype=f64)[out], m0[out], v0[out]
    for b in (bx, bm, bv):
        b[out] = 0
    return SimpleNamespace(x_new=xn, m=m, v=v, bx=bx, bm=bm, bv=bv, cap_x=cap_x, cap_m=cap_m, cap_v=cap_v, A=A, lr=lr, inside=~out)


def adam_step_float32(x_old, g, m0, v0, mask, x_new_prior, g_scale, alpha_d, alpha_b, gamma, lr, b1, b2, eps, i_batch, clip,
                      x0=0, nx=None, plant=None):
    """k_adam + adam_voxel with every operation rounded to float32 (numpy float32 arrays: no fusion), adam_args' constants.
    plant: None, 'wrap' (z + 1 at the last z plane does not wrap), 'swap_xz' (the index split uses NXv where it means NZv),
    'sgn_beta' (sgn(beta) taken from delta), 'slab_late' (the slab starts one plane late), 'mask_transposed' (the mask read at
    [x][y][z])."""
    NXv, NZv, NYv = x_old.shape[:3]
    nx = NXv - x0 if nx is None else nx
    n = NXv * NZv * NYv
    b1d, b2d, bc1, bc2 = adam_constants(b1, b2, i_batch)
    gs, ad, ab, gm, lrf, epsf = (f32(c) for c in (g_scale, alpha_d, alpha_b, gamma, lr, eps))
    b1f, b2f, om1, om2, ibc1, ibc2 = (f32(c) for c in (b1d, b2d, 1.0 - b1d, 1.0 - b2d, 1.0 / bc1, 1.0 / bc2))
    xo, gg = np.asarray(x_old, dtype=f32).reshape(n, 2), np.asarray(g, dtype=f32).reshape(n, 2)
    x_new, m, v = (np.array(a, dtype=f32).reshape(n, 2) for a in (x_new_prior, m0, v0))
    slab = NZv * NYv
    first = x0 + 1 if plant == 'slab_late' else x0
    idx = np.arange(first * slab, max(first, x0 + nx) * slab)
    if idx.size == 0:
        return tuple(a.reshape(x_old.shape) for a in (x_new, m, v))
    y, r = idx % NYv, idx // NYv
    z, x = (r % NXv, r // NXv) if plant == 'swap_xz' else (r % NZv, r // NZv)
    xd, xb = xo[idx, 0], xo[idx, 1]
    gd = gg[idx, 0] * gs + ad * np.sign(xd)
    gb = gg[idx, 1] * gs + ab * np.sign(xd if plant == 'sgn_beta' else xb)
    if gm != 0:
        def at(coord, extent, stride, step):
            to = (coord + extent + step) % extent
            return xo[(idx - coord * stride + to * stride) % n, 0]       # (% n: only a planted split leaves the volume)
        ym, yp = at(y, NYv, 1, -1), at(y, NYv, 1, 1)
        zm, zp = at(z, NZv, NYv, -1), at(z, NZv, NYv, 1)
        xm, xp = at(x, NXv, slab, -1), at(x, NXv, slab, 1)
        if plant == 'wrap':
            zp = np.where(z == NZv - 1, xd, zp)
        sg = np.sign
        T = (sg(xd - ym) - sg(yp - xd) + sg(xd - zm) - sg(zp - xd) + sg(xd - xm) - sg(xp - xd)).astype(f32)
        gd = gd + gm * T
    for c, gc in ((0, gd), (1, gb)):
        assert gc.dtype == f32
        mc = om1 * gc + b1f * m[idx, c]
        vc = om2 * gc * gc + b2f * v[idx, c]
        m[idx, c], v[idx, c] = mc, vc
        nc = xo[idx, c] - lrf * (mc * ibc1) / (np.sqrt(vc * ibc2) + epsf)
        assert nc.dtype == f32
        if mask is not None:
            mk = np.asarray(mask, dtype=f32)
            mk = mk.reshape(NXv, NYv, NZv).transpose(0, 2, 1).reshape(n) if plant == 'mask_transposed' else mk.reshape(n)
            nc = nc * mk[idx]
        if clip:
            nc = np.maximum(nc, f32(0))
        x_new[idx, c] = nc
    return tuple(a.reshape(x_old.shape) for a in (x_new, m, v))


def _ratio(tag, got, want, bound):
    """every element: |got - want| <= bound, equality where the bound is 0; returns the largest error-to-bound ratio"""
    err = np.abs(np.asarray(got, dtype=f64) - want)
    assert err.shape == bound.shape
    zero = bound == 0
    n_bad0 = int(np.count_nonzero(err[zero]))
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = float(np.max(np.where(zero, 0., err / bound), initial=0.))
    print('   {}: {} elements, {} with bound 0 ({} of them off), largest |error| {:.3e}, largest error / bound {:.3f}'.format(
        tag, err.size, int(zero.sum()), n_bad0, float(err.max(initial=0.)), ratio))
    assert n_bad0 == 0, '{}: {} elements that had to come back unchanged did not'.format(tag, n_bad0)
    assert ratio <= 1, '{}: error / bound {}'.format(tag, ratio)
    return ratio


def check_adam(tag, got, ref, exact_mv):
    """got = (x_new, m, v) of one call against adam_step_reference's result: the caps first, then every element of all three.
    exact_mv: m and v by np.array_equal (the reference must survive float32).  Returns the ratios {x, m, v} (m, v: 0 if exact)."""
    x_new, m, v = got
    print(tag, ': largest bound of x_new / lr {:.3e} (cap 1e-5)'.format(float(ref.bx.max(initial=0.)) / ref.lr))
    assert np.all(ref.bx <= ref.cap_x) and np.all(ref.bm <= ref.cap_m) and np.all(ref.bv <= ref.cap_v), tag + ': a bound exceeds its cap'
    out = {'x': _ratio('x_new', x_new, ref.x_new, ref.bx)}
    if exact_mv:
        same_m, same_v = np.array_equal(m, ref.m), np.array_equal(v, ref.v)
        print('   m array_equal', same_m, ' v array_equal', same_v)
        assert same_m and same_v, tag + ': m or v differs from the float64 reference'
        out.update(m=0., v=0.)
    else:
        out.update(m=_ratio('m', m, ref.m, ref.bm), v=_ratio('v', v, ref.v, ref.bv))
    return out


def _mask_of(rng, shape):
    return rng.choice(np.array([0, 1, 0.5], dtype=f32), size=shape, p=[0.25, 0.5, 0.25])


def exact_data(shape, seed, with_mask=True):
    """integer-valued x_old, g, m0 in [-4, 4] (delta and beta independent, ties between neighbours everywhere), v0 in [0, 8]"""
    rng = np.random.default_rng(seed)
    full = tuple(shape) + (2,)
    x_old, g, m0 = (rng.integers(-4, 5, size=full).astype(f32) for _ in range(3))
    v0 = rng.integers(0, 9, size=full).astype(f32)
    return x_old, g, m0, v0, (_mask_of(rng, shape) if with_mask else None)


def sentinels(shape):
    return np.full(tuple(shape) + (2,), SENTINEL, dtype=f32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def exact_reference(*args, **kwargs):
    """adam_step_reference for an exact case: asserts, before anything is launched, that the reference's m and v are float32
    numbers (they survive the round trip), so that np.array_equal against them is a fair demand"""
    ref = adam_step_reference(*args, **kwargs)
    assert np.array_equal(ref.m.astype(f32).astype(f64), ref.m) and np.array_equal(ref.v.astype(f32).astype(f64), ref.v), \
        'the reference moments are not float32 numbers'
    return ref


def run_exact(step, shape, variant, seed=1):
    """one whole-volume call on integer data; step(x_old, g, m0, v0, mask, x_new_prior, x0=, nx=, **constants) -> (x_new, m, v)"""
    var = EXACT_VARIANTS[variant]
    k = dict(EXACT, gamma=var['gamma'], clip=var['clip'])
    x_old, g, m0, v0, mask = exact_data(shape, seed, var['mask'])
    ref = exact_reference(x_old, g, m0, v0, mask, sentinels(shape), **k)
    got = step(x_old, g, m0, v0, mask, sentinels(shape), x0=0, nx=shape[0], **k)
    out = check_adam('exact {} {}'.format(shape, variant), got, ref, True)
    if not var['clip'] and np.prod(shape) > 8:
        assert np.any(ref.x_new < 0) and np.any(got[0] < 0)               # negative results survive without the clip
    return out


def run_slabs(step, shape, seed=2):
    """every split point (nx = 0 at both ends included), the single planes x0 = 0 and x0 = NXv - 1: every call against its own
    reference (outside the slab nothing moves), the union of two slab calls against the whole call bit for bit"""
    k = dict(EXACT)
    NXv = shape[0]
    x_old, g, m0, v0, mask = exact_data(shape, seed)
    ref = exact_reference(x_old, g, m0, v0, mask, sentinels(shape), **k)
    whole = step(x_old, g, m0, v0, mask, sentinels(shape), x0=0, nx=NXv, **k)
    worst = check_adam('whole {}'.format(shape), whole, ref, True)['x']
    for cut in range(NXv + 1):
        state = (sentinels(shape), m0, v0)
        for x0, nx in ((0, cut), (cut, NXv - cut)):
            ref = exact_reference(x_old, g, state[1], state[2], mask, state[0], x0=x0, nx=nx, **k)
            state = step(x_old, g, state[1], state[2], mask, state[0], x0=x0, nx=nx, **k)
            worst = max(worst, check_adam('slab {} x0 {} nx {}'.format(shape, x0, nx), state, ref, True)['x'])
        same = all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(state, whole))
        print('   cut at', cut, ': union of the two slab calls bit-identical to the whole call:', same)
        assert same
    for x0 in (0, NXv - 1):
        ref = exact_reference(x_old, g, m0, v0, mask, sentinels(shape), x0=x0, nx=1, **k)
        got = step(x_old, g, m0, v0, mask, sentinels(shape), x0=x0, nx=1, **k)
        worst = max(worst, check_adam('single plane {} x0 {}'.format(shape, x0), got, ref, True)['x'])
        assert np.array_equal(_bits(got[0][x0]), _bits(whole[0][x0])) and np.array_equal(_bits(got[1][x0]), _bits(whole[1][x0]))
        assert np.count_nonzero(got[0] == f32(SENTINEL)) >= 2 * (NXv - 1) * shape[1] * shape[2]
    return worst


def run_strided(step, n_cu, shape=STRIDED_SHAPE, seed=3):
    """more voxels than 16 * n_cu * 256 threads, no multiple of 8: one whole call and one two-slab split; m, v exact"""
    k = dict(EXACT)
    n = int(np.prod(shape))
    print('strided volume', shape, ':', n, 'voxels against 16 * {} * 256 = {}'.format(n_cu, 16 * n_cu * 256), ', n mod 8 =', n % 8)
    assert n > 16 * n_cu * 256 and n % 8 != 0
    cut = shape[0] // 2 + 1
    assert cut * shape[1] * shape[2] % 8 != 0                           # neither slab's range divides among the 8 XCDs evenly
    x_old, g, m0, v0, mask = exact_data(shape, seed)
    ref = exact_reference(x_old, g, m0, v0, mask, sentinels(shape), **k)
    whole = step(x_old, g, m0, v0, mask, sentinels(shape), x0=0, nx=shape[0], **k)
    worst = check_adam('strided whole', whole, ref, True)['x']
    state = (sentinels(shape), m0, v0)
    for x0, nx in ((0, cut), (cut, shape[0] - cut)):
        ref = exact_reference(x_old, g, state[1], state[2], mask, state[0], x0=x0, nx=nx, **k)
        state = step(x_old, g, state[1], state[2], mask, state[0], x0=x0, nx=nx, **k)
        worst = max(worst, check_adam('strided slab x0 {} nx {}'.format(x0, nx), state, ref, True)['x'])
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(state, whole))
    return worst


def bounded_data(case, seed=5):
    """delta ~ U(0, 2e-6), beta ~ U(0, 2e-7), independent, 15 % zeros each; without the clip a quarter of each negative"""
    c = BOUNDED_CASES[case]
    rng = np.random.default_rng(seed)
    shape = BOUNDED_SHAPE
    x = np.stack([rng.uniform(0, 2e-6, size=shape), rng.uniform(0, 2e-7, size=shape)], axis=-1)
    if not c['clip']:
        x *= rng.choice([1., -1.], size=x.shape, p=[0.75, 0.25])
    x[rng.uniform(size=x.shape) < 0.15] = 0
    mask = _mask_of(rng, shape) if c['mask'] else None
    return x.astype(f32), mask, rng


def run_bounded(step, case):
    """i_batch = 0, 1, 2, 3, 500 at production magnitudes; every step's reference starts from the state the step under test
    left, so errors do not compound.  Returns the largest ratios {x, m, v} over the steps."""
    c = BOUNDED_CASES[case]
    k = dict(PRODUCTION, gamma=c['gamma'], b1=c['b1'], b2=c['b2'], clip=c['clip'])
    shape = BOUNDED_SHAPE
    x, mask, rng = bounded_data(case)
    m, v = np.zeros(x.shape, f32), np.zeros(x.shape, f32)
    worst = dict(x=0., m=0., v=0.)
    for i_batch in I_BATCHES:
        g = (c['sigma'] * rng.normal(size=x.shape)).astype(f32)
        ref = adam_step_reference(x, g, m, v, mask, sentinels(shape), i_batch=i_batch, **k)
        got = step(x, g, m, v, mask, sentinels(shape), x0=0, nx=shape[0], i_batch=i_batch, **k)
        r = check_adam('bounded {} i_batch {}'.format(case, i_batch), got, ref, False)
        worst = {key: max(worst[key], r[key]) for key in worst}
        x, m, v = (np.array(a, dtype=f32) for a in got)
    return worst


# ================================================================================================================================
# bdof_regularizer_value
# ================================================================================================================================
def _fsum(a):
    return math.fsum(a.reshape(-1)) if a.size <= 1 << 17 else float(np.sum(a))      # (the large case is integer-valued: exact either way)


def reg_value_reference(x):
    """[sum |delta|, sum |beta|, TV(delta)] of an (NXv, NZv, NYv, 2) volume in float64 and the three bounds of the docstring"""
    x = np.asarray(x, dtype=f64)
    d, n = x[..., 0], x[..., 0].size
    tv = sum(_fsum(np.abs(np.roll(d, 1, axis=ax) - d)) for ax in range(3))
    sums = np.array([_fsum(np.abs(d)), _fsum(np.abs(x[..., 1])), tv])
    return sums, sums * np.array([n * 2. ** -53, n * 2. ** -53, U + n * 2. ** -53])


def reg_value_float32(x):
    """k_reg_value: |.| exact, the three backward differences in float32, everything added in float64"""
    x = np.asarray(x, dtype=f32)
    d = x[..., 0]
    tv = sum(float(np.sum(np.abs(np.roll(d, 1, axis=ax) - d).astype(f64))) for ax in range(3))
    return np.array([float(np.sum(np.abs(d).astype(f64))), float(np.sum(np.abs(x[..., 1]).astype(f64))), tv])


def reg_data(shape, seed, production=False):
    rng = np.random.default_rng(seed)
    if not production:
        return rng.integers(-4, 5, size=tuple(shape) + (2,)).astype(f32)
    x = np.stack([rng.uniform(0, 2e-6, size=shape), rng.uniform(0, 2e-7, size=shape)], axis=-1)
    x[rng.uniform(size=x.shape) < 0.15] = 0
    return x.astype(f32)


def check_reg(tag, got, x, exact):
    want, bound = reg_value_reference(x)
    got = np.asarray(got, dtype=f64)
    print(tag, ': sums', got, 'reference', want, '|difference|', np.abs(got - want), 'bound', 0 if exact else bound)
    if exact:
        assert np.array_equal(got, want), (tag, got, want)
        return 0.
    assert np.all(np.abs(got - want) <= bound), (tag, got, want, bound)
    return float(np.max(np.abs(got - want) / bound))


# ================================================================================================================================
# bdof_mask_shrink
# ================================================================================================================================
def mask_shrink_reference(x, mask, thresh):
    """mask where delta > float32(thresh), 0 elsewhere (NaN compares false); x: (n, 2), mask: (n,)"""
    with np.errstate(invalid='ignore'):
        keep = np.asarray(x, dtype=f32)[:, 0] > f32(thresh)
    return np.where(keep, np.asarray(mask, dtype=f32), f32(0))


def mask_shrink_float32(x, mask, thresh, plant=None):
    """k_mask_shrink; plant='shrink_beta': the test reads beta"""
    with np.errstate(invalid='ignore'):
        keep = np.asarray(x, dtype=f32)[:, 1 if plant == 'shrink_beta' else 0] > f32(thresh)
    return np.where(keep, np.asarray(mask, dtype=f32), f32(0))


def shrink_data(n, thresh, seed=7):
    """delta around the threshold (itself, its float32 neighbours, 0, negatives, +inf, NaN); beta on the other side of it for two
    voxels out of three; mask out of 0, 1, 0.5, -2"""
    rng = np.random.default_rng(seed)
    t = f32(thresh)
    pool = np.array([t, np.nextafter(t, f32(np.inf)), np.nextafter(t, f32(-np.inf)), 0, -1, -1e-15, -t, np.inf, np.nan,
                     2 * t + f32(1e-15), 1, 0.25, 1e-15, 3e-7], dtype=f32)
    delta = pool[(np.arange(n) + rng.integers(0, len(pool))) % len(pool)] if n < len(pool) else \
        np.concatenate([pool, rng.choice(pool, size=n - len(pool))])
    with np.errstate(invalid='ignore'):
        kd = delta > t
    other = np.arange(n) % 3 != 2
    kb = np.where(other, ~kd, kd)
    beta = np.where(kb, rng.choice(np.array([1, np.inf, 7.5], dtype=f32), size=n), rng.choice(np.array([0, -1, -np.inf], dtype=f32), size=n))
    beta = beta.astype(f32)
    assert np.array_equal(beta > t, kb) and 3 * np.count_nonzero(kb != kd) >= n, 'beta > thresh must disagree with delta > thresh on a third'
    mask = rng.choice(np.array([0, 1, 0.5, -2], dtype=f32), size=n)
    mask[0] = 1                                                          # (n = 1: a mask of 0 would hide the test's outcome)
    return np.stack([delta, beta], axis=-1), mask


def check_shrink(tag, got_mask, x, mask, thresh):
    want = mask_shrink_reference(x, mask, thresh)
    bad = int(np.count_nonzero(np.asarray(got_mask) != want))
    print(tag, ': n', len(mask), 'thresh', thresh, 'kept', int(np.count_nonzero(want)), 'zeroed', int(np.count_nonzero((want == 0) & (mask != 0))),
          'elements off', bad)
    assert np.asarray(got_mask).dtype == f32 and bad == 0, tag


def run_shrink(shrink, n, thresh):
    """shrink(x (n, 2), mask (n,), thresh) -> the new mask"""
    x, mask = shrink_data(n, thresh)
    check_shrink('mask shrink', shrink(x, mask, thresh), x, mask, thresh)


def run_reg(reg, shape, production=False, seed=9):
    """reg(x (NXv, NZv, NYv, 2)) -> the three sums; returns the largest error-to-bound ratio (0 for the exact cases)"""
    x = reg_data(shape, seed, production)
    return check_reg('regulariser value {}{}'.format(shape, ' production magnitudes' if production else ''), reg(x), x, not production)
