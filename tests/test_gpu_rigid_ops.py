"""bdof_rotate_rigid (k_rot_rigid<false>), bdof_rotate_rigid_adjoint (k_rot_rigid_adjoint) and bdof_set_object_rigid
(k_rot_rigid<true>) through their own entry points against the numpy restatement of tests/rigid_reference.py — the pattern of
tests/test_gpu_gradient_gathers.py: the kernels are fed directly, every output lies between sentinel-filled guards, rows outside
[row0, row0 + n_rows) must come back untouched, and no element is left out of any comparison.

Shapes: (NXv, NZv) = (7, 10); NYv in 6 (a partial wave), 64 (exactly one wave), 66 and 130 (one and two waves plus a remainder);
B in 1, 3, 5.

Exact cases: integer-valued data in [-4, 4] under the 24 signed permutation matrices with integer t (every weight exactly 0 or
1, every partial sum an integer far below 2^24): np.array_equal, with scale in 1, 0.5, 3 and accumulation from integers.

General cases: the tolerance is derived per element in rigid_reference (element_bound), not measured:
    |device - reference| <= 2^-24 (6 sum |g_i| + (n + 4) sum |w_i| |g_i|),   times scale, + 2^-24 |prior| when accumulating,
both sums over the restatement's taps; where the reference has no tap the device value is 0 (to 1e-12 of the largest reference
value: a source point within 1e-15 of a lattice plane may fall on either side of it)."""
import numpy as np
import pytest

import rigid_reference as rr

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
GUARD = 64
ERR_SIZE = -3                   # BDOF_ERR_SIZE (include/bdof.h)
NXV, NZV = 7, 10
NYS = [6, 64, 66, 130]
# theta: the values of the bilinear test (test_gpu_gradient_gathers.BILIN_ANGLES)
ANGLES = np.array([0.3, np.pi / 2, -1.1, np.pi, 0.0, -np.pi / 2, 2.5, 2 * np.pi, 4.0]).astype(np.float32).astype(np.float64)
TILTS = [0.5, -np.pi / 4, np.pi / 2, 0.0, 0.5, np.pi / 2, 0.0, -np.pi / 4, 0.5]
ROLLS = [0.0, 0.05, 0.0, 0.05, 0.05, 0.05, 0.0, 0.0, 0.05]
CENTERS = [2.6, 3.3, None, 2.4, 3.75, 1.5, 2.9, None, 4.2]


@pytest.fixture(scope='module')
def built():
    import __graft_entry__ as entry
    entry.build()


def bare_context():
    from beyond_dof_amd import _lib
    return _lib.Context(0)


class Guarded(object):
    """A device array between two sentinel-filled guards; download() checks the guards and returns the array."""

    def __init__(self, ctx, host):
        from beyond_dof_amd import _lib
        host = np.ascontiguousarray(host, dtype=np.float32)
        self.shape = host.shape
        g = np.full(GUARD, SENTINEL, dtype=np.float32)
        self.buf = _lib.DeviceBuffer.from_host(ctx, np.concatenate([g, host.reshape(-1), g]))
        self.ptr = self.buf.ptr + GUARD * 4

    def download(self):
        a = self.buf.download()
        assert np.all(a[:GUARD] == SENTINEL) and np.all(a[-GUARD:] == SENTINEL), 'a guard was overwritten'
        return a[GUARD:-GUARD].reshape(self.shape)


def sentinels(shape):
    return np.full(shape, SENTINEL, dtype=np.float32)


def assert_within(dev, ref, bound, what):
    err = np.abs(dev.astype(np.float64) - ref)
    tap = bound > 0
    worst = float((err[tap] / bound[tap]).max()) if tap.any() else 0.0
    print(what, 'largest |device - reference| / bound', worst, 'elements without a tap', int((~tap).sum()))
    assert worst <= 1.0, what
    assert np.all(err[~tap] <= 1e-12 * max(np.abs(ref).max(), 1.0)), what


class Device(object):
    def __init__(self, ny):
        from beyond_dof_amd import _lib
        self.ctx = bare_context()
        self.lib, self.h, self.ny = self.ctx.lib, self.ctx.handle, ny
        self.up = lambda a: _lib.DeviceBuffer.from_host(self.ctx, np.ascontiguousarray(a))

    def forward(self, dvol, dprm, B):
        out = Guarded(self.ctx, sentinels((B, NZV, NXV, self.ny, 2)))
        self.ctx.check(self.lib.bdof_rotate_rigid(self.h, dvol.ptr, NXV, NZV, self.ny, dprm.ptr, B, out.ptr))
        self.ctx.sync()
        return out.download()

    def adjoint(self, dgrot, dprm, B, start, row0, n_rows, acc, scale):
        g = Guarded(self.ctx, start)
        self.ctx.check(self.lib.bdof_rotate_rigid_adjoint(self.h, dgrot.ptr, NXV, NZV, self.ny, dprm.ptr, B, g.ptr, row0, n_rows, acc, scale))
        self.ctx.sync()
        return g.download()


# ---- exact cases ---------------------------------------------------------------------------------------------------------------------
def exact_geometries(ny):
    """[(12 numbers)]: the 24 signed permutations with integer t that keep part of the volume in view, shifted by a few voxels
    (the shift differs from one to the next), and one whose shift moves the volume wholly outside"""
    dims = np.array([NXV, NZV, ny])
    c = (dims - 1) // 2
    out = []
    for i, M in enumerate(rr.signed_permutations()):
        shift = np.array([(i % 3) - 1, ((i // 3) % 3) - 1, ((i // 2) % 5) - 2])
        out.append(np.concatenate([M, (c - M @ c + shift)[:, None]], axis=1).reshape(-1).astype(np.float64))
    outside = np.concatenate([np.eye(3), np.array([[NXV + 1.], [0.], [0.]])], axis=1).reshape(-1)
    return out, outside


@pytest.mark.parametrize('ny', NYS)
def test_exact_under_signed_permutations(built, ny):
    """forward and adjoint under every quarter turn and their products, plus shifts: bit for bit the restatement; a volume moved
    wholly outside gives zeros; slabs leave the rows outside them untouched; scale 1, 0.5, 3, accumulating from integers"""
    rng = np.random.default_rng(100 + ny)
    geos, outside = exact_geometries(ny)
    groups = [geos[0:1], geos[1:4], geos[4:9], geos[9:14], geos[14:19], geos[19:24], [geos[5], outside, geos[17]], [outside]]
    assert sorted(len(g) for g in groups) == [1, 1, 3, 3, 5, 5, 5, 5]
    dev = Device(ny)
    vol = rng.integers(-4, 5, size=(NXV, NZV, ny, 2)).astype(np.float32)
    grot = rng.integers(-4, 5, size=(5, NZV, NXV, ny, 2)).astype(np.float32)
    prior = rng.integers(-4, 5, size=(NXV, NZV, ny, 2)).astype(np.float32)
    dvol, dgrot = dev.up(vol), dev.up(grot)
    n = NXV * NZV
    cuts = [0, 3, 37, n]
    seen_nonzero = False
    for prms in groups:
        B = len(prms)
        for p in prms:
            assert set(np.unique(rr.taps(p, (NXV, NZV, ny), 'f32')[1])) <= {0.0, 1.0}
        dprm = dev.up(np.stack(prms))
        want = np.stack([rr.rotate_rigid(vol, p) for p in prms])
        got = dev.forward(dvol, dprm, B)
        assert np.array_equal(got, want), B
        rest = sum(rr.rotate_rigid_adjoint(grot[b], p) for b, p in enumerate(prms))
        whole = dev.adjoint(dgrot, dprm, B, sentinels((NXV, NZV, ny, 2)), 0, n, 0, 1.0)
        assert np.array_equal(whole, rest), B
        if all(p is outside for p in prms):
            assert not np.any(got) and not np.any(whole)
        seen_nonzero = seen_nonzero or bool(np.any(whole))
        cur = sentinels((NXV, NZV, ny, 2))
        for a, b in zip(cuts[:-1], cuts[1:]):
            cur = dev.adjoint(dgrot, dprm, B, cur, a, b - a, 0, 1.0)
            flat = cur.reshape(n, ny, 2)
            assert np.all(flat[b:] == SENTINEL) and np.array_equal(flat[:b], rest.reshape(n, ny, 2)[:b]), (a, b)
        for (a, cnt), acc, scale in (((0, n), 1, 0.5), ((5, 33), 1, 3.0), ((0, n), 0, 3.0), ((1, n - 2), 0, 0.5)):
            got = dev.adjoint(dgrot, dprm, B, prior, a, cnt, acc, scale).reshape(n, ny, 2)
            exp = prior.astype(np.float64).reshape(n, ny, 2).copy()
            exp[a:a + cnt] = scale * rest.reshape(n, ny, 2)[a:a + cnt] + (exp[a:a + cnt] if acc else 0.0)
            assert np.array_equal(got, exp), (a, cnt, acc, scale)
    assert seen_nonzero


# ---- general cases -------------------------------------------------------------------------------------------------------------------
def general_geometry(ny):
    from beyond_dof_amd import util
    return np.stack([util.rigid_geometry(ANGLES[i], (ny, NXV, NZV), TILTS[i], ROLLS[i], CENTERS[i])[0] for i in range(9)])


@pytest.mark.parametrize('ny', NYS)
def test_general_geometries_within_the_derived_bound(built, ny):
    """tilted, rolled, off-centre axes at the bilinear test's angles, B = 1, 3, 5 (each B starts at another geometry): forward and
    adjoint within the per-element bound of the float64 restatement, whole / in slabs (the bits of the whole call) / accumulating
    with scale 0.5 / twice (identical bits); and <R v, g> = <v, R^T g> on the device's outputs to the sum of the bounds"""
    rng = np.random.default_rng(200 + ny)
    prm_all = general_geometry(ny)
    vol = (1.0 + rng.normal(size=(NXV, NZV, ny, 2))).astype(np.float32)
    grot = (1.0 + rng.normal(size=(5, NZV, NXV, ny, 2))).astype(np.float32)
    prior = rng.normal(size=(NXV, NZV, ny, 2)).astype(np.float32)
    dev = Device(ny)
    dvol, dgrot = dev.up(vol), dev.up(grot)
    n = NXV * NZV
    cuts = [0, 3, 37, n]
    for B, start in ((1, 2), (3, 0), (5, 4), (3, 6)):
        prms = prm_all[start:start + B]
        dprm = dev.up(prms)
        f = [rr.forward_terms(vol, p) for p in prms]
        fref, fbound = np.stack([t[0] for t in f]), np.stack([rr.element_bound(*t[1:]) for t in f])
        rot = dev.forward(dvol, dprm, B)
        assert_within(rot, fref, fbound, 'forward NY {} B {}'.format(ny, B))
        t = [rr.adjoint_terms(grot[b], p) for b, p in enumerate(prms)]
        ref = sum(x[0] for x in t)
        bound = rr.element_bound(sum(x[1] for x in t), sum(x[2] for x in t), sum(x[3] for x in t))
        whole = dev.adjoint(dgrot, dprm, B, sentinels((NXV, NZV, ny, 2)), 0, n, 0, 1.0)
        assert_within(whole, ref, bound, 'adjoint NY {} B {}'.format(ny, B))
        assert np.array_equal(dev.adjoint(dgrot, dprm, B, sentinels((NXV, NZV, ny, 2)), 0, n, 0, 1.0), whole)       # run to run
        cur = sentinels((NXV, NZV, ny, 2))
        for a, b in zip(cuts[:-1], cuts[1:]):
            cur = dev.adjoint(dgrot, dprm, B, cur, a, b - a, 0, 1.0)
            flat = cur.reshape(n, ny, 2)
            assert np.all(flat[b:] == SENTINEL) and np.array_equal(flat[:b], whole.reshape(n, ny, 2)[:b]), (a, b)
        got = dev.adjoint(dgrot, dprm, B, prior, 0, n, 1, 0.5)
        assert_within(got, prior.astype(np.float64) + 0.5 * ref, 0.5 * bound + 2.0 ** -24 * np.abs(prior), 'adjoint accumulate NY {} B {}'.format(ny, B))
        got = dev.adjoint(dgrot, dprm, B, prior, 5, 33, 1, 0.5).reshape(n, ny, 2)
        want = prior.astype(np.float64).reshape(n, ny, 2).copy()
        want[5:38] += 0.5 * ref.reshape(n, ny, 2)[5:38]
        bnd = (0.5 * bound + 2.0 ** -24 * np.abs(prior)).reshape(n, ny, 2)
        assert np.array_equal(got[:5], want[:5]) and np.array_equal(got[38:], want[38:])
        assert_within(got[5:38], want[5:38], bnd[5:38], 'adjoint slab accumulate NY {} B {}'.format(ny, B))
        # adjointness from the two device outputs, in float64
        lhs = float(np.sum(rot.astype(np.float64) * grot[:B].astype(np.float64)))
        rhs = float(np.sum(vol.astype(np.float64) * whole.astype(np.float64)))
        slack = float(np.sum(fbound * np.abs(grot[:B])) + np.sum(bound * np.abs(vol)))
        print('pairing NY {} B {}: {} vs {}, |difference| / bound {}'.format(ny, B, lhs, rhs, abs(lhs - rhs) / slack))
        assert abs(lhs - rhs) <= slack


@pytest.mark.parametrize('ny', [6, 130])
def test_zero_tilt_and_roll_against_the_bilinear_kernel(built, ny):
    """bdof_rotate_rigid at zero tilt and roll against bdof_rotate_bilinear on the same volume.  The y factor is then exactly 0 or
    1, a weight has two inexact factors and n <= 4; the two kernels' weights differ by <= 4 * 2^-24 together (each factor within
    2^-24, one product rounding each) and each adds n <= 4 fused products, 2 n <= n + 4: the four-tap form of the bound."""
    from beyond_dof_amd import util
    rng = np.random.default_rng(300 + ny)
    vol = (1.0 + rng.normal(size=(NXV, NZV, ny, 2))).astype(np.float32)
    dev = Device(ny)
    dvol = dev.up(vol)
    prm = util.rigid_geometry(ANGLES, (ny, NXV, NZV))
    c, sn = np.cos(ANGLES), np.sin(ANGLES)
    H, W = NXV, NZV
    bil = np.stack([c, sn, ((W - 1) - (c * (W - 1) - sn * (H - 1))) / 2.0, ((H - 1) - (sn * (W - 1) + c * (H - 1))) / 2.0], axis=1)
    rigid = dev.forward(dvol, dev.up(prm), 9)
    out = Guarded(dev.ctx, sentinels((9, NZV, NXV, ny, 2)))
    dev.ctx.check(dev.lib.bdof_rotate_bilinear(dev.h, dvol.ptr, NXV, NZV, ny, dev.up(bil).ptr, 9, out.ptr))
    dev.ctx.sync()
    f = [rr.forward_terms(vol, p) for p in prm]
    assert max(t[3].max() for t in f) <= 4
    bound = np.stack([rr.element_bound(*t[1:], weight_terms=4) for t in f])
    assert_within(rigid, out.download().astype(np.float64), bound, 'rigid against bilinear NY {}'.format(ny))


# ---- the fused binding -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def engine(built):
    from beyond_dof_amd.engine import MultisliceEngine
    eng = MultisliceEngine(64, 64, 8, 3, with_grad=True)
    eng.set_physics(5000., 1e-7, 1e-4)
    eng.set_probe(np.ones((64, 64)), np.zeros((64, 64)))
    return eng


def test_fused_binding_gives_the_waves_of_rotate_then_bind(engine):
    """bdof_set_object_rigid against bdof_rotate_rigid followed by bdof_set_object: the same waves, bit for bit"""
    from beyond_dof_amd import _lib, util
    eng = engine
    NX, S, NY, B = 64, 8, 64, 3
    rng = np.random.default_rng(9)
    vol = np.zeros((NX, S, NY, 2), np.float32)
    vol[..., 0] = rng.uniform(0, 2e-5, size=(NX, S, NY))
    vol[..., 1] = 0.1 * vol[..., 0]
    prm = util.rigid_geometry([0.3, -1.1, 2.5], (NY, NX, S), 0.5, 0.03, 30.4)
    dvol, dprm = _lib.DeviceBuffer.from_host(eng.ctx, vol), _lib.DeviceBuffer.from_host(eng.ctx, prm)
    eng.ctx.check(eng.lib.bdof_set_object_rigid(eng.h, dvol.ptr, NX, S, NY, dprm.ptr, B, 0))
    fused = eng.forward(B)
    rows = _lib.DeviceBuffer(eng.ctx, B * S * NX * NY * 8, np.float32, (B, S, NX, NY, 2))
    eng.ctx.check(eng.lib.bdof_rotate_rigid(eng.h, dvol.ptr, NX, S, NY, dprm.ptr, B, rows.ptr))
    eng.set_volume(rows, B * S * NX, NY, None, 0, 0)
    two_pass = eng.forward(B)
    assert np.any(np.abs(fused - 1) > 1e-4) and np.array_equal(fused, two_pass)
    # the rows themselves, against the restatement
    got = rows.download()
    for b in range(B):
        ref, sg, swg, n = rr.forward_terms(vol, prm[b])
        assert_within(got[b], ref, rr.element_bound(sg, swg, n), 'rows of angle {}'.format(b))


def test_size_refusals(engine):
    """an odd NY, and a volume or a batch whose voxel indices pass 2^31, return BDOF_ERR_SIZE from all three entry points before
    anything is launched; the even neighbour of the odd NY is taken"""
    from beyond_dof_amd import _lib
    eng = engine
    lib, h = eng.lib, eng.h
    buf, out = _lib.DeviceBuffer.zeros(eng.ctx, (3, 4, 5, 6, 2), np.float32), _lib.DeviceBuffer.zeros(eng.ctx, (3, 4, 5, 6, 2), np.float32)
    prm = _lib.DeviceBuffer.from_host(eng.ctx, np.tile(np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).reshape(-1), (3, 1)))
    for shape in ((5, 4, 5, 1), (5, 4, 1, 1), (2048, 1024, 1024, 1), (1 << 10, 1 << 10, 2, 4096)):
        NXv, NZv, NYv, B = shape
        assert lib.bdof_rotate_rigid(h, buf.ptr, NXv, NZv, NYv, prm.ptr, B, out.ptr) == ERR_SIZE, shape
        assert lib.bdof_rotate_rigid_adjoint(h, buf.ptr, NXv, NZv, NYv, prm.ptr, B, out.ptr, 0, 1, 0, 1.0) == ERR_SIZE, shape
        assert lib.bdof_set_object_rigid(h, buf.ptr, NXv, NZv, NYv, prm.ptr, B, 0) == ERR_SIZE, shape
    assert lib.bdof_rotate_rigid(h, buf.ptr, 5, 4, 6, prm.ptr, 1, out.ptr) == 0
    assert lib.bdof_rotate_rigid_adjoint(h, buf.ptr, 4, 5, 6, prm.ptr, 1, out.ptr, 0, 20, 0, 1.0) == 0
    eng.ctx.sync()
