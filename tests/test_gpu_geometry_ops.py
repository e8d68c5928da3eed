"""bdof_rotate_rigid_param_grad (k_rot_rigid_param_grad + k_rot_rigid_param_sum) through its own entry point against the float64
restatement of tests/geometry_reference.py — the pattern of tests/test_gpu_rigid_ops.py: the kernels are fed directly, the output
lies between sentinel-filled guards, and every one of the 12 entries of every batch element is compared.

Shapes (NXv, NZv, NYv): (12, 10, 14); (8, 6, 130), where the lanes wrap past 64 and 128; (5, 7, 2), fewer rows than one full
pass of workgroups and one voxel pair per row.  B in 1, 3.  Geometries: a random rigid map; zero tilt and roll (the y fraction is
exactly 0 at every voxel: the right-derivative convention); the identity (every fraction 0); a map whose t moves half of the
outputs' source points outside the volume; a map wholly outside (the result is exactly 0).

The tolerance is derived per entry in geometry_reference (entry_bound), not measured:
    |device - reference| <= 2^-24 (4 SG + SWG),   SG = sum |g| |V| |o~_j|,  SWG = sum (n + 4) |w| |g| |V| |o~_j|
over the restatement's live corners."""
import numpy as np
import pytest

import geometry_reference as gr
import rigid_reference as rr

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
GUARD = 16
ERR_STATE, ERR_SIZE = -2, -3                   # include/bdof.h
SHAPES = [(12, 10, 14), (8, 6, 130), (5, 7, 2)]


@pytest.fixture(scope='module')
def built():
    import __graft_entry__ as entry
    entry.build()


def geometries(dims, rng):
    from beyond_dof_amd import util
    NX, NZ, NY = dims
    c = (np.array(dims) - 1) / 2.
    rows = lambda M, t: np.concatenate([M, np.reshape(t, (3, 1))], axis=1).reshape(-1)
    M = rr.random_rigid(rng)
    M2 = rr.random_rigid(rng)
    out = {
        'random': rows(M, c - M @ c + rng.uniform(-0.5, 0.5, size=3)),
        'zero tilt': util.rigid_geometry(0.3, (NY, NX, NZ), 0., 0., c[0] + 0.3)[0],
        'identity': rows(np.eye(3), np.zeros(3)),
        'half outside': rows(M2, c - M2 @ c + np.array([NX / 2., 0.2, 0.3])),
        'outside': rows(np.eye(3), [NX + 1., 0., 0.]),
    }
    assert not np.any(gr.cell(out['zero tilt'], dims)[1][2]) and all(not np.any(f) for f in gr.cell(out['identity'], dims)[1])
    return out


class Device(object):
    def __init__(self, dims):
        from beyond_dof_amd import _lib
        self.ctx = _lib.Context(0)
        self.lib, self.h, self.dims = self.ctx.lib, self.ctx.handle, dims
        self.up = lambda a: _lib.DeviceBuffer.from_host(self.ctx, np.ascontiguousarray(a))

    def param_grad(self, dvol, grot_ptr, dprm, B, start=None, accumulate=0):
        """the (B, 3, 4) result between float64 guards; start: what the output holds before the call (None: sentinels)"""
        host = np.full((B, 3, 4), SENTINEL) if start is None else np.asarray(start, dtype=np.float64)
        guard = np.full(GUARD, SENTINEL)
        buf = self.up(np.concatenate([guard, host.reshape(-1), guard]))
        NX, NZ, NY = self.dims
        self.ctx.check(self.lib.bdof_rotate_rigid_param_grad(self.h, dvol.ptr, grot_ptr, NX, NZ, NY, dprm.ptr, B, buf.ptr + GUARD * 8, accumulate))
        self.ctx.sync()
        a = buf.download()
        assert np.all(a[:GUARD] == SENTINEL) and np.all(a[-GUARD:] == SENTINEL), 'a guard was overwritten'
        return a[GUARD:-GUARD].reshape(B, 3, 4)


def held(dev, vol, g, prm, what):
    d, SG, SWG, _ = gr.param_terms(vol, g, prm)
    bound = gr.entry_bound(SG, SWG)
    err = np.abs(dev - d)
    tap = bound > 0
    worst = float((err[tap] / bound[tap]).max()) if tap.any() else 0.0
    print(what, 'largest |device - reference| / bound', worst, 'entries without a term', int((~tap).sum()))
    assert worst <= 1.0, what
    assert np.all(dev[~tap] == 0.0), what


@pytest.mark.parametrize('dims', SHAPES, ids=['x'.join(str(n) for n in s) for s in SHAPES])
def test_param_grad_within_the_derived_bound(built, dims):
    """B = 1 and 3 over the five geometries: every entry within the per-entry bound; element b has the same bits alone and in a batch;
    a second call gives the same bits; accumulate = 1 adds; the map wholly outside gives exactly 0"""
    NX, NZ, NY = dims
    rng = np.random.default_rng(400 + NY)
    geo = geometries(dims, rng)
    vol = (1.0 + rng.normal(size=(NX, NZ, NY, 2))).astype(np.float32)
    grot = (1.0 + rng.normal(size=(3, NZ, NX, NY, 2))).astype(np.float32)
    dev = Device(dims)
    dvol, dgrot = dev.up(vol), dev.up(grot)
    per_b = NZ * NX * NY * 8
    alone = {}
    for name, prm in geo.items():
        for b in range(3):
            alone[name, b] = dev.param_grad(dvol, dgrot.ptr + b * per_b, dev.up(prm[None]), 1)[0]
        held(alone[name, 0], vol, grot[0], prm, '{} {} B 1'.format(dims, name))
    assert not np.any(alone['outside', 0]) and np.any(alone['half outside', 0]) and np.any(alone['identity', 0])
    for names in (('random', 'zero tilt', 'identity'), ('half outside', 'outside', 'random')):
        dprm = dev.up(np.stack([geo[n] for n in names]))
        batch = dev.param_grad(dvol, dgrot.ptr, dprm, 3)
        for b, n in enumerate(names):
            held(batch[b], vol, grot[b], geo[n], '{} {} B 3 element {}'.format(dims, n, b))
            assert np.array_equal(batch[b], alone[n, b]), (n, b)
        assert np.array_equal(dev.param_grad(dvol, dgrot.ptr, dprm, 3), batch)
        prior = rng.normal(size=(3, 3, 4))
        assert np.array_equal(dev.param_grad(dvol, dgrot.ptr, dprm, 3, start=prior, accumulate=1), prior + batch)
        assert np.array_equal(dev.param_grad(dvol, dgrot.ptr, dprm, 3, start=prior, accumulate=0), batch)


def test_refusals(built):
    """the shape rule of bdof_rotate_rigid_adjoint: an odd NY and the 2^31 limits are BDOF_ERR_SIZE before anything is launched, the
    even neighbour is taken; grot = NULL on a ctx that holds no rotated-frame gradient is BDOF_ERR_STATE"""
    dev = Device((5, 4, 6))
    buf = dev.up(np.zeros((3, 4, 5, 6, 2), np.float32))
    prm = dev.up(np.tile(np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).reshape(-1), (3, 1)))
    out = dev.up(np.zeros((3, 12)))
    call = lambda grot, NXv, NZv, NYv, B: dev.lib.bdof_rotate_rigid_param_grad(dev.h, buf.ptr, grot, NXv, NZv, NYv, prm.ptr, B, out.ptr, 0)
    for shape in ((5, 4, 5, 1), (5, 4, 1, 1), (2048, 1024, 1024, 1), (1 << 10, 1 << 10, 2, 4096)):
        assert call(buf.ptr, *shape) == ERR_SIZE, shape
    assert call(None, 5, 4, 6, 1) == ERR_STATE
    assert call(buf.ptr, 5, 4, 6, 3) == 0
    dev.ctx.sync()
    assert np.array_equal(out.download(), np.zeros((3, 12)))           # (a zero volume)
