"""bdof_window_stack, bdof_window_stack_adjoint and bdof_window_position_grad (csrc/bdof_windows.h) through their own entry points
against the float64 restatement of tests/positions_reference.py — the pattern of tests/test_gpu_geometry_ops.py: the kernels are
fed directly, every output lies between sentinel-filled guards, and every element is compared.

Shapes (volNX, S, volNY; NX, NY): (12, 3, 14; 8, 6); (10, 2, 140; 6, 130), where the lanes wrap past 64 and 128; (5, 3, 4; 4, 2),
fewer rows than one pass of workgroups.  B in 1, 5.  Tables: the identity, and util.rotation_lookup's at an oblique angle.
Origins: generic fractions; exactly integer (the stack is the integer cut bit for bit; right-hand derivative); negative with a
fraction; half outside; wholly outside (stack, adjoint contribution and derivative exactly 0).

The tolerances are derived per element in positions_reference (element_bound, table_adjoint_terms, entry_bound), not measured."""
import numpy as np
import pytest

import positions_reference as pr

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
GUARD = 16
ERR_ARG, ERR_STATE, ERR_SIZE = -1, -2, -3              # include/bdof.h
SHAPES = [(12, 3, 14, 8, 6), (10, 2, 140, 6, 130), (5, 3, 4, 4, 2)]
NAMES = ('generic', 'integer', 'negative', 'half outside', 'outside')
N_THETA, ANGLE = 8, 2                                  # the oblique angle: 2 * (2 pi / 7)


@pytest.fixture(scope='module')
def built():
    import __graft_entry__ as entry
    entry.build()


def origins(shape):
    VX, S, VY, NX, NY = shape
    return {'generic': (1.3, 2.7), 'integer': (1.0, 2.0), 'negative': (-1.6, -0.35), 'half outside': (VX - NX / 2. + 0.25, VY - NY / 2. - 0.5),
            'outside': (VX + 3.5, 1.0)}


def tables(shape, kind):
    """(tab [n][S][VX], off, order, angle) as util.device_rotation_tables lays them out"""
    from beyond_dof_amd import util
    VX, S, VY, NX, NY = shape
    if kind == 'identity':
        n = S * VX
        return (np.arange(n, dtype=np.int32).reshape(1, S, VX), np.arange(n + 1, dtype=np.int32).reshape(1, -1),
                np.arange(n, dtype=np.int32).reshape(1, -1), 0)
    return util.device_rotation_tables(util.rotation_lookup((VY, VX, S), N_THETA), VX, S) + (ANGLE,)


class Device(object):
    def __init__(self, shape, bmax=5, flags=None):
        from beyond_dof_amd import _lib
        self.ctx = _lib.Context(0)
        self.lib, self.h, self.shape = self.ctx.lib, self.ctx.handle, shape
        VX, S, VY, NX, NY = shape
        self.ctx.check(self.lib.bdof_configure(self.h, NY, NX, S, bmax, _lib.CFG_GENERIC if flags is None else flags))
        self.up = lambda a: _lib.DeviceBuffer.from_host(self.ctx, np.ascontiguousarray(a))
        self.keep = []

    def tables(self, kind):
        VX, S, VY, NX, NY = self.shape
        tab, off, order, angle = tables(self.shape, kind)
        self.tab, self.angle = tab[angle], angle
        bufs = [self.up(tab), self.up(off), self.up(order)]
        self.keep.append(bufs)
        self.tab_ptr = bufs[0].ptr + angle * S * VX * 4
        self.ctx.check(self.lib.bdof_set_rotation_adjoint(self.h, bufs[1].ptr, bufs[2].ptr, VX * S))

    def guarded(self, host, dtype):
        guard = np.full(GUARD, SENTINEL, dtype=dtype)
        return self.up(np.concatenate([guard, np.asarray(host, dtype=dtype).reshape(-1), guard])), GUARD * np.dtype(dtype).itemsize

    def result(self, buf, shape):
        self.ctx.sync()
        a = buf.download()
        assert np.all(a[:GUARD] == SENTINEL) and np.all(a[-GUARD:] == SENTINEL), 'a guard was overwritten'
        return a[GUARD:-GUARD].reshape(shape)

    def stack(self, dvol, dorg, B):
        VX, S, VY, NX, NY = self.shape
        buf, at = self.guarded(np.full((B, S, NX, NY, 2), SENTINEL), np.float32)
        self.ctx.check(self.lib.bdof_window_stack(self.h, dvol.ptr, VX, VY, self.tab_ptr, dorg.ptr, B, buf.ptr + at))
        return self.result(buf, (B, S, NX, NY, 2))

    def adjoint(self, grot_ptr, dorg, B, start=None, accumulate=0, scale=1.0):
        VX, S, VY, NX, NY = self.shape
        buf, at = self.guarded(np.full((VX * S, VY, 2), SENTINEL) if start is None else start, np.float32)
        self.ctx.check(self.lib.bdof_window_stack_adjoint(self.h, grot_ptr, self.angle, dorg.ptr, B, buf.ptr + at, accumulate, scale))
        return self.result(buf, (VX * S, VY, 2))

    def position_grad(self, dvol, grot_ptr, dorg, B, start=None, accumulate=0):
        VX, S, VY, NX, NY = self.shape
        buf, at = self.guarded(np.full((B, 2), SENTINEL) if start is None else start, np.float64)
        self.ctx.check(self.lib.bdof_window_position_grad(self.h, dvol.ptr, VX, VY, self.tab_ptr, grot_ptr, dorg.ptr, B, buf.ptr + at, accumulate))
        return self.result(buf, (B, 2))


def within(dev, ref, bound, what):
    err = np.abs(dev.astype(np.float64) - ref)
    tap = bound > 0
    worst = float((err[tap] / bound[tap]).max()) if tap.any() else 0.0
    print(what, 'largest |device - reference| / bound', worst, 'elements without a term', int((~tap).sum()))
    assert worst <= 1.0, what
    assert np.all(dev[~tap] == 0.0), what


@pytest.mark.parametrize('kind', ['identity', 'oblique'])
@pytest.mark.parametrize('shape', SHAPES, ids=['x'.join(str(n) for n in s) for s in SHAPES])
def test_window_kernels_within_the_derived_bounds(built, shape, kind):
    VX, S, VY, NX, NY = shape
    rng = np.random.default_rng(900 + VY + (kind == 'oblique'))
    dev = Device(shape)
    dev.tables(kind)
    org = origins(shape)
    vol = (1.0 + rng.normal(size=(VX * S, VY, 2))).astype(np.float32)
    g = (1.0 + rng.normal(size=(5, S, NX, NY, 2))).astype(np.float32)
    R = vol[dev.tab]                                         # [S][VX][VY][C]
    dvol, dg = dev.up(vol), dev.up(g)
    per_b = S * NX * NY * 8
    all5 = np.array([org[n] for n in NAMES])
    d5 = dev.up(all5)

    # ---- forward
    ref, sg, swg, n = pr.forward_terms(R, all5, NX, NY)
    batch = dev.stack(dvol, d5, 5)
    within(batch, ref, pr.element_bound(sg, swg, n), '{} {} stack B 5'.format(shape, kind))
    i0 = np.floor(all5[1]).astype(int)
    assert np.array_equal(batch[1], R[:, i0[0]:i0[0] + NX, i0[1]:i0[1] + NY]), 'an integer origin is the integer cut, bit for bit'
    assert not np.any(batch[4]) and np.any(batch[3]) and np.any(batch[2])
    assert np.array_equal(dev.stack(dvol, d5, 5), batch)
    for b, name in enumerate(NAMES):
        assert np.array_equal(dev.stack(dvol, dev.up(all5[b:b + 1]), 1)[0], batch[b]), name

    # ---- adjoint
    terms = pr.table_adjoint_terms(pr.adjoint_terms(g, all5, VX, VY), dev.tab, VX * S)
    bound = pr.element_bound(*terms[1:])
    out = dev.adjoint(dg.ptr, d5, 5)
    within(out, terms[0], bound, '{} {} adjoint B 5'.format(shape, kind))
    assert np.array_equal(dev.adjoint(dg.ptr, d5, 5), out)
    one = pr.table_adjoint_terms(pr.adjoint_terms(g[:1], all5[:1], VX, VY), dev.tab, VX * S)
    within(dev.adjoint(dg.ptr, dev.up(all5[:1]), 1), one[0], pr.element_bound(*one[1:]), '{} {} adjoint B 1'.format(shape, kind))
    assert not np.any(dev.adjoint(dg.ptr + 4 * per_b, dev.up(all5[4:]), 1)), 'a window wholly outside adds exactly nothing'
    # the window outside adds nothing to a batch either: the first four alone give the same bits
    assert np.array_equal(dev.adjoint(dg.ptr, dev.up(all5[:4]), 4), out)
    # gvol = scale * result (+ gvol): one more rounding each, on top of the scaled bound
    prior = rng.normal(size=(VX * S, VY, 2)).astype(np.float32)
    for accumulate in (0, 1):
        got = dev.adjoint(dg.ptr, d5, 5, start=prior, accumulate=accumulate, scale=0.5)
        want = 0.5 * terms[0] + accumulate * prior
        err = np.abs(got - want)
        assert np.all(err <= 0.5 * bound + 2.0 ** -24 * (np.abs(prior) + np.abs(want))), accumulate

    # ---- derivative
    d, SG, SWG, _ = pr.position_terms(R, g, all5)
    pb = pr.entry_bound(SG, SWG)
    got = dev.position_grad(dvol, dg.ptr, d5, 5)
    within(got, d, pb, '{} {} position gradient B 5'.format(shape, kind))
    assert not np.any(got[4]) and np.all(got[:3] != 0)
    assert np.array_equal(dev.position_grad(dvol, dg.ptr, d5, 5), got)
    for b, name in enumerate(NAMES):
        alone = dev.position_grad(dvol, dg.ptr + b * per_b, dev.up(all5[b:b + 1]), 1)
        assert np.array_equal(alone[0], got[b]), name
    before = rng.normal(size=(5, 2))
    assert np.array_equal(dev.position_grad(dvol, dg.ptr, d5, 5, start=before, accumulate=1), before + got)
    assert np.array_equal(dev.position_grad(dvol, dg.ptr, d5, 5, start=before, accumulate=0), got)


def test_more_windows_on_a_column_than_the_list_holds(built):
    """B = 1025 windows of 4 x 2 at one origin: BDOF_ERR_SIZE from the adjoint before anything is launched (the output keeps its
    sentinels); with one of them moved off the frame the call goes through"""
    shape = (5, 3, 4, 4, 2)
    VX, S, VY, NX, NY = shape
    B = 1025
    dev = Device(shape, bmax=B)
    dev.tables('identity')
    rng = np.random.default_rng(1)
    vol = dev.up(rng.normal(size=(VX * S, VY, 2)).astype(np.float32))
    g = rng.normal(size=(B, S, NX, NY, 2)).astype(np.float32)
    dg = dev.up(g)
    org = np.tile([[0.5, 0.25]], (B, 1))
    dorg = dev.up(org)
    assert dev.stack(vol, dorg, B).shape[0] == B
    buf, at = dev.guarded(np.full((VX * S, VY, 2), SENTINEL), np.float32)
    assert dev.lib.bdof_window_stack_adjoint(dev.h, dg.ptr, 0, dorg.ptr, B, buf.ptr + at, 0, 1.0) == ERR_SIZE
    assert b'BDOF_WIN_MAXLIST' in dev.lib.bdof_last_error(dev.h)
    assert np.all(dev.result(buf, (VX * S, VY, 2)) == SENTINEL)
    org[7] = (VX + 2.0, 0.0)
    out = dev.adjoint(dg.ptr, dev.up(org), B)
    terms = pr.table_adjoint_terms(pr.adjoint_terms(g, org, VX, VY), dev.tab, VX * S)
    within(out, terms[0], pr.element_bound(*terms[1:]), '1024 windows on one column')


def test_refusals(built):
    """state: the adjoint without bdof_set_rotation_adjoint, then without a bdof_window_stack before it; grot = NULL on a ctx that
    holds no gradient workspace.  size: an odd NY of the volume or of the windows, the 2^31 limit.  argument: B outside [1, Bmax]"""
    shape = (5, 3, 4, 4, 2)
    VX, S, VY, NX, NY = shape
    dev = Device(shape)
    vol = dev.up(np.zeros((VX * S, VY + 2, 2), np.float32))
    g = dev.up(np.zeros((5, S, NX, NY, 2), np.float32))
    org = dev.up(np.zeros((5, 2)))
    out = dev.up(np.zeros((VX * S, VY, 2), np.float32))
    dpos = dev.up(np.zeros((5, 2)))
    tab = dev.up(np.arange(S * VX, dtype=np.int32))
    adjoint = lambda grot, B=5: dev.lib.bdof_window_stack_adjoint(dev.h, grot, 0, org.ptr, B, out.ptr, 0, 1.0)
    stack = lambda vx, vy, B=5: dev.lib.bdof_window_stack(dev.h, vol.ptr, vx, vy, tab.ptr, org.ptr, B, g.ptr)
    grad = lambda grot, vx, vy, B=5: dev.lib.bdof_window_position_grad(dev.h, vol.ptr, vx, vy, tab.ptr, grot, org.ptr, B, dpos.ptr, 0)
    assert adjoint(g.ptr) == ERR_STATE and b'bdof_set_rotation_adjoint' in dev.lib.bdof_last_error(dev.h)
    dev.tables('identity')
    assert adjoint(g.ptr) == ERR_STATE and b'bdof_window_stack' in dev.lib.bdof_last_error(dev.h)
    for call in (lambda vx, vy: stack(vx, vy), lambda vx, vy: grad(g.ptr, vx, vy)):
        assert call(VX, 5) == ERR_SIZE and call(1 << 20, 1 << 12) == ERR_SIZE
        assert call(0, VY) == ERR_ARG
    assert stack(VX, VY, 6) == ERR_ARG and stack(VX, VY, 0) == ERR_ARG and grad(g.ptr, VX, VY, 6) == ERR_ARG
    assert stack(VX, VY) == 0
    assert adjoint(None) == ERR_STATE and grad(None, VX, VY) == ERR_STATE              # (configured without a gradient workspace)
    assert adjoint(g.ptr, 6) == ERR_ARG
    assert adjoint(g.ptr) == 0 and grad(g.ptr, VX, VY) == 0
    dev.ctx.sync()
    assert not np.any(out.download()) and not np.any(dpos.download())                   # (a zero volume, zero gradients)
    odd = Device((5, 3, 4, 4, 3))
    assert odd.lib.bdof_window_stack(odd.h, vol.ptr, VX, VY, tab.ptr, org.ptr, 1, g.ptr) == ERR_SIZE
