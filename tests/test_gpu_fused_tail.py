"""The one-pass tail of a step on one rank (bdof_rotation_adjoint_adam: k_rot_adjoint<true>, k_rot_adjoint_heavy<true>, k_sum_chunks,
k_sum_mean) against the route it replaces: bdof_rotation_adjoint_rows, bdof_adam_step and the table pass of the next sweep.

The gradient row the fused kernels hold in registers has the bits the unfused ones store, and Adam and the modulation factors are
the same device functions, so the new volume, the moments, the gradient (re-made on request) and the whole table are compared
bit for bit.  The one value that may differ is the table's mean, summed in another fixed order; it is held to the project's bound
for a mean, (D + 2) 2^-53 mean|entry| against fsum / n, with D counted in the kernels:
  a lane / thread adds its pairs' two entries each in ascending order: 2 ceil(nv / 64) in the wave kernel, 2 ceil(nv / 256) in the
  heavy one (nv = NY / 2 float4 columns); 6 in the wave's shuffle tree (+ 3 over the four waves of a heavy row's workgroup);
  k_sum_chunks over chunks of 1024 row sums: at most 4 per thread, 8 in its tree; k_sum_mean over the ceil(n_dest / 1024) chunk sums:
  ceil(chunks / 256) per thread, 8 in its tree.
"""
import ctypes
import math

import numpy as np
import pytest

from oracle import bdof_oracle as orc

import test_gpu_gradient_gathers as gg

pytestmark = pytest.mark.gpu

E, PS = 5000., 1e-7
REG = dict(alpha_d=1.5e-8, alpha_b=1.5e-9, gamma=1e-11)
LR = 1e-7
N, N_THETA = 64, 48


def _D_fused(ny, n_dest):
    nv = ny // 2
    chunks = -(-n_dest // 1024)
    return max(2 * -(-nv // 64) + 6, 2 * -(-nv // 256) + 6 + 3) + min(4, -(-n_dest // 256)) + 8 + -(-chunks // 256) + 8


def _check_mean(tag, table, mean, D):
    n = table.size
    ref = complex(math.fsum(table.real.astype(np.float64)), math.fsum(table.imag.astype(np.float64))) / n
    tol = (D + 2) * 2. ** -53 * float(np.abs(table.astype(np.complex128)).mean())
    print('mean of the table,', tag, 'n', n, 'D', D, ': |device - fsum / n|', abs(mean - ref), 'bound', tol, 'mean', mean)
    assert abs(mean - ref) <= tol, (tag, mean, ref, tol)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope='module')
def case():
    import __graft_entry__ as entry
    entry.build()
    from beyond_dof_amd import util
    rng = np.random.default_rng(11)
    od = rng.uniform(0, 2e-6, size=(N, N, N))
    od[rng.uniform(size=od.shape) < 0.05] = 0.0                     # sign(0) = 0 in the L1 and TV terms
    ob = 0.1 * od
    coords = orc.rotation_lookup([N, N, N], N_THETA)
    _, off, _ = util.device_rotation_tables(coords, N, N)
    per_row = (off[:, 1:] - off[:, :-1]).sum(axis=0)
    assert per_row.max() > 256 and per_row.min() <= 256               # both the heavy and the wave epilogue run
    prj = 1 + 0.05 * rng.normal(size=(N_THETA, N, N))
    mask = (rng.uniform(size=(N, N, N)) > 0.2).astype(np.float32)
    return dict(od=od, ob=ob, coords=coords, prj=prj, mask=mask)


def _solver(case, mb):
    from beyond_dof_amd.solver import FullfieldSolver
    s = FullfieldSolver(N, N, N, N_THETA, mb, E, PS, free_prop_cm=None, coord_ls=case['coords'])
    s.set_volume(case['od'], case['ob'])
    s.set_mask(case['mask'])
    s.set_measurements(case['prj'])
    return s


def _state(s):
    s.ctx.sync()
    return s.get_volume(), s.m.download(), s.v.download()


@pytest.mark.parametrize('use_mask', [True, False], ids=['mask', 'no_mask'])
def test_fused_step_against_unfused_route(case, use_mask):
    """48 angles in one batch (wave and heavy rows), L1 and TV terms on: volume, m, v, gradient and table bit for bit, mean bounded"""
    idx = np.arange(N_THETA)
    a, b = _solver(case, N_THETA), _solver(case, N_THETA)
    a.step(0, idx, LR, use_mask=use_mask, **REG)
    assert a._g_stale                                                  # the one-pass tail ran
    b.loss_and_grad(idx)
    gb = b.gradient_to_host()
    b.adam_update(0, LR, use_mask=use_mask, **REG)
    (va, ma, wa), (vb, mb_, wb) = _state(a), _state(b)
    ta, mean_a = a.eng.modulation_table()
    tb, mean_b = b.eng.modulation_table()
    ga = a.gradient_to_host()
    assert not np.array_equal(vb[0], case['od'].astype(np.float32)) and np.any(mb_) and np.any(wb)
    assert np.array_equal(_bits(va[0]), _bits(vb[0])) and np.array_equal(_bits(va[1]), _bits(vb[1]))
    assert np.array_equal(_bits(ma), _bits(mb_)) and np.array_equal(_bits(wa), _bits(wb))
    assert np.array_equal(_bits(ga[0]), _bits(gb[0])) and np.array_equal(_bits(ga[1]), _bits(gb[1]))
    assert ta.size == N * N * N and np.any(ta) and np.array_equal(_bits(ta), _bits(tb))
    assert mean_a != 0                                                 # the mean rides on the carrier here: it was formed
    print('mean, one pass', mean_a, 'unfused', mean_b, '|difference|', abs(mean_a - mean_b))
    _check_mean('one-pass tail', ta, mean_a, _D_fused(N, N * N))


def test_two_fused_steps_against_two_unfused(case):
    """8 of the angles per step: the second step runs on the table and the mean the first one-pass tail left"""
    sched = [np.arange(0, N_THETA, 6), np.arange(3, N_THETA, 6)]
    a, b = _solver(case, 8), _solver(case, 8)
    for i, idx in enumerate(sched):
        a.step(i, idx, LR, **REG)
        b.loss_and_grad(idx)
        b.adam_update(i, LR, **REG)
    (va, _, _), (vb, _, _) = _state(a), _state(b)
    same = np.array_equal(_bits(va[0]), _bits(vb[0])) and np.array_equal(_bits(va[1]), _bits(vb[1]))
    print('volume after two steps:', 'bit-identical' if same else 'NOT bit-identical (the means round to other float32 carrier scalars)')
    if not same:
        # the bounds tests/test_gpu_fullfield.py holds a step to (test_reconstruct_fullfield_end_to_end)
        diff = np.abs(va[0].astype(np.float64) - vb[0])
        print('max |delta difference|', diff.max(), 'share above 0.05 lr', np.mean(diff > 0.05 * LR))
        assert np.mean(diff > 0.05 * LR) < 2e-3
        assert diff.max() <= 2.5 * LR * len(sched)
        assert np.linalg.norm(va[0].astype(np.float64) - vb[0]) <= 2e-3 * np.linalg.norm(vb[0])
        assert np.linalg.norm(va[1].astype(np.float64) - vb[1]) <= 2e-2 * np.linalg.norm(vb[1])


def _table_address(s):
    table, n = ctypes.c_void_p(), ctypes.c_size_t(0)
    s.ctx.check(s.ctx.lib.bdof_modulation_table(s.ctx.handle, ctypes.byref(table), ctypes.byref(n), None))
    return table.value, n.value


SENTINEL_ENTRY = np.array([-777.25, 333.5], dtype=np.float32)
AT = 12345


def _plant(s, addr):
    s.ctx.check(s.ctx.lib.bdof_memcpy_h2d(s.ctx.handle, addr + 8 * AT, SENTINEL_ENTRY.ctypes.data, 8))
    s.ctx.sync()


def _entry(s, addr):
    out = np.empty(2, dtype=np.float32)
    s.ctx.check(s.ctx.lib.bdof_memcpy_d2h(s.ctx.handle, out.ctypes.data, addr + 8 * AT, 8))
    s.ctx.sync()
    return out


def test_no_table_rebuild_after_a_fused_step(case):
    """a sentinel planted in the table survives the sweep that follows a one-pass tail, and goes when the table is rebuilt: after
    an unfused update (the control) and after set_volume from the host"""
    idx = np.arange(0, N_THETA, 6)
    s = _solver(case, 8)
    addr, n = _table_address(s)
    assert n == N * N * N
    # control: the unfused route rebuilds the table at the next sweep
    s.loss_and_grad(idx)
    s.adam_update(0, LR, **REG)
    _plant(s, addr)
    s.loss_and_grad(idx)
    assert _table_address(s) == (addr, n) and not np.array_equal(_entry(s, addr), SENTINEL_ENTRY)
    # one-pass tail: the table it wrote is the one the next sweep reads
    s.step(1, idx, LR, **REG)
    _plant(s, addr)
    s.loss_and_grad(idx)
    assert _table_address(s) == (addr, n) and np.array_equal(_entry(s, addr), SENTINEL_ENTRY)
    # a host upload of the volume: rebuilt
    vol = s.get_volume()
    s.set_volume(vol[0], vol[1])
    s.loss_and_grad(idx)
    fresh, _ = s.eng.modulation_table()
    assert _table_address(s) == (addr, n) and not np.array_equal(_entry(s, addr), SENTINEL_ENTRY)
    # ... to what the one-pass tail had written, but for the sentinel: the volume is the same
    s2 = _solver(case, 8)
    s2.set_volume(vol[0], vol[1])
    ref, _ = s2.eng.modulation_table()
    assert np.array_equal(_bits(fresh), _bits(ref))


def _call_fused(s, accumulate=0, row0=0, n_rows=None, x_new=None):
    from beyond_dof_amd import _lib
    lib, h = s.ctx.lib, s.ctx.handle
    n_rows = s.dim_x * s.dim_z if n_rows is None else n_rows
    new = s.x[1 - s.cur].ptr if x_new is None else x_new
    s.ctx.check(lib.bdof_rotation_adjoint_adam(h, s.mb, s.angle_buf.ptr, None, row0, n_rows, accumulate, 1.0, s.x[s.cur].ptr, new, s.m.ptr,
                                               s.v.ptr, None, s.dim_x, s.dim_z, s.dim_y, 1.0, 0.0, 0.0, 0.0, LR, 0.9, 0.999, 1e-8, 0, 1))
    return _lib


def test_refusals(case):
    from beyond_dof_amd._lib import BdofError
    from beyond_dof_amd.solver import FullfieldSolver
    s = _solver(case, 2)
    before = _state(s)
    with pytest.raises(BdofError, match='does not carry accumulate'):
        _call_fused(s, accumulate=1)
    with pytest.raises(BdofError, match='does not carry a row range'):
        _call_fused(s, row0=0, n_rows=N * N - 1)
    with pytest.raises(BdofError, match='does not carry a row range'):
        _call_fused(s, row0=4, n_rows=N * N - 4)
    with pytest.raises(BdofError, match='x_new must not alias x_old'):
        _call_fused(s, x_new=s.x[s.cur].ptr)
    after = _state(s)
    assert all(np.array_equal(p, q) for p, q in zip(before[0] + before[1:], after[0] + after[1:]))      # nothing ran
    bil = FullfieldSolver(N, N, N, 4, 2, E, PS, free_prop_cm=None, rotation='bilinear', theta=np.linspace(0, np.pi, 4, endpoint=False))
    bil.set_volume(case['od'], case['ob'])
    bil.rot.stage(bil.eng, bil.x[bil.cur], np.array([0, 1]), 2, bil.conv)                            # the object is now bound as a batch of rotated factors
    with pytest.raises(BdofError, match='does not carry the bilinear rotation'):
        _call_fused(bil)


def test_hand_made_table_ny_130():
    """NY = 130 (a second group of float4 columns with one lane), rows with 0, 1, 256 and 257 sources, through the entry point: the
    stored gradient is the exact scatter-add, and volume, moments and table are those of the separate calls on the same inputs"""
    import __graft_entry__ as entry
    entry.build()
    from beyond_dof_amd import _lib
    ny = 130
    c = gg.rot_case_wide(ny)
    nx, nz = c['nx'], c['nz']
    n = nx * nz
    dev = gg.RotDevice(ny, nx, nz, 5, c['dests'])
    eng, ctx, lib, h = dev.eng, dev.ctx, dev.lib, dev.h
    eng.set_physics(E, PS, None)
    eng.set_probe(np.ones((ny, nx)), np.zeros((ny, nx)))
    dev.set_grot(c['grot'])
    rest = gg.rot_adjoint_restated(c['grot'], dev.tab, c['ang'])
    rng = np.random.default_rng(7)
    x_old = rng.uniform(0, 2e-6, size=(n, ny, 2)).astype(np.float32)
    x_old[rng.uniform(size=(n, ny)) < 0.1] = 0
    m0 = (1e-9 * rng.normal(size=(n, ny, 2))).astype(np.float32)
    v0 = (1e-18 * rng.uniform(size=(n, ny, 2))).astype(np.float32)
    mask = (rng.uniform(size=(n, ny)) > 0.2).astype(np.float32)
    up = dev.up
    xo, mk, ang, tab = up(x_old), up(mask), up(c['ang']), up(dev.tab)
    kw = (nx, nz, ny, 1e-9, 1.5e-8, 1.5e-9, 1e-9, LR, 0.9, 0.999, 1e-8, 3, 1)

    def table_of(buf_ptr):
        ctx.check(lib.bdof_set_object(h, buf_ptr, n, ny, tab.ptr, nx, len(c['dests'])))
        return eng.modulation_table()

    table_of(xo.ptr)                                                   # the object whose step this is
    # the separate calls
    g_u = gg.Guarded(ctx, gg.sentinels((n, ny, 2)))
    xn_u, m_u, v_u = gg.Guarded(ctx, gg.sentinels((n, ny, 2))), gg.Guarded(ctx, m0), gg.Guarded(ctx, v0)
    ctx.check(lib.bdof_rotation_adjoint_rows(h, 5, ang.ptr, g_u.ptr, 0, n, 0, 1.0))
    ctx.check(lib.bdof_adam_step(h, xo.ptr, xn_u.ptr, g_u.ptr, m_u.ptr, v_u.ptr, mk.ptr, *kw))
    t_u, mean_u = table_of(xn_u.ptr)
    table_of(xo.ptr)
    # one pass, the gradient stored as well
    g_f = gg.Guarded(ctx, gg.sentinels((n, ny, 2)))
    xn_f, m_f, v_f = gg.Guarded(ctx, gg.sentinels((n, ny, 2))), gg.Guarded(ctx, m0), gg.Guarded(ctx, v0)
    ctx.check(lib.bdof_rotation_adjoint_adam(h, 5, ang.ptr, g_f.ptr, 0, n, 0, 1.0, xo.ptr, xn_f.ptr, m_f.ptr, v_f.ptr, mk.ptr, *kw))
    ctx.check(lib.bdof_set_object(h, xn_f.ptr, n, ny, tab.ptr, nx, len(c['dests'])))
    t_f, mean_f = eng.modulation_table()
    ctx.sync()
    g = g_f.download()
    assert np.array_equal(g, rest) and np.array_equal(g_u.download(), rest)
    assert not np.any(rest[0]) and np.any(rest[5]) and np.any(rest[60]) and np.any(rest[119])
    xn = xn_f.download()
    assert np.array_equal(_bits(xn), _bits(xn_u.download()))
    assert np.array_equal(_bits(m_f.download()), _bits(m_u.download())) and np.array_equal(_bits(v_f.download()), _bits(v_u.download()))
    assert np.array_equal(_bits(t_f), _bits(t_u)) and np.any(t_f)
    # the row without a source took its update from a zero gradient (the L1 term moves it), and has its table entries
    assert np.any(xn[0] != x_old[0]) and np.any(t_f.reshape(n, ny)[0])
    assert mean_f != 0
    print('mean, one pass', mean_f, 'separate', mean_u, '|difference|', abs(mean_f - mean_u))
    _check_mean('one-pass tail, NY = 130', t_f, mean_f, _D_fused(ny, n))
    # without the gradient pointer: the same, and nothing else is written
    xn_n, m_n, v_n = gg.Guarded(ctx, gg.sentinels((n, ny, 2))), gg.Guarded(ctx, m0), gg.Guarded(ctx, v0)
    table_of(xo.ptr)
    ctx.check(lib.bdof_rotation_adjoint_adam(h, 5, ang.ptr, None, 0, n, 0, 1.0, xo.ptr, xn_n.ptr, m_n.ptr, v_n.ptr, mk.ptr, *kw))
    ctx.sync()
    assert np.array_equal(_bits(xn_n.download()), _bits(xn)) and np.array_equal(_bits(m_n.download()), _bits(m_f.download()))
