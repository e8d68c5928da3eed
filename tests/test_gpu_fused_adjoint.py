"""The fused adjoint sweep of bdof_loss_grad (bdof_set_adjoint_fusion; k_slice_y_adj / k_slice_x_adj, csrc/bdof_kernels.h): below
the top slice one kernel per slice on lines of alternating direction, through the transposes of the separable Fresnel steps, reading
the phi tape the fused forward sweep leaves — its odd slots in tile blocks (k_slice_x<BLK>).

What is compared: the rotated-frame gradient rows of the fused-adjoint route, of stage 1 (fused forward sweep, two-kernel adjoint)
and of the two-kernel sweep against the float64 twin on the same context (bdof_loss_grad_tf_f64).  The fused-adjoint route's error
may be at most TWICE the two-kernel route's at the same shape (a different rounding sequence of the same length; a real mistake is
orders of magnitude), and every error sits within what tests/test_gpu_parity.py asserts for its quantity (loss 1e-5, wave 5e-6,
gradient 2e-4, all relative).  The forward arithmetic does not change with the adjoint route, only where the odd phi slots are
stored: loss and detector wave equal stage 1's bit for bit, and the blocked slots, un-blocked on the host, equal stage 1's.  The
figures are printed.  (Helpers after tests/test_gpu_fused_sweep.py's.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import bdof_oracle as orc

E_EV, PSIZE, FP = 5000., 1e-7, 1e-4
LOSS_TOL, WAVE_TOL, GRAD_TOL = 1e-5, 5e-6, 2e-4      # tests/test_gpu_parity.py's bounds for the float32 kernels
FACTOR = 2.0


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


@pytest.fixture(scope='module')
def engine_mod():
    import __graft_entry__ as entry
    entry.build()
    from beyond_dof_amd import engine
    return engine


def _probe(rng, Y, X):
    """Nearly uniform (so that MultisliceEngine.set_probe lets it ride on a scalar carrier), with a scattered part of its own."""
    return 1 + 0.02 * rng.normal(size=(Y, X)), 0.02 * rng.normal(size=(Y, X))


def _engine(engine_mod, Y, X, S, B, rng, fp=FP, **kw):
    eng = engine_mod.MultisliceEngine(Y, X, S, B, with_grad=True, engine='streaming', **kw)
    eng.set_physics(E_EV, PSIZE, fp)
    pr, pi = _probe(rng, Y, X)
    eng.set_probe(pr, pi)
    return eng, pr, pi


def _run(eng, B, meas, mode, adj=False, angle_idx=None, xoff=None, yoff=None, f64=False):
    """One loss + gradient: (loss, detector wave (B, Y, X) or None for the twin, g_delta, g_beta, (forward, adjoint) routes that ran)."""
    from beyond_dof_amd import _lib
    if f64:
        loss = eng.loss_grad(B, meas, angle_idx=angle_idx, xoff=xoff, yoff=yoff, f64=True)
        gd, gb = eng.grad_batch_to_host(B)
        return loss, None, gd, gb, None
    eng.set_sweep_fusion(mode)
    eng.set_adjoint_fusion(adj)
    m = eng._meas_to_device(meas)
    a, xo, yo = eng._idx_bufs(angle_idx, xoff, yoff)
    out = _lib.DeviceBuffer(eng.ctx, B * eng.nx * eng.ny * 8, np.complex64, (B, eng.nx, eng.ny))
    eng.ctx.check(eng.lib.bdof_loss_grad(eng.h, B, _lib._ptr(a), _lib._ptr(xo), _lib._ptr(yo), m.ptr, out.ptr))
    loss = eng.get_loss()
    ran = (eng.sweep_fused, eng.adjoint_fused)
    wave = eng._wave_to_host(out, B)
    gd, gb = eng.grad_batch_to_host(B)
    return loss, wave, gd, gb, ran


def _phi_tape(eng, B, S, blocked):
    """Tape slots 0 .. S-2 after a fused forward sweep (bdof_tape_slot) as [z][b][x][y]; blocked: the odd slots hold tile blocks
    [b][NY / T][NX][T], T = max(16, 4096 / NX) (include/bdof.h), and are un-blocked here."""
    out = np.empty((S - 1, B, eng.nx, eng.ny), dtype=np.complex64)
    eng.ctx.sync()
    T = max(16, 4096 // eng.nx)
    for z in range(S - 1):
        ptr = eng.lib.bdof_tape_slot(eng.h, z)
        assert ptr
        eng.ctx.check(eng.lib.bdof_memcpy_d2h(eng.h, out[z].ctypes.data, ptr, out[z].nbytes))
        if blocked and z % 2:
            out[z] = out[z].reshape(B, eng.ny // T, eng.nx, T).transpose(0, 2, 1, 3).reshape(B, eng.nx, eng.ny)
    return out


def _errors(run, twin, ref_wave):
    g = np.stack([run[2], run[3]])
    g64 = np.stack([twin[2], twin[3]])
    return abs(run[0] - twin[0]) / abs(twin[0]), rel(run[1], ref_wave), rel(g, g64)


def _check_routes(name, adj, stage1, two, twin, ref):
    """The adjoint route against stage 1 (forward results bit for bit) and against the two-kernel route (factor two, parity bounds)."""
    assert two[4] == (0, 0) and stage1[4] == (1, 0) and adj[4] == (1, 1), (two[4], stage1[4], adj[4])
    assert adj[0] == stage1[0], (name, adj[0], stage1[0])
    assert np.array_equal(adj[1], stage1[1]), name
    e_adj, e_one, e_two = _errors(adj, twin, ref), _errors(stage1, twin, ref), _errors(two, twin, ref)
    print('fused adjoint', name, 'errors (loss, wave, gradient): fused adjoint', tuple(float(e) for e in e_adj),
          ' stage 1', tuple(float(e) for e in e_one), ' two-kernel', tuple(float(e) for e in e_two))
    for e in (e_adj, e_one, e_two):
        assert e[0] <= LOSS_TOL and e[1] <= WAVE_TOL and e[2] <= GRAD_TOL, (name, e_adj, e_one, e_two)
    assert e_adj[2] <= FACTOR * e_two[2], (name, e_adj, e_two)


def _batch_case(engine_mod, B, Y, X, S, seed, dmax=2e-5, **kw):
    rng = np.random.default_rng(seed)
    eng, pr, pi = _engine(engine_mod, Y, X, S, B, rng, **kw)
    delta = rng.uniform(0, dmax, size=(B, Y, X, S)).astype(np.float32).astype(np.float64)
    beta = (0.1 * delta).astype(np.float32).astype(np.float64)
    eng.set_object_batch(delta, beta)
    p64 = (pr + 1j * pi).astype(np.complex64)
    ref, _ = orc.multislice_propagate_batch_numpy(delta, beta, p64.real.astype(np.float64), p64.imag.astype(np.float64), E_EV, PSIZE, FP,
                                                  delta.shape, return_probe_array=False)
    meas = (np.abs(ref) * (1 + 0.05 * rng.normal(size=ref.shape))).astype(np.float32).astype(np.float64)
    return eng, delta, beta, ref, meas, rng


def _accuracy(engine_mod, name, B, Y, X, S, seed):
    eng, delta, beta, ref, meas, rng = _batch_case(engine_mod, B, Y, X, S, seed)
    eng.enable_tf_f64()
    twin = _run(eng, B, meas, 0, f64=True)
    two = _run(eng, B, meas, 0)
    stage1 = _run(eng, B, meas, 1)
    adj = _run(eng, B, meas, 1, adj=True)
    _check_routes(name, adj, stage1, two, twin, ref)
    return eng, meas, adj


@pytest.mark.parametrize('Y,X', [(64, 128), (128, 64), (256, 64), (64, 256)])
def test_unequal_sides_vs_twin(engine_mod, Y, X):
    """NX != NY, S = 4, 2 fields: every swapped stride, swapped table (hx / hy, twY / twX) or swapped block size shows — the tile
    is 64, 32 and 16 rows for lines of 64, 128 and 256 points.  S = 4 runs the top slice unfused, then HEAD, the x-line kernel, LAST."""
    _accuracy(engine_mod, '{}x{}'.format(Y, X), 2, Y, X, 4, 5)


def test_lookup_table_64_vs_twin(engine_mod):
    """64 x 64 field, S = 6, 3 angles of a 12-angle rotation table built as the solver builds it (clamped border rows): the x-line
    adjoint kernel finds its table rows through the lookup, eight per thread; S = 6 also runs a y-line kernel that is neither HEAD
    nor LAST."""
    from beyond_dof_amd import util, _lib
    n, S, n_theta, B = 64, 6, 12, 3
    rng = np.random.default_rng(11)
    eng, pr, pi = _engine(engine_mod, n, n, S, B, rng)
    od = rng.uniform(0, 2e-5, size=(n, n, S)).astype(np.float32)              # (Y, X, Z)
    ob = (0.1 * od).astype(np.float32)
    coords = orc.rotation_lookup([n, n, S], n_theta)
    tab, _, _ = util.device_rotation_tables(coords, n, S)
    assert any(len(np.unique(t)) < t.size for t in tab)                        # clamped border rows: some source row feeds several
    rows = util.volume_to_rows(od, ob)                                         # [X][Z][Y][2]
    vol = _lib.DeviceBuffer.from_host(eng.ctx, rows)
    tbuf = _lib.DeviceBuffer.from_host(eng.ctx, tab)
    eng.set_volume(vol, n * S, n, tbuf, n, n_theta)
    idx = [1, 5, 10]
    flat = rows.reshape(n * S, n, 2).astype(np.float64)
    batch = np.stack([flat[tab[a]] for a in idx])                              # [b][z][x][y][2]
    delta, beta = util.rows_to_batch(batch)
    p64 = (pr + 1j * pi).astype(np.complex64)
    ref, _ = orc.multislice_propagate_batch_numpy(delta, beta, p64.real.astype(np.float64), p64.imag.astype(np.float64), E_EV, PSIZE, FP,
                                                  delta.shape, return_probe_array=False)
    meas = (np.abs(ref) * (1 + 0.05 * rng.normal(size=ref.shape))).astype(np.float32).astype(np.float64)
    eng.enable_tf_f64()
    twin = _run(eng, B, meas, 0, angle_idx=idx, f64=True)
    two = _run(eng, B, meas, 0, angle_idx=idx)
    stage1 = _run(eng, B, meas, 1, angle_idx=idx)
    adj = _run(eng, B, meas, 1, adj=True, angle_idx=idx)
    _check_routes('64^2 lookup', adj, stage1, two, twin, ref)


def test_flagship_line_length_second_tile_and_streams(engine_mod):
    """512 x 512, S = 4, 17 fields: PASSES = 2 and 16 values waiting in registers in the transposed phase, and 544 tiles on 512
    workgroup slots — some workgroup takes a second tile.  One sub-batch stream and two: bit-identical."""
    B = 17
    eng, meas, adj = _accuracy(engine_mod, '512^2 x 17', B, 512, 512, 4, 7)
    res = {}
    for n in (1, 2):
        eng.set_streams(n)
        assert eng.batch_groups(B) == n
        res[n] = _run(eng, B, meas, 1, adj=True)
        assert res[n][4] == (1, 1)
    eng.set_streams(-1)
    assert res[1][0] == res[2][0]
    for i in (1, 2, 3):
        assert np.array_equal(res[1][i], res[2][i])


def test_dither_bookkeeping_beyond_the_copies(engine_mod):
    """S = 70 slices at 64^2, more than the 64 dithered copies of every constant: the conjugated copy of each step — twiddles,
    sqrt(1/2), hx / hy — must be the one the forward sweep took for that step, also where the slice index wraps around."""
    _accuracy(engine_mod, '64^2 S=70', 2, 64, 64, 70, 29)


@pytest.mark.parametrize('z0', [3, 2])
def test_modulation_position(engine_mod, z0):
    """An object that is zero except for ONE voxel row at a known (b, x, z), z odd (an x-line slice) or even (a y-line slice that
    is neither the sweep's head nor its last), 64^2, S = 6.  What the row changes in the gradient rows of every slice, row by row,
    must be what it changes in the float64 twin; the other wavefield's rows are held to the same bound (they change by rounding
    only).  The blocked odd tape slots, un-blocked on the host, equal stage 1's bit for bit."""
    B, n, S = 2, 64, 6
    x0, b0 = 21, 1
    rng = np.random.default_rng(17)
    eng, pr, pi = _engine(engine_mod, n, n, S, B, rng)
    delta = np.zeros((B, n, n, S))
    delta[b0, :, x0, z0] = rng.uniform(1e-2, 2e-2, size=n).astype(np.float32)          # strong: k delta = 0.25 .. 0.5 rad in one slice
    beta = (0.1 * delta).astype(np.float32).astype(np.float64)
    meas = np.abs(1 + 0.05 * rng.normal(size=(B, n, n))).astype(np.float32).astype(np.float64)
    out, phi = {}, {}
    for name, (d, bt) in (('row', (delta, beta)), ('empty', (0 * delta, 0 * beta))):
        eng.set_object_batch(d, bt)
        eng.enable_tf_f64()
        out[name, 'twin'] = _run(eng, B, meas, 0, f64=True)
        out[name, 'two'] = _run(eng, B, meas, 0)
        out[name, 'stage1'] = _run(eng, B, meas, 1)
        phi[name, 'stage1'] = _phi_tape(eng, B, S, blocked=False)
        out[name, 'adj'] = _run(eng, B, meas, 1, adj=True)
        phi[name, 'adj'] = _phi_tape(eng, B, S, blocked=True)
        assert out[name, 'two'][4] == (0, 0) and out[name, 'stage1'][4] == (1, 0) and out[name, 'adj'][4] == (1, 1)
        assert np.array_equal(phi[name, 'adj'], phi[name, 'stage1'])
        assert out[name, 'adj'][0] == out[name, 'stage1'][0] and np.array_equal(out[name, 'adj'][1], out[name, 'stage1'][1])
    assert np.abs(phi['row', 'adj'][z0][b0, x0] - phi['empty', 'adj'][z0][b0, x0]).min() >= 0.1      # the tape does hold the row
    dt = np.stack([out['row', 'twin'][2] - out['empty', 'twin'][2], out['row', 'twin'][3] - out['empty', 'twin'][3]])     # [2][b][y][x][z]
    scale = np.sqrt((dt ** 2).sum(axis=(0, 2)))                                        # per (b, x, z) row
    assert scale[b0, x0, z0] > 0 and np.all(scale[1 - b0] == 0)                       # the other wavefield sees nothing
    worst = {}
    for m in ('two', 'adj'):
        dm = np.stack([out['row', m][2] - out['empty', m][2], out['row', m][3] - out['empty', m][3]]).astype(np.float64)
        err = np.sqrt(((dm - dt) ** 2).sum(axis=(0, 2)))
        worst[m] = float((err / scale[b0].max()).max())                                # all rows of both wavefields
    print('fused adjoint modulation position z =', z0, ': worst row error of the change in the gradient', worst)
    assert worst['two'] <= GRAD_TOL and worst['adj'] <= GRAD_TOL and worst['adj'] <= FACTOR * worst['two'], worst


@pytest.mark.parametrize('case', ['odd_S', 'S_2', 'binning', 'recompute', 'far_field', 'window_offsets', 'non_separable'])
def test_fallbacks_run_the_two_kernel_sweep(engine_mod, case):
    """The configurations that are not eligible for the fused forward sweep, with both switches on: bdof_adjoint_fused reports 0 and
    the results are bit-identical to everything off."""
    B, n = 2, 64
    rng = np.random.default_rng(23)
    S = {'odd_S': 5, 'S_2': 2}.get(case, 4)
    kw = {'binning': dict(slice_binning=2), 'recompute': dict(recompute=True)}.get(case, {})
    eng, pr, pi = _engine(engine_mod, n, n, S, B, rng, fp='inf' if case == 'far_field' else FP, **kw)
    delta = rng.uniform(0, 2e-5, size=(B, n, n, S))
    meas = np.abs(1 + 0.05 * rng.normal(size=(B, n, n)))
    run_kw = {}
    if case == 'window_offsets':
        from beyond_dof_amd import util, _lib
        od = rng.uniform(0, 2e-5, size=(n, n, S)).astype(np.float32)
        tab, _, _ = util.device_rotation_tables(orc.rotation_lookup([n, n, S], 4), n, S)
        eng.set_volume(_lib.DeviceBuffer.from_host(eng.ctx, util.volume_to_rows(od, 0.1 * od)), n * S, n,
                       _lib.DeviceBuffer.from_host(eng.ctx, tab), n, 4)
        run_kw = dict(angle_idx=[0, 2], xoff=[0, 0], yoff=[0, 0])             # offsets given, even if zero: the windowed path
    else:
        eng.set_object_batch(delta, 0.1 * delta)
    if case == 'non_separable':
        hs64 = eng.optics.table(eng._step_nm(), tiled=True, dtype=np.complex128).copy()
        hs64[3, 5] *= np.exp(1e-6j)                                           # one entry of the float64 table turned by 1e-6 rad
        eng.ctx.check(eng.lib.bdof_set_transfer_f64(eng.h, hs64.ctypes.data))
    r1 = _run(eng, B, meas, 1, adj=True, **run_kw)
    r0 = _run(eng, B, meas, 0, adj=False, **run_kw)
    assert r1[4] == (0, 0) and r0[4] == (0, 0)
    assert r1[0] == r0[0]
    for i in (1, 2, 3):
        assert np.array_equal(r1[i], r0[i])


def test_switch_and_query(engine_mod):
    from beyond_dof_amd import _lib
    rng = np.random.default_rng(31)
    eng, pr, pi = _engine(engine_mod, 64, 64, 4, 1, rng)
    assert eng.adjoint_fused == 0                                 # a new ctx: nothing has run yet
    with pytest.raises(_lib.BdofError):
        eng.ctx.check(eng.lib.bdof_set_adjoint_fusion(eng.h, 2))
    with pytest.raises(_lib.BdofError):
        eng.ctx.check(eng.lib.bdof_set_adjoint_fusion(eng.h, -1))
    delta = rng.uniform(0, 2e-5, size=(1, 64, 64, 4))
    eng.set_object_batch(delta, 0.1 * delta)
    meas = np.ones((1, 64, 64))
    eng.set_sweep_fusion(1)
    eng.loss_grad(1, meas)
    assert (eng.sweep_fused, eng.adjoint_fused) == (1, 0)         # a new ctx starts with the adjoint switch off
    assert _run(eng, 1, meas, 1, adj=True)[4] == (1, 1)
    assert _run(eng, 1, meas, 2, adj=True)[4] == (1, 1)           # bdof_sweep_fused keeps reporting stage 1
    assert _run(eng, 1, meas, 0, adj=True)[4] == (0, 0)           # the switch alone, without the fused forward sweep, runs nothing
    eng.forward(1)                                                # bdof_forward is not fused and leaves the record alone
    assert (eng.sweep_fused, eng.adjoint_fused) == (0, 0)
    assert _run(eng, 1, meas, 1, adj=False)[4] == (1, 0)
