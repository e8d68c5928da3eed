"""When the x-line slice kernels (k_slice_x / k_slice_x_adj, csrc/bdof_kernels.h) ask for their operands: the rotation lookups are
wave-private (one per lane at the top of a tile, handed to the using lanes by a wave shuffle), pass 0's table segments are requested
in the row phase and cross the phase barrier in registers, every other load of the transposed phase stands ahead of its first store.
The arithmetic is untouched, so what can go wrong is an operand: a wrong or stale lookup, a segment fetched for the wrong pass, row
or tile, the clamping at the volume's edge.  The cases aim there, at every line length (512 points is the only one with two
transposed passes) and with workgroups that run two tiles of different angles.

Rules and helpers are tests/test_gpu_fused_adjoint.py's: against the float64 twin on the same context (bdof_loss_grad_tf_f64),
within tests/test_gpu_parity.py's bounds, the fused-adjoint route's gradient error at most twice the two-kernel route's, loss and
detector wave bit-identical to the route with adjoint fusion off.  The figures are printed."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import bdof_oracle as orc

E_EV, PSIZE, FP = 5000., 1e-7, 1e-4
LOSS_TOL, WAVE_TOL, GRAD_TOL = 1e-5, 5e-6, 2e-4      # tests/test_gpu_parity.py's bounds for the float32 kernels
FACTOR = 2.0
NCU = 256           # MI355X, which the gpu mark asks for (tests/test_gpu_modulation.py); a row kernel's grid is at most 2 NCU workgroups


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


@pytest.fixture(scope='module')
def engine_mod():
    import __graft_entry__ as entry
    entry.build()
    from beyond_dof_amd import engine
    return engine


def _probe(rng, Y, X):
    return 1 + 0.02 * rng.normal(size=(Y, X)), 0.02 * rng.normal(size=(Y, X))


def _engine(engine_mod, Y, X, S, B, rng, **kw):
    eng = engine_mod.MultisliceEngine(Y, X, S, B, with_grad=True, engine='streaming', **kw)
    eng.set_physics(E_EV, PSIZE, FP)
    pr, pi = _probe(rng, Y, X)
    eng.set_probe(pr, pi)
    return eng, pr, pi


def _run(eng, B, meas, mode, adj=False, angle_idx=None, f64=False):
    """One loss + gradient: (loss, detector wave (B, Y, X) or None for the twin, g_delta, g_beta, (forward, adjoint) routes that ran)."""
    from beyond_dof_amd import _lib
    if f64:
        loss = eng.loss_grad(B, meas, angle_idx=angle_idx, f64=True)
        gd, gb = eng.grad_batch_to_host(B)
        return loss, None, gd, gb, None
    eng.set_sweep_fusion(mode)
    eng.set_adjoint_fusion(adj)
    m = eng._meas_to_device(meas)
    a, xo, yo = eng._idx_bufs(angle_idx, None, None)
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
    print('x-line operands', name, 'errors (loss, wave, gradient): fused adjoint', tuple(float(e) for e in e_adj),
          ' stage 1', tuple(float(e) for e in e_one), ' two-kernel', tuple(float(e) for e in e_two))
    for e in (e_adj, e_one, e_two):
        assert e[0] <= LOSS_TOL and e[1] <= WAVE_TOL and e[2] <= GRAD_TOL, (name, e_adj, e_one, e_two)
    assert e_adj[2] <= FACTOR * e_two[2], (name, e_adj, e_two)


def _table_case(engine_mod, Y, X, S, B, n_theta, angles, seed, vol_nx=None, vol_ny=None):
    """A (vol_ny, vol_nx, S) volume behind a rotation table built as the solver builds it (tests/test_gpu_fused_adjoint.py's
    test_lookup_table_64_vs_twin: clamped border rows), wavefield b at angle angles[b % len(angles)].  vol_nx < X: the x beyond the
    table have no source row; vol_ny < Y: the y beyond the volume are clamped in the load and their factors are zero.  Returns the
    engine, the angle list, the oracle's detector waves of the equivalent batch of rotated objects, the measurement."""
    from beyond_dof_amd import util, _lib
    vol_nx, vol_ny = vol_nx or X, vol_ny or Y
    rng = np.random.default_rng(seed)
    eng, pr, pi = _engine(engine_mod, Y, X, S, B, rng)
    od = rng.uniform(0, 2e-5, size=(vol_ny, vol_nx, S)).astype(np.float32)    # (Y, X, Z)
    ob = (0.1 * od).astype(np.float32)
    coords = orc.rotation_lookup([vol_ny, vol_nx, S], n_theta)
    tab, _, _ = util.device_rotation_tables(coords, vol_nx, S)
    assert any(len(np.unique(t)) < t.size for t in tab[angles])               # clamped border rows: some source row feeds several
    rows = util.volume_to_rows(od, ob)                                        # [X][Z][Y][2]
    vol = _lib.DeviceBuffer.from_host(eng.ctx, rows)
    tbuf = _lib.DeviceBuffer.from_host(eng.ctx, tab)
    eng.set_volume(vol, vol_nx * S, vol_ny, tbuf, vol_nx, n_theta)
    idx = [angles[b % len(angles)] for b in range(B)]
    flat = rows.reshape(vol_nx * S, vol_ny, 2).astype(np.float64)
    per_angle = {a: flat[tab[a]] for a in angles}                             # [z][x][y][2]
    batch = np.zeros((B, S, X, Y, 2))
    for b in range(B):
        batch[b, :, :vol_nx, :vol_ny] = per_angle[idx[b]]
    delta, beta = util.rows_to_batch(batch)
    p64 = (pr + 1j * pi).astype(np.complex64)
    ref, _ = orc.multislice_propagate_batch_numpy(delta, beta, p64.real.astype(np.float64), p64.imag.astype(np.float64), E_EV, PSIZE, FP,
                                                  delta.shape, return_probe_array=False)
    meas = (np.abs(ref) * (1 + 0.05 * rng.normal(size=ref.shape))).astype(np.float32).astype(np.float64)
    return eng, idx, ref, meas


def _routes(eng, B, meas, idx):
    eng.enable_tf_f64()
    twin = _run(eng, B, meas, 0, angle_idx=idx, f64=True)
    two = _run(eng, B, meas, 0, angle_idx=idx)
    stage1 = _run(eng, B, meas, 1, angle_idx=idx)
    adj = _run(eng, B, meas, 1, adj=True, angle_idx=idx)
    return adj, stage1, two, twin


def _one_stream_two_tiles(eng, B, tiles):
    """Put the whole batch on one sub-batch stream and assert that its `tiles` x-line tiles are more than the 2 x CU-count
    workgroups a row kernel's grid has at most, so that a workgroup runs two.  The CU count is asked of the engine itself: with
    the automatic split, batch_groups(Bq) is 2 exactly when Bq nx / 16 >= 2 x CU-count (Bq >= 4; include/bdof.h), and Bq is the
    largest batch with Bq nx / 16 <= tiles - 1."""
    Bq = (tiles - 1) * 16 // eng.nx
    assert Bq >= 4
    eng.set_streams(-1)
    assert eng.batch_groups(Bq) == 2, 'fewer than {} tiles fit twice on the CUs of this device ({} assumed)'.format(tiles, NCU)
    eng.set_streams(1)
    assert eng.batch_groups(B) == 1


@pytest.fixture(scope='module')
def lookup512(engine_mod):
    """512-point x-lines (two transposed passes) through the lookup, 64 rows per field = 4 tiles, S = 4, 2 NCU / 4 + 1 fields:
    one tile more than fits twice on every CU, so on one stream every workgroup runs two tiles, 64 or 65 fields apart; the fields
    cycle through three angles, so the two tiles of a workgroup never share an angle.  The table is 500 wide: x = 500 .. 511 have no
    source row, the rows beside them are the clamped border.  Computed once: the four routes on ONE stream (two tiles per
    workgroup, asserted), then the fused routes again on one and on two sub-batch streams (two streams: one tile per workgroup)."""
    Y, X, S = 64, 512, 4
    B = 2 * NCU // (Y // 16) + 1
    eng, idx, ref, meas = _table_case(engine_mod, Y, X, S, B, 12, [1, 5, 10], 41, vol_nx=500)
    assert all(idx[b] != idx[b + 64] and idx[b] != idx[b + 65] for b in range(B - 65))
    _one_stream_two_tiles(eng, B, B * (Y // 16))
    routes = _routes(eng, B, meas, idx)
    res = {}
    for n in (1, 2):
        eng.set_streams(n)
        assert eng.batch_groups(B) == n
        res[n] = _run(eng, B, meas, 1, adj=True, angle_idx=idx)
        assert res[n][4] == (1, 1)
    eng.set_streams(-1)
    print('x-line operands, one stream against two: loss', repr(res[1][0]), repr(res[2][0]),
          ' wave, g_delta, g_beta identical:', [bool(np.array_equal(res[1][i], res[2][i])) for i in (1, 2, 3)])
    return B, routes, ref, res


def test_512_lookup_two_tiles_per_workgroup(lookup512):
    """Gradient rows, wave and loss of the 512-point lookup case (lookup512) by the module's rules."""
    B, (adj, stage1, two, twin), ref, _ = lookup512
    _check_routes('512 x 64 lookup, {} fields'.format(B), adj, stage1, two, twin, ref)


def test_512_lookup_one_and_two_streams(lookup512):
    """One sub-batch stream (two tiles per workgroup) and two (one tile per workgroup): detector waves and gradient rows bit for bit,
    and both bit for bit the fused-adjoint run that was held against the float64 twin."""
    adj, res = lookup512[1][0], lookup512[3]
    for i in (1, 2, 3):
        assert np.array_equal(res[1][i], res[2][i])
        assert np.array_equal(res[1][i], adj[i])
    assert res[1][0] == adj[0]


def test_512_lookup_one_and_two_streams_loss(lookup512):
    """The same two runs: the loss, bit for bit.  The loss is the sum of per-workgroup float64 partials (k_sum_partials over what
    the detector launches of each sub-batch leave, csrc/bdof_capi.hip).  With a grid balanced over the sub-batch, 129 fields split
    65 + 64 put other tiles in a partial than one launch of 129 does, and the loss differed in its last bit (0.0025011268538299106
    on one stream, 0.00250112685382991 on two, with waves and gradient rows identical; with the 17 fields of
    tests/test_gpu_fused_adjoint.py the two groupings happen to round alike).  bdof_loss_grad's detector launches now take one tile
    per workgroup where the batch's tiles fit the partial buffer (loss_grid): the partials are per tile, whatever the split."""
    res = lookup512[3]
    assert res[1][0] == res[2][0]


@pytest.mark.parametrize('X,B', [(64, 2 * NCU + 1), (128, 5), (256, 5)])
def test_one_pass_lengths_lookup(engine_mod, X, B):
    """The one-pass instances: 64-, 128- and 256-point x-lines with a lookup (8, 16 and 32 lookups per wave), 64 rows per field,
    S = 6 (a y-line kernel that is neither head nor last runs too).  At 64 points a tile is a whole field: 2 NCU + 1 fields on ONE
    sub-batch stream (the automatic split would halve them) put a second tile, of another angle, on every workgroup but one —
    asserted.  The table is 4 short of the line: the last x have no source row."""
    eng, idx, ref, meas = _table_case(engine_mod, 64, X, 6, B, 12, [2, 7, 9], 43 + X, vol_nx=X - 4)
    if X == 64:
        assert all(idx[b] != idx[b + (B + 1) // 2] for b in range(B // 2))    # the two tiles of a workgroup: (B + 1) / 2 fields apart
        _one_stream_two_tiles(eng, B, B * 64 // max(16, 4096 // X))
    else:
        eng.set_streams(1)
    adj, stage1, two, twin = _routes(eng, B, meas, idx)
    _check_routes('{} x 64 lookup, {} fields'.format(X, B), adj, stage1, two, twin, ref)


def test_volume_narrower_than_the_field_in_y(engine_mod):
    """The clamped yc path.  A plain batch cannot reach it: bdof_set_object refuses volNY != NY without a rotation table.  With a
    table it takes a volume of 40 rows' length under a field of 64, which is what runs here (512-point lines, S = 4, 3 fields of 3
    angles): y = 40 .. 63 are clamped in the load, their factors are exactly zero, so there the forward sweep leaves the wave
    unmodulated — the oracle's batch holds zeros there — and the gradient rows obey the factor-two rule."""
    Y, X, S, B = 64, 512, 4, 3
    eng, idx, ref, meas = _table_case(engine_mod, Y, X, S, B, 12, [1, 5, 10], 47, vol_ny=40)
    adj, stage1, two, twin = _routes(eng, B, meas, idx)
    _check_routes('512 x 64 lookup, volume 40 long in y', adj, stage1, two, twin, ref)


def test_no_state_between_calls(engine_mod):
    """One context, angle set A then angle set B: the second call's loss, wave and gradient rows are bit for bit those of a fresh
    context given B alone (nothing of a call's lookups outlives it)."""
    Y, X, S, B = 64, 512, 4, 3
    eng, idx_b, ref, meas = _table_case(engine_mod, Y, X, S, B, 12, [3, 8, 11], 53, vol_nx=500)
    first = _run(eng, B, meas, 1, adj=True, angle_idx=[1, 5, 10])
    second = _run(eng, B, meas, 1, adj=True, angle_idx=idx_b)
    fresh_eng, idx_f, _, meas_f = _table_case(engine_mod, Y, X, S, B, 12, [3, 8, 11], 53, vol_nx=500)
    assert idx_f == idx_b and np.array_equal(meas_f, meas)
    fresh = _run(fresh_eng, B, meas, 1, adj=True, angle_idx=idx_b)
    assert first[4] == second[4] == fresh[4] == (1, 1)
    assert first[0] != second[0]                                              # the angles do matter
    assert second[0] == fresh[0]
    for i in (1, 2, 3):
        assert np.array_equal(second[i], fresh[i])


def test_one_voxel_row_512(engine_mod):
    """tests/test_gpu_fused_adjoint.py's test_modulation_position at an odd slice with 512-point x-lines: an object that is zero but
    for ONE voxel row at (b0, x0, z0 = 3), 64 rows per field, S = 6.  What the row changes in the gradient rows of every slice, row
    by row, is what it changes in the float64 twin; the other wavefield sees nothing.  The blocked odd tape slots read back through
    bdof_tape_slot and un-blocked on the host equal the BLK = false route's bit for bit."""
    B, Y, X, S = 2, 64, 512, 6
    x0, b0, z0 = 341, 1, 3                                                    # x0 = 4 w + i + 32 pass + 64 m: w 5, i 1, pass 0, m 5
    rng = np.random.default_rng(59)
    eng, pr, pi = _engine(engine_mod, Y, X, S, B, rng)
    delta = np.zeros((B, Y, X, S))
    delta[b0, :, x0, z0] = rng.uniform(1e-2, 2e-2, size=Y).astype(np.float32)            # strong: k delta = 0.25 .. 0.5 rad in one slice
    beta = (0.1 * delta).astype(np.float32).astype(np.float64)
    meas = np.abs(1 + 0.05 * rng.normal(size=(B, Y, X))).astype(np.float32).astype(np.float64)
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
    print('x-line operands, one voxel row at 512 points: worst row error of the change in the gradient', worst)
    assert worst['two'] <= GRAD_TOL and worst['adj'] <= GRAD_TOL and worst['adj'] <= FACTOR * worst['two'], worst
