"""Where the y-line slice kernels (k_slice_y / k_slice_y_adj, csrc/bdof_kernels.h) get their rotation lookups from: in k_slice_y every
lane fetches the lookups of its own rows at the top of a tile (LineRows) and the pass loop forms the table row's address from the
value in hand; k_slice_y_adj looks its row up inside the pass.  The arithmetic is untouched, so what can go wrong is an operand: the
lookup of another pass, wave, tile or wavefield, or a stale one.  The cases aim there: every instance kind (FIRST, plain, TAIL, HEAD,
LAST), the first and last wave and pass of a tile, the second tile of a workgroup, every line length.

Rules, fixtures and helpers are tests/test_gpu_fused_adjoint.py's: against the float64 twin on the same context
(bdof_loss_grad_tf_f64), within tests/test_gpu_parity.py's bounds, the fused-adjoint route's gradient error at most FACTOR times the
two-kernel route's, loss and detector wave bit-identical between the fused-adjoint and the fused-forward route.  Figures are printed."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import bdof_oracle as orc
import test_gpu_fused_adjoint as fa
from test_gpu_fused_adjoint import engine_mod      # noqa: F401  (the module-scoped fixture)

LOSS_TOL, GRAD_TOL, FACTOR = fa.LOSS_TOL, fa.GRAD_TOL, fa.FACTOR


def _bind_volume(eng, od, S, tab, n_theta):
    """Bind a (Y, X, Z) delta volume (beta = delta / 10) behind the rotation table; returns the [X Z][Y][2] float32 rows."""
    from beyond_dof_amd import util, _lib
    ny, nx = od.shape[0], od.shape[1]
    rows = util.volume_to_rows(od, (0.1 * od).astype(np.float32))
    eng.set_volume(_lib.DeviceBuffer.from_host(eng.ctx, rows), nx * S, ny, _lib.DeviceBuffer.from_host(eng.ctx, tab), nx, n_theta)
    return rows.reshape(nx * S, ny, 2)


def _four_routes(eng, B, meas, idx, stage1=True):
    eng.enable_tf_f64()
    out = {'twin': fa._run(eng, B, meas, 0, angle_idx=idx, f64=True), 'two': fa._run(eng, B, meas, 0, angle_idx=idx)}
    if stage1:
        out['stage1'] = fa._run(eng, B, meas, 1, angle_idx=idx)
    out['adj'] = fa._run(eng, B, meas, 1, adj=True, angle_idx=idx)
    assert out['two'][4] == (0, 0) and out['adj'][4] == (1, 1)
    if stage1:
        assert out['stage1'][4] == (1, 0)
        assert out['adj'][0] == out['stage1'][0] and np.array_equal(out['adj'][1], out['stage1'][1])      # forward results: bit for bit
    return out


def _change_errors(name, row, empty, target, unread, also=None):
    """test_modulation_position's rule for the change one voxel row makes.  target: a (b, x, z) the twin must see change; unread:
    wavefields whose angle never reads the row — the twin sees exactly nothing there.  Returns the worst row errors."""
    dt = np.stack([row['twin'][2] - empty['twin'][2], row['twin'][3] - empty['twin'][3]])           # [2][b][y][x][z]
    scale = np.sqrt((dt ** 2).sum(axis=(0, 2)))                                                      # per (b, x, z) row
    assert scale[target] > 0 and (also is None or scale[also] > 0)
    for b in unread:
        assert np.all(scale[b] == 0)
    worst = {}
    for m in ('two', 'adj'):
        dm = np.stack([row[m][2] - empty[m][2], row[m][3] - empty[m][3]]).astype(np.float64)
        err = np.sqrt(((dm - dt) ** 2).sum(axis=(0, 2)))
        worst[m] = float((err / scale.max()).max())                                                  # all rows of all wavefields
        dl, dl64 = row[m][0] - empty[m][0], row['twin'][0] - empty['twin'][0]
        # each loss lies within LOSS_TOL of its twin, so the change lies within twice that of the twin's change
        assert abs(dl - dl64) <= 2 * LOSS_TOL * abs(row['twin'][0]), (name, m, dl, dl64)
    print('y-line lookups', name, ': worst row error of the change in the gradient', worst)
    assert worst['two'] <= GRAD_TOL and worst['adj'] <= GRAD_TOL and worst['adj'] <= FACTOR * worst['two'], (name, worst)
    return worst


# ---- right row, every position a lookup can be hoisted wrongly from ----------------------------------------------------------------
N64, S64, NTHETA = 64, 6, 12
IDX64 = [10, 1, 5, 10]          # unsorted, 3 of 12 angles, one of them twice


@pytest.fixture(scope='module')
def table64(engine_mod):
    """64^2, S = 6, 4 wavefields at 3 of 12 angles: engine, table, measurement and the four routes of the EMPTY volume, computed once."""
    from beyond_dof_amd import util
    rng = np.random.default_rng(71)
    B = len(IDX64)
    eng, pr, pi = fa._engine(engine_mod, N64, N64, S64, B, rng)
    tab, _, _ = util.device_rotation_tables(orc.rotation_lookup([N64, N64, S64], NTHETA), N64, S64)
    meas = np.abs(1 + 0.05 * rng.normal(size=(B, N64, N64))).astype(np.float32).astype(np.float64)
    _bind_volume(eng, np.zeros((N64, N64, S64), dtype=np.float32), S64, tab, NTHETA)
    empty = _four_routes(eng, B, meas, IDX64)
    return eng, tab, meas, empty, rng


# (z0, x of the reading wavefield row, its wavefield).  At 64 points a tile is one wavefield in one pass (pass 0 is the last pass) and
# wave w holds rows 8 w .. 8 w + 7: x <= 7 is the first wave, x >= 56 the last.  S = 6: z = 0 runs k_slice_y<FIRST> and
# k_slice_y_adj<LAST>, z = 2 the plain instances, z = 4 k_slice_y<TAIL> and k_slice_y_adj<HEAD>.
@pytest.mark.parametrize('z0,xt,bt', [(0, 3, 3), (0, 60, 1), (2, 5, 1), (2, 58, 3), (4, 0, 2), (4, 63, 0)])
def test_one_voxel_row_through_the_table(table64, z0, xt, bt):
    """A volume that is zero but for ONE voxel row: the one wavefield row (bt, xt, z0) reads through the table.  What it changes in the
    loss and in the gradient rows of every slice, row by row and wavefield by wavefield, is what it changes in the float64 twin; a
    wavefield whose angle reads the row nowhere sees nothing.  Wavefields 0 and 3 share an angle: one detector wave, bit for bit."""
    eng, tab, meas, empty, rng = table64
    B = len(IDX64)
    s = int(tab[IDX64[bt], z0, xt])
    assert s >= 0
    xs, zs = divmod(s, S64)
    od = np.zeros((N64, N64, S64), dtype=np.float32)
    od[:, xs, zs] = rng.uniform(1e-2, 2e-2, size=N64).astype(np.float32)       # strong: k delta = 0.25 .. 0.5 rad in one slice
    flat = _bind_volume(eng, od, S64, tab, NTHETA)
    assert np.count_nonzero(flat[:, :, 0].any(axis=1)) == 1 and flat[s, :, 0].all()
    row = _four_routes(eng, B, meas, IDX64)
    unread = [b for b in range(B) if not np.any(tab[IDX64[b]] == s)]
    _change_errors('64^2 z {} x {} b {}'.format(z0, xt, bt), row, empty, (bt, xt, z0), unread)
    assert np.array_equal(row['adj'][1][0], row['adj'][1][3])                  # the angle that occurs twice: one detector wave


# ---- second tile of a workgroup ---------------------------------------------------------------------------------------------------
def test_second_tile_of_a_workgroup_512(engine_mod):
    """512^2, S = 4, 17 wavefields through the table: 544 tiles of 16 rows on 512 workgroup slots, so on one sub-batch stream the grid
    is 272 workgroups of two tiles, tile t and tile t + 272 — 8.5 wavefields apart.  Two voxel rows are perturbed.  One is what
    wavefield row (12, 300, 2) reads: tile 402, the second tile of the workgroup whose first is tile 130 of wavefield 4, at another
    angle (asserted); row 12 of its tile, so pass 1, wave 4, a plain instance.  The other is what (14, 320, 0) reads: tile 468 behind
    tile 196 of wavefield 6, row 0 of its tile, so pass 0, wave 0, in k_slice_y<FIRST> and k_slice_y_adj<LAST>.  A lookup kept from
    the first tile, or taken from the other pass, would put the change elsewhere.  One stream, two streams and a repeated call: bit
    for bit."""
    from beyond_dof_amd import util
    n, S, B, n_theta = 512, 4, 17, NTHETA
    bt, xt, z0 = 12, 300, 2
    idx = [(1, 5, 10)[b % 3] for b in range(B)]
    bu, xu, zu = 14, 320, 0
    for (b_, x_), first in (((bt, xt), 4), ((bu, xu), 6)):
        t1 = (b_ * n + x_) // 16 - 272
        assert t1 >= 0 and idx[t1 * 16 // n] != idx[b_] and t1 * 16 // n == first
    assert xt % 16 >= 8 and xu % 16 == 0                                       # pass 1; pass 0, first wave
    rng = np.random.default_rng(73)
    eng, pr, pi = fa._engine(engine_mod, n, n, S, B, rng)
    tab, _, _ = util.device_rotation_tables(orc.rotation_lookup([n, n, S], n_theta), n, S)
    meas = np.abs(1 + 0.05 * rng.normal(size=(B, n, n))).astype(np.float32).astype(np.float64)
    eng.set_streams(1)
    assert eng.batch_groups(B) == 1
    _bind_volume(eng, np.zeros((n, n, S), dtype=np.float32), S, tab, n_theta)
    empty = _four_routes(eng, B, meas, idx, stage1=False)
    s = int(tab[idx[bt], z0, xt])
    assert s >= 0 and s != int(tab[idx[4], z0, xt])                            # the first tile's angle reads another row there
    s2 = int(tab[idx[bu], zu, xu])
    assert s2 >= 0 and s2 != s and s2 != int(tab[idx[6], zu, xu])
    od = np.zeros((n, n, S), dtype=np.float32)
    for src in (s, s2):
        xs, zs = divmod(src, S)
        od[:, xs, zs] = rng.uniform(1e-2, 2e-2, size=n).astype(np.float32)
    _bind_volume(eng, od, S, tab, n_theta)
    row = _four_routes(eng, B, meas, idx, stage1=False)
    unread = [b for b in range(B) if not np.any((tab[idx[b]] == s) | (tab[idx[b]] == s2))]
    _change_errors('512^2 x 17, second tile', row, empty, (bt, xt, z0), unread, also=(bu, xu, zu))
    again = fa._run(eng, B, meas, 1, adj=True, angle_idx=idx)                  # a repeated call
    eng.set_streams(2)
    assert eng.batch_groups(B) == 2
    two_streams = fa._run(eng, B, meas, 1, adj=True, angle_idx=idx)
    eng.set_streams(-1)
    for other in (again, two_streams):
        assert other[4] == (1, 1) and other[0] == row['adj'][0]
        for i in (1, 2, 3):
            assert np.array_equal(other[i], row['adj'][i])


# ---- every line length and both tile shapes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('Y,X', [(64, 128), (128, 64), (256, 64), (64, 256)])
def test_every_line_length_plain_batch(engine_mod, Y, X):
    """NX != NY, S = 4, 2 wavefields, plain batch (no table: the lookup is arithmetic on x): y-lines of 64, 128 and 256 points, a row
    on 8, 16 and 32 lanes, so a wave fetches 8, 4 and 2 lookups; tiles of 64, 32 and 16 rows.  Gradient rows against the float64 twin
    under test_gpu_fused_adjoint.py's bound and ratio rule; loss and detector wave bit-identical between the fused-adjoint and the
    fused-forward route (fa._check_routes asserts both)."""
    fa._accuracy(engine_mod, 'y-line lookups {}x{}'.format(Y, X), 2, Y, X, 4, 79)


# ---- table against a plain batch --------------------------------------------------------------------------------------------------
def test_table_against_plain_batch(engine_mod):
    """The 64^2 case (S = 6, angles 10, 1, 5, 10 of 12) once through the lookup table and once as set_object_batch of the rows
    gathered on the host with the same table: the same wavefield rows meet the same table entries.  The mean modulation factor that
    rides on the carrier is formed over what is bound — the volume's 384 rows in one binding, the batch's 1536 gathered rows (border
    rows clamped, hence some repeated, one angle twice) in the other.  If the two means are equal the carrier scalars are, and loss
    and gradient rows must have equal bits.  They are NOT equal for this data (the branch that runs is printed), so the float32 sweeps
    round differently and the twin's bound applies instead: the twins of the two bindings agree to float64 rounding, and each
    binding's routes are held to the module's rules against the plain batch's twin."""
    from beyond_dof_amd import util
    rng = np.random.default_rng(83)
    B = len(IDX64)
    eng, pr, pi = fa._engine(engine_mod, N64, N64, S64, B, rng)
    tab, _, _ = util.device_rotation_tables(orc.rotation_lookup([N64, N64, S64], NTHETA), N64, S64)
    od = rng.uniform(0, 2e-5, size=(N64, N64, S64)).astype(np.float32)
    flat = _bind_volume(eng, od, S64, tab, NTHETA).astype(np.float64)
    mean_t = eng.modulation_table()[1]
    delta, beta = util.rows_to_batch(np.stack([flat[tab[a]] for a in IDX64]))          # [b][z][x][y][2] -> (B, Y, X, S)
    p64 = (pr + 1j * pi).astype(np.complex64)
    ref, _ = orc.multislice_propagate_batch_numpy(delta, beta, p64.real.astype(np.float64), p64.imag.astype(np.float64), fa.E_EV, fa.PSIZE,
                                                  fa.FP, delta.shape, return_probe_array=False)
    meas = (np.abs(ref) * (1 + 0.05 * rng.normal(size=ref.shape))).astype(np.float32).astype(np.float64)
    t = _four_routes(eng, B, meas, IDX64)
    eng.set_object_batch(delta, beta)
    mean_p = eng.modulation_table()[1]
    p = _four_routes(eng, B, meas, None)
    same = mean_t == mean_p
    print('y-line lookups, table against plain batch: mean c - 1', mean_t, mean_p, '-> equal bits required' if same else '-> twin bound')
    if same:
        assert t['adj'][0] == p['adj'][0]
        for i in (2, 3):
            assert np.array_equal(t['adj'][i], p['adj'][i])
    else:
        g64 = np.stack([p['twin'][2], p['twin'][3]])
        assert fa.rel(np.stack([t['twin'][2], t['twin'][3]]), g64) <= 1e-9 and abs(t['twin'][0] - p['twin'][0]) <= 1e-12 * abs(p['twin'][0])
        for name, r in (('table', t), ('plain', p)):
            fa._check_routes('y-line lookups 64^2 ' + name, r['adj'], r['stage1'], r['two'], p['twin'], ref)
