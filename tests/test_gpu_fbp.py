"""The analytic start on the device: bdof_backproject and bdof_ctf_retrieve through their own entry points against the float64
restatement of tests/fbp_reference.py, FullfieldSolver.analytic_volume for every rotation kind, and reconstruct_fullfield's
initial_guess='ctf-fbp'.

bdof_backproject's tolerance is derived per element, not measured.  With u = 2^-24 and, per element,
mag = sum_b |w_b| sum_taps weight |q| (the restatement returns it), the device rounds: the two factors of a tap's weight and their
product (3), the four-tap sum (4 fused multiply-adds on partial sums of at most the taps' magnitude sum), the product scale * w_b
(1), and the running sum over the B angles (B fused multiply-adds on partial sums of at most scale * mag):
    |device - reference| <= u (B + 8) scale mag + 1e-12 scale max|q| sum_b |w_b|
the last term for the float64 coordinates (a point within 1e-15 of a lattice line may take its taps from either side: the
interpolant is continuous) and the second-order terms.  bdof_ctf_retrieve: |device - reference| <= 2^-23 |reference| + 1e-10 max|reference|
(the float64 pipeline is rounded once)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fbp_reference as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -777.25
GUARD = 64
ENERGY, PSIZE = 5000., 1e-7


@pytest.fixture(scope='module')
def built():
    import __graft_entry__ as entry
    entry.build()


class Guarded(object):
    """A float32 device array between two sentinel-filled guards; download() checks the guards and returns the array."""

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


class Device(object):
    def __init__(self):
        from beyond_dof_amd import _lib
        self.ctx = _lib.Context(0)
        self.lib, self.h = self.ctx.lib, self.ctx.handle
        self.up = lambda a: _lib.DeviceBuffer.from_host(self.ctx, np.ascontiguousarray(a))

    def backproject(self, q, rows, w, vol_shape, start=None, row0=0, n_rows=None, accumulate=0, scale=(1., 1.)):
        """the volume [X][Z][Y][2] after one call; start: what it held before (sentinels if None)"""
        NX, NZ, NY = vol_shape
        B, NXd, NYd = q.shape
        vol = Guarded(self.ctx, np.full(tuple(vol_shape) + (2,), SENTINEL, dtype=np.float32) if start is None else start)
        dq, dr, dw = self.up(q.astype(np.float32)), self.up(np.asarray(rows, dtype=np.float64)), self.up(np.asarray(w, dtype=np.float32))
        self.ctx.check(self.lib.bdof_backproject(self.h, dq.ptr, NXd, NYd, dr.ptr, dw.ptr, B, vol.ptr, NX, NZ, NY, row0,
                                                 NX * NZ if n_rows is None else n_rows, accumulate, scale[0], scale[1]))
        self.ctx.sync()
        return vol.download()

    def retrieve(self, meas, wgt, a0_sq, filters):
        B, D, NX, NY = meas.shape
        q = Guarded(self.ctx, np.full((B, NX, NY), SENTINEL, dtype=np.float32))
        dm, df = self.up(meas.astype(np.float32)), self.up(filters.astype(np.complex128))
        dwgt = None if wgt is None else self.up(wgt.astype(np.float32))
        self.ctx.check(self.lib.bdof_ctf_retrieve(self.h, dm.ptr, None if dwgt is None else dwgt.ptr, a0_sq, df.ptr, B, D, NX, NY, q.ptr))
        self.ctx.sync()
        return q.download()


def backproject_bound(q, w, mag, scale, B):
    return 2.0 ** -24 * (B + 8) * scale * mag + 1e-12 * scale * np.abs(q).max() * np.abs(w).sum()


def assert_within(dev, want, bound, what):
    err = np.abs(dev.astype(np.float64) - want)
    worst = float((err / bound).max())
    print(what, 'largest |device - reference| / bound', worst)
    assert worst <= 1.0, what


# ---- bdof_backproject ------------------------------------------------------------------------------------------------------------
def test_backproject_exact_under_cube_rotations(built):
    """(NX, NZ, NY) = (8, 8, 6), integer frames of another size, the 24 cube rotations with integer offsets: bit for bit the
    integer sums, both channels (scale 1 and 0.5), taps outside the detector counting 0"""
    vol_shape, det_shape = (8, 8, 6), (7, 9)
    rng = np.random.default_rng(2)
    Ms = ref.cube_rotations()
    ts = [rng.integers(-2, 3, size=3).astype(np.float64) + (np.array(vol_shape) // 2 - np.rint(M @ (np.array([det_shape[0], vol_shape[1], det_shape[1]]) // 2)))
          for M in Ms]
    rows = np.stack([np.concatenate([M, t[:, None]], axis=1).reshape(12) for M, t in zip(Ms, ts)])
    q = rng.integers(-9, 10, size=(24,) + det_shape).astype(np.float64)
    want = ref.integer_backprojection(q, Ms, ts, vol_shape)
    assert np.any(want != 0)
    dev = Device()
    got = dev.backproject(q, rows, np.ones(24), vol_shape, scale=(1., 0.5))
    np.testing.assert_array_equal(got[..., 0], want.astype(np.float32))
    np.testing.assert_array_equal(got[..., 1], (0.5 * want).astype(np.float32))


def _general_case(vol_shape, det_shape, n_angles, seed):
    from beyond_dof_amd import util
    NX, NZ, NY = vol_shape
    rng = np.random.default_rng(seed)
    theta = np.sort(rng.uniform(0, 2 * np.pi, n_angles))
    rows = util.rigid_geometry(theta, (NY, NX, NZ), axis_tilt=0.3, axis_roll=0.1, center=(NX - 1) / 2. + 1.7,
                               shifts=rng.uniform(-1.5, 1.5, size=(n_angles, 2)))
    q = rng.normal(size=(n_angles,) + tuple(det_shape)).astype(np.float32).astype(np.float64)
    w = rng.uniform(0.1, 0.4, size=n_angles).astype(np.float32).astype(np.float64)
    return rows, q, w


@pytest.mark.parametrize('vol_shape,det_shape,n_angles', [((20, 12, 16), (23, 16), 7), ((64, 64, 64), (64, 64), 5)])
def test_backproject_against_restatement(built, vol_shape, det_shape, n_angles):
    """tilt 0.3, roll 0.1, the centre 1.7 pixels off, per-angle shifts: taps fall outside the detector and no symmetry hides an index
    mistake; 64^3 so that several workgroups and slabs take part.  Then the same bits slab-wise, in two host batches and repeated."""
    rows, q, w = _general_case(vol_shape, det_shape, n_angles, 7 + n_angles)
    NX, NZ, NY = vol_shape
    sd, sb = 10., 1.
    want, mag = ref.backproject(q, rows, w, vol_shape)
    if vol_shape[0] < 64:                                # the small case has taps outside the detector
        assert ref.backproject(np.ones_like(q), rows, w, vol_shape)[0].min() < 0.9 * w.sum()
    dev = Device()
    whole = dev.backproject(q, rows, w, vol_shape, scale=(sd, sb))
    assert_within(whole[..., 0], sd * want, backproject_bound(q, w, mag, sd, n_angles), 'delta {}'.format(vol_shape))
    assert_within(whole[..., 1], sb * want, backproject_bound(q, w, mag, sb, n_angles), 'beta {}'.format(vol_shape))
    # a repeated call
    np.testing.assert_array_equal(dev.backproject(q, rows, w, vol_shape, scale=(sd, sb)), whole)
    # slabs: rows outside a slab stay as they were, the slabs together are the whole volume
    edges = [0, 5, NX * NZ // 3 + 1, NX * NZ]
    vol = np.full(tuple(vol_shape) + (2,), SENTINEL, dtype=np.float32)
    for r0, r1 in zip(edges[:-1], edges[1:]):
        after = dev.backproject(q, rows, w, vol_shape, start=vol, row0=r0, n_rows=r1 - r0, scale=(sd, sb))
        flat_before, flat_after = vol.reshape(NX * NZ, NY, 2), after.reshape(NX * NZ, NY, 2)
        np.testing.assert_array_equal(flat_after[:r0], flat_before[:r0])
        np.testing.assert_array_equal(flat_after[r1:], flat_before[r1:])
        vol = after
    np.testing.assert_array_equal(vol, whole)
    # two host batches, the second accumulating: the sum of one call
    k = n_angles // 2 + 1
    first = dev.backproject(q[:k], rows[:k], w[:k], vol_shape, scale=(sd, sb))
    both = dev.backproject(q[k:], rows[k:], w[k:], vol_shape, start=first, accumulate=1, scale=(sd, sb))
    np.testing.assert_array_equal(both, whole)


def test_backproject_refusals(built):
    dev = Device()
    rows, q, w = _general_case((4, 4, 4), (4, 4), 2, 1)
    with pytest.raises(Exception, match='rows outside'):
        dev.backproject(q, rows, w, (4, 4, 4), row0=10, n_rows=8)


# ---- bdof_ctf_retrieve -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nx,ny', [(12, 10), (64, 48)])
@pytest.mark.parametrize('fp', [1e-3, (5e-4, 1e-3, 2e-3)])
def test_ctf_retrieve_against_restatement(built, nx, ny, fp):
    from beyond_dof_amd import analytic
    B = 5
    D = 3 if isinstance(fp, tuple) else 1
    rng = np.random.default_rng(nx + D)
    filters = analytic.ctf_filters(nx, ny, ENERGY, PSIZE, fp, 32, 10., 1e-2)
    meas = (1.3 * (1 + 0.05 * rng.normal(size=(B, D, nx, ny)))).astype(np.float32)
    dev = Device()
    got = dev.retrieve(meas, None, 1.3 ** 2, filters)
    want = ref.ctf_retrieve(meas, None, 1.3 ** 2, filters)
    bound = 2.0 ** -23 * np.abs(want) + 1e-10 * np.abs(want).max()
    assert_within(got, want, bound, 'ctf {}x{} D={}'.format(nx, ny, D))
    # weights: zero-weight pixels take no part, whatever they hold
    wgt = (rng.uniform(size=(nx, ny)) > 0.1).astype(np.float32)
    wgt[0, 0] = wgt[nx - 1, ny - 1] = 0
    zeros, nans = meas.copy(), meas.copy()
    zeros[..., wgt == 0] = 0
    nans[..., wgt == 0] = np.nan
    got_z, got_n = dev.retrieve(zeros, wgt, 1.3 ** 2, filters), dev.retrieve(nans, wgt, 1.3 ** 2, filters)
    assert np.all(np.isfinite(got_n))
    np.testing.assert_array_equal(got_n.view(np.uint32), got_z.view(np.uint32))
    want_w = ref.ctf_retrieve(nans, wgt, 1.3 ** 2, filters)
    assert_within(got_n, want_w, 2.0 ** -23 * np.abs(want_w) + 1e-10 * np.abs(want_w).max(), 'ctf weighted {}x{} D={}'.format(nx, ny, D))


# ---- FullfieldSolver.analytic_volume ---------------------------------------------------------------------------------------------
N, N_THETA, MB = 32, 24, 8


def _solver(rotation, fp=1e-3, **kw):
    from beyond_dof_amd.solver import FullfieldSolver
    theta = -np.linspace(0, 2 * np.pi, N_THETA)
    return FullfieldSolver(N, N, N, N_THETA, MB, ENERGY, PSIZE, free_prop_cm=fp, rotation=rotation, theta=theta, **kw)


def _analytic_correlation(rotation, fp=1e-3, **kw):
    d = ref.phantom(N, np.random.default_rng(0))
    s = _solver(rotation, fp, **kw)
    s.set_volume(d, 0.1 * d)
    prj = np.abs(s.forward_angles(np.arange(N_THETA)))
    s.set_volume(np.zeros_like(d), np.zeros_like(d))
    s.analytic_volume(prj)
    delta, beta = s.get_volume()
    assert delta.min() >= 0 and beta.min() >= 0 and np.all(np.isfinite(delta))
    assert np.abs(delta - 10 * beta).max() <= 1e-5 * delta.max()            # one sum, two scales
    corr = float(np.corrcoef(delta.ravel(), d.ravel())[0, 1])
    print('analytic_volume', rotation, fp, kw, 'delta correlation', corr)
    return corr, delta


CORR = {}


@pytest.mark.parametrize('name,rotation,kw', [('trilinear', 'trilinear', {}), ('trilinear_off', 'trilinear', dict(axis_tilt=0.2, center=17.0)),
                                              ('bilinear', 'bilinear', {}), ('nearest', 'nearest', {})])
def test_analytic_volume_every_rotation(built, name, rotation, kw):
    """data of the solver's own forward model at 32^3, 24 angles: an orientation or centre mistake in the rows of a rotation kind
    shows as a collapse of the correlation"""
    CORR[name], _ = _analytic_correlation(rotation, **kw)
    assert CORR[name] >= 0.97


def test_analytic_volume_three_planes(built):
    if 'nearest' not in CORR:
        CORR['nearest'], _ = _analytic_correlation('nearest')
    corr, _ = _analytic_correlation('nearest', fp=[5e-4, 1e-3, 2e-3])
    assert corr >= 0.97 and corr >= CORR['nearest'] - 0.01


def test_analytic_volume_mask_and_refusals(built):
    d = ref.phantom(N, np.random.default_rng(0))
    s = _solver('nearest')
    s.set_volume(d, 0.1 * d)
    prj = np.abs(s.forward_angles(np.arange(N_THETA)))
    mask = np.zeros((N, N, N), dtype=np.float32)
    mask[8:24, 8:24, 8:24] = 1
    s.set_mask(mask)
    s.analytic_volume(prj)
    delta, _ = s.get_volume()
    assert np.all(delta[mask == 0] == 0) and delta[mask == 1].max() > 1e-7
    with pytest.raises(ValueError, match='ctf_regularization'):
        s.analytic_volume(prj, ctf_regularization=0.)
    with pytest.raises(ValueError, match='all'):
        s.analytic_volume(prj[:5])
    # phase_only: delta alone
    s.set_mask(None)
    s.analytic_volume(prj, object_type='phase_only')
    delta, beta = s.get_volume()
    assert np.all(beta == 0) and delta.max() > 0


def test_analytic_volume_two_ranks_identical(built, tmp_path):
    """two gloo ranks on one GPU: every rank computes the whole volume from all angles — the single rank's bits on both"""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from test_gpu_dist import _launch_two
    procs = _launch_two('_fbp_dist_worker.py', tmp_path)
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=300)[0].decode())
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    assert all(p.returncode == 0 for p in procs), '\n'.join(o[-3000:] for o in outs)
    r0, r1 = [np.load(str(tmp_path / 'fbp_rank{}.npz'.format(r))) for r in range(2)]
    assert np.array_equal(r0['d'], r1['d']) and np.array_equal(r0['b'], r1['b'])
    import _fbp_dist_worker as w
    d, b = w.run(None)
    assert np.array_equal(r0['d'], d) and np.array_equal(r0['b'], b) and d.max() > 0


# ---- reconstruct_fullfield(initial_guess='ctf-fbp') ------------------------------------------------------------------------------
def test_entry_point_starts_lower_and_writes_summary(built, tmp_path):
    import contextlib
    import io
    import re
    from beyond_dof_amd import h5io
    from beyond_dof_amd.fullfield import reconstruct_fullfield, _read_mask
    d = ref.phantom(N, np.random.default_rng(0))
    s = _solver('nearest')
    s.set_volume(d, 0.1 * d)
    prj = s.forward_angles(np.arange(N_THETA))
    del s
    case = tmp_path / 'case'
    case.mkdir()
    h5io.write_dataset(str(case / 'data.h5'), 'exchange/data', prj.astype(np.complex64))
    cwd = os.getcwd()
    os.chdir(str(tmp_path))                          # (the lookup tables of rotation='nearest' are written to the working directory)
    try:
        losses = {}
        for name, guess, extra in (('zeros', [np.zeros_like(d), np.zeros_like(d)], {}),
                                   ('ctf-fbp', 'ctf-fbp', dict(delta_beta_ratio=10., ctf_regularization=1e-2, write_support_mask=3e-7))):
            out = io.StringIO()
            with contextlib.redirect_stdout(out):
                rd, rb = reconstruct_fullfield('data.h5', theta_st=0, theta_end=2 * np.pi, n_epochs=2, learning_rate=2e-8, minibatch_size=MB,
                                               energy_ev=ENERGY, psize_cm=PSIZE, free_prop_cm=1e-3, save_path=str(case), output_folder='out_' + name,
                                               shrink_cycle=None, seed=3, alpha_d=1e-9, alpha_b=1e-10, gamma=0, initial_guess=guess, **extra)
            losses[name] = float(re.findall(r'\(data term ([-+0-9.e]+)\)', out.getvalue())[-1])
            assert ('Initializing with CTF retrieval' in out.getvalue()) == (name == 'ctf-fbp')
        print('data term after 2 epochs:', losses)
        assert losses['ctf-fbp'] < losses['zeros']
        assert np.corrcoef(rd.ravel(), d.ravel())[0, 1] >= 0.97
        summary = open(str(case / 'out_ctf-fbp' / 'summary.txt')).read().split('\n')
        for line in (('initial_guess', 'ctf-fbp'), ('delta_beta_ratio', '10.0'), ('ctf_regularization', '0.01')):
            assert '{:<20}{}'.format(*line) in summary, line
        assert 'ctf_regularization' not in open(str(case / 'out_zeros' / 'summary.txt')).read()
        mask = _read_mask(str(case), N)
        assert mask is not None and mask.shape == (N, N, N) and 0 < mask.mean() < 0.5
    finally:
        os.chdir(cwd)


def _zero_start_run(root, tmp_path, name):
    out = str(tmp_path / (name + '.npz'))
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', '_fbp_bits_worker.py'), root, str(tmp_path / name), out],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode()[-3000:]
    return np.load(out)


def test_zero_start_keeps_the_parents_bits(built, tmp_path):
    """initial_guess=[zeros, zeros] through reconstruct_fullfield, rotation='nearest' and 'trilinear' (whose summary goes through the
    rewritten branch): delta, beta and summary.txt are those the commit before the analytic start gave — recorded from a build of
    that commit on an MI355X (tests/golden/g22_zero_start_parent.npz, by this test's own worker) and, where BDOF_PARENT_TREE names a
    built tree of it, run beside this one as well.  The comparison is of bits.  Should another ROCm or rocFFT version ever move
    them, record the file again with tests/_fbp_bits_worker.py from a build of that commit; do not loosen the comparison."""
    got = _zero_start_run(ROOT, tmp_path, 'this')
    refs = {'golden': np.load(os.path.join(ROOT, 'tests', 'golden', 'g22_zero_start_parent.npz'))}
    if os.environ.get('BDOF_PARENT_TREE'):
        refs['parent tree'] = _zero_start_run(os.environ['BDOF_PARENT_TREE'], tmp_path, 'parent')
    for name, want in refs.items():
        assert sorted(want.files) == sorted(got.files) == sorted(k + r for k in ('b_', 'd_', 'summary_') for r in ('nearest', 'trilinear'))
        for k in want.files:
            assert np.array_equal(got[k], want[k]), (name, k)
    assert got['d_nearest'].max() > 0 and got['d_trilinear'].max() > 0


def test_support_mask_is_for_the_next_run(built, tmp_path):
    """multiscale_level=2 with write_support_mask: the mask is written after the last level, so the finer level of the SAME run does
    not read it — the run has the bits of one that writes none — and it lies at the full resolution where the next run looks"""
    import contextlib
    import io
    from beyond_dof_amd import h5io
    from beyond_dof_amd.fullfield import reconstruct_fullfield, _read_mask
    from beyond_dof_amd.solver import FullfieldSolver
    n = 64
    d = ref.phantom(n, np.random.default_rng(0))
    s = FullfieldSolver(n, n, n, N_THETA, MB, ENERGY, PSIZE, free_prop_cm=1e-3)
    s.set_volume(d, 0.1 * d)
    prj = s.forward_angles(np.arange(N_THETA)).astype(np.complex64)
    del s
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        out = {}
        for name, extra in (('with', dict(write_support_mask=3e-7)), ('without', {})):
            os.makedirs(name)
            h5io.write_dataset(os.path.join(name, 'data.h5'), 'exchange/data', prj)
            with contextlib.redirect_stdout(io.StringIO()):
                out[name] = reconstruct_fullfield('data.h5', theta_st=0, theta_end=2 * np.pi, n_epochs=1, learning_rate=2e-8, minibatch_size=MB,
                                                  energy_ev=ENERGY, psize_cm=PSIZE, free_prop_cm=1e-3, save_path=name, output_folder='out',
                                                  shrink_cycle=None, seed=3, alpha_d=1e-9, alpha_b=1e-10, gamma=0, initial_guess='ctf-fbp',
                                                  multiscale_level=2, **extra)
        assert np.array_equal(out['with'][0], out['without'][0]) and np.array_equal(out['with'][1], out['without'][1])
        assert out['with'][0].shape == (n, n, n) and out['with'][0].max() > 1e-7
        mask = _read_mask('with', n)
        assert mask is not None and mask.shape == (n, n, n) and 0 < mask.mean() < 0.5
        assert _read_mask('without', n) is None
    finally:
        os.chdir(cwd)
