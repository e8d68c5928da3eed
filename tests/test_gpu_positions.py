"""Sub-pixel probe positions through PtychoSolver and reconstruct_ptychography (position_offsets, refine_positions).

Parity: object, probe (32^2) and the 9 positions of rigid_reference.ptycho_problem with offsets U(-0.9, 0.9), under
rotation='nearest' and 'trilinear', on the resident and the generic engine, against the float64 restatement of
tests/positions_reference.py: loss to LOSS_BOUND, volume gradient to GRADIENT_BOUND, every entry of position_gradient() to
GRADIENT_BOUND of the sum of the absolute values of its terms.  Zero offsets give the loss of the index-math path bit for bit.
With neither keyword nothing new runs.  Recovery: data simulated by the solver's own forward at true offsets U(-0.8, 0.8), the
true volume held still, 100 steps at position_learning_rate 0.05: every position within one tenth of the largest initial error."""
import os

import numpy as np
import pytest

import positions_reference as pr
import rigid_reference as rr

pytestmark = pytest.mark.gpu

PSZ = pr.PSZ
N_POS = len(rr.PTY_POS)
IDX = np.arange(N_POS)


@pytest.fixture(scope='module')
def built():
    import __graft_entry__ as entry
    entry.build()


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b))


def solver(kind, engine, **kw):
    from beyond_dof_amd.solver import PtychoSolver
    p = rr.ptycho_problem(PSZ)
    geo = dict(rotation='trilinear', theta=rr.ptycho_theta(), axis_tilt=rr.PTY_TILT) if kind == 'trilinear' else {}
    s = PtychoSolver(rr.PTY_SHAPE, (PSZ, PSZ), rr.PTY_POS, rr.PTY_N_THETA, N_POS, rr.E_EV, rr.PSIZE_CM, p['pr'], p['pi'], engine=engine,
                     **dict(geo, **kw))
    s.set_volume(p['od'], p['ob'])
    return s


@pytest.mark.parametrize('engine', ['resident', 'generic'])
@pytest.mark.parametrize('kind', ['nearest', 'trilinear'])
def test_parity_at_fractional_positions(built, kind, engine):
    ref = pr.solver_problem(kind)
    s = solver(kind, engine, position_offsets=ref['off'])
    loss = s.loss_and_grad(rr.PTY_THETA, IDX, ref['meas'])
    gd, gb = s.gradient_to_host()
    dpos = s.position_gradient()
    figures = (abs(loss - ref['loss']) / ref['loss'], rel(gd, ref['gd']), rel(gb, ref['gb']))
    ratio = np.abs(dpos - ref['dpos']) / ref['T']
    print(kind, engine, 'loss', loss, 'reference', ref['loss'], 'relative', figures[0], 'g_delta', figures[1], 'g_beta', figures[2],
          'position gradient: largest |device - reference| / sum |terms|', float(ratio.max()), 'bounds', pr.LOSS_BOUND, pr.GRADIENT_BOUND)
    assert np.array_equal(s.position_gradient(), dpos)
    assert np.array_equal(s.positions(), np.broadcast_to(ref['off'], (rr.PTY_N_THETA, N_POS, 2)))
    assert figures[0] <= pr.LOSS_BOUND
    assert figures[1] <= pr.GRADIENT_BOUND and figures[2] <= pr.GRADIENT_BOUND
    assert float(ratio.max()) <= pr.GRADIENT_BOUND
    # the detector waves of forward() come down the same path
    wave = s.forward(rr.PTY_THETA, IDX)
    assert rel(np.abs(wave), np.abs(ref['wave'])) <= 1e-5


@pytest.mark.parametrize('kind', ['nearest', 'trilinear'])
def test_zero_offsets_give_the_loss_of_the_index_math_path(built, kind):
    ref = pr.solver_problem(kind, zero=True)
    plain, zero = solver(kind, None), solver(kind, None, position_offsets=np.zeros((N_POS, 2)))
    a = plain.loss_and_grad(rr.PTY_THETA, IDX, ref['meas'])
    b = zero.loss_and_grad(rr.PTY_THETA, IDX, ref['meas'])
    ga, gb = plain.gradient_to_host(), zero.gradient_to_host()
    print(kind, 'loss', a, b, 'reference', ref['loss'], 'gradient: same bits', np.array_equal(ga[0], gb[0]) and np.array_equal(ga[1], gb[1]),
          'g_delta', rel(gb[0], ref['gd']), 'g_beta', rel(gb[1], ref['gb']))
    assert a == b
    assert rel(gb[0], ref['gd']) <= pr.GRADIENT_BOUND and rel(gb[1], ref['gb']) <= pr.GRADIENT_BOUND
    with pytest.raises(ValueError, match='position_offsets'):
        plain.positions()


def test_without_the_keywords_nothing_new_runs(built):
    """neither keyword, and both given as None: no stack is allocated, two steps leave the same volume bit for bit — and it is not the
    volume of a solver that refines; the entry point refuses gradient accumulation while refining"""
    from beyond_dof_amd.ptychography import reconstruct_ptychography
    ref = pr.solver_problem('nearest')
    vols = []
    for kw in ({}, dict(position_offsets=None, refine_positions=None), dict(refine_positions='per_angle')):
        s = solver('nearest', None, **kw)
        assert (s.pos is None) == ('refine_positions' not in kw or kw['refine_positions'] is None) and hasattr(s, 'stack') == (s.pos is not None)
        s.reset_moments()
        for i in range(2):
            s.step(i, rr.PTY_THETA, IDX, ref['meas'], 1e-8)
        vols.append(s.get_volume())
        if s.pos is not None:
            moved = np.any(s.positions() != 0, axis=(1, 2))
            assert np.array_equal(np.nonzero(moved)[0], [rr.PTY_THETA])           # only the step's angle
    assert np.array_equal(vols[0][0], vols[1][0]) and np.array_equal(vols[0][1], vols[1][1])
    assert not np.array_equal(vols[0][0], vols[2][0])
    with pytest.raises(ValueError, match='n_batch_per_update'):
        reconstruct_ptychography('nothing.h5', rr.PTY_POS, (PSZ, PSZ), rr.PTY_SHAPE, refine_positions='shared', n_batch_per_update=2)


# ---- recovery ----------------------------------------------------------------------------------------------------------------------------
R_SHAPE, R_PSZ, STEPS = (32, 32, 16), 16, 100
R_POS = np.array([(y, x) for y in (8, 16, 24) for x in (8, 16, 24)])


def _blobs():
    """12 gaussian blobs of unequal weight and width, zero near the faces"""
    rng = np.random.default_rng(12)
    y, x, z = np.meshgrid(np.arange(32), np.arange(32), np.arange(16), indexing='ij')
    od = np.zeros(R_SHAPE)
    for _ in range(12):
        cy, cx, cz = rng.uniform(5, 27), rng.uniform(5, 27), rng.uniform(3, 13)
        w, a = rng.uniform(1.5, 3.0), rng.uniform(1e-4, 4e-4)
        od += a * np.exp(-((y - cy) ** 2 + (x - cx) ** 2 + (z - cz) ** 2) / (2 * w ** 2))
    od[od < 1e-6] = 0.
    return od, 0.1 * od


def _recovery_solver(od, ob, **kw):
    from beyond_dof_amd import util
    from beyond_dof_amd.solver import PtychoSolver
    probe = util.gaussian_probe((R_PSZ, R_PSZ), 4., 4., 0.5)
    s = PtychoSolver(R_SHAPE, (R_PSZ, R_PSZ), R_POS, 2, len(R_POS), rr.E_EV, rr.PSIZE_CM, probe[0], probe[1], **kw)
    s.set_volume(od, ob)
    return s


@pytest.mark.parametrize('mode', ['per_angle', 'shared'])
def test_refinement_recovers_the_positions(built, mode):
    od, ob = _blobs()
    rng = np.random.default_rng(5)
    true = rng.uniform(-0.8, 0.8, size=(len(R_POS), 2) if mode == 'shared' else (2, len(R_POS), 2))
    idx = np.arange(len(R_POS))
    sim = _recovery_solver(od, ob, position_offsets=true)
    data = np.stack([np.abs(sim.forward(t, idx)) for t in range(2)])
    s = _recovery_solver(od, ob, refine_positions=mode, position_learning_rate=0.05)
    s.set_measurements(data)
    s.reset_moments()
    full = np.broadcast_to(true, (2, len(R_POS), 2))
    worst = lambda: float(np.sqrt(np.sum((s.positions() - full) ** 2, axis=-1)).max())
    start = worst()
    first = s.step(0, 0, idx, None, 0.0, want_loss=True)
    for i in range(1, STEPS):
        s.step(i, i % 2, idx, None, 0.0)
        if i + 1 in (25, 50):
            print(mode, 'after', i + 1, 'steps: largest position error', worst())
    last = s.loss_and_grad(1, idx)
    print(mode, 'largest position error', start, '->', worst(), 'after', STEPS, 'steps; loss', first, '->', last)
    d, b = s.get_volume()
    assert np.array_equal(d, od.astype(np.float32)) and np.array_equal(b, ob.astype(np.float32))           # the volume stood still
    assert worst() <= start / 10.


def test_reconstruct_ptychography_refines_records_and_carries_the_positions(built, tmp_path, monkeypatch):
    """the entry point over two multiscale levels: the fine level starts from the coarse level's offsets in its own units,
    positions.npy holds the offsets in full-resolution pixels and summary.txt the refined_positions line"""
    from beyond_dof_amd import h5io, ptychography
    monkeypatch.chdir(tmp_path)
    od, ob = _blobs()
    rng = np.random.default_rng(8)
    true = rng.uniform(-0.8, 0.8, size=(len(R_POS), 2))
    idx = np.arange(len(R_POS))
    sim = _recovery_solver(od, ob, position_offsets=true)
    data = np.stack([sim.forward(t, idx) for t in range(2)])
    os.makedirs('case')
    h5io.write_dataset('case/data.h5', 'exchange/data', np.abs(data).astype(np.complex64))
    built_with, solvers = [], []
    real = ptychography.PtychoSolver

    def recording(*args, **kw):
        built_with.append(np.array(kw['position_offsets']))
        solvers.append(real(*args, **kw))
        return solvers[-1]
    monkeypatch.setattr(ptychography, 'PtychoSolver', recording)
    ptychography.reconstruct_ptychography('data.h5', R_POS, (R_PSZ, R_PSZ), R_SHAPE, n_epochs=10, learning_rate=0., minibatch_size=len(R_POS),
                                          energy_ev=rr.E_EV, psize_cm=rr.PSIZE_CM, save_path='case', output_folder='out', multiscale_level=2,
                                          initial_guess=[od[::2, ::2, ::2], ob[::2, ::2, ::2]], seed=1, probe_mag_sigma=4., probe_phase_sigma=4.,
                                          probe_phase_max=0.5, refine_positions='shared', position_learning_rate=0.05)
    rec = np.load(os.path.join('case', 'out', 'positions.npy'))
    assert rec.shape == (2, len(R_POS), 2) and len(built_with) == 2
    assert not np.any(built_with[0]) and np.any(built_with[1])
    assert np.array_equal(built_with[1], solvers[0].positions() * 2)          # coarse pixels -> full-resolution pixels
    assert np.array_equal(rec, solvers[1].positions()) and not np.array_equal(rec, built_with[1])
    text = open(os.path.join('case', 'out', 'summary.txt')).read()
    print(text.splitlines()[-1])
    assert 'refined_positions' in text and 'largest move' in text
