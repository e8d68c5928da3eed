"""Gradient parity at 2e-5: every adjoint path of the transfer-function model on the device against the float64 reference of
tests/reference_model.py, at data that does not cancel in the seed (reference_model.measurement_wide).

The cases, their inputs and their bounds are tests/gradient_cases.py's; tests/test_gradient_conditioning.py shows without a GPU
that a plain complex64 restatement stays below half of every bound used here, and that adjoint mistakes of 5e-5 to 2e-4 — which
the 2e-4 of the other files lets through — exceed it.  Every case does the same: object and probe as the device holds them, the
float64 reference, wide amplitudes on the reference's detector wave, ONE loss_grad; it asserts the loss to 1e-5, g_delta and
g_beta (and the probe gradient where the case has one) to the case's bound, and that the route the case names is the one that
ran.  The figures are printed before they are asserted (MEASUREMENTS.md)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import gradient_cases as gc

E, PS = gc.E, gc.PS


@pytest.fixture(scope='module')
def engine_mod():
    import __graft_entry__ as entry
    entry.build()
    from beyond_dof_amd import engine
    return engine


def _check(tag, c, e):
    print('tight gradient', tag, 'loss / g_delta / g_beta (/ g_probe) rel err', e, 'bound', c['bound'])
    assert e[0] <= gc.LOSS_BOUND, (tag, e)
    assert max(e[1:]) <= c['bound'], (tag, e, c['bound'])


def _run(engine_mod, c):
    p = gc.problem(c)
    B, Y, X, S = c['B'], c['Y'], c['X'], c['S']
    eng = engine_mod.MultisliceEngine(Y, X, S, B, with_grad=True, engine=c['engine'], recompute=c.get('recompute', False),
                                      adjoint64=c.get('adjoint64', False), slice_binning=c.get('b', 1))
    eng.set_physics(E, PS, gc._fp(c), variant=c['variant'])
    eng.set_probe(p['pr'], p['pi'])
    # the far field's gaussian probe rides on a carrier field, the structured plane wave on a scalar
    assert eng.probe_stack == (c['fp'] == 'inf')
    if 'loss' in c:
        eng.set_loss(c['loss'], gc.MU)
    if p['w'] is not None:
        eng.set_detector_weights(p['w'])
    if c.get('probe_grad'):
        eng.enable_probe_grad(True)
    eng.set_object_batch(p['delta32'], p['beta32'])
    if c.get('fused'):
        eng.set_sweep_fusion(1)
        eng.set_adjoint_fusion(True)
    if 'streams' in c:
        eng.set_streams(c['streams'])
        assert eng.batch_groups(B) == c['streams']
    loss = eng.loss_grad(B, p['meas'])
    # the route: the engine is pinned by name; of the streaming engine's sweeps the library says which ran
    assert (eng.sweep_fused, eng.adjoint_fused) == ((1, 1) if c.get('fused') else (0, 0)), (eng.sweep_fused, eng.adjoint_fused)
    assert eng.recompute == bool(c.get('recompute')) and eng.adjoint64 == bool(c.get('adjoint64')) and eng.n_steps == S // c.get('b', 1)
    assert eng.n_planes == (len(c['fp']) if isinstance(c['fp'], tuple) else 1)
    if c['regime'] == 'weak' and c['fp'] != 'inf':
        assert eng.meas_ref > 0                     # wide data keeps the residual split (test_wide_data_keeps_the_residual_split)
    gd, gb = eng.grad_batch_to_host(B)
    gp = eng.probe_grad() if c.get('probe_grad') else None
    _check(gc.case_id(c), c, gc.errors(c, p, loss, gd, gb, gp))


def _of(*paths):
    return [c for c in gc.CASES if c['path'] in paths]


@pytest.mark.parametrize('c', _of('two-kernel'), ids=gc.case_id)
def test_streaming_two_kernel_route(engine_mod, c):
    """k_row_fwd, k_row_loss, k_row_bwd: every line length and both orientations, the three detectors, both variants, three
    regimes, and 70 steps (the dithered copies of every constant wrap at 64)."""
    _run(engine_mod, c)


@pytest.mark.parametrize('c', _of('fused'), ids=gc.case_id)
def test_fused_sweep_and_fused_adjoint(engine_mod, c):
    """k_slice_* and k_slice_*_adj on the blocked phi tape."""
    _run(engine_mod, c)


@pytest.mark.parametrize('c', _of('tape-free'), ids=gc.case_id)
def test_tape_free_adjoint(engine_mod, c):
    """recompute=True: the marched-back wave divided by c."""
    _run(engine_mod, c)


@pytest.mark.parametrize('c', _of('resident'), ids=gc.case_id)
def test_resident_engine(engine_mod, c):
    """EpiMod, EpiBwd, ResPoint of the LDS-resident kernel."""
    _run(engine_mod, c)


@pytest.mark.parametrize('c', _of('generic', 'generic-adjoint64'), ids=gc.case_id)
def test_generic_engine(engine_mod, c):
    """k_g_modulate / k_g_bwd, and k_g_bwd64 under adjoint64."""
    _run(engine_mod, c)


@pytest.mark.parametrize('c', _of('streams'), ids=gc.case_id)
def test_sub_batch_streams(engine_mod, c):
    """7 wavefields split over two streams, against the reference rather than against the one-stream run."""
    _run(engine_mod, c)


@pytest.mark.parametrize('c', _of('binning', 'planes', 'weights', 'poisson', 'probe-gradient'), ids=gc.case_id)
def test_model_options(engine_mod, c):
    """Slice binning, two detector planes, detector weights (the reference's seed is the weighted one), the Poisson term, and
    bdof_probe_grad against G(psi_0) summed over the batch."""
    _run(engine_mod, c)


# ---- the solver level ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', [c for c in gc.SOLVER_CASES if c['path'] == 'fullfield-solver'], ids=gc.solver_id)
def test_fullfield_solver(engine_mod, c):
    """64^3, three angles through the rotation tables, near-field detector, against reference_model.fullfield_loss_and_grad."""
    from beyond_dof_amd.solver import FullfieldSolver
    p = gc.solver_problem(c)
    n, idx = gc.N, p['idx']
    prj = np.zeros((gc.N_THETA, n, n))
    prj[idx] = p['meas']
    s = FullfieldSolver(n, n, n, gc.N_THETA, len(idx), E, PS, free_prop_cm=p['fp'], coord_ls=p['coords'])
    s.set_volume(p['delta32'], p['beta32'])
    s.set_measurements(prj)
    loss = s.loss_and_grad(idx)
    assert (s.sweep_fused, s.adjoint_fused) == (1, 1)               # the solver's own choice of route
    gd, gb = s.gradient_to_host()
    _check(gc.solver_id(c), c, (float(abs(loss - p['loss']) / abs(p['loss'])), float(gc.rel(gd, p['gd'])), float(gc.rel(gb, p['gb']))))


@pytest.mark.parametrize('c', [c for c in gc.SOLVER_CASES if c['path'] == 'ptycho-solver'], ids=gc.solver_id)
def test_ptycho_solver(engine_mod, c):
    """64^3, a 64-pixel probe at four positions (three windows hang over the volume's edge), far field, against
    reference_model.ptycho_loss_and_grad; the wide amplitudes sit on the reference's detector waves."""
    from beyond_dof_amd.solver import PtychoSolver
    p = gc.solver_problem(c)
    n = gc.N
    s = PtychoSolver((n, n, n), p['psz'], gc.PTY_POS, gc.N_THETA, len(gc.PTY_POS), E, PS, p['pr'], p['pi'], coord_ls=p['coords'])
    s.set_volume(p['delta32'], p['beta32'])
    loss = s.loss_and_grad(gc.PTY_THETA, np.arange(len(gc.PTY_POS)), p['meas'])
    assert s.eng.probe_stack and (s.eng.sweep_fused, s.eng.adjoint_fused) == (0, 0)      # a carrier field; no fused sweep in the far field
    gd, gb = s.gradient_to_host()
    _check(gc.solver_id(c), c, (float(abs(loss - p['loss']) / abs(p['loss'])), float(gc.rel(gd, p['gd'])), float(gc.rel(gb, p['gb']))))
