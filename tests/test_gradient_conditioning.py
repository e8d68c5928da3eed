"""The tight gradient bound of tests/gradient_cases.py, argued without a GPU.

1. Condition of the bound: at every case tests/test_gpu_gradient_tight.py runs, the model restated in plain complex64
   (modulation_reference.c64_loss_and_grad: scipy.fft, no carrier splitting, no dithered constants) stays at or below HALF the
   case's bound on g_delta, g_beta and the probe gradient, and the loss below half of 1e-5 — the factor of two over plain
   complex64 that test_modulation_reference.py asks of the 2e-4 bounds.  A bound other than 2e-5 is the rule's (bound_rule).
2. The bound sees what 2e-4 does not: the float64 model with ONE defect in its adjoint sweep (reference_model.AdjointHook)
   against the clean model, at the case named beside the defect, lands strictly between twice the new bound and 2e-4 — above
   what device rounding could mask, below what the other files' bound notices.
3. The data is what it claims: the residual split stays on under measurement_wide, and scaled data leaves g_delta empty.
Every test prints its figures (MEASUREMENTS.md)."""
import numpy as np
import pytest

import gradient_cases as gc
import modulation_reference as mref
import reference_model as ref_model

OLD_BOUND = 2e-4                                      # tests/test_gpu_parity.py


# ---- 1. condition of the bound --------------------------------------------------------------------------------------------------
def _check_condition(tag, c, e):
    worst = max(e[1:])
    print('complex64 restatement', tag, 'loss / g_delta / g_beta (/ g_probe) rel err', e, 'bound', c['bound'])
    assert e[0] <= 0.5 * gc.LOSS_BOUND, e
    assert worst <= 0.5 * c['bound'], (e, c['bound'])
    assert gc.BOUND <= c['bound'] <= 1e-4
    if c['bound'] != gc.BOUND:                       # an exception is the rule's figure, not a rounder one
        assert worst > 0.5 * gc.BOUND and c['bound'] <= gc.bound_rule(worst), (worst, c['bound'])


@pytest.mark.parametrize('c', gc.CASES, ids=gc.case_id)
def test_complex64_restatement_stays_below_half_the_bound(c):
    _check_condition(gc.case_id(c), c, gc.restatement(c))


@pytest.mark.parametrize('c', gc.SOLVER_CASES, ids=gc.solver_id)
def test_complex64_restatement_of_the_solver_cases(c):
    """The rotated fields the solver hands its engine, in the rotated frame: the rotation tables and the windows are index work."""
    _check_condition(gc.solver_id(c), c, gc.solver_restatement(c))


def test_every_path_of_the_issue_has_its_cases():
    ids = [gc.case_id(c) for c in gc.CASES] + [gc.solver_id(c) for c in gc.SOLVER_CASES]
    assert len(set(ids)) == len(ids)
    paths = {c['path'] for c in gc.CASES + gc.SOLVER_CASES}
    assert paths == {'two-kernel', 'fused', 'tape-free', 'resident', 'generic', 'generic-adjoint64', 'streams', 'binning', 'planes',
                     'weights', 'poisson', 'probe-gradient', 'fullfield-solver', 'ptycho-solver'}
    two = [c for c in gc.CASES if c['path'] == 'two-kernel']
    for shape in ((64, 64), (128, 128), (64, 256), (256, 128), (512, 512)):
        assert {c['fp'] for c in two if (c['Y'], c['X']) == shape and c['variant'] == 'numpy_skip_last'} >= set(gc.FPS), shape
    assert {(c['Y'], c['X']) for c in two} >= {(1024, 1024), (512, 1024)}
    assert {c['fp'] for c in two if c['variant'] == 'tf_all'} == set(gc.FPS)
    assert {c['regime'] for c in two if (c['Y'], c['X']) == (64, 128)} == {'weak', 'pi', 'absorbing'}
    assert any(c['S'] == 70 for c in two)
    assert not gc.LEFT_OUT


def test_bound_rule():
    assert gc.bound_rule(7.3e-6) == 2e-5 and gc.bound_rule(1e-5) == 2e-5
    assert gc.bound_rule(1.01e-5) == 3e-5 and gc.bound_rule(2.47e-5) == 5e-5 and gc.bound_rule(2.97e-5) == 6e-5 and gc.bound_rule(3.51e-5) == 8e-5
    assert gc.bound_rule(4.9e-5) == 1e-4 and gc.bound_rule(5.1e-5) > 1e-4


# ---- 2. the bound sees what 2e-4 does not -----------------------------------------------------------------------------------------
class LastRowFromPsi(ref_model.AdjointHook):
    """The last step's gradient row formed from psi (the wave before the modulation) instead of phi = c psi: a row kernel that
    reads the field buffer where it should read the tape."""
    def row_field(self, i, phis, cs):
        return phis[i] / cs[i] if i == len(phis) - 1 else phis[i]


class AbsorptionDropped(ref_model.AdjointHook):
    """conj(c) replaced by its phase: the adjoint un-turns the phase and forgets exp(-k beta)."""
    def back_factor(self, i, cs):
        return np.conj(cs[i]) / np.abs(cs[i])


class OneFactorSkipped(ref_model.AdjointHook):
    """Step 1 carries G(phi) back without conj(c): an off-by-one in which slices a fused kernel modulates."""
    def back_factor(self, i, cs):
        return np.ones_like(cs[i]) if i == 1 else np.conj(cs[i])


class HalfABin(ref_model.AdjointHook):
    """Under slice binning the back factor of step 1 is formed from the first voxel slice of its bin alone."""
    def __init__(self, first):
        self.first = first

    def back_factor(self, i, cs):
        return np.conj(self.first) if i == 1 else np.conj(cs[i])


def _by_id(case_id):
    return next(c for c in gc.CASES if gc.case_id(c) == case_id)


def _half_a_bin(c, p):
    k, b = mref.K64, c['b']
    return HalfABin(np.exp(1j * k * p['delta_eff'][..., b]) * np.exp(-k * p['beta_eff'][..., b]))


WEAK = 'two-kernel-64x64-weak-0.0001'               # B = 2, 64 x 64, S = 5, free_prop 1e-4: test_forward_and_gradient_vs_oracle's
# (defect, case, the quantities it must show in: 1 g_delta, 2 g_beta, 3 probe gradient)
DEFECTS = [('last row from psi', LastRowFromPsi, WEAK, (1, 2)),
           ('absorption dropped', AbsorptionDropped, WEAK, (1, 2)),
           ('one factor skipped', OneFactorSkipped, WEAK, (1, 2)),
           ('absorption dropped, k_slice_*_adj', AbsorptionDropped, 'fused-64x128-weak-0.0001-S=4-fused=True', (1, 2)),
           ('last row from psi, EpiBwd', LastRowFromPsi, 'resident-64x64-weak-0.0001-S=6', (1, 2)),
           ('one factor skipped, k_g_bwd', OneFactorSkipped, 'generic-72x72-weak-0.0001-S=6', (1, 2)),
           ('absorption dropped, probe gradient', AbsorptionDropped, 'probe-gradient-64x128-weak-0.0001-S=6-probe_grad=True', (1, 2, 3)),
           ('absorption dropped, detector planes', AbsorptionDropped, 'planes-64x128-weak-(5e-05, 0.0001)-S=6', (1, 2)),
           ('half a bin', _half_a_bin, 'binning-64x64-weak-0.0001-S=6-b=2', (1, 2))]


@pytest.mark.parametrize('name,make,case_id,shows', DEFECTS, ids=[d[0] for d in DEFECTS])
def test_bound_tells_a_wrong_adjoint_from_a_right_one(name, make, case_id, shows):
    """Each defect is invisible to 2e-4 and visible to the new bound with a factor of two to spare, in float64, at wide data."""
    c = _by_id(case_id)
    p = gc.problem(c)
    hook = make(c, p) if make is _half_a_bin else make()
    _, gd, gb, g0, _ = ref_model.loss_and_grad(p['delta_eff'], p['beta_eff'], p['pr'], p['pi'], gc.E, gc.PS, p['meas'], gc._fp(c),
                                              c['variant'], c.get('b', 1), term=gc.terms(c, p['w'])[0], hook=hook)
    e = (None, float(gc.rel(gd, p['gd'])), float(gc.rel(gb, p['gb'])), float(gc.rel(g0.sum(axis=0), p['gp'])))
    print('defect:', name, 'at', case_id, 'g_delta / g_beta / g_probe rel err', e[1:], 'bound', c['bound'])
    for q in shows:
        assert 2 * c['bound'] < e[q] < OLD_BOUND, (name, q, e)


class WrongTapeSlot(ref_model.AdjointHook):
    """Step 1's gradient row formed from the tape slot of step 0."""
    def row_field(self, i, phis, cs):
        return phis[0] if i == 1 else phis[i]


class PlaneMissing(ref_model.AdjointHook):
    """The fan-in over the detector planes stops after the first."""
    def plane_terms(self, terms):
        return terms[:1]


@pytest.mark.parametrize('name,make,case_id', [('wrong tape slot', WrongTapeSlot, WEAK),
                                               ('wrong tape slot for a bin', WrongTapeSlot, 'binning-64x64-weak-0.0001-S=6-b=2'),
                                               ('plane missing', PlaneMissing, 'planes-64x128-weak-(5e-05, 0.0001)-S=6')])
def test_gross_defects_exceed_both_bounds(name, make, case_id):
    """Not every mistake needs the new bound: these two are far above 2e-4 as well, which is why the catalogue leaves them out."""
    c = _by_id(case_id)
    p = gc.problem(c)
    _, gd, gb, _, _ = ref_model.loss_and_grad(p['delta_eff'], p['beta_eff'], p['pr'], p['pi'], gc.E, gc.PS, p['meas'], gc._fp(c),
                                             c['variant'], c.get('b', 1), hook=make())
    e = (float(gc.rel(gd, p['gd'])), float(gc.rel(gb, p['gb'])))
    print('gross defect:', name, 'at', case_id, 'g_delta / g_beta rel err', e)
    assert min(e) > 100 * OLD_BOUND, (name, e)


def test_the_clean_hook_is_the_model():
    c = _by_id(WEAK)
    p = gc.problem(c)
    out = ref_model.loss_and_grad(p['delta_eff'], p['beta_eff'], p['pr'], p['pi'], gc.E, gc.PS, p['meas'], c['fp'], hook=ref_model.AdjointHook())
    assert out[0] == p['loss'] and np.array_equal(out[1], p['gd']) and np.array_equal(out[2], p['gb'])


# ---- 3. the data is what it claims --------------------------------------------------------------------------------------------------
def test_wide_data_keeps_the_residual_split():
    """MultisliceEngine.choose_residual_split switches the split off when mean|m - |a0|| > mean(m)."""
    c = _by_id(WEAK)
    p = gc.problem(c)
    a0 = abs(complex((p['pr'] + 1j * p['pi']).astype(np.complex64).astype(np.complex128).mean()))      # MultisliceEngine._scalar_carrier
    m = p['meas']
    print('wide data: |a0|', a0, 'mean|m - |a0||', np.abs(m - a0).mean(), 'mean m', m.mean(), 'min / max of m', m.min(), m.max())
    assert np.abs(m - a0).mean() < m.mean()
    assert m.min() >= 0 and 1.8 < m.max() / a0 < 2.3 and np.array_equal(m, m.astype(np.float32).astype(np.float64))
    again = gc.wide(ref_model.forward(p['delta_eff'], p['beta_eff'], p['pr'], p['pi'], gc.E, gc.PS, c['fp'])[0])
    assert np.array_equal(again, m)                                                    # deterministic
    other = ref_model.measurement_wide(np.ones((2, 8, 8)), seed=1)
    assert not np.array_equal(other, ref_model.measurement_wide(np.ones((2, 8, 8)), seed=0))
    assert not np.array_equal(ref_model.measurement_wide(np.ones((2, 8, 8))), mref.measurement(np.ones((2, 8, 8))))     # a stream of its own


def test_scaled_data_leaves_g_delta_empty():
    """m = 3 |ref|: G(d) is proportional to d, conj(phi) G(phi) to |phi|^2, and g_delta is what is left of its imaginary part."""
    c = _by_id(WEAK)
    p = gc.problem(c)
    wave, _ = ref_model.forward(p['delta_eff'], p['beta_eff'], p['pr'], p['pi'], gc.E, gc.PS, c['fp'])
    ratios = {}
    for name, m in (('3 |ref|', 3 * np.abs(wave)), ('0', 0 * np.abs(wave)), ('wide', p['meas'])):
        _, gd, gb, _, _ = ref_model.loss_and_grad(p['delta_eff'], p['beta_eff'], p['pr'], p['pi'], gc.E, gc.PS, m, c['fp'])
        ratios[name] = float(np.linalg.norm(gd) / np.linalg.norm(gb))
    print('|g_delta| / |g_beta| by data:', ratios)
    assert ratios['3 |ref|'] < 1e-3 and ratios['0'] < 1e-3
    assert 0.3 < ratios['wide'] < 3
