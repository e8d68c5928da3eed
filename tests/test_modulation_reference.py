"""tests/modulation_reference.py checked against itself and against the oracle (no GPU): the exact factor is the oracle's, the
device algorithm restated in numpy float32 satisfies the bound on every case, the cases reach every branch, every plausible
defect of the algorithm exceeds the bound somewhere, and the strong-phase engine cases leave the project's float32 bounds
(tests/test_gpu_parity.py) a factor of two above what a plain complex64 restatement of the oracle reaches."""
import functools

import numpy as np
import pytest

import modulation_reference as mref

K32 = np.float32(mref.K64)


@functools.lru_cache(maxsize=None)
def _case(name):
    out = {'sweep': mref.sweep, 'switches': lambda k: mref.switches(k)[:2], 'special': mref.special}[name](K32)
    for a in out:
        a.setflags(write=False)
    return out


CASES = ('sweep', 'switches', 'special')


def test_reference_is_the_oracles_factor():
    """np.exp(1j*k*d) * np.exp(-k*b) - 1 (oracle/bdof_oracle.py, multislice_propagate_batch_numpy) at moderate arguments, where
    its cancellation costs nothing: to 1e-15."""
    rng = np.random.default_rng(0)
    x32 = rng.uniform(-3, 3, 4000).astype(np.float32)
    y32 = -rng.uniform(0, 1, 4000).astype(np.float32)
    k = mref.K64
    d, b = x32.astype(np.float64) / k, -y32.astype(np.float64) / k
    oracle = np.exp(1j * k * d) * np.exp(-k * b) - 1
    assert np.abs(mref.reference(x32, y32) - oracle).max() <= 1e-15


def test_cases_stay_in_the_domain_and_have_their_sizes():
    for name in CASES:
        x, y = mref.arguments(*_case(name), K32)
        assert np.abs(x).max() <= mref.X_MAX and y.min() >= mref.Y_MIN and y.max() <= mref.Y_MAX, name
    assert _case('sweep')[0].size == (1 << 21) + 77
    x, y = mref.arguments(*_case('sweep'), K32)
    assert np.abs(x).min() < 1e-8 and np.abs(x).max() > 9e4 and y.min() < -90 and y.max() > 9 and 0.15 < (y > 0).mean() < 0.25
    d, b = _case('special')
    assert np.all(d[mref.SPECIAL_ZERO] == 0) and np.all(b[mref.SPECIAL_ZERO] == 0) and np.signbit(d[1]) and not np.signbit(d[0])
    assert np.all(mref.arguments(d, b, K32)[1][mref.SPECIAL_OPAQUE] == -100)


@pytest.mark.parametrize('name', CASES)
def test_emulated_kernel_stays_within_the_bound(name):
    """The algorithm of slice_modulation_m1 with a correctly rounded exponential: what the bound allows for the device's own
    exponential on top is the rest up to 1."""
    d, b = _case(name)
    ratio, where = mref.worst(mref.emulate(d, b, K32), d, b, K32)
    print('emulated kernel,', name, ': worst |emulated - reference| / bound', ratio, 'at', where)
    assert ratio <= 1.0, (ratio, where)
    if name == 'special':
        assert np.all(mref.emulate(d, b, K32)[mref.SPECIAL_ZERO] == 0)


def test_cases_reach_every_branch():
    x, y = mref.arguments(*_case('sweep'), K32)
    n, q, series = mref.classify(x, y)
    for sign in (-1, 1):
        for quadrant in range(4):
            assert ((np.sign(n) == sign) & (q == quadrant)).sum() >= 50000, (sign, quadrant)
    assert series.sum() >= 500000 and (~series).sum() >= 500000
    for positive in (False, True):
        assert (series & ((y > 0) == positive)).sum() >= 100000 and (~series & ((y > 0) == positive)).sum() >= 40000
    # both sides of each switch: n = m and n = m + 1 around x = (2m + 1) pi / 4, for every m; the series and e - 1 around |y| = 0.1
    d, b, m = mref.switches(K32)
    x, y = mref.arguments(d, b, K32)
    n, q, series = mref.classify(x, y)
    assert d.size == len(mref.SWITCH_M) * 7 * 15
    for mm in mref.SWITCH_M:
        assert set(np.unique(n[m == mm])) == {mm, mm + 1}, mm
        for positive in (False, True):
            side = (m == mm) & (y != 0) & ((y > 0) == positive)
            assert (series & side).sum() >= 14 and (~series & side).sum() >= 14, (mm, positive)
    assert {int(v) for v in np.unique(q)} == {0, 1, 2, 3} and (n < 0).sum() >= 4000 and (n > 0).sum() >= 4000


@pytest.mark.parametrize('wrong', mref.WRONG)
def test_cases_tell_a_wrong_kernel_from_a_right_one(wrong):
    """Each defect exceeds the bound somewhere in the cases the device is given."""
    worst = 0.0
    for name in CASES:
        d, b = _case(name)
        worst = max(worst, mref.worst(mref.emulate(d, b, K32, wrong=wrong), d, b, K32)[0])
    print(wrong, ': worst ratio', worst)
    assert worst > 1.0, (wrong, worst)


@pytest.mark.parametrize('case', mref.ENGINE_CASES, ids=str)
def test_engine_cases_leave_the_float32_bounds_a_factor_of_two(case):
    """The condition for asking the engines for test_gpu_parity.py's bounds at strong phase: the oracle's model in plain complex64
    (scipy.fft, no carrier splitting) stays below half of each of them, at every case test_gpu_modulation.py runs."""
    c = mref.engine_case(*case)
    d, loss, gd, gb = mref.c64_loss_and_grad(c['delta_eff'], c['beta_eff'], c['pr'], c['pi'], c['meas'], case[3])
    e = mref.errors(c, d, loss, gd, gb)
    print('complex64 restatement', case, 'wave / intensity / loss / g_delta / g_beta rel err', e)
    assert mref.within(e, 0.5), e


def test_engine_regimes_are_what_they_claim():
    k = mref.K64
    for name in mref.REGIMES:
        d, b = mref.regime(name, (mref.B, 64, 64, mref.S))
        x, y = mref.arguments(d, b, K32)
        de, be = mref.oracle_inputs(d, b)
        assert np.array_equal((k * de).astype(np.float32), x) and np.array_equal((-k * be).astype(np.float32), y)
        n, q, series = mref.classify(x, y)
        if name == 'pi':
            assert {int(v) for v in np.unique(q)} == {0, 1, 2, 3} and (n < 0).any() and abs(np.mean(mref.reference(x, y)) + 1) < 0.05
        elif name == 'wrapped':
            assert np.abs(x).max() > 50 and np.abs(mref.reference(x, y)).max() < 0.03 and set(np.unique(n)) >= {-32, 0, 32}
        else:
            assert y.min() < -0.59 and (~series).mean() > 0.8 and x.max() > 0.99


def _solver_volume(n=64, seed=3):
    d32, b32 = mref.regime('pi', (n, n, n), seed=seed)                                 # test_gpu_modulation.py::_volume
    return mref.oracle_inputs(d32, b32)


def test_solver_cases_in_plain_complex64():
    """The two solver cases of test_gpu_modulation.py run 64 slices of regime 'pi', ten times the depth the bounds above were
    argued at, and plain complex64 does NOT keep a factor of two there: this test pins the levels it does reach (measured
    figures in the comments), so that a reader sees the headroom of each device bound.
      full field (bounds loss 1e-5, gradients 2e-4): loss 2.5e-6, g_delta 7.0e-5 — below half; g_beta 3.3e-4 — above the bound.
      ptychography windows (bounds intensity 1.2e-5, loss 5e-5, gradients 1e-3): 6.0e-6, 1.7e-5, 1.1e-4 / 7.3e-4 — below the bounds.
    The device is expected to beat the restatement, and does (MEASUREMENTS: full-field gradients 3e-5, ptychography gradients
    1e-4 and below): its transfer function and twiddles are dithered over the slices, so their roundings do not add up
    coherently over 64 slices as one fixed complex64 table's do, and the ptychography probe rides on a float64 carrier field.
    The convolution propagator has no complex64 restatement; its case is 6 slices of 'pi' at 64 x 128, where the
    transfer-function restatement above stays below half of every bound."""
    from oracle import bdof_oracle as orc
    n, n_theta, fp = 64, 4, 1e-4
    de, be = _solver_volume()
    coords = orc.rotation_lookup([n, n, n], n_theta)
    one, zero = np.ones((n, n)), np.zeros((n, n))
    rot = np.stack([orc.apply_rotation(np.stack([de, be], axis=3), coords[j]) for j in (1, 3)])
    ref, _ = orc.multislice_propagate_batch_numpy(rot[..., 0], rot[..., 1], one, zero, mref.E_EV, mref.PSIZE_CM, fp, rot[..., 0].shape,
                                                  return_probe_array=False)
    meas = mref.measurement(ref)
    rl, rgd, rgb = orc.multislice_loss_and_grad(rot[..., 0], rot[..., 1], one, zero, mref.E_EV, mref.PSIZE_CM, meas, fp)
    d, l, gd, gb = mref.c64_loss_and_grad(rot[..., 0], rot[..., 1], one, zero, meas, fp)
    e = (abs(l - rl) / rl, mref.rel(gd, rgd), mref.rel(gb, rgb))
    print('complex64 restatement, full-field case: loss / g_delta / g_beta rel err', e, 'mean amplitude', np.abs(ref).mean())
    assert e[0] <= 0.5 * 1e-5 and e[1] <= 0.5 * 2e-4 and 2e-4 < e[2] <= 2 * 2e-4, e
    assert np.abs(ref).mean() < 2e-4                                                   # the dark exit wave of MEASUREMENTS' defect
    psz = (64, 64)
    pos = np.array([(32, 32), (32, 33), (10, 50), (60, 8)])
    prr, pii = orc.gaussian_probe(psz, 6., 6., 0.5)
    pad, half = orc.ptycho_pad_amounts(pos, psz, (n, n, n))
    rot = orc.apply_rotation(np.stack([de, be], axis=3), coords[2])
    obj_pad = np.pad(rot, ((pad[0, 0], pad[0, 1]), (pad[1, 0], pad[1, 1]), (0, 0), (0, 0)), mode='constant')
    subs = np.stack([obj_pad[p[0] + pad[0, 0] - half[0]:p[0] + pad[0, 0] - half[0] + psz[0],
                             p[1] + pad[1, 0] - half[1]:p[1] + pad[1, 0] - half[1] + psz[1]] for p in pos])
    ref, _ = orc.multislice_propagate_batch_numpy(subs[..., 0], subs[..., 1], prr, pii, mref.E_EV, mref.PSIZE_CM, 'inf', subs[..., 0].shape,
                                                  return_probe_array=False)
    meas = mref.measurement(ref)
    rl, rgd, rgb = orc.multislice_loss_and_grad(subs[..., 0], subs[..., 1], prr, pii, mref.E_EV, mref.PSIZE_CM, meas, 'inf')
    d, l, gd, gb = mref.c64_loss_and_grad(subs[..., 0], subs[..., 1], prr, pii, meas, 'inf')
    e = (mref.rel(np.abs(d) ** 2, np.abs(ref) ** 2), abs(l - rl) / rl, mref.rel(gd, rgd), mref.rel(gb, rgb))
    print('complex64 restatement, ptychography windows: intensity / loss / g_delta / g_beta rel err', e)
    assert e[0] <= 1.2e-5 and e[1] <= 5e-5 and e[2] <= 1e-3 and e[3] <= 1e-3, e
    assert e[0] > 5e-7 and e[1] > 2e-6 and e[3] > 1e-4, e                              # the weak-object set of test_gpu_ptycho.py is out of its reach
