"""Detector weights off the GPU: the float64 reference the GPU tests compare against (tests/reference_model.py under
tests/weights_reference.py's data term) against the
oracle and the Poisson reference at w = 1, against central differences of its own weighted loss, and for what w = 0 means; the
keyword surface of the two entry points; the checks of a weight plane; the HDF5 writer that puts a weight plane beside the data;
the C symbol."""
import numpy as np
import pytest

from oracle import bdof_oracle as orc

import poisson_reference as pref
import reference_model as ref_model
import weights_reference as wref
from reference_model import rel, setup as _setup

loss_only = ref_model.loss_only
MU = 2e6
EPS = np.finfo(np.float64).eps


def _weighted(w, loss_type):
    return ref_model.data_term(wref.weighted_loss, wref.weighted_seed, w, loss_type, MU)


@pytest.mark.parametrize('fp', [None, 1e-4, 'inf'])
@pytest.mark.parametrize('variant', ['numpy_skip_last', 'tf_all'])
def test_unit_weights_reproduce_the_unweighted_references(fp, variant):
    """w = 1: the oracle's least-squares loss and gradient, and poisson_reference's.  Bounds: the weighted code multiplies by 1.0 and
    sums instead of taking a mean, which moves the last bit of the loss only; against the oracle the forward sweep is a second
    implementation of the same float64 arithmetic (multislice_propagate_batch_numpy against the loop inside
    multislice_loss_and_grad), whose results differ by the rounding of S = 6 transforms of 16 x 16 points, a few eps each, and the
    gradient is linear in a residual that is 5 % of the amplitude, which divides that by 0.05: 64 eps on the loss and 4096 eps
    (9e-13) on a gradient's relative L2 error leave an order of magnitude over both."""
    delta, beta, pr, pi, rng = _setup()
    ref, _ = ref_model.forward(delta, beta, pr, pi, 5000., 1e-7, fp, variant)
    meas = np.abs(ref) * np.abs(1 + 0.05 * rng.normal(size=ref.shape))
    one = np.ones(ref.shape[1:])
    l, gd, gb, gp = ref_model.loss_and_grad(delta, beta, pr, pi, 5000., 1e-7, meas, fp, variant, term=_weighted(one, 'lsq'))[:4]
    rl, rgd, rgb, rgp = orc.multislice_loss_and_grad(delta, beta, pr, pi, 5000., 1e-7, meas, fp, variant, return_probe_grad=True)
    e = (abs(l - rl) / rl, rel(gd, rgd), rel(gb, rgb), rel(gp, rgp))
    print('unit weights against the oracle (lsq)', fp, variant, e)
    assert e[0] <= 64 * EPS and max(e[1:]) <= 4096 * EPS, e
    l, gd, gb, gp = ref_model.loss_and_grad(delta, beta, pr, pi, 5000., 1e-7, meas, fp, variant, term=_weighted(one, 'poisson'))[:4]
    rl, rgd, rgb, rgp = ref_model.loss_and_grad(delta, beta, pr, pi, 5000., 1e-7, meas, fp, variant,
                                                term=ref_model.data_term(pref.poisson_loss, pref.poisson_seed, MU))[:4]
    e = (abs(l - rl) / rl, rel(gd, rgd), rel(gb, rgb), rel(gp, rgp))
    print('unit weights against poisson_reference', fp, variant, e)
    assert e[0] <= 8 * EPS and max(e[1:]) <= 8 * EPS, e          # the same forward sweep and the same seed, times 1.0


@pytest.mark.parametrize('loss_type', ['lsq', 'poisson'])
@pytest.mark.parametrize('fp', [None, 1e-4, 'inf'])
@pytest.mark.parametrize('variant', ['numpy_skip_last', 'tf_all'])
def test_weighted_gradient_against_central_differences(loss_type, fp, variant):
    """The cases and the 1e-6 of test_poisson_reference.py, with a weight plane that has zeros.  The step is 2e-8, not that test's
    1e-7: a central difference is off by step^2 L''' / 6 + eps L / step, and along these +-1 directions the first term is 7.5e-7 at
    1e-7 in the far field whatever the direction (measured at steps of 1e-7, 1e-6 and 1e-5: it goes with step^2), which is 2e-6 of
    a directional derivative that happens to come out at 0.33 where its neighbours are 23 and -1.8.  At 2e-8 the two terms are
    3e-8 and 2e-8."""
    delta, beta, pr, pi, rng = _setup()
    ref, _ = ref_model.forward(delta, beta, pr, pi, 5000., 1e-7, fp, variant)
    meas = np.abs(ref) * np.abs(1 + 0.05 * rng.normal(size=ref.shape))
    w = wref.random_weights(ref.shape[1:], rng)
    assert (w == 0).sum() > 5
    args = (5000., 1e-7, meas, fp, variant)
    term = _weighted(w, loss_type)
    loss, gd, gb, gp = ref_model.loss_and_grad(delta, beta, pr, pi, *args, term=term)[:4]
    assert abs(loss - loss_only(delta, beta, pr, pi, *args, term=term)) <= 1e-14 * abs(loss)
    assert gp.shape == ref.shape
    errs = []
    for which in (0, 1):
        for _ in range(3):
            v = rng.choice([-1.0, 1.0], size=delta.shape)
            eps = 2e-8
            if which == 0:
                lp, lm = loss_only(delta + eps * v, beta, pr, pi, *args, term=term), loss_only(delta - eps * v, beta, pr, pi, *args, term=term)
            else:
                lp, lm = loss_only(delta, beta + eps * v, pr, pi, *args, term=term), loss_only(delta, beta - eps * v, pr, pi, *args, term=term)
            fd = (lp - lm) / (2 * eps)
            an = float(np.sum((gd if which == 0 else gb) * v))
            errs.append(abs(fd - an) / abs(an))
    print('weights reference, directional derivatives rel err', loss_type, fp, variant, errs)
    assert max(errs) <= 1e-6, errs


@pytest.mark.parametrize('loss_type', ['lsq', 'poisson'])
def test_weighted_probe_gradient_against_central_differences(loss_type):
    """As test_reference_probe_gradient_against_central_differences: steps between float32 numbers, 1e-4."""
    delta, beta, pr, pi, rng = _setup(seed=2)
    pr, pi = pr.astype(np.float32).astype(np.float64), pi.astype(np.float32).astype(np.float64)
    ref, _ = ref_model.forward(delta, beta, pr, pi, 5000., 1e-7, 1e-4)
    meas = np.abs(ref) * np.abs(1 + 0.05 * rng.normal(size=ref.shape))
    w = wref.random_weights(ref.shape[1:], rng)
    tail, term = (5000., 1e-7, meas, 1e-4), _weighted(w, loss_type)
    g = ref_model.loss_and_grad(delta, beta, pr, pi, *tail, term=term)[3].sum(axis=0)
    step = np.float32(2.0 ** -10)
    for part in (0, 1):
        v = rng.choice([-1.0, 1.0], size=pr.shape) * float(step)
        args_p = (pr + v, pi) if part == 0 else (pr, pi + v)
        args_m = (pr - v, pi) if part == 0 else (pr, pi - v)
        lp, lm = loss_only(delta, beta, *args_p, *tail, term=term), loss_only(delta, beta, *args_m, *tail, term=term)
        an = float(np.sum((g.real if part == 0 else g.imag) * v))
        assert abs((lp - lm) / 2 - an) <= 1e-4 * abs(an), (part, (lp - lm) / 2, an)


@pytest.mark.parametrize('loss_type', ['lsq', 'poisson'])
@pytest.mark.parametrize('fp', [None, 'inf'])
def test_amplitudes_under_a_zero_weight_take_no_part(loss_type, fp):
    """Whatever m holds where w = 0 — NaN, inf, a saturated count, a negative number — loss and gradients do not move by a bit."""
    delta, beta, pr, pi, rng = _setup(seed=3)
    ref, _ = ref_model.forward(delta, beta, pr, pi, 5000., 1e-7, fp)
    meas = np.abs(ref) * np.abs(1 + 0.05 * rng.normal(size=ref.shape))
    w = wref.random_weights(ref.shape[1:], rng)
    dirty = meas.copy()
    junk = np.array([np.nan, np.inf, 65535.0, -1.0, 1e30])
    dirty[:, w == 0] = junk[rng.integers(0, len(junk), size=dirty[:, w == 0].shape)]
    assert np.isnan(dirty).any() and np.isinf(dirty).any()
    a = ref_model.loss_and_grad(delta, beta, pr, pi, 5000., 1e-7, meas, fp, term=_weighted(w, loss_type))[:4]
    b = ref_model.loss_and_grad(delta, beta, pr, pi, 5000., 1e-7, dirty, fp, term=_weighted(w, loss_type))[:4]
    assert a[0] == b[0] and np.isfinite(a[0])
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x, y) and np.isfinite(x).all()
    # ... and the divisor is the pixel count: halving every weight halves the loss, masking pixels does not renormalise it
    half = ref_model.loss_and_grad(delta, beta, pr, pi, 5000., 1e-7, meas, fp, term=_weighted(0.5 * w, loss_type))
    assert abs(half[0] - 0.5 * a[0]) <= 4 * EPS * a[0]


def test_weight_keywords_are_checked_before_anything_touches_a_file_or_a_gpu(tmp_path):
    """detector_weights is a keyword of both entry points, not something **kwargs swallows: with the real-space propagator it is a
    ValueError at the top of the call."""
    from beyond_dof_amd.fullfield import reconstruct_fullfield
    from beyond_dof_amd.ptychography import reconstruct_ptychography
    ff = dict(save_path=str(tmp_path), n_epochs=1, minibatch_size=1)
    pt = dict(probe_pos=[(8, 8)], probe_size=(8, 8), obj_size=(16, 16, 16), save_path=str(tmp_path), n_epochs=1, minibatch_size=1)
    w = np.ones((8, 8), dtype=np.float32)
    with pytest.raises(ValueError, match='detector_weights'):
        reconstruct_fullfield('data.h5', detector_weights=w, propagator='conv', **ff)
    with pytest.raises(ValueError, match='detector_weights'):
        reconstruct_ptychography('data.h5', detector_weights=w, propagator='conv', **pt)
    with pytest.raises(ValueError, match='detector_weights'):
        reconstruct_fullfield('data.h5', detector_weights='exchange/weights', propagator='conv', **ff)


def test_a_weight_plane_is_checked():
    from beyond_dof_amd.engine import check_detector_weights, read_detector_weights
    good = np.ones((6, 8))
    out = check_detector_weights(good, 6, 8)
    assert out.dtype == np.float32 and out.shape == (6, 8)
    assert read_detector_weights(None, 'nowhere.h5', (6, 8)) is None
    for bad in (np.ones((8, 6)), np.ones((1, 6, 8)), -good, np.where(np.arange(48).reshape(6, 8) == 5, np.nan, 1.0),
                np.where(np.arange(48).reshape(6, 8) == 5, np.inf, 1.0), np.zeros((6, 8)), good.astype(np.complex64)):
        with pytest.raises(ValueError, match='detector_weights'):
            check_detector_weights(bad, 6, 8)


def test_weights_travel_in_the_data_file(tmp_path):
    """h5io.write_datasets puts 'exchange/weights' beside 'exchange/data'; both read back, one dataset alone is written as before."""
    from beyond_dof_amd import h5io
    from beyond_dof_amd.engine import read_detector_weights
    rng = np.random.default_rng(0)
    data = (rng.normal(size=(3, 6, 8)) + 1j * rng.normal(size=(3, 6, 8))).astype(np.complex64)
    w = wref.random_weights((6, 8), rng)
    path = str(tmp_path / 'both.h5')
    h5io.write_datasets(path, {'exchange/data': data, 'exchange/weights': w})
    assert np.array_equal(h5io.read_dataset(path), data)
    assert np.array_equal(h5io.read_dataset(path, 'exchange/weights'), w)
    assert np.array_equal(read_detector_weights('exchange/weights', path, (6, 8)), w)
    with pytest.raises(ValueError, match='detector_weights'):
        read_detector_weights('exchange/nothing', path, (6, 8))
    with pytest.raises(ValueError, match='detector_weights'):
        read_detector_weights('exchange/weights', path, (8, 6))
    one, many = str(tmp_path / 'one.h5'), str(tmp_path / 'many.h5')
    h5io.write_dataset(one, 'exchange/data', data)
    h5io.write_datasets(many, {'exchange/data': data})
    assert open(one, 'rb').read() == open(many, 'rb').read()
    with pytest.raises(ValueError):
        h5io.write_datasets(path, {'exchange/data': data, 'other/weights': w})


def test_detector_weights_symbols_are_bound_and_exported():
    import __graft_entry__ as entry
    from beyond_dof_amd import _lib
    assert 'bdof_set_detector_weights' in _lib.EXPORTED_SYMBOLS and 'bdof_adjoint_carrier' in _lib.EXPORTED_SYMBOLS
    entry.build()
    lib = _lib.load()
    assert hasattr(lib, 'bdof_set_detector_weights')
    assert lib.bdof_set_detector_weights(None, None) != 0          # no context: an argument error, not a crash
    assert lib.bdof_adjoint_carrier(None, 1, None, None) != 0
