"""The Poisson (photon-counting) data term off the GPU: the float64 reference the GPU tests compare against
(tests/reference_model.py under tests/poisson_reference.py's data term) is itself checked against central differences of its
own loss; the loss's defining properties; the keyword surface of the two entry points; the C symbol."""
import numpy as np
import pytest

import poisson_reference as pref
import reference_model as ref_model
from reference_model import setup as _setup

MU = 2e6
POISSON = ref_model.data_term(pref.poisson_loss, pref.poisson_seed, MU)


@pytest.mark.parametrize('fp', [None, 1e-4, 'inf'])
@pytest.mark.parametrize('variant', ['numpy_skip_last', 'tf_all'])
def test_reference_gradient_against_central_differences(fp, variant):
    """16 x 16 x 6, B = 2: the analytic gradient along six random directions (three of delta, three of beta, as golden vector G20
    takes directional derivatives) against central differences of poisson_loss over orc.multislice_propagate_batch_numpy, to the
    1e-6 the oracle's own gradient is held to there."""
    delta, beta, pr, pi, rng = _setup()
    ref, _ = ref_model.forward(delta, beta, pr, pi, 5000., 1e-7, fp, variant)
    meas = np.abs(ref) * np.abs(1 + 0.05 * rng.normal(size=ref.shape))
    loss, gd, gb, gp = ref_model.loss_and_grad(delta, beta, pr, pi, 5000., 1e-7, meas, fp, variant, term=POISSON)[:4]
    assert abs(loss - ref_model.loss_only(delta, beta, pr, pi, 5000., 1e-7, meas, fp, variant, term=POISSON)) <= 1e-14 * abs(loss)
    assert gp.shape == ref.shape
    errs = []
    for which in (0, 1):
        for _ in range(3):
            v = rng.choice([-1.0, 1.0], size=delta.shape)
            eps = 1e-7
            if which == 0:
                lp = ref_model.loss_only(delta + eps * v, beta, pr, pi, 5000., 1e-7, meas, fp, variant, term=POISSON)
                lm = ref_model.loss_only(delta - eps * v, beta, pr, pi, 5000., 1e-7, meas, fp, variant, term=POISSON)
            else:
                lp = ref_model.loss_only(delta, beta + eps * v, pr, pi, 5000., 1e-7, meas, fp, variant, term=POISSON)
                lm = ref_model.loss_only(delta, beta - eps * v, pr, pi, 5000., 1e-7, meas, fp, variant, term=POISSON)
            fd = (lp - lm) / (2 * eps)
            an = float(np.sum((gd if which == 0 else gb) * v))
            errs.append(abs(fd - an) / abs(an))
    print('poisson reference, directional derivatives rel err', fp, variant, errs)
    assert max(errs) <= 1e-6, errs


def test_reference_probe_gradient_against_central_differences():
    """The probe gradient the module returns: sum over the batch of G(psi_0) = dL/d probe_real + i dL/d probe_imag.  The forward
    model rounds the probe to complex64 (np_funcs.py:20-21), so the differences step between float32 numbers."""
    delta, beta, pr, pi, rng = _setup(seed=2)
    pr, pi = pr.astype(np.float32).astype(np.float64), pi.astype(np.float32).astype(np.float64)
    ref, _ = ref_model.forward(delta, beta, pr, pi, 5000., 1e-7, 1e-4)
    meas = np.abs(ref) * np.abs(1 + 0.05 * rng.normal(size=ref.shape))
    _, _, _, gp = ref_model.loss_and_grad(delta, beta, pr, pi, 5000., 1e-7, meas, 1e-4, term=POISSON)[:4]
    g = gp.sum(axis=0)
    step = np.float32(2.0 ** -10)               # exactly representable beside values of size one: no rounding of the stepped probe
    for part in (0, 1):
        v = rng.choice([-1.0, 1.0], size=pr.shape) * float(step)
        args_p = (pr + v, pi) if part == 0 else (pr, pi + v)
        args_m = (pr - v, pi) if part == 0 else (pr, pi - v)
        lp = ref_model.loss_only(delta, beta, *args_p, 5000., 1e-7, meas, 1e-4, term=POISSON)
        lm = ref_model.loss_only(delta, beta, *args_m, 5000., 1e-7, meas, 1e-4, term=POISSON)
        an = float(np.sum((g.real if part == 0 else g.imag) * v))
        # central differences with a step of 1e-3: their own truncation error is (step)^2 ~ 1e-6 relative
        assert abs((lp - lm) / 2 - an) <= 1e-4 * abs(an), (part, (lp - lm) / 2, an)


def test_loss_is_zero_at_the_fit_and_twice_mu_least_squares_near_it():
    rng = np.random.default_rng(1)
    d = (1 + 0.2 * rng.normal(size=(2, 16, 16))) * np.exp(1j * rng.uniform(0, 6, size=(2, 16, 16)))
    a = np.abs(d)
    assert pref.poisson_loss(d, a, MU) == 0.0
    assert np.all(pref.poisson_seed(d, a, MU) == 0)
    eps = 1e-3
    m = a * (1 + eps)
    ratio = pref.poisson_loss(d, m, MU) / (2 * MU * pref.lsq_loss(d, m))
    # mu (a^2 - m^2 - 2 m^2 ln(a / m)) with m = a (1 + eps) is 2 mu a^2 eps^2 (1 + eps / 3 + O(eps^2)); least squares a^2 eps^2
    print('poisson / (2 mu lsq) at eps = 1e-3:', ratio)
    assert abs(ratio - 1) <= 2 * eps
    assert abs(ratio - (1 + eps / 3)) <= 10 * eps ** 2
    # m = 0: mu a^2; a = 0: nothing
    assert abs(pref.poisson_loss(d, np.zeros_like(a), MU) - MU * np.mean(a ** 2)) <= 1e-12 * MU
    assert pref.poisson_loss(np.zeros_like(d), a, MU) == 0.0


def test_loss_keywords_are_checked_before_anything_touches_a_file_or_a_gpu(tmp_path):
    """loss_type / poisson_multiplier are keywords of both entry points (the reference's tensorflow_recon/ptychography.py carries
    poisson_multiplier); a wrong value is a ValueError at the top of the call — not swallowed by **kwargs."""
    from beyond_dof_amd.fullfield import reconstruct_fullfield
    from beyond_dof_amd.ptychography import reconstruct_ptychography
    ff = dict(save_path=str(tmp_path), n_epochs=1, minibatch_size=1)
    pt = dict(probe_pos=[(8, 8)], probe_size=(8, 8), obj_size=(16, 16, 16), save_path=str(tmp_path), n_epochs=1, minibatch_size=1)
    with pytest.raises(ValueError, match='loss_type'):
        reconstruct_fullfield('data.h5', loss_type='bogus', **ff)
    with pytest.raises(ValueError, match='loss_type'):
        reconstruct_ptychography('data.h5', loss_type='bogus', **pt)
    for bad in (0, -1.0):
        with pytest.raises(ValueError, match='poisson_multiplier'):
            reconstruct_fullfield('data.h5', loss_type='poisson', poisson_multiplier=bad, **ff)
        with pytest.raises(ValueError, match='poisson_multiplier'):
            reconstruct_ptychography('data.h5', loss_type='poisson', poisson_multiplier=bad, **pt)
    with pytest.raises(ValueError, match='poisson'):
        reconstruct_fullfield('data.h5', loss_type='poisson', propagator='conv', **ff)
    with pytest.raises(ValueError, match='poisson'):
        reconstruct_ptychography('data.h5', loss_type='poisson', propagator='conv', **pt)
    # any propagator value other than 'fft' is refused with the Poisson term, known to the entry point or not (the tiled
    # propagator itself is refused in C, bdof_field_loss_seed: tests/test_gpu_poisson.py)
    with pytest.raises(ValueError, match="propagator='fft'"):
        reconstruct_fullfield('data.h5', loss_type='poisson', propagator='anything-else', **ff)


def test_set_loss_symbol_is_bound_and_exported():
    import __graft_entry__ as entry
    from beyond_dof_amd import _lib
    assert 'bdof_set_loss' in _lib.EXPORTED_SYMBOLS
    entry.build()
    lib = _lib.load()
    assert hasattr(lib, 'bdof_set_loss')
    assert lib.bdof_set_loss(None, 0, 1.0) != 0          # no context: an argument error, not a crash
    assert (_lib.LOSS_LSQ, _lib.LOSS_POISSON) == (0, 1)
