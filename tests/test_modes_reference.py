"""Probe modes off the GPU: the float64 reference the GPU tests compare against (tests/modes_reference.py) is checked against
central differences of its own loss, against the single-probe model at M = 1, and against the two identities of the model — a
zero mode contributes nothing, a unitary mix of the modes changes nothing — and the host logic of beyond_dof_amd/modes.py
(keywords, starting modes, orthogonalisation) is checked.

The reference starts every sweep from a complex64 probe, as the forward model does (np_funcs.py:20-21, reference_model._sweep).
Two tests need probes whose perturbed or mixed values survive that rounding exactly, or they would measure the rounding (6e-8)
and not the model: they take modes on the grid 2^-12 and steps / mixing matrices with dyadic entries (see each test)."""
import numpy as np
import pytest

import modes_reference as mref
import poisson_reference as pref
import reference_model as ref_model
import weights_reference as wref
from reference_model import rel

E, PS = 5000., 1e-7
MU = 2e6


def _grid(a, bits=12):
    """a rounded to multiples of 2^-bits: exact in float32 with room below for dyadic steps and mixes"""
    return np.round(np.asarray(a) * 2.0 ** bits) / 2.0 ** bits


def _setup(M=3, seed=0):
    """B = 2, 16 x 16 x 6 and M modes: the structured probe of reference_model.setup and M - 1 random fields of half its size."""
    delta, beta, pr, pi, rng = ref_model.setup(B=2, Y=16, X=16, S=6, seed=seed)
    modes = [pr + 1j * pi] + [0.5 * (rng.normal(size=pr.shape) + 1j * rng.normal(size=pr.shape)) for _ in range(M - 1)]
    return delta, beta, _grid(np.array(modes).real) + 1j * _grid(np.array(modes).imag), rng


def _term(kind, weighted, rng, shape):
    w = wref.random_weights(shape, rng) if weighted else None
    if weighted:
        return ref_model.data_term(wref.weighted_loss, wref.weighted_seed, w, kind, MU)
    if kind == 'poisson':
        return ref_model.data_term(pref.poisson_loss, pref.poisson_seed, MU)
    return ref_model.lsq


def _meas(d, rng):
    a = mref.amplitude(d)
    return a * np.abs(1 + 0.05 * rng.normal(size=a.shape))


@pytest.mark.parametrize('fp', [None, 1e-4, 'inf'])
@pytest.mark.parametrize('kind', ['lsq', 'poisson'])
@pytest.mark.parametrize('weighted', [False, True])
def test_reference_gradient_against_central_differences(fp, kind, weighted):
    """B = 2, 16 x 16 x 6, M = 3.  Six +-1 directions in (delta, beta) (three each, step 1e-7, redrawn while nearly orthogonal to
    the gradient, as tests/test_binning_reference.py does) and, for every mode, one direction along its real and one along its
    imaginary part, all to 1e-6.  The modes lie on the grid 2^-12, a mode direction has entries k / 64 (|k| <= 64) and the step is
    2^-16: P +- h u lies on the grid 2^-22 below 4, which float32 holds exactly, so the complex64 start of the sweep changes
    nothing and the difference quotient is the float64 model's."""
    delta, beta, modes, rng = _setup()
    term = _term(kind, weighted, rng, delta.shape[1:3])
    meas = _meas(mref.forward(delta, beta, modes, E, PS, fp), rng)
    loss, gd, gb, gm, _ = mref.loss_and_grad(delta, beta, modes, E, PS, meas, fp, term=term)
    assert abs(loss - mref.loss_only(delta, beta, modes, E, PS, meas, fp, term=term)) <= 1e-14 * abs(loss)
    assert gm.shape == modes.shape
    errs = []
    eps = 1e-7
    for which in (0, 1):
        for _ in range(3):
            g = gd if which == 0 else gb
            v = rng.choice([-1.0, 1.0], size=delta.shape)
            while abs(np.sum(g * v)) < 0.1 * np.linalg.norm(g):
                v = rng.choice([-1.0, 1.0], size=delta.shape)
            dd, db = (eps * v, 0) if which == 0 else (0, eps * v)
            lp = mref.loss_only(delta + dd, beta + db, modes, E, PS, meas, fp, term=term)
            lm = mref.loss_only(delta - dd, beta - db, modes, E, PS, meas, fp, term=term)
            an = float(np.sum(g * v))
            errs.append(abs((lp - lm) / (2 * eps) - an) / abs(an))
    h = 2.0 ** -16
    for m in range(modes.shape[0]):
        for part in (1.0, 1j):
            g = gm[m].real if part == 1.0 else gm[m].imag
            u = rng.integers(-64, 65, size=g.shape) / 64.0
            while abs(np.sum(g * u)) < 0.1 * np.linalg.norm(g) * np.linalg.norm(u) / np.sqrt(u.size):
                u = rng.integers(-64, 65, size=g.shape) / 64.0
            step = np.zeros(modes.shape, dtype=np.complex128)
            step[m] = h * u * part
            assert np.array_equal((modes + step).astype(np.complex64).astype(np.complex128), modes + step)
            lp = mref.loss_only(delta, beta, modes + step, E, PS, meas, fp, term=term)
            lm = mref.loss_only(delta, beta, modes - step, E, PS, meas, fp, term=term)
            an = float(np.sum(g * u))
            errs.append(abs((lp - lm) / (2 * h) - an) / abs(an))
    print('modes reference, directional derivatives rel err', fp, kind, weighted, errs)
    assert max(errs) <= 1e-6, errs


@pytest.mark.parametrize('fp', [None, 1e-4, 'inf'])
@pytest.mark.parametrize('kind', ['lsq', 'poisson'])
def test_one_mode_is_the_single_probe_model(fp, kind):
    delta, beta, modes, rng = _setup(M=1)
    term = _term(kind, True, rng, delta.shape[1:3])
    p = modes[0]
    ref, _ = ref_model.forward(delta, beta, p.real, p.imag, E, PS, fp)
    meas = np.abs(ref) * np.abs(1 + 0.05 * rng.normal(size=ref.shape))
    rl, rgd, rgb, rg0, rd = ref_model.loss_and_grad(delta, beta, p.real, p.imag, E, PS, meas, fp, term=term)
    loss, gd, gb, gm, d = mref.loss_and_grad(delta, beta, modes, E, PS, meas, fp, term=term)
    errs = (abs(loss - rl) / abs(rl), rel(gd, rgd), rel(gb, rgb), rel(gm[0], rg0.sum(axis=0)), rel(d[0], rd))
    print('M = 1 against reference_model.loss_and_grad', fp, kind, errs)
    assert max(errs) <= 1e-14, errs


@pytest.mark.parametrize('fp', [None, 1e-4, 'inf'])
@pytest.mark.parametrize('kind', ['lsq', 'poisson'])
def test_a_zero_mode_changes_nothing(fp, kind):
    delta, beta, modes, rng = _setup(M=2)
    term = _term(kind, True, rng, delta.shape[1:3])
    meas = _meas(mref.forward(delta, beta, modes, E, PS, fp), rng)
    rl, rgd, rgb, rgm, _ = mref.loss_and_grad(delta, beta, modes, E, PS, meas, fp, term=term)
    more = np.concatenate([modes, np.zeros((1,) + modes.shape[1:], dtype=modes.dtype)])
    loss, gd, gb, gm, _ = mref.loss_and_grad(delta, beta, more, E, PS, meas, fp, term=term)
    errs = (abs(loss - rl) / abs(rl), rel(gd, rgd), rel(gb, rgb), rel(gm[:2], rgm))
    print('zero mode appended', fp, kind, errs)
    assert max(errs) <= 1e-14, errs
    assert np.all(gm[2] == 0)


def _dyadic_unitary(rng):
    """A random member of D1 (H / 2) D2 Pi: H the 4 x 4 Hadamard matrix, D1 and D2 diagonal with entries from {1, i, -1, -i}, Pi a
    permutation.  Unitary, every mode mixed into every other, and all entries in {+-1/2, +-i/2}: a mix of modes on the grid 2^-12
    lies on the grid 2^-13 and survives the reference's complex64 start exactly."""
    h2 = np.array([[1, 1], [1, -1]])
    u = np.kron(h2, h2) / 2.0
    d1, d2 = [np.diag(1j ** rng.integers(0, 4, size=4)) for _ in range(2)]
    return d1 @ u @ d2 @ np.eye(4)[rng.permutation(4)]


@pytest.mark.parametrize('fp', [None, 1e-4, 'inf'])
@pytest.mark.parametrize('kind', ['lsq', 'poisson'])
def test_a_unitary_mix_of_the_modes_changes_nothing(fp, kind):
    """P'_m = sum_n U_mn P_n: loss and volume gradient unchanged to 1e-12.  The mode gradients, in the convention of the library
    and of the reference (g = dL/dRe P + i dL/dIm P, so dL = Re sum_n conj(g_n) dP_n), follow the modes: g'_m = sum_n U_mn g_n —
    which is conj(U) acting on the conjugate-convention gradient dL/dRe P - i dL/dIm P."""
    delta, beta, modes, rng = _setup(M=4)
    term = _term(kind, True, rng, delta.shape[1:3])
    meas = _meas(mref.forward(delta, beta, modes, E, PS, fp), rng)
    u = _dyadic_unitary(rng)
    assert np.abs(u @ u.conj().T - np.eye(4)).max() == 0 and np.count_nonzero(u) == 16
    mixed = np.einsum('mn,nyx->myx', u, modes)
    assert np.array_equal(mixed.astype(np.complex64).astype(np.complex128), mixed)
    rl, rgd, rgb, rgm, _ = mref.loss_and_grad(delta, beta, modes, E, PS, meas, fp, term=term)
    loss, gd, gb, gm, _ = mref.loss_and_grad(delta, beta, mixed, E, PS, meas, fp, term=term)
    errs = (abs(loss - rl) / abs(rl), rel(gd, rgd), rel(gb, rgb), rel(gm, np.einsum('mn,nyx->myx', u, rgm)))
    print('unitary mix', fp, kind, errs)
    assert max(errs) <= 1e-12, errs
    assert rel(gm, rgm) > 0.1                                   # (the mix really moved the modes)


# ---- host logic: beyond_dof_amd/modes.py ---------------------------------------------------------------------------------------
def test_check_probe_modes_names_what_it_refuses():
    from beyond_dof_amd.modes import check_probe_modes
    assert check_probe_modes(1) == 1 and check_probe_modes(np.int64(8)) == 8
    assert check_probe_modes(3, propagator='fft', slice_binning=1, adjoint_precision='float32', engine='resident') == 3
    for bad in (0, 9, -1, 1.5, True, 'x', None):
        with pytest.raises(ValueError, match='n_probe_modes'):
            check_probe_modes(bad)
    with pytest.raises(ValueError, match="propagator='conv'"):
        check_probe_modes(2, propagator='conv')
    with pytest.raises(ValueError, match='slice_binning'):
        check_probe_modes(2, slice_binning=2)
    for prec in ('first-step', 'float64'):
        with pytest.raises(ValueError, match='adjoint_precision'):
            check_probe_modes(2, adjoint_precision=prec)
    with pytest.raises(ValueError, match="engine='streaming'"):
        check_probe_modes(2, engine='streaming')


@pytest.mark.parametrize('M', [1, 2, 3, 8])
@pytest.mark.parametrize('shape', [(36, 36), (24, 40)])
def test_initial_modes_powers_and_orthogonality(M, shape):
    from beyond_dof_amd import modes, util
    pr, pi = util.gaussian_probe(shape, shape[0] / 6., shape[1] / 6., 0.5)
    probe = pr + 1j * pi
    p0 = np.sum(np.abs(probe) ** 2)
    for power in (0.02, 0.3):
        P = modes.initial_modes(probe, M, power)
        assert P.shape == (M,) + shape and P.dtype == np.complex128
        pw = modes.mode_power(P)
        want = np.array([1.0] + [power] * (M - 1))
        assert abs(pw.sum() - p0) <= 1e-12 * p0                                     # the set carries the probe's power
        assert np.abs(pw / pw.sum() - want / want.sum()).max() <= 1e-12             # later modes at `power` of mode 0
        flat = P.reshape(M, -1)
        gram = flat @ flat.conj().T
        off = np.abs(gram - np.diag(np.diag(gram))).max() / p0
        print('initial_modes', M, shape, power, 'largest off-diagonal of the Gram matrix / power', off)
        assert off <= 1e-12
        assert rel(P[0] * np.sqrt(want.sum()), probe) <= 1e-14                      # mode 0 is the probe, rescaled
    for bad in ((probe, 0), (probe, 9), (np.zeros(shape), 2), (probe[None], 2)):
        with pytest.raises(ValueError):
            modes.initial_modes(*bad)
    with pytest.raises(ValueError, match='probe_mode_power'):
        modes.initial_modes(probe, 2, 0.0)


def test_orthogonalize_diagonalises_and_preserves_the_intensity():
    from beyond_dof_amd import modes, util
    rng = np.random.default_rng(5)
    pr, pi = util.gaussian_probe((36, 36), 6., 6., 0.5)
    P = modes.initial_modes(pr + 1j * pi, 3, 0.3)
    a = rng.normal(size=(3, 3)) + 1j * rng.normal(size=(3, 3))           # any invertible mix: not orthogonal any more
    Q = np.einsum('mn,nyx->myx', a, P)
    O = modes.orthogonalize(Q)
    flat = O.reshape(3, -1)
    gram = flat @ flat.conj().T
    pw = np.real(np.diag(gram))
    off = np.abs(gram - np.diag(np.diag(gram))).max() / pw.sum()
    inten = np.abs(np.sum(np.abs(O) ** 2, axis=0) - np.sum(np.abs(Q) ** 2, axis=0)).max() / np.sum(np.abs(Q) ** 2, axis=0).max()
    print('orthogonalize: off-diagonal / total power', off, 'powers', pw, 'intensity change', inten)
    assert off <= 1e-13
    assert np.all(np.diff(pw) <= 0)
    assert inten <= 1e-13
    # already orthogonal modes in descending order come back as they are, up to a phase per mode
    O2 = modes.orthogonalize(O)
    for m in range(3):
        assert abs(abs(np.vdot(O[m], O2[m])) - pw[m]) <= 1e-12 * pw[m]
    assert modes.summary_line(O).startswith('probe_mode_power') and len(modes.summary_line(O).split()) == 4


def test_probe_modes_symbols_are_bound_and_exported():
    import __graft_entry__ as entry
    from beyond_dof_amd import _lib
    assert 'bdof_set_probe_modes' in _lib.EXPORTED_SYMBOLS and 'bdof_probe_grad_modes' in _lib.EXPORTED_SYMBOLS
    entry.build()
    lib = _lib.load()
    assert lib.bdof_set_probe_modes(None, 2, None, None, None) != 0          # no context: an argument error, not a crash
    assert lib.bdof_probe_grad_modes(None, None, 0) != 0
