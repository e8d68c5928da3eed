"""Slice binning off the GPU: the float64 reference the GPU tests compare against (tests/reference_model.py) is pinned to the
oracle where the two models coincide (b = 1; objects that leave all but one slice of a bin empty), its gradient is checked
against central differences of its own loss, and the keyword surface of the two entry points and the C symbol are checked."""
import numpy as np
import pytest

from oracle import bdof_oracle as orc

import reference_model as ref_model
from reference_model import rel

E, PS = 5000., 1e-7
DETECTORS = [None, 1e-4, 'inf']


def _setup():
    return ref_model.setup(S=12)


@pytest.mark.parametrize('fp', DETECTORS)
@pytest.mark.parametrize('variant', ['numpy_skip_last', 'tf_all'])
def test_binning_one_is_the_oracle_exactly(fp, variant):
    delta, beta, pr, pi, rng = _setup()
    ref, ref_after = orc.multislice_propagate_batch_numpy(delta, beta, pr, pi, E, PS, fp, delta.shape, variant=variant)
    d, after = ref_model.forward(delta, beta, pr, pi, E, PS, fp, variant, b=1)
    assert np.array_equal(d, ref) and np.array_equal(after, ref_after)
    meas = np.abs(ref) * np.abs(1 + 0.05 * rng.normal(size=ref.shape))
    rl, rgd, rgb, rgp = orc.multislice_loss_and_grad(delta, beta, pr, pi, E, PS, meas, fp, variant, return_probe_grad=True)
    loss, gd, gb, gp, _ = ref_model.loss_and_grad(delta, beta, pr, pi, E, PS, meas, fp, variant, b=1)
    diffs = (abs(loss - rl), np.abs(gd - rgd).max(), np.abs(gb - rgb).max(), np.abs(gp - rgp).max())
    print('b = 1 against the oracle: differences', fp, variant, diffs)
    assert diffs == (0.0, 0.0, 0.0, 0.0), diffs


@pytest.mark.parametrize('b', [2, 3, 4])
@pytest.mark.parametrize('fp', DETECTORS)
def test_first_slice_of_each_bin_only_gives_the_unbinned_wave(b, fp):
    """tf_all, object only in the first voxel slice of every bin: the unbinned model modulates once and then takes b steps of dz
    through empty slices, H(dz)^b = H(b dz) — the binned wave IS the oracle's."""
    delta, beta, pr, pi, _ = _setup()
    keep = np.zeros(delta.shape[-1])
    keep[::b] = 1
    delta, beta = delta * keep, beta * keep
    ref, _ = orc.multislice_propagate_batch_numpy(delta, beta, pr, pi, E, PS, fp, delta.shape, variant='tf_all')
    d, _ = ref_model.forward(delta, beta, pr, pi, E, PS, fp, 'tf_all', b=b)
    e = rel(d, ref)
    print('identity 1 (first slice of each bin, tf_all)', b, fp, e)
    assert e <= 1e-13


@pytest.mark.parametrize('b', [2, 3, 4])
@pytest.mark.parametrize('fp', DETECTORS)
def test_last_slice_of_each_bin_only_gives_the_unbinned_amplitudes(b, fp):
    """numpy_skip_last, plane probe, object only in the last voxel slice of every bin: the unbinned model differs by b - 1 steps
    of the plane wave through empty space in front of the first modulation — a constant phase, so |d| is the oracle's."""
    delta, beta, _, _, _ = _setup()
    Y, X = delta.shape[1:3]
    pr, pi = np.ones((Y, X)), np.zeros((Y, X))
    keep = np.zeros(delta.shape[-1])
    keep[b - 1::b] = 1
    delta, beta = delta * keep, beta * keep
    ref, _ = orc.multislice_propagate_batch_numpy(delta, beta, pr, pi, E, PS, fp, delta.shape)
    d, _ = ref_model.forward(delta, beta, pr, pi, E, PS, fp, 'numpy_skip_last', b=b)
    e = rel(np.abs(d), np.abs(ref))
    print('identity 2 (last slice of each bin, numpy_skip_last, plane probe)', b, fp, e)
    assert e <= 1e-13


@pytest.mark.parametrize('b', [2, 3, 4])
def test_binned_and_unbinned_models_differ_for_a_general_object(b):
    """What makes the GPU tests able to tell the two models apart: for a random object the amplitudes differ by far more than
    any bound they assert (1e-5)."""
    delta, beta, pr, pi, _ = _setup()
    ref, _ = orc.multislice_propagate_batch_numpy(delta, beta, pr, pi, E, PS, 1e-4, delta.shape)
    d, _ = ref_model.forward(delta, beta, pr, pi, E, PS, 1e-4, 'numpy_skip_last', b=b)
    e = rel(np.abs(d), np.abs(ref))
    print('binned against unbinned |d|, random object', b, e)
    assert e >= 1e-3


@pytest.mark.parametrize('b', [2, 3, 4])
@pytest.mark.parametrize('fp', DETECTORS)
@pytest.mark.parametrize('variant', ['numpy_skip_last', 'tf_all'])
def test_reference_gradient_against_central_differences(b, fp, variant):
    """16 x 16 x 12, B = 2: directional derivatives along six +-1 directions (three of delta, three of beta) against central
    differences (step 1e-7) of the reference's own loss, to the 1e-6 golden vector G20 and test_poisson_reference.py hold their
    gradients to.  A +-1 direction's derivative g . v is a sum of 6144 signed terms with standard deviation ||g||_2; a direction
    that happens to be nearly orthogonal to the gradient (|g . v| < 0.1 ||g||_2, 8 % of the draws) measures nothing — the
    difference quotient's own truncation error, (1e-7)^2 D^3 L / 6, is then divided by a number that cancelled towards zero —
    and is drawn again.  The criterion looks at the direction alone, never at the error."""
    delta, beta, pr, pi, rng = _setup()
    ref, _ = ref_model.forward(delta, beta, pr, pi, E, PS, fp, variant, b)
    meas = np.abs(ref) * np.abs(1 + 0.05 * rng.normal(size=ref.shape))
    loss, gd, gb, gp, _ = ref_model.loss_and_grad(delta, beta, pr, pi, E, PS, meas, fp, variant, b)
    assert abs(loss - ref_model.loss_only(delta, beta, pr, pi, E, PS, meas, fp, variant, b)) <= 1e-14 * abs(loss)
    assert gp.shape == ref.shape
    for i in range(delta.shape[-1] // b):                   # the slices of a bin share their row
        for j in range(1, b):
            assert np.array_equal(gd[..., i * b + j], gd[..., i * b]) and np.array_equal(gb[..., i * b + j], gb[..., i * b])
    errs = []
    eps = 1e-7
    for which in (0, 1):
        for _ in range(3):
            g = gd if which == 0 else gb
            v = rng.choice([-1.0, 1.0], size=delta.shape)
            while abs(np.sum(g * v)) < 0.1 * np.linalg.norm(g):
                v = rng.choice([-1.0, 1.0], size=delta.shape)
            if which == 0:
                lp = ref_model.loss_only(delta + eps * v, beta, pr, pi, E, PS, meas, fp, variant, b)
                lm = ref_model.loss_only(delta - eps * v, beta, pr, pi, E, PS, meas, fp, variant, b)
            else:
                lp = ref_model.loss_only(delta, beta + eps * v, pr, pi, E, PS, meas, fp, variant, b)
                lm = ref_model.loss_only(delta, beta - eps * v, pr, pi, E, PS, meas, fp, variant, b)
            an = float(np.sum(g * v))
            errs.append(abs((lp - lm) / (2 * eps) - an) / abs(an))
    print('binned reference, directional derivatives rel err', b, fp, variant, errs)
    assert max(errs) <= 1e-6, errs


def test_binning_keywords_are_checked_before_anything_touches_a_file_or_a_gpu(tmp_path):
    from beyond_dof_amd.engine import check_slice_binning
    from beyond_dof_amd.fullfield import reconstruct_fullfield
    from beyond_dof_amd.ptychography import reconstruct_ptychography
    ff = dict(save_path=str(tmp_path), n_epochs=1, minibatch_size=1)
    pt = dict(probe_pos=[(8, 8)], probe_size=(8, 8), obj_size=(16, 16, 16), save_path=str(tmp_path), n_epochs=1, minibatch_size=1)
    for bad in (0, -1, 1.5, 'x'):
        with pytest.raises(ValueError, match='slice_binning'):
            check_slice_binning(bad)
        with pytest.raises(ValueError, match='slice_binning'):
            reconstruct_fullfield('data.h5', slice_binning=bad, **ff)
        with pytest.raises(ValueError, match='slice_binning'):
            reconstruct_ptychography('data.h5', slice_binning=bad, **pt)
    check_slice_binning(1)
    check_slice_binning(np.int64(4))
    for entry, kw in ((reconstruct_fullfield, ff), (reconstruct_ptychography, pt)):
        with pytest.raises(ValueError, match='slice_binning'):
            entry('data.h5', slice_binning=2, propagator='conv', **kw)
        for prec in ('first-step', 'float64'):
            with pytest.raises(ValueError, match='slice_binning'):
                entry('data.h5', slice_binning=2, adjoint_precision=prec, **kw)
    with pytest.raises(ValueError, match='slice_binning'):
        reconstruct_fullfield('data.h5', slice_binning=2, rotation='bilinear', **ff)
    # a depth the binning does not divide, known from the arguments alone: 16 % 3
    with pytest.raises(ValueError, match='slice_binning'):
        reconstruct_ptychography('data.h5', slice_binning=3, **pt)


def test_set_slice_binning_symbol_is_bound_and_exported():
    import __graft_entry__ as entry
    from beyond_dof_amd import _lib
    assert 'bdof_set_slice_binning' in _lib.EXPORTED_SYMBOLS
    entry.build()
    lib = _lib.load()
    assert hasattr(lib, 'bdof_set_slice_binning')
    assert lib.bdof_set_slice_binning(None, 2) != 0          # no context: an argument error, not a crash
