"""Several detector planes per wavefield off the GPU: the float64 reference the GPU tests compare against
(tests/reference_model.py) is pinned to its own single distance where the two detector stages coincide (one plane; two equal
planes), its gradient is checked against central differences of its own loss, the planes of the GPU tests' object are shown to
differ by far more than the GPU tests' bounds, and the keyword surface of every layer and the C symbol are checked."""
import numpy as np
import pytest

import reference_model as ref_model
from reference_model import rel

E, PS = 5000., 1e-7
DIST = (5e-5, 1e-4, 2e-4)


def _setup():
    return ref_model.setup(S=12)


@pytest.mark.parametrize('b', [1, 2])
@pytest.mark.parametrize('variant', ['numpy_skip_last', 'tf_all'])
def test_one_plane_is_the_single_distance_reference_exactly(variant, b):
    delta, beta, pr, pi, rng = _setup()
    ref, _ = ref_model.forward(delta, beta, pr, pi, E, PS, 1e-4, variant, b)
    d, _ = ref_model.forward(delta, beta, pr, pi, E, PS, [1e-4], variant, b)
    assert d.shape == (2, 1, 16, 16) and np.array_equal(d[:, 0], ref)
    meas = np.abs(ref) * np.abs(1 + 0.05 * rng.normal(size=ref.shape))
    rl, rgd, rgb, rgp, rd = ref_model.loss_and_grad(delta, beta, pr, pi, E, PS, meas, 1e-4, variant, b)
    loss, gd, gb, gp, dd = ref_model.loss_and_grad(delta, beta, pr, pi, E, PS, meas[:, None], [1e-4], variant, b)
    diffs = (abs(loss - rl), np.abs(gd - rgd).max(), np.abs(gb - rgb).max(), np.abs(gp - rgp).max(), np.abs(dd[:, 0] - rd).max())
    print('D = 1 against the single distance: differences', variant, b, diffs)
    assert diffs == (0.0, 0.0, 0.0, 0.0, 0.0), diffs


@pytest.mark.parametrize('b', [1, 2])
@pytest.mark.parametrize('variant', ['numpy_skip_last', 'tf_all'])
def test_two_equal_planes_are_one_plane(variant, b):
    """Two planes at the same distance with the same amplitudes: the mean over 2 B frames is the mean over B, and the two seeds,
    each half of the one plane's, add up to it."""
    delta, beta, pr, pi, rng = _setup()
    ref, _ = ref_model.forward(delta, beta, pr, pi, E, PS, 1e-4, variant, b)
    meas = np.abs(ref) * np.abs(1 + 0.05 * rng.normal(size=ref.shape))
    rl, rgd, rgb, _, _ = ref_model.loss_and_grad(delta, beta, pr, pi, E, PS, meas, 1e-4, variant, b)
    loss, gd, gb, _, d = ref_model.loss_and_grad(delta, beta, pr, pi, E, PS, np.stack([meas, meas], axis=1), [1e-4, 1e-4], variant, b)
    e = (abs(loss - rl) / abs(rl), rel(gd, rgd), rel(gb, rgb))
    print('two equal planes against one: loss / g_delta / g_beta rel', variant, b, e)
    assert np.array_equal(d[:, 0], d[:, 1])
    assert max(e) <= 1e-13, e


@pytest.mark.parametrize('b', [1, 2])
@pytest.mark.parametrize('variant', ['numpy_skip_last', 'tf_all'])
def test_reference_gradient_against_central_differences(variant, b):
    """16 x 16 x 12, B = 2, three planes: directional derivatives along six +-1 directions (three of delta, three of beta)
    against central differences (step 1e-7) of the reference's own loss, to 1e-6 — the bound and the draw-again rule of
    test_binning_reference.py (a direction nearly orthogonal to the gradient measures nothing and is drawn again; the criterion
    looks at the direction alone)."""
    delta, beta, pr, pi, rng = _setup()
    ref, _ = ref_model.forward(delta, beta, pr, pi, E, PS, DIST, variant, b)
    assert ref.shape == (2, 3, 16, 16)
    meas = np.abs(ref) * np.abs(1 + 0.05 * rng.normal(size=ref.shape))
    loss, gd, gb, gp, d = ref_model.loss_and_grad(delta, beta, pr, pi, E, PS, meas, DIST, variant, b)
    assert abs(loss - ref_model.loss_only(delta, beta, pr, pi, E, PS, meas, DIST, variant, b)) <= 1e-14 * abs(loss)
    assert rel(d, ref) <= 1e-15
    errs = []
    eps = 1e-7
    for which in (0, 1):
        for _ in range(3):
            g = gd if which == 0 else gb
            v = rng.choice([-1.0, 1.0], size=delta.shape)
            while abs(np.sum(g * v)) < 0.1 * np.linalg.norm(g):
                v = rng.choice([-1.0, 1.0], size=delta.shape)
            if which == 0:
                lp = ref_model.loss_only(delta + eps * v, beta, pr, pi, E, PS, meas, DIST, variant, b)
                lm = ref_model.loss_only(delta - eps * v, beta, pr, pi, E, PS, meas, DIST, variant, b)
            else:
                lp = ref_model.loss_only(delta, beta + eps * v, pr, pi, E, PS, meas, DIST, variant, b)
                lm = ref_model.loss_only(delta, beta - eps * v, pr, pi, E, PS, meas, DIST, variant, b)
            an = float(np.sum(g * v))
            errs.append(abs((lp - lm) / (2 * eps) - an) / abs(an))
    print('multi-distance reference, directional derivatives rel err', variant, b, errs)
    assert max(errs) <= 1e-6, errs


def test_planes_of_the_gpu_tests_object_differ():
    """What lets the GPU tests tell a wrong table or a dropped plane from the right result: on their weak 64 x 64 x 6 object
    neighbouring planes differ by at least 1e-4 in |d| (relative L2), 20 times the bound on the wave."""
    rng = np.random.default_rng(0)
    delta = rng.uniform(0, 2e-5, size=(2, 64, 64, 6))
    beta = 0.1 * delta
    d, _ = ref_model.forward(delta, beta, np.ones((64, 64)), np.zeros((64, 64)), E, PS, DIST)
    e = [rel(np.abs(d[:, j]), np.abs(d[:, j + 1])) for j in range(2)]
    ei = [rel(np.abs(d[:, j]) ** 2, np.abs(d[:, j + 1]) ** 2) for j in range(2)]
    meas = np.abs(d) * np.abs(1 + 0.05 * rng.normal(size=d.shape))
    _, gd3, _, _, _ = ref_model.loss_and_grad(delta, beta, np.ones((64, 64)), np.zeros((64, 64)), E, PS, meas, DIST)
    _, gd1, _, _, _ = ref_model.loss_and_grad(delta, beta, np.ones((64, 64)), np.zeros((64, 64)), E, PS, meas[:, 1:2], DIST[1:2])
    print('weak object, neighbouring planes: |d| rel', e, 'intensity rel', ei, 'three-plane gradient against the middle plane alone', rel(gd3, gd1))
    assert min(e) >= 1e-4, e
    assert rel(gd3, gd1) >= 1e-2


def test_distances_keyword():
    from beyond_dof_amd import util
    assert util.detector_distances(None) == (None, None) and util.detector_distances('inf') == ('inf', None)
    assert util.detector_distances(1e-4) == (1e-4, None)
    assert util.detector_distances([1e-4]) == (1e-4, None) and util.detector_distances(np.array([1e-4])) == (1e-4, None)
    assert util.detector_distances((5e-5, 1e-4))[1] == (5e-5, 1e-4)
    for bad in ([], [1e-4, None], [1e-4, 'inf'], [1e-4, 0.0], [1e-4, -1e-4], [1e-4, np.nan], [1e-4, np.inf], [[1e-4, 2e-4]], [1e-4] * 9, 'far'):
        with pytest.raises(ValueError, match='free_prop_cm'):
            util.detector_distances(bad)
    one, seq = util.Optics(E, PS, 1e-4, util.PI, 16, 16), util.Optics(E, PS, [1e-4], util.PI, 16, 16)
    assert one.det_nm == seq.det_nm and seq.n_planes == 1 and seq.det_planes_nm is None
    three = util.Optics(E, PS, DIST, util.PI, 16, 16)
    assert three.n_planes == 3 and three.det_planes_nm == tuple(z * 1e7 for z in DIST)


def test_planes_keywords_are_checked_before_anything_touches_a_file_or_a_gpu(tmp_path):
    from beyond_dof_amd.engine import check_model_options

    def check_planes_path(free_prop_cm, **path):
        return check_model_options(free_prop_cm=free_prop_cm, **path)
    from beyond_dof_amd.fullfield import reconstruct_fullfield
    from beyond_dof_amd.simulation import create_fullfield_data_numpy
    from beyond_dof_amd.solver import FullfieldSolver
    two = [5e-5, 1e-4]
    assert check_planes_path(None) == 1 and check_planes_path('inf') == 1 and check_planes_path(1e-4) == 1 and check_planes_path([1e-4]) == 1
    assert check_planes_path(two) == 2 and check_planes_path(two, detector_kernel='IR') == 2
    ff = dict(save_path=str(tmp_path), n_epochs=1, minibatch_size=1)
    for bad in ([1e-4, None], [1e-4, 'inf'], [0.0, 1e-4], [-1e-4, 1e-4], [1e-4, np.inf], [1e-4] * 9):
        with pytest.raises(ValueError, match='free_prop_cm'):
            check_planes_path(bad)
        with pytest.raises(ValueError, match='free_prop_cm'):
            reconstruct_fullfield('data.h5', free_prop_cm=bad, **ff)
        with pytest.raises(ValueError, match='free_prop_cm'):
            FullfieldSolver(16, 16, 16, 4, 2, E, PS, free_prop_cm=bad)
        with pytest.raises(ValueError, match='free_prop_cm'):
            create_fullfield_data_numpy(E, PS, bad, 4, 'phantom', str(tmp_path), 'data.h5')
    # what does not carry several planes, at every layer
    for kw in (dict(propagator='conv'), dict(adjoint_precision='float64'), dict(adjoint_precision='first-step'), dict(rotation='bilinear'),
               dict(detector_kernel='auto'), dict(probe_type='optimizable')):
        with pytest.raises(ValueError, match='detector planes'):
            reconstruct_fullfield('data.h5', free_prop_cm=two, **dict(ff, **kw))
    for kw in (dict(propagator='conv'), dict(adjoint64=True), dict(adjoint64='first'), dict(recompute=True),
               dict(rotation='bilinear', theta=np.zeros(4)), dict(detector_kernel='auto')):
        with pytest.raises(ValueError, match='detector planes'):
            FullfieldSolver(16, 16, 16, 4, 2, E, PS, free_prop_cm=two, **kw)
    for kw in (dict(propagator='conv'), dict(adjoint_precision='float64'), dict(rotation='bilinear'), dict(recompute=True), dict(adjoint64=True),
               dict(detector_kernel='auto')):
        with pytest.raises(ValueError, match='detector planes'):
            check_planes_path(two, **kw)
    # one plane given as a sequence is the scalar: nothing of the above applies to it
    assert check_planes_path([1e-4], propagator='conv', adjoint_precision='float64', rotation='bilinear', recompute=True, detector_kernel='auto') == 1


def test_set_detector_planes_symbol_is_bound_and_exported():
    import __graft_entry__ as entry
    from beyond_dof_amd import _lib, util
    assert 'bdof_set_detector_planes' in _lib.EXPORTED_SYMBOLS
    assert _lib.MAX_PLANES == util.MAX_DETECTOR_PLANES == 8
    entry.build()
    lib = _lib.load()
    assert hasattr(lib, 'bdof_set_detector_planes')
    assert lib.bdof_set_detector_planes(None, 2, None, None) != 0          # no context: an argument error, not a crash
