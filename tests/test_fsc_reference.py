"""The numpy restatement of the Fourier shell correlation (tests/fsc_reference.py) tested on its own, and the host functions of
beyond_dof_amd.resolution that need no device: thresholds and the resolution read off a curve."""
import warnings

import numpy as np
import pytest

import fsc_reference as fr

SHAPES = fr.SHAPES + [(12, 12, 12), (7, 9, 1), (4, 6, 10)]


def _white(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape), rng.standard_normal(shape)


@pytest.mark.parametrize('shape', SHAPES)
def test_integer_rule_is_the_rounded_radius(shape):
    """s = floor(rho + 1/2), rho = Nref |f|, wherever rho is more than 1e-6 from a shell boundary; (16, 12, 20) has 44 points ON one."""
    s, rho = fr.shell_grid(shape), fr.rho_grid(shape)
    on_boundary = np.abs(rho + 0.5 - np.round(rho + 0.5)) <= 1e-6
    assert np.array_equal(s[~on_boundary], np.floor(rho[~on_boundary] + 0.5).astype(np.int64))
    assert on_boundary.sum() == (44 if shape == (16, 12, 20) else 0)
    assert s.ravel()[0] == 0 and np.all(s >= 0)


@pytest.mark.parametrize('shape', fr.SHAPES)
def test_every_reported_shell_of_the_device_shapes_holds_ten_points(shape):
    nref = fr.geometry(shape)[0]
    count = np.bincount(fr.shell_grid(shape).ravel())
    assert count[1:nref // 2].min() >= 10


@pytest.mark.parametrize('shape', SHAPES)
def test_packed_transform_gives_both_channels(shape):
    d, b = _white(shape, 1)
    d, b = 1e-6 * d, 1e-7 * b
    for sep, packed in zip(fr.spectra(d, b), fr.spectra_packed(d, b)):
        assert np.abs(sep - packed).max() <= 1e-14 * np.abs(sep).max()


@pytest.mark.parametrize('shape', SHAPES)
def test_counts_and_parseval_over_all_shells(shape):
    a, b = _white(shape, 2), _white(shape, 3)
    sums = fr.shell_sums(a, b, fr.n_shells_all(shape))
    n = float(np.prod(shape))
    assert sums[:, 0].sum() == n
    for col, vol in ((2, a[0]), (3, b[0]), (5, a[1]), (6, b[1])):
        assert abs(sums[:, col].sum() - n * np.sum(vol ** 2)) <= 1e-12 * n * np.sum(vol ** 2)
    # dropped shells: the first rows do not change
    assert np.array_equal(fr.shell_sums(a, b, 3), sums[:3])


def test_known_values():
    shape = (16, 12, 20)
    a = _white(shape, 4)
    populated = fr.shell_sums(a, a)[:, 0] > 0
    for scale, want in ((1.0, 1.0), (-1.0, -1.0), (3.0, 1.0)):
        b = (scale * a[0], scale * a[1])
        for c in fr.curves(fr.shell_sums(a, b)):
            assert np.abs(c[populated] - want).max() <= 1e-14
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        zero = fr.curves(fr.shell_sums(a, (np.zeros(shape), np.zeros(shape))))
    assert all(np.all(c == 0) for c in zero)


@pytest.mark.parametrize('sigma', [0.5, 1.0])
def test_noise_lowers_every_shell_to_the_expected_value(sigma):
    """b = a + sigma noise on white a: every shell within 4 / sqrt(n_points) of 1 / sqrt(1 + sigma^2) (measured worst case:
    1.21 / sqrt(n_points))."""
    shape = (32, 32, 32)
    a, noise = _white(shape, 5), _white(shape, 6)
    sums = fr.shell_sums(a, (a[0] + sigma * noise[0], a[1] + sigma * noise[1]))
    for c in fr.curves(sums):
        assert np.all(np.abs(c - 1 / np.sqrt(1 + sigma ** 2)) <= 4 / np.sqrt(sums[:, 0]))


def test_threshold_curve():
    from beyond_dof_amd import resolution
    n = np.array([18., 200., 5000.])
    assert np.array_equal(resolution.threshold_curve(0.143, n), np.full(3, 0.143))
    assert np.array_equal(resolution.threshold_curve(0.5, n), np.full(3, 0.5))
    r = 1 / np.sqrt(n / 2)
    assert np.allclose(resolution.threshold_curve('half-bit', n), (0.2071 + 1.9102 * r) / (1.2071 + 0.9102 * r), rtol=1e-15)
    assert abs(float(resolution.threshold_curve('half-bit', 1e12)) - 0.2071 / 1.2071) < 1e-5       # many points: the half-bit level
    with pytest.raises(ValueError):
        resolution.threshold_curve('one-bit', n)


def test_resolution_of_a_made_up_curve():
    from beyond_dof_amd import resolution
    nref = 16
    # rows 0 .. 7: cross, P_a = P_b = 1 -> the curve is the cross column; delta falls linearly, beta stays at 1
    sums = np.zeros((nref // 2, 7))
    sums[:, 0] = 100
    sums[:, [2, 3, 5, 6]] = 1
    sums[:, 1] = [1.0, 0.9, 0.8, 0.7, 0.6, 0.4, 0.2, 0.0]
    sums[:, 4] = 1
    rec = resolution.record_from_sums(sums, nref, psize_cm=1e-7)
    assert np.array_equal(rec.shell, np.arange(1, 8)) and np.array_equal(rec.frequency, np.arange(1, 8) / 16.0)
    assert np.array_equal(rec.n_points, np.full(7, 100)) and np.array_equal(rec.fsc_delta, sums[1:, 1]) and np.all(rec.fsc_beta == 1)
    res = resolution.resolution(rec, 0.5)
    assert res['beta'] is None
    # 0.6 at shell 4, 0.4 at shell 5: the crossing of 0.5 is at 4.5
    assert abs(res['delta'].shell - 4.5) < 1e-12 and abs(res['delta'].frequency - 4.5 / 16) < 1e-15
    assert abs(res['delta'].half_period - 1e-7 * 16 / 9.0) < 1e-20
    assert abs(resolution.resolution(rec, 0.5, psize_cm=2e-7)['delta'].half_period - 2e-7 * 16 / 9.0) < 1e-20
    assert resolution.resolution(rec, 0.95)['delta'].shell == 1.0                # below at the first shell already
    # half-bit with 100 points per shell
    t = float(resolution.threshold_curve('half-bit', 100))
    want = 5 + (0.4 - t) / 0.2 if t < 0.4 else 4 + (0.6 - t) / 0.2
    assert abs(resolution.resolution(rec, 'half-bit')['delta'].shell - want) < 1e-12
    # a signed curve: a negative value is below every threshold
    sums[3, 1] = -0.5
    assert resolution.resolution(resolution.record_from_sums(sums, nref), 0.143)['delta'].shell < 3.0
    # zero power: the curve is 0 there, without a warning
    sums[2, [2, 5]] = 0
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert resolution.record_from_sums(sums, nref).fsc_delta[1] == 0


def test_shell_count_is_the_corner_shell_plus_one():
    from beyond_dof_amd import resolution
    for shape in SHAPES:
        assert resolution.shell_count(shape) == fr.n_shells_all(shape)
    with pytest.raises(ValueError):
        resolution.shell_count((1, 16, 1))


def test_mismatched_shapes_are_refused_on_the_host():
    """before any device work: the check needs no library"""
    from beyond_dof_amd import resolution
    a = (np.zeros((8, 8, 8)), np.zeros((8, 8, 8)))
    with pytest.raises(ValueError):
        resolution.fourier_shell_correlation(a, (np.zeros((8, 8, 6)), np.zeros((8, 8, 6))))
    with pytest.raises(ValueError):
        resolution.read_reference(a, (8, 8, 6))
    with pytest.raises(ValueError):
        resolution.fourier_ring_correlation(a, a)
