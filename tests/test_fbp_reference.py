"""The analytic start on the host (beyond_dof_amd/analytic.py) against the float64 restatement of tests/fbp_reference.py: the
ramp's transfer, the CTF inversion on data of its own linear model, the back-projection under the cube rotations, the angle
weights, the whole chain on the example's phantom, and the refusals."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fbp_reference as ref                        # noqa: E402
from beyond_dof_amd import analytic, util          # noqa: E402

ENERGY, PSIZE = 5000., 1e-7


def test_ramp_transfer_is_abs_f():
    """The DTFT of the taps is |f| on |f| <= 1/2.  Truncated at |m| <= M the missing odd taps contribute at most
    (2 / pi^2) sum_{odd m > M} 1 / m^2 <= (2 / pi^2) / (2 (M - 1)) = 1 / (pi^2 (M - 1))."""
    n = 1024
    M = n - 1
    h = analytic.ramp_taps(n)
    assert h.shape == (2 * n - 1,) and h[M] == 0.25 and h[M + 2] == 0 and h[M + 1] == h[M - 1] == -1 / np.pi ** 2
    m = np.arange(-M, M + 1)
    f = np.linspace(-0.5, 0.5, 401)
    H = (h[None, :] * np.cos(2 * np.pi * f[:, None] * m[None, :])).sum(axis=1)
    err = np.abs(H - np.abs(f)).max()
    print('ramp: max |H(f) - |f|| = {:.3e} at {} taps (bound {:.3e})'.format(err, 2 * n - 1, 1 / (np.pi ** 2 * (M - 1))))
    assert err <= 1 / (np.pi ** 2 * (M - 1))
    np.testing.assert_array_equal(ref.ramp_rows(np.eye(8)[:, :, None])[:, :, 0], analytic.ramp_taps(8)[(np.arange(8)[:, None] - np.arange(8)[None, :]) + 7])


@pytest.mark.parametrize('object_type', analytic.OBJECT_TYPES)
@pytest.mark.parametrize('fp', [1e-3, (5e-4, 1e-3, 2e-3)])
def test_ctf_inverts_its_linear_model(object_type, fp):
    """g^_d = C_d B^  ->  B^ sum C^2 / (sum C^2 + reg), to 1e-12 of the largest coefficient; D = 1 and 3"""
    nx, ny, depth = 12, 10, 8
    rng = np.random.default_rng(1)
    C, reg = analytic.ctf_transfer(nx, ny, ENERGY, PSIZE, fp, depth, 10., 1e-2, object_type)
    D = len(C)
    assert C.shape == (D, nx, ny) and D == (3 if isinstance(fp, tuple) else 1)
    k2 = 2 * 2 * np.pi / (1240. / ENERGY)
    assert reg == pytest.approx(1e-2 * D * k2 ** 2 * (101. if object_type == 'normal' else 1.), rel=1e-14)
    Bhat = np.fft.fft2(1e-3 / k2 * rng.normal(size=(2, nx, ny)))                 # contrasts of a few 1e-3 .. 1e-2
    g = np.fft.ifft2(C[None] * Bhat[:, None])                                 # (B, D, nx, ny); C is Hermitian, so g is real
    assert np.abs(g.imag).max() <= 1e-15 * np.abs(g.real).max()
    g = g.real
    assert np.abs(g).max() < 0.5
    filters = analytic.ctf_filters(nx, ny, ENERGY, PSIZE, fp, depth, 10., 1e-2, object_type)
    assert filters.dtype == np.complex128 and filters.shape == C.shape
    P = ref.ctf_invert(np.sqrt(1 + g), None, 1.0, filters)
    C2 = (np.abs(C) ** 2).sum(axis=0)
    want = Bhat * (C2 / (C2 + reg))[None]
    assert np.abs(np.fft.fft2(P) - want).max() <= 1e-12 * np.abs(want).max()
    # a scalar carrier divides out
    P2 = ref.ctf_invert(1.7 * np.sqrt(1 + g), None, 1.7 ** 2, filters)
    assert np.abs(P2 - P).max() <= 1e-12 * np.abs(P).max()
    # a masked pixel holding NaN changes nothing
    wgt = np.ones((nx, ny))
    wgt[3, 4] = wgt[0, 0] = 0
    m0 = np.sqrt(1 + g)
    m0[..., wgt == 0] = 0.3
    mn = m0.copy()
    mn[..., wgt == 0] = np.nan
    np.testing.assert_array_equal(ref.ctf_retrieve(mn, wgt, 1.0, filters), ref.ctf_retrieve(m0, wgt, 1.0, filters))


@pytest.mark.parametrize('object_type,real_form', [('normal', lambda chi: 10. * np.sin(chi) - np.cos(chi)), ('phase_only', np.sin),
                                                   ('absorption_only', lambda chi: -np.cos(chi))])
def test_ctf_transfer_on_a_symmetric_mesh(object_type, real_form):
    """an odd axis' mesh is symmetric: the transfer is the real 2k (r sin chi - cos chi), 2k sin chi, -2k cos chi, with
    z = free_prop + depth / 2; an even axis' mesh is not, and the transfer is complex there"""
    nx, ny, depth = 9, 7, 6
    lam, dz = 1240. / ENERGY, PSIZE * 1e7
    k = 2 * np.pi / lam
    C, _ = analytic.ctf_transfer(nx, ny, ENERGY, PSIZE, 2e-4, depth, 10., 1e-2, object_type)
    f2 = np.fft.ifftshift(np.linspace(-0.5 / dz, 0.5 / dz, nx))[:, None] ** 2 + np.fft.ifftshift(np.linspace(-0.5 / dz, 0.5 / dz, ny))[None, :] ** 2
    assert f2[0, 0] == 0
    chi = np.pi * lam * (2e-4 * 1e7 + depth * dz / 2) * f2
    assert np.abs(C[0] - 2 * k * real_form(chi)).max() <= 1e-12 * 2 * k * 11
    assert np.abs(analytic.ctf_transfer(8, 8, ENERGY, PSIZE, 2e-4, depth, 10., 1e-2, object_type)[0].imag).max() > 1e-3 * k
    np.testing.assert_array_equal(analytic.model_mesh(8, dz), np.fft.ifftshift(np.linspace(-0.5 / dz, 0.5 / dz, 8)))


def _cube_case(vol_shape, det_shape, rng):
    Ms = ref.cube_rotations()
    assert len(Ms) == 24
    ts = [rng.integers(-2, 3, size=3).astype(np.float64) + (np.array(vol_shape) // 2 - np.rint(M @ (np.array([det_shape[0], vol_shape[1], det_shape[1]]) // 2)))
          for M in Ms]
    rows = np.stack([np.concatenate([M, t[:, None]], axis=1).reshape(12) for M, t in zip(Ms, ts)])
    q = rng.integers(-9, 10, size=(24,) + tuple(det_shape)).astype(np.float64)
    return Ms, ts, rows, q


def test_backprojection_cube_rotations_exact():
    """signed permutations, integer offsets, integer frames: the bilinear back-projection IS an integer sum, taps outside count 0"""
    vol_shape, det_shape = (8, 8, 6), (7, 9)
    Ms, ts, rows, q = _cube_case(vol_shape, det_shape, np.random.default_rng(2))
    got, mag = ref.backproject(q, rows, np.ones(24), vol_shape)
    want = ref.integer_backprojection(q, Ms, ts, vol_shape)
    np.testing.assert_array_equal(got, want.astype(np.float64))
    # some taps do fall outside: a voxel that every angle reached would have 24 taps
    hits = ref.backproject(np.ones_like(q), rows, np.ones(24), vol_shape)[0]
    assert hits.min() < 24 and hits.max() == 24


def test_angle_weights():
    for theta, total in ((-np.linspace(0, 2 * np.pi, 24), np.pi), (np.linspace(0, np.pi, 13), np.pi), (np.linspace(0.2, 1.7, 9), 1.5)):
        w = analytic.angle_weights(theta)
        assert w.shape == theta.shape and np.all(w > 0)
        assert w.sum() == pytest.approx(total, rel=1e-14)
    w = analytic.angle_weights(-np.linspace(0, 2 * np.pi, 24))
    assert w[0] == pytest.approx(w[1] / 2) and w[-1] == pytest.approx(w[1] / 2)        # the doubled end angle halves itself
    shuffled = np.array([0.3, 0.1, 0.2, 0.0])
    np.testing.assert_allclose(analytic.angle_weights(shuffled)[np.argsort(shuffled)], analytic.angle_weights(np.sort(shuffled)))


def test_rotation_rows():
    shape, n = (6, 9, 8), 7
    theta = -np.linspace(0, np.pi, n)
    rows, ang = analytic.rotation_rows('trilinear', n, shape, theta, 0.2, 0.1, 4.5)
    np.testing.assert_array_equal(rows, util.rigid_geometry(theta, shape, 0.2, 0.1, 4.5))
    np.testing.assert_array_equal(ang, theta)
    rows, ang = analytic.rotation_rows('bilinear', n, shape, theta)
    np.testing.assert_array_equal(rows, util.rigid_geometry(theta, shape))
    rm = util.rigid_geometry(theta, shape).reshape(n, 3, 4)
    rows, ang = analytic.rotation_rows('trilinear', n, shape, None, rotation_matrices=rm)
    np.testing.assert_allclose(ang, theta, atol=1e-12)
    # 'nearest': the continuous map whose rounding is util.rotation_lookup's table, at that function's own angles
    rows, ang = analytic.rotation_rows('nearest', n, shape, theta)
    np.testing.assert_array_equal(ang, np.linspace(0, 2 * np.pi, n))
    ny, nx, nz = shape
    xs, zs = np.repeat(np.arange(nx), nz), np.tile(np.arange(nz), nx)
    for row, table in zip(rows.reshape(n, 3, 4), util.rotation_lookup(shape, n)):
        p = row[:, :3] @ np.stack([xs, zs, np.zeros_like(xs)]).astype(np.float64) + row[:, 3:4]
        assert np.abs(p[2]).max() == 0 and row[2, 2] == 1
        rounded = np.stack([np.clip(np.round(p[0]), 0, nx - 1), np.clip(np.round(p[1]), 0, nz - 1)], axis=1)
        near_half = (np.abs(p[:2] - np.floor(p[:2]) - 0.5) < 1e-9).any(axis=0)
        np.testing.assert_array_equal(rounded[~near_half], table[~near_half])
    with pytest.raises(ValueError):
        analytic.rotation_rows('cubic', n, shape, theta)


@pytest.mark.parametrize('case,geometry', [('nominal', {}), ('tilted', dict(axis_tilt=0.2, center=17.0))])
def test_end_to_end_phantom(case, geometry):
    """32^3, 24 angles over 2 pi, 5 keV, 1 nm, 10 um, beta = delta / 10, r = 10, eps = 1e-2: the analytic start correlates with the
    phantom to 0.97 at least and its data loss is at most 0.05 of the zero volume's.  Measured here (one run): nominal 0.9881 and
    0.0100, tilted 0.9902 and 0.0142."""
    n, n_theta, fp = 32, 24, 1e-3
    d = ref.phantom(n, np.random.default_rng(0))
    theta = -np.linspace(0, 2 * np.pi, n_theta)
    rows = util.rigid_geometry(theta, (n, n, n), **geometry)
    prj = ref.forward_amplitudes(d, 0.1 * d, rows, ENERGY, PSIZE, [fp])
    C, reg = analytic.ctf_transfer(n, n, ENERGY, PSIZE, fp, n, 10., 1e-2)
    delta, beta = ref.analytic_start(prj, rows, analytic.angle_weights(theta), C, reg, PSIZE, 10., (n, n, n))
    corr = np.corrcoef(delta.ravel(), d.ravel())[0, 1]
    dc, bc = np.clip(delta, 0, None), np.clip(beta, 0, None)
    loss = np.mean((ref.forward_amplitudes(dc, bc, rows, ENERGY, PSIZE, [fp]) - prj) ** 2) / np.mean((1.0 - prj) ** 2)
    print('analytic start, {}: delta correlation {:.4f}, relative L2 {:.3f}, data loss / zero-volume loss {:.4f}'.format(
        case, corr, np.linalg.norm(delta - d) / np.linalg.norm(d), loss))
    assert corr >= 0.97
    assert loss <= 0.05


def test_refusals():
    ok = dict(propagator='fft', probe_real=np.ones((4, 5)), probe_imag=np.zeros((4, 5)))
    assert analytic.check_analytic(**ok) == 1.0
    assert analytic.check_analytic('fft', 0.6 * np.ones((4, 5)), 0.8 * np.ones((4, 5))) == pytest.approx(1.0)
    assert analytic.check_analytic('fft', 2 * np.ones((4, 5)), None) == pytest.approx(4.0)
    with pytest.raises(ValueError, match='propagator'):
        analytic.check_analytic(**dict(ok, propagator='conv'))
    gauss = np.exp(-((np.arange(5) - 2.) ** 2) / 2)[None, :] * np.ones((4, 1))
    with pytest.raises(ValueError, match='plane-wave'):
        analytic.check_analytic('fft', gauss, np.zeros((4, 5)))
    with pytest.raises(ValueError, match='plane-wave'):
        analytic.check_analytic('fft', np.zeros((4, 5)), np.zeros((4, 5)))
    with pytest.raises(ValueError, match='delta_beta_ratio'):
        analytic.check_analytic(delta_beta_ratio=-1., **ok)
    for eps in (0., -1e-2, np.nan):
        with pytest.raises(ValueError, match='ctf_regularization'):
            analytic.check_analytic(ctf_regularization=eps, **ok)
    with pytest.raises(ValueError, match='object_type'):
        analytic.check_analytic(object_type='both', **ok)
    with pytest.raises(ValueError, match='far field'):
        analytic.check_analytic(free_prop_cm='inf', **ok)


def test_entry_points_refuse_strings():
    """an unknown initial_guess string, and the ptychography entry point, raise before any file is read or device touched"""
    from beyond_dof_amd.fullfield import reconstruct_fullfield
    from beyond_dof_amd.ptychography import reconstruct_ptychography
    with pytest.raises(ValueError, match="'ctf-fbp'"):
        reconstruct_fullfield('no_such_file.h5', initial_guess='paganin')
    for bad in ('3e-7', -1., np.nan, [1e-7]):
        with pytest.raises(ValueError, match='threshold'):
            reconstruct_fullfield('no_such_file.h5', initial_guess='ctf-fbp', write_support_mask=bad)
    with pytest.raises(ValueError, match='save_path'):
        reconstruct_fullfield('no_such_file.h5', initial_guess='ctf-fbp', write_support_mask=1e-7, save_path='no_such_directory')
    with pytest.raises(ValueError, match='ctf-fbp'):
        reconstruct_fullfield('no_such_file.h5', write_support_mask=1e-7)
    with pytest.raises(ValueError, match='full field'):
        reconstruct_ptychography('no_such_file.h5', [(0, 0)], (4, 4), (8, 8, 8), initial_guess='ctf-fbp')


def test_support_mask(tmp_path):
    from beyond_dof_amd.fullfield import _read_mask
    n = 16
    y, x, z = np.mgrid[:n, :n, :n].astype(np.float64)
    d = 1e-6 * np.exp(-((y - 8) ** 2 + (x - 8) ** 2 + (z - 8) ** 2) / (2 * 2.5 ** 2))
    d[3, 0, 0] = 1e-3                                            # a bright voxel outside the cylinder
    mask = analytic.support_mask(d, 3e-7, save_path=str(tmp_path))
    assert mask.dtype == np.float32 and mask.shape == d.shape and set(np.unique(mask)) == {0., 1.}
    assert mask[8, 8, 8] == 1 and mask[3, 0, 0] == 0 and mask[8, 1, 1] == 0 and mask[0, 8, 8] == 0
    # the blur is scipy.ndimage.gaussian_filter(mode='constant')'s: unit mass away from the edge, a 9-tap kernel at sigma 1
    one = np.zeros((n, n, n))
    one[8, 8, 8] = 1
    b = analytic._blur(one, 1)
    assert b.sum() == pytest.approx(1.0) and b[8, 8, 12] > 0 and b[8, 8, 13] == 0
    g = np.exp(-0.5 * np.arange(-4, 5) ** 2)
    assert b[8, 8, 8] == pytest.approx((g[4] / g.sum()) ** 3)
    np.testing.assert_array_equal(_read_mask(str(tmp_path), n), mask)
