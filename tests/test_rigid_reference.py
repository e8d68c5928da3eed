"""rotation='trilinear' without a GPU: the numpy restatement (tests/rigid_reference.py) against scipy and against the oracle's
bilinear rotation, its adjointness, util.rigid_geometry against matrices written by hand, the refusals of the Python layers,
the candidate box the adjoint kernel searches, and where the solver-level gradient bound of tests/test_gpu_rigid.py comes from."""
import numpy as np
import pytest

from oracle import bdof_oracle as orc

import gradient_cases as gc
import rigid_reference as rr
from beyond_dof_amd import util

X, Z, Y = 7, 9, 10
GEOMETRIES = [dict(theta=0.3), dict(theta=-1.1, axis_tilt=0.5), dict(theta=2.5, axis_roll=0.05), dict(theta=0.7, center=2.6),
              dict(theta=4.0, axis_tilt=-np.pi / 4, axis_roll=0.05, center=3.3), dict(theta=np.pi / 2, axis_tilt=np.pi / 2, center=2.5),
              dict(theta=0.0, axis_tilt=0.5, axis_roll=-0.2, center=4.75)]


def _prm(g, shape=(Y, X, Z)):
    g = dict(g)
    return util.rigid_geometry(g.pop('theta'), shape, **g)[0]


@pytest.mark.parametrize('g', GEOMETRIES, ids=[str(i) for i in range(len(GEOMETRIES))])
def test_restatement_against_scipy(g):
    """scipy.ndimage.affine_transform(order=1, mode='grid-constant', cval=0) on the [X][Z][Y] array with (M, t) is the same map"""
    from scipy import ndimage
    rng = np.random.default_rng(1)
    vol = 1.0 + rng.normal(size=(X, Z, Y, 2))
    prm = _prm(g)
    m = prm.reshape(3, 4)
    got = rr.rotate_rigid(vol, prm)                                             # [z][x][y][c]
    for c in range(2):
        want = ndimage.affine_transform(vol[..., c], m[:, :3], offset=m[:, 3], order=1, mode='grid-constant', cval=0.0)
        assert np.abs(got[..., c].transpose(1, 0, 2) - want).max() <= 1e-13


@pytest.mark.parametrize('theta', [0.3, -1.1, np.pi / 2, 2.5, 0.0])
def test_restatement_against_the_bilinear_oracle_at_zero_tilt_and_roll(theta):
    rng = np.random.default_rng(2)
    obj = 1.0 + rng.normal(size=(Y, X, Z, 2))
    prm = _prm(dict(theta=theta))
    assert np.abs(rr.rotate_volume(obj, prm) - orc.rotate_bilinear(obj, theta)).max() <= 1e-13
    g = rng.normal(size=(Y, X, Z, 2))
    assert np.abs(rr.rotate_volume_adjoint(g, prm) - orc.rotate_bilinear_adjoint(g, theta)).max() <= 1e-13


@pytest.mark.parametrize('g', GEOMETRIES, ids=[str(i) for i in range(len(GEOMETRIES))])
def test_adjointness(g):
    rng = np.random.default_rng(3)
    v, gr = rng.normal(size=(X, Z, Y, 2)), rng.normal(size=(Z, X, Y, 2))
    prm = _prm(g)
    lhs, rhs = np.sum(rr.rotate_rigid(v, prm) * gr), np.sum(v * rr.rotate_rigid_adjoint(gr, prm))
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0)
    # ... and of the float32 restatement to float32's accuracy, with the terms of the bound consistent with the reference
    ref, sg, swg, n = rr.adjoint_terms(gr, prm)
    assert np.abs(ref - rr.rotate_rigid_adjoint(gr, prm)).max() <= 1e-13 and n.max() >= 1 and np.all(swg <= sg + 1e-12)
    a32 = rr.rotate_rigid_adjoint(gr.astype(np.float32), prm, 'f32')
    assert np.all(np.abs(a32 - rr.rotate_rigid_adjoint(gr.astype(np.float32), prm)) <= rr.element_bound(sg, swg, n) * 1.01 + 1e-30)


def test_geometry_against_hand_written_matrices():
    for kw, M, t in rr.hand_written(X, Z, Y):
        prm = _prm(kw).reshape(3, 4)
        assert np.abs(prm[:, :3] - np.asarray(M, dtype=float)).max() <= 1e-15, kw
        assert np.abs(prm[:, 3] - t).max() <= 1e-14, kw


def test_geometry_is_rigid_and_a_shear_is_refused():
    th = -np.linspace(0, 2 * np.pi, 9)
    prm = util.rigid_geometry(th, (Y, X, Z), 0.5, 0.03, 2.4).reshape(9, 3, 4)
    M = prm[:, :, :3]
    assert np.abs(np.einsum('nji,njk->nik', M, M) - np.eye(3)).max() <= 1e-14 and np.all(np.abs(np.linalg.det(M) - 1) <= 1e-14)
    assert np.array_equal(util.check_rigid(prm, 9), prm.reshape(9, 12))
    sheared = prm.copy()
    sheared[4, 0, 1] += 1e-6
    with pytest.raises(ValueError, match='rigid'):
        util.check_rigid(sheared, 9)
    mirrored = prm.copy()
    mirrored[2, :, 0] *= -1
    with pytest.raises(ValueError, match='rigid'):
        util.check_rigid(mirrored, 9)
    with pytest.raises(ValueError, match='shape'):
        util.check_rigid(prm[:8], 9)


def test_solver_refusals_that_need_no_gpu():
    from beyond_dof_amd.solver import FullfieldSolver
    th = np.zeros(4)
    args = (64, 64, 64, 4, 2, 5000., 1e-7)
    with pytest.raises(ValueError, match="rotation must be 'nearest', 'bilinear' or 'trilinear'"):
        FullfieldSolver(*args, rotation='cubic')
    with pytest.raises(ValueError, match="needs the projection angles theta or rotation_matrices"):
        FullfieldSolver(*args, rotation='trilinear')
    sheared = util.rigid_geometry(th, (64, 64, 64)).reshape(4, 3, 4)
    sheared[1, 2, 0] = 0.01
    with pytest.raises(ValueError, match='rigid'):
        FullfieldSolver(*args, rotation='trilinear', rotation_matrices=sheared)
    with pytest.raises(ValueError, match='n_theta'):
        FullfieldSolver(*args, rotation='trilinear', theta=np.zeros(3))
    # slice binning, detector planes and the float64 paths keep to the rotation tables, with their present texts
    with pytest.raises(ValueError, match="slice_binning > 1 runs on the rotation tables"):
        FullfieldSolver(*args, rotation='trilinear', theta=th, slice_binning=2)
    with pytest.raises(ValueError, match="several detector planes run on the rotation tables"):
        FullfieldSolver(*args, rotation='trilinear', theta=th, free_prop_cm=[5e-5, 1e-4])
    with pytest.raises(ValueError, match="float64 paths"):
        FullfieldSolver(*args, rotation='trilinear', theta=th, adjoint64='first')


def test_ptycho_solver_refusals_that_need_no_gpu():
    from beyond_dof_amd.solver import PtychoSolver
    pr, pi = np.ones((32, 32)), np.zeros((32, 32))
    args = ((64, 64, 32), (32, 32), [(32, 32)], 4, 1, 5000., 1e-7, pr, pi)
    with pytest.raises(ValueError, match="rotation must be 'nearest' or 'trilinear'"):
        PtychoSolver(*args, rotation='bilinear')
    with pytest.raises(ValueError, match="needs the projection angles theta or rotation_matrices"):
        PtychoSolver(*args, rotation='trilinear')
    with pytest.raises(ValueError, match='n_theta'):
        PtychoSolver(*args, rotation='trilinear', theta=np.zeros(5))
    sheared = util.rigid_geometry(np.zeros(4), (64, 64, 32)).reshape(4, 3, 4)
    sheared[0, 0, 2] = 1e-3
    with pytest.raises(ValueError, match='rigid'):
        PtychoSolver(*args, rotation='trilinear', rotation_matrices=sheared)
    with pytest.raises(ValueError, match="slice_binning > 1 runs on the rotation tables"):
        PtychoSolver(*args, rotation='trilinear', theta=np.zeros(4), slice_binning=2, adjoint64=None)


def test_candidate_box_of_the_adjoint():
    """What k_rot_rigid_adjoint relies on: an output o that has voxel v' among its taps lies, with o* = M^T (v' - t), within
    sum_j |M_ji| <= sqrt(3) of o* on axis i, and in floor(o*) - 1 .. floor(o*) + 2 — over 200 random rigid maps"""
    rng = np.random.default_rng(5)
    dims = (6, 5, 7)
    for _ in range(200):
        M = rr.random_rigid(rng)
        t = rng.uniform(-2, 2, size=3) + (np.array(dims) - 1) / 2. - M @ ((np.array(dims) - 1) / 2.)
        prm = np.concatenate([M, t[:, None]], axis=1).reshape(-1)
        idx, w = rr.taps(prm, dims)
        o = np.stack(np.meshgrid(*[np.arange(n) for n in dims], indexing='ij'), axis=-1).astype(float)       # [x][z][y][3]
        r = np.abs(M).sum(axis=0)
        assert np.all(r <= np.sqrt(3) + 1e-12)
        for i in range(8):
            live = w[i] != 0
            k = idx[i][live]
            v = np.stack([k // (dims[1] * dims[2]), (k // dims[2]) % dims[1], k % dims[2]], axis=-1).astype(float)
            ostar = (v - t) @ M                                                                         # M^T (v' - t)
            d = o[live] - ostar
            assert np.all(np.abs(d) < r), np.abs(d).max(axis=0)
            off = o[live] - np.floor(ostar)
            assert off.min() >= -1 and off.max() <= 2


def test_signed_permutations_give_weights_of_zero_and_one():
    for M in rr.signed_permutations():
        prm = np.concatenate([M, np.array([[3], [-2], [1]])], axis=1).reshape(-1).astype(float)
        _, w = rr.taps(prm, (4, 5, 6), 'f32')
        assert set(np.unique(w)) <= {0.0, 1.0}


@pytest.mark.parametrize('fp', [1e-4, None])
def test_where_the_solver_gradient_bound_comes_from(fp):
    """gradient_cases.bound_rule on the float32 / complex64 restatement of the composed 64^3 case: the constant that
    tests/test_gpu_rigid.py holds the device to is what the rule gives here, on the CPU"""
    figure = rr.composed_figure(fp)
    print('composed float32 restatement, free_prop_cm', fp, 'worst gradient error', figure)
    assert gc.bound_rule(figure) <= rr.SOLVER_GRADIENT_BOUND
    assert figure <= 0.5 * rr.SOLVER_GRADIENT_BOUND


@pytest.mark.parametrize('psz', [32, 64])
def test_where_the_ptychography_gradient_bound_comes_from(psz):
    """the same rule on the float32 / complex64 restatement of the ptychography case (rotation, windows, far field)"""
    figure = rr.ptycho_composed_figure(psz)
    print('ptychography float32 restatement, probe', psz, 'worst gradient error', figure)
    assert gc.bound_rule(figure) == rr.PTYCHO_GRADIENT_BOUND[psz]
    assert figure <= 0.5 * rr.PTYCHO_GRADIENT_BOUND[psz]
