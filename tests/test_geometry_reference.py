"""The geometry gradient of rotation='trilinear' off the GPU: the float64 restatement of dL/d(M | t) (tests/geometry_reference.py)
against central differences of the pairing it differentiates, the host chain rule (util.rigid_geometry_gradient) against central
differences of util.rigid_geometry, the per-angle shifts, the right-derivative convention, the ValueErrors of refine_geometry that
need no device, and where the solver-level bounds of tests/test_gpu_geometry.py come from."""
import numpy as np
import pytest

import geometry_reference as gr
import gradient_cases as gc
import rigid_reference as rr

from beyond_dof_amd import rotation, util

DIMS = (12, 10, 14)             # (NX, NZ, NY)
H = 1e-6


def _case(seed):
    rng = np.random.default_rng(seed)
    NX, NZ, NY = DIMS
    vol = rng.normal(size=(NX, NZ, NY, 2))
    g = rng.normal(size=(NZ, NX, NY, 2))
    M = rr.random_rigid(rng)
    c = (np.array(DIMS) - 1) / 2.
    t = c - M @ c + rng.uniform(-1.5, 1.5, size=3)
    return vol, g, np.concatenate([M, t[:, None]], axis=1).reshape(-1)


@pytest.mark.parametrize('seed', [3, 4, 5])
def test_restatement_against_central_differences(seed):
    """no voxel changes its cell under +-h in any of the 12 entries (asserted), so the pairing is exactly linear in the entry there
    and the central difference is the derivative up to rounding: 1e-9 of the entry's sum of |terms|"""
    vol, g, prm = _case(seed)
    d, _, _, T = gr.param_terms(vol, g, prm)
    base = gr.cell(prm, DIMS)[0]
    worst = 0.0
    for k in range(12):
        e = np.zeros(12)
        e[k] = H
        for s in (prm + e, prm - e):
            assert all(np.array_equal(a, b) for a, b in zip(gr.cell(s, DIMS)[0], base)), 'a voxel changed its cell: choose another seed'
        fd = (gr.pairing(vol, g, prm + e) - gr.pairing(vol, g, prm - e)) / (2 * H)
        worst = max(worst, abs(fd - d[k // 4, k % 4]) / T[k // 4, k % 4])
    print('seed', seed, 'largest |fd - analytic| / sum |terms|', worst)
    assert worst <= 1e-9


def _geometry_loss(w, theta, shape, tilt, roll, center, shifts):
    return float(np.sum(w * util.rigid_geometry(theta, shape, tilt, roll, center, shifts)))


def test_chain_rule_against_central_differences():
    """every parameter, shifts included, for a listed subset of the angles (in an order of its own): 1e-7 relative, h = 1e-6"""
    rng = np.random.default_rng(0)
    shape, n = (14, 12, 10), 5
    theta = rng.uniform(-3, 3, size=n)
    tilt, roll, center = 0.4, -0.07, 4.3
    shifts = rng.uniform(-1, 1, size=(n, 2))
    index = np.array([3, 0, 4])
    dprm = rng.normal(size=(len(index), 12))
    w = np.zeros((n, 12))
    w[index] = dprm
    got = util.rigid_geometry_gradient(theta, shape, tilt, roll, center, shifts, dprm, index)
    L = lambda **kw: _geometry_loss(w, **dict(dict(theta=theta, shape=shape, tilt=tilt, roll=roll, center=center, shifts=shifts), **kw))
    worst = 0.0

    def held(name, analytic, plus, minus):
        nonlocal worst
        fd = (plus - minus) / (2 * H)
        err = abs(fd - analytic) / abs(fd)
        worst = max(worst, err)
        assert err <= 1e-7, (name, fd, analytic)
    held('axis_tilt', got['axis_tilt'], L(tilt=tilt + H), L(tilt=tilt - H))
    held('axis_roll', got['axis_roll'], L(roll=roll + H), L(roll=roll - H))
    held('center', got['center'], L(center=center + H), L(center=center - H))
    for k, i in enumerate(index):
        e = np.zeros(n)
        e[i] = H
        held('theta', got['theta'][k], L(theta=theta + e), L(theta=theta - e))
        for c in range(2):
            e2 = np.zeros((n, 2))
            e2[i, c] = H
            held('shifts', got['shifts'][k, c], L(shifts=shifts + e2), L(shifts=shifts - e2))
    print('largest relative error of the chain rule', worst)
    assert got['theta'].shape == (3,) and got['shifts'].shape == (3, 2)


def test_shifts_none_and_zero_give_the_same_rows_and_a_horizontal_shift_is_a_centre():
    theta = -np.linspace(0, 2 * np.pi, 7).astype(np.float32).astype(np.float64)
    shape = (14, 12, 10)
    for center in (None, 4.3):
        base = util.rigid_geometry(theta, shape, 0.5, 0.03, center)
        assert np.array_equal(util.rigid_geometry(theta, shape, 0.5, 0.03, center, None), base)
        assert np.array_equal(util.rigid_geometry(theta, shape, 0.5, 0.03, center, np.zeros((7, 2))), base)
        assert np.array_equal(util.rigid_prm(7, shape, theta, 0.5, 0.03, center, None, np.zeros((7, 2))), base)
    s = 0.75                                                  # (4.25 + 0.75 is exact in binary: the two rows agree bit for bit)
    sh = np.zeros((7, 2))
    sh[:, 0] = s
    assert np.array_equal(util.rigid_geometry(theta, shape, 0.5, 0.03, 4.25, sh), util.rigid_geometry(theta, shape, 0.5, 0.03, 4.25 + s))
    with pytest.raises(ValueError, match='shifts must have shape'):
        util.rigid_geometry(theta, shape, shifts=np.zeros((6, 2)))


@pytest.mark.parametrize('which', ['identity', 'quarter turn'])
def test_right_derivative_convention(which):
    """integer matrices and t: every fraction is exactly 0, every voxel sits on the lattice.  The restatement's dL/dt equals the
    one-sided difference to the right, (L(t + h) - L(t)) / h, and not the one to the left"""
    rng = np.random.default_rng(8)
    NX, NZ, NY = 6, 6, 8
    vol = rng.normal(size=(NX, NZ, NY, 2))
    g = rng.normal(size=(NZ, NX, NY, 2))
    M = np.eye(3) if which == 'identity' else np.array([[0., 1., 0.], [-1., 0., 0.], [0., 0., 1.]])
    c = np.array([2., 2., 3.])
    prm = np.concatenate([M, (c - M @ c)[:, None]], axis=1).reshape(-1)
    assert all(not np.any(f) for f in gr.cell(prm, (NX, NZ, NY))[1])
    d, _, _, T = gr.param_terms(vol, g, prm)
    h = 2.0 ** -20
    for a in range(3):
        e = np.zeros(12)
        e[4 * a + 3] = h
        L0 = gr.pairing(vol, g, prm)
        right, left = (gr.pairing(vol, g, prm + e) - L0) / h, (L0 - gr.pairing(vol, g, prm - e)) / h
        assert abs(right - d[a, 3]) <= 1e-9 * T[a, 3], (a, right, d[a, 3])
        assert abs(left - d[a, 3]) > 1e-3 * T[a, 3], (a, left, d[a, 3])


def test_refusals_before_a_device_is_opened():
    """the ValueErrors of refine_geometry that rotation.choose raises (the solvers call it before they allocate anything); gradient
    accumulation is refused by step(), which needs a device (tests/test_gpu_geometry.py)"""
    from beyond_dof_amd.solver import FullfieldSolver, PtychoSolver
    theta = np.linspace(0, 3, 4)
    mats = util.rigid_geometry(theta, (8, 8, 8)).reshape(4, 3, 4)
    ff = lambda **kw: FullfieldSolver(8, 8, 8, 4, 2, 5000., 1e-7, theta=theta, **kw)
    pt = lambda **kw: PtychoSolver((8, 8, 8), (4, 4), [(4, 4)], 4, 1, 5000., 1e-7, np.ones((4, 4)), np.zeros((4, 4)), theta=theta, **kw)
    for make in (ff, pt):
        with pytest.raises(ValueError, match="rotation='trilinear' only"):
            make(rotation='nearest', refine_geometry=('center',))
        with pytest.raises(ValueError, match='not together with rotation_matrices'):
            make(rotation='trilinear', rotation_matrices=mats, refine_geometry=('center',))
        with pytest.raises(ValueError, match='names out of'):
            make(rotation='trilinear', refine_geometry=('centre',))
    with pytest.raises(ValueError, match="rotation='trilinear' only"):
        ff(rotation='bilinear', refine_geometry=('theta',))
    assert rotation.check_refine('center', 'trilinear', None) == ('center',) and rotation.check_refine((), 'nearest', mats) == ()


def test_host_adam_moves_only_the_listed_angles_and_by_the_rate():
    """RigidGeometry.update: Adam's first step is rate * sign(g); a per-angle entry outside the step's angles stays, with its counter"""
    geo = rotation.RigidGeometry((16, 12, 10), np.linspace(0, 3, 5), 0.1, 0.0, None, refine=('center', 'theta', 'shifts'), rate=0.05)
    before = geo.values()
    assert before['center'] == 5.5
    index = np.array([1, 3])
    grad = dict(center=2.0, axis_tilt=9., axis_roll=9., theta=np.array([-1., 4.]), shifts=np.array([[1., -1.], [0.5, 2.]]))
    geo.update(geo.dense(grad, index))
    after = geo.values()
    assert np.isclose(after['center'], 5.5 - 0.05, rtol=0, atol=1e-9)
    assert np.allclose(after['theta'] - before['theta'], [0, 0.05 / 8, 0, -0.05 / 8, 0], rtol=0, atol=1e-10)
    assert np.allclose(after['shifts'], [[0, 0], [-0.05, 0.05], [0, 0], [-0.05, -0.05], [0, 0]], rtol=0, atol=1e-9)
    assert after['axis_tilt'] == before['axis_tilt'] and list(geo.t['theta']) == [0, 1, 0, 1, 0]
    assert np.array_equal(geo.prm(), util.rigid_geometry(after['theta'], (16, 12, 10), 0.1, 0.0, float(after['center']), after['shifts']))


def test_two_ranks_hold_the_same_geometry_after_the_sum():
    """what step() does across ranks, on the host: each rank's dense vector lists its own angles, the sum divided by the size goes to
    every rank's Adam — the ranks end with the same values, the angles of both have moved, a shared name took the mean gradient"""
    make = lambda: rotation.RigidGeometry((16, 12, 10), np.linspace(0, 3, 5), 0.1, 0.0, 6.0, refine=('center', 'theta'), rate=0.05)
    a, b = make(), make()
    ga = dict(center=3.0, axis_tilt=0., axis_roll=0., theta=np.array([1., -1.]), shifts=np.zeros((2, 2)))
    gb = dict(center=-1.0, axis_tilt=0., axis_roll=0., theta=np.array([2., 2.]), shifts=np.zeros((2, 2)))
    total = (a.dense(ga, np.array([0, 1])) + b.dense(gb, np.array([3, 4]))) / 2
    a.update(total)
    b.update(total)
    va, vb = a.values(), b.values()
    assert all(np.array_equal(va[k], vb[k]) for k in va)
    assert np.array_equal(np.nonzero(va['theta'] != np.linspace(0, 3, 5))[0], [0, 1, 3, 4])
    assert np.isclose(va['center'], 6.0 - 0.05, rtol=0, atol=1e-9) and np.isclose(a.m['center'], 0.1 * 1.0)


def _dense_before_hostopt(self, grad, index):
    """RigidGeometry.dense as it stood before hostopt.pack, verbatim"""
    parts = []
    for k in self.refine:
        full = np.zeros_like(self.value[k])
        if full.ndim:
            np.add.at(full, np.asarray(index), grad[k])
        else:
            full += grad[k]
        parts.append(full.reshape(-1))
    seen = np.zeros(self.n_theta)
    seen[np.asarray(index)] = 1.
    return np.concatenate(parts + [seen])


def _update_before_hostopt(self, dense, b1=0.9, b2=0.999, eps=1e-8):
    """RigidGeometry.update as it stood before hostopt.MaskedAdam, verbatim"""
    seen, at = dense[-self.n_theta:] > 0, 0
    for k in self.refine:
        g = dense[at:at + self.value[k].size].reshape(self.value[k].shape)
        at += self.value[k].size
        move = np.ones(self.value[k].shape, dtype=bool) if self.value[k].ndim == 0 else (seen if g.ndim == 1 else np.repeat(seen[:, None], 2, axis=1))
        self.t[k] = self.t[k] + move
        self.m[k] = np.where(move, b1 * self.m[k] + (1 - b1) * g, self.m[k])
        self.v[k] = np.where(move, b2 * self.v[k] + (1 - b2) * g * g, self.v[k])
        t = np.maximum(self.t[k], 1)
        step = self.rate[k] * (self.m[k] / (1 - b1 ** t)) / (np.sqrt(self.v[k] / (1 - b2 ** t)) + eps)
        self.value[k] = np.where(move, self.value[k] - step, self.value[k])


def test_masked_adam_has_the_bits_of_the_update_it_replaced():
    """all five names — scalars, (n,) and (n, 2), each at its own rate — over six steps of random float64 gradients: angle 4 is
    never listed, step 1 lists angle 3 twice, step 2 lists nothing (the scalars still move), steps 3 and 4 stand for a sum over two
    ranks (/ 2).  Value, m, v and t are the same bits after every step, and so is the vector the ranks add."""
    import types
    from beyond_dof_amd import hostopt
    rng = np.random.default_rng(11)
    n, names = 5, util.GEOMETRY_NAMES
    assert set(names) == {'center', 'axis_tilt', 'axis_roll', 'theta', 'shifts'}
    theta = rng.uniform(-3, 3, size=n)
    geo = rotation.RigidGeometry((16, 12, 10), theta, 0.1, -0.02, 5.25, refine=names, rate=0.05)
    assert len({geo.rate[k] for k in ('center', 'theta')}) == 2 and all(isinstance(o, hostopt.MaskedAdam) for o in geo.opt.values())
    old = types.SimpleNamespace(refine=names, n_theta=n, rate=dict(geo.rate), value=geo.values(), m={k: np.zeros_like(geo.value[k]) for k in names},
                                v={k: np.zeros_like(geo.value[k]) for k in names}, t={k: np.zeros(geo.value[k].shape, dtype=np.int64) for k in names})
    listed = [[1, 3], [3, 3], [], [0, 1, 3], [2], [1, 0]]
    for step, index in enumerate(listed):
        index = np.array(index, dtype=np.int64)
        grad = dict(center=rng.normal(), axis_tilt=rng.normal(), axis_roll=rng.normal(), theta=rng.normal(size=len(index)),
                    shifts=rng.normal(size=(len(index), 2)))
        dense = _dense_before_hostopt(old, grad, index)
        assert np.array_equal(geo.dense(grad, index), dense)
        if step in (3, 4):
            dense = (dense + _dense_before_hostopt(old, {k: 3 * g for k, g in grad.items()}, index)) / 2
        _update_before_hostopt(old, dense)
        geo.update(dense)
        for k in names:
            assert geo.value[k].shape == old.value[k].shape and geo.value[k].dtype == np.float64
            assert np.array_equal(geo.value[k], old.value[k]) and np.array_equal(geo.m[k], old.m[k]), (step, k)
            assert np.array_equal(geo.v[k], old.v[k]) and np.array_equal(geo.t[k], old.t[k]), (step, k)
    assert list(geo.t['theta']) == [2, 3, 1, 3, 0] and geo.t['center'] == 6 and np.array_equal(geo.value['theta'][4], theta[4])
    assert np.array_equal(geo.t['shifts'], np.repeat(geo.t['theta'][:, None], 2, axis=1))


# ---- where the solver-level bounds come from ---------------------------------------------------------------------------------------------
def test_where_the_geometry_gradient_bound_comes_from():
    """gradient_cases.bound_rule on the float32 / complex64 restatement of dL/d(M | t) of the composed 64^3 case, relative to every
    entry's sum of |terms| (the entries cancel to about a hundredth of it, which the second assertion records)"""
    figure = gr.geometry_composed_figure()
    ref = gr.solver_geometry_problem()
    print('float32 restatement of dL/dprm: worst |f32 - f64| / sum |terms|', figure, '; |entry| / sum |terms|', np.abs(ref['d'] / ref['T']).max())
    assert gc.bound_rule(figure) == gr.GEOMETRY_GRADIENT_BOUND
    assert np.abs(ref['d'] / ref['T']).max() < 0.1


def test_where_the_ptychography_geometry_gradient_bound_comes_from():
    figure = gr.ptycho_geometry_composed_figure(32)
    print('ptychography, float32 restatement of dL/dprm: worst |f32 - f64| / sum |terms|', figure)
    assert gc.bound_rule(figure) == gr.PTYCHO_GEOMETRY_GRADIENT_BOUND
