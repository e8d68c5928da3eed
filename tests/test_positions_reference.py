"""The float64 restatement of the fractional window cut (tests/positions_reference.py) against itself and against
reference_model.ptycho_loss_and_grad, and the host side of the feature (beyond_dof_amd/positions.py).  No GPU."""
import numpy as np
import pytest

import positions_reference as pr
import reference_model as ref_model

E_EV, PSIZE_CM = 5000., 1e-7
SHAPE, PSZ = (16, 18, 4), (8, 6)                                         # (Y, X, Z), (py, px)
POS = np.array([(5, 6), (9, 11), (8, 5), (14, 16)])                      # the last one overhangs


def _case(seed=3):
    from beyond_dof_amd import util
    from oracle import bdof_oracle as orc
    rng = np.random.default_rng(seed)
    od = rng.uniform(0, 2e-3, size=SHAPE)
    ob = rng.uniform(0, 2e-4, size=SHAPE)
    coord = util.rotation_lookup(SHAPE, 5)[1]
    probe_r, probe_i = orc.gaussian_probe(PSZ, 3., 3., 0.5)
    off = rng.uniform(-0.9, 0.9, size=(len(POS), 2))
    rot = pr.nearest(coord)
    wave = pr.ptycho_forward(od, ob, rot, POS, off, PSZ, probe_r, probe_i, E_EV, PSIZE_CM)
    meas = ref_model.measurement_wide(wave, 0)
    return dict(od=od, ob=ob, coord=coord, rot=rot, pr=probe_r, pi=probe_i, off=off, meas=meas)


def test_position_derivative_against_central_differences():
    """generic fractions: the analytic derivative of every offset to 1e-6 relative of central differences of the restatement's own loss"""
    c = _case()
    out = pr.ptycho_loss_and_grad(c['od'], c['ob'], c['rot'], POS, c['off'], PSZ, c['pr'], c['pi'], E_EV, PSIZE_CM, c['meas'])
    h = 1e-5
    floor = 1e-9 * np.abs(out['dpos']).max()          # (an entry may vanish: the nearest rotation repeats rows at the frame's edge)
    for b in range(len(POS)):
        for k in range(2):
            up, dn = c['off'].copy(), c['off'].copy()
            up[b, k] += h
            dn[b, k] -= h
            fd = (pr.ptycho_loss(c['od'], c['ob'], c['rot'], POS, up, PSZ, c['pr'], c['pi'], E_EV, PSIZE_CM, c['meas'])
                  - pr.ptycho_loss(c['od'], c['ob'], c['rot'], POS, dn, PSZ, c['pr'], c['pi'], E_EV, PSIZE_CM, c['meas'])) / (2 * h)
            print(b, k, 'analytic', out['dpos'][b, k], 'central differences', fd)
            assert abs(out['dpos'][b, k] - fd) <= 1e-6 * abs(fd) + floor, (b, k)


def test_zero_offsets_are_the_integer_model_exactly():
    c = _case()
    zero = np.zeros((len(POS), 2))
    out = pr.ptycho_loss_and_grad(c['od'], c['ob'], c['rot'], POS, zero, PSZ, c['pr'], c['pi'], E_EV, PSIZE_CM, c['meas'])
    loss, gd, gb = ref_model.ptycho_loss_and_grad(c['od'], c['ob'], c['coord'], POS, POS, c['meas'], c['pr'], c['pi'], PSZ, E_EV, PSIZE_CM)
    assert out['loss'] == float(loss)
    assert np.array_equal(out['gd'], gd) and np.array_equal(out['gb'], gb)


@pytest.mark.parametrize('origin', [[(2.3, 1.7), (5.5, -2.25)], [(3.0, 4.0), (-1.0, 2.0)], [(-2.3, 9.6), (11.5, 3.5)], [(40.0, 2.0), (-30.5, 1.0)]],
                         ids=['generic', 'integer', 'overhang', 'outside'])
def test_adjoint_identity(origin):
    rng = np.random.default_rng(5)
    S, VX, VY, NX, NY = 3, 12, 14, 8, 6
    v = rng.normal(size=(S, VX, VY, 2))
    g = rng.normal(size=(2, S, NX, NY, 2))
    lhs = np.sum(pr.window_cut(v, origin, NX, NY) * g)
    rhs = np.sum(v * pr.window_cut_adjoint(g, origin, VX, VY))
    scale = np.sum(np.abs(pr.window_cut(np.abs(v), origin, NX, NY) * np.abs(g)))
    assert abs(lhs - rhs) <= 1e-13 * max(scale, 1.0)
    if origin[0][0] == 40.0:
        assert lhs == 0.0 and not np.any(pr.window_cut_adjoint(g, origin, VX, VY))


def test_integer_origin_is_the_integer_cut_and_takes_the_right_hand_derivative():
    rng = np.random.default_rng(6)
    R = rng.normal(size=(2, 9, 10, 2))
    W = pr.window_cut(R, [(2.0, 3.0)], 4, 4)
    assert np.array_equal(W[0], R[:, 2:6, 3:7])
    g = rng.normal(size=(1, 2, 4, 4, 2))
    d = pr.position_terms(R, g, [(2.0, 3.0)])[0][0]
    h = 1e-6
    right = [(np.sum(pr.window_cut(R, [(2.0 + h * (k == 0), 3.0 + h * (k == 1))], 4, 4) * g) - np.sum(W * g)) / h for k in range(2)]
    assert np.allclose(d, right, rtol=1e-6, atol=1e-9)


# ---- ProbePositions ------------------------------------------------------------------------------------------------------------------
def test_an_entry_moves_only_when_listed():
    from beyond_dof_amd.positions import ProbePositions
    p = ProbePositions(3, 5, None, 'per_angle', rate=0.05)
    g = np.array([[1., -2.], [0.5, 0.25]])
    p.update(p.dense(g, 1, [0, 3]))
    moved = np.zeros((3, 5, 2), dtype=bool)
    moved[1, [0, 3]] = True
    assert np.array_equal(p.values() != 0, moved)
    # Adam's first step is rate * sign(g) (to eps)
    assert np.allclose(p.values()[1, [0, 3]], -0.05 * np.sign(g), rtol=1e-6)
    assert np.array_equal(p.t[1, [0, 3]], np.ones((2, 2))) and p.t.sum() == 4
    before = p.values()
    p.update(p.dense(g[:1], 2, [4]))
    after = p.values()
    assert np.array_equal(after[1], before[1]) and np.all(after[2, 4] != 0) and p.t[1, 0, 0] == 1 and p.t[2, 4, 0] == 1


def test_shared_sums_over_angles_and_moves_every_angle():
    from beyond_dof_amd.positions import ProbePositions
    start = np.arange(3 * 4 * 2, dtype=float).reshape(3, 4, 2) * 0.01
    p = ProbePositions(3, 4, start, 'shared', rate=0.1)
    a, b = p.dense(np.array([[1., 1.], [3., -1.]]), 0, [1, 2]), p.dense(np.array([[-2., 1.]]), 2, [1])
    g, seen = p.split(a + b)
    assert np.array_equal(g, [[0, 0], [-1., 2.], [3., -1.], [0, 0]]) and np.array_equal(seen, [False, True, True, False])
    # a position listed twice in one minibatch adds as well
    assert np.array_equal(p.split(p.dense(np.array([[1., 1.], [2., 2.]]), 0, [3, 3]))[0][3], [3., 3.])
    p.update((a + b) / 2)
    step = p.values() - start
    assert np.allclose(step[:, 1], [0.1, -0.1], rtol=1e-6) and np.allclose(step[:, 2], [-0.1, 0.1], rtol=1e-6) and not np.any(step[:, [0, 3]])


def _dense_before_hostopt(self, grad, i_theta, pos_idx):
    """ProbePositions.dense as it stood before hostopt.pack, verbatim"""
    full, seen = np.zeros(self.m.shape), np.zeros(self.m.shape[:-1])
    at = (np.asarray(pos_idx),) if self.mode == 'shared' else (np.full(len(pos_idx), int(i_theta)), np.asarray(pos_idx))
    np.add.at(full, at, np.asarray(grad, dtype=np.float64))
    seen[at] = 1.
    return np.concatenate([full.reshape(-1), seen.reshape(-1)])


def _split_before_hostopt(self, dense):
    n = self.m.size
    return dense[:n].reshape(self.m.shape), dense[n:].reshape(self.m.shape[:-1]) > 0


def _update_before_hostopt(self, dense, b1=0.9, b2=0.999, eps=1e-8):
    """ProbePositions.update as it stood before hostopt.MaskedAdam, verbatim"""
    g, seen = _split_before_hostopt(self, dense)
    move = np.repeat(seen[..., None], 2, axis=-1)
    self.t = self.t + move
    self.m = np.where(move, b1 * self.m + (1 - b1) * g, self.m)
    self.v = np.where(move, b2 * self.v + (1 - b2) * g * g, self.v)
    t = np.maximum(self.t, 1)
    step = np.where(move, self.rate * (self.m / (1 - b1 ** t)) / (np.sqrt(self.v / (1 - b2 ** t)) + eps), 0.)
    self.offset = self.offset - step


@pytest.mark.parametrize('mode', ['shared', 'per_angle'])
def test_masked_adam_has_the_bits_of_the_update_it_replaced(mode):
    """5 angles, 6 positions, six steps of random float64 gradients: position 5 is never listed, step 1 lists position 4 twice,
    step 2 lists nothing, steps 3 and 4 stand for a sum over two ranks (/ 2) that list different angles.  'shared' holds (n_pos, 2)
    entries against offsets (n_theta, n_pos, 2).  Offsets, m, v, t and the vector the ranks add: the same bits after every step."""
    import types
    from beyond_dof_amd import hostopt
    from beyond_dof_amd.positions import ProbePositions
    rng = np.random.default_rng(12)
    n_theta, n_pos = 5, 6
    start = rng.uniform(-0.9, 0.9, size=(n_theta, n_pos, 2))
    p = ProbePositions(n_theta, n_pos, start, mode, rate=0.07)
    shape = (n_pos, 2) if mode == 'shared' else (n_theta, n_pos, 2)
    assert isinstance(p.opt, hostopt.MaskedAdam) and p.m.shape == shape
    old = types.SimpleNamespace(mode=mode, rate=0.07, offset=start.copy(), m=np.zeros(shape), v=np.zeros(shape), t=np.zeros(shape, dtype=np.int64))
    listed = [(1, [0, 3]), (2, [4, 4]), (0, []), (1, [0, 1, 2]), (4, [3]), (2, [4, 0])]
    for step, (i_theta, pos_idx) in enumerate(listed):
        pos_idx = np.array(pos_idx, dtype=np.int64)
        grad = rng.normal(size=(len(pos_idx), 2))
        dense = _dense_before_hostopt(old, grad, i_theta, pos_idx)
        assert np.array_equal(p.dense(grad, i_theta, pos_idx), dense)
        if step in (3, 4):
            dense = (dense + _dense_before_hostopt(old, rng.normal(size=(2, 2)), 3, [2, 1 if step == 3 else 0])) / 2
        for a, b in zip(p.split(dense), _split_before_hostopt(old, dense)):
            assert np.array_equal(a, b)
        _update_before_hostopt(old, dense)
        p.update(dense)
        assert p.values().shape == (n_theta, n_pos, 2) and p.values().dtype == np.float64
        assert np.array_equal(p.values(), old.offset) and np.array_equal(p.m, old.m) and np.array_equal(p.v, old.v), step
        assert np.array_equal(p.t, old.t) and p.t.dtype == np.int64, step
    # steps that listed each position (under 'per_angle' summed over the angles, of which steps 3 and 4 list two)
    assert list(p.t[..., 0]) == [4, 1, 2, 2, 2, 0] if mode == 'shared' else list(p.t[..., 0].sum(axis=0)) == [4, 2, 3, 2, 2, 0]


def test_dense_vector_round_trip_and_level_units():
    from beyond_dof_amd import positions
    p = positions.ProbePositions(2, 3, None, 'per_angle')
    g = np.array([[0.5, -1.5], [2., 4.]])
    got, seen = p.split(p.dense(g, 1, [2, 0]))
    assert np.array_equal(got[1, [2, 0]], g) and seen.sum() == 2 and seen[1, 2] and seen[1, 0]
    off = np.array([[1.0, -3.0], [0.5, 0.25], [0., 2.]])
    assert np.array_equal(positions.to_level(off, 2), off / 2) and np.array_equal(positions.from_level(positions.to_level(off, 4), 4), off)
    assert np.array_equal(positions.ProbePositions(2, 3, off).values(), np.broadcast_to(off, (2, 3, 2)))
    line = positions.summary_line(np.zeros((2, 3, 2)), np.broadcast_to(off, (2, 3, 2)))
    assert line.startswith('refined_positions') and 'largest move 3.16228' in line


def test_check_positions_refusals():
    from beyond_dof_amd.positions import check_positions
    assert check_positions(None, None, 4, 3) is None
    assert np.array_equal(check_positions(None, 'shared', 4, 3), np.zeros((4, 2)))
    assert check_positions(np.zeros((3, 4, 2)), None, 4, 3).shape == (3, 4, 2)
    assert check_positions(np.zeros((4, 2)), 'per_angle', 4, 3, adjoint_precision='float32').shape == (4, 2)
    with pytest.raises(ValueError, match='refine_positions'):
        check_positions(None, 'every', 4, 3)
    for kw, word in ((dict(propagator='conv'), "propagator='conv'"), (dict(slice_binning=2), 'slice_binning'),
                     (dict(adjoint_precision='first-step'), 'adjoint_precision'), (dict(adjoint_precision='float64'), 'adjoint_precision')):
        with pytest.raises(ValueError, match='position_offsets.*' + word):
            check_positions(np.zeros((4, 2)), None, 4, 3, **kw)
        with pytest.raises(ValueError, match='refine_positions.*' + word):
            check_positions(None, 'shared', 4, 3, **kw)
    with pytest.raises(ValueError, match='refine_positions.*n_batch_per_update'):
        check_positions(None, 'per_angle', 4, 3, n_batch_per_update=2)
    assert check_positions(np.zeros((4, 2)), None, 4, 3, n_batch_per_update=2) is not None          # (fixed offsets accumulate freely)
    for shape in ((4,), (5, 2), (4, 3), (2, 4, 2), (3, 4, 3)):
        with pytest.raises(ValueError, match='position_offsets'):
            check_positions(np.zeros(shape), None, 4, 3)
    with pytest.raises(ValueError, match='position_offsets'):
        check_positions(np.full((4, 2), np.nan), None, 4, 3)


def test_the_solver_and_the_entry_point_refuse_before_anything_is_allocated():
    """no GPU here: a refusal that came after the first allocation would surface as a BdofError, not a ValueError"""
    from beyond_dof_amd.solver import PtychoSolver
    from beyond_dof_amd.ptychography import reconstruct_ptychography
    one = np.ones((8, 8))
    with pytest.raises(ValueError, match='position_offsets'):
        PtychoSolver((16, 16, 4), (8, 8), POS, 3, 4, E_EV, PSIZE_CM, one, 0 * one, position_offsets=np.zeros((3, 2)))
    with pytest.raises(ValueError, match='refine_positions.*adjoint_precision'):
        PtychoSolver((16, 16, 4), (8, 8), POS, 3, 4, E_EV, PSIZE_CM, one, 0 * one, refine_positions='shared', adjoint64='first')
    with pytest.raises(ValueError, match='refine_positions.*n_batch_per_update'):
        reconstruct_ptychography('nothing.h5', POS, (8, 8), (16, 16, 4), refine_positions='shared', n_batch_per_update=2)
    with pytest.raises(ValueError, match='position_offsets.*adjoint_precision'):
        reconstruct_ptychography('nothing.h5', POS, (8, 8), (16, 16, 4), position_offsets=np.zeros((4, 2)), adjoint_precision='first-step')


@pytest.mark.parametrize('kind', ['nearest', 'trilinear'])
def test_the_solver_level_bound_follows_the_restatement(kind):
    """the float32 / complex64 restatement of the GPU parity case stays under the bound the device is held to, and is what the
    reference file says it is"""
    vol, pos = pr.composed_figure(kind)
    print(kind, 'complex64 restatement: volume gradient', vol, 'position gradient / sum |terms|', pos, 'bound', pr.GRADIENT_BOUND)
    assert vol <= pr.GRADIENT_BOUND and pos <= pr.GRADIENT_BOUND
    assert vol <= 1.02 * pr.COMPOSED_FIGURE[kind][0] and pos <= 1.02 * pr.COMPOSED_FIGURE[kind][1]
