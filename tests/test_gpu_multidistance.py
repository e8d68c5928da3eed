"""Several detector planes per wavefield (bdof_set_detector_planes; free_prop_cm as a sequence of distances through MultisliceEngine,
FullfieldSolver, reconstruct_fullfield and the simulator) on the device, through the two engines that carry them, against the float64
reference of tests/reference_model.py.

Bounds: the ones tests/test_gpu_parity.py and tests/test_gpu_binning.py assert for the same single-plane cases — forward
intensities relative L2 1e-5, wave 5e-6, loss relative 1e-5, gradients relative L2 2e-4.  The planes run the same float32 line
transforms and table products as the one plane; the fan-in adds D float32 terms, about sqrt(D) 6e-8 relative.  Objects, probes and
measurements follow test_gpu_binning.py::_reference.  Every test prints what it measured before it asserts."""
import functools
import os
import re
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import bdof_oracle as orc

import poisson_reference as pref
import reference_model as ref_model
import weights_reference as wref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, PS, MU = 5000., 1e-7, 2e6
DIST = (5e-5, 1e-4, 2e-4)


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


@pytest.fixture(scope='module')
def engine_mod():
    import __graft_entry__ as entry
    entry.build()
    from beyond_dof_amd import engine
    return engine


def _probe(kind, Y, X, rng):
    if kind == 'plane':
        return np.ones((Y, X)), np.zeros((Y, X))
    if kind == 'gaussian':
        return orc.gaussian_probe((Y, X), Y / 10., Y / 10., 0.5)
    return 1 + 0.1 * rng.normal(size=(Y, X)), 0.1 * rng.normal(size=(Y, X))


POISSON = ref_model.data_term(pref.poisson_loss, pref.poisson_seed, MU)


@functools.lru_cache(maxsize=None)
def _reference(B, Y, X, S, dist, variant, probe, b=1, loss='lsq', seed=0):
    """Object, probe, measurement (B, D, Y, X) and the float64 reference of one case, computed once and shared (read only)."""
    rng = np.random.default_rng(seed)
    delta = rng.uniform(0, 2e-5, size=(B, Y, X, S))
    beta = 0.1 * delta
    pr, pi = _probe(probe, Y, X, rng)
    ref, _ = ref_model.forward(delta, beta, pr, pi, E, PS, dist, variant, b)
    meas = np.abs(ref) * np.abs(1 + 0.05 * rng.normal(size=ref.shape))
    rl, rgd, rgb, _, _ = ref_model.loss_and_grad(delta, beta, pr, pi, E, PS, meas, dist, variant, b,
                                                 term=POISSON if loss == 'poisson' else ref_model.lsq)
    out = (delta, beta, pr, pi, meas, ref, rl, rgd, rgb)
    for a in out[:6] + out[7:]:
        a.setflags(write=False)
    return out


def _engine(engine_mod, engine, B, Y, X, S, dist, variant, case, b=1, loss='lsq'):
    delta, beta, pr, pi = case[:4]
    eng = engine_mod.MultisliceEngine(Y, X, S, B, with_grad=True, engine=engine, slice_binning=b)
    if loss == 'poisson':
        eng.set_loss('poisson', MU)
    eng.set_physics(E, PS, list(dist), variant=variant)
    assert eng.n_planes == len(dist)
    eng.set_probe(pr, pi)
    eng.set_object_batch(delta, beta)
    return eng


def _errors(wave, lossv, gd, gb, case):
    ref, rl, rgd, rgb = case[5:]
    return (rel(np.abs(wave) ** 2, np.abs(ref) ** 2), rel(wave, ref), abs(lossv - rl) / abs(rl), rel(gd, rgd), rel(gb, rgb))


def _within_bounds(e):
    assert e[0] <= 1e-5 and e[1] <= 5e-6, e
    assert e[2] <= 1e-5, e
    assert e[3] <= 2e-4 and e[4] <= 2e-4, e


def _run_and_check(engine_mod, tag, engine, B, Y, X, S, dist, variant, probe, b=1, loss='lsq', prepare=None):
    case = _reference(B, Y, X, S, tuple(dist), variant, probe, b, loss)
    eng = _engine(engine_mod, engine, B, Y, X, S, dist, variant, case, b, loss)
    if prepare:
        prepare(eng)
    wave = eng.forward(B)
    assert wave.shape == (B, len(dist), Y, X)
    lossv = eng.loss_grad(B, case[4])
    gd, gb = eng.grad_batch_to_host(B)
    e = _errors(wave, lossv, gd, gb, case)
    print('planes', tag, engine, (Y, X, S), 'D', len(dist), 'b', b, probe, variant, loss, 'intensity / wave / loss / g_delta / g_beta rel err', e)
    _within_bounds(e)
    return eng, (wave, lossv, gd, gb)


ENGINE_SHAPES = [('streaming', 64, 64), ('streaming', 64, 256), ('generic', 64, 64), ('generic', 96, 80)]


@pytest.mark.parametrize('engine,Y,X', ENGINE_SHAPES)
@pytest.mark.parametrize('D', [2, 3])
@pytest.mark.parametrize('probe', ['plane', 'random'])
@pytest.mark.parametrize('variant', ['numpy_skip_last', 'tf_all'])
def test_engine_vs_reference(engine_mod, engine, Y, X, D, probe, variant):
    """'plane': the scalar carrier with residual splitting, per plane the carrier times that plane's DC value; 'random': a
    structured probe on its mean as the scalar carrier — with several planes MultisliceEngine takes the deviation from the mean
    in RMS (0.14 here), where one plane's rule, the largest deviation (0.4), would put this probe on a carrier field."""
    _run_and_check(engine_mod, 'parity', engine, 2, Y, X, 6, DIST[:D], variant, probe)


@pytest.mark.parametrize('n', [64, 128, 256, 512, 1024])
def test_every_streaming_plan_once(engine_mod, n):
    """Up to 256 points the fan-out keeps a line's spectrum across the planes, from 512 on it reads the line again per plane."""
    _run_and_check(engine_mod, 'plans', 'streaming', 1, n, n, 4, DIST[:2], 'numpy_skip_last', 'plane')


def test_sweep_forms(engine_mod):
    """64 x 64, D = 3: the two-kernel sweep, the fused forward sweep and the fused forward + adjoint sweeps all end in the same
    fan-out / fan-in; each within the bounds of the reference, and so are the fused results measured against the unfused ones."""
    got = {}
    for name, fwd, adj in (('two-kernel', 0, False), ('fused forward', 1, False), ('fused forward + adjoint', 1, True)):
        def prepare(eng, fwd=fwd, adj=adj):
            eng.set_sweep_fusion(fwd)
            eng.set_adjoint_fusion(adj)
        eng, got[name] = _run_and_check(engine_mod, name, 'streaming', 2, 64, 64, 6, DIST, 'numpy_skip_last', 'random', prepare=prepare)
        assert eng.lib.bdof_sweep_fused(eng.h) == fwd and eng.lib.bdof_adjoint_fused(eng.h) == int(adj), name
    base = got['two-kernel']
    for name in ('fused forward', 'fused forward + adjoint'):
        w, l, gd, gb = got[name]
        e = (rel(np.abs(w) ** 2, np.abs(base[0]) ** 2), rel(w, base[0]), abs(l - base[1]) / abs(base[1]), rel(gd, base[2]), rel(gb, base[3]))
        print('planes', name, 'against the two-kernel sweep: intensity / wave / loss / g_delta / g_beta rel', e)
        _within_bounds(e)


@pytest.mark.parametrize('engine,Y,X', [('streaming', 64, 64), ('generic', 96, 80)])
def test_planes_with_the_poisson_loss(engine_mod, engine, Y, X):
    _run_and_check(engine_mod, 'poisson', engine, 2, Y, X, 6, DIST[:2], 'numpy_skip_last', 'plane', loss='poisson')


@pytest.mark.parametrize('engine,Y,X', [('streaming', 64, 64), ('generic', 96, 80)])
def test_planes_with_slice_binning(engine_mod, engine, Y, X):
    _run_and_check(engine_mod, 'slice binning', engine, 2, Y, X, 6, DIST[:2], 'tf_all', 'random', b=2)


@pytest.mark.parametrize('engine,Y,X', [('streaming', 64, 64), ('generic', 96, 80)])
@pytest.mark.parametrize('loss', ['lsq', 'poisson'])
def test_planes_with_detector_weights(engine_mod, engine, Y, X, loss):
    """One weight plane shared by both detector planes, with a block of zeros: against the weighted reference, and NaN in the
    amplitudes under w = 0 — in every plane — changes nothing, bit for bit."""
    B, S, dist = 2, 6, DIST[:2]
    delta, beta, pr, pi, meas = _reference(B, Y, X, S, dist, 'numpy_skip_last', 'plane')[:5]
    rng = np.random.default_rng(5)
    w = rng.uniform(0.25, 1.75, size=(Y, X))
    w[10:20, 30:45] = 0
    term = ref_model.data_term(wref.weighted_loss, wref.weighted_seed, w, loss, MU)
    rl, rgd, rgb, _, _ = ref_model.loss_and_grad(delta, beta, pr, pi, E, PS, meas, dist, term=term)
    eng = engine_mod.MultisliceEngine(Y, X, S, B, with_grad=True, engine=engine)
    eng.set_loss(loss, MU)
    eng.set_physics(E, PS, list(dist))
    eng.set_detector_weights(w)
    eng.set_probe(pr, pi)
    eng.set_object_batch(delta, beta)
    lossv = eng.loss_grad(B, meas)
    gd, gb = eng.grad_batch_to_host(B)
    e = (abs(lossv - rl) / abs(rl), rel(gd, rgd), rel(gb, rgb))
    print('planes with detector weights', engine, (Y, X), loss, 'loss / g_delta / g_beta rel err', e)
    assert e[0] <= 1e-5 and e[1] <= 2e-4 and e[2] <= 2e-4, e
    dirty = np.array(meas)
    dirty[:, :, 10:20, 30:45] = np.nan
    loss2 = eng.loss_grad(B, dirty)
    gd2, gb2 = eng.grad_batch_to_host(B)
    same = (loss2 == lossv, np.array_equal(gd2, gd), np.array_equal(gb2, gb))
    print('NaN under w = 0 in both planes: loss / g_delta / g_beta identical', same)
    assert all(same)


@pytest.mark.parametrize('engine,Y,X', [('streaming', 64, 256), ('generic', 96, 80)])
def test_one_plane_as_a_sequence_is_bit_identical_to_the_scalar(engine_mod, engine, Y, X):
    """free_prop_cm=[1e-4] gives the bits of free_prop_cm=1e-4; so does a context whose planes were set and then cleared by
    bdof_set_detector_planes(ctx, 1, ...) or by NULL tables."""
    B, S, variant = 2, 6, 'numpy_skip_last'
    delta, beta, pr, pi, meas = _reference(B, Y, X, S, (1e-4,), variant, 'random')[:5]
    got = []
    for how in ('scalar', 'sequence', 'cleared by D = 1', 'cleared by NULL'):
        eng = engine_mod.MultisliceEngine(Y, X, S, B, with_grad=True, engine=engine)
        if how.startswith('cleared'):
            eng.set_physics(E, PS, list(DIST), variant=variant)
            tables = np.zeros((1, X, Y), dtype=np.complex64)
            dcs = np.ones((1, 2))
            if how.endswith('D = 1'):
                eng.ctx.check(eng.lib.bdof_set_detector_planes(eng.h, 1, tables.ctypes.data, dcs.ctypes.data))
            else:
                eng.ctx.check(eng.lib.bdof_set_detector_planes(eng.h, 3, None, None))
            # the library is back to one plane, that of bdof_set_physics: DIST[0]; bind that distance's host state
            eng.n_planes = 1
            fp = DIST[0]
        else:
            fp = 1e-4 if how == 'scalar' else [1e-4]
            eng.set_physics(E, PS, fp, variant=variant)
        assert eng.n_planes == 1
        eng.set_probe(pr, pi)
        eng.set_object_batch(delta, beta)
        wave = eng.forward(B)
        assert wave.shape == (B, Y, X)
        m = meas[:, 0]
        loss = eng.loss_grad(B, m)
        got.append((how, fp, wave, loss) + tuple(eng.grad_batch_to_host(B)))
        if how == 'sequence':
            assert eng.loss_grad(B, meas) == loss             # (B, 1, Y, X) amplitudes are taken as well
    for ref_i, other_i in ((0, 1), (2, 3)):
        same = [np.array_equal(np.asarray(a), np.asarray(c)) for a, c in zip(got[ref_i][2:], got[other_i][2:])]
        print(got[other_i][0], 'against', got[ref_i][0], engine, (Y, X), 'wave / loss / g_delta / g_beta identical:', same)
        assert all(same)
    # the cleared contexts against a scalar engine at the distance bdof_set_physics holds
    eng = engine_mod.MultisliceEngine(Y, X, S, B, with_grad=True, engine=engine)
    eng.set_physics(E, PS, DIST[0], variant=variant)
    eng.set_probe(pr, pi)
    eng.set_object_batch(delta, beta)
    wave = eng.forward(B)
    loss = eng.loss_grad(B, meas[:, 0])
    fresh = (wave, loss) + tuple(eng.grad_batch_to_host(B))
    same = [np.array_equal(np.asarray(a), np.asarray(c)) for a, c in zip(fresh, got[2][2:])]
    print('planes set and cleared against a context that never had them', engine, (Y, X), 'wave / loss / g_delta / g_beta identical:', same)
    assert all(same)


@pytest.mark.parametrize('engine,Y,X', [('streaming', 64, 64), ('generic', 96, 80)])
def test_batch_layout_plane_order_and_isolation(engine_mod, engine, Y, X):
    B, S, variant = 2, 6, 'numpy_skip_last'
    case = _reference(B, Y, X, S, DIST, variant, 'plane')
    delta, beta, pr, pi, meas, ref, rl = case[:7]
    eng = _engine(engine_mod, engine, B, Y, X, S, DIST, variant, case)
    wave = eng.forward(B)
    # a batch of one on the same context: wavefield 0's planes, bit for bit (frames are [B][D]: nothing of wavefield 1 moves them)
    first = eng.forward(1)
    print('planes of wavefield 0: batch of 2 against batch of 1 identical', np.array_equal(first[0], wave[0]))
    assert first.shape == (1, 3, Y, X) and np.array_equal(first[0], wave[0])
    # wavefield 1 bound alone on a context of its own (another mean-refraction carrier: to the bound on the wave)
    solo = engine_mod.MultisliceEngine(Y, X, S, 1, with_grad=True, engine=engine)
    solo.set_physics(E, PS, list(DIST), variant=variant)
    solo.set_probe(pr, pi)
    solo.set_object_batch(delta[1:], beta[1:])
    e = rel(solo.forward(1)[0], wave[1])
    print('planes of wavefield 1: batch of 2 against a context of its own, rel', e)
    assert e <= 5e-6
    # the reversed list gives the reversed planes
    eng.set_physics(E, PS, list(DIST[::-1]), variant=variant)
    back = eng.forward(B)
    same = [np.array_equal(back[:, j], wave[:, 2 - j]) for j in range(3)]
    print('reversed distances give the reversed planes', same)
    assert all(same)
    # perturbing the amplitudes of one plane alone moves the loss by what the reference says
    eng.set_physics(E, PS, list(DIST), variant=variant)
    base = eng.loss_grad(B, meas)
    for j in range(3):
        pert = np.array(meas)
        pert[:, j] *= 1.02
        rl_pert = float(np.mean((np.abs(ref) - pert) ** 2))
        want, got = rl_pert - rl, eng.loss_grad(B, pert) - base
        print('plane', j, 'amplitudes * 1.02: loss change', got, 'reference', want, 'difference', abs(got - want))
        assert abs(got - want) <= 1e-5 * (rl_pert + rl)            # each of the two losses to the bound on a loss


def test_fullfield_solver_with_two_planes(engine_mod):
    """FullfieldSolver at 64^3, 8 angles, minibatch 4, D = 2: forward_angles, loss_and_grad and gradient_to_host against the
    reference with the rotation and its adjoint, to the bounds of test_fullfield_solver_rotation_table_path; one step moves the
    volume and leaves it finite."""
    from beyond_dof_amd.solver import FullfieldSolver
    n, n_theta, mb, dist = 64, 8, 4, DIST[:2]
    rng = np.random.default_rng(0)
    od = rng.uniform(0, 2e-5, size=(n, n, n))
    ob = 0.1 * od
    coords = orc.rotation_lookup([n, n, n], n_theta)
    idx = np.sort(rng.choice(n_theta, mb, replace=False))
    one, zero = np.ones((n, n)), np.zeros((n, n))
    rot = np.stack([orc.apply_rotation(np.stack([od, ob], axis=3), coords[j]) for j in idx])
    ref, _ = ref_model.forward(rot[..., 0], rot[..., 1], one, zero, E, PS, dist)
    prj = np.zeros((n_theta, 2, n, n))
    prj[idx] = (np.abs(ref) * np.abs(1 + 0.05 * rng.normal(size=ref.shape))).astype(np.float32)
    s = FullfieldSolver(n, n, n, n_theta, mb, E, PS, free_prop_cm=list(dist), coord_ls=coords)
    assert s.n_planes == 2 and s.eng.n_planes == 2
    s.set_volume(od, ob)
    s.set_measurements(prj)
    w = s.forward_angles(idx)
    assert w.shape == (mb, 2, n, n)
    loss = s.loss_and_grad(idx)
    gd, gb = s.gradient_to_host()
    rl, rgd, rgb, _ = ref_model.fullfield_loss_and_grad(od, ob, coords, idx, prj[idx], one, zero, E, PS, dist)
    e = (rel(np.abs(w) ** 2, np.abs(ref) ** 2), abs(loss - rl) / abs(rl), rel(gd, rgd), rel(gb, rgb))
    print('planes, full-field solver 64^3, D = 2: intensity / loss / g_delta / g_beta rel err', e)
    assert e[0] <= 1e-5 and e[1] <= 1e-5 and e[2] <= 2e-4 and e[3] <= 2e-4, e
    s.reset_moments()
    s.step(0, idx, 1e-7)
    d1, b1 = s.get_volume()
    moved = float(np.abs(d1 - od).max())
    print('one step: finite', bool(np.isfinite(d1).all() and np.isfinite(b1).all()), 'largest change of delta', moved)
    assert np.isfinite(d1).all() and np.isfinite(b1).all() and moved > 0


def _losses_printed(text):
    return [float(v) for v in re.findall(r'Epoch \d+ \(rank 0\); loss = ([-+.\deE]+|nan|inf)', text)]


def test_simulator_and_entry_point_with_two_planes(engine_mod, tmp_path, monkeypatch, capsys):
    """create_fullfield_data_numpy with two distances writes (n_theta, 2, Y, X); reconstruct_fullfield on that file at 64^3 for two
    epochs runs, writes its outputs, and its loss falls; a file whose shape does not fit the distances is refused with both shapes."""
    from beyond_dof_amd import h5io, simulation, tiffio
    from beyond_dof_amd.fullfield import reconstruct_fullfield
    monkeypatch.chdir(tmp_path)
    n, n_theta, mb, dist = 64, 8, 4, [5e-5, 1e-4]
    rng = np.random.default_rng(11)
    z, y, x = np.mgrid[:n, :n, :n]
    true_d = np.zeros((n, n, n))
    for _ in range(6):
        c = rng.uniform(n * 0.3, n * 0.7, size=3)
        r = rng.uniform(n * 0.08, n * 0.2)
        true_d += 1e-6 * np.exp(-((z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2) / (2 * r ** 2))
    os.makedirs('phantom')
    np.save('phantom/grid_delta.npy', true_d)
    np.save('phantom/grid_beta.npy', 0.1 * true_d)
    dat = simulation.create_fullfield_data_numpy(E, PS, dist, n_theta, 'phantom', 'case', 'data.h5', batch_size=4)
    on_disk = np.asarray(h5io.read_dataset('case/data.h5'))
    print('simulated data', dat.shape, dat.dtype, 'on disk', on_disk.shape)
    assert dat.shape == (n_theta, 2, n, n) and on_disk.shape == (n_theta, 2, n, n)
    one = simulation.create_fullfield_data_numpy(E, PS, dist[1], n_theta, 'phantom', 'case', 'one.h5', batch_size=4)
    e = rel(dat[:, 1], one)
    print('plane 1 of the two-plane data against a single-distance simulation at its distance, rel', e)
    assert one.shape == (n_theta, n, n) and e <= 1e-5              # each of the two within the bound on a wave, 5e-6
    init = [np.full((n, n, n), 8.7e-7), np.full((n, n, n), 5.1e-8)]
    kw = dict(theta_st=0, theta_end=2 * np.pi, n_epochs=2, learning_rate=1e-7, minibatch_size=mb, energy_ev=E, psize_cm=PS, save_path='case',
              shrink_cycle=None, seed=7, alpha_d=0., alpha_b=0., gamma=0., initial_guess=init)
    capsys.readouterr()
    rd, rb = reconstruct_fullfield('data.h5', free_prop_cm=dist, output_folder='out', **kw)
    losses = _losses_printed(capsys.readouterr().out)
    print('reconstruct_fullfield with two planes: losses per epoch', losses)
    assert len(losses) == 2 and np.isfinite(losses).all() and losses[1] < losses[0]
    assert np.isfinite(rd).all() and np.isfinite(rb).all() and rd.shape == (n, n, n)
    for name in ('delta_ds_1', 'beta_ds_1'):
        assert np.asarray(tiffio.read_tiff(os.path.join('case', 'out', name))).shape == (n, n, n)
    with pytest.raises(ValueError, match=r'\(8, 2, 64, 64\)') as ei:
        reconstruct_fullfield('data.h5', free_prop_cm=list(DIST), output_folder='out3', **kw)
    assert '(n_theta, 3, Y, X)' in str(ei.value)
    with pytest.raises(ValueError, match=r'\(8, 64, 64\)'):
        reconstruct_fullfield('one.h5', free_prop_cm=dist, output_folder='out1', **kw)


def test_three_plane_reconstruction_converges_to_the_phantom():
    """examples/reconstruct_phantom.py's case simulated and reconstructed with three detector planes, held to the bounds
    test_gpu_convergence.py holds the single-distance run to (which measures correlation 0.988, relative L2 error 0.16)."""
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    import reconstruct_phantom as ex
    r = ex.run(128, 60, 100, 2e-8, fp=(5e-4, 1e-3, 2e-3), quiet=True)
    print('full-field convergence with three planes (5e-4, 1e-3, 2e-3) cm (single distance 1e-3: 0.988 / 0.16)', r)
    assert r['delta_corr'] >= 0.95 and r['delta_rel_l2'] <= 0.3, r
    assert 0.5 * r['phantom_peak'] <= r['delta_peak'] <= 1.5 * r['phantom_peak'], r


def test_refusals_on_the_device(engine_mod):
    """What does not carry several detector planes says so instead of running one plane."""
    from beyond_dof_amd import _lib, util
    M = engine_mod.MultisliceEngine
    Y = X = 64
    S, B = 6, 2
    one, zero = np.ones((Y, X)), np.zeros((Y, X))
    o = util.Optics(E, PS, list(DIST), util.PI, Y, X)
    tables = np.ascontiguousarray(np.stack([o.table(d) for d in o.det_planes_nm]))
    dcs = np.ascontiguousarray(np.stack([o.dc(d) for d in o.det_planes_nm]))

    def planes(eng, D=3):
        return eng.lib.bdof_set_detector_planes(eng.h, D, tables.ctypes.data, dcs.ctypes.data)

    def says(eng):
        return b'detector planes' in eng.lib.bdof_last_error(eng.h)

    # ---- Python, before the library is asked
    for kw in (dict(recompute=True), dict(adjoint64=True)):
        with pytest.raises(ValueError, match='detector planes'):
            M(Y, X, S, B, **kw).set_physics(E, PS, list(DIST))
    with pytest.raises(ValueError, match='detector planes'):
        M(Y, X, S, B).set_physics(E, PS, list(DIST), detector_kernel='auto')
    eng = M(Y, X, S, B)
    eng.set_physics(E, PS, list(DIST))
    eng.set_probe(one, zero)
    for call in (lambda: eng.set_conv(E, PS), eng.enable_tf_f64, lambda: eng.set_probe(*orc.gaussian_probe((Y, X), 6., 6., 0.5)),
                 lambda: eng.forward(B, conv=True), lambda: eng.loss_grad(B, np.ones((B, 3, Y, X)), conv=True),
                 lambda: eng.loss_grad(B, np.ones((B, 3, Y, X)), f64=True)):
        with pytest.raises(ValueError, match='detector planes'):
            call()
    with pytest.raises(ValueError, match='detector plane'):
        eng.loss_grad(B, np.ones((B, Y, X)))                       # amplitudes of one plane
    with pytest.raises(ValueError, match='free_prop_cm'):
        eng.set_physics(E, PS, [1e-4] * 9)
    gauss = M(Y, X, S, B)
    gauss.set_physics(E, PS, 1e-4)
    gauss.set_probe(*orc.gaussian_probe((Y, X), 6., 6., 0.5))
    assert gauss.probe_stack
    with pytest.raises(ValueError, match='detector planes'):
        gauss.set_physics(E, PS, list(DIST))
    # ---- the library itself, under the Python checks
    lib, h = eng.lib, eng.h
    assert lib.bdof_loss_grad_tf_f64(h, B, None, None, None, None, 0.0) != 0 and says(eng)
    assert lib.bdof_forward_conv(h, B, None, None, None, None) != 0 and says(eng)
    assert lib.bdof_loss_grad_conv(h, B, None, None, None, None, None) != 0 and says(eng)
    assert lib.bdof_set_conv(h, None, None, 17, 0., 0., 0., 0., 0.) != 0 and says(eng)
    assert lib.bdof_forward_range(h, B, None, None, None, 0, 2, None, None, 1) != 0 and says(eng)
    assert lib.bdof_adjoint_range(h, B, None, None, None, 0, 2, None, None, None, None) != 0 and says(eng)
    assert lib.bdof_set_range_carrier(h, None, 0, 0, 0) != 0 and says(eng)
    stack, det = np.zeros((S, X, Y), dtype=np.complex64), np.zeros((X, Y), dtype=np.complex64)
    assert lib.bdof_set_probe_stack(h, stack.ctypes.data, det.ctypes.data) != 0 and says(eng)
    assert planes(eng, 9) == _lib.load().bdof_set_detector_planes(None, 2, None, None) != 0          # the cap: BDOF_ERR_ARG
    assert planes(eng, 0) != 0
    assert planes(gauss) != 0 and says(gauss)                       # a carrier field is active
    for flag in (_lib.CFG_RECOMPUTE, _lib.CFG_ADJOINT64):
        plain = M(Y, X, S, B)
        plain.ctx.check(plain.lib.bdof_configure(plain.h, Y, X, S, B, _lib.CFG_GRAD | flag))
        plain.set_physics(E, PS, 1e-4)
        assert planes(plain) != 0 and says(plain), flag
    for fp in (None, 'inf'):
        plain = M(Y, X, S, B)
        plain.set_physics(E, PS, fp)
        assert planes(plain) != 0 and says(plain), fp
    plain = M(Y, X, S, B)
    assert planes(plain) != 0                                       # before bdof_set_physics
    # ---- the planes do not survive bdof_set_physics or bdof_configure
    assert lib.bdof_set_range_carrier(h, None, 0, 0, 0) != 0
    eng.set_physics(E, PS, 1e-4)
    assert eng.n_planes == 1 and lib.bdof_set_range_carrier(h, None, 0, 0, 0) == 0
    eng.set_physics(E, PS, list(DIST))
    assert lib.bdof_set_range_carrier(h, None, 0, 0, 0) != 0
    eng.ctx.check(lib.bdof_configure(h, Y, X, S, B, _lib.CFG_GRAD))
    assert lib.bdof_set_range_carrier(h, None, 0, 0, 0) == 0
