"""The Poisson (photon-counting) data term (bdof_set_loss, MultisliceEngine.set_loss, loss_type='poisson') on the device, through
every engine that forms a seed on the transfer-function path, against the float64 reference of tests/reference_model.py under tests/poisson_reference.py's data term.

Bounds: the ones tests/test_gpu_parity.py asserts for the identical least-squares cases — loss relative 1e-5, gradients relative L2
2e-4 — because the Poisson seed is the least-squares seed times mu (a + m) / a, a factor good to 1e-7; the float64 twin at the
bounds of test_float64_transfer_function_path_vs_oracle.  Every test prints what it measured before it asserts."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import bdof_oracle as orc

import poisson_reference as pref
import reference_model as ref_model

MU = 2e6
POISSON = ref_model.data_term(pref.poisson_loss, pref.poisson_seed, MU)


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


def _case(engine_mod, B, Y, X, S, fp, variant, probe, seed=0, **eng_kw):
    """Shapes and measurement construction of test_forward_and_gradient_vs_oracle; m = |ref| |1 + 0.05 N| >= 0."""
    rng = np.random.default_rng(seed)
    delta = rng.uniform(0, 2e-5, size=(B, Y, X, S))
    beta = 0.1 * delta
    pr, pi = _probe(probe, Y, X, rng)
    residual_split = eng_kw.pop('residual_split', True)
    eng = engine_mod.MultisliceEngine(Y, X, S, B, with_grad=True, **eng_kw)
    eng.residual_split = residual_split
    eng.set_physics(5000., 1e-7, fp, variant=variant)
    eng.set_probe(pr, pi)
    eng.set_object_batch(delta, beta)
    ref, _ = ref_model.forward(delta, beta, pr, pi, 5000., 1e-7, fp, variant)
    meas = np.abs(ref) * np.abs(1 + 0.05 * rng.normal(size=ref.shape))
    return eng, delta, beta, pr, pi, meas


ENGINE_SHAPES = [('streaming', 128, 128), ('streaming', 64, 256), ('resident', 72, 72), ('resident', 128, 128),
                 ('generic', 64, 64), ('generic', 96, 80)]


@pytest.mark.parametrize('engine,Y,X', ENGINE_SHAPES)
@pytest.mark.parametrize('fp', [None, 1e-4, 'inf'])
@pytest.mark.parametrize('probe', ['plane', 'random', 'gaussian'])
@pytest.mark.parametrize('variant', ['numpy_skip_last', 'tf_all'])
def test_poisson_loss_and_gradient_vs_reference(engine_mod, engine, Y, X, fp, probe, variant):
    """'plane': residual splitting (with 'inf' the float64 DC bin and the adjoint carrier); 'random': a scalar carrier under a
    structured probe; 'gaussian': the float64 carrier field."""
    B, S = 2, 5
    eng, delta, beta, pr, pi, meas = _case(engine_mod, B, Y, X, S, fp, variant, probe, engine=engine)
    eng.set_loss('poisson', MU)
    loss = eng.loss_grad(B, meas)
    gd, gb = eng.grad_batch_to_host(B)
    rl, rgd, rgb, _, _ = ref_model.loss_and_grad(delta, beta, pr, pi, 5000., 1e-7, meas, fp, variant, term=POISSON)
    e = (abs(loss - rl) / abs(rl), rel(gd, rgd), rel(gb, rgb))
    print('poisson parity', engine, (Y, X), fp, probe, variant, 'loss / g_delta / g_beta rel err', e)
    assert e[0] <= 1e-5, e
    assert e[1] <= 2e-4 and e[2] <= 2e-4, e


@pytest.mark.parametrize('fp,variant', [(None, 'numpy_skip_last'), (1e-4, 'tf_all')])
def test_poisson_plain_residual_form_on_the_resident_engine(engine_mod, fp, variant):
    """Scalar carrier with residual splitting off: the resident engine's float32 |d| - m (seed_plain) under the Poisson kind, which
    the cases above do not reach (their real-space detectors split, their far-field ones carry a float64 field).  The engine's
    smallest shape; bounds of test_poisson_loss_and_gradient_vs_reference."""
    B, S, n = 2, 2, 32
    eng, delta, beta, pr, pi, meas = _case(engine_mod, B, n, n, S, fp, variant, 'plane', seed=5, engine='resident', residual_split=False)
    assert eng.meas_ref == 0.0 and not eng.probe_stack
    eng.set_loss('poisson', MU)
    loss = eng.loss_grad(B, meas)
    gd, gb = eng.grad_batch_to_host(B)
    rl, rgd, rgb, _, _ = ref_model.loss_and_grad(delta, beta, pr, pi, 5000., 1e-7, meas, fp, variant, term=POISSON)
    e = (abs(loss - rl) / abs(rl), rel(gd, rgd), rel(gb, rgb))
    print('poisson resident plain form', fp, variant, 'loss / g_delta / g_beta rel err', e)
    assert e[0] <= 1e-5, e
    assert e[1] <= 2e-4 and e[2] <= 2e-4, e


@pytest.mark.parametrize('Y,X', [(64, 64), (72, 72), (64, 256)])
@pytest.mark.parametrize('fp', [None, 1e-4, 'inf'])
@pytest.mark.parametrize('variant', ['numpy_skip_last', 'tf_all'])
def test_poisson_float64_twin_vs_reference(engine_mod, Y, X, fp, variant):
    """bdof_loss_grad_tf_f64 under the Poisson kind: cases, rounding of the inputs and bounds of
    test_float64_transfer_function_path_vs_oracle (loss 1e-8; gradient rows are stored as float32: 2e-7)."""
    B, S = 2, 6
    rng = np.random.default_rng(0)
    delta = rng.uniform(0, 2e-5, size=(B, Y, X, S)).astype(np.float32).astype(np.float64)
    beta = (0.1 * delta).astype(np.float32).astype(np.float64)
    pr, pi = _probe('gaussian' if fp == 'inf' else 'random', Y, X, rng)
    p64 = (np.asarray(pr) + 1j * np.asarray(pi)).astype(np.complex64)
    pr64, pi64 = p64.real.astype(np.float64), p64.imag.astype(np.float64)
    eng = engine_mod.MultisliceEngine(Y, X, S, B, with_grad=True)
    eng.set_physics(5000., 1e-7, fp, variant=variant)
    eng.set_probe(pr, pi)
    eng.set_object_batch(delta, beta)
    ref, _ = ref_model.forward(delta, beta, pr64, pi64, 5000., 1e-7, fp, variant)
    meas = (np.abs(ref) * np.abs(1 + 0.05 * rng.normal(size=ref.shape))).astype(np.float32).astype(np.float64)
    rl, rgd, rgb, _, _ = ref_model.loss_and_grad(delta, beta, pr64, pi64, 5000., 1e-7, meas, fp, variant, term=POISSON)
    eng.set_loss('poisson', MU)
    eng.enable_tf_f64()
    loss = eng.loss_grad(B, meas, f64=True)
    gd, gb = eng.grad_batch_to_host(B)
    e = (abs(loss - rl) / abs(rl), rel(gd, rgd), rel(gb, rgb))
    print('poisson float64 twin', (Y, X), fp, variant, e)
    assert e[0] <= 1e-8 and e[1] <= 2e-7 and e[2] <= 2e-7, e


@pytest.mark.parametrize('setting', ['recompute', 'adjoint64', 'probe_grad'])
def test_poisson_seed_only_settings(engine_mod, setting):
    """Settings that only move the seed on: the tape-free adjoint, the float64 adjoint sweep (generic engine), the probe gradient."""
    B, S, fp = 2, 5, 1e-4
    kw = {'recompute': dict(recompute=True), 'adjoint64': dict(engine='generic', adjoint64=True), 'probe_grad': {}}[setting]
    eng, delta, beta, pr, pi, meas = _case(engine_mod, B, 64, 64, S, fp, 'numpy_skip_last', 'random', seed=4, **kw)
    eng.set_loss('poisson', MU)
    if setting == 'probe_grad':
        eng.enable_probe_grad(True)
    loss = eng.loss_grad(B, meas)
    gd, gb = eng.grad_batch_to_host(B)
    rl, rgd, rgb, g0, _ = ref_model.loss_and_grad(delta, beta, pr, pi, 5000., 1e-7, meas, fp, term=POISSON)
    e = [abs(loss - rl) / abs(rl), rel(gd, rgd), rel(gb, rgb)]
    if setting == 'probe_grad':
        e.append(rel(eng.probe_grad(), g0.sum(axis=0)))
    print('poisson', setting, 'loss / g_delta / g_beta (/ g_probe) rel err', e)
    assert e[0] <= 1e-5, e
    assert max(e[1:]) <= 2e-4, e


def test_poisson_solver_parity_64_cubed(engine_mod):
    """FullfieldSolver(loss_type='poisson') at 64^3, two angles: rotation -> reference module -> rotation adjoint."""
    from beyond_dof_amd.solver import FullfieldSolver
    n, n_theta, fp = 64, 4, 1e-4
    rng = np.random.default_rng(6)
    od = rng.uniform(0, 2e-5, size=(n, n, n))
    ob = 0.1 * od
    coords = orc.rotation_lookup([n, n, n], n_theta)
    one, zero = np.ones((n, n)), np.zeros((n, n))
    idx = [1, 3]
    rot = np.stack([orc.apply_rotation(np.stack([od, ob], axis=3), coords[j]) for j in idx])
    ref, _ = ref_model.forward(rot[..., 0], rot[..., 1], one, zero, 5000., 1e-7, fp)
    meas = np.ones((n_theta, n, n))
    meas[idx] = np.abs(ref) * np.abs(1 + 0.05 * rng.normal(size=ref.shape))
    s = FullfieldSolver(n, n, n, n_theta, 2, 5000., 1e-7, free_prop_cm=fp, coord_ls=coords, loss_type='poisson', poisson_multiplier=MU)
    s.set_measurements(meas)
    s.set_volume(od, ob)
    loss = s.loss_and_grad(idx)
    gd, gb = s.gradient_to_host()
    rl, rgd, rgb, _, _ = ref_model.loss_and_grad(rot[..., 0], rot[..., 1], one, zero, 5000., 1e-7, meas[idx], fp, term=POISSON)
    wd = sum(orc.apply_rotation_adjoint(rgd[k], coords[j]) for k, j in enumerate(idx))
    wb = sum(orc.apply_rotation_adjoint(rgb[k], coords[j]) for k, j in enumerate(idx))
    e = (abs(loss - rl) / abs(rl), rel(gd, wd), rel(gb, wb))
    print('poisson solver parity 64^3', e)
    assert e[0] <= 1e-5 and e[1] <= 2e-4 and e[2] <= 2e-4, e


@pytest.mark.parametrize('engine,Y,X,fp,probe', [('streaming', 128, 128, 1e-4, 'plane'), ('streaming', 128, 128, 'inf', 'plane'),
                                                 ('resident', 72, 72, 'inf', 'gaussian'), ('generic', 96, 80, None, 'random')])
def test_least_squares_is_untouched_by_a_poisson_visit(engine_mod, engine, Y, X, fp, probe):
    """set_loss('lsq') after set_loss('poisson'): loss and gradient bit-identical to an engine that never called it."""
    B, S = 2, 5
    out = []
    for visit in (False, True):
        eng, delta, beta, pr, pi, meas = _case(engine_mod, B, Y, X, S, fp, 'numpy_skip_last', probe, engine=engine)
        if visit:
            eng.set_loss('poisson', MU)
            lp = eng.loss_grad(B, meas)
            eng.set_loss('lsq')
        loss = eng.loss_grad(B, meas)
        out.append((loss,) + tuple(eng.grad_batch_to_host(B)))
    assert lp != out[0][0]
    assert out[0][0] == out[1][0]
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])


def test_paths_without_a_poisson_term_raise(engine_mod):
    """The real-space propagator (float32 and float64) and the tiled propagator's field loss compute least squares only: under
    the Poisson kind they fail through bdof_last_error; a wrong kind or multiplier is refused; least squares runs them again."""
    from beyond_dof_amd import _lib
    B, Y, X, S = 2, 64, 64, 4
    eng, delta, beta, pr, pi, meas = _case(engine_mod, B, Y, X, S, None, 'numpy_skip_last', 'plane')
    eng.set_conv(5000., 1e-7, 5)
    eng.set_object_batch(delta, beta)
    l_conv = eng.loss_grad(B, meas, conv=True)
    field = _lib.DeviceBuffer.from_host(eng.ctx, np.ones((X, Y), dtype=np.complex64))
    m1 = _lib.DeviceBuffer.from_host(eng.ctx, np.full((X, Y), 0.9, dtype=np.float32))
    eng.ctx.check(eng.lib.bdof_field_loss_seed(eng.h, field.ptr, m1.ptr, X, Y))
    eng.set_loss('poisson', MU)
    with pytest.raises(_lib.BdofError, match='least-squares'):
        eng.loss_grad(B, meas, conv=True)
    with pytest.raises(_lib.BdofError, match='least-squares'):
        eng.ctx.check(eng.lib.bdof_field_loss_seed(eng.h, field.ptr, m1.ptr, X, Y))
    eng.enable_conv_f64()
    with pytest.raises(_lib.BdofError, match='least-squares'):
        eng.loss_grad(B, meas, conv=True, f64=True)
    assert eng.lib.bdof_set_loss(eng.h, 2, 1.0) != 0 and eng.lib.bdof_set_loss(eng.h, 1, 0.0) != 0 and eng.lib.bdof_set_loss(eng.h, 1, -3.0) != 0
    with pytest.raises(ValueError, match='loss_type'):
        eng.set_loss('bogus')
    with pytest.raises(ValueError, match='poisson_multiplier'):
        eng.set_loss('poisson', 0)
    assert eng.loss_type == 'poisson' and eng.poisson_multiplier == MU          # the refused calls left the setting whole
    eng.set_loss('lsq')
    assert eng.loss_grad(B, meas, conv=True) == l_conv
    from beyond_dof_amd.solver import FullfieldSolver
    with pytest.raises(ValueError, match='poisson'):
        FullfieldSolver(64, 64, 64, 2, 1, 5000., 1e-7, propagator='conv', loss_type='poisson')


# ---- end to end -------------------------------------------------------------------------------------------------------------
E2E_MU = 2e4            # photons per unit intensity of the simulated data = poisson_multiplier: 0.7 % noise on a unit amplitude
# Margin on the correlation with the phantom: twice the spread (max - min) of the least-squares runs over the noise seeds 0, 1, 2,
# measured once on an MI355X (MEASUREMENTS.md, "the Poisson data term", beside this test's name):
#   least squares 0.017966, 0.014733, 0.012524   Poisson 0.017939, 0.014682, 0.012496   ->   2 * (0.017966 - 0.012524) = 0.010885
E2E_MARGIN = 0.01088


def _e2e_phantom(n):
    rng = np.random.default_rng(11)
    z, y, x = np.mgrid[:n, :n, :n]
    d = np.zeros((n, n, n))
    for _ in range(6):
        c = rng.uniform(n * 0.3, n * 0.7, size=3)
        r = rng.uniform(n * 0.08, n * 0.2)
        d += 1e-6 * np.exp(-((z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2) / (2 * r ** 2))
    return d, 0.1 * d


def _e2e_run(noise_seed, loss_type, tmp):
    """One small full-field reconstruction at 64^3, near-field detector, from data with Poisson noise of simulation.py at
    mu = E2E_MU: (loss of the run's own kind at the start, at the end, correlation of delta with the phantom)."""
    from beyond_dof_amd import h5io, simulation
    from beyond_dof_amd.fullfield import reconstruct_fullfield
    from beyond_dof_amd.solver import FullfieldSolver
    n, n_theta, mb, fp = 64, 8, 4, 1e-4
    true_d, true_b = _e2e_phantom(n)
    coords = orc.rotation_lookup([n, n, n], n_theta)
    one, zero = np.ones((n, n)), np.zeros((n, n))
    case = os.path.join(tmp, 'case{}'.format(noise_seed))
    if not os.path.exists(os.path.join(case, 'noisy.h5')):
        os.makedirs(case)
        rot = np.stack([orc.apply_rotation(np.stack([true_d, true_b], axis=3), c) for c in coords])
        prj, _ = ref_model.forward(rot[..., 0], rot[..., 1], one, zero, 5000., 1e-7, fp)
        h5io.write_dataset(os.path.join(case, 'clean.h5'), 'exchange/data', prj.astype(np.complex64))
        # n_ph_tx / n_sample_pixel photons per unit intensity (simulation.create_noisy_data): E2E_MU of them
        simulation.create_noisy_data(os.path.join(case, 'clean.h5'), os.path.join(case, 'noisy.h5'), E2E_MU, n_sample_pixel=1,
                                     is_ptycho=False, rng=np.random.RandomState(noise_seed))
    init_d, init_b = np.full((n, n, n), 8.7e-7), np.full((n, n, n), 5.1e-8)
    d, b = reconstruct_fullfield('noisy.h5', theta_st=0, theta_end=2 * np.pi, n_epochs=5, learning_rate=1e-7, minibatch_size=mb,
                                 energy_ev=5000, psize_cm=1e-7, free_prop_cm=fp, save_path=case, output_folder='out_' + loss_type,
                                 initial_guess=[init_d, init_b], shrink_cycle=None, seed=7, alpha_d=0., alpha_b=0., gamma=0.,
                                 loss_type=loss_type, poisson_multiplier=E2E_MU)
    meas = np.abs(np.asarray(h5io.read_dataset(os.path.join(case, 'noisy.h5'))))
    s = FullfieldSolver(n, n, n, n_theta, n_theta, 5000., 1e-7, free_prop_cm=fp, coord_ls=coords, loss_type=loss_type, poisson_multiplier=E2E_MU)
    s.set_measurements(meas)
    s.set_volume(init_d, init_b)
    l0 = s.loss_and_grad(np.arange(n_theta))
    s.set_volume(d, b)
    l1 = s.loss_and_grad(np.arange(n_theta))
    return l0, l1, float(np.corrcoef(d.ravel(), true_d.ravel())[0, 1])


def test_poisson_reconstruction_end_to_end(engine_mod, tmp_path, monkeypatch):
    """loss_type='poisson' and 'lsq' on the same noisy file, three noise seeds: the Poisson run lowers its loss and correlates with
    the phantom no worse than the least-squares run minus E2E_MARGIN (twice the measured spread of the least-squares runs; the
    six correlations are in MEASUREMENTS.md, "the Poisson data term").  Five epochs from a flat start recover little at this
    noise level — all six correlations are below 0.02 — so this test says that the two data terms move the volume alike, not
    that either reconstructs well."""
    monkeypatch.chdir(tmp_path)
    runs = {(seed, kind): _e2e_run(seed, kind, str(tmp_path)) for seed in (0, 1, 2) for kind in ('lsq', 'poisson')}
    for key in sorted(runs):
        print('poisson e2e', key, 'loss start / end / correlation with the phantom', runs[key])
    for seed in (0, 1, 2):
        l0, l1, corr = runs[(seed, 'poisson')]
        assert l1 < l0, (seed, l0, l1)
        assert corr >= runs[(seed, 'lsq')][2] - E2E_MARGIN, (seed, corr, runs[(seed, 'lsq')][2], E2E_MARGIN)


def test_poisson_ptychography_lowers_its_loss(engine_mod, tmp_path, monkeypatch):
    """reconstruct_ptychography(loss_type='poisson') on NOISE-FREE data: the loss over the data set goes down.  The run IS far
    field — PtychoSolver fixes free_prop_cm='inf' as the reference's ptychography does, there is no other detector to choose — so
    what this covers is far-field ptychography without noise, and nothing else.  Noisy far-field data has bins with a measured
    count over a model intensity near zero, where the bare likelihood is unbounded: that case is not covered."""
    from beyond_dof_amd import h5io
    from beyond_dof_amd.ptychography import reconstruct_ptychography
    from beyond_dof_amd.solver import PtychoSolver
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(0)
    n, n_theta, psz = 64, 2, (64, 64)
    pos = np.array([(y, x) for y in (16, 48) for x in (16, 32, 48)])
    od = rng.uniform(0, 2e-5, size=(n, n, n))
    ob = 0.1 * od
    coords = orc.rotation_lookup([n, n, n], n_theta)
    prr, pii = orc.gaussian_probe(psz, 6., 6., 0.5)
    pad, half = orc.ptycho_pad_amounts(pos, psz, (n, n, n))
    data = np.zeros((n_theta, len(pos)) + psz, dtype=np.complex64)
    for t in range(n_theta):
        rot = orc.apply_rotation(np.stack([od, ob], axis=3), coords[t])
        obj_pad = np.pad(rot, ((pad[0, 0], pad[0, 1]), (pad[1, 0], pad[1, 1]), (0, 0), (0, 0)), mode='constant')
        subs = np.stack([obj_pad[p[0] + pad[0, 0] - half[0]:p[0] + pad[0, 0] - half[0] + psz[0],
                                 p[1] + pad[1, 0] - half[1]:p[1] + pad[1, 0] - half[1] + psz[1]] for p in pos])
        data[t], _ = ref_model.forward(subs[..., 0], subs[..., 1], prr, pii, 5000., 1e-7, 'inf')
    os.makedirs('case')
    h5io.write_dataset('case/data.h5', 'exchange/data', data)
    init_d, init_b = np.full((n, n, n), 8e-6), np.full((n, n, n), 8e-7)
    d, b = reconstruct_ptychography('data.h5', [tuple(p) for p in pos], psz, (n, n, n), theta_st=0, theta_end=2 * np.pi, n_epochs=2,
                                    learning_rate=2e-7, minibatch_size=3, energy_ev=5000, psize_cm=1e-7, save_path='case',
                                    output_folder='out', initial_guess=[init_d, init_b], probe_type='gaussian', seed=3,
                                    probe_mag_sigma=6., probe_phase_sigma=6., probe_phase_max=0.5, loss_type='poisson', poisson_multiplier=MU)
    s = PtychoSolver((n, n, n), psz, pos, n_theta, len(pos), 5000., 1e-7, prr, pii, coord_ls=coords, loss_type='poisson', poisson_multiplier=MU)

    def total(dd, bb):
        s.set_volume(dd, bb)
        return sum(s.loss_and_grad(t, np.arange(len(pos)), np.abs(data[t])) for t in range(n_theta))
    l0, l1 = total(init_d, init_b), total(d, b)
    print('poisson ptychography loss start / end', l0, l1)
    assert np.isfinite(l1) and l1 < l0
