"""Probe modes through PtychoSolver, reconstruct_ptychography and the simulator.

Volume 32 x 32 x 16, 9 positions, 2 angles, M = 2 modes of a 36^2 probe (the resident engine) and of a 20^2 probe (the generic
engine).  The float64 reference is tests/modes_reference.py between the window arithmetic of tests/positions_reference.py (at zero
offsets the integer cut, value for value) and a rotation: the lookup tables, or tests/rigid_reference.py's rigid map.  Bounds as in
tests/test_gpu_modes.py: loss 2e-5, volume gradient 2e-4; position_gradient() and geometry_gradient() within 2e-4 of the float64
restatement fed the same mode-summed window gradient, relative to the sum of the absolute values of an entry's terms (as
tests/test_gpu_positions.py and tests/test_gpu_geometry.py measure them)."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import geometry_reference as gr
import modes_reference as mref
import positions_reference as pr
import rigid_reference as rr
from reference_model import rel

E, PS = 5000., 1e-7
SHAPE, N_THETA, I_THETA = (32, 32, 16), 2, 1
POS = np.array([(y, x) for y in (8, 16, 24) for x in (8, 16, 24)])
IDX = np.arange(len(POS))
LOSS_BOUND, GRAD_BOUND = 2e-5, 2e-4
THETA, TILT = np.array([-0.25, -1.125]), 0.125               # rotation='trilinear': two angles under a small tilt (float32 numbers)
PROBES = [(36, 'resident'), (20, 'generic')]
FLOAT32_NOISE = 1e-6        # 6e-8 sqrt(320): test_mode_optimization_steps_follow_the_float64_loop


@pytest.fixture(scope='module')
def built():
    import __graft_entry__ as entry
    entry.build()


def _volume():
    rng = np.random.default_rng(23)
    od = np.zeros(SHAPE)
    od[3:-3, 3:-3, 2:-2] = rng.uniform(0, 2e-5, size=(26, 26, 12))
    od = od.astype(np.float32).astype(np.float64)
    return od, (np.float32(0.1) * od.astype(np.float32)).astype(np.float64)


def _modes(psz, power=0.3):
    from beyond_dof_amd import modes, util
    p = util.gaussian_probe((psz, psz), psz / 6., psz / 6., 0.5)
    return modes.initial_modes(p[0] + 1j * p[1], 2, power).astype(np.complex64)


def _rotation(kind):
    from beyond_dof_amd import util
    if kind == 'nearest':
        return pr.nearest(util.rotation_lookup(SHAPE, N_THETA)[I_THETA]), None
    prm = util.rigid_geometry(THETA, SHAPE, TILT)[I_THETA]
    return ((lambda obj: rr.rotate_volume(obj, prm)), (lambda g: rr.rotate_volume_adjoint(g, prm))), prm


def _offsets():
    return np.random.default_rng(41).uniform(-0.9, 0.9, size=(len(POS), 2))


@functools.lru_cache(maxsize=None)
def _problem(psz, kind='nearest', fractional=False):
    """float64: amplitudes, loss, volume gradient, mode gradients and — from the mode-summed window gradient — the position and the
    geometry derivatives with their term sums; computed once, read only"""
    od, ob = _volume()
    modes = _modes(psz)
    (rotate, rotate_adjoint), prm = _rotation(kind)
    off = _offsets() if fractional else np.zeros((len(POS), 2))
    R = pr.to_frame(rotate(np.stack([od, ob], axis=3)))
    org = pr.origins(POS, off, (psz, psz))
    subs = pr.window_cut(R, org, psz, psz).transpose(0, 3, 2, 1, 4)                  # (B, py, px, Z, C)
    rng = np.random.default_rng([psz, 7])
    a = mref.amplitude(mref.forward(subs[..., 0], subs[..., 1], modes, E, PS, 'inf'))
    meas = (a * np.abs(1 + 0.05 * rng.normal(size=a.shape))).astype(np.float32)
    loss, gd, gb, gm, d = mref.loss_and_grad(subs[..., 0], subs[..., 1], modes, E, PS, meas.astype(np.float64), 'inf')
    g = np.stack([gd, gb], axis=-1).transpose(0, 3, 2, 1, 4)                         # [B][S][NX][NY][C], the modes summed
    g_rot = pr.window_cut_adjoint(g, org, R.shape[1], R.shape[2])                    # [S][X][Y][C]
    g_vol = rotate_adjoint(pr.from_frame(g_rot))
    out = dict(od=od, ob=ob, modes=modes, off=off, meas=meas, loss=float(loss), gd=g_vol[..., 0], gb=g_vol[..., 1], gm=gm, amp=a)
    if fractional:
        dpos, _, _, T = pr.position_terms(R, g, org)
        out.update(dpos=dpos[:, ::-1], T=T[:, ::-1])
    if prm is not None:
        t = gr.param_terms(gr.to_rows([od, ob]), g_rot, prm)
        out.update(geometry=gr.chain([t], np.array([I_THETA]), THETA, SHAPE, TILT, 0., None),
                   sums=gr.geometry_term_sums(t[3][None], np.array([I_THETA]), THETA, SHAPE, TILT, 0., None))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _solver(psz, p, modes=None, **kw):
    from beyond_dof_amd.solver import PtychoSolver
    modes = p['modes'] if modes is None else modes
    s = PtychoSolver(SHAPE, (psz, psz), POS, N_THETA, len(POS), E, PS, modes.real, modes.imag, **kw)
    s.set_volume(p['od'], p['ob'])
    return s


@pytest.mark.parametrize('psz,engine', PROBES)
def test_loss_and_gradient_against_the_reference(built, psz, engine):
    p = _problem(psz)
    s = _solver(psz, p)
    assert s.n_modes == 2 and s.eng.batch_max == 2 * len(POS)
    loss = s.loss_and_grad(I_THETA, IDX, p['meas'])
    gd, gb = s.gradient_to_host()
    errs = (abs(loss - p['loss']) / p['loss'], rel(gd, p['gd']), rel(gb, p['gb']))
    print('PtychoSolver, 2 modes', psz, engine, '(loss, g_delta, g_beta)', errs)
    assert errs[0] <= LOSS_BOUND and max(errs[1:]) <= GRAD_BOUND, errs
    wave = s.forward(I_THETA, IDX)
    assert wave.shape == (2, len(POS), psz, psz)
    assert rel(np.sqrt(np.sum(np.abs(wave) ** 2, axis=0)), p['amp']) <= 1e-5


@pytest.mark.parametrize('psz,engine', PROBES)
def test_fractional_positions(built, psz, engine):
    p = _problem(psz, fractional=True)
    s = _solver(psz, p, position_offsets=p['off'])
    loss = s.loss_and_grad(I_THETA, IDX, p['meas'])
    gd, gb = s.gradient_to_host()
    dpos = s.position_gradient()
    ratio = float(np.max(np.abs(dpos - p['dpos']) / p['T']))
    errs = (abs(loss - p['loss']) / p['loss'], rel(gd, p['gd']), rel(gb, p['gb']))
    print('position_offsets, 2 modes', psz, engine, '(loss, g_delta, g_beta)', errs, 'position gradient: largest |device - reference| / sum |terms|', ratio)
    assert errs[0] <= LOSS_BOUND and max(errs[1:]) <= GRAD_BOUND, errs
    assert np.all(np.isfinite(dpos)) and ratio <= GRAD_BOUND


@pytest.mark.parametrize('psz,engine', PROBES)
def test_trilinear_rotation_and_geometry_gradient(built, psz, engine):
    p = _problem(psz, kind='trilinear')
    s = _solver(psz, p, rotation='trilinear', theta=THETA, axis_tilt=TILT)
    loss = s.loss_and_grad(I_THETA, IDX, p['meas'])
    gd, gb = s.gradient_to_host()
    got = s.geometry_gradient()
    errs = (abs(loss - p['loss']) / p['loss'], rel(gd, p['gd']), rel(gb, p['gb']))
    worst = 0.0
    for name in ('center', 'axis_tilt', 'axis_roll', 'theta', 'shifts'):
        ratio = np.abs(np.asarray(got[name]) - np.asarray(p['geometry'][name])) / np.asarray(p['sums'][name])
        assert np.all(np.isfinite(np.asarray(got[name])))
        worst = max(worst, float(np.max(ratio)))
    print("rotation='trilinear', 2 modes", psz, engine, '(loss, g_delta, g_beta)', errs, 'geometry gradient: largest |device - reference| / sum |terms|', worst)
    assert errs[0] <= LOSS_BOUND and max(errs[1:]) <= GRAD_BOUND, errs
    assert worst <= GRAD_BOUND


def _ref_step(od, ob, modes, meas, i_theta, psz):
    """loss, volume gradient (2, Y, X, Z) and mode gradients of one minibatch (all positions of one angle) in float64"""
    from beyond_dof_amd import util
    rotate, rotate_adjoint = pr.nearest(util.rotation_lookup(SHAPE, N_THETA)[i_theta])
    R = pr.to_frame(rotate(np.stack([od, ob], axis=3)))
    org = pr.origins(POS, np.zeros((len(POS), 2)), (psz, psz))
    subs = pr.window_cut(R, org, psz, psz).transpose(0, 3, 2, 1, 4)
    loss, gd, gb, gm, _ = mref.loss_and_grad(subs[..., 0], subs[..., 1], modes, E, PS, meas, 'inf')
    g = np.stack([gd, gb], axis=-1).transpose(0, 3, 2, 1, 4)
    g_vol = rotate_adjoint(pr.from_frame(pr.window_cut_adjoint(g, org, R.shape[1], R.shape[2])))
    return loss, np.array([g_vol[..., 0], g_vol[..., 1]]), gm


@pytest.mark.parametrize('psz,engine', PROBES)
def test_mode_optimization_steps_follow_the_float64_loop(built, psz, engine):
    """Three steps of PtychoSolver.step with two optimisable modes (object AND modes updated) against the same loop in float64:
    the object by cnn_propagator/util.py:280-291 and the clip, the modes by a standard Adam on their real and imaginary parts,
    as tests/test_gpu_probe.py::test_probe_optimization_steps_follow_the_oracle does for one probe, with its caps.  Before the
    device is asked, the reference loop is run a second time from mode gradients perturbed by FLOAT32_NOISE of their norm — what
    float32 arithmetic alone does to them: its unit round-off 6e-8 times the square root of the ~320 rounded operations a pixel
    passes through (16 slices, two 2-D transforms each, ~5 radix passes per dimension).  For the seed used here the two float64
    loops must agree on all but a quarter of the cap's share of pixels: the steps are sign-stable, and the cap measures the
    device.  (Perturbed by the whole 2e-4 the gradients are allowed, 2 % to 7 % of the pixels in the modes' tails step
    differently: Adam's first steps are sign-like, and the cap is only meaningful for an engine near float32's own accuracy.)"""
    from oracle import bdof_oracle as orc
    p = _problem(psz)
    plr, lr = 1e-3, 1e-7
    start = (0.9 * p['modes']).astype(np.complex128)
    meas = p['meas'].astype(np.float64)

    def loop(noise):
        rng = np.random.default_rng(3)
        x, m, v = np.array([p['od'], p['ob']]), None, None
        q = start.copy()
        pm, pv = np.zeros_like(q), np.zeros_like(q)
        losses = []
        for it in range(3):
            q32 = q.astype(np.complex64)
            loss, g, gq = _ref_step(x[0], x[1], q32, meas, it % N_THETA, psz)
            if noise:
                gq = gq + noise * np.linalg.norm(gq) / np.sqrt(gq.size) * (rng.normal(size=gq.shape) + 1j * rng.normal(size=gq.shape))
            losses.append(loss)
            x, m, v = orc.apply_gradient_adam(x, g, it, m, v, step_size=lr)
            x = np.clip(x, 0, None)
            t = it + 1
            pm = 0.9 * pm + 0.1 * gq
            pv = 0.999 * pv + 0.001 * (gq.real ** 2 + 1j * gq.imag ** 2)
            mh, vh = pm / (1 - 0.9 ** t), pv / (1 - 0.999 ** t)
            q = q - plr * (mh.real / (np.sqrt(vh.real) + 1e-8) + 1j * mh.imag / (np.sqrt(vh.imag) + 1e-8))
        return losses, q

    ref_losses, ref_q = loop(0.0)
    _, noisy_q = loop(FLOAT32_NOISE)
    stable = float(np.mean(np.abs(noisy_q - ref_q) > 0.05 * plr))
    print('reference loop against itself under gradients perturbed by', FLOAT32_NOISE, ': share of mode pixels that step differently', stable)
    assert stable < 5e-3 / 4
    s = _solver(psz, p, modes=start)
    s.enable_probe_optimization(start.real, start.imag, plr)
    s.reset_moments()
    losses = [s.step(it, it % N_THETA, IDX, p['meas'], lr, want_loss=True) for it in range(3)]
    got = s.get_probe()
    got = got[0] + 1j * got[1]
    assert got.shape == (2, psz, psz)
    share = float(np.mean(np.abs(got - ref_q) > 0.05 * plr))
    print('mode optimisation', psz, engine, 'losses', losses, 'reference', ref_losses, 'share of mode pixels off by more than 0.05 lr', share)
    for a, b in zip(losses, ref_losses):
        assert abs(a - b) <= 1e-4 * abs(b)
    assert np.abs(got - start).max() > 0.5 * plr
    assert share < 5e-3


# ---- recovery: nobody had run this before; the constants below are the one measurement there is (MEASUREMENTS.md, "Probe modes") -----
R_PSZ, R_STEPS, R_PLR = 36, 300, 3e-3
# Measured once on an MI355X (one run, one seed): after 300 steps (150 epochs) at probe learning rate 3e-3 the relative powers went
# from 0.980 / 0.020 to 0.738 / 0.262 — an error of 0.038 against 0.7 / 0.3 —, the loss per epoch fell in every one of the 149 epoch
# to epoch comparisons (5.11 -> 7.8e-3), and the single-mode fit ended at 0.482, 62 times the two-mode fit's loss.
POWER_ERROR_BOUND = 0.076       # twice the measured error of the relative powers
LOSS_RATIO_BOUND = 10.0         # the single-mode fit's final loss over the two-mode fit's: the issue's ten (measured: 62)


def _strong_volume():
    """Ten gaussian blobs with a phase of order one radian through the depth.  The weak object of the parity tests (8e-3 rad)
    leaves every window's pattern at sum_m |F P_m|^2: only the Fourier-space diagonal of the modes' density matrix is measured, one
    mode fits such data as well as two, and nothing pins the powers.  Structure that the probe is scanned over does."""
    rng = np.random.default_rng(12)
    y, x, z = np.meshgrid(np.arange(32), np.arange(32), np.arange(16), indexing='ij')
    od = np.zeros(SHAPE)
    for _ in range(10):
        cy, cx, cz = rng.uniform(5, 27), rng.uniform(5, 27), rng.uniform(3, 13)
        w, a = rng.uniform(1.5, 3.0), rng.uniform(2e-3, 8e-3)
        od += a * np.exp(-((y - cy) ** 2 + (x - cx) ** 2 + (z - cz) ** 2) / (2 * w ** 2))
    od[od < 1e-5] = 0.
    od = od.astype(np.float32).astype(np.float64)
    return od, (np.float32(0.1) * od.astype(np.float32)).astype(np.float64)


def test_mode_optimization_recovers_the_second_mode(built):
    """The volume held at the truth (learning rate 0), data simulated with two modes of relative power 0.7 / 0.3, the fit started
    from mode 0 exact and mode 1 at 0.02 of mode 0's power: the loss falls from epoch to epoch (an epoch: both angles), and after
    orthogonalize_probe_modes the relative powers approach 0.7 / 0.3.  A single-mode fit of the same data under the same budget
    ends at a loss many times the two-mode fit's."""
    from beyond_dof_amd import modes, util
    from beyond_dof_amd.solver import PtychoSolver
    od, ob = _strong_volume()
    g = util.gaussian_probe((R_PSZ, R_PSZ), R_PSZ / 6., R_PSZ / 6., 0.5)
    truth = modes.initial_modes(g[0] + 1j * g[1], 2, 3. / 7.)
    assert np.abs(modes.relative_power(truth) - (0.7, 0.3)).max() < 1e-12
    sim = PtychoSolver(SHAPE, (R_PSZ, R_PSZ), POS, N_THETA, len(POS), E, PS, truth.real, truth.imag)
    sim.set_volume(od, ob)
    data = np.stack([np.sqrt(np.sum(np.abs(sim.forward(t, IDX)) ** 2, axis=0)) for t in range(N_THETA)])
    del sim

    def fit(start):
        s = PtychoSolver(SHAPE, (R_PSZ, R_PSZ), POS, N_THETA, len(POS), E, PS, start.real, start.imag)
        s.set_volume(od, ob)
        s.set_measurements(data)
        s.enable_probe_optimization(start.real, start.imag, R_PLR)
        s.reset_moments()
        losses = [s.step(i, i % N_THETA, IDX, None, 0.0, want_loss=True) for i in range(R_STEPS)]
        d, b = s.get_volume()
        assert np.array_equal(d, od.astype(np.float32)) and np.array_equal(b, ob.astype(np.float32))       # the volume stood still
        return s, np.array(losses).reshape(-1, N_THETA).mean(axis=1)

    start = np.array([truth[0], truth[1] * np.sqrt(0.02 * modes.mode_power(truth)[0] / modes.mode_power(truth)[1])])
    s2, epochs2 = fit(start)
    powers = s2.orthogonalize_probe_modes()
    assert s2.probe_t == 0 and not np.any(s2.probe_m) and not np.any(s2.probe_v)
    err = float(np.abs(powers - (0.7, 0.3)).max())
    s1, epochs1 = fit(truth[0] * np.sqrt(1. / 0.7))                   # one mode carrying the whole power
    ratio = float(epochs1[-1] / epochs2[-1])
    rising = int(np.sum(np.diff(epochs2) > 0))
    print('recovery: two-mode loss per epoch', epochs2[0], '->', epochs2[-1], 'epochs in which it rose', rising, 'of', len(epochs2) - 1,
          '\n   relative powers', modes.relative_power(start), '->', powers, 'largest error against (0.7, 0.3)', err,
          '\n   single-mode loss per epoch', epochs1[0], '->', epochs1[-1], 'ratio single / two modes', ratio)
    assert rising == 0
    assert err < abs(modes.relative_power(start)[1] - 0.3)
    assert err <= POWER_ERROR_BOUND
    assert ratio >= LOSS_RATIO_BOUND


# ---- the entry point and the simulator -----------------------------------------------------------------------------------------------------
E_PSZ = 20


def _write_case(tmp_path):
    from beyond_dof_amd import h5io, modes, util
    from beyond_dof_amd.solver import PtychoSolver
    od, ob = _volume()
    g = util.gaussian_probe((E_PSZ, E_PSZ), 4., 4., 0.5)
    truth = modes.initial_modes(g[0] + 1j * g[1], 2, 3. / 7.)
    sim = PtychoSolver(SHAPE, (E_PSZ, E_PSZ), POS, N_THETA, len(POS), E, PS, truth.real, truth.imag)
    sim.set_volume(od, ob)
    data = np.stack([np.sqrt(np.sum(np.abs(sim.forward(t, IDX)) ** 2, axis=0)) for t in range(N_THETA)])
    os.makedirs(os.path.join(str(tmp_path), 'case'), exist_ok=True)
    h5io.write_dataset(os.path.join(str(tmp_path), 'case', 'data.h5'), 'exchange/data', data.astype(np.complex64))
    return od, ob, truth


def _reconstruct(tmp_path, out, **kw):
    from beyond_dof_amd.ptychography import reconstruct_ptychography
    od, ob = _volume()
    return reconstruct_ptychography('data.h5', POS, (E_PSZ, E_PSZ), SHAPE, theta_st=0, theta_end=2 * np.pi, n_epochs=2, learning_rate=1e-7,
                                    minibatch_size=len(POS), energy_ev=E, psize_cm=PS, save_path=os.path.join(str(tmp_path), 'case'),
                                    output_folder=out, initial_guess=[0.5 * od, 0.5 * ob], seed=1, probe_mag_sigma=4., probe_phase_sigma=4.,
                                    probe_phase_max=0.5, **kw)


def test_reconstruct_ptychography_with_two_optimisable_modes(built, tmp_path):
    from beyond_dof_amd import modes, util
    _write_case(tmp_path)
    g = util.gaussian_probe((E_PSZ, E_PSZ), 4., 4., 0.5)
    mag, phase = np.abs(g[0] + 1j * g[1]), np.angle(g[0] + 1j * g[1])
    d, b = _reconstruct(tmp_path, 'out', n_probe_modes=2, probe_type='optimizable', probe_initial=[mag, phase], probe_learning_rate=1e-3)
    assert d.shape == SHAPE and np.all(np.isfinite(d)) and np.all(np.isfinite(b))
    rec = np.load(os.path.join(str(tmp_path), 'case', 'out', 'probe_modes.npy'))
    assert rec.shape == (2, E_PSZ, E_PSZ) and np.iscomplexobj(rec) and np.all(np.isfinite(rec))
    flat = rec.reshape(2, -1)
    gram = flat @ flat.conj().T
    assert abs(gram[0, 1]) <= 1e-10 * gram[0, 0].real and gram[0, 0].real >= gram[1, 1].real        # orthogonalised at the end of the last epoch
    text = open(os.path.join(str(tmp_path), 'case', 'out', 'summary.txt')).read()
    line = [l for l in text.splitlines() if l.startswith('probe_mode_power')]
    print(line)
    assert len(line) == 1 and len(line[0].split()) == 3
    assert np.allclose([float(v) for v in line[0].split()[1:]], modes.relative_power(rec), rtol=1e-5)
    # probe_initial that already holds the modes is taken as it is; a count that contradicts it raises
    m0 = modes.initial_modes(g[0] + 1j * g[1], 2, 0.1)
    with pytest.raises(ValueError, match='n_probe_modes'):
        _reconstruct(tmp_path, 'out3', n_probe_modes=3, probe_type='fixed', probe_initial=[np.abs(m0), np.angle(m0)])
    _reconstruct(tmp_path, 'out2', n_probe_modes=2, probe_type='fixed', probe_initial=[np.abs(m0), np.angle(m0)])
    assert rel(np.load(os.path.join(str(tmp_path), 'case', 'out2', 'probe_modes.npy')), m0) <= 1e-12
    for bad in (dict(propagator='conv'), dict(slice_binning=2), dict(adjoint_precision='float64')):
        with pytest.raises(ValueError, match='probe modes'):
            _reconstruct(tmp_path, 'out4', n_probe_modes=2, **bad)


def test_one_probe_mode_is_the_run_without_the_keyword(built, tmp_path):
    _write_case(tmp_path)
    a = _reconstruct(tmp_path, 'plain')
    c = _reconstruct(tmp_path, 'one', n_probe_modes=1)
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
    assert not os.path.exists(os.path.join(str(tmp_path), 'case', 'one', 'probe_modes.npy'))


def test_solvers_refuse_what_does_not_carry_modes(built):
    from beyond_dof_amd.solver import FullfieldSolver, PtychoSolver
    m = _modes(20)
    with pytest.raises(ValueError, match='probe modes'):
        FullfieldSolver(32, 32, 16, 2, 1, E, PS, probe_real=np.ones((2, 32, 32)), probe_imag=np.zeros((2, 32, 32)))
    for bad in (dict(propagator='conv'), dict(slice_binning=2), dict(adjoint64=True), dict(adjoint64='first'), dict(engine='streaming')):
        with pytest.raises(ValueError, match='probe modes'):
            PtychoSolver(SHAPE, (20, 20), POS, N_THETA, len(POS), E, PS, m.real, m.imag, **bad)
    s = _solver(20, _problem(20))
    with pytest.raises(ValueError, match='enable_probe_optimization'):
        s.enable_probe_optimization(m[0].real, m[0].imag)
    with pytest.raises(ValueError, match='orthogonalize_probe_modes'):
        s.orthogonalize_probe_modes()


def test_simulated_data_is_the_root_of_the_summed_intensities(built, tmp_path):
    """create_ptychography_data_batch_numpy(probe_modes=...) against its own simulations of one mode each"""
    from beyond_dof_amd import modes, simulation, util
    od, ob = _volume()
    np.save(os.path.join(str(tmp_path), 'grid_delta.npy'), od)
    np.save(os.path.join(str(tmp_path), 'grid_beta.npy'), ob)
    g = util.gaussian_probe((E_PSZ, E_PSZ), 4., 4., 0.5)
    m = modes.initial_modes(g[0] + 1j * g[1], 2, 0.3)
    kw = dict(probe_size=(E_PSZ, E_PSZ), theta_end=np.pi, probe_circ_mask=None, minibatch_size=5)
    both = simulation.create_ptychography_data_batch_numpy(E, PS, 2, str(tmp_path), str(tmp_path), 'both.h5', POS, probe_modes=m, **kw)
    single = [simulation.create_ptychography_data_batch_numpy(E, PS, 2, str(tmp_path), str(tmp_path), 'mode{}.h5'.format(i), POS,
                                                              probe_modes=m[i:i + 1], **kw) for i in range(2)]
    want = np.sqrt(np.abs(single[0]) ** 2 + np.abs(single[1]) ** 2)
    e = rel(both.real, want)
    print('simulated modes against the root of the summed single-mode intensities', e, 'largest imaginary part', np.abs(both.imag).max())
    assert both.shape == (2, len(POS), E_PSZ, E_PSZ) and e <= 1e-6 and not np.any(both.imag)
