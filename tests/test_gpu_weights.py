"""Detector weights (bdof_set_detector_weights, MultisliceEngine.set_detector_weights, detector_weights=...) on the device, through
every engine that forms a seed on the transfer-function path, against the float64 reference of tests/reference_model.py under tests/weights_reference.py's data term.

Bounds: those of tests/test_gpu_poisson.py — loss relative 1e-5, gradients relative L2 2e-4 — because a weight is one exact
float32 factor on a seed and on two sums whose error those bounds already cover; the float64 twin at 1e-8 / 2e-7.  Under a
beamstop the gradient's error is stated over the norm of the UNWEIGHTED reference gradient of the same case (masking DC removes
most of the seed and none of the float32 error of the transforms); the error over the weighted norm is printed beside it.  The
exact checks have no tolerance.  Every test prints what it measured before it asserts."""
import functools
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import bdof_oracle as orc

import reference_model as ref_model
import weights_reference as wref

MU = 2e6
E, PS = 5000., 1e-7
B, S = 2, 6
LOSSES = ['lsq', 'poisson']
JUNK = np.array([np.nan, np.inf, 1e30, -1.0])


def rel(a, b, over=None):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b if over is None else over), 1e-300)


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


@functools.lru_cache(maxsize=None)
def _data(Y, X, fp, probe, seed=0, f32=False):
    """Object, probe, amplitudes m = |ref| |1 + 0.05 N| and a weight plane; f32: the inputs rounded as the float64 twin reads them."""
    rng = np.random.default_rng(seed)
    delta = rng.uniform(0, 2e-5, size=(B, Y, X, S))
    beta = 0.1 * delta
    pr, pi = _probe(probe, Y, X, rng)
    if f32:
        delta, beta = delta.astype(np.float32).astype(np.float64), beta.astype(np.float32).astype(np.float64)
        p = (np.asarray(pr) + 1j * np.asarray(pi)).astype(np.complex64)
        pr, pi = p.real.astype(np.float64), p.imag.astype(np.float64)
    ref, _ = ref_model.forward(delta, beta, pr, pi, E, PS, fp)
    meas = np.abs(ref) * np.abs(1 + 0.05 * rng.normal(size=ref.shape))
    if f32:
        meas = meas.astype(np.float32).astype(np.float64)
    w = wref.random_weights((Y, X), rng)
    for a in (delta, beta, meas, w):
        a.setflags(write=False)
    return delta, beta, pr, pi, meas, w


def _term(w, loss_type):
    return ref_model.data_term(wref.weighted_loss, wref.weighted_seed, w, loss_type, MU)


@functools.lru_cache(maxsize=None)
def _reference(Y, X, fp, probe, loss_type, weights='random', seed=0, f32=False):
    """The reference's (loss, g_delta, g_beta, g_probe) of a _data case: computed once, shared, never written to."""
    delta, beta, pr, pi, meas, w = _data(Y, X, fp, probe, seed, f32)
    w = {'random': w, 'beamstop': wref.beamstop((Y, X)), 'none': np.ones((Y, X), dtype=np.float32)}[weights]
    out = ref_model.loss_and_grad(delta, beta, pr, pi, E, PS, meas, fp, term=_term(w, loss_type))[:4]
    for a in out[1:]:
        a.setflags(write=False)
    return out


def _engine(engine_mod, Y, X, fp, probe, seed=0, f32=False, **kw):
    delta, beta, pr, pi, meas, w = _data(Y, X, fp, probe, seed, f32)
    eng = engine_mod.MultisliceEngine(Y, X, S, B, with_grad=True, **kw)
    eng.set_physics(E, PS, fp)
    eng.set_probe(pr, pi)
    eng.set_object_batch(delta, beta)
    return eng, meas, w


def _grot_bytes(eng):
    """The rotated-frame gradient rows of the last loss_grad as they lie in bdof_grot."""
    n = B * S * eng.nx * eng.ny
    out = np.empty(2 * n, dtype=np.float32)
    eng.ctx.check(eng.lib.bdof_memcpy_d2h(eng.h, out.ctypes.data, eng.lib.bdof_grot(eng.h), n * 8))
    return out.tobytes()


# 64 x 256: a transposed plane shows; 72: resident without a fused plan; 64: resident with one; 96 x 80: generic, not square
ENGINE_SHAPES = [('streaming', 128, 128), ('streaming', 64, 256), ('resident', 72, 72), ('resident', 64, 64), ('resident', 128, 128),
                 ('generic', 64, 64), ('generic', 96, 80)]


# ---- 1. against the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('engine,Y,X', ENGINE_SHAPES)
@pytest.mark.parametrize('fp', [None, 1e-4, 'inf'])
@pytest.mark.parametrize('probe', ['plane', 'random', 'gaussian'])
@pytest.mark.parametrize('loss_type', LOSSES)
def test_weighted_loss_and_gradient_vs_reference(engine_mod, engine, Y, X, fp, probe, loss_type):
    """'plane': residual splitting (with 'inf' the float64 DC bin and the adjoint carrier, on the streaming or generic engine
    whatever `engine` says); 'random': a scalar carrier under a structured probe; 'gaussian': the float64 carrier field."""
    eng, meas, w = _engine(engine_mod, Y, X, fp, probe, engine=engine)
    eng.set_loss(loss_type, MU)
    eng.set_detector_weights(w)
    loss = eng.loss_grad(B, meas)
    gd, gb = eng.grad_batch_to_host(B)
    rl, rgd, rgb, _ = _reference(Y, X, fp, probe, loss_type)
    e = (abs(loss - rl) / abs(rl), rel(gd, rgd), rel(gb, rgb))
    unweighted = np.linalg.norm(_reference(Y, X, fp, probe, loss_type, 'none')[1])
    print('weights parity', engine, (Y, X), fp, probe, loss_type, 'loss / g_delta / g_beta rel err', e,
          '|g_delta| weighted / unweighted', np.linalg.norm(rgd) / unweighted)
    assert e[0] <= 1e-5, e
    assert e[1] <= 2e-4 and e[2] <= 2e-4, e


@pytest.mark.parametrize('Y,X', [(64, 64), (72, 72), (64, 256)])
@pytest.mark.parametrize('fp', [None, 1e-4, 'inf'])
@pytest.mark.parametrize('loss_type', LOSSES)
def test_weighted_float64_twin_vs_reference(engine_mod, Y, X, fp, loss_type):
    """bdof_loss_grad_tf_f64 under weights: cases, rounding of the inputs and bounds of test_poisson_float64_twin_vs_reference
    (loss 1e-8; gradient rows are stored as float32: 2e-7)."""
    probe = 'gaussian' if fp == 'inf' else 'random'
    eng, meas, w = _engine(engine_mod, Y, X, fp, probe, f32=True)
    eng.set_loss(loss_type, MU)
    eng.set_detector_weights(w)
    eng.enable_tf_f64()
    loss = eng.loss_grad(B, meas, f64=True)
    gd, gb = eng.grad_batch_to_host(B)
    rl, rgd, rgb, _ = _reference(Y, X, fp, probe, loss_type, f32=True)
    e = (abs(loss - rl) / abs(rl), rel(gd, rgd), rel(gb, rgb))
    print('weights float64 twin', (Y, X), fp, loss_type, e)
    assert e[0] <= 1e-8 and e[1] <= 2e-7 and e[2] <= 2e-7, e


# ---- 2. beamstop ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('engine,Y,X', [('streaming', 128, 128), ('streaming', 64, 256), ('resident', 72, 72), ('generic', 96, 80)])
@pytest.mark.parametrize('probe', ['plane', 'gaussian'])
@pytest.mark.parametrize('loss_type', LOSSES)
def test_beamstop_over_the_dc_bin(engine_mod, engine, Y, X, probe, loss_type):
    """Far field, w = 0 on a disc of radius 3 around the centre of the shifted frame.  The gradient's error over the norm of the
    unweighted reference gradient is held to 2e-4; over the weighted norm it is printed (MEASUREMENTS.md has both per engine).
    Where the adjoint carrier runs (plane wave: streaming and generic engines) gcar and gt0 come out exactly 0."""
    eng, meas, _ = _engine(engine_mod, Y, X, 'inf', probe, engine=engine)
    w = wref.beamstop((Y, X))
    assert w[Y // 2, X // 2] == 0 and (w == 0).sum() == 29
    eng.set_loss(loss_type, MU)
    carrier = None
    if probe == 'plane':
        eng.loss_grad(B, meas)
        carrier = eng.adjoint_carrier(B)
        assert carrier is not None and np.all(np.abs(carrier[0]) > 0) and np.all(np.abs(carrier[1]) > 0)
    eng.set_detector_weights(w)
    loss = eng.loss_grad(B, meas)
    gd, gb = eng.grad_batch_to_host(B)
    rl, rgd, rgb, _ = _reference(Y, X, 'inf', probe, loss_type, 'beamstop')
    _, ugd, ugb, _ = _reference(Y, X, 'inf', probe, loss_type, 'none')
    e = (abs(loss - rl) / abs(rl), rel(gd, rgd, ugd), rel(gb, rgb, ugb))
    print('beamstop', engine, (Y, X), probe, loss_type, 'loss rel err', e[0], 'g_delta / g_beta err over the unweighted norm', e[1:],
          'over the weighted norm', (rel(gd, rgd), rel(gb, rgb)), '|g| weighted / unweighted', np.linalg.norm(rgd) / np.linalg.norm(ugd))
    assert e[0] <= 1e-5, e
    assert e[1] <= 2e-4 and e[2] <= 2e-4, e
    if probe == 'plane':
        carrier = eng.adjoint_carrier(B)
        assert carrier is not None
        assert np.all(carrier[0] == 0) and np.all(carrier[1] == 0), carrier
    else:
        assert eng.adjoint_carrier(B) is None


# ---- 3. exact checks -----------------------------------------------------------------------------------------------------------
EXACT = [('streaming', 128, 128, 1e-4, 'plane'), ('streaming', 64, 256, 'inf', 'plane'), ('streaming', 128, 128, 'inf', 'gaussian'),
         ('resident', 72, 72, None, 'plane'), ('resident', 72, 72, 'inf', 'gaussian'), ('resident', 64, 64, 1e-4, 'random'),
         ('generic', 96, 80, None, 'random'), ('generic', 96, 80, 'inf', 'plane'), ('generic', 96, 80, 1e-4, 'gaussian')]


@pytest.mark.parametrize('engine,Y,X,fp,probe', EXACT)
@pytest.mark.parametrize('loss_type', LOSSES)
def test_unit_weights_and_cleared_weights_are_no_weights(engine_mod, engine, Y, X, fp, probe, loss_type):
    """w = 1 everywhere: the loss (a double) and the bytes of bdof_grot equal those of an engine that never heard of weights; after
    a visit with real weights, set_detector_weights(None) gives them again."""
    eng, meas, w = _engine(engine_mod, Y, X, fp, probe, engine=engine)
    eng.set_loss(loss_type, MU)
    l0 = eng.loss_grad(B, meas)
    g0 = _grot_bytes(eng)
    eng.set_detector_weights(np.ones((Y, X)))
    l1 = eng.loss_grad(B, meas)
    g1 = _grot_bytes(eng)
    eng.set_detector_weights(w)
    lw = eng.loss_grad(B, meas)
    gw = _grot_bytes(eng)
    eng.set_detector_weights(None)
    assert eng.detector_weights is None
    l2 = eng.loss_grad(B, meas)
    g2 = _grot_bytes(eng)
    assert lw != l0 and gw != g0          # the visit did something
    assert l1 == l0 and g1 == g0
    assert l2 == l0 and g2 == g0


@pytest.mark.parametrize('engine,Y,X,fp,probe', EXACT)
@pytest.mark.parametrize('loss_type', LOSSES)
def test_amplitudes_under_a_zero_weight_take_no_part(engine_mod, engine, Y, X, fp, probe, loss_type):
    """NaN, inf, 1e30 and -1 in the w = 0 pixels: loss and bdof_grot bit-identical to amplitudes that hold 0 there."""
    eng, meas, w = _engine(engine_mod, Y, X, fp, probe, engine=engine)
    eng.set_loss(loss_type, MU)
    eng.set_detector_weights(w)
    rng = np.random.default_rng(1)
    clean, dirty = meas.copy(), meas.copy()
    clean[:, w == 0] = 0.0
    dirty[:, w == 0] = JUNK[rng.integers(0, len(JUNK), size=dirty[:, w == 0].shape)]
    la = eng.loss_grad(B, clean)
    ga = _grot_bytes(eng)
    lb = eng.loss_grad(B, dirty)
    gb = _grot_bytes(eng)
    assert np.isfinite(la) and np.isfinite(np.frombuffer(ga, dtype=np.float32)).all()
    assert la == lb and ga == gb


def _solver_case(kind, weights, coords):
    from beyond_dof_amd.solver import FullfieldSolver, PtychoSolver
    n = 64
    if kind == 'fullfield':
        return FullfieldSolver(n, n, n, 4, 2, E, PS, free_prop_cm=1e-4, coord_ls=coords, detector_weights=weights)
    prr, pii = orc.gaussian_probe((36, 36), 6., 6., 0.5)
    return PtychoSolver((n, n, n), (36, 36), PTY_POS, 3, len(PTY_POS), E, PS, prr, pii, coord_ls=coords, detector_weights=weights)


PTY_POS = np.array([(32, 32), (20, 40), (5, 62), (60, 3)])          # test_ptycho_solver_window_path's: windows over the volume's edge


@pytest.mark.parametrize('kind', ['fullfield', 'ptycho'])
def test_solver_measurements_under_a_zero_weight_take_no_part(engine_mod, kind):
    """set_measurements of both solvers goes through meas_layout: the resident amplitude stacks of junk and of zeros are the same
    bytes, and so are loss and volume gradient."""
    n = 64
    rng = np.random.default_rng(2)
    od = rng.uniform(0, 2e-5, size=(n, n, n))
    ob = 0.1 * od
    shape = (4, n, n) if kind == 'fullfield' else (3, len(PTY_POS), 36, 36)
    coords = orc.rotation_lookup([n, n, n], shape[0])
    w = wref.random_weights(shape[-2:], rng)
    meas = 1 + 0.05 * rng.normal(size=shape) if kind == 'fullfield' else rng.uniform(0, 30, size=shape)
    clean, dirty = meas.copy(), meas.copy()
    clean[..., w == 0] = 0.0
    dirty[..., w == 0] = JUNK[rng.integers(0, len(JUNK), size=dirty[..., w == 0].shape)]
    out = []
    for m in (clean, dirty):
        s = _solver_case(kind, w, coords)
        s.set_volume(od, ob)
        s.set_measurements(m)
        stack = (s.meas if kind == 'fullfield' else s.meas_all)
        raw = stack.download((int(np.prod(shape)),), np.float32).tobytes()
        loss = s.loss_and_grad([1, 3]) if kind == 'fullfield' else s.loss_and_grad(1, np.arange(len(PTY_POS)))
        gd, gb = s.gradient_to_host()
        out.append((raw, loss, gd.tobytes(), gb.tobytes()))
    assert np.isfinite(out[0][1]) and np.isfinite(np.frombuffer(out[0][0], dtype=np.float32)).all()
    assert out[0] == out[1]


# ---- 4. settings that only move the seed on ------------------------------------------------------------------------------------
@pytest.mark.parametrize('setting', ['recompute', 'adjoint64', 'probe_grad', 'fused'])
def test_weights_seed_only_settings(engine_mod, setting):
    """The tape-free adjoint, the float64 adjoint sweep (generic engine), the probe gradient, and the fused forward + adjoint
    sweeps (64 x 64, near field, plane wave): the seed is weighted before any of them sees it."""
    fp, loss_type = 1e-4, 'lsq'
    kw = {'recompute': dict(recompute=True), 'adjoint64': dict(engine='generic', adjoint64=True), 'probe_grad': {},
          'fused': dict(engine='streaming')}[setting]
    probe = 'plane' if setting == 'fused' else 'random'
    eng, meas, w = _engine(engine_mod, 64, 64, fp, probe, seed=4, **kw)
    eng.set_detector_weights(w)
    if setting == 'probe_grad':
        eng.enable_probe_grad(True)
    if setting == 'fused':
        eng.set_sweep_fusion(1)
        eng.set_adjoint_fusion(True)
    loss = eng.loss_grad(B, meas)
    if setting == 'fused':
        assert (eng.sweep_fused, eng.adjoint_fused) == (1, 1)
    gd, gb = eng.grad_batch_to_host(B)
    rl, rgd, rgb, g0 = _reference(64, 64, fp, probe, loss_type, seed=4)
    e = [abs(loss - rl) / abs(rl), rel(gd, rgd), rel(gb, rgb)]
    if setting == 'probe_grad':
        e.append(rel(eng.probe_grad(), g0.sum(axis=0)))
    print('weights', setting, 'loss / g_delta / g_beta (/ g_probe) rel err', e)
    assert e[0] <= 1e-5, e
    assert max(e[1:]) <= 2e-4, e


# ---- 5. solvers ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('loss_type', LOSSES)
def test_fullfield_solver_with_weights_64_cubed(engine_mod, loss_type):
    """FullfieldSolver(detector_weights=...) at 64^3, two angles: rotation -> reference -> rotation adjoint."""
    from beyond_dof_amd.solver import FullfieldSolver
    n, n_theta, fp = 64, 4, 1e-4
    rng = np.random.default_rng(6)
    od = rng.uniform(0, 2e-5, size=(n, n, n))
    ob = 0.1 * od
    coords = orc.rotation_lookup([n, n, n], n_theta)
    one, zero = np.ones((n, n)), np.zeros((n, n))
    idx = [1, 3]
    rot = np.stack([orc.apply_rotation(np.stack([od, ob], axis=3), coords[j]) for j in idx])
    ref, _ = ref_model.forward(rot[..., 0], rot[..., 1], one, zero, E, PS, fp)
    w = wref.random_weights((n, n), rng)
    meas = np.ones((n_theta, n, n))
    meas[idx] = np.abs(ref) * np.abs(1 + 0.05 * rng.normal(size=ref.shape))
    meas[:, w == 0] = np.nan
    s = FullfieldSolver(n, n, n, n_theta, 2, E, PS, free_prop_cm=fp, coord_ls=coords, loss_type=loss_type, poisson_multiplier=MU,
                        detector_weights=w)
    s.set_measurements(meas)
    s.set_volume(od, ob)
    loss = s.loss_and_grad(idx)
    gd, gb = s.gradient_to_host()
    rl, rgd, rgb, _, _ = ref_model.loss_and_grad(rot[..., 0], rot[..., 1], one, zero, E, PS, meas[idx], fp, term=_term(w, loss_type))
    wd = sum(orc.apply_rotation_adjoint(rgd[k], coords[j]) for k, j in enumerate(idx))
    wb = sum(orc.apply_rotation_adjoint(rgb[k], coords[j]) for k, j in enumerate(idx))
    e = (abs(loss - rl) / abs(rl), rel(gd, wd), rel(gb, wb))
    print('weights, full-field solver 64^3', loss_type, e)
    assert e[0] <= 1e-5 and e[1] <= 2e-4 and e[2] <= 2e-4, e


@pytest.mark.parametrize('loss_type', LOSSES)
def test_ptycho_solver_with_beamstop_and_dead_pixels(engine_mod, loss_type):
    """PtychoSolver(detector_weights=...) at 64^3 with a 36 x 36 probe (far field): a beamstop plus scattered dead pixels, windows
    over the volume's edge; rotation, windows and their adjoints are the oracle's."""
    from beyond_dof_amd.solver import PtychoSolver
    n, n_theta, i_theta, psz = 64, 3, 1, (36, 36)
    rng = np.random.default_rng(0)
    od = rng.uniform(0, 2e-5, size=(n, n, n))
    ob = 0.1 * od
    coords = orc.rotation_lookup([n, n, n], n_theta)
    prr, pii = orc.gaussian_probe(psz, 6., 6., 0.5)
    w = wref.beamstop(psz) * (wref.random_weights(psz, rng) > 0)
    assert w[18, 18] == 0 and 40 < (w == 0).sum() < 300
    s = PtychoSolver((n, n, n), psz, PTY_POS, n_theta, len(PTY_POS), E, PS, prr, pii, coord_ls=coords, loss_type=loss_type,
                     poisson_multiplier=MU, detector_weights=w)
    s.set_volume(od, ob)
    sel = np.arange(len(PTY_POS))
    wave = s.forward(i_theta, sel)
    meas = np.abs(wave).astype(np.float64) * np.abs(1 + 0.05 * rng.normal(size=wave.shape))
    meas[:, w == 0] = 1e6           # the direct beam behind the stop, hot pixels
    loss = s.loss_and_grad(i_theta, sel, meas)
    gd, gb = s.gradient_to_host()
    rl, rgd, rgb = ref_model.ptycho_loss_and_grad(od, ob, coords[i_theta], PTY_POS, PTY_POS[sel], meas, prr, pii, psz, E, PS,
                                                  term=_term(w, loss_type))
    e = (abs(loss - rl) / abs(rl), rel(gd, rgd), rel(gb, rgb))
    print('weights, ptychography solver', loss_type, 'loss / g_delta / g_beta rel err', e)
    assert e[0] <= 1e-5 and e[1] <= 2e-4 and e[2] <= 2e-4, e


# ---- 6. entry points -----------------------------------------------------------------------------------------------------------
def _losses_printed(text):
    return [float(v) for v in re.findall(r'Epoch \d+ \(rank 0\); loss = ([-+.\deE]+|nan|inf)', text)]


def _tiffs(folder):
    from beyond_dof_amd import tiffio
    return [np.asarray(tiffio.read_tiff(os.path.join(folder, name))) for name in ('delta_ds_1', 'beta_ds_1')]


def test_reconstruct_ptychography_with_weights(engine_mod, tmp_path, monkeypatch, capsys):
    """Data and sizes of test_poisson_ptychography_lowers_its_loss.  Run A: clean data + weights; run B: the same data with 1e6 and NaN
    in the w = 0 pixels, same weights, same seed — the written delta_ds_1 / beta_ds_1 are the same bits; by dataset name they are
    again; the printed loss falls; a multiscale_level=2 run goes through."""
    from beyond_dof_amd import h5io
    from beyond_dof_amd.ptychography import reconstruct_ptychography
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
        data[t], _ = ref_model.forward(subs[..., 0], subs[..., 1], prr, pii, E, PS, 'inf')
    w = (wref.beamstop(psz) * (wref.random_weights(psz, rng) > 0)).astype(np.float32)
    dirty = data.copy()
    zero = np.argwhere(w == 0)
    for j, (y, x) in enumerate(zero):
        dirty[:, :, y, x] = np.nan if j % 2 else 1e6
    os.makedirs('case')
    h5io.write_dataset('case/clean.h5', 'exchange/data', data)
    h5io.write_datasets('case/dirty.h5', {'exchange/data': dirty, 'exchange/weights': w})
    init_d, init_b = np.full((n, n, n), 8e-6), np.full((n, n, n), 8e-7)

    def run(fname, weights, out, **kw):
        capsys.readouterr()
        kw.setdefault('initial_guess', [init_d, init_b])
        reconstruct_ptychography(fname, [tuple(p) for p in pos], psz, (n, n, n), theta_st=0, theta_end=2 * np.pi, n_epochs=2,
                                 learning_rate=2e-7, minibatch_size=3, energy_ev=E, psize_cm=PS, save_path='case', output_folder=out,
                                 probe_type='gaussian', seed=3, probe_mag_sigma=6., probe_phase_sigma=6.,
                                 probe_phase_max=0.5, detector_weights=weights, **kw)
        return _losses_printed(capsys.readouterr().out)

    la = run('clean.h5', w, 'out_a')
    lb = run('dirty.h5', w, 'out_b')
    lc = run('dirty.h5', 'exchange/weights', 'out_c')
    with capsys.disabled():
        print('ptychography with weights, printed losses', la, lb, lc)
    a, b, c = _tiffs('case/out_a'), _tiffs('case/out_b'), _tiffs('case/out_c')
    for x, y, z in zip(a, b, c):
        assert np.isfinite(x).all()
        assert x.tobytes() == y.tobytes() == z.tobytes()
    assert la == lb == lc and len(la) == 2 and np.isfinite(la).all()
    assert la[-1] < la[0], la
    run('dirty.h5', 'exchange/weights', 'out_ms', multiscale_level=2, initial_guess=[init_d[::2, ::2, ::2], init_b[::2, ::2, ::2]])
    assert all(np.isfinite(x).all() for x in _tiffs('case/out_ms'))
    with pytest.raises(ValueError, match='detector_weights'):
        run('dirty.h5', w, 'out_conv', propagator='conv')


def test_reconstruct_fullfield_with_weights(engine_mod, tmp_path, monkeypatch, capsys):
    """The full-field sibling (64^3, near-field detector, eight angles): runs A and B bit-identical, the plane by dataset name too,
    the printed loss falls, a multiscale_level=2 run goes through, propagator='conv' is refused."""
    from beyond_dof_amd import h5io
    from beyond_dof_amd.fullfield import reconstruct_fullfield
    monkeypatch.chdir(tmp_path)
    n, n_theta, mb, fp = 64, 8, 4, 1e-4
    rng = np.random.default_rng(11)
    z, y, x = np.mgrid[:n, :n, :n]
    true_d = np.zeros((n, n, n))
    for _ in range(6):
        c = rng.uniform(n * 0.3, n * 0.7, size=3)
        r = rng.uniform(n * 0.08, n * 0.2)
        true_d += 1e-6 * np.exp(-((z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2) / (2 * r ** 2))
    true_b = 0.1 * true_d
    coords = orc.rotation_lookup([n, n, n], n_theta)
    one, zero = np.ones((n, n)), np.zeros((n, n))
    rot = np.stack([orc.apply_rotation(np.stack([true_d, true_b], axis=3), c) for c in coords])
    prj, _ = ref_model.forward(rot[..., 0], rot[..., 1], one, zero, E, PS, fp)
    data = prj.astype(np.complex64)
    w = wref.random_weights((n, n), rng)
    dirty = data.copy()
    for j, (yy, xx) in enumerate(np.argwhere(w == 0)):
        dirty[:, yy, xx] = np.nan if j % 2 else 1e6
    os.makedirs('case')
    h5io.write_dataset('case/clean.h5', 'exchange/data', data)
    h5io.write_datasets('case/dirty.h5', {'exchange/data': dirty, 'exchange/weights': w})
    init_d, init_b = np.full((n, n, n), 8.7e-7), np.full((n, n, n), 5.1e-8)

    def run(fname, weights, out, **kw):
        capsys.readouterr()
        kw.setdefault('initial_guess', [init_d, init_b])
        reconstruct_fullfield(fname, theta_st=0, theta_end=2 * np.pi, n_epochs=3, learning_rate=1e-7, minibatch_size=mb, energy_ev=E,
                              psize_cm=PS, free_prop_cm=fp, save_path='case', output_folder=out, shrink_cycle=None, seed=7, alpha_d=0.,
                              alpha_b=0., gamma=0., detector_weights=weights, **kw)
        return _losses_printed(capsys.readouterr().out)

    la = run('clean.h5', w, 'out_a')
    lb = run('dirty.h5', w, 'out_b')
    lc = run('dirty.h5', 'exchange/weights', 'out_c')
    with capsys.disabled():
        print('full field with weights, printed losses', la, lb, lc)
    a, b, c = _tiffs('case/out_a'), _tiffs('case/out_b'), _tiffs('case/out_c')
    for u, v, t in zip(a, b, c):
        assert np.isfinite(u).all()
        assert u.tobytes() == v.tobytes() == t.tobytes()
    assert la == lb == lc and len(la) == 3 and np.isfinite(la).all()
    assert la[-1] < la[0], la
    run('dirty.h5', 'exchange/weights', 'out_ms', multiscale_level=2, initial_guess=[init_d[::2, ::2, ::2], init_b[::2, ::2, ::2]])
    assert all(np.isfinite(u).all() for u in _tiffs('case/out_ms'))
    with pytest.raises(ValueError, match='detector_weights'):
        run('dirty.h5', w, 'out_conv', propagator='conv')


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------
def test_paths_without_detector_weights_raise(engine_mod):
    """The real-space propagator (float32 and float64) and the tiled propagator's field loss carry no weights: with weights set
    they fail through bdof_last_error, naming detector weights; cleared, they run again and give what they gave."""
    from beyond_dof_amd import _lib
    from beyond_dof_amd.solver import FullfieldSolver, PtychoSolver
    Y = X = 64
    eng, meas, w = _engine(engine_mod, Y, X, None, 'plane')
    eng.set_conv(E, PS, 5)
    delta, beta = _data(Y, X, None, 'plane')[:2]
    eng.set_object_batch(delta, beta)
    l_conv = eng.loss_grad(B, meas, conv=True)
    field = _lib.DeviceBuffer.from_host(eng.ctx, np.ones((X, Y), dtype=np.complex64))
    m1 = _lib.DeviceBuffer.from_host(eng.ctx, np.full((X, Y), 0.9, dtype=np.float32))
    eng.ctx.check(eng.lib.bdof_field_loss_seed(eng.h, field.ptr, m1.ptr, X, Y))
    eng.set_detector_weights(w)
    with pytest.raises(_lib.BdofError, match='detector weights'):
        eng.loss_grad(B, meas, conv=True)
    assert b'detector weights' in eng.lib.bdof_last_error(eng.h)
    with pytest.raises(_lib.BdofError, match='detector weights'):
        eng.ctx.check(eng.lib.bdof_field_loss_seed(eng.h, field.ptr, m1.ptr, X, Y))
    eng.enable_conv_f64()
    with pytest.raises(_lib.BdofError, match='detector weights'):
        eng.loss_grad(B, meas, conv=True, f64=True)
    for bad in (np.ones((X + 1, Y)), np.ones((1, Y, X)), -np.ones((Y, X)), np.full((Y, X), np.nan), np.zeros((Y, X)),
                np.where(np.arange(Y * X).reshape(Y, X) == 7, np.inf, 1.0)):
        with pytest.raises(ValueError, match='detector_weights'):
            eng.set_detector_weights(bad)
    assert np.array_equal(eng.detector_weights, w)          # the refused calls left the setting whole
    eng.set_detector_weights(None)
    assert eng.loss_grad(B, meas, conv=True) == l_conv
    with pytest.raises(ValueError, match='detector_weights'):
        FullfieldSolver(64, 64, 64, 2, 1, E, PS, propagator='conv', detector_weights=np.ones((64, 64)))
    prr, pii = orc.gaussian_probe((36, 36), 6., 6., 0.5)
    with pytest.raises(ValueError, match='detector_weights'):
        PtychoSolver((64, 64, 64), (36, 36), PTY_POS, 3, 4, E, PS, prr, pii, propagator='conv', detector_weights=np.ones((36, 36)))


def test_the_library_clears_the_weights_on_configure_and_refuses_them_before(engine_mod):
    """bdof_set_detector_weights before bdof_configure is a state error; bdof_configure clears the weights (the shape may change)."""
    import ctypes
    from beyond_dof_amd import _lib
    ctx = _lib.Context(0, None)
    lib, h = ctx.lib, ctx.handle
    one = np.ones((64, 64), dtype=np.float32)
    assert lib.bdof_set_detector_weights(h, one.ctypes.data) == -2
    assert b'bdof_configure' in lib.bdof_last_error(h)
    eng, meas, w = _engine(engine_mod, 64, 64, 1e-4, 'plane', engine='streaming')
    l0 = eng.loss_grad(B, meas)
    eng.set_detector_weights(w)
    lw = eng.loss_grad(B, meas)
    assert lw != l0
    # the same geometry again on the same ctx: nothing of the weights is left
    eng.ctx.check(eng.lib.bdof_configure(eng.h, 64, 64, S, B, _lib.CFG_GRAD | _lib.CFG_NO_RESIDENT))
    eng._reset_host_state()
    assert eng.detector_weights is None
    delta, beta, pr, pi = _data(64, 64, 1e-4, 'plane')[:4]
    eng.set_physics(E, PS, 1e-4)
    eng.set_probe(pr, pi)
    eng.set_object_batch(delta, beta)
    assert eng.loss_grad(B, meas) == l0
