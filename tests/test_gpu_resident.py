"""LDS-resident engine (csrc/bdof_resident.h): one workgroup carries a small square wavefield through all slices, forward,
loss and adjoint in a single launch.  Every supported size against the oracle; against the two other device engines on
sizes they share; with a rotation table and ptychography windows; batches larger than the grid."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import bdof_oracle as orc

SIZES = [32, 36, 48, 64, 72, 80, 96, 128]


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


@pytest.fixture(scope='module')
def engine_mod():
    import __graft_entry__ as entry
    entry.build()
    from beyond_dof_amd import engine
    return engine


def _inputs(n, B, S, fp, seed):
    rng = np.random.default_rng(seed)
    delta = rng.uniform(0, 2e-5, size=(B, n, n, S))
    beta = 0.1 * delta
    if fp == 'inf':
        pr, pi = orc.gaussian_probe((n, n), n / 8., n / 8., 0.5)
    else:
        pr, pi = 1 + 0.1 * rng.normal(size=(n, n)), 0.1 * rng.normal(size=(n, n))
    return rng, delta, beta, pr, pi


def _engine(engine_mod, n, B, S, fp, variant, delta, beta, pr, pi, engine):
    eng = engine_mod.MultisliceEngine(n, n, S, B, with_grad=True, engine=engine)
    eng.set_physics(5000., 1e-7, fp, variant=variant)
    eng.set_probe(pr, pi)
    eng.set_object_batch(delta, beta)
    return eng


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('fp,variant', [(None, 'numpy_skip_last'), (1e-4, 'tf_all'), ('inf', 'numpy_skip_last'), (None, 'tf_all'),
                                        (1e-4, 'numpy_skip_last')])
def test_resident_sizes_vs_oracle(engine_mod, n, fp, variant):
    B, S = 3, 5
    rng, delta, beta, pr, pi = _inputs(n, B, S, fp, n)
    eng = _engine(engine_mod, n, B, S, fp, variant, delta, beta, pr, pi, 'resident')
    wave = eng.forward(B)
    ref, _ = orc.multislice_propagate_batch_numpy(delta, beta, pr, pi, 5000., 1e-7, fp, delta.shape, variant=variant,
                                                  return_probe_array=False)
    assert rel(np.abs(wave) ** 2, np.abs(ref) ** 2) <= 1e-5
    assert rel(wave, ref) <= 5e-6
    meas = np.abs(ref) * (1 + 0.05 * rng.normal(size=ref.shape))
    loss = eng.loss_grad(B, meas)
    gd, gb = eng.grad_batch_to_host(B)
    rl, rgd, rgb = orc.multislice_loss_and_grad(delta, beta, pr, pi, 5000., 1e-7, meas, fp, variant)
    assert abs(loss - rl) <= 1e-5 * abs(rl)
    assert rel(gd, rgd) <= 2e-4 and rel(gb, rgb) <= 2e-4


@pytest.mark.parametrize('n,other', [(64, 'streaming'), (128, 'streaming'), (72, 'generic'), (96, 'generic')])
def test_resident_agrees_with_the_other_device_engines(engine_mod, n, other):
    """Three independent device implementations of the same operator: the waves agree to float32 round-off, more
    slices than in the oracle comparison (40), plane-wave probe (carrier splitting active)."""
    B, S, fp = 2, 40, 1e-4
    rng = np.random.default_rng(n)
    delta = rng.uniform(0, 2e-5, size=(B, n, n, S))
    beta = 0.1 * delta
    pr, pi = np.ones((n, n)), np.zeros((n, n))
    out = {}
    for engine in ('resident', other):
        eng = _engine(engine_mod, n, B, S, fp, 'numpy_skip_last', delta, beta, pr, pi, engine)
        wave = eng.forward(B)
        meas = np.ones((B, n, n))
        loss = eng.loss_grad(B, meas)
        out[engine] = (wave, loss) + tuple(eng.grad_batch_to_host(B))
    a, b = out['resident'], out[other]
    assert rel(a[0], b[0]) <= 2e-6
    assert abs(a[1] - b[1]) <= 1e-4 * abs(b[1])
    assert rel(a[2], b[2]) <= 2e-4 and rel(a[3], b[3]) <= 2e-4


@pytest.mark.parametrize('fp,variant', [(None, 'numpy_skip_last'), (1e-4, 'tf_all')])
def test_resident_plain_residual_form(engine_mod, fp, variant):
    """Scalar carrier with residual splitting switched off (what the solvers do for an optimisable probe): the detector block adds
    the carrier and takes |d| - m in float32 (seed_plain) — the one residual form the other resident tests do not reach, at the
    engine's smallest shape.  Bounds of test_resident_sizes_vs_oracle."""
    n, B, S = 32, 2, 2
    rng, delta, beta, _, _ = _inputs(n, B, S, fp, 11)
    pr, pi = np.ones((n, n)), np.zeros((n, n))          # a plane wave: a scalar carrier whatever the seed
    eng = engine_mod.MultisliceEngine(n, n, S, B, with_grad=True, engine='resident')
    eng.residual_split = False
    eng.set_physics(5000., 1e-7, fp, variant=variant)
    eng.set_probe(pr, pi)
    eng.set_object_batch(delta, beta)
    assert eng.meas_ref == 0.0 and not eng.probe_stack
    ref, _ = orc.multislice_propagate_batch_numpy(delta, beta, pr, pi, 5000., 1e-7, fp, delta.shape, variant=variant,
                                                  return_probe_array=False)
    meas = np.abs(ref) * (1 + 0.05 * rng.normal(size=ref.shape))
    loss = eng.loss_grad(B, meas)
    gd, gb = eng.grad_batch_to_host(B)
    rl, rgd, rgb = orc.multislice_loss_and_grad(delta, beta, pr, pi, 5000., 1e-7, meas, fp, variant)
    e = (abs(loss - rl) / abs(rl), rel(gd, rgd), rel(gb, rgb))
    print('resident plain form', fp, variant, 'loss / g_delta / g_beta rel err', e)
    assert e[0] <= 1e-5
    assert e[1] <= 2e-4 and e[2] <= 2e-4


def test_resident_batch_larger_than_the_grid_and_auto_selection(engine_mod):
    """More wavefields than workgroups the launch may have (the kernel loops), and the automatic choice: a 64^2 field has a
    fused plan, so small batches stream and large ones (>= CUs / 4 wavefields) go resident — same numbers either way."""
    n, S, fp = 64, 3, 'inf'
    B = 4500
    rng = np.random.default_rng(0)
    delta = rng.uniform(0, 2e-5, size=(B, n, n, S)).astype(np.float32)
    beta = 0.1 * delta
    pr, pi = orc.gaussian_probe((n, n), 8., 8., 0.5)
    eng = _engine(engine_mod, n, B, S, fp, 'numpy_skip_last', delta, beta, pr, pi, 'auto')
    wave = eng.forward(B)
    pick = [0, 1, 2047, 4159, 4160, 4161, 4499]
    ref, _ = orc.multislice_propagate_batch_numpy(delta[pick], beta[pick], pr, pi, 5000., 1e-7, fp, delta[pick].shape,
                                                  return_probe_array=False)
    assert rel(wave[pick], ref) <= 5e-6
    meas = np.abs(wave) * (1 + 0.05 * rng.normal(size=wave.shape))
    loss = eng.loss_grad(B, meas)
    gd, gb = eng.grad_batch_to_host(B)
    rl, rgd, rgb = orc.multislice_loss_and_grad(delta[pick], beta[pick], pr, pi, 5000., 1e-7, meas[pick], fp)
    # the oracle's loss / gradient are means over ITS batch: rescale to the full batch
    assert rel(gd[pick] * B / len(pick), rgd) <= 2e-4
    small = _engine(engine_mod, n, 2, S, fp, 'numpy_skip_last', delta[:2], beta[:2], pr, pi, 'auto')
    assert rel(small.forward(2), wave[:2]) <= 2e-6
    assert np.isfinite(loss) and loss > 0


@pytest.mark.parametrize('n', [64, 72])
@pytest.mark.parametrize('S', [1, 2])
@pytest.mark.parametrize('fp,variant', [(None, 'numpy_skip_last'), (1e-4, 'tf_all'), ('inf', 'tf_all')])
def test_resident_one_and_two_slices(engine_mod, n, S, fp, variant):
    """Fewer slices than the 3-slot row ring and the load pipeline look ahead (both the fused-epilogue and the plain form)."""
    B = 2
    rng, delta, beta, pr, pi = _inputs(n, B, S, fp, 7 * n + S)
    eng = _engine(engine_mod, n, B, S, fp, variant, delta, beta, pr, pi, 'resident')
    wave = eng.forward(B)
    ref, _ = orc.multislice_propagate_batch_numpy(delta, beta, pr, pi, 5000., 1e-7, fp, delta.shape, variant=variant,
                                                  return_probe_array=False)
    assert rel(wave, ref) <= 5e-6
    meas = np.abs(ref) * (1 + 0.05 * rng.normal(size=ref.shape))
    loss = eng.loss_grad(B, meas)
    gd, gb = eng.grad_batch_to_host(B)
    rl, rgd, rgb = orc.multislice_loss_and_grad(delta, beta, pr, pi, 5000., 1e-7, meas, fp, variant)
    assert abs(loss - rl) <= 1e-5 * abs(rl)
    # one slice and no detector step: |d| does not depend on delta at all (pure phase), the exact delta-gradient is 0 —
    # compare against the scale of the whole gradient
    scale = np.sqrt(np.linalg.norm(rgd) ** 2 + np.linalg.norm(rgb) ** 2)
    assert np.linalg.norm(gd - rgd) <= 2e-4 * scale and np.linalg.norm(gb - rgb) <= 2e-4 * scale


@pytest.mark.parametrize('n', [64, 72, 96])
def test_resident_is_deterministic(engine_mod, n):
    """Same inputs, three runs on a chip-filling batch: identical bits (no atomics; the wave-local passes of the 72^2
    instance rely on LDS ordering inside a wave, the others on workgroup barriers — a race would show up here)."""
    B, S = 300, 6
    rng = np.random.default_rng(n)
    delta = rng.uniform(0, 2e-5, size=(B, n, n, S)).astype(np.float32)
    beta = 0.1 * delta
    pr, pi = orc.gaussian_probe((n, n), n / 8., n / 8., 0.5)
    eng = _engine(engine_mod, n, B, S, 'inf', 'numpy_skip_last', delta, beta, pr, pi, 'resident')
    meas = rng.uniform(0.5, 1.5, size=(B, n, n)).astype(np.float32) * n
    runs = []
    for _ in range(3):
        wave = eng.forward(B)
        loss = eng.loss_grad(B, meas)
        gd, gb = eng.grad_batch_to_host(B)
        runs.append((wave, loss, gd, gb))
    for r in runs[1:]:
        assert np.array_equal(r[0], runs[0][0]) and r[1] == runs[0][1]
        assert np.array_equal(r[2], runs[0][2]) and np.array_equal(r[3], runs[0][3])
    pick = [0, 150, 299]
    ref, _ = orc.multislice_propagate_batch_numpy(delta[pick], beta[pick], pr, pi, 5000., 1e-7, 'inf', delta[pick].shape,
                                                  return_probe_array=False)
    assert rel(runs[0][0][pick], ref) <= 5e-6


def test_cfg5_full_size_properties(engine_mod):
    """cfg5 at its full size (400 probe positions of 72 x 72, 256 slices) is beyond what the float64 oracle finishes in
    seconds: size-independent properties instead.  (1) A pure-phase object (beta = 0) conserves the energy of the wave
    through 256 transfer-function steps; (2) Parseval between the exit wave and the un-normalised far field; (3) the model
    is linear in the probe: doubling it doubles every wave exactly (power of two); (4) a sample of positions against the
    oracle at reduced depth is covered by the other tests — here the full-depth waves of two engines are compared on a
    subset (resident vs rocFFT, different FFT code)."""
    n, S, B = 72, 256, 400
    rng = np.random.default_rng(5)
    delta = (rng.random((B, n, n, S), dtype=np.float32) * np.float32(2e-6))
    beta = np.zeros_like(delta)
    pr, pi = orc.gaussian_probe((n, n), 6., 6., 0.5)
    e0 = float(np.sum(pr ** 2 + pi ** 2))
    eng = _engine(engine_mod, n, B, S, None, 'numpy_skip_last', delta, beta, pr, pi, 'resident')
    exit_wave = eng.forward(B)
    energy = np.sum(np.abs(exit_wave.astype(np.complex128)) ** 2, axis=(1, 2))
    # plain float32 transform chains drift in energy systematically (rocFFT: -1.25e-7 per slice at 72^2, 3.3e-5 after 255
    # steps, tools/gpu_check_energy.py); here the irrational butterfly constants are hi + lo pairs and the probe's own
    # free-space propagation is carried as a float64-computed field (bdof_set_probe_field), so only the scattered wave runs
    # through float32: what is left with an object in the beam is a few 1e-7 on average over the 400 wavefields, below
    # 4e-6 for each of them at full depth.
    drift = energy / e0 - 1
    assert np.max(np.abs(drift)) <= 4e-6 and abs(np.mean(drift)) <= 1.5e-6
    far = _engine(engine_mod, n, B, S, 'inf', 'numpy_skip_last', delta, beta, pr, pi, 'resident')
    d = far.forward(B)
    efar = np.sum(np.abs(d.astype(np.complex128)) ** 2, axis=(1, 2))
    assert np.max(np.abs(efar / (n * n * energy) - 1)) <= 2e-6
    eng2 = _engine(engine_mod, n, B, S, None, 'numpy_skip_last', delta, beta, 2 * pr, 2 * pi, 'resident')
    assert np.array_equal(eng2.forward(B), 2 * exit_wave)
    sub = slice(0, 8)
    gen = _engine(engine_mod, n, 8, S, None, 'numpy_skip_last', delta[sub], beta[sub], pr, pi, 'generic')
    assert rel(gen.forward(8), exit_wave[sub]) <= 1e-6            # both ride on the carrier field of the probe


@pytest.mark.parametrize('engine', ['resident', 'generic'])
def test_cfg5_full_depth_vs_oracle(engine_mod, engine):
    """cfg5's probe size and FULL depth (72 x 72, 256 slices, gaussian probe, far field) against the float64 oracle on a few
    wavefields.  A float32 transform chain on the whole wave is limited by its own arithmetic at this depth: 2.6e-5 in
    intensity on rocFFT even with the energy drift calibrated out (3.5e-5 without; numpy's float32 FFT with an exact
    transfer function: 1.7e-5; BDOF_NO_PROBE_STACK=1 python tools/gpu_check_depth.py).  The resident and the rocFFT engine
    carry the probe's free-space propagation as a float64-computed carrier FIELD (bdof_set_probe_stack) and run only the
    scattered wave through float32: 1.4e-7 in intensity, gradients to 2e-5 — the localised-probe analogue of the
    plane-wave carrier."""
    n, S, B = 72, 256, 3
    rng = np.random.default_rng(55)
    delta = rng.uniform(0, 2e-6, size=(B, n, n, S))
    beta = 0.1 * delta
    pr, pi = orc.gaussian_probe((n, n), 6., 6., 0.5)
    eng = _engine(engine_mod, n, B, S, 'inf', 'numpy_skip_last', delta, beta, pr, pi, engine)
    assert eng.probe_stack
    tol = dict(intensity=1e-6, energy=2e-7, loss=5e-6, grad=1e-4)
    wave = eng.forward(B)
    ref, _ = orc.multislice_propagate_batch_numpy(delta, beta, pr, pi, 5000., 1e-7, 'inf', delta.shape, return_probe_array=False)
    assert rel(np.abs(wave) ** 2, np.abs(ref) ** 2) <= tol['intensity']
    assert abs(np.sum(np.abs(wave.astype(np.complex128)) ** 2) / np.sum(np.abs(ref) ** 2) - 1) <= tol['energy']
    meas = np.abs(ref) * (1 + 0.05 * rng.normal(size=ref.shape))
    loss = eng.loss_grad(B, meas)
    rl, rgd, rgb = orc.multislice_loss_and_grad(delta, beta, pr, pi, 5000., 1e-7, meas, 'inf')
    gd, gb = eng.grad_batch_to_host(B)
    assert abs(loss - rl) <= tol['loss'] * abs(rl)
    assert rel(gd, rgd) <= tol['grad'] and rel(gb, rgb) <= tol['grad']


@pytest.mark.parametrize('fp,variant', [(None, 'numpy_skip_last'), (None, 'tf_all'), (1e-4, 'numpy_skip_last'), (1e-4, 'tf_all'),
                                        ('inf', 'tf_all')])
def test_probe_stack_all_detectors(engine_mod, fp, variant):
    """The carrier field through every detector mode / variant (64 slices), with and without it: same answer as the oracle,
    at least ten times closer with it."""
    n, S, B = 72, 64, 2
    rng = np.random.default_rng(8)
    delta = rng.uniform(0, 2e-6, size=(B, n, n, S))
    beta = 0.1 * delta
    pr, pi = orc.gaussian_probe((n, n), 6., 6., 0.5)
    ref, _ = orc.multislice_propagate_batch_numpy(delta, beta, pr, pi, 5000., 1e-7, fp, delta.shape, variant=variant,
                                                  return_probe_array=False)
    meas = np.abs(ref) * (1 + 0.05 * rng.normal(size=ref.shape))
    rl, rgd, rgb = orc.multislice_loss_and_grad(delta, beta, pr, pi, 5000., 1e-7, meas, fp, variant)
    errs = {}
    for stack in (True, False):
        if not stack:
            os.environ['BDOF_NO_PROBE_STACK'] = '1'
        try:
            eng = _engine(engine_mod, n, B, S, fp, variant, delta, beta, pr, pi, 'auto')
        finally:
            os.environ.pop('BDOF_NO_PROBE_STACK', None)
        assert eng.probe_stack == stack
        wave = eng.forward(B)
        loss = eng.loss_grad(B, meas)
        gd, gb = eng.grad_batch_to_host(B)
        errs[stack] = (rel(wave, ref), abs(loss - rl) / abs(rl), rel(gd, rgd), rel(gb, rgb))
    assert errs[True][0] <= 2e-7 and errs[True][1] <= 2e-6 and errs[True][2] <= 5e-5 and errs[True][3] <= 5e-5
    assert errs[False][0] <= 1e-5
    assert errs[True][0] * 10 <= errs[False][0]


def test_physics_change_refreshes_the_probe_carrier(engine_mod):
    """The carrier field belongs to (probe, physics): changing the detector after set_probe must rebuild it."""
    n, S, B = 72, 24, 2
    rng, delta, beta, pr, pi = _inputs(n, B, S, 'inf', 3)
    eng = engine_mod.MultisliceEngine(n, n, S, B, with_grad=False)
    eng.set_physics(5000., 1e-7, None)
    eng.set_probe(pr, pi)
    eng.set_object_batch(delta, beta)
    for fp in (1e-4, 'inf', None):
        eng.set_physics(5000., 1e-7, fp)
        ref, _ = orc.multislice_propagate_batch_numpy(delta, beta, pr, pi, 5000., 1e-7, fp, delta.shape, return_probe_array=False)
        assert eng.probe_stack and rel(eng.forward(B), ref) <= 2e-7
