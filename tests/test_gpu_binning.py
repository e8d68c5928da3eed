"""Slice binning (bdof_set_slice_binning, MultisliceEngine(slice_binning=b), the solvers' and entry points' keyword) on the device,
through the two engines that carry it, against the float64 reference of tests/reference_model.py.

Bounds: the ones tests/test_gpu_parity.py asserts for the identical unbinned cases — forward intensities relative L2 1e-5, wave
5e-6, loss relative 1e-5, gradients relative L2 2e-4 — because binning changes which table rows are multiplied into a step's
modulation, not the precision class of anything.  Objects and measurements are those of test_gpu_poisson.py::_case.  Every test
prints what it measured before it asserts."""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import bdof_oracle as orc

import poisson_reference as pref
import reference_model as ref_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, PS, MU = 5000., 1e-7, 2e6


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
def _reference(B, Y, X, S, fp, variant, probe, b, loss='lsq', seed=0, first_only=False):
    """Object, probe, measurement and the float64 reference of one case, computed once and shared by the engines that run it
    (read only).  first_only: the object is non-zero in the first voxel slice of every bin only."""
    rng = np.random.default_rng(seed)
    delta = rng.uniform(0, 2e-5, size=(B, Y, X, S))
    if first_only:
        keep = np.zeros(S)
        keep[::b] = 1
        delta = delta * keep
    beta = 0.1 * delta
    pr, pi = _probe(probe, Y, X, rng)
    ref, _ = ref_model.forward(delta, beta, pr, pi, E, PS, fp, variant, b)
    meas = np.abs(ref) * np.abs(1 + 0.05 * rng.normal(size=ref.shape))
    rl, rgd, rgb, _, _ = ref_model.loss_and_grad(delta, beta, pr, pi, E, PS, meas, fp, variant, b,
                                                 term=POISSON if loss == 'poisson' else ref_model.lsq)
    out = (delta, beta, pr, pi, meas, ref, rl, rgd, rgb)
    for a in out[:-3] + out[-2:]:
        a.setflags(write=False)
    return out


def _engine(engine_mod, engine, B, Y, X, S, fp, variant, case, b, loss='lsq'):
    delta, beta, pr, pi = case[:4]
    eng = engine_mod.MultisliceEngine(Y, X, S, B, with_grad=True, engine=engine, slice_binning=b)
    assert eng.slice_binning == b and eng.n_steps == S // b
    if loss == 'poisson':
        eng.set_loss('poisson', MU)
    eng.set_physics(E, PS, fp, variant=variant)
    eng.set_probe(pr, pi)
    eng.set_object_batch(delta, beta)
    return eng


def _bins_share_their_row(g, b):
    return all(np.array_equal(g[..., i * b + j], g[..., i * b]) for i in range(g.shape[-1] // b) for j in range(1, b))


def _run_and_check(engine_mod, tag, engine, B, Y, X, S, fp, variant, probe, b, loss='lsq', seed=0):
    case = _reference(B, Y, X, S, fp, variant, probe, b, loss, seed)
    delta, beta, pr, pi, meas, ref, rl, rgd, rgb = case
    eng = _engine(engine_mod, engine, B, Y, X, S, fp, variant, case, b, loss)
    wave = eng.forward(B)
    lossv = eng.loss_grad(B, meas)
    gd, gb = eng.grad_batch_to_host(B)
    e = (rel(np.abs(wave) ** 2, np.abs(ref) ** 2), rel(wave, ref), abs(lossv - rl) / abs(rl), rel(gd, rgd), rel(gb, rgb))
    print('binning', tag, engine, (Y, X, S), 'b', b, fp, probe, variant, loss, 'intensity / wave / loss / g_delta / g_beta rel err', e)
    assert e[0] <= 1e-5 and e[1] <= 5e-6, e
    assert e[2] <= 1e-5, e
    assert e[3] <= 2e-4 and e[4] <= 2e-4, e
    assert _bins_share_their_row(gd, b) and _bins_share_their_row(gb, b)          # bit for bit
    return eng


ENGINE_SHAPES = [('streaming', 64, 64), ('streaming', 64, 256), ('generic', 64, 64), ('generic', 96, 80)]


@pytest.mark.parametrize('engine,Y,X', ENGINE_SHAPES)
@pytest.mark.parametrize('b', [2, 3])
@pytest.mark.parametrize('fp', [None, 1e-4, 'inf'])
@pytest.mark.parametrize('probe', ['plane', 'random', 'gaussian'])
@pytest.mark.parametrize('variant', ['numpy_skip_last', 'tf_all'])
def test_binned_engine_vs_reference(engine_mod, engine, Y, X, b, fp, probe, variant):
    """'plane': the scalar carrier (cbar^b per step) with residual splitting, with 'inf' the float64 DC bin and the adjoint
    carrier; 'random': a scalar carrier under a structured probe; 'gaussian': the carrier-field stack of n_steps planes."""
    _run_and_check(engine_mod, 'parity', engine, 2, Y, X, 6, fp, variant, probe, b)


@pytest.mark.parametrize('n', [64, 128, 256, 512, 1024])
def test_every_fused_plan_once(engine_mod, n):
    _run_and_check(engine_mod, 'plans', 'streaming', 1, n, n, 4, 1e-4, 'numpy_skip_last', 'plane', 2)


@pytest.mark.parametrize('engine,Y,X', [('streaming', 64, 64), ('generic', 96, 80)])
@pytest.mark.parametrize('variant', ['numpy_skip_last', 'tf_all'])
def test_one_bin_holds_the_whole_depth(engine_mod, engine, Y, X, variant):
    """b = S: one step; under numpy_skip_last no propagation inside the object at all."""
    eng = _run_and_check(engine_mod, 'b = S', engine, 2, Y, X, 4, 1e-4, variant, 'random', 4)
    assert eng.n_steps == 1


@pytest.mark.parametrize('engine,Y,X', [('streaming', 64, 64), ('generic', 96, 80)])
@pytest.mark.parametrize('fp', [1e-4, 'inf'])
def test_binned_poisson_loss(engine_mod, engine, Y, X, fp):
    """The binned forward wave through poisson_reference.py's loss and seed, back through the binned adjoint."""
    _run_and_check(engine_mod, 'poisson', engine, 2, Y, X, 6, fp, 'numpy_skip_last', 'plane', 2, loss='poisson')


@pytest.mark.parametrize('engine,Y,X', [('streaming', 64, 256), ('generic', 96, 80)])
def test_binning_one_is_bit_identical_to_no_binning(engine_mod, engine, Y, X):
    """slice_binning=1, bdof_set_slice_binning(ctx, 1) called explicitly, and no keyword at all: the same bits."""
    B, S, fp, variant = 2, 6, 1e-4, 'numpy_skip_last'
    delta, beta, pr, pi, meas = _reference(B, Y, X, S, fp, variant, 'random', 1)[:5]
    got = []
    for how in ('none', 'keyword', 'call'):
        kw = dict(slice_binning=1) if how == 'keyword' else {}
        eng = engine_mod.MultisliceEngine(Y, X, S, B, with_grad=True, engine=engine, **kw)
        if how == 'call':
            eng.ctx.check(eng.lib.bdof_set_slice_binning(eng.h, 1))
        eng.set_physics(E, PS, fp, variant=variant)
        eng.set_probe(pr, pi)
        eng.set_object_batch(delta, beta)
        wave = eng.forward(B)
        loss = eng.loss_grad(B, meas)
        got.append((wave, loss) + tuple(eng.grad_batch_to_host(B)))
    for other in got[1:]:
        same = [np.array_equal(np.asarray(a), np.asarray(c)) for a, c in zip(got[0], other)]
        print('b = 1 against no binning', engine, (Y, X), 'wave / loss / g_delta / g_beta identical:', same)
        assert all(same)


@pytest.mark.parametrize('engine', ['streaming', 'generic'])
@pytest.mark.parametrize('b', [2, 3])
def test_pinned_to_the_unbinned_oracle(engine_mod, engine, b):
    """tf_all with the object in the first voxel slice of every bin only: the binned model IS the oracle's unbinned one
    (H(dz)^b = H(b dz), tests/test_binning_reference.py), so the device is compared with orc.multislice_loss_and_grad itself;
    the gradient at the slices that hold the object (the empty slices' unbinned gradient is another quantity)."""
    B, Y, X, S, fp = 2, 64, 64, 6, 1e-4
    case = _reference(B, Y, X, S, fp, 'tf_all', 'random', b, first_only=True)
    delta, beta, pr, pi, meas = case[:5]
    ref, _ = orc.multislice_propagate_batch_numpy(delta, beta, pr, pi, E, PS, fp, delta.shape, variant='tf_all')
    rl, rgd, rgb = orc.multislice_loss_and_grad(delta, beta, pr, pi, E, PS, meas, fp, 'tf_all')
    eng = _engine(engine_mod, engine, B, Y, X, S, fp, 'tf_all', case, b)
    wave = eng.forward(B)
    loss = eng.loss_grad(B, meas)
    gd, gb = eng.grad_batch_to_host(B)
    e = (rel(np.abs(wave) ** 2, np.abs(ref) ** 2), rel(wave, ref), abs(loss - rl) / abs(rl), rel(gd[..., ::b], rgd[..., ::b]),
         rel(gb[..., ::b], rgb[..., ::b]))
    print('binning against the unbinned oracle', engine, 'b', b, 'intensity / wave / loss / g_delta / g_beta rel err', e)
    assert e[0] <= 1e-5 and e[1] <= 5e-6 and e[2] <= 1e-5 and e[3] <= 2e-4 and e[4] <= 2e-4, e
    assert _bins_share_their_row(gd, b) and _bins_share_their_row(gb, b)


@pytest.mark.parametrize('b', [2, 4])
def test_fullfield_solver_rotation_table_path(engine_mod, b):
    """FullfieldSolver at 64^3: the binned loader looks its b source rows up in the rotation table; the gradient goes through the
    unchanged rotation adjoint over the full [B][S][NX][NY] rotated-frame gradient."""
    from beyond_dof_amd.solver import FullfieldSolver
    n, n_theta, mb, fp = 64, 8, 4, 1e-4
    rng = np.random.default_rng(0)
    od = rng.uniform(0, 2e-5, size=(n, n, n))
    ob = 0.1 * od
    coords = orc.rotation_lookup([n, n, n], n_theta)
    idx = np.sort(rng.choice(n_theta, mb, replace=False))
    one, zero = np.ones((n, n)), np.zeros((n, n))
    rot = np.stack([orc.apply_rotation(np.stack([od, ob], axis=3), coords[j]) for j in idx])
    ref, _ = ref_model.forward(rot[..., 0], rot[..., 1], one, zero, E, PS, fp, 'numpy_skip_last', b)
    prj = np.zeros((n_theta, n, n))
    prj[idx] = (np.abs(ref) * np.abs(1 + 0.05 * rng.normal(size=ref.shape))).astype(np.float32)
    s = FullfieldSolver(n, n, n, n_theta, mb, E, PS, free_prop_cm=fp, coord_ls=coords, slice_binning=b)
    assert s.eng.slice_binning == b
    s.set_volume(od, ob)
    s.set_measurements(prj)
    w = s.forward_angles(idx)
    loss = s.loss_and_grad(idx)
    gd, gb = s.gradient_to_host()
    rl, rgd, rgb, _ = ref_model.fullfield_loss_and_grad(od, ob, coords, idx, prj[idx], one, zero, E, PS, fp, b=b)
    e = (rel(np.abs(w) ** 2, np.abs(ref) ** 2), abs(loss - rl) / abs(rl), rel(gd, rgd), rel(gb, rgb))
    print('binning, full-field solver 64^3', 'b', b, 'intensity / loss / g_delta / g_beta rel err', e)
    assert e[0] <= 1e-5 and e[1] <= 1e-5 and e[2] <= 2e-4 and e[3] <= 2e-4, e


@pytest.mark.parametrize('psz,pos', [((64, 64), [(32, 32), (28, 36), (10, 32), (32, 60)]), ((36, 36), [(32, 32), (20, 40), (5, 62), (60, 3)])],
                         ids=['64-streaming', '36-generic'])
def test_ptycho_solver_window_path(engine_mod, psz, pos):
    """PtychoSolver, object 64^3, b = 2: windows cut by index math, two or more of the four hanging over the volume's edge in
    x and in y (rows and columns outside the volume are factors of 1 in a bin's product).  36 x 36 has an LDS-resident plan,
    which binning never takes: the generic engine runs it."""
    from beyond_dof_amd.solver import PtychoSolver
    n, n_theta, b, i_theta = 64, 3, 2, 1
    rng = np.random.default_rng(0)
    od = rng.uniform(0, 2e-5, size=(n, n, n))
    ob = 0.1 * od
    pos = np.array(pos)
    coords = orc.rotation_lookup([n, n, n], n_theta)
    prr, pii = orc.gaussian_probe(psz, 6., 6., 0.5)
    s = PtychoSolver((n, n, n), psz, pos, n_theta, len(pos), E, PS, prr, pii, coord_ls=coords, slice_binning=b)
    assert s.eng.slice_binning == b
    s.set_volume(od, ob)
    sel = np.arange(len(pos))
    w = s.forward(i_theta, sel)
    meas = np.abs(w).astype(np.float64) * np.abs(1 + 0.05 * rng.normal(size=w.shape))
    loss = s.loss_and_grad(i_theta, sel, meas)
    gd, gb = s.gradient_to_host()
    rl, rgd, rgb = ref_model.ptycho_loss_and_grad(od, ob, coords[i_theta], pos, pos[sel], meas, prr, pii, psz, E, PS, b=b)
    e = (abs(loss - rl) / abs(rl), rel(gd, rgd), rel(gb, rgb))
    print('binning, ptychography solver', psz, 'b', b, 'loss / g_delta / g_beta rel err', e)
    assert e[0] <= 1e-5 and e[1] <= 2e-4 and e[2] <= 2e-4, e


def test_refusals_on_the_device(engine_mod):
    """What does not carry binning says so instead of running the unbinned model."""
    M = engine_mod.MultisliceEngine
    for kw in (dict(engine='resident'), dict(recompute=True), dict(adjoint64=True)):
        with pytest.raises(ValueError, match='slice_binning'):
            M(64, 64, 6, 2, slice_binning=2, **kw)
    with pytest.raises(ValueError, match='slice_binning'):
        M(64, 64, 6, 2, slice_binning=4)
    eng = M(64, 64, 6, 2, slice_binning=2)
    eng.set_physics(E, PS, 1e-4)
    eng.set_probe(np.ones((64, 64)), np.zeros((64, 64)))
    with pytest.raises(ValueError, match='slice_binning'):
        eng.set_conv(E, PS)
    with pytest.raises(ValueError, match='slice_binning'):
        eng.enable_tf_f64()
    with pytest.raises(ValueError, match='slice_binning'):
        eng.enable_conv_f64()
    # ... and the library itself, under the Python checks
    lib, h = eng.lib, eng.h
    assert lib.bdof_set_slice_binning(h, 3) != 0 and b'bdof_configure' in lib.bdof_last_error(h)      # after bdof_set_physics
    assert lib.bdof_loss_grad_tf_f64(h, 2, None, None, None, None, 0.0) != 0 and b'slice binning' in lib.bdof_last_error(h)
    assert lib.bdof_forward_conv(h, 2, None, None, None, None) != 0 and b'slice binning' in lib.bdof_last_error(h)
    assert lib.bdof_forward_range(h, 2, None, None, None, 0, 2, None, None, 1) != 0 and b'slice binning' in lib.bdof_last_error(h)
    assert lib.bdof_adjoint_range(h, 2, None, None, None, 0, 2, None, None, None, None) != 0 and b'slice binning' in lib.bdof_last_error(h)
    assert lib.bdof_set_range_carrier(h, None, 0, 0, 0) != 0 and b'slice binning' in lib.bdof_last_error(h)
    from beyond_dof_amd import _lib
    for flag in (_lib.CFG_ALWAYS_RESIDENT, _lib.CFG_RECOMPUTE, _lib.CFG_ADJOINT64, _lib.CFG_NO_GROT):
        plain = M(64, 64, 6, 2)
        plain.ctx.check(plain.lib.bdof_configure(plain.h, 64, 64, 6, 2, _lib.CFG_GRAD | flag))
        assert plain.lib.bdof_set_slice_binning(plain.h, 2) != 0 and b'does not carry' in plain.lib.bdof_last_error(plain.h), flag
        assert plain.lib.bdof_set_slice_binning(plain.h, 1) == 0
    plain = M(64, 64, 6, 2)
    assert plain.lib.bdof_set_slice_binning(plain.h, 4) != 0 and plain.lib.bdof_set_slice_binning(plain.h, 0) != 0      # 6 % 4; < 1
    assert plain.lib.bdof_set_slice_binning(plain.h, 3) == 0
    plain.ctx.check(plain.lib.bdof_configure(plain.h, 64, 64, 6, 2, _lib.CFG_GRAD))                  # not sticky: back to 1
    assert plain.lib.bdof_set_range_carrier(plain.h, None, 0, 0, 0) == 0


def test_binned_reconstruction_converges_to_the_phantom():
    """examples/reconstruct_phantom.py's case reconstructed with slice_binning=2 from data simulated unbinned, held to the bounds
    of the unbinned run in test_gpu_convergence.py (which measures correlation 0.988, relative L2 error 0.16): the binned
    model's mismatch with the data is ~1e-4 of the contrast, four orders below the signal being fitted."""
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    import reconstruct_phantom as ex
    r = ex.run(128, 60, 100, 2e-8, 1e-3, quiet=True, slice_binning=2)
    print('full-field convergence with slice_binning=2 (unbinned: 0.988 / 0.16)', r)
    assert r['delta_corr'] >= 0.95 and r['delta_rel_l2'] <= 0.3, r
    assert 0.5 * r['phantom_peak'] <= r['delta_peak'] <= 1.5 * r['phantom_peak'], r
