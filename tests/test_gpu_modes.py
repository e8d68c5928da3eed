"""Probe modes (bdof_set_probe_modes, include/bdof.h) at engine level against the float64 reference tests/modes_reference.py:
loss, volume gradient and mode gradients on the resident and the generic engine, the exact properties of the modes path (repeat,
zero mode, removal) and every refusal.

Data: B = 3 windows, S = 6, objects delta ~ U(0, 2e-5), beta = 0.1 delta (tests/test_gpu_probe.py; rounded to float32, which is
what the device holds), Gaussian modes from modes.initial_modes with power = 0.3 — no mode is negligible — and amplitudes
m = a_ref |1 + 0.05 N|.  Bounds are the project's own for this data: loss 2e-5 relative, volume and probe gradients 2e-4 relative
L2 (tests/test_gpu_probe.py, tests/test_gpu_poisson.py); under the wide amplitudes a_ref U(0, 2) of reference_model.measurement_wide
the volume gradient 2e-5 (tests/gradient_cases.py).  Every test prints what it measured before it asserts."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import modes_reference as mref
import poisson_reference as pref
import reference_model as ref_model
import weights_reference as wref
from reference_model import rel

E, PS, MU = 5000., 1e-7, 2e6
B, S = 3, 6
LOSS_BOUND, GRAD_BOUND, WIDE_BOUND = 2e-5, 2e-4, 2e-5
ERR_ARG, ERR_STATE = -1, -2


def _modes(Y, X, M, power=0.3):
    from beyond_dof_amd import modes, util
    pr, pi = util.gaussian_probe((Y, X), Y / 6., Y / 6., 0.5)
    return modes.initial_modes(pr + 1j * pi, M, power).astype(np.complex64)        # (what the engine and the reference both start from)


def _weights(Y, X):
    return wref.random_weights((Y, X), np.random.default_rng([Y, X, 3]))          # no symmetry: an index-order mix-up shows


def _term(kind, w):
    if w is not None:
        return ref_model.data_term(wref.weighted_loss, wref.weighted_seed, w, kind, MU)
    if kind == 'poisson':
        return ref_model.data_term(pref.poisson_loss, pref.poisson_seed, MU)
    return ref_model.lsq


@functools.lru_cache(maxsize=None)
def _problem(Y, X, M, fp, variant='numpy_skip_last', kind='lsq', weighted=False, wide=False):
    """The data of a case and its float64 reference, computed once: dict(delta, beta, modes, meas, w, loss, gd, gb, gm, d)."""
    rng = np.random.default_rng([Y, X, S])
    delta = rng.uniform(0, 2e-5, size=(B, Y, X, S)).astype(np.float32).astype(np.float64)
    beta = (0.1 * delta).astype(np.float32).astype(np.float64)
    modes = _modes(Y, X, M)
    a = mref.amplitude(mref.forward(delta, beta, modes, E, PS, fp, variant))
    meas = ref_model.measurement_wide(a) if wide else a * np.abs(1 + 0.05 * rng.normal(size=a.shape))
    meas = meas.astype(np.float32)
    w = _weights(Y, X) if weighted else None
    loss, gd, gb, gm, d = mref.loss_and_grad(delta, beta, modes, E, PS, meas.astype(np.float64), fp, variant, term=_term(kind, w))
    for v in (delta, beta, modes, meas, gd, gb, gm, d):
        v.setflags(write=False)
    return dict(delta=delta, beta=beta, modes=modes, meas=meas, w=w, loss=loss, gd=gd, gb=gb, gm=gm, d=d)


def _engine(engine, Y, X, fp, variant='numpy_skip_last', kind='lsq', w=None, batch_max=B * 3, **kw):
    import __graft_entry__ as entry
    entry.build()
    from beyond_dof_amd.engine import MultisliceEngine
    eng = MultisliceEngine(Y, X, S, batch_max, with_grad=True, engine=engine, **kw)
    eng.set_physics(E, PS, fp, variant=variant)
    if kind == 'poisson':
        eng.set_loss('poisson', MU)
    if w is not None:
        eng.set_detector_weights(w)
    return eng


def _grot_bits(eng):
    """the rotated-frame gradient [B][S][NX][NY] as the device holds it"""
    out = np.empty((B, S, eng.nx, eng.ny, 2), dtype=np.float32)
    eng.ctx.check(eng.lib.bdof_memcpy_d2h(eng.h, out.ctypes.data, eng.lib.bdof_grot(eng.h), out.nbytes))
    return out


def _run(engine, Y, X, p, fp, variant='numpy_skip_last', kind='lsq', modes=None, eng=None):
    """(loss, g_delta, g_beta, mode gradients, engine) of one loss_grad under the problem's modes (or `modes`)."""
    modes = p['modes'] if modes is None else modes
    eng = eng or _engine(engine, Y, X, fp, variant, kind, p['w'])
    eng.set_probe_modes(modes.real, modes.imag)
    eng.enable_probe_grad(True)
    eng.set_object_batch(p['delta'], p['beta'])
    loss = eng.loss_grad(B, p['meas'])
    gd, gb = eng.grad_batch_to_host(B)
    return loss, gd, gb, eng.probe_grad(), eng


def _errors(p, loss, gd, gb, gm):
    return abs(loss - p['loss']) / abs(p['loss']), rel(gd, p['gd']), rel(gb, p['gb']), rel(gm, p['gm'])


# resident plans: 32^2, 36^2 (its adjoint reads the tape in another thread mapping than the forward sweep wrote it) and 72^2 (the
# plan with the e < N N guard: ptychography's size); generic: 36^2 and the non-square 40 x 24
SIZES = [('resident', 32, 32), ('resident', 36, 36), ('resident', 72, 72), ('generic', 36, 36), ('generic', 40, 24)]
PARITY = [(e, y, x, 2, 'inf') for e, y, x in SIZES if (y, x) != (36, 36)] + \
         [(e, 36, 36, M, fp) for e in ('resident', 'generic') for M in (1, 2, 3) for fp in (None, 1e-4, 'inf')]


@pytest.mark.parametrize('engine,Y,X,M,fp', PARITY)
def test_loss_and_gradients_against_the_reference(engine, Y, X, M, fp):
    p = _problem(Y, X, M, fp)
    loss, gd, gb, gm, eng = _run(engine, Y, X, p, fp)
    errs = _errors(p, loss, gd, gb, gm)
    print('modes parity (loss, g_delta, g_beta, g_modes)', engine, (Y, X), 'M', M, fp, errs)
    assert gm.shape == (M, Y, X)
    assert errs[0] <= LOSS_BOUND and max(errs[1:]) <= GRAD_BOUND, errs
    wave = eng.forward(B)
    assert wave.shape == (M, B, Y, X)
    e_int = rel(np.sum(np.abs(wave) ** 2, axis=0), np.sum(np.abs(p['d']) ** 2, axis=0))
    print('   forward: summed intensity rel err', e_int, 'waves', rel(wave, p['d']))
    assert e_int <= 1e-5                                           # (the bound smoke() holds a forward intensity to)


@pytest.mark.parametrize('engine,Y,X', [('resident', 36, 36), ('generic', 36, 36), ('generic', 40, 24)])
@pytest.mark.parametrize('kind', ['lsq', 'poisson'])
@pytest.mark.parametrize('weighted', [False, True])
def test_both_data_terms_with_and_without_weights(engine, Y, X, kind, weighted):
    p = _problem(Y, X, 2, 'inf', kind=kind, weighted=weighted)
    errs = _errors(p, *_run(engine, Y, X, p, 'inf', kind=kind)[:4])
    print('modes parity, data terms (loss, g_delta, g_beta, g_modes)', engine, (Y, X), kind, 'weighted' if weighted else 'unweighted', errs)
    assert errs[0] <= LOSS_BOUND and max(errs[1:]) <= GRAD_BOUND, errs


@pytest.mark.parametrize('engine', ['resident', 'generic'])
def test_tf_all_variant(engine):
    p = _problem(36, 36, 2, 1e-4, variant='tf_all')
    errs = _errors(p, *_run(engine, 36, 36, p, 1e-4, variant='tf_all')[:4])
    print('modes parity, tf_all (loss, g_delta, g_beta, g_modes)', engine, errs)
    assert errs[0] <= LOSS_BOUND and max(errs[1:]) <= GRAD_BOUND, errs


def test_resident_and_generic_engines_agree():
    p = _problem(36, 36, 2, 'inf')
    lr, gdr, gbr, gmr, _ = _run('resident', 36, 36, p, 'inf')
    lg, gdg, gbg, gmg, _ = _run('generic', 36, 36, p, 'inf')
    errs = (abs(lr - lg) / abs(lg), rel(gdr, gdg), rel(gbr, gbg), rel(gmr, gmg))
    print('resident against generic, 36^2, M = 2 (loss, g_delta, g_beta, g_modes)', errs)
    assert errs[0] <= LOSS_BOUND and max(errs[1:]) <= GRAD_BOUND, errs


@pytest.mark.parametrize('engine', ['resident', 'generic'])
def test_wide_amplitudes_hold_the_tight_gradient_bound(engine):
    """amplitudes a_ref U(0, 2): no cancellation in the seed, so the volume gradient is held to the 2e-5 of tests/gradient_cases.py"""
    p = _problem(36, 36, 2, 'inf', wide=True)
    errs = _errors(p, *_run(engine, 36, 36, p, 'inf')[:4])
    print('modes parity, wide amplitudes (loss, g_delta, g_beta, g_modes)', engine, errs)
    assert errs[0] <= LOSS_BOUND and max(errs[1:3]) <= WIDE_BOUND and errs[3] <= GRAD_BOUND, errs


@pytest.mark.parametrize('engine', ['resident', 'generic'])
def test_the_same_call_twice_gives_the_same_bits(engine):
    p = _problem(36, 36, 2, 'inf')
    loss, _, _, gm, eng = _run(engine, 36, 36, p, 'inf')
    grot = _grot_bits(eng)
    loss2 = eng.loss_grad(B, p['meas'])
    grot2, gm2 = _grot_bits(eng), eng.probe_grad()
    same = (loss == loss2, np.array_equal(grot.view(np.uint32), grot2.view(np.uint32)), np.array_equal(gm.view(np.uint32), gm2.view(np.uint32)))
    print('repeat: loss, grot, mode gradients identical', engine, same)
    assert all(same)


@pytest.mark.parametrize('engine', ['resident', 'generic'])
def test_a_zero_mode_gives_the_bits_of_one_mode(engine):
    """On the modes path M = 2 with mode 1 identically zero: the loss, bdof_grot and the gradient of mode 0 have the bits of M = 1 —
    the sign of a zero included: k_modes_sum_rows does not add a term that is zero — and mode 1's own gradient is exactly zero."""
    p1 = _problem(36, 36, 1, 'inf')
    loss1, _, _, gm1, eng = _run(engine, 36, 36, p1, 'inf')
    grot1 = _grot_bits(eng)
    two = np.concatenate([p1['modes'], np.zeros_like(p1['modes'])])
    loss2, _, _, gm2, eng = _run(engine, 36, 36, p1, 'inf', modes=two, eng=eng)
    grot2 = _grot_bits(eng)
    same = (loss1 == loss2, np.array_equal(grot1.view(np.uint32), grot2.view(np.uint32)),
            np.array_equal(gm1[0].view(np.uint32), gm2[0].view(np.uint32)), bool(np.all(gm2[1] == 0)))
    print('zero mode: loss, grot, gradient of mode 0 equal, gradient of mode 1 zero', engine, same)
    assert all(same)


@pytest.mark.parametrize('engine', ['resident', 'generic'])
def test_a_unitary_mix_on_the_device(engine):
    p = _problem(36, 36, 3, 'inf')
    loss, gd, gb, _, eng = _run(engine, 36, 36, p, 'inf')
    rng = np.random.default_rng(11)
    u, _ = np.linalg.qr(rng.normal(size=(3, 3)) + 1j * rng.normal(size=(3, 3)))
    mixed = np.einsum('mn,nyx->myx', u, p['modes'].astype(np.complex128))
    loss_u, gd_u, gb_u, _, _ = _run(engine, 36, 36, p, 'inf', modes=mixed, eng=eng)
    errs = (abs(loss_u - loss) / abs(loss), rel(gd_u, gd), rel(gb_u, gb))
    print('unitary mix on the device (loss, g_delta, g_beta against the unmixed run)', engine, errs)
    assert errs[0] <= LOSS_BOUND and max(errs[1:]) <= GRAD_BOUND, errs


@pytest.mark.parametrize('engine', ['resident', 'generic'])
@pytest.mark.parametrize('fp', [None, 'inf'])
def test_one_mode_against_the_plain_path(engine, fp):
    """The modes path at M = 1 and the single-probe path (set_probe: bdof_set_probe_field) are two computations of one model: both
    are held to the float64 reference; their mutual difference is printed (MEASUREMENTS.md records it), not asserted tighter."""
    p = _problem(36, 36, 1, fp)
    loss_m, gd_m, gb_m, gm_m, eng = _run(engine, 36, 36, p, fp)
    eng.set_probe_modes(None, None)
    eng.set_probe(p['modes'][0].real, p['modes'][0].imag)
    loss_p = eng.loss_grad(B, p['meas'])
    gd_p, gb_p = eng.grad_batch_to_host(B)
    gp_p = eng.probe_grad()
    assert gp_p.shape == (36, 36)
    e_m, e_p = _errors(p, loss_m, gd_m, gb_m, gm_m), _errors(p, loss_p, gd_p, gb_p, gp_p[None])
    mutual = (abs(loss_m - loss_p) / abs(loss_p), rel(gd_m, gd_p), rel(gb_m, gb_p), rel(gm_m[0], gp_p))
    print('M = 1', engine, fp, 'modes path against the reference', e_m, '\n   plain path against the reference', e_p, '\n   modes path against plain path', mutual)
    for e in (e_m, e_p):
        assert e[0] <= LOSS_BOUND and max(e[1:]) <= GRAD_BOUND, e


def _plain_step(eng, p):
    eng.set_probe(p['modes'][0].real, p['modes'][0].imag)
    eng.set_object_batch(p['delta'], p['beta'])
    loss = eng.loss_grad(B, p['meas'])
    return loss, _grot_bits(eng)


@pytest.mark.parametrize('engine', ['resident', 'generic'])
def test_removing_the_modes_gives_back_the_plain_bits(engine):
    """bdof_set_probe_modes(ctx, 0, NULL, ...) goes back to the probe bdof_set_probe* last set (the library call alone: loss_grad
    asks the engine's host state nothing); MultisliceEngine.set_probe_modes(None, None), which also hands that probe over again,
    gives the same bits once more."""
    p = _problem(36, 36, 2, 'inf')
    eng = _engine(engine, 36, 36, 'inf')
    loss0, grot0 = _plain_step(eng, p)
    _run(engine, 36, 36, p, 'inf', eng=eng)
    eng.ctx.check(eng.lib.bdof_set_probe_modes(eng.h, 0, None, None, None))
    loss1 = eng.loss_grad(B, p['meas'])
    grot1 = _grot_bits(eng)
    eng.set_probe_modes(None, None)
    assert eng.n_modes == 0
    loss2 = eng.loss_grad(B, p['meas'])
    grot2 = _grot_bits(eng)
    same = (loss0 == loss1 == loss2, np.array_equal(grot0.view(np.uint32), grot1.view(np.uint32)), np.array_equal(grot0.view(np.uint32), grot2.view(np.uint32)))
    print('plain step before the modes, after bdof_set_probe_modes(0) and after set_probe_modes(None, None): loss, grot identical', engine, same)
    assert all(same)


def _set_modes_rc(eng, modes):
    """bdof_set_probe_modes called as MultisliceEngine.set_probe_modes calls it, returning (code, bdof_last_error)"""
    o = eng.optics
    hT = o.table(eng._step_nm(), tiled=True, fold=False, transpose=True, dtype=np.complex128)
    hdT = eng._detector_table(np.complex128, fold=False, transpose=True, tiled=True)
    pm = np.ascontiguousarray(modes.transpose(0, 2, 1).astype(np.complex128))
    rc = eng.lib.bdof_set_probe_modes(eng.h, modes.shape[0], pm.ctypes.data, hT.ctypes.data, None if hdT is None else hdT.ctypes.data)
    return rc, (eng.lib.bdof_last_error(eng.h) or b'').decode()


REFUSED_CTX = [('a streaming-only ctx', 64, dict(engine='streaming')), ('BDOF_CFG_RECOMPUTE', 64, dict(engine='auto', recompute=True)),
               ('BDOF_CFG_ADJOINT64', 36, dict(engine='auto', adjoint64=True)), ('slice binning', 36, dict(engine='generic', slice_binning=2))]


@pytest.mark.parametrize('what,N,kw', REFUSED_CTX, ids=[r[0] for r in REFUSED_CTX])
def test_a_ctx_that_does_not_carry_the_modes_refuses_them(what, N, kw):
    p = _problem(N, N, 2, 'inf')
    engine = kw.pop('engine') if 'engine' in kw else 'auto'
    eng = _engine(engine, N, N, 'inf', **kw)
    kw['engine'] = engine
    before = _plain_step(eng, p)
    rc, msg = _set_modes_rc(eng, p['modes'])
    print(what, '->', rc, msg)
    assert rc == ERR_STATE and 'probe modes' in msg
    after = _plain_step(eng, p)                                    # the ctx still runs a plain step: the one it ran before
    assert np.isfinite(after[0]) and after[0] == before[0] and np.array_equal(after[1], before[1])


def test_what_does_not_carry_the_modes_refuses_under_them():
    """With modes in force: detector planes, the real-space propagator, the float64 twin, the single-probe gradient and a batch of
    more than Bmax wavefields each give the documented code and name the probe modes; the ctx then still runs a plain step."""
    p = _problem(36, 36, 2, 1e-4)
    eng = _engine('generic', 36, 36, 1e-4, batch_max=2 * B)
    _run('generic', 36, 36, p, 1e-4, eng=eng)
    lib, h = eng.lib, eng.h

    def err():
        return (lib.bdof_last_error(h) or b'').decode()
    tables = np.ones((2, 36, 36), dtype=np.complex64)
    dcs = np.ones(2, dtype=np.complex128)
    ks = np.ones(5, dtype=np.complex64)
    from beyond_dof_amd._lib import DeviceBuffer
    meas = DeviceBuffer.from_host(eng.ctx, eng.meas_layout(p['meas']))
    gprobe = DeviceBuffer.zeros(eng.ctx, (36, 36), np.complex64)
    calls = [('bdof_set_detector_planes', ERR_STATE, lambda: lib.bdof_set_detector_planes(h, 2, tables.ctypes.data, dcs.ctypes.data)),
             ('bdof_set_conv', ERR_STATE, lambda: lib.bdof_set_conv(h, ks.ctypes.data, ks.ctypes.data, 5, 1., 0., 1., 0., 1.)),
             ('bdof_loss_grad_tf_f64', ERR_STATE, lambda: lib.bdof_loss_grad_tf_f64(h, B, None, None, None, meas.ptr, 0.)),
             ('bdof_probe_grad', ERR_STATE, lambda: lib.bdof_probe_grad(h, gprobe.ptr, 0)),
             ('bdof_forward(keep_tape)', ERR_STATE, lambda: lib.bdof_forward(h, B, None, None, None, None, 1)),
             ('B M > Bmax', ERR_ARG, lambda: lib.bdof_loss_grad(h, B + 1, None, None, None, meas.ptr, None))]
    for name, code, call in calls:
        rc = call()
        print(name, '->', rc, err())
        assert rc == code and 'probe modes' in err(), (name, rc, err())
    # the modes are still in force and unharmed
    loss = eng.loss_grad(B, p['meas'])
    assert abs(loss - p['loss']) <= LOSS_BOUND * abs(p['loss'])
    eng.set_probe_modes(None, None)
    loss, _ = _plain_step(eng, p)
    assert np.isfinite(loss)
    # ... and the other way round: detector planes first, then the modes
    eng2 = _engine('generic', 36, 36, [1e-4, 2e-4])
    rc, msg = _set_modes_rc(eng2, p['modes'])
    print('modes under detector planes ->', rc, msg)
    assert rc == ERR_STATE and 'probe modes' in msg
    rc = lib.bdof_set_probe_modes(h, 9, tables.ctypes.data, tables.ctypes.data, tables.ctypes.data)
    print('M = 9 ->', rc, err())
    assert rc == ERR_ARG and 'probe modes' in err()


def test_engine_keywords_are_refused_on_the_host():
    p = _problem(36, 36, 2, 'inf')
    eng = _engine('generic', 36, 36, 'inf')
    with pytest.raises(ValueError, match='probe modes'):
        eng.set_probe_modes(p['modes'].real[:, :20], p['modes'].imag[:, :20])
    with pytest.raises(ValueError, match='n_probe_modes'):
        eng.set_probe_modes(np.zeros((9, 36, 36)), np.zeros((9, 36, 36)))
    with pytest.raises(ValueError, match='probe modes'):
        eng.set_probe_modes(p['modes'].real[0], p['modes'].imag[0])
