"""The cases of the tight gradient check — numpy, test side, shared by tests/test_gradient_conditioning.py (no GPU: what a plain
complex64 restatement reaches at every case, what the bound sees) and tests/test_gpu_gradient_tight.py (the device), so that the
two cannot drift apart.

Every case is one loss + gradient of the transfer-function model against the float64 reference of tests/reference_model.py with
  - the object as the device holds it (float32 delta, beta; the reference at modulation_reference.oracle_inputs of them),
  - a probe and amplitudes that are float32 numbers,
  - amplitudes m = |ref| U(0, 2) (reference_model.measurement_wide: no cancellation in the seed).

BOUND = 2e-5 on rel(g, g_ref) for g_delta, g_beta and, where the case has one, the probe gradient; LOSS_BOUND = 1e-5.  The bound
of a case is BOUND unless the complex64 restatement of that case (modulation_reference.c64_loss_and_grad) itself exceeds half of
it: then it is twice the restatement's figure rounded up to one significant digit, written in the case ('bound'), and
test_gradient_conditioning.py holds the restatement to half of whatever stands here.  No bound comes from a device figure.  A case
whose bound would pass 1e-4 is left out (LEFT_OUT says which and why).
"""
import functools

import numpy as np

from oracle import bdof_oracle as orc

import modulation_reference as mref
import poisson_reference as pref
import reference_model as ref_model
import weights_reference as wref

f32, f64 = np.float32, np.float64
E, PS = mref.E_EV, mref.PSIZE_CM
BOUND, LOSS_BOUND = 2e-5, 1e-5
MU = 2e6                                              # tests/test_gpu_poisson.py
PLANES = (5e-5, 1e-4)
FPS = (None, 1e-4, 'inf')


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def bound_rule(figure):
    """The bound the module's docstring gives a case whose complex64 restatement reaches `figure` (its worst gradient error)."""
    if figure <= 0.5 * BOUND:
        return BOUND
    e = np.floor(np.log10(2 * figure))
    return float('{:.0e}'.format(np.ceil(2 * figure / 10 ** e - 1e-9) * 10 ** e))


# ---- the table ----------------------------------------------------------------------------------------------------------------------
def _case(path, Y, X, regime='weak', fp=1e-4, B=2, S=5, variant='numpy_skip_last', engine='streaming', bound=BOUND, **opt):
    """opt: fused (fused forward + adjoint sweeps), recompute, adjoint64, b (slice binning), streams, weights ('random', 'beamstop'),
    loss ('poisson'), probe_grad.  fp: None, 'inf', a distance in cm or a tuple of distances (detector planes)."""
    assert set(opt) <= {'fused', 'recompute', 'adjoint64', 'b', 'streams', 'weights', 'loss', 'probe_grad'}, opt
    c = dict(path=path, Y=Y, X=X, regime=regime, fp=fp, B=B, S=S, variant=variant, engine=engine, bound=bound)
    c.update(opt)
    return c


def case_id(c):
    skip = ('path', 'Y', 'X', 'regime', 'fp', 'bound', 'engine')
    extra = ['{}={}'.format(k, c[k]) for k in sorted(c) if k not in skip and not (k, c[k]) in (('B', 2), ('S', 5), ('variant', 'numpy_skip_last'))]
    return '-'.join([c['path'], '{}x{}'.format(c['Y'], c['X']), c['regime'], str(c['fp'])] + extra)


def _streaming():
    out = []
    for Y, X in ((64, 64), (128, 128), (64, 256), (256, 128)):
        out += [_case('two-kernel', Y, X, fp=fp) for fp in FPS]
    out += [_case('two-kernel', 512, 512, fp=fp, B=1, S=3) for fp in FPS]
    out += [_case('two-kernel', 1024, 1024, fp=None, B=1, S=3), _case('two-kernel', 512, 1024, fp='inf', B=1, S=3)]   # test_larger_sizes_vs_oracle's
    out += [_case('two-kernel', 64, 64, fp=fp, variant='tf_all') for fp in FPS]
    out += [_case('two-kernel', 64, 128, regime=r, fp=fp) for r in ('weak', 'pi', 'absorbing') for fp in FPS]
    out += [_case('two-kernel', 64, 64, fp=1e-4, S=70)]      # more steps than the 64 dithered copies of every constant
    return out


def _others():
    out = []
    for r in ('weak', 'pi'):
        # S = 4: the smallest the fused sweeps admit (even, above 2; tests/test_gpu_fused_adjoint.py)
        out += [_case('fused', 64, 128, r, S=4, fused=True), _case('fused', 256, 256, r, S=4, fused=True),
                _case('fused', 512, 512, r, B=1, S=4, fused=True)]
        out += [_case('resident', n, n, r, S=6, engine='resident') for n in (64, 128)]
        out += [_case('generic', 72, 72, r, S=6, engine='generic'), _case('generic-adjoint64', 72, 72, r, S=6, engine='generic', adjoint64=True)]
        out += [_case('streams', 64, 128, r, B=7, S=6, streams=2)]
        out += [_case('binning', 64, 64, r, S=6, b=2)]
        out += [_case('planes', 64, 128, r, fp=PLANES, S=6)]
        out += [_case('weights', 64, 128, r, S=6, weights='random'), _case('weights', 64, 128, r, fp='inf', S=6, weights='beamstop')]
        out += [_case('poisson', 64, 128, r, S=6, loss='poisson')]
        out += [_case('probe-gradient', 64, 128, r, S=6, probe_grad=True)]
    out += [_case('tape-free', 64, 128, 'pi', S=6, recompute=True)]
    return out


CASES = _streaming() + _others()
# 64 steps deep: the restatement's g_beta reaches 3.0e-5 (full field, 'pi'), 2.5e-5 and 3.5e-5 (ptychography), hence these bounds
SOLVER_CASES = [dict(path='fullfield-solver', regime='weak', bound=BOUND), dict(path='fullfield-solver', regime='pi', bound=6e-5),
                dict(path='ptycho-solver', regime='weak', bound=5e-5), dict(path='ptycho-solver', regime='pi', bound=8e-5)]
LEFT_OUT = {}                   # no case's bound passes 1e-4: none is left out


def solver_id(c):
    return '{}-{}'.format(c['path'], c['regime'])


# ---- objects, probes, data ----------------------------------------------------------------------------------------------------------
def obj(regime, shape, seed=0):
    """(delta32, beta32, delta_eff, beta_eff).  'weak': delta in [0, 2e-5], beta = 0.1 delta (tests/test_gpu_parity.py); else a
    regime of modulation_reference.  The float64 pair is what the device's float32 arguments k delta, -k beta amount to."""
    if regime == 'weak':
        d32 = np.random.default_rng([seed, 5]).uniform(0, 2e-5, shape).astype(f32)
        b32 = (f32(0.1) * d32).astype(f32)
    else:
        d32, b32 = mref.regime(regime, shape, seed=seed)
    return (d32, b32) + mref.oracle_inputs(d32, b32)


def probe(fp, Y, X):
    """A gaussian probe (a carrier field) in the far field, as elsewhere; a plane wave with 2 % of structure (a scalar carrier)
    otherwise.  Rounded to float32."""
    pr, pi = mref.probe('gaussian' if fp == 'inf' else 'structured', Y, X)
    return np.asarray(pr).astype(f32).astype(f64), np.asarray(pi).astype(f32).astype(f64)


def wide(ref_wave, seed=0):
    return ref_model.measurement_wide(ref_wave, seed).astype(f32).astype(f64)


def _weights(c):
    kind = c.get('weights')
    if kind is None:
        return None
    if kind == 'beamstop':
        return wref.beamstop((c['Y'], c['X']))
    return wref.random_weights((c['Y'], c['X']), np.random.default_rng(3))


def terms(c, w=None):
    """(the float64 data term, its complex64 restatement) of a case."""
    loss_type = c.get('loss', 'lsq')
    if w is not None:
        return ref_model.data_term(wref.weighted_loss, wref.weighted_seed, w, loss_type, MU), mref.c64_term(loss_type, MU, w)
    if loss_type == 'poisson':
        return ref_model.data_term(pref.poisson_loss, pref.poisson_seed, MU), mref.c64_term('poisson', MU)
    return ref_model.lsq, mref.c64_term()


def _fp(c):
    return list(c['fp']) if isinstance(c['fp'], tuple) else c['fp']


@functools.lru_cache(maxsize=4)
def _problem(key):
    c = dict(key)
    d32, b32, de, be = obj(c['regime'], (c['B'], c['Y'], c['X'], c['S']))
    pr, pi = probe(c['fp'], c['Y'], c['X'])
    fp, b = _fp(c), c.get('b', 1)
    wave, _ = ref_model.forward(de, be, pr, pi, E, PS, fp, c['variant'], b)
    meas = wide(wave)
    w = _weights(c)
    loss, gd, gb, g0, _ = ref_model.loss_and_grad(de, be, pr, pi, E, PS, meas, fp, c['variant'], b, term=terms(c, w)[0])
    out = dict(delta32=d32, beta32=b32, delta_eff=de, beta_eff=be, pr=pr, pi=pi, meas=meas, w=w, loss=loss, gd=gd, gb=gb, gp=g0.sum(axis=0))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def problem(c):
    """Inputs and float64 results of a case, computed once and shared (read only): dict(delta32, beta32, delta_eff, beta_eff, pr,
    pi, meas, w, loss, gd, gb, gp) — gp = G(psi_0) summed over the batch."""
    return _problem(tuple(sorted(c.items())))


def errors(c, p, loss, gd, gb, gp=None):
    """(loss, g_delta, g_beta[, probe gradient]) relative errors against the case's float64 results."""
    e = [abs(loss - p['loss']) / abs(p['loss']), rel(gd, p['gd']), rel(gb, p['gb'])]
    if c.get('probe_grad'):
        e.append(rel(gp, p['gp']))
    return tuple(float(v) for v in e)


def restatement(c, p=None):
    """errors() of the plain complex64 restatement of a case."""
    p = p or problem(c)
    _, loss, gd, gb, g0 = mref.c64_loss_and_grad(p['delta_eff'], p['beta_eff'], p['pr'], p['pi'], p['meas'], _fp(c), c['variant'],
                                                b=c.get('b', 1), term=terms(c, p['w'])[1], probe_grad=True)
    return errors(c, p, loss, gd, gb, g0.astype(np.complex128).sum(axis=0))


# ---- the solver level ---------------------------------------------------------------------------------------------------------------
N, N_THETA = 64, 4
FF_ANGLES = (0, 1, 3)
PTY_POS = np.array([(32, 32), (32, 33), (10, 50), (60, 8)])          # tests/test_gpu_modulation.py: three windows hang over the edge
PTY_THETA = 2


@functools.lru_cache(maxsize=None)
def _solver_problem(path, regime):
    d32, b32, de, be = obj(regime, (N, N, N), seed=3)
    coords = orc.rotation_lookup([N, N, N], N_THETA)
    out = dict(delta32=d32, beta32=b32, delta_eff=de, beta_eff=be, coords=coords)
    stack = np.stack([de, be], axis=3)
    if path == 'fullfield-solver':
        fp, idx = 1e-4, np.array(FF_ANGLES)
        pr, pi = np.ones((N, N)), np.zeros((N, N))
        rot = np.stack([orc.apply_rotation(stack, coords[j]) for j in idx])
        wave, _ = ref_model.forward(rot[..., 0], rot[..., 1], pr, pi, E, PS, fp)
        meas = wide(wave)
        loss, gd, gb, _ = ref_model.fullfield_loss_and_grad(de, be, coords, idx, meas, pr, pi, E, PS, fp)
        out.update(fp=fp, idx=idx, rot=rot)
    else:
        fp, psz = 'inf', (N, N)
        pr, pi = [np.asarray(v).astype(f32).astype(f64) for v in orc.gaussian_probe(psz, 6., 6., 0.5)]
        pad, half = orc.ptycho_pad_amounts(PTY_POS, psz, (N, N, N))
        rot1 = orc.apply_rotation(stack, coords[PTY_THETA])
        obj_pad = np.pad(rot1, ((pad[0, 0], pad[0, 1]), (pad[1, 0], pad[1, 1]), (0, 0), (0, 0)), mode='constant')
        rot = np.stack([obj_pad[p[0] + pad[0, 0] - half[0]:p[0] + pad[0, 0] - half[0] + psz[0],
                                p[1] + pad[1, 0] - half[1]:p[1] + pad[1, 0] - half[1] + psz[1]] for p in PTY_POS])
        wave, _ = ref_model.forward(rot[..., 0], rot[..., 1], pr, pi, E, PS, fp)
        meas = wide(wave)
        loss, gd, gb = ref_model.ptycho_loss_and_grad(de, be, coords[PTY_THETA], PTY_POS, PTY_POS, meas, pr, pi, psz, E, PS)
        out.update(fp=fp, psz=psz)
    out.update(pr=pr, pi=pi, meas=meas, loss=loss, gd=gd, gb=gb)
    # the rotated-frame results, for the restatement: the rotation and the windows are index work that float32 does exactly
    rl, rgd, rgb, _, _ = ref_model.loss_and_grad(rot[..., 0], rot[..., 1], pr, pi, E, PS, meas, fp)
    out.update(rot_delta=rot[..., 0], rot_beta=rot[..., 1], rot_gd=rgd, rot_gb=rgb)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def solver_problem(c):
    """A 64^3 volume, float64 results in the volume's frame (loss, gd, gb) and in the rotated frame (rot_*): the full-field
    solver's three angles through the rotation tables behind a plane wave, near-field detector; the ptychography solver's four
    windows at one angle, far field, amplitudes on the reference's detector waves."""
    return _solver_problem(c['path'], c['regime'])


def solver_restatement(c):
    """(loss, g_delta, g_beta) errors of the complex64 restatement on the solver's rotated fields, in the rotated frame."""
    p = solver_problem(c)
    _, loss, gd, gb = mref.c64_loss_and_grad(p['rot_delta'], p['rot_beta'], p['pr'], p['pi'], p['meas'], p['fp'])
    return (float(abs(loss - p['loss']) / abs(p['loss'])), float(rel(gd, p['rot_gd'])), float(rel(gb, p['rot_gb'])))
