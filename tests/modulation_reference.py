"""Reference of the modulation table c - 1 = exp(i k delta) exp(-k beta) - 1 (csrc/bdof_kernels.h: slice_modulation_m1, sin_cosm1,
k_modulation_table, k_rot_bilinear<MOD>) — numpy, test side, shared by test_modulation_reference.py (no GPU) and test_gpu_modulation.py.

  reference(x32, y32)   the exact factor in float64, AT the float32 arguments the device forms: x32 = fl32(k32 delta32),
                        y32 = fl32(-k32 beta32), k32 = float32(engine.k).  At |x| = 1e5 a float32 argument is spaced 0.008 rad: a
                        reference at the float64 product k delta would measure that spacing, not the kernel.
  bound(x32, y32)       per-entry bound on |device - reference| (complex modulus):
                            8 2^-24 |reference|  +  e^y (2^-22 + |y| 2^-23) (|sin x| + [|y| >= 0.1])
                        The first term is the polynomial arithmetic, relative to |c - 1| itself — small where c - 1 is small, the
                        property the c - 1 form exists for.  The second is the hardware exponential: one ulp of e^y plus the
                        rounding of y log2(e) in front of exp2; it enters through Im = e sin x always and through Re only on the
                        e - 1 branch (|y| >= 0.1).
  emulate(...)          slice_modulation_m1 restated in numpy float32, fmaf(a, b, c) = float32(float64(a) float64(b) + float64(c)),
                        with a correctly rounded exponential: shows that the algorithm alone satisfies the bound, and — through its
                        `wrong` variants — that the cases below tell a subtly wrong kernel from a right one.
  sweep / switches / special   the cases.  Domain: |x| <= 1e5, -100 <= y <= 10.
  regime / oracle_inputs / c64_*   strong-phase objects for every engine, and a plain complex64 restatement of the oracle (scipy.fft,
                        no carrier splitting): the error level a float32 engine can be asked for at these objects.  With the
                        options of tests/reference_model.py (slice binning, detector planes, a data term, the probe gradient) it
                        also conditions the bounds of tests/gradient_cases.py.
"""
import numpy as np
import scipy.fft

from oracle import bdof_oracle as orc

f32, f64 = np.float32, np.float64
E_EV, PSIZE_CM = 5000., 1e-7
K64 = 2. * orc.PI * 1.0 / (1240. / E_EV)                 # np_funcs.py:32 at 5 keV, 1 nm (MultisliceEngine.k after set_physics)
K64_CONV = 2. * np.pi * 1.0 / (1240. / E_EV)             # propagation.py:25: numpy's pi (set_conv)
X_MAX, Y_MIN, Y_MAX = 1e5, -100., 10.
Y_SWITCH = f32(0.1)                                      # below: the expm1 series; from here on: e - 1

TWO_OVER_PI = f32(0.636619772367581343)
CW1, CW2, CW3 = f32(1.5703125), f32(4.837512969970703125e-4), f32(7.54978995489188216e-8)


# ---- arguments --------------------------------------------------------------------------------------------------------------------
def arguments(delta32, beta32, k32):
    """(x32, y32) as slice_modulation_m1 forms them: one float32 product each."""
    delta32, beta32, k32 = np.asarray(delta32, f32), np.asarray(beta32, f32), f32(k32)
    return k32 * delta32, (-k32) * beta32


def classify(x32, y32):
    """(n, quadrant, series) per entry: the reduction's integer n = rint(x 2/pi) and q = (int)n & 3 as the device takes them,
    and whether the expm1 series (True) or e - 1 (False) runs."""
    n = np.rint(np.asarray(x32, f32) * TWO_OVER_PI).astype(np.int64)
    return n, n & 3, np.abs(np.asarray(y32, f32)) < Y_SWITCH


# ---- exact value and bound ----------------------------------------------------------------------------------------------------------
def reference(x32, y32):
    """expm1(y) cos(x) + (cos(x) - 1)  +  i exp(y) sin(x) in float64 (cos x - 1 as -2 sin^2(x / 2): the same number, no cancellation)."""
    x, y = np.asarray(x32, f32).astype(f64), np.asarray(y32, f32).astype(f64)
    cm1 = -2. * np.sin(0.5 * x) ** 2
    return np.expm1(y) * (1. + cm1) + cm1 + 1j * np.exp(y) * np.sin(x)


def bound(x32, y32):
    x, y = np.asarray(x32, f32).astype(f64), np.asarray(y32, f32).astype(f64)
    em1_branch = (np.abs(np.asarray(y32, f32)) >= Y_SWITCH).astype(f64)
    return 8. * 2. ** -24 * np.abs(reference(x32, y32)) + np.exp(y) * (2. ** -22 + np.abs(y) * 2. ** -23) * (np.abs(np.sin(x)) + em1_branch)


# ---- the device function in numpy float32 ---------------------------------------------------------------------------------------------
def _fma(a, b, c):
    return (np.asarray(a, f32).astype(f64) * np.asarray(b, f32).astype(f64) + np.asarray(c, f32).astype(f64)).astype(f32)


WRONG = ('quadrants_rotated', 'q2_sign', 'q1_plus_sp', 'fmod_quadrant', 'no_third_constant', 'em1_everywhere', 'series_to_half')


def emulate(delta32, beta32, k32, wrong=None, exp32=None):
    """slice_modulation_m1(db, k) as complex64.  wrong: one of WRONG — the same function with one plausible defect.  exp32: the
    float32 exponential in place of the correctly rounded one (measurements of what an exponential that is off costs)."""
    assert wrong is None or wrong in WRONG
    x, y = arguments(delta32, beta32, k32)
    one = f32(1)
    with np.errstate(over='ignore', invalid='ignore'):
        n = np.rint(x * TWO_OVER_PI)
        r = _fma(-n, CW1, x)
        r = _fma(-n, CW2, r)
        if wrong != 'no_third_constant':
            r = _fma(-n, CW3, r)
        r2 = r * r
        sp = _fma(r * r2, _fma(r2, _fma(r2, f32(-1.9515295891e-4), f32(8.3321608736e-3)), f32(-1.6666654611e-1)), r)
        cpm1 = _fma(r2 * r2, _fma(r2, _fma(r2, f32(2.443315711809948e-5), f32(-1.388731625493765e-3)), f32(4.166664568298827e-2)), f32(-0.5) * r2)
        if wrong == 'fmod_quadrant':
            q = np.fmod(n, f32(4)).astype(np.int64)            # -3 .. 3: the remainder takes the sign of n
        else:
            q = n.astype(np.int64) & 3
        if wrong == 'quadrants_rotated':
            q = (q + 1) & 3
        cp = one + cpm1
        s = np.where(q == 0, sp, np.where(q == 1, cp, np.where(q == 2, sp if wrong == 'q2_sign' else -sp, -cp)))
        cm1 = np.where(q == 0, cpm1, np.where(q == 1, (sp - one) if wrong == 'q1_plus_sp' else (-sp - one),
                                              np.where(q == 2, f32(-2) - cpm1, sp - one)))
        e = np.exp(y.astype(f64)).astype(f32) if exp32 is None else exp32(y)
        poly = y * _fma(y * f32(0.5), _fma(y * (one / f32(3)), _fma(y * f32(0.25), _fma(y, f32(0.2), one), one), one), one)
        switch = {'em1_everywhere': f32(0), 'series_to_half': f32(0.5)}.get(wrong, Y_SWITCH)
        em1 = np.where(np.abs(y) < switch, poly, e - one)
        return (_fma(em1, one + cm1, cm1) + 1j * (e * s).astype(f64)).astype(np.complex64)


# ---- cases --------------------------------------------------------------------------------------------------------------------------
def _ulps(v32, steps):
    """v32 moved by `steps` float32 neighbours (steps: integer array, broadcast)."""
    v32 = np.asarray(v32, f32)
    i = v32.view(np.int32).astype(np.int64)
    i = np.where(i < 0, -(i & 0x7fffffff), i)                   # sign-magnitude -> monotone integer
    i = i + steps
    i = np.where(i < 0, (-i) | 0x80000000, i)
    return i.astype(np.uint32).view(f32)


def solve(target, k32, lo=-np.inf, hi=np.inf):
    """A float32 v with fl32(k32 v) equal to the float32 target where one exists among the neighbours of target / k32 (k32 = 25.3
    skips some products), else the closest; stepped towards zero while the product lies outside [lo, hi]."""
    k32 = f32(k32)
    t = np.asarray(target, f32)
    v0 = (t.astype(f64) / f64(k32)).astype(f32)
    best = v0
    err = np.abs((k32 * v0).astype(f64) - t)
    for s in (-1, 1, -2, 2):
        v = _ulps(v0, s)
        e = np.abs((k32 * v).astype(f64) - t)
        better = e < err
        best, err = np.where(better, v, best), np.where(better, e, err)
    out = (k32 * best < f32(lo)) | (k32 * best > f32(hi))
    while out.any():
        best = np.where(out, _ulps(best, -np.sign(best).astype(np.int64)), best)
        out = (k32 * best < f32(lo)) | (k32 * best > f32(hi))
    return best.astype(f32)


def _object(x_target, y_target, k32):
    """(delta32, beta32) whose device arguments are the targets (or their nearest reachable neighbours), inside the domain."""
    return solve(x_target, k32, -X_MAX, X_MAX), (-solve(y_target, k32, Y_MIN, Y_MAX) + f32(0)).astype(f32)


SWEEP_N = (1 << 21) + 77          # > 16 * 256 entries per CU on 256 CUs: the grid-stride loop takes a second and a ragged third trip


def sweep(k32, n=SWEEP_N, seed=11):
    """|x| and |y| log-uniform from 1e-9 to the domain's edge, x of both signs, a fifth of the y positive."""
    rng = np.random.default_rng(seed)
    x = np.exp(rng.uniform(np.log(1e-9), np.log(X_MAX), n)) * rng.choice([-1., 1.], n)
    pos = rng.random(n) < 0.2
    y = np.where(pos, np.exp(rng.uniform(np.log(1e-9), np.log(Y_MAX), n)), -np.exp(rng.uniform(np.log(1e-9), np.log(-Y_MIN), n)))
    return _object(x.astype(f32), y.astype(f32), k32)


SWITCH_M = list(range(-40, 41)) + [-63660, -61234, -60001, -60000, 60000, 60001, 61234, 63660]


def switches(k32):
    """x = fl32((2m + 1) pi / 4) moved by -3 .. 3 ulps (where n = rint(x 2/pi) changes) crossed with y = +-0.1f moved by -3 .. 3 ulps
    and y = 0.  Returns (delta32, beta32, m of every entry)."""
    m = np.array(SWITCH_M, dtype=np.int64)
    step = np.arange(-3, 4)
    xs = _ulps(((2 * m[:, None] + 1) * (np.pi / 4)).astype(f32), step[None, :])                  # [m][7]
    ys = np.concatenate([_ulps(np.full(7, Y_SWITCH), step), _ulps(np.full(7, -Y_SWITCH), step), np.zeros(1, f32)])
    X, Y = np.broadcast_arrays(xs[:, :, None], ys[None, None, :])
    M = np.broadcast_to(m[:, None, None], X.shape)
    d, b = _object(X.ravel(), Y.ravel(), k32)
    return d, b, M.ravel().copy()


SPECIAL_ZERO = slice(0, 2)        # entries that must compare equal to 0
SPECIAL_OPAQUE = slice(2, 6)      # y = -100: c - 1 = -1 within the bound


def special(k32):
    """(0, 0) and (-0.0, 0): vacuum and out-of-volume rows rely on a factor of exactly 1.  y = -100.  x an exact multiple of 2 pi
    rounded to float32, at 8, 1000 and 15000 turns."""
    turns = (2. * np.pi * np.array([8., 1000., 15000.])).astype(f32)
    x = np.concatenate([f32([0., -0., 0., 1., -2., 99999.]), np.repeat(turns, 4), -turns])
    y = np.concatenate([f32([0., 0., Y_MIN, Y_MIN, Y_MIN, Y_MIN]), np.tile(f32([0., -1e-3, -0.5, 0.25]), 3), f32([0., 0., 0.])])
    d, b = _object(x, y, k32)
    d[1] = f32(-0.)
    return d, b


def worst(table, delta32, beta32, k32):
    """(worst ratio |table - reference| / bound, description of the entry it sits at)."""
    x, y = arguments(delta32, beta32, k32)
    err, bnd = np.abs(np.asarray(table).astype(np.complex128) - reference(x, y)), bound(x, y)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(err == 0, 0., err / bnd)               # the bound is 0 at (0, 0): only an exact 0 passes there
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    i = int(np.argmax(ratio))
    n, q, series = classify(x, y)
    return float(ratio[i]), 'entry {}: x = {!r}, y = {!r}, n = {}, quadrant {}, {} branch'.format(
        i, float(x[i]), float(y[i]), int(n[i]), int(q[i]), 'series' if series[i] else 'e - 1')


# ---- strong-phase objects for the engines ------------------------------------------------------------------------------------------------
REGIMES = ('pi', 'wrapped', 'absorbing')


def regime(name, shape, k64=K64, seed=0):
    """(delta32, beta32) of `shape`, float32 as the device stores them.  Phase per voxel k delta / absorption k beta:
    'pi': U[-pi, pi] / U[0, 0.3] — mean modulation near 0, the carrier dies out; 'wrapped': 2 pi m + U[-0.02, 0.02], integer m in
    -8 .. 8 / 1e-3 — a weak object to physics, a large argument to the reduction; 'absorbing': U[0, 1] / U[0, 0.6]."""
    rng = np.random.default_rng([seed, REGIMES.index(name)])
    if name == 'pi':
        x, a = rng.uniform(-np.pi, np.pi, shape), rng.uniform(0, 0.3, shape)
    elif name == 'wrapped':
        x, a = 2 * np.pi * rng.integers(-8, 9, shape) + rng.uniform(-0.02, 0.02, shape), np.full(shape, 1e-3)
    else:
        x, a = rng.uniform(0, 1, shape), rng.uniform(0, 0.6, shape)
    return (x / k64).astype(f32), (a / k64).astype(f32)


def oracle_inputs(delta32, beta32, k64=K64):
    """(delta_eff, beta_eff) in float64 with k64 delta_eff = x32 and -k64 beta_eff = y32: handed to the float64 oracle, both sides
    see the same phases, and the comparison measures the engine, not the rounding of k delta to float32 (2e-7 rad at pi)."""
    x, y = arguments(delta32, beta32, f32(k64))
    return x.astype(f64) / k64, -y.astype(f64) / k64


def probe(kind, Y, X, seed=0):
    """'gaussian': localised, rides on a carrier field.  'structured': a plane wave with 2 % of structure — every pixel within a
    quarter of the mean, so the engine carries the mean as a scalar and the table's mean rides on it (MultisliceEngine.set_probe)."""
    rng = np.random.default_rng([seed, 77])
    if kind == 'gaussian':
        return orc.gaussian_probe((Y, X), Y / 10., Y / 10., 0.5)
    assert kind == 'structured'
    return 1 + 0.02 * rng.normal(size=(Y, X)), 0.02 * rng.normal(size=(Y, X))


def measurement(ref_wave, seed=0):
    rng = np.random.default_rng([seed, 78])
    return np.abs(ref_wave) * (1 + 0.05 * rng.normal(size=ref_wave.shape))


# ---- the oracle's transfer-function model in plain complex64 ---------------------------------------------------------------------------------
def _c64_kernel(dist_nm, grid_shape):
    voxel_nm = np.array([PSIZE_CM] * 3) * 1.e7
    return np.fft.ifftshift(orc.get_kernel(dist_nm, 1240. / E_EV, voxel_nm, grid_shape)).astype(np.complex64)


def c64_term(loss_type='lsq', mu=2e6, w=None):
    """A data term (d, meas_abs) -> (loss, G(d)) for c64_loss_and_grad: the seed of tests/reference_model.py's lsq, of
    poisson_reference.poisson_seed or, with a weight plane w, of weights_reference.weighted_seed, every factor float32 /
    complex64; the loss is summed in float64 from the float32 amplitudes.  Where w == 0 the amplitude takes no part."""
    def term(d, meas_abs):
        c8 = np.complex64
        assert d.dtype == c8
        absd = np.abs(d)
        m = np.asarray(meas_abs, f32)
        ww = None if w is None else np.asarray(w, f32)
        if ww is not None:
            m = np.where(ww > 0, m, f32(0))
        with np.errstate(divide='ignore', invalid='ignore'):
            if loss_type == 'lsq':
                resid = absd - m
                per_pixel = resid.astype(f64) ** 2
                unit = np.where(absd > 0, d / absd, 0).astype(c8)
                G = (f32(2.0 / d.size) * resid * unit).astype(c8)
            else:
                a64, m64 = absd.astype(f64), m.astype(f64)
                log_term = np.where((m64 > 0) & (a64 > 0), 2.0 * m64 * m64 * np.log1p((a64 - m64) / np.where(m64 > 0, m64, 1.0)), 0.0)
                per_pixel = np.where(a64 > 0, mu * ((a64 - m64) * (a64 + m64) - log_term), 0.0)
                ratio = np.where(absd > 0, f32(1) - (m * m) / (absd * absd), f32(0)).astype(f32)
                G = (f32(2.0 * mu / d.size) * ratio * d).astype(c8)
        if ww is not None:
            per_pixel, G = ww.astype(f64) * per_pixel, (ww * G).astype(c8)
        return float(np.sum(per_pixel) / d.size), G
    return term


def c64_loss_and_grad(delta, beta, probe_real, probe_imag, meas_abs, free_prop_cm=None, variant='numpy_skip_last', k64=K64, b=1,
                      term=None, probe_grad=False):
    """tests/reference_model.py's loss_and_grad (b = 1, one detector, least squares: orc.multislice_loss_and_grad) operation for
    operation with every field, table and factor in complex64 / float32 (scipy.fft keeps the type) and no carrier splitting:
    (detector wave(s), loss, g_delta, g_beta) and, with probe_grad, G(psi_0) [B, Y, X] behind them.  b: slice binning;
    free_prop_cm: None, 'inf', a distance or a sequence of distances; term: a data term of c64_term (None: least squares)."""
    B, Y, X, S = delta.shape
    assert b >= 1 and S % b == 0
    n = S // b
    c8 = np.complex64
    term = term or c64_term()
    h = _c64_kernel(1.0 * b, (Y, X, S))
    c = np.stack([np.exp(1j * k64 * delta[..., i * b:(i + 1) * b].sum(axis=-1)) * np.exp(-k64 * beta[..., i * b:(i + 1) * b].sum(axis=-1))
                  for i in range(n)], axis=-1).astype(c8)                               # the factors themselves rounded once
    psi = np.zeros((B, Y, X), dtype=c8) + (np.asarray(probe_real) + 1j * np.asarray(probe_imag)).astype(c8)
    planes = isinstance(free_prop_cm, (list, tuple, np.ndarray))

    def step(f, hh):
        return scipy.fft.ifft2(scipy.fft.fft2(f, axes=(1, 2)) * hh, axes=(1, 2))

    phis = []
    for i in range(n):
        phi = psi * c[..., i]
        phis.append(phi)
        psi = step(phi, h) if (i < n - 1 or variant == 'tf_all') else phi
    if free_prop_cm is None:
        d = psi
    elif planes:
        hds = [_c64_kernel(z * 1e7, (Y, X, S)) for z in free_prop_cm]
        d = np.stack([step(psi, hd) for hd in hds], axis=1)
    elif free_prop_cm == 'inf':
        d = scipy.fft.fftshift(scipy.fft.fft2(psi, axes=(1, 2)), axes=(1, 2))
    else:
        hd = _c64_kernel(free_prop_cm * 1e7, (Y, X, S))
        d = step(psi, hd)
    assert d.dtype == c8
    loss, G = term(d, meas_abs)
    if free_prop_cm is None:
        pass
    elif planes:
        Gd = G
        G = step(Gd[:, 0], np.conj(hds[0]))
        for j in range(1, len(hds)):
            G = G + step(Gd[:, j], np.conj(hds[j]))
    elif free_prop_cm == 'inf':
        G = f32(Y * X) * scipy.fft.ifft2(scipy.fft.ifftshift(G, axes=(1, 2)), axes=(1, 2))
    else:
        G = step(G, np.conj(hd))
    gd, gb = np.zeros((B, Y, X, S), f32), np.zeros((B, Y, X, S), f32)
    k = f32(k64)
    for i in range(n - 1, -1, -1):
        if i < n - 1 or variant == 'tf_all':
            G = step(G, np.conj(h))
        t = np.conj(phis[i]) * G
        for j in range(b):
            gd[..., i * b + j] = k * t.imag
            gb[..., i * b + j] = -k * t.real
        G = np.conj(c[..., i]) * G
    assert G.dtype == c8
    return (d, loss, gd, gb, G) if probe_grad else (d, loss, gd, gb)


# ---- the engine cases, shared by the CPU check of the bounds and the GPU file ------------------------------------------------------------
B, S = 2, 6
STREAMING_CASES = [(Y, X, r, fp) for (Y, X) in ((64, 64), (64, 128)) for r in REGIMES for fp in (None, 1e-4, 'inf')]
RESIDENT_CASES = [(64, 64, r, fp) for r in REGIMES for fp in (1e-4, 'inf')]
GENERIC_CASES = [(72, 72, r, 1e-4) for r in REGIMES]
ENGINE_CASES = sorted(set(STREAMING_CASES + RESIDENT_CASES + GENERIC_CASES), key=str)
BOUNDS = {'wave': 5e-6, 'intensity': 1e-5, 'loss': 1e-5, 'gradient': 2e-4}           # tests/test_gpu_parity.py


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


_cases = {}


def engine_case(Y, X, name, fp, variant='numpy_skip_last'):
    """Object, probe, measurement and the float64 oracle's results of one case, computed once and shared (read only):
    dict(delta32, beta32, delta_eff, beta_eff, pr, pi, meas, wave, loss, gd, gb).  A gaussian probe for 'inf', as elsewhere; a scalar carrier otherwise."""
    key = (Y, X, name, fp, variant)
    if key not in _cases:
        d32, b32 = regime(name, (B, Y, X, S))
        de, be = oracle_inputs(d32, b32)
        pr, pi = probe('gaussian' if fp == 'inf' else 'structured', Y, X)
        wave, _ = orc.multislice_propagate_batch_numpy(de, be, pr, pi, E_EV, PSIZE_CM, fp, de.shape, variant=variant, return_probe_array=False)
        meas = measurement(wave)
        loss, gd, gb = orc.multislice_loss_and_grad(de, be, pr, pi, E_EV, PSIZE_CM, meas, fp, variant)
        case = dict(delta32=d32, beta32=b32, delta_eff=de, beta_eff=be, pr=pr, pi=pi, meas=meas, wave=wave, loss=loss, gd=gd, gb=gb)
        for v in case.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cases[key] = case
    return _cases[key]


def errors(case, wave, loss, gd, gb):
    """(wave, intensity, loss, g_delta, g_beta) relative errors against the case's oracle results (loss None: skipped)."""
    return (rel(wave, case['wave']), rel(np.abs(wave) ** 2, np.abs(case['wave']) ** 2),
            abs(loss - case['loss']) / abs(case['loss']), rel(gd, case['gd']), rel(gb, case['gb']))


def within(e, scale=1.0):
    b = BOUNDS
    return (e[0] <= scale * b['wave'] and e[1] <= scale * b['intensity'] and e[2] <= scale * b['loss']
            and e[3] <= scale * b['gradient'] and e[4] <= scale * b['gradient'])
