"""Float64 reference of the detector weights (bdof_set_detector_weights, include/bdof.h) — numpy, test side.

One plane w >= 0 shared by every measurement of a run.  With l the per-pixel term of the data term (least squares: (|d| - m)^2;
Poisson: the deviance of tests/poisson_reference.py) over B wavefields of Y X pixels
    L    = sum(w l) / (B Y X)            — the divisor is the pixel count, not sum(w)
    G(d) = w (the unweighted seed)
and a pixel with w = 0 takes no part, whatever m holds there (NaN, inf, a saturated count).

The forward model, the propagation kernels and the rotation / window functions are the oracle's own; this module restates the
weighted loss, the weighted seed and the adjoint sweep that carries the seed back (as poisson_reference does for its term), for
both data terms, and returns the probe gradient as well."""
import numpy as np

from oracle import bdof_oracle as orc

import poisson_reference as pref


def _masked(meas_abs, w):
    """The amplitudes with 0 where w == 0: what is there in the data must not reach the arithmetic (0 * NaN is NaN)."""
    return np.where(np.asarray(w) > 0, np.asarray(meas_abs, dtype=np.float64), 0.0)


def pixel_terms(d, meas_abs, loss_type, mu):
    """Per-pixel loss term l (no weight, no mean) of detector waves d against amplitudes meas_abs."""
    a = np.abs(d)
    m = np.asarray(meas_abs, dtype=np.float64)
    if loss_type == 'lsq':
        return (a - m) ** 2
    with np.errstate(divide='ignore', invalid='ignore'):
        log_term = np.where((m > 0) & (a > 0), 2.0 * m * m * np.log1p((a - m) / np.where(m > 0, m, 1.0)), 0.0)
    return np.where(a > 0, mu * ((a - m) * (a + m) - log_term), 0.0)


def weighted_loss(d, meas_abs, w, loss_type='lsq', mu=2e6):
    return float(np.sum(w * pixel_terms(d, _masked(meas_abs, w), loss_type, mu)) / d.size)


def weighted_seed(d, meas_abs, w, loss_type='lsq', mu=2e6):
    """G(d) = dL/dRe d + i dL/dIm d."""
    m = _masked(meas_abs, w)
    if loss_type == 'poisson':
        return w * pref.poisson_seed(d, m, mu)
    a = np.abs(d)
    with np.errstate(divide='ignore', invalid='ignore'):
        unit = np.where(a > 0, d / a, 0)
    return w * (2.0 * (a - m) * unit / d.size)


def loss_only(delta, beta, probe_real, probe_imag, energy_ev, psize_cm, meas_abs, w, loss_type='lsq', mu=2e6, free_prop_cm=None,
              variant='numpy_skip_last'):
    d, _ = pref.forward(delta, beta, probe_real, probe_imag, energy_ev, psize_cm, free_prop_cm, variant)
    return weighted_loss(d, meas_abs, w, loss_type, mu)


def loss_and_grad(delta, beta, probe_real, probe_imag, energy_ev, psize_cm, meas_abs, w, loss_type='lsq', mu=2e6, free_prop_cm=None,
                  variant='numpy_skip_last', pi=orc.PI):
    """(loss, g_delta [B, Y, X, S], g_beta, g_probe [B, Y, X] complex = dL/dRe psi_0 + i dL/dIm psi_0 per wavefield).
    w: (Y, X), in the orientation of one detector frame (the far field fftshifted, as the oracle's forward model returns it)."""
    B, Y, X, S = delta.shape
    w = np.asarray(w, dtype=np.float64)
    assert w.shape == (Y, X)
    voxel_nm = np.array([psize_cm] * 3) * 1.e7
    lmbda_nm = 1240. / energy_ev
    h = orc.get_kernel(voxel_nm[-1], lmbda_nm, voxel_nm, (Y, X, S), pi=pi)
    k = 2. * pi * voxel_nm[-1] / lmbda_nm
    d, after = pref.forward(delta, beta, probe_real, probe_imag, energy_ev, psize_cm, free_prop_cm, variant)
    psi0 = np.zeros((B, Y, X), dtype=np.complex64)
    psi0 += (np.asarray(probe_real) + 1j * np.asarray(probe_imag))          # the forward model's complex64 start (np_funcs.py:20-21)
    loss = weighted_loss(d, meas_abs, w, loss_type, mu)
    G = weighted_seed(d, meas_abs, w, loss_type, mu)

    def prop_adj(G, hh):
        return np.fft.ifft2(np.fft.ifftshift(np.fft.fftshift(np.fft.fft2(G), axes=[1, 2]) * np.conj(hh), axes=[1, 2]))

    if free_prop_cm == 'inf':
        G = (Y * X) * np.fft.ifft2(np.fft.ifftshift(G, axes=[1, 2]))
    elif free_prop_cm is not None:
        G = prop_adj(G, orc.get_kernel(free_prop_cm * 1e7, lmbda_nm, voxel_nm, (Y, X, S), pi=pi))
    g_delta, g_beta = np.zeros((B, Y, X, S)), np.zeros((B, Y, X, S))
    for i in range(S - 1, -1, -1):
        if i < S - 1 or variant == 'tf_all':
            G = prop_adj(G, h)
        c = np.exp(1j * k * delta[..., i]) * np.exp(-k * beta[..., i])
        phi = (psi0.astype(np.complex128) if i == 0 else after[i - 1]) * c      # the wave that left slice i's modulation
        t = np.conj(phi) * G
        g_delta[..., i] = k * t.imag
        g_beta[..., i] = -k * t.real
        G = np.conj(c) * G
    return loss, g_delta, g_beta, G


def random_weights(shape, rng, zero_fraction=0.1):
    """Uniform in [0.25, 1.75] with about zero_fraction of the pixels at 0, and a weight > 0 on the DC bin of a far-field frame
    (the centre of the fftshifted frame) and on pixel (0, 0): mean about 0.9, so a weighted gradient keeps the size of the
    unweighted one."""
    Y, X = shape
    w = rng.uniform(0.25, 1.75, size=shape)
    w[rng.uniform(size=shape) < zero_fraction] = 0.0
    for y, x in ((Y // 2, X // 2), (0, 0)):
        if w[y, x] == 0:
            w[y, x] = 1.0
    return w.astype(np.float32)


def beamstop(shape, radius=3):
    """1 everywhere but 0 on a disc around the centre of the fftshifted frame (which is the DC bin)."""
    Y, X = shape
    y, x = np.mgrid[:Y, :X]
    return ((y - Y // 2) ** 2 + (x - X // 2) ** 2 > radius ** 2).astype(np.float32)


def ptycho_loss_and_grad(obj_delta, obj_beta, coord_old, probe_pos_all, this_pos_batch, this_prj_batch, probe_real, probe_imag,
                         probe_size, energy_ev, psize_cm, w, loss_type='lsq', mu=2e6, variant='numpy_skip_last'):
    """Rotate, pad, cut the windows (the oracle's functions), weighted far-field loss and gradient, scatter back, crop, rotation
    adjoint: (loss, g_delta, g_beta) with the gradients in the volume's frame."""
    obj_size = obj_delta.shape
    obj_rot = orc.apply_rotation(np.stack([obj_delta, obj_beta], axis=3), coord_old)
    pad, half = orc.ptycho_pad_amounts(probe_pos_all, probe_size, obj_size)
    obj_pad = np.pad(obj_rot, ((pad[0, 0], pad[0, 1]), (pad[1, 0], pad[1, 1]), (0, 0), (0, 0)), mode='constant')

    def window(pos):
        p0, p1 = int(pos[0]) + pad[0, 0] - half[0], int(pos[1]) + pad[1, 0] - half[1]
        return slice(p0, p0 + probe_size[0]), slice(p1, p1 + probe_size[1])

    subs = np.stack([obj_pad[window(pos)] for pos in this_pos_batch])
    loss, gd_sub, gb_sub, _ = loss_and_grad(subs[..., 0], subs[..., 1], probe_real, probe_imag, energy_ev, psize_cm, this_prj_batch, w,
                                            loss_type, mu, 'inf', variant)
    g_pad = np.zeros(obj_pad.shape)
    for bi, pos in enumerate(this_pos_batch):
        win = window(pos)
        g_pad[win[0], win[1], :, 0] += gd_sub[bi]
        g_pad[win[0], win[1], :, 1] += gb_sub[bi]
    g_rot = g_pad[pad[0, 0]:pad[0, 0] + obj_size[0], pad[1, 0]:pad[1, 0] + obj_size[1]]
    g = orc.apply_rotation_adjoint(g_rot, coord_old)
    return loss, g[..., 0], g[..., 1]
