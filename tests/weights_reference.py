"""Float64 reference of the detector weights (bdof_set_detector_weights, include/bdof.h) — numpy, test side.

One plane w >= 0 shared by every measurement of a run.  With l the per-pixel term of the data term (least squares: (|d| - m)^2;
Poisson: the deviance of tests/poisson_reference.py) over B wavefields of Y X pixels
    L    = sum(w l) / (B Y X)            — the divisor is the pixel count, not sum(w)
    G(d) = w (the unweighted seed)
and a pixel with w = 0 takes no part, whatever m holds there (NaN, inf, a saturated count).

This module holds the weighted loss and the weighted seed of both data terms, and the weight planes of the tests; the model
around them is tests/reference_model.py's, which takes them as its data term
(reference_model.data_term(weighted_loss, weighted_seed, w, loss_type, mu))."""
import numpy as np

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
