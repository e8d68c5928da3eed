"""Float64 reference of the Poisson (photon-counting) data term — numpy, test side.

oracle/bdof_oracle.py's multislice_loss_and_grad hard-codes the least-squares seed, so this module restates the detector-plane
loss / seed (include/bdof.h, bdof_set_loss) and nothing else; tests/reference_model.py takes them as its data term
(reference_model.data_term(poisson_loss, poisson_seed, mu)) and carries the seed back.

Per detector pixel, a = |d|, m the measured amplitude, mu photons per unit intensity:
    L = mean( mu (a^2 - m^2 - 2 m^2 ln(a / m)) )        (m = 0: mu a^2; a = 0: nothing)
    G(d) = dL/dRe d + i dL/dIm d = (2 mu / n) (1 - m^2 / a^2) d
"""
import numpy as np


def poisson_loss(d, meas_abs, mu):
    """The deviance above of detector waves d against amplitudes meas_abs (same shape), as a mean over all pixels."""
    a = np.abs(d)
    m = np.asarray(meas_abs, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        log_term = np.where((m > 0) & (a > 0), 2.0 * m * m * np.log1p((a - m) / np.where(m > 0, m, 1.0)), 0.0)
    term = np.where(a > 0, mu * ((a - m) * (a + m) - log_term), 0.0)
    return float(np.mean(term))


def poisson_seed(d, meas_abs, mu):
    a = np.abs(d)
    m = np.asarray(meas_abs, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        w = np.where(a > 0, 1.0 - (m * m) / (a * a), 0.0)
    return (2.0 * mu / d.size) * w * d


def lsq_loss(d, meas_abs):
    return float(np.mean((np.abs(d) - meas_abs) ** 2))
