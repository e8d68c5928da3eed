"""Float64 reference of the Poisson (photon-counting) data term — numpy, test side.

oracle/bdof_oracle.py's multislice_loss_and_grad hard-codes the least-squares seed, so this module restates the two things that
differ and nothing else: the detector-plane loss / seed (include/bdof.h, bdof_set_loss) and the adjoint sweep that carries the
seed back.  The forward model (multislice_propagate_batch_numpy), the propagation kernels and the rotation functions are the
oracle's own.

Per detector pixel, a = |d|, m the measured amplitude, mu photons per unit intensity:
    L = mean( mu (a^2 - m^2 - 2 m^2 ln(a / m)) )        (m = 0: mu a^2; a = 0: nothing)
    G(d) = dL/dRe d + i dL/dIm d = (2 mu / n) (1 - m^2 / a^2) d
"""
import numpy as np

from oracle import bdof_oracle as orc


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


def forward(delta, beta, probe_real, probe_imag, energy_ev, psize_cm, free_prop_cm=None, variant='numpy_skip_last'):
    """The oracle's forward model, unmodified: (detector wave [B, Y, X], wave after every slice step [S, B, Y, X])."""
    return orc.multislice_propagate_batch_numpy(delta, beta, probe_real, probe_imag, energy_ev, psize_cm, free_prop_cm,
                                                delta.shape, variant=variant)


def loss_only(delta, beta, probe_real, probe_imag, energy_ev, psize_cm, meas_abs, mu, free_prop_cm=None, variant='numpy_skip_last'):
    d, _ = forward(delta, beta, probe_real, probe_imag, energy_ev, psize_cm, free_prop_cm, variant)
    return poisson_loss(d, meas_abs, mu)


def poisson_loss_and_grad(delta, beta, probe_real, probe_imag, energy_ev, psize_cm, meas_abs, mu, free_prop_cm=None,
                          variant='numpy_skip_last', pi=orc.PI):
    """(loss, g_delta [B, Y, X, S], g_beta, g_probe [B, Y, X] complex = dL/dRe psi_0 + i dL/dIm psi_0 per wavefield)."""
    B, Y, X, S = delta.shape
    voxel_nm = np.array([psize_cm] * 3) * 1.e7
    lmbda_nm = 1240. / energy_ev
    h = orc.get_kernel(voxel_nm[-1], lmbda_nm, voxel_nm, (Y, X, S), pi=pi)
    k = 2. * pi * voxel_nm[-1] / lmbda_nm
    d, after = forward(delta, beta, probe_real, probe_imag, energy_ev, psize_cm, free_prop_cm, variant)
    psi0 = np.zeros((B, Y, X), dtype=np.complex64)
    psi0 += (np.asarray(probe_real) + 1j * np.asarray(probe_imag))          # the forward model's complex64 start (np_funcs.py:20-21)
    loss = poisson_loss(d, meas_abs, mu)
    G = poisson_seed(d, meas_abs, mu)

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
