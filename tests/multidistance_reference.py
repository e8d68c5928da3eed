"""Float64 reference of several detector planes per wavefield (bdof_set_detector_planes, include/bdof.h) — numpy, test side.

The object sweep is tests/binning_reference.py's (b voxel slices per step; b = 1 is the oracle's model), the propagation kernel
(get_kernel) and the step (_propagate) are the oracle's own.  Only the stage behind the exit wave is restated: with psi the wave
that enters the detector step (phi_{n-1} under 'numpy_skip_last', P phi_{n-1} under 'tf_all') and D distances z_0 .. z_{D-1} in cm

    d_j    = P(z_j) psi                               detector waves (B, D, Y, X), in the order of the distances
    L      = the data term over all B D Y X pixels    (least squares: mean((|d| - m)^2); any other by `loss_and_seed`)
    G(psi) = sum_j P(z_j)^H G(d_j)

and the sweep back through the object is binning_reference's, operation for operation: D = 1 gives its numbers exactly.
"""
import numpy as np

from oracle import bdof_oracle as orc

import binning_reference as bref

lsq_loss_and_seed = bref.lsq_loss_and_seed


def _kernels(distances_cm, lmbda_nm, voxel_nm, grid_shape, pi):
    if len(distances_cm) < 1:
        raise ValueError('at least one detector plane')
    return [orc.get_kernel(z * 1e7, lmbda_nm, voxel_nm, grid_shape, pi=pi) for z in distances_cm]


def _sweep(delta, beta, probe_real, probe_imag, energy_ev, psize_cm, variant, b, pi, dtype):
    """binning_reference's forward sweep up to the wave in front of the detector step: (psi, phis, cs, optics)."""
    voxel_nm, lmbda_nm, h, k = bref._optics(delta.shape, energy_ev, psize_cm, b, pi)
    n = delta.shape[-1] // b
    psi = bref._start(delta.shape, probe_real, probe_imag)
    if dtype is not None:
        psi = psi.astype(dtype)
    phis, cs = [], []
    for i in range(n):
        c = bref._bin_factor(delta, beta, k, i, b)
        phi = psi * c
        phis.append(phi)
        cs.append(c)
        psi = orc._propagate(phi, h) if (i < n - 1 or variant == 'tf_all') else phi
    return psi, phis, cs, (voxel_nm, lmbda_nm, h, k)


def forward(delta, beta, probe_real, probe_imag, energy_ev, psize_cm, distances_cm, variant='numpy_skip_last', b=1, pi=orc.PI):
    """Detector waves (B, D, Y, X): binning_reference.forward's wave at every distance."""
    B, Y, X, S = delta.shape
    psi, _, _, (voxel_nm, lmbda_nm, _, _) = _sweep(delta, beta, probe_real, probe_imag, energy_ev, psize_cm, variant, b, pi, None)
    return np.stack([orc._propagate(psi, hd) for hd in _kernels(distances_cm, lmbda_nm, voxel_nm, (Y, X, S), pi)], axis=1)


def loss_and_grad(delta, beta, probe_real, probe_imag, energy_ev, psize_cm, meas_abs, distances_cm, variant='numpy_skip_last',
                  b=1, pi=orc.PI, loss_and_seed=lsq_loss_and_seed):
    """(loss, g_delta [B, Y, X, S], g_beta, g_probe [B, Y, X] complex = G(psi_0) per wavefield, detector waves [B, D, Y, X]).
    meas_abs: (B, D, Y, X).  loss_and_seed(d, meas_abs) -> (loss, G(d)) on the (B, D, Y, X) arrays: the least-squares term by
    default; poisson_reference's and weights_reference's terms plug in (a (Y, X) weight plane broadcasts over the planes)."""
    B, Y, X, S = delta.shape
    psi, phis, cs, (voxel_nm, lmbda_nm, h, k) = _sweep(delta, beta, probe_real, probe_imag, energy_ev, psize_cm, variant, b, pi,
                                                        np.complex128)
    hds = _kernels(distances_cm, lmbda_nm, voxel_nm, (Y, X, S), pi)
    d = np.stack([orc._propagate(psi, hd) for hd in hds], axis=1)
    meas_abs = np.asarray(meas_abs)
    assert meas_abs.shape == d.shape, (meas_abs.shape, d.shape)
    loss, Gd = loss_and_seed(d, meas_abs)

    def prop_adj(G, hh):
        return np.fft.ifft2(np.fft.ifftshift(np.fft.fftshift(np.fft.fft2(G), axes=[1, 2]) * np.conj(hh), axes=[1, 2]))

    G = prop_adj(Gd[:, 0], hds[0])
    for j in range(1, len(hds)):
        G = G + prop_adj(Gd[:, j], hds[j])
    n = S // b
    g_delta, g_beta = np.zeros((B, Y, X, S)), np.zeros((B, Y, X, S))
    for i in range(n - 1, -1, -1):
        if i < n - 1 or variant == 'tf_all':
            G = prop_adj(G, h)
        t = np.conj(phis[i]) * G
        for j in range(b):
            g_delta[..., i * b + j] = k * t.imag
            g_beta[..., i * b + j] = -k * t.real
        G = np.conj(cs[i]) * G
    return loss, g_delta, g_beta, G, d


def loss_only(delta, beta, probe_real, probe_imag, energy_ev, psize_cm, meas_abs, distances_cm, variant='numpy_skip_last', b=1):
    d = forward(delta, beta, probe_real, probe_imag, energy_ev, psize_cm, distances_cm, variant, b)
    return float(np.mean((np.abs(d) - meas_abs) ** 2))


def fullfield_loss_and_grad(obj_delta, obj_beta, coord_ls, this_ind_batch, this_prj_batch, probe_real, probe_imag, energy_ev,
                            psize_cm, distances_cm, variant='numpy_skip_last', b=1):
    """Rotate, loss and gradient over the planes, rotation adjoint; no regulariser.  this_prj_batch: (n, D, Y, X).
    Returns (loss, g_delta, g_beta, detector waves (n, D, Y, X))."""
    obj_stack = np.stack([obj_delta, obj_beta], axis=3)
    rot = np.stack([orc.apply_rotation(obj_stack, coord_ls[j]) for j in this_ind_batch])
    loss, gd_rot, gb_rot, _, d = loss_and_grad(rot[..., 0], rot[..., 1], probe_real, probe_imag, energy_ev, psize_cm,
                                               np.abs(this_prj_batch), distances_cm, variant, b)
    gd, gb = np.zeros_like(obj_delta), np.zeros_like(obj_beta)
    for bi, j in enumerate(this_ind_batch):
        gd += orc.apply_rotation_adjoint(gd_rot[bi], coord_ls[j])
        gb += orc.apply_rotation_adjoint(gb_rot[bi], coord_ls[j])
    return loss, gd, gb, d
