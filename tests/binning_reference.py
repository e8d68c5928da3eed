"""Float64 reference of slice binning (include/bdof.h, bdof_set_slice_binning) — numpy, test side.

oracle/bdof_oracle.py takes one Fresnel step per voxel slice.  This module restates the multislice model with one step per
b voxel slices and nothing else; the propagation kernel (get_kernel), the step (_propagate), the rotation functions and the
window arithmetic are the oracle's own.  With S the voxel depth, S % b == 0, n = S / b, for step i = 0 .. n-1

    c_i     = exp(i k sum_j delta[..., i b + j]) exp(-k sum_j beta[..., i b + j]),  j < b,   k = 2 PI dz / lambda (per voxel)
    phi_i   = c_i psi_i
    psi_i+1 = P_b phi_i,   P_b the transfer-function step of get_kernel(b dz, ...)      (i < n-1, or every i under 'tf_all')

and every voxel slice of a bin receives the bin's one gradient row, g_delta[..., i b + j] = k Im(conj(phi_i) G(phi_i)),
g_beta[..., i b + j] = -k Re(conj(phi_i) G(phi_i)), G(psi_i) = conj(c_i) G(phi_i).  b = 1 is the oracle's model, operation
for operation.
"""
import numpy as np

from oracle import bdof_oracle as orc


def _optics(shape, energy_ev, psize_cm, b, pi):
    B, Y, X, S = shape
    if b < 1 or S % b:
        raise ValueError('the slice binning must divide the depth')
    voxel_nm = np.array([psize_cm] * 3) * 1.e7
    lmbda_nm = 1240. / energy_ev
    delta_nm = voxel_nm[-1]
    h = orc.get_kernel(delta_nm * b, lmbda_nm, voxel_nm, (Y, X, S), pi=pi)
    k = 2. * pi * delta_nm / lmbda_nm
    return voxel_nm, lmbda_nm, h, k


def _bin_factor(delta, beta, k, i, b):
    return np.exp(1j * k * delta[..., i * b:(i + 1) * b].sum(axis=-1)) * np.exp(-k * beta[..., i * b:(i + 1) * b].sum(axis=-1))


def _start(shape, probe_real, probe_imag):
    psi = np.zeros(shape[:3], dtype=np.complex64)
    psi += (np.asarray(probe_real) + 1j * np.asarray(probe_imag))      # the forward model's complex64 start (np_funcs.py:20-21)
    return psi


def _detector(psi, free_prop_cm, lmbda_nm, voxel_nm, grid_shape, pi):
    if free_prop_cm is None:
        return psi, None
    if free_prop_cm == 'inf':
        return np.fft.fftshift(np.fft.fft2(psi), axes=[1, 2]), None
    hd = orc.get_kernel(free_prop_cm * 1e7, lmbda_nm, voxel_nm, grid_shape, pi=pi)
    return orc._propagate(psi, hd), hd


def forward(delta, beta, probe_real, probe_imag, energy_ev, psize_cm, free_prop_cm=None, variant='numpy_skip_last', b=1, pi=orc.PI):
    """(detector wave [B, Y, X], wave after every step [n, B, Y, X]) — multislice_propagate_batch_numpy with binning b."""
    B, Y, X, S = delta.shape
    voxel_nm, lmbda_nm, h, k = _optics(delta.shape, energy_ev, psize_cm, b, pi)
    n = S // b
    psi = _start(delta.shape, probe_real, probe_imag)
    after = []
    for i in range(n):
        psi = psi * _bin_factor(delta, beta, k, i, b)
        if i < n - 1 or variant == 'tf_all':
            psi = orc._propagate(psi, h)
        after.append(psi)
    d, _ = _detector(psi, free_prop_cm, lmbda_nm, voxel_nm, (Y, X, S), pi)
    return d, np.array(after)


def lsq_loss_and_seed(d, meas_abs):
    """mean((|d| - m)^2) and G(d) = dL/dRe d + i dL/dIm d, as multislice_loss_and_grad forms them."""
    absd = np.abs(d)
    resid = absd - meas_abs
    with np.errstate(divide='ignore', invalid='ignore'):
        unit = np.where(absd > 0, d / absd, 0)
    return np.mean(resid ** 2), 2.0 * resid * unit / d.size


def loss_and_grad(delta, beta, probe_real, probe_imag, energy_ev, psize_cm, meas_abs, free_prop_cm=None, variant='numpy_skip_last',
                  b=1, pi=orc.PI, loss_and_seed=lsq_loss_and_seed):
    """(loss, g_delta [B, Y, X, S], g_beta, g_probe [B, Y, X] complex = G(psi_0) per wavefield, detector wave).
    loss_and_seed(d, meas_abs) -> (loss, G(d)): the least-squares term by default, any other data term by argument."""
    B, Y, X, S = delta.shape
    voxel_nm, lmbda_nm, h, k = _optics(delta.shape, energy_ev, psize_cm, b, pi)
    n = S // b
    psi = _start(delta.shape, probe_real, probe_imag).astype(np.complex128)
    phis, cs = [], []
    for i in range(n):
        c = _bin_factor(delta, beta, k, i, b)
        phi = psi * c
        phis.append(phi)
        cs.append(c)
        psi = orc._propagate(phi, h) if (i < n - 1 or variant == 'tf_all') else phi
    d, hd = _detector(psi, free_prop_cm, lmbda_nm, voxel_nm, (Y, X, S), pi)
    loss, G = loss_and_seed(d, meas_abs)

    def prop_adj(G, hh):
        return np.fft.ifft2(np.fft.ifftshift(np.fft.fftshift(np.fft.fft2(G), axes=[1, 2]) * np.conj(hh), axes=[1, 2]))

    if free_prop_cm is None:
        pass
    elif free_prop_cm == 'inf':
        G = (Y * X) * np.fft.ifft2(np.fft.ifftshift(G, axes=[1, 2]))
    else:
        G = prop_adj(G, hd)
    g_delta, g_beta = np.zeros((B, Y, X, S)), np.zeros((B, Y, X, S))
    for i in range(n - 1, -1, -1):
        if i < n - 1 or variant == 'tf_all':
            G = prop_adj(G, h)
        t = np.conj(phis[i]) * G
        for j in range(b):                                  # the bin's one row to each of its voxel slices
            g_delta[..., i * b + j] = k * t.imag
            g_beta[..., i * b + j] = -k * t.real
        G = np.conj(cs[i]) * G
    return loss, g_delta, g_beta, G, d


def loss_only(delta, beta, probe_real, probe_imag, energy_ev, psize_cm, meas_abs, free_prop_cm=None, variant='numpy_skip_last', b=1):
    d, _ = forward(delta, beta, probe_real, probe_imag, energy_ev, psize_cm, free_prop_cm, variant, b)
    return float(np.mean((np.abs(d) - meas_abs) ** 2))


# ---- compositions: orc.fullfield_loss_and_grad / orc.ptycho_loss_and_grad with the binned model in the middle --------------------
def fullfield_loss_and_grad(obj_delta, obj_beta, coord_ls, this_ind_batch, this_prj_batch, probe_real, probe_imag, energy_ev,
                            psize_cm, free_prop_cm=None, variant='numpy_skip_last', b=1):
    """Rotate, binned loss and gradient, rotation adjoint; no regulariser (fullfield_loss_and_grad(with_reg=False))."""
    obj_stack = np.stack([obj_delta, obj_beta], axis=3)
    rot = np.stack([orc.apply_rotation(obj_stack, coord_ls[j]) for j in this_ind_batch])
    loss, gd_rot, gb_rot, _, _ = loss_and_grad(rot[..., 0], rot[..., 1], probe_real, probe_imag, energy_ev, psize_cm,
                                               np.abs(this_prj_batch), free_prop_cm, variant, b)
    gd, gb = np.zeros_like(obj_delta), np.zeros_like(obj_beta)
    for bi, j in enumerate(this_ind_batch):
        gd += orc.apply_rotation_adjoint(gd_rot[bi], coord_ls[j])
        gb += orc.apply_rotation_adjoint(gb_rot[bi], coord_ls[j])
    return loss, gd, gb


def ptycho_loss_and_grad(obj_delta, obj_beta, coord_old, probe_pos_all, this_pos_batch, this_prj_batch, probe_real, probe_imag,
                         probe_size, energy_ev, psize_cm, variant='numpy_skip_last', b=1):
    """Rotate, pad, cut the windows, binned far-field loss and gradient, scatter back, crop, rotation adjoint."""
    obj_size = obj_delta.shape
    obj_rot = orc.apply_rotation(np.stack([obj_delta, obj_beta], axis=3), coord_old)
    pad, half = orc.ptycho_pad_amounts(probe_pos_all, probe_size, obj_size)
    obj_pad = np.pad(obj_rot, ((pad[0, 0], pad[0, 1]), (pad[1, 0], pad[1, 1]), (0, 0), (0, 0)), mode='constant')

    def window(pos):
        p0, p1 = int(pos[0]) + pad[0, 0] - half[0], int(pos[1]) + pad[1, 0] - half[1]
        return slice(p0, p0 + probe_size[0]), slice(p1, p1 + probe_size[1])

    subs = np.stack([obj_pad[window(pos)] for pos in this_pos_batch])
    loss, gd_sub, gb_sub, _, _ = loss_and_grad(subs[..., 0], subs[..., 1], probe_real, probe_imag, energy_ev, psize_cm,
                                               np.abs(this_prj_batch), 'inf', variant, b)
    g_pad = np.zeros(obj_pad.shape)
    for bi, pos in enumerate(this_pos_batch):
        w = window(pos)
        g_pad[w[0], w[1], :, 0] += gd_sub[bi]
        g_pad[w[0], w[1], :, 1] += gb_sub[bi]
    g_rot = g_pad[pad[0, 0]:pad[0, 0] + obj_size[0], pad[1, 0]:pad[1, 0] + obj_size[1]]
    g = orc.apply_rotation_adjoint(g_rot, coord_old)
    return loss, g[..., 0], g[..., 1]
