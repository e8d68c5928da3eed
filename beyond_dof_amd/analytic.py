"""Host side of the analytic starting volume for full field (DESIGN §3 "Analytic start"; device side: csrc/bdof_fbp.h):
contrast-transfer-function (CTF) retrieval of the projected absorption from the detector planes, a real-space Ram-Lak filter and a
back-projection through the rigid maps the run rotates with.  Everything here is float64 numpy; the device takes the filters, the
rows of the maps and the angle weights that these functions build.

The model, in the project's sign convention (a slice modulates with exp(i k (delta + i beta) dz), a free-space step multiplies the
spectrum by exp(-i pi lambda z f^2)): to first order in the projected B = int beta dz and r B = int delta dz of a homogeneous
object (delta = r beta), the intensity of a unit plane wave a distance z behind the object's mid-plane has the contrast
    g^ = I^ - delta_0 = 2k (r sin chi - cos chi) B^,      chi = pi lambda z f^2
(the sine term has the sign opposite to the textbook's, whose modulation is exp(-i k delta dz)).  The forward model's transfer
function sits on the reference's inclusive-linspace mesh, not on the periodic transform's own frequencies (model_mesh), and at
holographic distances chi runs through many turns inside the band: the retrieval inverts the transfer of THAT model
(ctf_transfer), or the start would not be one for the optimiser that refines it."""
import os

import numpy as np

from . import tiffio, util

OBJECT_TYPES = ('normal', 'phase_only', 'absorption_only')


def _distances_nm(free_prop_cm, depth, psize_nm):
    """z_d of every detector plane: its distance from the object's exit plane plus half the object's depth"""
    free_prop_cm, planes = util.detector_distances(free_prop_cm)
    if isinstance(free_prop_cm, str):
        raise ValueError("the analytic start inverts near-field contrast: free_prop_cm='inf' (far field) has none")
    dist = [0.0] if free_prop_cm is None else [float(free_prop_cm)] if planes is None else list(planes)
    return [d * 1e7 + 0.5 * depth * psize_nm for d in dist]


def model_mesh(n, psize_nm):
    """The frequency the forward model's transfer function carries at FFT index j of an n-point axis: util.get_kernel puts H on
    the inclusive linspace(-1 / (2 psize), 1 / (2 psize), n), centred (the reference's mesh), so the step between
    bins is n / (n - 1) of the periodic transform's and, for even n, bin 0 sits half a step above zero: H(-f) != H(f) there."""
    return np.fft.ifftshift(np.linspace(-1. / (2. * psize_nm), 1. / (2. * psize_nm), int(n)))


def ctf_transfer(nx, ny, energy_ev, psize_cm, free_prop_cm, depth, delta_beta_ratio=10., ctf_regularization=1e-2, object_type='normal'):
    """(C, reg): C (D, nx, ny) complex128, the transfer C_d of the projected quantity B (in nm) to the contrast of plane d in the
    un-shifted index order of a frame's transform [kx][ky], and the regulariser of the inversion
        B^ = sum_d conj(C_d) g^_d / (sum_d |C_d|^2 + reg),     reg = ctf_regularization D (2k)^2 (1 + r^2)
    — ctf_regularization relative to the largest value |C_d|^2 can take, which for the two restricted object types is (2k)^2
    (there 1 stands in place of 1 + r^2).  The transfer is that of the forward model the run fits with: with H_d the model's
    multiplier exp(-i pi lambda z_d (u^2 + v^2)) on ITS mesh (model_mesh) divided by its value at bin 0 (the phase the unscattered
    wave picks up: on an even axis bin 0 is not zero frequency), H+ = H_d at a bin and H- = H_d at the mirrored bin,
        'normal'          C = k (i r (H+ - conj H-) - (H+ + conj H-)),   B the projected beta
        'phase_only'      C = i k (H+ - conj H-),                        B the projected delta
        'absorption_only' C = -k (H+ + conj H-),                         B the projected beta
    which on a symmetric mesh (H- = H+ = exp(-i chi)) are the real 2k (r sin chi - cos chi), 2k sin chi and -2k cos chi.
    depth: voxels along the beam."""
    if object_type not in OBJECT_TYPES:
        raise ValueError('object_type must be one of {}'.format(OBJECT_TYPES))
    psize_nm = float(psize_cm) * 1e7
    lmbda_nm = 1240. / energy_ev
    k = 2 * np.pi / lmbda_nm
    r = float(delta_beta_ratio)
    f2 = model_mesh(nx, psize_nm)[:, None] ** 2 + model_mesh(ny, psize_nm)[None, :] ** 2
    mirror = np.ix_((-np.arange(int(nx))) % int(nx), (-np.arange(int(ny))) % int(ny))
    C = []
    for z in _distances_nm(free_prop_cm, depth, psize_nm):
        Hp = np.exp(-1j * np.pi * lmbda_nm * z * (f2 - f2[0, 0]))        # relative to the unscattered wave, which rides on bin 0
        Hm = np.conj(Hp[mirror])
        C.append(k * {'normal': 1j * r * (Hp - Hm) - (Hp + Hm), 'phase_only': 1j * (Hp - Hm), 'absorption_only': -(Hp + Hm)}[object_type])
    C = np.stack(C)
    reg = float(ctf_regularization) * len(C) * (2 * k) ** 2 * (1 + r * r if object_type == 'normal' else 1.)
    return C, reg


def ctf_filters(nx, ny, *args, **kwargs):
    """The filters bdof_ctf_retrieve takes: complex128 (D, nx, ny), G_d = conj(C_d) / (sum |C|^2 + reg) / (nx ny) (ctf_transfer's arguments)."""
    C, reg = ctf_transfer(nx, ny, *args, **kwargs)
    return np.ascontiguousarray((np.conj(C) / ((np.abs(C) ** 2).sum(axis=0) + reg) / (int(nx) * int(ny))).astype(np.complex128))


def ramp_taps(n):
    """The exact real-space Ram-Lak taps h[m], m = -(n - 1) .. n - 1 (index m + n - 1): 1/4, -1 / (pi^2 m^2) for odd m, 0 for the
    other even m — the inverse transform of |f| on |f| <= 1/2 at unit spacing."""
    m = np.arange(-(int(n) - 1), int(n))
    h = np.zeros(len(m))
    h[m == 0] = 0.25
    odd = m % 2 != 0
    h[odd] = -1.0 / (np.pi ** 2 * (m[odd].astype(np.float64) ** 2))
    return h


def angle_weights(theta):
    """The quadrature weights of the back-projection: trapezoid weights of |theta_i| (in their sorted order) times
    pi / max(span, pi).  Full turns are folded onto the half turn a parallel beam needs (2 pi inclusive sums to pi, and its doubled
    end angle halves itself), less than pi of coverage is not inflated (the weights then sum to the span)."""
    th = np.abs(np.atleast_1d(np.asarray(theta, dtype=np.float64)))
    if len(th) < 2:
        return np.full(len(th), np.pi)
    order = np.argsort(th, kind='stable')
    s = th[order]
    d = np.diff(s)
    w = np.empty(len(s))
    w[0], w[-1] = d[0] / 2, d[-1] / 2
    w[1:-1] = (d[:-1] + d[1:]) / 2
    out = np.empty(len(s))
    out[order] = w * (np.pi / max(s[-1] - s[0], np.pi))
    return out


def rotation_rows(rotation, n_theta, shape, theta=None, axis_tilt=0., axis_roll=0., center=None, rotation_matrices=None, shifts=None):
    """(rows, angles): the (n_theta, 12) float64 rows of the rigid map (M | t) per angle that each rotation kind samples the volume
    (Y, X, Z) = shape through — beam-frame voxel o = (x, z, y) reads the volume at p = M o + t — and the angle of each for
    angle_weights.
      'trilinear': util.rigid_prm of the keywords, rotation_matrices, tilt, roll, centre and shifts included (under
                   rotation_matrices without theta the angle is read off M's first row);
      'bilinear':  util.rigid_geometry(theta, shape), whose M0 is that rotation's own map;
      'nearest':   the continuous map the lookup tables round.  util.rotation_lookup takes the angles linspace(0, 2 pi, n_theta)
                   whatever theta_st / theta_end say, turns in the opposite sense of M0 (x' = cos x - sin z, z' = sin x + cos z) and
                   about the centres floor(n / 2), so these rows are built explicitly here: theta is ignored."""
    n_theta = int(n_theta)
    if rotation == 'trilinear':
        rows = util.rigid_prm(n_theta, shape, theta, axis_tilt, axis_roll, center, rotation_matrices, shifts)
        if theta is None or rotation_matrices is not None and len(np.atleast_1d(theta)) != n_theta:
            theta = np.unwrap(np.arctan2(rows[:, 1], rows[:, 0]))
        return rows, np.asarray(theta, dtype=np.float64)
    if rotation == 'bilinear':
        if theta is None or len(np.atleast_1d(theta)) != n_theta:
            raise ValueError("rotation='bilinear' needs the n_theta projection angles theta")
        return util.rigid_geometry(theta, shape), np.asarray(theta, dtype=np.float64)
    if rotation == 'nearest':
        ny, nx, nz = [int(a) for a in shape]
        c = np.array([np.floor(nx / 2), np.floor(nz / 2), 0.])
        angles = np.linspace(0, 2 * np.pi, n_theta)
        rows = np.empty((n_theta, 3, 4))
        for i, a in enumerate(angles):
            M = np.array([[np.cos(a), -np.sin(a), 0.], [np.sin(a), np.cos(a), 0.], [0., 0., 1.]])
            rows[i, :, :3] = M
            rows[i, :, 3] = c - M @ c
        return rows.reshape(n_theta, 12), angles
    raise ValueError("rotation must be 'nearest', 'bilinear' or 'trilinear'")


def check_analytic(propagator='fft', probe_real=None, probe_imag=None, delta_beta_ratio=10., ctf_regularization=1e-2, object_type='normal',
                   free_prop_cm=None):
    """The host-side refusals of the analytic start (ValueError), before anything runs; returns |a0|^2 of the plane-wave probe.
    propagator='conv' has no reason to carry it; the contrast m^2 / |a0|^2 - 1 assumes a plane wave, so a probe that is not one
    scalar a0 != 0 over the whole frame (a localised probe, an optimisable one that has moved off its carrier) raises; so do a
    negative delta_beta_ratio, a ctf_regularization <= 0, an unknown object_type and the far field."""
    if propagator != 'fft':
        raise ValueError("the analytic start runs with the transfer-function propagator (propagator='fft') only")
    if object_type not in OBJECT_TYPES:
        raise ValueError('object_type must be one of {}'.format(OBJECT_TYPES))
    if not np.isfinite(delta_beta_ratio) or delta_beta_ratio < 0:
        raise ValueError('delta_beta_ratio must be finite and >= 0, not {}'.format(delta_beta_ratio))
    if not np.isfinite(ctf_regularization) or ctf_regularization <= 0:
        raise ValueError('ctf_regularization must be finite and > 0, not {}'.format(ctf_regularization))
    _distances_nm(free_prop_cm, 1, 1.)
    if probe_real is None:
        return 1.0
    probe = np.asarray(probe_real, dtype=np.float64) + 1j * (0. if probe_imag is None else np.asarray(probe_imag, dtype=np.float64))
    a0 = complex(np.mean(probe))
    if probe.ndim > 2 or not np.all(np.isfinite(probe)) or abs(a0) == 0 or np.max(np.abs(probe - a0)) > 1e-6 * abs(a0):
        raise ValueError('the analytic start assumes a plane-wave probe (one scalar a0 over the frame): this probe is not one')
    return abs(a0) ** 2


def _blur(a, sigma):
    """scipy.ndimage.gaussian_filter(a, sigma, mode='constant') of a 3-D array: truncated at 4 sigma, zero outside"""
    radius = int(4.0 * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1)
    g = np.exp(-0.5 * (x / float(sigma)) ** 2)
    g /= g.sum()
    for axis in range(a.ndim):
        pad = [(radius, radius) if i == axis else (0, 0) for i in range(a.ndim)]
        p = np.pad(a, pad)
        n = a.shape[axis]
        a = sum(g[j] * np.take(p, np.arange(j, j + n), axis=axis) for j in range(len(g)))
    return a


def support_mask(delta, threshold, sigma=1, save_path=None):
    """The finite-support mask of tensorflow_recon/coarse_phase_retrival_and_recon.py:42-47 from a coarse delta (Y, X, Z):
    |delta| blurred with a Gaussian of `sigma` voxels (zero outside), 1 where it exceeds `threshold`, 0 outside the cylinder of
    0.9 of the half width about the rotation axis (tomopy.circ_mask(mask, 0, ratio=0.9)).  float32 (Y, X, Z).  save_path: written
    as <save_path>/fin_sup_mask/mask_00000.tiff ..., where reconstruct_fullfield looks for it."""
    rec = _blur(np.abs(np.asarray(delta, dtype=np.float64)), sigma)
    mask = (rec > threshold).astype(np.float32)
    _, dx, dz = mask.shape
    rad1, rad2 = dx / 2., dz / 2.
    r2 = min(rad1, rad2) ** 2
    x = (np.arange(dx) + 0.5 - rad1)[:, None]
    z = (np.arange(dz) + 0.5 - rad2)[None, :]
    mask *= (x * x + z * z < 0.9 * 0.9 * r2).astype(np.float32)
    if save_path is not None:
        tiffio.write_tiff_stack(mask, os.path.join(save_path, 'fin_sup_mask', 'mask'), dtype='float32', overwrite=True)
    return mask
