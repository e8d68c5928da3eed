"""The float64 reference model of the tests — numpy, test side: the multislice model with every option the library carries,
each part written once.  The propagation kernel (get_kernel), the step (_propagate), the rotation functions and the window
arithmetic are oracle/bdof_oracle.py's own; what is restated here is what the oracle fixes: one step per voxel slice, one
detector plane and the least-squares seed.

Slice binning (include/bdof.h, bdof_set_slice_binning).  With S the voxel depth, S % b == 0, n = S / b, for step i = 0 .. n-1

    c_i     = exp(i k sum_j delta[..., i b + j]) exp(-k sum_j beta[..., i b + j]),  j < b,   k = 2 PI dz / lambda (per voxel)
    phi_i   = c_i psi_i
    psi_i+1 = P_b phi_i,   P_b the transfer-function step of get_kernel(b dz, ...)      (i < n-1, or every i under 'tf_all')

and every voxel slice of a bin receives the bin's one gradient row, g_delta[..., i b + j] = k Im(conj(phi_i) G(phi_i)),
g_beta[..., i b + j] = -k Re(conj(phi_i) G(phi_i)), G(psi_i) = conj(c_i) G(phi_i).  b = 1 is the oracle's model, operation
for operation.

The detector stage (bdof_set_detector_planes).  With psi the wave behind the last step, free_prop_cm is None (d = psi), 'inf'
(d = fftshift(F psi)), one distance z in cm (d = P(z) psi), or a sequence of D distances z_0 .. z_{D-1}:

    d_j    = P(z_j) psi                               detector waves (B, D, Y, X), in the order of the distances
    G(psi) = sum_j P(z_j)^H G(d_j)

and a sequence of one gives the numbers of its scalar exactly.

The data term is an argument, (d, meas_abs) -> (loss, G(d)) with G(d) = dL/dRe d + i dL/dIm d over all pixels of d: `lsq` here,
mean((|d| - m)^2), as multislice_loss_and_grad forms it; poisson_reference.py's and weights_reference.py's through `data_term`
(a (Y, X) weight plane broadcasts over wavefields and planes).

Two kinds of test data: `measurement_wide` here (amplitudes spread over [0, 2 |ref|]: the tight gradient bound of
tests/gradient_cases.py) beside the 5 % noise of the other files.  `AdjointHook` lets a test put one defect into the adjoint
sweep of loss_and_grad (tests/test_gradient_conditioning.py); without one the sweep is the model above.
"""
import numpy as np

from oracle import bdof_oracle as orc


def setup(B=2, Y=16, X=16, S=6, seed=0):
    """The random object and structured probe of the test_*_reference.py files: (delta, beta, probe_real, probe_imag, rng)."""
    rng = np.random.default_rng(seed)
    delta = rng.uniform(0, 2e-3, size=(B, Y, X, S))
    beta = rng.uniform(0, 2e-4, size=(B, Y, X, S))
    pr = 1 + 0.1 * rng.normal(size=(Y, X))
    pi = 0.1 * rng.normal(size=(Y, X))
    return delta, beta, pr, pi, rng


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def lsq(d, meas_abs):
    absd = np.abs(d)
    resid = absd - meas_abs
    with np.errstate(divide='ignore', invalid='ignore'):
        unit = np.where(absd > 0, d / absd, 0)
    return np.mean(resid ** 2), 2.0 * resid * unit / d.size


def data_term(loss, seed, *args):
    """(d, meas_abs) -> (loss, G(d)) of a module's pair of functions, e.g. data_term(pref.poisson_loss, pref.poisson_seed, mu)."""
    return lambda d, meas_abs: (loss(d, meas_abs, *args), seed(d, meas_abs, *args))


def measurement_wide(ref_wave, seed=0):
    """Amplitudes m = |ref| U(0, 2) per pixel for a float64 detector wave `ref` (a generator of its own stream, deterministic).

    Why not m = |ref| (1 + 0.05 N), the data of the other files.  The least-squares seed is G(d) = (2 / n) (1 - m / |d|) d and the
    object gradient is g_delta = k Im(conj(phi) G(phi)), g_beta = -k Re(conj(phi) G(phi)).  With 5 % data 1 - m / |d| is the
    difference of two float32 numbers that agree to 5 %, so a float32 engine's gradient error is its forward error divided by
    0.05: that quotient, not the adjoint kernels, sets the 2e-4 of tests/test_gpu_parity.py, and an adjoint mistake of 1e-4
    hides under it.

    Why not scaled data, m = s |ref| (s = 3, or m = 0).  Then 1 - m / |d| = 1 - s is ONE number, G(d) is proportional to d,
    the adjoint sweep carries it back to a multiple of phi (the sweep is the adjoint of a unitary step and of the modulation that
    made phi), and conj(phi) G(phi) is proportional to |phi|^2: real.  g_delta, its imaginary part, is left with what absorption
    breaks of that symmetry — 1.4e-5 of g_beta at a weak object, in float64 — which on a float32 device is all rounding: a relative
    bound on it says nothing (tests/test_gradient_conditioning.py::test_scaled_data_leaves_g_delta_empty).

    Only the pixel-to-pixel VARIATION of m / |d| feeds g_delta.  U(0, 2) makes that variation of order one: no cancellation in the
    seed (|1 - m / |d|| is 0.5 on average), g_delta and g_beta of the same size, and the same forward noise gives a gradient error
    7 to 9 times smaller than under the 5 % data.  The mean of m stays |ref|, so for a wave on a scalar carrier a0 the residual
    split of MultisliceEngine.choose_residual_split stays on: mean|m - |a0|| is about |a0| / 2, below mean(m)."""
    rng = np.random.default_rng([seed, 79])
    return np.abs(ref_wave) * rng.uniform(0, 2, size=np.shape(ref_wave))


class AdjointHook(object):
    """What loss_and_grad's adjoint sweep asks at each place a kernel could go wrong; this one answers as the model does.  A test
    subclasses it to restate ONE defect (step i counts propagation steps, 0 .. n-1; cs[i] is the bin's factor, phis[i] = cs[i] psi_i)."""

    def row_field(self, i, phis, cs):
        """The field whose conjugate multiplies G(phi_i) in the gradient row of step i."""
        return phis[i]

    def back_factor(self, i, cs):
        """G(psi_i) = back_factor G(phi_i)."""
        return np.conj(cs[i])

    def plane_terms(self, terms):
        """The list P(z_j)^H G(d_j) whose sum is G(psi) under several detector planes."""
        return terms


def _optics(shape, energy_ev, psize_cm, b, pi):
    """(voxel_nm, lmbda_nm, the kernel of a step of b voxel slices, k per voxel)."""
    B, Y, X, S = shape
    if b < 1 or S % b:
        raise ValueError('the slice binning must divide the depth')
    voxel_nm = np.array([psize_cm] * 3) * 1.e7
    lmbda_nm = 1240. / energy_ev
    delta_nm = voxel_nm[-1]
    h = orc.get_kernel(delta_nm * b, lmbda_nm, voxel_nm, (Y, X, S), pi=pi)
    k = 2. * pi * delta_nm / lmbda_nm
    return voxel_nm, lmbda_nm, h, k


def _sweep(delta, beta, probe_real, probe_imag, h, k, variant, b):
    """(psi behind the last step, [phi_i], [c_i], psi after every step)."""
    psi = np.zeros(delta.shape[:3], dtype=np.complex64)
    psi += (np.asarray(probe_real) + 1j * np.asarray(probe_imag))      # the forward model's complex64 start (np_funcs.py:20-21)
    n = delta.shape[-1] // b
    phis, cs, after = [], [], []
    for i in range(n):
        c = np.exp(1j * k * delta[..., i * b:(i + 1) * b].sum(axis=-1)) * np.exp(-k * beta[..., i * b:(i + 1) * b].sum(axis=-1))
        phi = psi * c
        phis.append(phi)
        cs.append(c)
        psi = orc._propagate(phi, h) if (i < n - 1 or variant == 'tf_all') else phi
        after.append(psi)
    return psi, phis, cs, after


def _planes(free_prop_cm):
    return isinstance(free_prop_cm, (list, tuple, np.ndarray))


def _detector(psi, free_prop_cm, lmbda_nm, voxel_nm, grid_shape, pi):
    """(detector wave(s), kernel(s) of the step to the detector)."""
    if free_prop_cm is None:
        return psi, None
    if _planes(free_prop_cm):
        if len(free_prop_cm) < 1:
            raise ValueError('at least one detector plane')
        hds = [orc.get_kernel(z * 1e7, lmbda_nm, voxel_nm, grid_shape, pi=pi) for z in free_prop_cm]
        return np.stack([orc._propagate(psi, hd) for hd in hds], axis=1), hds
    if free_prop_cm == 'inf':
        return np.fft.fftshift(np.fft.fft2(psi), axes=[1, 2]), None
    hd = orc.get_kernel(free_prop_cm * 1e7, lmbda_nm, voxel_nm, grid_shape, pi=pi)
    return orc._propagate(psi, hd), hd


def prop_adj(G, hh):
    return np.fft.ifft2(np.fft.ifftshift(np.fft.fftshift(np.fft.fft2(G), axes=[1, 2]) * np.conj(hh), axes=[1, 2]))


def forward(delta, beta, probe_real, probe_imag, energy_ev, psize_cm, free_prop_cm=None, variant='numpy_skip_last', b=1, pi=orc.PI):
    """(detector wave [B, Y, X] — [B, D, Y, X] for D distances —, wave after every step [n, B, Y, X]):
    multislice_propagate_batch_numpy with binning b and detector planes."""
    B, Y, X, S = delta.shape
    voxel_nm, lmbda_nm, h, k = _optics(delta.shape, energy_ev, psize_cm, b, pi)
    psi, _, _, after = _sweep(delta, beta, probe_real, probe_imag, h, k, variant, b)
    return _detector(psi, free_prop_cm, lmbda_nm, voxel_nm, (Y, X, S), pi)[0], np.array(after)


def loss_only(delta, beta, probe_real, probe_imag, energy_ev, psize_cm, meas_abs, free_prop_cm=None, variant='numpy_skip_last', b=1,
              term=lsq):
    d, _ = forward(delta, beta, probe_real, probe_imag, energy_ev, psize_cm, free_prop_cm, variant, b)
    return float(term(d, meas_abs)[0])


def loss_and_grad(delta, beta, probe_real, probe_imag, energy_ev, psize_cm, meas_abs, free_prop_cm=None, variant='numpy_skip_last',
                  b=1, pi=orc.PI, term=lsq, hook=None):
    """(loss, g_delta [B, Y, X, S], g_beta, g_probe [B, Y, X] complex = G(psi_0) per wavefield, detector wave(s)).
    meas_abs has the shape of the detector waves; term(d, meas_abs) -> (loss, G(d)) is the data term.  hook: an AdjointHook
    (test side: a defective adjoint sweep to measure a bound against); None is the model."""
    hook = hook or AdjointHook()
    B, Y, X, S = delta.shape
    voxel_nm, lmbda_nm, h, k = _optics(delta.shape, energy_ev, psize_cm, b, pi)
    psi, phis, cs, _ = _sweep(delta, beta, probe_real, probe_imag, h, k, variant, b)
    d, hd = _detector(psi, free_prop_cm, lmbda_nm, voxel_nm, (Y, X, S), pi)
    assert np.shape(meas_abs) == d.shape, (np.shape(meas_abs), d.shape)
    loss, G = term(d, meas_abs)
    if _planes(free_prop_cm):
        terms = hook.plane_terms([prop_adj(G[:, j], hd[j]) for j in range(len(hd))])
        G = terms[0]
        for t in terms[1:]:
            G = G + t
    elif free_prop_cm == 'inf':
        G = (Y * X) * np.fft.ifft2(np.fft.ifftshift(G, axes=[1, 2]))
    elif free_prop_cm is not None:
        G = prop_adj(G, hd)
    n = S // b
    g_delta, g_beta = np.zeros((B, Y, X, S)), np.zeros((B, Y, X, S))
    for i in range(n - 1, -1, -1):
        if i < n - 1 or variant == 'tf_all':
            G = prop_adj(G, h)
        t = np.conj(hook.row_field(i, phis, cs)) * G
        for j in range(b):                                  # the bin's one row to each of its voxel slices
            g_delta[..., i * b + j] = k * t.imag
            g_beta[..., i * b + j] = -k * t.real
        G = hook.back_factor(i, cs) * G
    return loss, g_delta, g_beta, G, d


# ---- compositions: orc.fullfield_loss_and_grad / orc.ptycho_loss_and_grad with this model in the middle -------------------------
def fullfield_loss_and_grad(obj_delta, obj_beta, coord_ls, this_ind_batch, this_prj_batch, probe_real, probe_imag, energy_ev,
                            psize_cm, free_prop_cm=None, variant='numpy_skip_last', b=1, term=lsq):
    """Rotate, loss and gradient, rotation adjoint; no regulariser (fullfield_loss_and_grad(with_reg=False)).  this_prj_batch:
    (n, Y, X), or (n, D, Y, X) for D distances.  Returns (loss, g_delta, g_beta, detector waves)."""
    obj_stack = np.stack([obj_delta, obj_beta], axis=3)
    rot = np.stack([orc.apply_rotation(obj_stack, coord_ls[j]) for j in this_ind_batch])
    loss, gd_rot, gb_rot, _, d = loss_and_grad(rot[..., 0], rot[..., 1], probe_real, probe_imag, energy_ev, psize_cm,
                                               np.abs(this_prj_batch), free_prop_cm, variant, b, term=term)
    gd, gb = np.zeros_like(obj_delta), np.zeros_like(obj_beta)
    for bi, j in enumerate(this_ind_batch):
        gd += orc.apply_rotation_adjoint(gd_rot[bi], coord_ls[j])
        gb += orc.apply_rotation_adjoint(gb_rot[bi], coord_ls[j])
    return loss, gd, gb, d


def ptycho_loss_and_grad(obj_delta, obj_beta, coord_old, probe_pos_all, this_pos_batch, this_prj_batch, probe_real, probe_imag,
                         probe_size, energy_ev, psize_cm, variant='numpy_skip_last', b=1, term=lsq):
    """Rotate, pad, cut the windows, far-field loss and gradient, scatter back, crop, rotation adjoint: (loss, g_delta, g_beta)
    with the gradients in the volume's frame."""
    obj_size = obj_delta.shape
    obj_rot = orc.apply_rotation(np.stack([obj_delta, obj_beta], axis=3), coord_old)
    pad, half = orc.ptycho_pad_amounts(probe_pos_all, probe_size, obj_size)
    obj_pad = np.pad(obj_rot, ((pad[0, 0], pad[0, 1]), (pad[1, 0], pad[1, 1]), (0, 0), (0, 0)), mode='constant')

    def window(pos):
        p0, p1 = int(pos[0]) + pad[0, 0] - half[0], int(pos[1]) + pad[1, 0] - half[1]
        return slice(p0, p0 + probe_size[0]), slice(p1, p1 + probe_size[1])

    subs = np.stack([obj_pad[window(pos)] for pos in this_pos_batch])
    loss, gd_sub, gb_sub, _, _ = loss_and_grad(subs[..., 0], subs[..., 1], probe_real, probe_imag, energy_ev, psize_cm,
                                               np.abs(this_prj_batch), 'inf', variant, b, term=term)
    g_pad = np.zeros(obj_pad.shape)
    for bi, pos in enumerate(this_pos_batch):
        w = window(pos)
        g_pad[w[0], w[1], :, 0] += gd_sub[bi]
        g_pad[w[0], w[1], :, 1] += gb_sub[bi]
    g_rot = g_pad[pad[0, 0]:pad[0, 0] + obj_size[0], pad[1, 0]:pad[1, 0] + obj_size[1]]
    g = orc.apply_rotation_adjoint(g_rot, coord_old)
    return loss, g[..., 0], g[..., 1]
