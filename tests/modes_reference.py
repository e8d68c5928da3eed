"""Float64 reference of the probe modes (bdof_set_probe_modes, include/bdof.h) — numpy, test side, built on
tests/reference_model.py.

M modes P_0 .. P_{M-1} (complex (M, Y, X)) on B objects (windows), the recorded intensity their incoherent sum:

    d_m  = reference_model.forward under probe P_m                    (M, B, Y, X)
    a    = sqrt(sum_m |d_m|^2)                                        (B, Y, X)
    L    = term(a, meas)[0]                                           the data term on the amplitude a: its mean runs over the
                                                                      B Y X measured pixels, not times M
    f    = term(a, meas)[1] / a        (0 where a == 0)               the data term's one factor per pixel, G(a) = f a
    G(d_m) = f d_m

`term` is any data term of reference_model.loss_and_grad — reference_model.lsq, or poisson_reference's and weights_reference's
through reference_model.data_term — handed the real amplitude a as its detector wave.  The adjoint sweep is
reference_model.loss_and_grad's, once per mode, with a `term` closure that hands back (L, f d_m); the volume gradients are the
sums over the modes, the gradient w.r.t. mode m is the sum over the objects of that sweep's G(psi_0)."""
import numpy as np

import reference_model as ref_model


def forward(delta, beta, modes, energy_ev, psize_cm, free_prop_cm=None, variant='numpy_skip_last'):
    """The detector waves of every (mode, object), (M, B, Y, X)."""
    return np.stack([ref_model.forward(delta, beta, p.real, p.imag, energy_ev, psize_cm, free_prop_cm, variant)[0] for p in np.asarray(modes)])


def amplitude(d):
    return np.sqrt(np.sum(np.abs(d) ** 2, axis=0))


def shared_factor(a, meas_abs, term=ref_model.lsq):
    """(loss, f): the data term on the mode-summed amplitude a and its per-pixel factor, G(d_m) = f d_m."""
    loss, g = term(a.astype(np.complex128), meas_abs)
    with np.errstate(divide='ignore', invalid='ignore'):
        f = np.where(a > 0, np.real(g) / np.where(a > 0, a, 1.0), 0.0)
    return float(loss), f


def loss_only(delta, beta, modes, energy_ev, psize_cm, meas_abs, free_prop_cm=None, variant='numpy_skip_last', term=ref_model.lsq):
    d = forward(delta, beta, modes, energy_ev, psize_cm, free_prop_cm, variant)
    return shared_factor(amplitude(d), meas_abs, term)[0]


def loss_and_grad(delta, beta, modes, energy_ev, psize_cm, meas_abs, free_prop_cm=None, variant='numpy_skip_last', term=ref_model.lsq):
    """(loss, g_delta [B, Y, X, S], g_beta, g_modes [M, Y, X] complex = dL/dRe P_m + i dL/dIm P_m, detector waves [M, B, Y, X])."""
    modes = np.asarray(modes)
    d = forward(delta, beta, modes, energy_ev, psize_cm, free_prop_cm, variant)
    loss, f = shared_factor(amplitude(d), meas_abs, term)
    g_delta, g_beta, g_modes = np.zeros(delta.shape), np.zeros(delta.shape), []
    for m, p in enumerate(modes):
        _, gd, gb, g0, dm = ref_model.loss_and_grad(delta, beta, p.real, p.imag, energy_ev, psize_cm, meas_abs, free_prop_cm, variant,
                                                    term=lambda dd, _meas: (loss, f * dd))
        assert np.array_equal(dm, d[m])
        g_delta += gd
        g_beta += gb
        g_modes.append(g0.sum(axis=0))
    return loss, g_delta, g_beta, np.array(g_modes), d
