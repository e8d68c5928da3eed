"""Mixed-state probe modes of ptychography (partial coherence, fly scans): the validation of the keywords (host side, ValueError
before anything is allocated), a starting set of modes from one probe, and the orthogonalisation of a set.

The recorded intensity is the incoherent sum I = sum_m |d_m|^2 over M orthogonal probe modes (Thibault & Menzel; Adorym's
n_probe_modes), the model of bdof_set_probe_modes (include/bdof.h).  Modes are complex arrays (M, py, px).

Gauge: a unitary mix P'_m = sum_n U_mn P_n of the modes leaves every intensity unchanged, so a fit only fixes the modes up to
such a mix; orthogonalize() picks the one whose Gram matrix is diagonal with descending powers — the coherent-mode decomposition."""
import numpy as np

MAX_MODES = 8       # BDOF_MAX_MODES


def check_probe_modes(n_modes, propagator='fft', slice_binning=1, adjoint_precision=None, engine=None):
    """The number of probe modes against what carries them: ValueError with the keyword's name.  Returns the number as an int."""
    if isinstance(n_modes, bool) or not isinstance(n_modes, (int, np.integer)) or not 1 <= n_modes <= MAX_MODES:
        raise ValueError('n_probe_modes must be an integer in [1, {}], not {!r}'.format(MAX_MODES, n_modes))
    if propagator == 'conv':
        raise ValueError("probe modes run with the transfer-function propagator: not together with propagator='conv'")
    if int(slice_binning) > 1:
        raise ValueError('probe modes run on the resident and generic engines, which take one step per voxel slice: not together with slice_binning > 1')
    if adjoint_precision not in (None, 'float32'):
        raise ValueError("probe modes run the float32 sweeps: not together with adjoint_precision={!r}".format(adjoint_precision))
    if engine == 'streaming':
        raise ValueError("probe modes run on the resident and generic engines: not together with engine='streaming'")
    return int(n_modes)


def as_modes(probe_real, probe_imag):
    """(probe_real, probe_imag) of shape (M, py, px) as one complex128 array, checked (ValueError)."""
    modes = np.asarray(probe_real, dtype=np.float64) + 1j * np.asarray(probe_imag, dtype=np.float64)
    if modes.ndim != 3:
        raise ValueError('probe modes are (M, py, px) arrays, not {}'.format(modes.shape))
    check_probe_modes(modes.shape[0])
    if not np.all(np.isfinite(modes)):
        raise ValueError('probe modes must be finite')
    return np.ascontiguousarray(modes)


_EXPONENTS = ((1, 0), (0, 1), (1, 1), (2, 0), (0, 2), (2, 1), (1, 2))      # x, y, xy, x^2, y^2, x^2 y, x y^2: MAX_MODES - 1 of them


def _monomials(shape, n):
    """The first n monomials of _EXPONENTS in the centred coordinates normalised to [-1, 1], (py, px) each."""
    py, px = shape
    y = (np.arange(py) - (py - 1) / 2.) / max((py - 1) / 2., 1.)
    x = (np.arange(px) - (px - 1) / 2.) / max((px - 1) / 2., 1.)
    y, x = np.meshgrid(y, x, indexing='ij')
    return [x ** i * y ** j for i, j in _EXPONENTS[:n]]


def mode_power(modes):
    """sum |P_m|^2 per mode, (M,)."""
    modes = np.asarray(modes)
    return np.sum(np.abs(modes) ** 2, axis=tuple(range(1, modes.ndim)))


def initial_modes(probe, n_modes, power=0.02):
    """M starting modes from one complex probe (py, px): mode 0 is the probe; mode k >= 1 the probe times the next monomial in the
    centred, normalised coordinates (x, y, xy, x^2, ...), made orthogonal to the earlier modes (Gram-Schmidt) and scaled to `power`
    of the probe's power; the whole set is then rescaled so that the total power is the probe's.  complex128 (M, py, px)."""
    n_modes = check_probe_modes(n_modes)
    probe = np.asarray(probe, dtype=np.complex128)
    if probe.ndim != 2:
        raise ValueError('initial_modes takes one (py, px) probe, not {}'.format(probe.shape))
    if not float(power) > 0:
        raise ValueError('probe_mode_power must be > 0')
    p0 = float(np.sum(np.abs(probe) ** 2))
    if not p0 > 0:
        raise ValueError('initial_modes needs a probe that is not zero')
    modes = [probe]
    for mono in _monomials(probe.shape, n_modes - 1):
        q = probe * mono
        for _ in range(2):                       # twice: the second pass removes what rounding left of the first
            for e in modes:
                q = q - e * (np.vdot(e, q) / np.vdot(e, e))
        modes.append(q * np.sqrt(float(power) * p0 / float(np.sum(np.abs(q) ** 2))))
    modes = np.array(modes)
    return modes / np.sqrt(1. + (n_modes - 1) * float(power))


def orthogonalize(modes):
    """The modes mixed by the eigenvectors of their M x M Gram matrix, in descending order of power: a unitary mix, so
    sum_m |P_m(r)|^2 is unchanged at every pixel, after which the modes are mutually orthogonal."""
    modes = np.asarray(modes, dtype=np.complex128)
    flat = modes.reshape(modes.shape[0], -1)
    gram = flat @ flat.conj().T                             # G_mn = <P_n, P_m>
    w, v = np.linalg.eigh(gram)                             # G = V diag(w) V^H
    order = np.argsort(w)[::-1]
    return (v[:, order].conj().T @ flat).reshape(modes.shape)


def relative_power(modes):
    p = mode_power(modes)
    return p / p.sum()


def summary_line(modes):
    """the probe_mode_power line of summary.txt: the modes' relative powers"""
    return '{:<20}{}\n'.format('probe_mode_power', ' '.join('{:.6g}'.format(v) for v in relative_power(modes)))
