"""Float64 numpy restatement of bdof_shell_correlation (include/bdof.h; csrc/bdof_shells.h) for the tests: two separate real
transforms per volume and the integer shell rule, written from the header's text and sharing no code with the product.

Volumes here are arrays of any axis order (the shell rule is symmetric in the axes); axes of length 1 are ignored."""
import math

import numpy as np

# (X, Z, Y) of the device tests: a power of two twice; axes whose L / N_i differ, with spectrum points exactly on a shell boundary;
# radix 3, 5, 7; odd lengths; rings
SHAPES = [(8, 8, 8), (32, 32, 32), (16, 12, 20), (18, 10, 14), (15, 9, 21), (24, 1, 16)]


def geometry(shape):
    """(Nref, L, w) of a shape: shortest and least common multiple of the axes longer than 1, w = L / Nref."""
    axes = [int(n) for n in shape if int(n) > 1]
    assert len(axes) >= 2
    L = 1
    for n in axes:
        L = L * n // math.gcd(L, n)
    return min(axes), L, L // min(axes)


def signed_index(n):
    j = np.arange(n, dtype=np.int64)
    return np.where(j < (n + 1) // 2, j, j - n)


def u_grid(shape):
    """u = 4 sum (k_i L / N_i)^2 on the transform's grid, int64."""
    _, L, _ = geometry(shape)
    u = np.zeros(shape, dtype=np.int64)
    for ax, n in enumerate(shape):
        k = signed_index(n) * (L // n if n > 1 else 0)
        u = u + 4 * (k * k).reshape([-1 if i == ax else 1 for i in range(len(shape))])
    return u


def _isqrt(q):
    m = np.sqrt(q.astype(np.float64)).astype(np.int64)
    m = np.where(m * m > q, m - 1, m)
    return np.where((m + 1) * (m + 1) <= q, m + 1, m)


def shell_grid(shape):
    """The shell of every point: the integer s with (2s - 1)^2 w^2 <= u < (2s + 1)^2 w^2, i.e. with m = floor(sqrt(u) / w) =
    isqrt(u // w^2) the largest s with 2s - 1 <= m."""
    _, _, w = geometry(shape)
    s = (_isqrt(u_grid(shape) // (w * w)) + 1) // 2
    u = u_grid(shape)
    assert np.all((2 * s + 1) ** 2 * w * w > u) and np.all(((2 * s - 1) ** 2 * w * w <= u) | (s == 0))
    return s


def rho_grid(shape):
    """rho = Nref |f| in floating point, f in cycles per voxel."""
    nref, _, _ = geometry(shape)
    f2 = np.zeros(shape)
    for ax, n in enumerate(shape):
        f = signed_index(n) / float(n) if n > 1 else np.zeros(1)
        f2 = f2 + (f * f).reshape([-1 if i == ax else 1 for i in range(len(shape))])
    return nref * np.sqrt(f2)


def n_shells_all(shape):
    return int(shell_grid(shape).max()) + 1


def spectra(delta, beta):
    """(F_delta, F_beta): two separate transforms of the real channels."""
    return np.fft.fftn(np.asarray(delta, dtype=np.float64)), np.fft.fftn(np.asarray(beta, dtype=np.float64))


def spectra_packed(delta, beta):
    """The same from ONE complex transform C = F (delta + i beta): (C(k) + conj C(-k)) / 2 and (C(k) - conj C(-k)) / (2i)."""
    C = np.fft.fftn(np.asarray(delta, dtype=np.float64) + 1j * np.asarray(beta, dtype=np.float64))
    Cm = C
    for ax in range(C.ndim):
        Cm = np.roll(np.flip(Cm, axis=ax), 1, axis=ax)              # C(-k)
    return (C + np.conj(Cm)) / 2, (C - np.conj(Cm)) / 2j


def shell_sums(a, b, n_shells=None):
    """[n_shells][7] of two (delta, beta) pairs: n_points; sum Re(Fa conj Fb), sum |Fa|^2, sum |Fb|^2 of delta; the same of beta.
    Points of a shell >= n_shells are dropped."""
    shape = np.shape(a[0])
    s = shell_grid(shape).ravel()
    if n_shells is None:
        n_shells = int(s.max()) + 1
    keep = s < n_shells
    out = np.zeros((n_shells, 7))
    out[:, 0] = np.bincount(s[keep], minlength=n_shells)
    for j, (fa, fb) in enumerate(zip(spectra(*a), spectra(*b))):
        for i, term in enumerate(((fa * np.conj(fb)).real, np.abs(fa) ** 2, np.abs(fb) ** 2)):
            out[:, 1 + 3 * j + i] = np.bincount(s[keep], weights=term.ravel()[keep], minlength=n_shells)
    return out


def curves(sums):
    """(fsc_delta, fsc_beta): cross / sqrt(P_a P_b) where the product is positive, else 0 — no division is made elsewhere."""
    out = []
    for j in (1, 4):
        den = sums[:, j + 1] * sums[:, j + 2]
        c = np.zeros(len(sums))
        ok = den > 0
        c[ok] = sums[ok, j] / np.sqrt(den[ok])
        out.append(c)
    return out
