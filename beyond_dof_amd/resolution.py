"""Fourier shell / ring correlation of two (delta, beta) volumes and the resolution it gives — what
tensorflow_recon/util.py:975-1048 (fourier_shell_correlation, fourier_ring_correlation; plot_fsc.py) computes on the host with one
mask volume per radius, here as one pass over the spectra on the device (bdof_shell_correlation, include/bdof.h).

Shells are hard: a point of spatial frequency f (cycles per voxel) lies in shell floor(Nref |f| + 1/2), Nref the shortest axis —
on a cube the rounded index radius, the centre line of the reference's blurred shell of that radius.  The curve is signed,
cross / sqrt(P_a P_b); the reference reports its absolute value.
"""
import collections
import ctypes
import math
import os

import numpy as np

from . import _lib, tiffio, util
from ._lib import DeviceBuffer

N_TERMS = 7        # per shell: n_points, then (cross, P_a, P_b) of delta and of beta

ShellRecord = collections.namedtuple('ShellRecord', 'shell frequency n_points fsc_delta fsc_beta sums nref psize_cm')
ShellRecord.__doc__ = """shell: 1 .. nref // 2 - 1 (the reference's arange(1, radius_max)); frequency: shell / nref, cycles per voxel;
n_points: spectrum points per shell; fsc_delta, fsc_beta: the two curves; sums: the raw (len(shell), 7) rows of
bdof_shell_correlation; nref: the shortest axis longer than 1; psize_cm: the voxel size, if it was given."""
Resolution = collections.namedtuple('Resolution', 'shell frequency half_period')

_ctx = None


def _default_ctx():
    global _ctx
    if _ctx is None:
        _ctx = _lib.Context(0)
    return _ctx


def reference_length(shape):
    """Nref of a volume shape: the shortest axis longer than 1."""
    axes = [int(n) for n in shape if int(n) > 1]
    if len(axes) < 2:
        raise ValueError('a shell correlation needs at least two axes longer than 1, not the shape {}'.format(tuple(shape)))
    return min(axes)


def shell_count(shape):
    """The number of shells that hold a point: 1 + the shell of the spectrum's corner, by the integer rule of include/bdof.h."""
    nref = reference_length(shape)
    axes = [int(n) for n in shape if int(n) > 1]
    lcm = 1
    for n in axes:
        lcm = lcm * n // math.gcd(lcm, n)
    w = lcm // nref
    u = 4 * sum(((n // 2) * (lcm // n)) ** 2 for n in axes)
    return (math.isqrt(u // (w * w)) + 1) // 2 + 1


def curves(sums):
    """(fsc_delta, fsc_beta) of rows of sums: cross / sqrt(P_a P_b) where that product is positive, else 0."""
    sums = np.asarray(sums, dtype=np.float64)
    out = []
    for j in (1, 4):
        den = sums[:, j + 1] * sums[:, j + 2]
        ok = den > 0
        out.append(np.where(ok, sums[:, j] / np.sqrt(np.where(ok, den, 1.0)), 0.0))
    return out[0], out[1]


def _rows(v):
    """A volume argument with its shape (X, Z, Y): a DeviceBuffer [X][Z][Y][2] as it is, a host (delta, beta) pair in the
    reference's (y, x, z) order as 3-D arrays (2-D: (y, x), one slice)."""
    if isinstance(v, DeviceBuffer):
        if len(v.shape) != 4 or v.shape[3] != 2 or v.dtype != np.float32:
            raise ValueError('a device volume is float32 rows [X][Z][Y][2], not {} {}'.format(v.dtype, v.shape))
        return v, tuple(v.shape[:3])
    delta, beta = (np.asarray(c) for c in v)
    if delta.shape != beta.shape or delta.ndim not in (2, 3):
        raise ValueError('a volume is a (delta, beta) pair of equal 2-D or 3-D arrays, not shapes {} and {}'.format(delta.shape, beta.shape))
    if delta.ndim == 2:
        delta, beta = delta[:, :, None], beta[:, :, None]
    y, x, z = delta.shape
    return (delta, beta), (x, z, y)


def shell_sums(a, b, n_shells=None, ctx=None):
    """The (n_shells, 7) sums of bdof_shell_correlation for two volumes (each a host (delta, beta) pair in (y, x, z) order, or a
    DeviceBuffer of rows); n_shells defaults to every shell up to the corner of the spectrum."""
    ra, shape_a = _rows(a)
    rb, shape_b = (ra, shape_a) if b is a else _rows(b)
    if shape_a != shape_b:
        raise ValueError('the two volumes differ in shape: (X, Z, Y) = {} and {}'.format(shape_a, shape_b))
    if n_shells is None:
        n_shells = shell_count(shape_a)
    if ctx is None:
        ctx = next((v.ctx for v in (ra, rb) if isinstance(v, DeviceBuffer)), None) or _default_ctx()
    da = ra if isinstance(ra, DeviceBuffer) else DeviceBuffer.from_host(ctx, util.volume_to_rows(*ra))
    db = da if rb is ra else rb if isinstance(rb, DeviceBuffer) else DeviceBuffer.from_host(ctx, util.volume_to_rows(*rb))
    out = np.zeros((max(int(n_shells), 0), N_TERMS), dtype=np.float64)
    ctx.check(ctx.lib.bdof_shell_correlation(ctx.handle, da.ptr, db.ptr, shape_a[0], shape_a[1], shape_a[2], int(n_shells),
                                             out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
    for buf, src in ((da, ra), (db, rb)):
        if buf is not src:
            buf.free()
    return out


def record_from_sums(sums, nref, psize_cm=None):
    """The ShellRecord of rows 0 .. nref // 2 - 1 of the sums (shell 0, the mean, is not reported)."""
    sums = np.asarray(sums, dtype=np.float64)[1:nref // 2]
    shell = np.arange(1, nref // 2)
    fd, fb = curves(sums)
    return ShellRecord(shell, shell / float(nref), sums[:, 0].astype(np.int64), fd, fb, sums, nref, psize_cm)


def fourier_shell_correlation(a, b, psize_cm=None, ctx=None):
    """Shell correlation of the volumes a and b: each a (delta, beta) pair of host arrays in the reference's (y, x, z) order, or a
    DeviceBuffer of rows [X][Z][Y][2].  Returns a ShellRecord; psize_cm, the voxel size, is kept in it for resolution()."""
    nref = reference_length(_rows(a)[1])
    return record_from_sums(shell_sums(a, b, nref // 2, ctx), nref, psize_cm)


def fourier_ring_correlation(a, b, psize_cm=None, ctx=None):
    """fourier_shell_correlation of 2-D arrays: a and b are (delta, beta) pairs of (y, x) images."""
    for v in (a, b):
        if not isinstance(v, DeviceBuffer) and np.ndim(v[0]) != 2:
            raise ValueError('a ring correlation takes 2-D arrays')
    return fourier_shell_correlation(a, b, psize_cm, ctx)


def threshold_curve(kind, n_points):
    """The threshold per shell: a number (0.5, 0.143) as it is, or 'half-bit', (0.2071 + 1.9102 / sqrt(n)) / (1.2071 + 0.9102 / sqrt(n))
    with n = n_points / 2 — a real volume's spectrum holds each value twice."""
    n_points = np.asarray(n_points, dtype=np.float64)
    if kind == 'half-bit':
        r = 1.0 / np.sqrt(np.maximum(n_points / 2.0, 1e-300))
        return (0.2071 + 1.9102 * r) / (1.2071 + 0.9102 * r)
    if isinstance(kind, str):
        raise ValueError("a threshold is a number or 'half-bit', not {!r}".format(kind))
    return np.full(n_points.shape, float(kind))


def _first_crossing(shell, fsc, thr, nref, psize):
    below = np.nonzero(fsc < thr)[0]
    if not len(below):
        return None
    i = int(below[0])
    s = float(shell[i])
    if i > 0:
        above, under = fsc[i - 1] - thr[i - 1], fsc[i] - thr[i]            # above >= 0 > under
        s = shell[i - 1] + (shell[i] - shell[i - 1]) * above / (above - under)
    return Resolution(s, s / nref, psize * nref / (2.0 * s))


def resolution(record, kind='half-bit', psize_cm=None):
    """Where each curve first falls below the threshold, linearly interpolated between the shells either side: a dict of
    'delta' and 'beta', each a Resolution (shell, frequency in cycles per voxel, half-period length psize_cm nref / (2 shell) —
    psize_cm defaults to the record's, and without either the length is in voxels) or None if the curve never crosses.  A curve already below at the first shell crosses there."""
    thr = threshold_curve(kind, record.n_points)
    psize_cm = record.psize_cm if psize_cm is None else psize_cm
    psize = 1.0 if psize_cm is None else float(psize_cm)
    return {name: _first_crossing(record.shell, np.asarray(fsc), thr, record.nref, psize)
            for name, fsc in (('delta', record.fsc_delta), ('beta', record.fsc_beta))}


# ---- fsc_reference= of the reconstruction entry points ------------------------------------------------------------------------
def _read_array(path):
    return np.load(path) if str(path).lower().endswith('.npy') else tiffio.read_tiff(path)


def read_reference(fsc_reference, shape):
    """fsc_reference as a (delta, beta) pair of arrays of `shape` (y, x, z): given as such, or as two .npy / TIFF paths."""
    if len(fsc_reference) != 2:
        raise ValueError('fsc_reference is a (delta, beta) pair of arrays or of .npy / TIFF paths')
    pair = tuple(np.asarray(_read_array(v) if isinstance(v, (str, os.PathLike)) else v) for v in fsc_reference)
    for v in pair:
        if tuple(v.shape) != tuple(shape):
            raise ValueError('fsc_reference has the shape {}, the final volume {}'.format(tuple(v.shape), tuple(shape)))
    return pair


def summary_lines(record, kind, psize_cm):
    """the resolution_delta / resolution_beta lines of summary.txt"""
    out = ''
    for name, r in sorted(resolution(record, kind, psize_cm).items(), reverse=True):
        text = 'no crossing of the {} threshold up to shell {}'.format(kind, int(record.shell[-1])) if r is None else \
            '{:.6g} cm half period (shell {:.4g}, {:.6g} cycles per voxel, {} threshold)'.format(r.half_period, r.shell, r.frequency, kind)
        out += '{:<20}{}\n'.format('resolution_' + name, text)
    return out


def write_report(record, output_folder, kind, psize_cm):
    """fsc.npy (a dict of the record's arrays) into the output folder, and the two resolution lines behind summary.txt"""
    np.save(os.path.join(output_folder, 'fsc.npy'), dict(record._asdict()))
    with open(os.path.join(output_folder, 'summary.txt'), 'a') as f:
        f.write(summary_lines(record, kind, psize_cm))
