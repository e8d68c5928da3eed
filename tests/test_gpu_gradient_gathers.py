"""The gathers that carry a gradient from the frame it was computed in (rotated rows, probe windows, tiles) back into the
[X][Z][Y] volume gradient (csrc/bdof_kernels.h, csrc/bdof_field.h), each through its own entry point against a numpy
restatement written here — the pattern of test_gpu_tile_ops.py.  The kernels are fed directly: the frame gradient is uploaded
into bdof_grot, the tables are built by util.device_rotation_tables from SYNTHETIC coordinate lists, so every list length a
kernel branches on is chosen here and asserted on the host before the launch.

Index kernels (rotation adjoint, window adjoint, tile gradient, tile cut^H with taper 0, field gather) are exact: all data are
integer-valued float32 in [-4, 4], every partial sum is an integer far below 2^24, so every summation order gives the same
float32 and the assertion is np.array_equal against an int64 / float64 restatement (np.add.at over the table); scale is one of
1, 0.5, 3 (exact), an accumulating call starts from integers.  Every output lies between sentinel-filled guards; rows outside
[row0, row0 + n_rows) and the guards must come back untouched, and no element is left out of any comparison.

The one tolerance is the bilinear pair's, derived per element, not measured.  Let the reference's taps of an element have
weights w_i (>= 0) and inputs g_i, n of them with w_i != 0.  The device forms each weight as a product of two float32 factors
in [0, 1], each the rounding of a float64 fraction (or of 1 - it): absolute error of a weight <= 4 * 2^-24.  It then adds n
fused products in float32 (each step rounds the running sum, <= 2^-24 of sum |w_i| |g_i| per step), applies `scale` and, when
accumulating, adds the prior value (one more rounding each, counted in the "+ 4").  Hence
    |device - reference| <= 2^-24 * (4 * sum |g_i|  +  (n + 4) * sum |w_i| |g_i|)   (+ 2^-24 |prior| when accumulating),
times `scale` (0.5 scales every term exactly).  Both sums are formed here from orc._bilinear_taps, next to the reference.
Where the bound is 0 (no tap) the device value must be 0 to within 1e-12 of the largest reference value."""
import ctypes

import numpy as np
import pytest

from oracle import bdof_oracle as orc

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
GUARD = 64                      # elements of sentinel before and after every output
ERR_SIZE = -3                   # BDOF_ERR_SIZE (include/bdof.h)
WIN_MAXLIST = TILE_MAXLIST = 1024
ROTADJ_MAXLIST = 256


def ints(rng, shape, dtype=np.float32):
    """integer-valued data in [-4, 4]"""
    return rng.integers(-4, 5, size=shape).astype(dtype)


def cints(rng, shape, dtype=np.complex64):
    return (rng.integers(-4, 5, size=shape) + 1j * rng.integers(-4, 5, size=shape)).astype(dtype)


# ================================================================================================================================
# The restatements (host only; tests/test_gradient_gather_restatements.py checks them against the oracle)
# ================================================================================================================================
def tables_from_dests(dests, nx, nz):
    """util.device_rotation_tables from synthetic coordinate lists: dests[a][z * nx + x] is the volume row (x' * nz + z') that
    rotated row (z, x) of angle a is gathered from."""
    from beyond_dof_amd import util
    coords = []
    for d in dests:
        c = np.asarray(d, dtype=np.int64).reshape(nz, nx).T.reshape(-1)         # the reference's lists are indexed x * nz + z
        coords.append(np.stack([c // nz, c % nz], axis=1))
    tab, off, order = util.device_rotation_tables(coords, nx, nz)
    assert all(np.array_equal(tab[a].reshape(-1), dests[a]) for a in range(len(dests)))
    return tab, off, order


def rot_adjoint_restated(grot, tab, angle_of_b):
    """grot [B][n_src][NY][2] (integers), tab [n_angles][S][NX] -> int64 [n_dest][NY][2]: the scatter-add over the table"""
    out = np.zeros(grot.shape[1:], dtype=np.int64)
    for b, a in enumerate(angle_of_b):
        np.add.at(out, tab[a].reshape(-1), grot[b].astype(np.int64))
    return out


def window_adjoint_restated(grot, tab_a, xoff, yoff, volNX, volNY):
    """grot [B][S][NX][NY][2], tab_a [S][volNX] of the batch's angle -> int64 [S * volNX][volNY][2]: overlap-add of the windows
    into the rotated frame (pixels outside the volume dropped), then the scatter-add over the table"""
    B, S, NX, NY = grot.shape[:4]
    pad = np.zeros((S, volNX, volNY, 2), dtype=np.int64)
    g = grot.astype(np.int64)
    for b in range(B):
        xs, ys = xoff[b] + np.arange(NX), yoff[b] + np.arange(NY)
        mx, my = (xs >= 0) & (xs < volNX), (ys >= 0) & (ys < volNY)
        np.add.at(pad, (slice(None), xs[mx][:, None], ys[my][None, :]), g[b][:, mx][:, :, my])
    out = np.zeros((S * volNX, volNY, 2), dtype=np.int64)
    np.add.at(out, tab_a.reshape(-1), pad.reshape(S * volNX, volNY, 2))
    return out


def tiles_grad_restated(grot, tab, x0, y0, z0, n_rows, volNY):
    """grot [B][nz][TX][TY][2], tab [S][volNX] -> int64 [n_rows][volNY][2]; tile pixels beyond the volume contribute nothing"""
    B, nz, TX, TY = grot.shape[:4]
    volNX = tab.shape[1]
    out = np.zeros((n_rows, volNY, 2), dtype=np.int64)
    g = grot.astype(np.int64)
    for b in range(B):
        xs, ys = x0[b] + np.arange(TX), y0[b] + np.arange(TY)
        mx, my = (xs >= 0) & (xs < volNX), (ys >= 0) & (ys < volNY)
        dest = tab[z0:z0 + nz][:, xs[mx]]                                                       # [nz][x inside]
        np.add.at(out, (dest[:, :, None], ys[my][None, None, :]), g[b][:, mx][:, :, my])
    return out


def cut_adjoint_restated(tiles, x0, y0, FX, FY):
    """taper 0: tiles [B][TX][TY] complex -> complex128 [FX][FY], periodic"""
    B, TX, TY = tiles.shape
    out = np.zeros((FX, FY), dtype=np.complex128)
    for b in range(B):
        np.add.at(out, (np.mod(x0[b] + np.arange(TX), FX)[:, None], np.mod(y0[b] + np.arange(TY), FY)[None, :]), tiles[b].astype(np.complex128))
    return out


def expected_rows(prior, rest, row0, n_rows, accumulate, scale):
    """What a *_rows call leaves in a destination that held `prior`: float64 (all values exact)"""
    out = prior.astype(np.float64).copy()
    new = scale * rest[row0:row0 + n_rows].astype(np.float64)
    out[row0:row0 + n_rows] = new + (out[row0:row0 + n_rows] if accumulate else 0.0)
    return out


# ---- bilinear: reference + per-element bound ----------------------------------------------------------------------------------
BILIN_ANGLES = np.array([0.3, np.pi / 2, -1.1, np.pi, 0.0, -np.pi / 2, 2.5, 2 * np.pi, 4.0]).astype(np.float32).astype(np.float64)
BILIN_NXV, BILIN_NZV = 7, 10


def bilinear_prm(theta, H, W):
    """the solver's own expression (util.bilinear_prm)"""
    th = np.asarray(theta, dtype=np.float64)
    c, sn = np.cos(th), np.sin(th)
    return np.stack([c, sn, ((W - 1) - (c * (W - 1) - sn * (H - 1))) / 2.0, ((H - 1) - (sn * (W - 1) + c * (H - 1))) / 2.0], axis=1)


def bilinear_tap_matrices(theta, H, W):
    """Aw[dest][src] = sum of the weights with which volume row dest = h2 * W + w2 feeds rotated row src = h * W + w, A1 the
    number of those taps with a non-zero weight: from orc._bilinear_taps"""
    Aw, A1 = np.zeros((H * W, H * W)), np.zeros((H * W, H * W))
    src = np.arange(H * W).reshape(H, W)
    for h2, w2, wt in orc._bilinear_taps(theta, H, W):
        np.add.at(Aw, (h2 * W + w2, src), wt)
        np.add.at(A1, (h2 * W + w2, src), (wt != 0).astype(np.float64))
    return Aw, A1


def bilinear_forward_reference(vol, thetas):
    """vol [H][W][NY][2] float32 -> reference and bound, both [B][W][H][NY][2] float64 (the device's row order [b][z][x])"""
    H, W, NY = vol.shape[:3]
    obj = vol.astype(np.float64).transpose(2, 0, 1, 3)                                         # (Y, X, Z, C)
    flat = np.abs(vol.astype(np.float64)).reshape(H * W, -1)
    ref, bound = [], []
    for th in thetas:
        ref.append(orc.rotate_bilinear(obj, th).transpose(2, 1, 0, 3))
        Aw, A1 = bilinear_tap_matrices(th, H, W)
        n = A1.sum(axis=0)[:, None]
        bd = 2.0 ** -24 * (4 * (A1.T @ flat) + (n + 4) * (Aw.T @ flat))
        bound.append(bd.reshape(H, W, NY, 2).transpose(1, 0, 2, 3))
    return np.stack(ref), np.stack(bound)


def bilinear_adjoint_terms(grot, thetas):
    """grot [B][W][H][NY][2] float32 -> per batch element: reference contribution, sum |g_i|, sum |w_i| |g_i| (each
    [H][W][NY][2]) and the tap count n [H * W]; a batch of the first B elements sums the first B of each"""
    B, W, H, NY = grot.shape[:4]
    terms = []
    for b, th in enumerate(thetas):
        g = grot[b].astype(np.float64)
        ref = orc.rotate_bilinear_adjoint(g.transpose(2, 1, 0, 3), th).transpose(1, 2, 0, 3)
        Aw, A1 = bilinear_tap_matrices(th, H, W)
        flat = np.abs(g).transpose(1, 0, 2, 3).reshape(H * W, -1)
        terms.append((ref, (A1 @ flat).reshape(H, W, NY, 2), (Aw @ flat).reshape(H, W, NY, 2), A1.sum(axis=1)))
    return terms


def bilinear_adjoint_reference(terms, B):
    ref = sum(t[0] for t in terms[:B])
    sg, swg, n = sum(t[1] for t in terms[:B]), sum(t[2] for t in terms[:B]), sum(t[3] for t in terms[:B])
    H, W = ref.shape[:2]
    return ref, 2.0 ** -24 * (4 * sg + (n.reshape(H, W, 1, 1) + 4) * swg)


def assert_within(dev, ref, bound, what):
    """|dev - ref| <= bound element by element; where the bound is 0 the device value is 0 to 1e-12 of the largest reference value"""
    err = np.abs(dev.astype(np.float64) - ref)
    tap = bound > 0
    worst = float((err[tap] / bound[tap]).max()) if tap.any() else 0.0
    print(what, 'largest |device - reference| / bound', worst, 'elements without a tap', int((~tap).sum()))
    assert worst <= 1.0, what
    assert np.all(err[~tap] <= 1e-12 * np.abs(ref).max()), what


# ================================================================================================================================
# The cases: geometry and data, with their preconditions asserted on the host (also run by the host-only test)
# ================================================================================================================================
def dests_from_counts(rng, n, special, n_angles):
    """per angle the destination row of each of the n rotated rows: special[d] = (count in angle 0, 1, ..), the other rows share
    what is left at random (short lists), the order of the sources is shuffled"""
    free = np.array([d for d in range(n) if d not in special])
    dests, counts = [], np.zeros((n_angles, n), dtype=np.int64)
    for a in range(n_angles):
        for d, c in special.items():
            counts[a, d] = c[a]
        counts[a, free] = rng.multinomial(n - counts[a].sum(), np.full(len(free), 1.0 / len(free)))
        dests.append(rng.permutation(np.repeat(np.arange(n), counts[a])).astype(np.int64))
    return dests, counts


def rot_case_main():
    """30 x 40 = 1200 rows, 3 angles, NY = 8.  Batch A = 3 elements (angles 2, 0, 1): rows with 0, 1, 7 (odd), exactly 256 (wave
    path) and 257 (heavy path) sources, and one where angle 0 alone brings 515 (two full 256-entry stages of the heavy kernel and
    a remainder that is no multiple of 4).  Batch B = 66 elements, angles repeated and unsorted (22 x 0, 21 x 1, 21 x 2 in the
    first 64, then 2, 2): rows 450..453 are built for the second chunk of 64."""
    rng = np.random.default_rng(21)
    nx, nz, ny = 30, 40, 8
    special = {0: (0, 0, 0), 7: (1, 0, 0), 301: (3, 2, 2), 602: (100, 100, 56), 1001: (100, 100, 57), 1199: (515, 1, 2),
               450: (0, 0, 12), 451: (1, 1, 3), 452: (0, 10, 2), 453: (1, 9, 2)}
    dests, counts = dests_from_counts(rng, nx * nz, special, 3)
    ang_a = np.array([2, 0, 1], dtype=np.int32)
    ang_b = np.concatenate([rng.permutation(np.repeat([0, 1, 2], [22, 21, 21])), [2, 2]]).astype(np.int32)
    tot_a = counts[ang_a].sum(axis=0)
    assert [int(tot_a[d]) for d in (0, 7, 301, 602, 1001)] == [0, 1, 7, 256, 257]
    assert counts[0, 1199] > 512 and counts[0, 1199] % 4 != 0 and counts[0, 1199] % 256 % 4 != 0
    first, full = counts[ang_b[:64]].sum(axis=0), counts[ang_b].sum(axis=0)
    assert len(ang_b) == 66 and not np.all(np.diff(ang_b) >= 0)
    assert 0 < first[450] <= ROTADJ_MAXLIST < full[450]          # the list is partly written, then the row is deferred
    assert first[453] <= ROTADJ_MAXLIST and full[453] == 257
    assert first[451] < full[451] <= ROTADJ_MAXLIST and first[452] < full[452] == ROTADJ_MAXLIST     # stay on the wave path over both chunks
    grot = ints(rng, (66, nx * nz, ny, 2))
    return dict(nx=nx, nz=nz, ny=ny, dests=dests, ang_a=ang_a, ang_b=ang_b, grot=grot, prior=ints(rng, (nx * nz, ny, 2)))


def rot_case_wide(ny):
    """10 x 12 = 120 rows, 3 angles, 5 elements (angles 0, 1, 0, 2, 1): rows with 0, 1, exactly 256 and 257 sources, for NY = 130 (a
    second column group with one lane) and NY = 516 (a second pass of 256 float4 columns, in the wave and in the heavy kernel)"""
    rng = np.random.default_rng(22)
    nx, nz = 10, 12
    special = {0: (0, 0, 0), 5: (0, 0, 1), 60: (50, 50, 56), 119: (50, 50, 57)}
    dests, counts = dests_from_counts(rng, nx * nz, special, 3)
    ang = np.array([0, 1, 0, 2, 1], dtype=np.int32)
    tot = counts[ang].sum(axis=0)
    assert [int(tot[d]) for d in (0, 5, 60, 119)] == [0, 1, 256, 257]
    assert ny // 2 > 64 and (ny != 516 or ny // 2 > 256)
    return dict(nx=nx, nz=nz, ny=ny, dests=dests, ang=ang, grot=ints(rng, (5, nx * nz, ny, 2)))


def rot_case_grid():
    """128 x 128 = 16384 rows of NY = 4, 2 angles, 2 elements: more rows than 4 x 2048 workgroups take in one pass (256 CUs x 8);
    every list is short"""
    rng = np.random.default_rng(23)
    nx = nz = 128
    dests = [rng.integers(0, nx * nz, size=nx * nz) for _ in range(2)]
    ang = np.array([1, 0], dtype=np.int32)
    tot = sum(np.bincount(d, minlength=nx * nz) for d in dests)
    assert nx * nz > 4 * 2048 and 1 < tot.max() <= 32 and tot.min() == 0
    return dict(nx=nx, nz=nz, ny=4, dests=dests, ang=ang, grot=ints(rng, (2, nx * nz, 4, 2)))


WINDOW_SHAPES = [(5, 7), (6, 4)]


def window_case(NX, NY):
    """volume (9, 11, 260), 2 angles, called with angle 1.  Windows NX x NY: origins negative, overhanging the high edge, fully
    outside, duplicated; on column 3.. stacks of 1, 4, 5 and 7 windows over one y (the unroll-by-4 loop and its tail).  S = 11:
    the last z chunk of 8 is short; volNY = 260: the y loop strides."""
    rng = np.random.default_rng(31)
    volNX, S, volNY = 9, 11, 260
    org = [(2, 150), (-2, -3), (7, 256), (-1, 258), (2, 200), (2, 200),                          # first one inside; edges; a duplicate
           (9, 10), (-NX, 0), (0, 260), (3, -NY),                                                 # fully outside
           (3, 20)] + [(3, 40)] * 4 + [(3, 60)] * 5 + [(3, 80)] * 3 + [(3, 81)] * 2 + [(3, 82), (3, 83)] + [(1, 120)]
    xoff, yoff = np.array([o[0] for o in org], dtype=np.int32), np.array([o[1] for o in org], dtype=np.int32)
    B = len(org)
    cover = np.zeros((volNX, volNY), dtype=np.int64)
    outside = 0
    for b in range(B):
        xs, ys = xoff[b] + np.arange(NX), yoff[b] + np.arange(NY)
        mx, my = (xs >= 0) & (xs < volNX), (ys >= 0) & (ys < volNY)
        np.add.at(cover, (xs[mx][:, None], ys[my][None, :]), 1)
        outside += not (mx.any() and my.any())
    assert outside >= 4 and {1, 4, 5, 7} <= set(np.unique(cover[3])) and cover.max() == 7
    assert xoff.min() < 0 and yoff.min() < 0 and (xoff + NX).max() > volNX and (yoff + NY).max() > volNY
    assert S % 8 != 0 and volNY > 256
    dests = [rng.integers(0, volNX * S, size=volNX * S) for _ in range(2)]
    assert not np.array_equal(dests[0], dests[1]) and np.bincount(dests[1], minlength=volNX * S).min() == 0
    return dict(NX=NX, NY=NY, volNX=volNX, S=S, volNY=volNY, xoff=xoff, yoff=yoff, B=B, dests=dests, angle=1,
                grot=ints(rng, (B, S, NX, NY, 2)), prior=ints(rng, (volNX * S, volNY, 2)))


def window_case_limit():
    """4 x 4 windows, S = 3, volume (6, 3, 12), Bmax = 1025, every window on column 1: with B = 1024 the overlap-add kernel's list is
    full on columns 1..4, with B = 1025 the call takes the fallback kernel"""
    rng = np.random.default_rng(32)
    NX = NY = 4
    volNX, S, volNY, Bmax = 6, 3, 12, 1025
    xoff = np.full(Bmax, 1, dtype=np.int32)
    yoff = rng.integers(-3, volNY, size=Bmax).astype(np.int32)
    assert np.all((xoff[:1024] <= 1) & (1 < xoff[:1024] + NX)) and len(xoff[:1024]) == WIN_MAXLIST and Bmax > WIN_MAXLIST
    dests = [rng.integers(0, volNX * S, size=volNX * S) for _ in range(2)]
    return dict(NX=NX, NY=NY, volNX=volNX, S=S, volNY=volNY, xoff=xoff, yoff=yoff, B=Bmax, dests=dests, angle=1,
                grot=ints(rng, (Bmax, S, NX, NY, 2)), prior=ints(rng, (volNX * S, volNY, 2)))


def tile_tab(kind, S, volNX):
    """'rows': every (x, z) its own volume row x * S + z; 'slab': one row per x shared by all slices (a slab object), so the
    kernel's register accumulation over dest == cur runs"""
    x, z = np.arange(volNX, dtype=np.int32), np.arange(S, dtype=np.int32)
    if kind == 'slab':
        return np.ascontiguousarray(np.broadcast_to(x[None, :], (S, volNX))), volNX
    return np.ascontiguousarray((x[None, :] * S + z[:, None]).astype(np.int32)), volNX * S


def tile_cover(x0, y0, TX, TY, volNX, volNY):
    cover = np.zeros((volNX, volNY), dtype=np.int64)
    for b in range(len(x0)):
        xs, ys = x0[b] + np.arange(TX), y0[b] + np.arange(TY)
        mx, my = (xs >= 0) & (xs < volNX), (ys >= 0) & (ys < volNY)
        np.add.at(cover, (xs[mx][:, None], ys[my][None, :]), 1)
    return cover


TILE_CASES = [('rows', 2, 3), ('slab', 2, 3), ('slab', 0, 6)]


def tile_case(kind, z0, nz):
    """tiles 6 x 4 on a volume of 11 x 14 columns, S = 6: origins negative and beyond the volume, 12 tiles on one origin (more
    than the MAXM = 9 a thread keeps in registers: the spill loop), a slice range that does not start at 0"""
    rng = np.random.default_rng(41)
    TX, TY, volNX, volNY, S = 6, 4, 11, 14, 6
    org = [(1, 2), (-3, -2), (9, 12), (11, 0), (20, 20), (-6, 3), (0, -4)] + [(4, 5)] * 12 + \
        [(int(rng.integers(-4, 10)), int(rng.integers(-3, 13))) for _ in range(8)] + [(2, 7)]
    x0, y0 = np.array([o[0] for o in org], dtype=np.int32), np.array([o[1] for o in org], dtype=np.int32)
    cover = tile_cover(x0, y0, TX, TY, volNX, volNY)
    assert cover.max() > 9 and x0.min() < 0 and y0.min() < 0 and (x0 + TX).max() > volNX and (y0 + TY).max() > volNY
    tab, n_rows = tile_tab(kind, S, volNX)
    return dict(TX=TX, TY=TY, volNX=volNX, volNY=volNY, S=S, z0=z0, nz=nz, x0=x0, y0=y0, B=len(org), tab=tab, n_rows=n_rows,
                grot=ints(rng, (len(org), nz, TX, TY, 2)), prior=ints(rng, (n_rows, volNY, 2)))


def tile_case_grid():
    """2100 volume columns of 6: more than the 2048 workgroups of the launch (256 CUs x 8)"""
    rng = np.random.default_rng(42)
    TX, TY, volNX, volNY, S = 6, 4, 2100, 6, 2
    B = 60
    x0 = np.concatenate([[2046, 2094, 2097, -2], rng.integers(-5, volNX, size=B - 4)]).astype(np.int32)
    y0 = rng.integers(-3, volNY, size=B).astype(np.int32)
    assert volNX > 2048 and tile_cover(x0, y0, TX, TY, volNX, volNY)[2048:].sum() > 0
    tab, n_rows = tile_tab('rows', S, volNX)
    return dict(TX=TX, TY=TY, volNX=volNX, volNY=volNY, S=S, z0=0, nz=S, x0=x0, y0=y0, B=B, tab=tab, n_rows=n_rows,
                grot=ints(rng, (B, S, TX, TY, 2)), prior=ints(rng, (n_rows, volNY, 2)))


def tile_case_cap():
    """1100 tiles of 4 x 4, all on x0 = 0: every covered volume column lists 1100 > BDOF_TILE_MAXLIST tiles"""
    rng = np.random.default_rng(43)
    TX = TY = 4
    volNX, volNY, S, B = 5, 9, 2, 1100
    x0 = np.zeros(B, dtype=np.int32)
    y0 = rng.integers(-3, volNY, size=B).astype(np.int32)
    assert B > TILE_MAXLIST and np.all(x0 == 0)
    tab, n_rows = tile_tab('rows', S, volNX)
    return dict(TX=TX, TY=TY, volNX=volNX, volNY=volNY, S=S, z0=0, nz=S, x0=x0, y0=y0, B=B, tab=tab, n_rows=n_rows,
                grot=ints(rng, (B, S, TX, TY, 2)), prior=ints(rng, (n_rows, volNY, 2)))


def cut_case_cap():
    """field 4 x 4, 1100 tiles of 4 x 4, taper 0: every field row lists 1100 > BDOF_TILE_MAXLIST (tile, row) pairs"""
    rng = np.random.default_rng(44)
    FX = FY = TX = TY = 4
    B = 1100
    x0, y0 = rng.integers(-8, 9, size=B).astype(np.int32), rng.integers(-8, 9, size=B).astype(np.int32)
    assert B * (TX // FX) > TILE_MAXLIST
    return dict(FX=FX, FY=FY, TX=TX, TY=TY, B=B, x0=x0, y0=y0, tiles=cints(rng, (B, TX, TY)), minus=cints(rng, (B, TX, TY)),
                prior=cints(rng, (FX, FY), np.complex128))


# ================================================================================================================================
# Device plumbing
# ================================================================================================================================
@pytest.fixture(scope='module')
def built():
    import __graft_entry__ as entry
    entry.build()


class Guarded(object):
    """A device array between two sentinel-filled guards; download() checks the guards and returns the array."""

    def __init__(self, ctx, host, sentinel=SENTINEL):
        from beyond_dof_amd import _lib
        host = np.ascontiguousarray(host)
        self.shape, self.sentinel = host.shape, host.dtype.type(sentinel)
        g = np.full(GUARD, self.sentinel, dtype=host.dtype)
        self.buf = _lib.DeviceBuffer.from_host(ctx, np.concatenate([g, host.reshape(-1), g]))
        self.ptr = self.buf.ptr + GUARD * host.dtype.itemsize          # GUARD * itemsize is a multiple of 256 bytes: alignment kept

    def download(self):
        a = self.buf.download()
        assert np.all(a[:GUARD] == self.sentinel) and np.all(a[-GUARD:] == self.sentinel), 'a guard was overwritten'
        return a[GUARD:-GUARD].reshape(self.shape)


def sentinels(shape, dtype=np.float32):
    return np.full(shape, SENTINEL, dtype=dtype)


class RotDevice(object):
    """An engine of the smallest shape a case needs ('generic': any NY, NX >= 1), the case's tables bound, its frame gradient in
    bdof_grot."""

    def __init__(self, ny, nx, n_slice, bmax, dests, vol_nx=None, vol_ny=None):
        from beyond_dof_amd import _lib
        from beyond_dof_amd.engine import MultisliceEngine
        vol_nx = nx if vol_nx is None else vol_nx
        self.tab, off, order = tables_from_dests(dests, vol_nx, n_slice)
        self.n_dest = vol_nx * n_slice
        self.eng = MultisliceEngine(ny, nx, n_slice, bmax, with_grad=True, engine='generic')
        self.ctx, self.lib, self.h = self.eng.ctx, self.eng.lib, self.eng.h
        up = lambda a: _lib.DeviceBuffer.from_host(self.ctx, np.ascontiguousarray(a))
        self.up = up
        if vol_ny is not None:               # the window path reads the volume's shape and the table's presence off the bound object
            self.eng.set_volume(up(np.zeros((self.n_dest, vol_ny, 2), np.float32)), self.n_dest, vol_ny, up(self.tab), vol_nx, len(dests))
        self.eng.set_rotation_adjoint(up(off), up(order), self.n_dest)
        self.room = bmax * n_slice * nx * ny * 2 * 4

    def set_grot(self, grot):
        grot = np.ascontiguousarray(grot, dtype=np.float32)
        assert grot.nbytes <= self.room
        self.ctx.check(self.lib.bdof_memcpy_h2d(self.h, self.lib.bdof_grot(self.h), grot.ctypes.data, grot.nbytes))

    def rows(self, angle_of_b, prior, row0, n_rows, accumulate, scale):
        ang, out = self.up(np.asarray(angle_of_b, dtype=np.int32)), Guarded(self.ctx, prior)
        self.ctx.check(self.lib.bdof_rotation_adjoint_rows(self.h, len(angle_of_b), ang.ptr, out.ptr, row0, n_rows, int(accumulate), scale))
        self.ctx.sync()
        return out.download()

    def windows(self, B, angle, xoff, yoff, prior, accumulate, scale):
        xo, yo, out = self.up(xoff[:B]), self.up(yoff[:B]), Guarded(self.ctx, prior)
        self.ctx.check(self.lib.bdof_window_rotation_adjoint(self.h, B, angle, xo.ptr, yo.ptr, out.ptr, int(accumulate), scale))
        self.ctx.sync()
        return out.download()


def bare_context():
    from beyond_dof_amd import _lib
    return _lib.Context(0)


# ================================================================================================================================
# 4. bdof_rotation_adjoint_rows: k_rot_adjoint + k_rot_adjoint_heavy
# ================================================================================================================================
@pytest.fixture(scope='module')
def rot_main(built):
    c = rot_case_main()
    dev = RotDevice(c['ny'], c['nx'], c['nz'], 66, c['dests'])
    dev.set_grot(c['grot'])
    c['rest_a'] = rot_adjoint_restated(c['grot'][:3], dev.tab, c['ang_a'])
    c['rest_b'] = rot_adjoint_restated(c['grot'], dev.tab, c['ang_b'])
    return c, dev


def test_rotation_adjoint_list_lengths(rot_main):
    """rows with 0, 1, 7, exactly 256 (wave path), 257 (heavy path) and 518 sources (515 of one angle: full stages and the
    remainder loop of the heavy kernel); every row of a sentinel-filled gradient is overwritten"""
    c, dev = rot_main
    n = c['nx'] * c['nz']
    got = dev.rows(c['ang_a'], sentinels((n, c['ny'], 2)), 0, n, 0, 1.0)
    assert np.array_equal(got, c['rest_a'])
    assert not np.any(c['rest_a'][0]) and np.any(c['rest_a'][1001]) and np.any(c['rest_a'][1199])


def test_rotation_adjoint_second_chunk_of_64(rot_main):
    """66 elements with repeated, unsorted angles: the second chunk of 64 lanes, a list abandoned half-written for the heavy
    path, and rows that stay on the wave path over both chunks (one of them with exactly 256 sources)"""
    c, dev = rot_main
    n = c['nx'] * c['nz']
    got = dev.rows(c['ang_b'], sentinels((n, c['ny'], 2)), 0, n, 0, 1.0)
    assert np.array_equal(got, c['rest_b'])


def test_rotation_adjoint_slabs_accumulate_scale(rot_main):
    """slabs whose row0 / n_rows are no multiples of 4, one after another: each leaves every row outside it untouched, together
    they give the whole call; then accumulate = 1 on a gradient of integers with scale 0.5, and scale 3"""
    c, dev = rot_main
    n, rest = c['nx'] * c['nz'], c['rest_b']
    cuts = [0, 5, 303, 610, 1199, n]
    assert any(a % 4 for a in cuts[1:-1]) and any((b - a) % 4 for a, b in zip(cuts[:-1], cuts[1:]))
    cur = sentinels((n, c['ny'], 2))
    for a, b in zip(cuts[:-1], cuts[1:]):
        new = dev.rows(c['ang_b'], cur, a, b - a, 0, 1.0)
        assert np.array_equal(new, expected_rows(cur, rest, a, b - a, 0, 1.0)), (a, b)
        cur = new
    assert np.array_equal(cur, rest)
    for (a, cnt), acc, scale in (((0, n), 1, 0.5), ((303, 307), 1, 3.0), ((0, n), 0, 3.0), ((1, 1198), 0, 0.5)):
        got = dev.rows(c['ang_b'], c['prior'], a, cnt, acc, scale)
        assert np.array_equal(got, expected_rows(c['prior'], rest, a, cnt, acc, scale)), (a, cnt, acc, scale)


@pytest.mark.parametrize('ny', [130, 516])
def test_rotation_adjoint_wide_rows(built, ny):
    """NY = 130: the second group of 64 float4 columns has one lane; NY = 516: a second pass of 256 columns, wave and heavy kernel"""
    c = rot_case_wide(ny)
    dev = RotDevice(ny, c['nx'], c['nz'], 5, c['dests'])
    dev.set_grot(c['grot'])
    n = c['nx'] * c['nz']
    rest = rot_adjoint_restated(c['grot'], dev.tab, c['ang'])
    assert np.array_equal(dev.rows(c['ang'], sentinels((n, ny, 2)), 0, n, 0, 1.0), rest)
    prior = ints(np.random.default_rng(5), (n, ny, 2))
    assert np.array_equal(dev.rows(c['ang'], prior, 3, 115, 1, 0.5), expected_rows(prior, rest, 3, 115, 1, 0.5))


def test_rotation_adjoint_grid_stride(built):
    """16384 rows of NY = 4: the row loop of k_rot_adjoint strides over the grid"""
    c = rot_case_grid()
    dev = RotDevice(c['ny'], c['nx'], c['nz'], 2, c['dests'])
    dev.set_grot(c['grot'])
    n = c['nx'] * c['nz']
    assert np.array_equal(dev.rows(c['ang'], sentinels((n, 4, 2)), 0, n, 0, 1.0), rot_adjoint_restated(c['grot'], dev.tab, c['ang']))


# ================================================================================================================================
# 5. bdof_window_rotation_adjoint: k_window_overlap_add + the rotation adjoint; k_window_rot_adjoint above 1024 windows
# ================================================================================================================================
def window_restated(c, B):
    tab, _, _ = tables_from_dests(c['dests'], c['volNX'], c['S'])
    return window_adjoint_restated(c['grot'][:B], tab[c['angle']], c['xoff'][:B], c['yoff'][:B], c['volNX'], c['volNY'])


@pytest.mark.parametrize('shape', WINDOW_SHAPES, ids=['5x7', '6x4'])
def test_window_adjoint(built, shape):
    """an odd and an even window: origins negative, overhanging, outside and duplicated, 1 / 4 / 5 / 7 windows over one y, a
    short last z chunk, a striding y loop, the second angle's tables; then accumulate and scale"""
    c = window_case(*shape)
    dev = RotDevice(c['NY'], c['NX'], c['S'], c['B'], c['dests'], c['volNX'], c['volNY'])
    dev.set_grot(c['grot'])
    rest = window_restated(c, c['B'])
    n = c['volNX'] * c['S']
    got = dev.windows(c['B'], c['angle'], c['xoff'], c['yoff'], sentinels((n, c['volNY'], 2)), 0, 1.0)
    assert np.array_equal(got, rest)
    for acc, scale in ((1, 0.5), (0, 3.0), (1, 1.0)):
        got = dev.windows(c['B'], c['angle'], c['xoff'], c['yoff'], c['prior'], acc, scale)
        assert np.array_equal(got, expected_rows(c['prior'], rest, 0, n, acc, scale)), (acc, scale)


def test_window_adjoint_at_and_above_the_list_limit(built):
    """B = 1024 windows on one column: the overlap-add kernel at its list limit; B = 1025: the fallback k_window_rot_adjoint"""
    c = window_case_limit()
    dev = RotDevice(c['NY'], c['NX'], c['S'], c['B'], c['dests'], c['volNX'], c['volNY'])
    dev.set_grot(c['grot'])
    n = c['volNX'] * c['S']
    for B in (1024, 1025):
        rest = window_restated(c, B)
        got = dev.windows(B, c['angle'], c['xoff'], c['yoff'], sentinels((n, c['volNY'], 2)), 0, 1.0)
        assert np.array_equal(got, rest), B
        got = dev.windows(B, c['angle'], c['xoff'], c['yoff'], c['prior'], 1, 0.5)
        assert np.array_equal(got, expected_rows(c['prior'], rest, 0, n, 1, 0.5)), B
    assert not np.array_equal(window_restated(c, 1024), window_restated(c, 1025))


# ================================================================================================================================
# 6, 7. bdof_tiles_grad_add (k_tiles_grad_add) and the list cap of it and of k_tiles_cut_adjoint
# ================================================================================================================================
class TileGradDevice(object):
    def __init__(self, c):
        from beyond_dof_amd import _lib
        self.ctx = bare_context()
        self.lib, self.h = self.ctx.lib, self.ctx.handle
        self.up = lambda a: _lib.DeviceBuffer.from_host(self.ctx, np.ascontiguousarray(a))
        # bdof_set_object and the slice-range check want a configured ctx: the tile's shape, S slices, no gradient workspace
        self.ctx.check(self.lib.bdof_configure(self.h, c['TY'], c['TX'], c['S'], 1, _lib.CFG_GENERIC))
        self.vol, self.tab = self.up(np.zeros((c['n_rows'], c['volNY'], 2), np.float32)), self.up(c['tab'][None])
        self.ctx.check(self.lib.bdof_set_object(self.h, self.vol.ptr, c['n_rows'], c['volNY'], self.tab.ptr, c['volNX'], 1))

    def grad_add(self, c):
        g, x0, y0, out = self.up(c['grot']), self.up(c['x0']), self.up(c['y0']), Guarded(self.ctx, c['prior'])
        self.ctx.check(self.lib.bdof_tiles_grad_add(self.h, g.ptr, out.ptr, c['B'], c['TX'], c['TY'], x0.ptr, y0.ptr, c['z0'], c['nz']))
        self.ctx.sync()
        return out.download()


def tile_expected(c):
    rest = tiles_grad_restated(c['grot'], c['tab'], c['x0'], c['y0'], c['z0'], c['n_rows'], c['volNY'])
    return c['prior'].astype(np.float64) + rest            # the call always accumulates


@pytest.mark.parametrize('kind,z0,nz', TILE_CASES, ids=['rows-z2', 'slab-z2', 'slab-all'])
def test_tiles_grad_add(built, kind, z0, nz):
    """non-square tiles on a non-square volume, origins beyond every edge, 12 tiles on one origin (the spill path), rows shared
    over z (the register accumulation), z0 != 0, into a gradient that already holds integers"""
    c = tile_case(kind, z0, nz)
    assert np.array_equal(TileGradDevice(c).grad_add(c), tile_expected(c))


def test_tiles_grad_add_grid_stride(built):
    c = tile_case_grid()
    assert np.array_equal(TileGradDevice(c).grad_add(c), tile_expected(c))


def test_tiles_grad_add_beyond_the_list(built):
    """1100 tiles on one volume column: all of them are summed (the kernel lists them 1024 at a time)"""
    c = tile_case_cap()
    got, want = TileGradDevice(c).grad_add(c), tile_expected(c)
    print('bdof_tiles_grad_add, 1100 tiles: largest |device - restatement|', np.abs(got - want).max())
    assert np.array_equal(got, want)


def test_tiles_gather_adjoint_beyond_the_list(built):
    """1100 tiles on every field row, taper 0: bdof_tiles_gather_adjoint and bdof_tiles_gather_adjoint_diff64 (with and without
    tiles_b / accumulate) sum all of them; one tile that alone wraps onto a field row more than 1024 times is refused"""
    from beyond_dof_amd import _lib
    c = cut_case_cap()
    ctx = bare_context()
    lib, h = ctx.lib, ctx.handle
    up = lambda a: _lib.DeviceBuffer.from_host(ctx, np.ascontiguousarray(a))
    t, m, x0, y0 = up(c['tiles']), up(c['minus']), up(c['x0']), up(c['y0'])
    geo = (c['FX'], c['FY'], c['B'], c['TX'], c['TY'], x0.ptr, y0.ptr, 0)
    want = cut_adjoint_restated(c['tiles'], c['x0'], c['y0'], c['FX'], c['FY'])
    out = Guarded(ctx, np.full((c['FX'], c['FY']), SENTINEL, np.complex64))
    ctx.check(lib.bdof_tiles_gather_adjoint(h, t.ptr, out.ptr, *geo))
    ctx.sync()
    got = out.download()
    print('bdof_tiles_gather_adjoint, 1100 tiles: largest |device - restatement|', np.abs(got - want).max())
    assert np.array_equal(got, want)
    want_diff = cut_adjoint_restated(c['tiles'].astype(np.complex128) - c['minus'], c['x0'], c['y0'], c['FX'], c['FY'])
    for minus, acc, ref in ((None, 0, want), (m.ptr, 0, want_diff), (m.ptr, 1, want_diff + c['prior']), (None, 1, want + c['prior'])):
        out = Guarded(ctx, c['prior'] if acc else np.full((c['FX'], c['FY']), SENTINEL, np.complex128))
        ctx.check(lib.bdof_tiles_gather_adjoint_diff64(h, t.ptr, minus, out.ptr, *geo, acc))
        ctx.sync()
        got = out.download()
        print('bdof_tiles_gather_adjoint_diff64, tiles_b', minus is not None, 'accumulate', acc, np.abs(got - ref).max())
        assert np.array_equal(got, ref), (minus is not None, acc)
    # ceil(TX / FX) = 1025 pairs of one tile on one field row: more than a workgroup lists
    wide, f1 = up(np.zeros((1, 1025, 2), np.complex64)), up(np.zeros((1, 2), np.complex64))
    assert lib.bdof_tiles_gather_adjoint(h, wide.ptr, f1.ptr, 1, 2, 1, 1025, 2, x0.ptr, y0.ptr, 0) == ERR_SIZE
    assert lib.bdof_tiles_gather_adjoint(h, wide.ptr, f1.ptr, 1, 2, 1, 1024, 2, x0.ptr, y0.ptr, 0) == 0
    ctx.sync()


# ================================================================================================================================
# 8. bdof_gather_fields: k_gather_fields (16-byte words) and k_gather_fields4 (4-byte words)
# ================================================================================================================================
@pytest.mark.parametrize('words,B', [(35 * 35, 3), (35 * 35, 1030), (4 * 306, 3), (4 * 306, 1030), (16641, 3), (4 * 16387, 3)],
                         ids=['4B-B3', '4B-B1030', '16B-B3', '16B-B1030', '4B-long', '16B-long'])
def test_gather_fields(built, words, B):
    """dst[b] = src[idx[b]] bit for bit: fields of 4 * (odd) bytes (the 4-byte kernel; a 35 x 35 float field, so fields start off
    16-byte alignment) and of 16 * k bytes (the float4 kernel); idx unsorted with repeats; B = 1030 > the grid's 1024 rows; the two
    long fields exceed the 64 x 256 words of one pass over a field"""
    from beyond_dof_amd import _lib
    nbytes = 4 * words
    assert (nbytes % 16 != 0 and words % 2 == 1) if words in (35 * 35, 16641) else nbytes % 16 == 0
    rng = np.random.default_rng(words + B)
    n_src = 7
    src = rng.integers(0, 2 ** 32, size=(n_src, words), dtype=np.uint32)
    idx = rng.integers(0, n_src, size=B).astype(np.int32)
    idx[:2], idx[-1] = (5, 2), 5
    assert len(set(idx.tolist())) < B and not np.all(np.diff(idx) >= 0)
    ctx = bare_context()
    s, i = _lib.DeviceBuffer.from_host(ctx, src), _lib.DeviceBuffer.from_host(ctx, idx)
    out = Guarded(ctx, np.full((B, words), 0xDEADBEEF, np.uint32), sentinel=0xDEADBEEF)
    ctx.check(ctx.lib.bdof_gather_fields(ctx.handle, out.ptr, s.ptr, i.ptr, B, ctypes.c_size_t(nbytes)))
    ctx.sync()
    assert np.array_equal(out.download(), src[idx])


# ================================================================================================================================
# 9. bdof_rotate_bilinear (k_rot_bilinear<false>) and bdof_rotate_bilinear_adjoint (k_rot_bilinear_adjoint<1, 2, 4, 8>)
# ================================================================================================================================
BILIN_NY = [2, 64, 130, 258, 514, 1024]
BILIN_B = [1, 3, 4, 5, 9]


@pytest.mark.parametrize('ny', BILIN_NY)
def test_bilinear_rotation_and_adjoint(built, ny):
    """a 7 x 10 x NY volume, non-zero up to every border, rotated to the first B of nine float32-rounded angles (generic ones,
    0, +-pi/2, pi, 2 pi) for every B in BILIN_B: forward, adjoint whole / in slabs / accumulating with scale 0.5, each element
    within the derived bound of the float64 oracle; and the pairing <R x, y> = <x, R^T y> on the device's outputs"""
    from beyond_dof_amd import _lib
    H, W = BILIN_NXV, BILIN_NZV
    rng = np.random.default_rng(900 + ny)
    vol = (1.0 + rng.normal(size=(H, W, ny, 2))).astype(np.float32)
    grot = (1.0 + rng.normal(size=(9, W, H, ny, 2))).astype(np.float32)
    prior = rng.normal(size=(H, W, ny, 2)).astype(np.float32)
    assert np.all(vol != 0) and np.all(grot != 0)
    fwd_ref, fwd_bound = bilinear_forward_reference(vol, BILIN_ANGLES)
    terms = bilinear_adjoint_terms(grot, BILIN_ANGLES)
    ctx = bare_context()
    lib, h = ctx.lib, ctx.handle
    up = lambda a: _lib.DeviceBuffer.from_host(ctx, np.ascontiguousarray(a))
    dvol, dgrot, prm = up(vol), up(grot), up(bilinear_prm(BILIN_ANGLES, H, W))
    cuts = [0, 3, 37, H * W]
    for B in BILIN_B:
        out = Guarded(ctx, sentinels((B, W, H, ny, 2)))
        ctx.check(lib.bdof_rotate_bilinear(h, dvol.ptr, H, W, ny, prm.ptr, B, out.ptr))
        ctx.sync()
        rot = out.download()
        assert_within(rot, fwd_ref[:B], fwd_bound[:B], 'forward NY {} B {}'.format(ny, B))

        def adjoint(start, row0, n_rows, acc, scale):
            g = Guarded(ctx, start)
            ctx.check(lib.bdof_rotate_bilinear_adjoint(h, dgrot.ptr, H, W, ny, prm.ptr, B, g.ptr, row0, n_rows, acc, scale))
            ctx.sync()
            return g.download()

        ref, bound = bilinear_adjoint_reference(terms, B)
        whole = adjoint(sentinels((H, W, ny, 2)), 0, H * W, 0, 1.0)
        assert_within(whole, ref, bound, 'adjoint NY {} B {}'.format(ny, B))
        cur = sentinels((H, W, ny, 2))
        for a, b in zip(cuts[:-1], cuts[1:]):
            cur = adjoint(cur, a, b - a, 0, 1.0)
            flat = cur.reshape(H * W, ny, 2)
            assert np.all(flat[b:] == SENTINEL) and np.array_equal(flat[:b], whole.reshape(H * W, ny, 2)[:b]), (a, b)
        got = adjoint(prior, 0, H * W, 1, 0.5)
        assert_within(got, prior.astype(np.float64) + 0.5 * ref, 0.5 * bound + 2.0 ** -24 * np.abs(prior), 'adjoint accumulate NY {} B {}'.format(ny, B))
        got = adjoint(prior, 5, 33, 1, 0.5).reshape(H * W, ny, 2)
        want = prior.astype(np.float64).reshape(H * W, ny, 2).copy()
        want[5:38] += 0.5 * ref.reshape(H * W, ny, 2)[5:38]
        bnd = np.zeros_like(want)
        bnd[5:38] = (0.5 * bound + 2.0 ** -24 * np.abs(prior)).reshape(H * W, ny, 2)[5:38]
        assert np.array_equal(got[:5], want[:5]) and np.array_equal(got[38:], want[38:])
        assert_within(got[5:38], want[5:38], bnd[5:38], 'adjoint slab accumulate NY {} B {}'.format(ny, B))
        # pairing, on the downloaded arrays in float64: x = vol, y = grot[:B]
        lhs = float(np.sum(rot.astype(np.float64) * grot[:B].astype(np.float64)))
        rhs = float(np.sum(vol.astype(np.float64) * whole.astype(np.float64)))
        print('pairing NY {} B {}: {} vs {}'.format(ny, B, lhs, rhs))
        assert abs(lhs - rhs) <= 1e-6 * abs(lhs)


def test_bilinear_adjoint_refuses_ny_above_1024(built):
    from beyond_dof_amd import _lib
    H, W, ny = BILIN_NXV, BILIN_NZV, 1026
    ctx = bare_context()
    g = _lib.DeviceBuffer.zeros(ctx, (1, W, H, ny, 2), np.float32)
    out = _lib.DeviceBuffer.zeros(ctx, (H, W, ny, 2), np.float32)
    prm = _lib.DeviceBuffer.from_host(ctx, bilinear_prm(BILIN_ANGLES[:1], H, W))
    assert ctx.lib.bdof_rotate_bilinear_adjoint(ctx.handle, g.ptr, H, W, ny, prm.ptr, 1, out.ptr, 0, H * W, 0, 1.0) == ERR_SIZE
    assert ctx.lib.bdof_rotate_bilinear_adjoint(ctx.handle, g.ptr, H, W, 1024, prm.ptr, 1, out.ptr, 0, H * W, 0, 1.0) == 0
    ctx.sync()
