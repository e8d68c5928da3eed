"""float64 numpy restatement of the analytic start (beyond_dof_amd/analytic.py, csrc/bdof_fbp.h), written for the tests: the
retrieval, the ramp and the back-projection as the header states them, and a multislice forward model of its own to make data."""
import numpy as np


def phantom(n, rng):
    """examples/reconstruct_phantom.py's blobs, in float64: host order (Y, X, Z)"""
    z, y, x = np.mgrid[:n, :n, :n].astype(np.float64)
    d = np.zeros((n, n, n))
    for _ in range(10):
        c = rng.uniform(n * 0.3, n * 0.7, size=3)
        r = rng.uniform(n * 0.04, n * 0.12)
        d += 1e-6 * np.exp(-((z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2) / (2 * r ** 2))
    return d


def ramp_rows(P):
    """q[..., x, y] = sum_x' h[x - x'] P[..., x', y], zero outside the frame; h written out here, not taken from the package"""
    n = P.shape[-2]
    m = np.arange(-(n - 1), n)
    h = np.where(m == 0, 0.25, np.where(m % 2 != 0, -1.0 / (np.pi ** 2 * np.maximum(m * m, 1).astype(np.float64)), 0.0))
    x = np.arange(n)
    T = h[(x[:, None] - x[None, :]) + n - 1]                    # T[x, x'] = h[x - x']
    return np.einsum('xs,...sy->...xy', T, P)


def contrast(meas, wgt, a0_sq):
    m = np.asarray(meas).astype(np.float64)
    g = m * m / a0_sq - 1.0
    if wgt is not None:
        g = np.where(np.asarray(wgt) != 0, g, 0.0)
    return g


def ctf_invert(meas, wgt, a0_sq, filters):
    """meas (B, D, NX, NY); filters (D, NX, NY) with the transforms' 1 / (NX NY) folded in (what bdof_ctf_retrieve takes) -> the
    retrieved projection P (B, NX, NY), before the ramp"""
    g = contrast(meas, wgt, a0_sq)
    nx, ny = g.shape[-2:]
    return (np.fft.ifft2(np.fft.fft2(g) * (filters * (nx * ny))[None])).real.sum(axis=1)


def ctf_retrieve(meas, wgt, a0_sq, filters):
    """... -> q (B, NX, NY), the ramp-filtered projection"""
    return ramp_rows(ctf_invert(meas, wgt, a0_sq, filters))


def cube_rotations():
    """the 24 signed permutation matrices with determinant +1"""
    import itertools
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1, -1), repeat=3):
            M = np.zeros((3, 3))
            for i in range(3):
                M[i, perm[i]] = signs[i]
            if np.linalg.det(M) > 0:
                out.append(M)
    return out


def integer_backprojection(q, Ms, ts, vol_shape):
    """sum_b q_b[o_x, o_y] with o = M_b^T (p - t_b) for signed permutations M and integer t, by index arithmetic in integers"""
    NX, NZ, NY = vol_shape
    out = np.zeros(vol_shape, dtype=np.int64)
    for b, (M, t) in enumerate(zip(Ms, ts)):
        Mi, ti = np.rint(M).astype(np.int64), np.rint(t).astype(np.int64)
        for x in range(NX):
            for z in range(NZ):
                for y in range(NY):
                    o = Mi.T @ (np.array([x, z, y]) - ti)
                    if 0 <= o[0] < q[b].shape[0] and 0 <= o[2] < q[b].shape[1]:
                        out[x, z, y] += int(q[b][o[0], o[2]])
    return out


def bilinear_taps(shape, ox, oy):
    """[(index x, index y, weight, inside)] of the four taps at float64 coordinates (arrays): weights as products of float64 factors"""
    nx, ny = shape
    fx, fy = np.floor(ox), np.floor(oy)
    rx, ry = ox - fx, oy - fy
    out = []
    for i, wx in ((0, 1 - rx), (1, rx)):
        for j, wy in ((0, 1 - ry), (1, ry)):
            px, py = fx.astype(np.int64) + i, fy.astype(np.int64) + j
            inside = (px >= 0) & (px < nx) & (py >= 0) & (py < ny)
            out.append((np.clip(px, 0, nx - 1), np.clip(py, 0, ny - 1), wx * wy, inside))
    return out


def backproject(q, rows, w, vol_shape):
    """(sum_b w_b bilinear(q_b; o_x, o_y), sum_b |w_b| sum_taps weight |q|) over the volume [X][Z][Y], o = M^T (p - t): the value
    and the magnitude sum a float32 rounding bound is stated against"""
    NX, NZ, NY = vol_shape
    p = np.stack(np.meshgrid(np.arange(NX), np.arange(NZ), np.arange(NY), indexing='ij')).reshape(3, -1).astype(np.float64)
    out, mag = np.zeros(p.shape[1]), np.zeros(p.shape[1])
    for b in range(len(q)):
        m = np.asarray(rows[b], dtype=np.float64).reshape(3, 4)
        o = m[:, :3].T @ (p - m[:, 3:4])
        for px, py, wt, inside in bilinear_taps(q[b].shape, o[0], o[2]):
            v = np.where(inside, q[b][px, py], 0.0)
            out += w[b] * wt * v
            mag += abs(w[b]) * wt * np.abs(v)
    return out.reshape(vol_shape), mag.reshape(vol_shape)


def trilinear_rotate(vol, row):
    """rotated[x, z, y] = trilinear sample of vol [X][Z][Y] at p = M o + t, o = (x, z, y); taps outside count 0"""
    NX, NZ, NY = vol.shape
    m = np.asarray(row, dtype=np.float64).reshape(3, 4)
    o = np.stack(np.meshgrid(np.arange(NX), np.arange(NZ), np.arange(NY), indexing='ij')).reshape(3, -1).astype(np.float64)
    p = m[:, :3] @ o + m[:, 3:4]
    f = np.floor(p)
    r = p - f
    i0 = f.astype(np.int64)
    out = np.zeros(p.shape[1])
    for c in range(8):
        bits = ((c >> 2) & 1, (c >> 1) & 1, c & 1)
        idx = [i0[a] + bits[a] for a in range(3)]
        wt = np.prod([r[a] if bits[a] else 1 - r[a] for a in range(3)], axis=0)
        inside = np.all([(idx[a] >= 0) & (idx[a] < vol.shape[a]) for a in range(3)], axis=0)
        out += np.where(inside, wt * vol[tuple(np.clip(idx[a], 0, vol.shape[a] - 1) for a in range(3))], 0.0)
    return out.reshape(vol.shape)


def forward_amplitudes(delta, beta, rows, energy_ev, psize_cm, free_prop_cm):
    """|detector wave| (n, D, Y, X) of the volume (Y, X, Z) under the maps `rows`: per voxel slice along z the modulation
    exp(i k (delta + i beta) dz) and a free-space step exp(-i pi lambda dz f^2), then the step to each detector plane; a unit plane
    wave.  f on the mesh of the product's forward model, written out here: the inclusive linspace(-1 / (2 dz), 1 / (2 dz), n),
    centred (cnn_propagator/util.py:73-102).  free_prop_cm: a sequence of D distances."""
    lam = 1240. / energy_ev
    dz = psize_cm * 1e7
    k = 2 * np.pi / lam
    vd, vb = np.transpose(delta, (1, 2, 0)), np.transpose(beta, (1, 2, 0))        # (x, z, y)
    NX, NZ, NY = vd.shape
    mesh = lambda n: np.fft.ifftshift(np.linspace(-0.5 / dz, 0.5 / dz, n))
    f2 = mesh(NX)[:, None] ** 2 + mesh(NY)[None, :] ** 2
    H1 = np.exp(-1j * np.pi * lam * dz * f2)
    Hd = [np.exp(-1j * np.pi * lam * fp * 1e7 * f2) for fp in free_prop_cm]
    out = np.empty((len(rows), len(Hd), NY, NX))
    for i, row in enumerate(rows):
        rd, rb = trilinear_rotate(vd, row), trilinear_rotate(vb, row)
        psi = np.ones((NX, NY), dtype=np.complex128)
        for z in range(NZ):
            psi = np.fft.ifft2(np.fft.fft2(psi * np.exp(1j * k * dz * (rd[:, z, :] + 1j * rb[:, z, :]))) * H1)
        spec = np.fft.fft2(psi)
        for d, h in enumerate(Hd):
            out[i, d] = np.abs(np.fft.ifft2(spec * h)).T
    return out


def analytic_start(prj_abs, rows, angle_w, C, reg, psize_cm, delta_beta_ratio, vol_shape, wgt=None, a0_sq=1.0):
    """(delta, beta) (Y, X, Z) of the whole chain for object_type='normal': prj_abs (n, D, Y, X); C, reg of the transfer; vol_shape (X, Z, Y)"""
    nx, ny = prj_abs.shape[-1], prj_abs.shape[-2]
    filters = np.conj(C) / ((np.abs(C) ** 2).sum(axis=0) + reg) / (nx * ny)
    q = ctf_retrieve(np.swapaxes(prj_abs, -2, -1), None if wgt is None else np.asarray(wgt).T, a0_sq, filters)
    beta = backproject(q, rows, angle_w, vol_shape)[0] / (psize_cm * 1e7)
    beta = np.transpose(beta, (2, 0, 1))
    return delta_beta_ratio * beta, beta
