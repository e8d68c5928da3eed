"""Host-side helpers of the hot path, mirroring the names of the reference's cnn_propagator/util.py.

Everything here is set-up work that runs once per reconstruction (transfer functions, rotation
lookup tables, task splitting); the per-step arithmetic lives in libbdof.so.  Tables are computed in
float64 exactly as the reference does so that the integer lookups are bit-identical.
"""
import os
import sys

import numpy as np

PI = 3.1415927   # the reference's literal (cnn_propagator/util.py:20); it enters k and H


def get_kernel(dist_nm, lmbda_nm, voxel_nm, grid_shape, pi=PI):
    """Fresnel transfer function H(u, v) on the reference's inclusive linspace mesh
    (cnn_propagator/util.py:73-102).  Returns a centred (Y, X) complex128 array."""
    ny, nx = int(grid_shape[0]), int(grid_shape[1])
    v = np.linspace(-1. / (2. * voxel_nm[1]), 1. / (2. * voxel_nm[1]), ny)     # rows: v_max = 1/(2 voxel[1])
    u = np.linspace(-1. / (2. * voxel_nm[0]), 1. / (2. * voxel_nm[0]), nx)     # cols: u_max = 1/(2 voxel[0])
    uu, vv = np.meshgrid(u, v)
    k = 2 * pi / lmbda_nm
    return np.exp(1j * k * dist_nm) * np.exp(-1j * pi * lmbda_nm * dist_nm * (uu ** 2 + vv ** 2))


def get_kernel_ir(dist_nm, lmbda_nm, voxel_nm, grid_shape, pi=PI):
    """Impulse-response form of the Fresnel kernel (cnn_propagator/util.py:105-127): the real-space kernel sampled on the
    pixel grid, Fourier transformed, times the pixel area.  The reference's propagator never selects it (np_funcs.py:55
    forces 'TF' after computing the sampling criterion of :51-53); here it is the detector step's `detector_kernel='IR'`
    option (detector_kernel below, MultisliceEngine.set_physics), 'auto' applies the reference's criterion."""
    ny, nx = int(grid_shape[0]), int(grid_shape[1])
    k = 2 * pi / lmbda_nm
    sy, sx = voxel_nm[0] * ny, voxel_nm[1] * nx
    x = np.arange(-sx / 2., -sx / 2. + sx, voxel_nm[1])
    y = np.arange(-sy / 2., -sy / 2. + sy, voxel_nm[0])
    xx, yy = np.meshgrid(x, y)
    h = np.exp(1j * k * dist_nm) / (1j * lmbda_nm * dist_nm) * np.exp(1j * k / (2 * dist_nm) * (xx ** 2 + yy ** 2))
    return np.fft.fftshift(np.fft.fft2(h)) * voxel_nm[0] * voxel_nm[1]


def upsample_2x(arr):
    """Multiscale hand-over (cnn_propagator/util.py:350-360): zero-stuffing by 2 along the three spatial axes followed by a
    sigma-1 gaussian filter; 4-D arrays channel by channel."""
    from scipy.ndimage import gaussian_filter
    arr = np.asarray(arr)
    if arr.ndim == 4:
        return np.stack([upsample_2x(arr[..., i]) for i in range(arr.shape[3])], axis=3)
    out = np.zeros([2 * n for n in arr.shape])
    out[::2, ::2, ::2] = arr
    return gaussian_filter(out, 1)


def get_kernel_tile(dist_nm, lmbda_nm, voxel_nm, tile_shape, field_shape, pi=PI):
    """The transfer function of a (FY, FX) FIELD's propagator, sampled at the FFT frequencies of a (TY, TX) tile of it.

    get_kernel puts H on an inclusive linspace of N points (quirk Q4): centred index k of an N-point axis, i.e. FFT frequency
    f = (k - N//2) / (N dx), carries u(f) = -u_max + (f N dx + N//2) * 2 u_max / (N - 1).  A tile cut out of the field must apply
    the SAME operator, so its bins (FFT frequencies (j - T//2) / (T dx)) take H at u(f) of the field's mesh, not of a T-point
    mesh of its own (whose effective step is (T - 1) / T instead of (N - 1) / N of the nominal one: 0.34 % in distance between
    512 and 4096 points, 0.7 rad at the band edge after 1024 slices).  Equals get_kernel when tile_shape == field_shape."""
    def axis(t, n, vox):
        u_max = 1. / (2. * vox)
        f = (np.arange(t) - t // 2) / (t * vox)
        return -u_max + (f * n * vox + n // 2) * 2. * u_max / (n - 1)
    v = axis(int(tile_shape[0]), int(field_shape[0]), voxel_nm[1])
    u = axis(int(tile_shape[1]), int(field_shape[1]), voxel_nm[0])
    uu, vv = np.meshgrid(u, v)
    k = 2 * pi / lmbda_nm
    return np.exp(1j * k * dist_nm) * np.exp(-1j * pi * lmbda_nm * dist_nm * (uu ** 2 + vv ** 2))


def detector_kernel_kind(kind, dist_nm, lmbda_nm, voxel_nm, grid_shape):
    """'TF' or 'IR' for the detector step.  'auto' is the criterion cnn_propagator/np_funcs.py:51-53 computes (and then
    overrides with 'TF' at :55): transfer function where the mean voxel size exceeds lambda z / L, impulse response otherwise."""
    if kind in ('TF', 'IR'):
        return kind
    if kind != 'auto':
        raise ValueError("detector_kernel must be 'TF', 'IR' or 'auto'")
    voxel_nm = np.asarray(voxel_nm, dtype=float)
    size_nm = np.array(grid_shape) * voxel_nm[:len(grid_shape)]
    crit_samp = lmbda_nm * dist_nm / np.prod(size_nm) ** (1. / len(size_nm))
    return 'TF' if np.prod(voxel_nm) ** (1. / 3) > crit_samp else 'IR'


def centred_kernel(dist_nm, lmbda_nm, voxel_nm, ny, nx, pi=PI, field_shape=None, kernel='TF'):
    """The centred (ny, nx) multiplier of one propagation step: get_kernel, get_kernel_tile (a tile of a larger field) or
    get_kernel_ir (kernel='IR', whole fields only)."""
    if kernel == 'IR':
        if field_shape is not None:
            raise ValueError("kernel='IR' is defined for whole fields, not for tiles of a larger one")
        return get_kernel_ir(dist_nm, lmbda_nm, voxel_nm, (ny, nx), pi=pi)
    if kernel != 'TF':
        raise ValueError("kernel must be 'TF' or 'IR'")
    if field_shape is None:
        return get_kernel(dist_nm, lmbda_nm, voxel_nm, (ny, nx), pi=pi)
    return get_kernel_tile(dist_nm, lmbda_nm, voxel_nm, (ny, nx), field_shape, pi=pi)


def device_transfer_function(dist_nm, lmbda_nm, voxel_nm, ny, nx, pi=PI, field_shape=None, dtype=np.complex64, kernel='TF'):
    """H prepared for libbdof: un-shifted [ky][kx], 1/(NX*NY) folded in, complex64 (complex128: the float64 adjoint sweep's
    table, bdof_set_physics_f64).  field_shape: the (ny, nx) wavefield is a tile of a larger field whose propagator it applies
    (get_kernel_tile).  kernel='IR': the impulse-response form (get_kernel_ir, cnn_propagator/util.py:105-127)."""
    h = centred_kernel(dist_nm, lmbda_nm, voxel_nm, ny, nx, pi, field_shape, kernel)
    hs = np.fft.ifftshift(h) / float(nx * ny)
    return np.ascontiguousarray(hs.astype(dtype))


def transfer_function_dc(dist_nm, lmbda_nm, voxel_nm, ny, nx, pi=PI, field_shape=None, kernel='TF'):
    """(re, im) of ifftshift(H)[0][0]: the factor a constant wave picks up in one transfer-function step."""
    h = centred_kernel(dist_nm, lmbda_nm, voxel_nm, ny, nx, pi, field_shape, kernel)
    v = complex(np.fft.ifftshift(h)[0, 0])
    return v.real, v.imag


MAX_DETECTOR_PLANES = 8      # BDOF_MAX_PLANES (include/bdof.h): detector planes per wavefield


def detector_distances(free_prop_cm):
    """free_prop_cm as every layer takes it -> (free_prop_cm, planes): None, 'inf' or a distance pass as they are, with planes
    None; a sequence of D finite positive distances in cm (several detector planes per angle, bdof_set_detector_planes) comes
    back as a tuple of floats with planes = that tuple — except a sequence of one, which IS its scalar (planes None).  Raises
    ValueError for anything else inside a sequence (None, 'inf', zero, negative, non-finite) and for more than
    MAX_DETECTOR_PLANES entries."""
    if isinstance(free_prop_cm, str):
        if free_prop_cm != 'inf':
            raise ValueError("free_prop_cm must be None, a distance in cm, a sequence of distances or 'inf'")
        return free_prop_cm, None
    if free_prop_cm is None or np.ndim(free_prop_cm) == 0:
        return free_prop_cm, None
    seq = list(free_prop_cm) if np.ndim(free_prop_cm) == 1 else None
    if not seq:
        raise ValueError('free_prop_cm as a sequence holds one distance per detector plane: at least one, in one dimension')
    if len(seq) > MAX_DETECTOR_PLANES:
        raise ValueError('free_prop_cm holds {} detector planes, more than the {} that are carried'.format(len(seq), MAX_DETECTOR_PLANES))
    for d in seq:
        if isinstance(d, (str, bool)) or d is None or not isinstance(d, (int, float, np.integer, np.floating)) or not np.isfinite(d) or not d > 0:
            raise ValueError('free_prop_cm as a sequence of detector planes takes finite distances > 0 in cm, not {!r}'.format(d))
    if len(seq) == 1:
        return seq[0], None
    return tuple(float(d) for d in seq), tuple(float(d) for d in seq)


class Optics(object):
    """Units and propagation multipliers of one (ny, nx) wavefield geometry: what the engine and the tiled propagator take
    every wavelength, voxel size, k and transfer-function table from.  free_prop_cm: None (no detector step), a distance in cm,
    a sequence of distances (detector planes, detector_distances: det_planes_nm holds them and det_nm the first; a sequence of
    one is its scalar) or 'inf' (far field); field_shape: the wavefield is a tile of a (FY, FX) field (get_kernel_tile)."""

    def __init__(self, energy_ev, psize_cm, free_prop_cm, pi, ny, nx, field_shape=None):
        free_prop_cm, planes = detector_distances(free_prop_cm)
        self.det_planes_nm = None if planes is None else tuple(d * 1e7 for d in planes)
        if planes is not None:
            free_prop_cm = planes[0]
        self.voxel_nm = np.array([psize_cm] * 3) * 1.e7 if np.isscalar(psize_cm) else np.array(psize_cm) * 1.e7
        self.lmbda_nm = 1240. / energy_ev
        self.delta_nm = self.voxel_nm[-1]                      # slice thickness
        self.pi = pi                                           # enters k and H: the reference's literal, or numpy's (set_conv)
        self.k = 2. * pi * self.delta_nm / self.lmbda_nm
        self.det_nm = None if free_prop_cm is None or isinstance(free_prop_cm, str) else free_prop_cm * 1e7
        self.ny, self.nx, self.field_shape = int(ny), int(nx), field_shape
        self.n_planes = 1 if self.det_planes_nm is None else len(self.det_planes_nm)      # frames per wavefield at the detector

    def _args(self, tiled, kernel='TF'):
        return self.lmbda_nm, self.voxel_nm, self.ny, self.nx, self.pi, self.field_shape if tiled else None, kernel

    def slice_kernel(self, tiled):
        """Centred multiplier of one slice step.  tiled=False: the (ny, nx) mesh's own even for a tile of a larger field."""
        return centred_kernel(self.delta_nm, *self._args(tiled))

    def detector_kernel(self, kind, tiled=False):
        """Centred multiplier of the step to the detector, kind 'TF' or 'IR' (whole fields only)."""
        return centred_kernel(self.det_nm, *self._args(tiled, kind))

    def table(self, dist_nm, kernel='TF', tiled=False, fold=True, transpose=False, dtype=np.complex64):
        """The multiplier of a step over dist_nm in device layout: un-shifted, [ky][kx] or, if transpose, [kx][ky].  fold: 1/(nx*ny)
        folded in (device_transfer_function: the sweeps' tables) or not (the carrier fields' and the host's)."""
        lmbda_nm, voxel_nm, ny, nx, pi, fs, kernel = self._args(tiled, kernel)
        if fold:
            h = device_transfer_function(dist_nm, lmbda_nm, voxel_nm, ny, nx, pi, fs, dtype, kernel)
        else:
            h = np.fft.ifftshift(centred_kernel(dist_nm, lmbda_nm, voxel_nm, ny, nx, pi, fs, kernel)).astype(dtype)
        return np.ascontiguousarray(h.T) if transpose else h

    def dc(self, dist_nm, kernel='TF', tiled=False):
        """(re, im) array of the factor a constant wave picks up over dist_nm (transfer_function_dc)."""
        return np.array(transfer_function_dc(dist_nm, *self._args(tiled, kernel)))


def conv_kernel_separable(delta_nm, lmbda_nm, voxel_nm, grid_shape, kernel_size, pi=PI):
    """The truncated real-space Fresnel kernel of cnn_propagator/propagation.py:35-44 in separable form:
    K[p][q] = e * ky[p] * kx[q].  H on the (Y-1, X-1) mesh is e * outer(fv, fu), so its inverse FFT, fftshift and centre
    crop factorise exactly.  Returns (ky, kx, e) in complex128."""
    ny, nx = int(grid_shape[0]) - 1, int(grid_shape[1]) - 1
    half = int((kernel_size - 1) / 2)

    def one(n, vox):
        f = np.exp(-1j * pi * lmbda_nm * delta_nm * np.linspace(-1. / (2. * vox), 1. / (2. * vox), n) ** 2)
        k1 = np.fft.fftshift(np.fft.ifft(np.fft.ifftshift(f)))
        mid = int((n - 1) / 2)
        return k1[mid - half:mid + half + 1]

    ky = one(ny, voxel_nm[1])       # rows of H follow v_max = 1/(2 voxel[1])  (get_kernel)
    kx = one(nx, voxel_nm[0])
    e = np.exp(1j * (2 * pi / lmbda_nm) * delta_nm)
    return ky, kx, e


def conv_probe_stack(probe, ky, kx, e, n_slice):
    """The probe carried through EMPTY space by the real-space propagator's own step (cnn_propagator/propagation.py:79-104
    without an object), in float64: p_0 = probe, p_{z+1} = K * pad(p_z, edge_z) ('valid' true convolution, K = e ky (x) kx),
    edge_{z+1} = sum(K) edge_z, edge_0 = 1.  Returns the S + 1 planes (S + 1, Y, X) complex128 — the carrier field of
    bdof_set_conv_probe_stack.  Two 1-D passes of shifted adds: cheap enough for a 512^2 x 512 stack."""
    h = (len(ky) - 1) // 2
    ksum = e * ky.sum() * kx.sum()
    p = np.array(probe, dtype=np.complex128)
    ny, nx = p.shape
    planes = np.empty((n_slice + 1, ny, nx), dtype=np.complex128)
    planes[0] = p
    edge = 1.0 + 0j
    for z in range(n_slice):
        padded = np.pad(p, h, mode='constant', constant_values=edge)
        t = np.zeros((ny, nx + 2 * h), dtype=np.complex128)
        for a in range(2 * h + 1):                    # out[y] = sum_a ky[a] in[y + 2h - a]: a true convolution
            t += ky[a] * padded[2 * h - a:2 * h - a + ny, :]
        q = np.zeros((ny, nx), dtype=np.complex128)
        for b in range(2 * h + 1):
            q += kx[b] * t[:, 2 * h - b:2 * h - b + nx]
        p = e * q
        edge = edge * ksum
        planes[z + 1] = p
    return planes


def rotation_lookup(array_size, n_theta):
    """Nearest-neighbour rotation source coordinates for every angle, as save_rotation_lookup builds
    them (cnn_propagator/util.py:294-332) but kept in memory: list of (X*Z, 2) int arrays.  Angles are
    linspace(0, 2*pi, n_theta) whatever theta_st/theta_end say (reference behaviour)."""
    ny, nx, nz = [int(a) for a in array_size]
    cx, cz = np.floor(nx / 2), np.floor(nz / 2)
    xs = np.repeat(np.arange(nx), nz) - cx
    zs = np.tile(np.arange(nz), nx) - cz
    new = np.stack([xs, zs]).astype(np.float32)
    out = []
    for theta in np.linspace(0, 2 * np.pi, n_theta):
        rot = np.array([[np.cos(theta), -np.sin(theta)], [np.sin(theta), np.cos(theta)]])
        old = np.matmul(rot, new)
        c1 = np.clip(np.round(old[0] + cx).astype(int), 0, nx - 1)
        c2 = np.clip(np.round(old[1] + cz).astype(int), 0, nz - 1)
        out.append(np.stack([c1, c2], axis=1))
    return out


def save_rotation_lookup(array_size, n_theta, dest_folder=None):
    """Drop-in for cnn_propagator/util.py:294-347: writes the same .npy files and returns the tables.  The folder appears
    atomically (written under a temporary name, then renamed), so a concurrent reader never sees half of it."""
    coords = rotation_lookup(array_size, n_theta)
    if dest_folder is None:
        dest_folder = 'arrsize_{}_{}_{}_ntheta_{}'.format(array_size[0], array_size[1], array_size[2], n_theta)
    tmp = '{}.tmp{}'.format(dest_folder.rstrip('/'), os.getpid())
    os.makedirs(tmp, exist_ok=True)
    for i, arr in enumerate(coords):
        np.save(os.path.join(tmp, '{:04}'.format(i)), arr)
    ny, nx, nz = [int(a) for a in array_size]
    coord0 = np.repeat(np.arange(ny), nx * nz)
    coord1 = np.tile(np.repeat(np.arange(nx), nz), ny).astype(float)
    coord2 = np.tile(np.tile(np.arange(nz), nx), ny).astype(float)
    for i, coord in enumerate([coord0, coord1, coord2]):
        np.save(os.path.join(tmp, 'coord{}_vec'.format(i)), coord)
    if os.path.isdir(dest_folder):                      # refresh an existing (possibly incomplete) folder file by file
        for f in os.listdir(tmp):
            os.replace(os.path.join(tmp, f), os.path.join(dest_folder, f))
        os.rmdir(tmp)
    else:
        os.rename(tmp, dest_folder)
    return coords


def rotation_lookup_files(array_size, n_theta, comm):
    """The tables of the run, through the reference's files (cnn_propagator/fullfield.py:209-215, ptychography.py:149-158):
    rank 0 writes the folder if it is missing or incomplete, EVERY rank passes the same barrier, then every rank reads."""
    folder = 'arrsize_{}_{}_{}_ntheta_{}'.format(array_size[0], array_size[1], array_size[2], n_theta)
    if comm.rank == 0:
        complete = all(os.path.exists(os.path.join(folder, '{:04}.npy'.format(i))) for i in range(n_theta))
        if not complete:
            save_rotation_lookup(array_size, n_theta, folder)
    comm.Barrier()
    return read_all_origin_coords(folder, n_theta)


def read_all_origin_coords(src_folder, n_theta):
    """cnn_propagator/util.py:369-374."""
    return [np.load(os.path.join(src_folder, '{:04}.npy'.format(i))) for i in range(n_theta)]


def device_rotation_tables(coords, nx, nz):
    """int32 tables for libbdof from the reference-style coordinate lists.

    tab[a][z][x]   = source row (x' * Z + z') of the [X][Z][Y] volume feeding rotated row (x, z)
    off/order      = per-angle inverse (CSR): for every volume row the rotated rows (z*X + x) it feeds
    """
    n = len(coords)
    tab = np.empty((n, nz, nx), dtype=np.int32)
    off = np.empty((n, nx * nz + 1), dtype=np.int32)
    order = np.empty((n, nz * nx), dtype=np.int32)
    for a, c in enumerate(coords):
        src = (c[:, 0] * nz + c[:, 1]).reshape(nx, nz)       # indexed [x][z]
        t = np.ascontiguousarray(src.T)                       # [z][x]
        tab[a] = t
        dest = t.reshape(-1)                                  # indexed by s = z*X + x
        order[a] = np.argsort(dest, kind='stable')
        off[a, 0] = 0
        np.cumsum(np.bincount(dest, minlength=nx * nz), out=off[a, 1:])
    return tab, off, order


def _rigid_factors(shape, axis_tilt, axis_roll, center):
    """T, R, c_v, c_o of rigid_geometry and the derivatives dT / d axis_tilt, dR / d axis_roll"""
    ny, nx, nz = [int(a) for a in shape]
    ca, sa, cr, sr = np.cos(float(axis_tilt)), np.sin(float(axis_tilt)), np.cos(float(axis_roll)), np.sin(float(axis_roll))
    T = np.array([[1., 0., 0.], [0., ca, sa], [0., -sa, ca]])
    R = np.array([[cr, 0., sr], [0., 1., 0.], [-sr, 0., cr]])
    dT = np.array([[0., 0., 0.], [0., -sa, ca], [0., -ca, -sa]])
    dR = np.array([[-sr, 0., cr], [0., 0., 0.], [-cr, 0., -sr]])
    c_v = np.array([(nx - 1) / 2., (nz - 1) / 2., (ny - 1) / 2.])
    c_o = c_v.copy()
    if center is not None:
        c_o[0] = float(center)
    return T, R, dT, dR, c_v, c_o


def _rigid_shifts(shifts, n):
    """shifts (n, 2) = (horizontal, vertical) per angle as the (n, 3) offsets of c_o: (sx, 0, sy); None: zeros"""
    off = np.zeros((n, 3))
    if shifts is not None:
        sh = np.asarray(shifts, dtype=np.float64)
        if sh.shape != (n, 2):
            raise ValueError('shifts must have shape (n_theta, 2) = ({}, 2), not {}'.format(n, sh.shape))
        off[:, 0], off[:, 2] = sh[:, 0], sh[:, 1]
    return off


def rigid_geometry(theta, shape, axis_tilt=0., axis_roll=0., center=None, shifts=None):
    """(n_theta, 12) float64: the rows of (M | t) of rotation='trilinear' for a volume of shape (Y, X, Z).  Output voxel
    o = (x, z, y) of the beam frame samples the volume at p = M o + t in index coordinates (x', z', y'), with

        M(theta) = M0(theta) T(axis_tilt) R(axis_roll),      t = c_v - M c_o
        M0: x' =  cos x + sin z ; z' = -sin x + cos z ; y' = y       (the bilinear rotation's own map)
        T : z' =  cos z + sin y ; y' = -sin z + cos y ; x' = x       (axis tilted towards the beam: laminography)
        R : x' =  cos x + sin y ; y' = -sin x + cos y ; z' = z       (axis rolled about the beam)
        c_v = ((X - 1) / 2, (Z - 1) / 2, (Y - 1) / 2),  c_o = c_v with its first entry replaced by `center` if given,
        plus (sx_i, 0, sy_i) for angle i if `shifts` is given

    center: the detector column the axis projects onto, as a (possibly fractional) pixel index.  Angles in radians.
    shifts: (n_theta, 2), the detector offset (horizontal, vertical) of every angle in pixels; None and zeros give the same rows."""
    th = np.atleast_1d(np.asarray(theta, dtype=np.float64))
    T, R, _, _, c_v, c_o = _rigid_factors(shape, axis_tilt, axis_roll, center)
    off = _rigid_shifts(shifts, len(th))
    out = np.empty((len(th), 3, 4))
    for i, a in enumerate(th):
        c, s = np.cos(a), np.sin(a)
        M = np.array([[c, s, 0.], [-s, c, 0.], [0., 0., 1.]]) @ T @ R
        out[i, :, :3] = M
        out[i, :, 3] = c_v - M @ (c_o + off[i])
    return out.reshape(len(th), 12)


GEOMETRY_NAMES = ('center', 'axis_tilt', 'axis_roll', 'theta', 'shifts')


def rigid_geometry_gradient(theta, shape, axis_tilt, axis_roll, center, shifts, dprm, index):
    """The chain rule of rigid_geometry: dprm (len(index), 12) = dL/d(M | t) of the angles `index` of theta -> dict of
    dL/d theta (len(index), of the listed angles), axis_tilt, axis_roll, center (scalars, summed over the listed angles) and
    shifts (len(index), 2).  Analytic, float64: with G = (G_M | G_t) the row of an angle and a parameter moving M by dM,
        dL = <G_M, dM> - G_t . (dM c_o),        dL/d c_o = -M^T G_t
    (center is c_o's first entry for every angle, a shift the first and third of its own angle's)."""
    th = np.atleast_1d(np.asarray(theta, dtype=np.float64))
    index = np.atleast_1d(np.asarray(index, dtype=np.int64))
    G = np.asarray(dprm, dtype=np.float64).reshape(len(index), 3, 4)
    T, R, dT, dR, c_v, c_o = _rigid_factors(shape, axis_tilt, axis_roll, center)
    off = _rigid_shifts(shifts, len(th))
    out = dict(theta=np.zeros(len(index)), axis_tilt=0.0, axis_roll=0.0, center=0.0, shifts=np.zeros((len(index), 2)))
    for k, i in enumerate(index):
        c, s = np.cos(th[i]), np.sin(th[i])
        M0 = np.array([[c, s, 0.], [-s, c, 0.], [0., 0., 1.]])
        dM0 = np.array([[-s, c, 0.], [-c, -s, 0.], [0., 0., 0.]])
        GM, Gt, co = G[k, :, :3], G[k, :, 3], c_o + off[i]
        d = lambda dM: float(np.sum(GM * dM) - Gt @ (dM @ co))
        out['theta'][k] = d(dM0 @ T @ R)
        out['axis_tilt'] += d(M0 @ dT @ R)
        out['axis_roll'] += d(M0 @ T @ dR)
        dco = -(M0 @ T @ R).T @ Gt
        out['center'] += float(dco[0])
        out['shifts'][k] = dco[0], dco[2]
    return out


def check_rigid(rotation_matrices, n_theta):
    """A user's rotation_matrices (n_theta, 3, 4) = (M | t) as the (n_theta, 12) float64 the kernels take.  ValueError unless
    every M is orthonormal (|M^T M - I| <= 1e-9) with det > 0: the adjoint's candidate search relies on M preserving distances."""
    m = np.array(rotation_matrices, dtype=np.float64)
    if m.shape != (int(n_theta), 3, 4):
        raise ValueError('rotation_matrices must have shape (n_theta, 3, 4) = ({}, 3, 4), not {}'.format(int(n_theta), m.shape))
    M = m[:, :, :3]
    dev = np.abs(np.einsum('nji,njk->nik', M, M) - np.eye(3)).max(axis=(1, 2))
    if not np.all(np.isfinite(m)) or np.any(dev > 1e-9) or np.any(np.linalg.det(M) <= 0):
        raise ValueError('rotation_matrices must be rigid: every 3 x 3 part orthonormal to 1e-9 with det > 0 '
                         '(largest |M^T M - I| is {:.3g})'.format(float(np.nanmax(dev))))
    return np.ascontiguousarray(m.reshape(len(m), 12))


def rigid_prm(n_theta, shape, theta, axis_tilt=0., axis_roll=0., center=None, rotation_matrices=None, shifts=None):
    """(n_theta, 12) float64 rows of (M | t) for rotation='trilinear' from a solver's keywords (ValueError for what is missing, of
    the wrong length or not rigid): rotation_matrices if given, else rigid_geometry of theta and the axis keywords."""
    if theta is None and rotation_matrices is None:
        raise ValueError("rotation='trilinear' needs the projection angles theta or rotation_matrices")
    if rotation_matrices is not None:
        return check_rigid(rotation_matrices, n_theta)
    if len(np.atleast_1d(theta)) != int(n_theta):
        raise ValueError('theta must hold n_theta = {} angles'.format(int(n_theta)))
    return rigid_geometry(theta, shape, axis_tilt, axis_roll, center, shifts)


def bilinear_prm(n_theta, shape, theta, *ignored):
    """(n_theta, 4) float64 rows (cos, sin, x_off, y_off) for rotation='bilinear': the per-angle projective transform of
    tf.contrib.image.rotate for images of height X and width Z of a (Y, X, Z) volume; the geometry keywords are ignored."""
    if theta is None:
        raise ValueError("rotation='bilinear' needs the projection angles theta")
    th = np.asarray(theta, dtype=np.float64)
    assert len(th) == int(n_theta)
    H, W = int(shape[1]), int(shape[2])
    c, sn = np.cos(th), np.sin(th)
    return np.stack([c, sn, ((W - 1) - (c * (W - 1) - sn * (H - 1))) / 2.0, ((H - 1) - (sn * (W - 1) + c * (H - 1))) / 2.0], axis=1)


class RotationKeywords(object):
    """The rotation keywords of an entry point's **kwargs.  rotation: the value as given ('nearest' if absent); with `only`, a
    value outside it stays ignored and counts as 'nearest'.  For rotation='trilinear' — a rigid map per angle, sampled trilinearly —
    the geometry: axis_tilt / axis_roll (radians), center (the detector column the axis projects onto, a pixel index of the
    full-resolution data) or rotation_matrices (n_theta, 3, 4) in voxels of the full-resolution volume.  With any other rotation
    the four are ignored and for_level gives no keyword.  refine_geometry / geometry_learning_rate go to the solver as they are
    (which refuses them for another rotation); what a level has refined is kept in full-resolution units (keep) and handed to
    the next level (level_values)."""

    def __init__(self, kwargs, only=None):
        self.rotation = kwargs.get('rotation', 'nearest')
        if only is not None and self.rotation not in only:
            self.rotation = 'nearest'
        self.trilinear = self.rotation == 'trilinear'
        self.axis_tilt, self.axis_roll = float(kwargs.get('axis_tilt', 0.)), float(kwargs.get('axis_roll', 0.))
        self.center, self.rotation_matrices = kwargs.get('center'), kwargs.get('rotation_matrices')
        refine = kwargs.get('refine_geometry', ())
        self.refine = (refine,) if isinstance(refine, str) else tuple(refine or ())
        self.rate = float(kwargs.get('geometry_learning_rate', 0.05))
        self.refined = None                       # the last level's geometry() in full-resolution units

    def select(self, n_theta, index=None):
        """Once the data are read: keep the rotation_matrices of the angles the run keeps (index: a slice or an index array, as
        theta_downsample picks them) and hold them to check_rigid for the n_theta that are left."""
        if self.trilinear and self.rotation_matrices is not None:
            m = np.asarray(self.rotation_matrices, dtype=np.float64)
            self.rotation_matrices = check_rigid(m if index is None else m[index], n_theta).reshape(-1, 3, 4)

    def for_level(self, ds_level):
        """The solver's geometry keywords at multiscale level ds_level.  The levels are strided, not binned: voxel i of a level is
        voxel i * ds_level of the full resolution, so an explicit centre and the translations divide by ds_level (the default
        centre is the level's own middle column)."""
        if not self.trilinear:
            return {}
        geometry = dict(axis_tilt=self.axis_tilt, axis_roll=self.axis_roll, center=None if self.center is None else float(self.center) / ds_level)
        if self.rotation_matrices is not None:
            level = self.rotation_matrices.copy()
            level[:, :, 3] /= ds_level
            geometry['rotation_matrices'] = level
        if self.refine:
            geometry.update(refine_geometry=self.refine, geometry_learning_rate=self.rate)
        return geometry

    def keep(self, values, ds_level):
        """a solver's geometry() at level ds_level, in full-resolution units: center and shifts times ds_level"""
        self.refined = dict(values, center=np.asarray(values['center']) * ds_level, shifts=np.asarray(values['shifts']) * ds_level)
        return self.refined

    def record(self, values, ds_level, output_folder, summary=False):
        """keep(), written as geometry.npy (a dict of arrays; np.load(..., allow_pickle=True).item()) and, with summary, as
        refined_<name> lines behind what summary.txt holds"""
        refined = self.keep(values, ds_level)
        np.save(os.path.join(output_folder, 'geometry.npy'), refined)
        if summary:
            with open(os.path.join(output_folder, 'summary.txt'), 'a') as f:
                for name in GEOMETRY_NAMES:
                    f.write('{:<20}{}\n'.format('refined_' + name, np.array2string(np.asarray(refined[name]), threshold=10 ** 6).replace('\n', ' ')))

    def level_values(self, ds_level):
        """what keep() holds, in the units of level ds_level (None: nothing refined yet)"""
        if self.refined is None:
            return None
        return dict(self.refined, center=self.refined['center'] / ds_level, shifts=self.refined['shifts'] / ds_level)

    def summary(self):
        """The geometry as a run's summary records it (the matrices only as 'given')."""
        return dict(self.for_level(1), center=self.center, rotation_matrices=None if self.rotation_matrices is None else 'given')


def split_tasks(arr, split_size):
    """cnn_propagator/util.py:271-277."""
    return [arr[i:i + split_size] for i in range(0, len(arr), split_size)]


def mag_phase_to_real_imag(mag, phase):
    """cnn_propagator/util.py:265-268."""
    a = mag * np.exp(1j * phase)
    return a.real, a.imag


def gaussian_probe(shape, probe_mag_sigma, probe_phase_sigma, probe_phase_max):
    """Gaussian probe of cnn_propagator/fullfield.py:299-310 / ptychography.py:212-222."""
    py = np.arange(shape[0]) - (shape[0] - 1.) / 2
    px = np.arange(shape[1]) - (shape[1] - 1.) / 2
    pxx, pyy = np.meshgrid(px, py)
    mag = np.exp(-(pxx ** 2 + pyy ** 2) / (2 * probe_mag_sigma ** 2))
    phase = probe_phase_max * np.exp(-(pxx ** 2 + pyy ** 2) / (2 * probe_phase_sigma ** 2))
    return mag_phase_to_real_imag(mag, phase)


def print_flush(a, designate_rank=None, this_rank=None):
    """cnn_propagator/util.py:248-256."""
    if designate_rank is None or this_rank == designate_rank:
        print(a)
    sys.stdout.flush()


# ---- layout conversion between the reference's arrays and libbdof's device layout ------------------
def volume_to_rows(obj_delta, obj_beta):
    """(Y, X, Z) delta and beta -> [X][Z][Y] (delta, beta) pairs, float32."""
    pair = np.stack([obj_delta, obj_beta], axis=-1)
    return np.ascontiguousarray(pair.transpose(1, 2, 0, 3).astype(np.float32))


def rows_to_volume(rows):
    """Inverse of volume_to_rows: [X][Z][Y][2] -> (delta, beta) each (Y, X, Z)."""
    v = rows.transpose(2, 0, 1, 3)
    return np.ascontiguousarray(v[..., 0]), np.ascontiguousarray(v[..., 1])


def batch_to_rows(grid_delta_batch, grid_beta_batch):
    """(B, Y, X, S) rotated object batches -> [b][z][x][y] pairs, float32."""
    pair = np.stack([grid_delta_batch, grid_beta_batch], axis=-1)
    return np.ascontiguousarray(pair.transpose(0, 3, 2, 1, 4).astype(np.float32))


def rows_to_batch(rows):
    """[b][z][x][y][2] -> (g_delta, g_beta) each (B, Y, X, S)."""
    v = rows.transpose(0, 3, 2, 1, 4)
    return np.ascontiguousarray(v[..., 0]), np.ascontiguousarray(v[..., 1])
