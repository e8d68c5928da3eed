"""rotation='trilinear' restated in numpy — test side, shared by tests/test_rigid_reference.py (no GPU), tests/test_gpu_rigid_ops.py
and tests/test_gpu_rigid.py, so that the three cannot drift apart.

The map (include/bdof.h, bdof_rotate_rigid): output voxel o = (x, z, y) of the beam frame samples the volume at p = M o + t in
index coordinates (x', z', y'), trilinearly over the 8 surrounding voxels; a tap outside the volume counts 0.  prm = the 12
numbers of (M | t), row by row.  Device layouts: volume rows [X][Z][Y], rotated rows [z][x][y].

taps() gives the eight (index, weight) pairs of every output voxel; rotate_rigid() gathers with them, rotate_rigid_adjoint() is
the scatter-add with the same weights.  weights='f32' forms them as the kernels do (three float32 factors, each the rounding of a
fraction or of one minus it, multiplied in float32) and sums in float32: the float32 restatement the solver-level bound is
derived from (composed_figure below)."""
import functools

import numpy as np

f32, f64 = np.float32, np.float64


def taps(prm, dims, weights='f64'):
    """prm: 12 numbers (M | t); dims = (NX, NZ, NY).  (idx, w), both [8][NX][NZ][NY]: the flat index (x' NZ + z') NY + y' of tap
    i = 4 ix + 2 iz + iy (0 where the tap is outside the volume) and its weight (0 there)."""
    m = np.asarray(prm, dtype=f64).reshape(3, 4)
    NX, NZ, NY = dims
    x, z, y = np.meshgrid(np.arange(NX, dtype=f64), np.arange(NZ, dtype=f64), np.arange(NY, dtype=f64), indexing='ij')
    i0, fr = [], []
    for a in range(3):
        p = ((m[a, 0] * x + m[a, 3]) + m[a, 1] * z) + m[a, 2] * y
        fl = np.floor(p)
        i0.append(fl.astype(np.int64))
        fr.append(p - fl)
    if weights == 'f32':
        fac = [((1.0 - f).astype(f32), f.astype(f32)) for f in fr]
    else:
        fac = [(1.0 - f, f) for f in fr]
    idx = np.zeros((8, NX, NZ, NY), dtype=np.int64)
    w = np.zeros((8, NX, NZ, NY), dtype=f32 if weights == 'f32' else f64)
    for i in range(8):
        ix, iz, iy = i >> 2, (i >> 1) & 1, i & 1
        px, pz, py = i0[0] + ix, i0[1] + iz, i0[2] + iy
        inside = (px >= 0) & (px < NX) & (pz >= 0) & (pz < NZ) & (py >= 0) & (py < NY)
        idx[i] = np.where(inside, (px * NZ + pz) * NY + py, 0)
        w[i] = np.where(inside, (fac[0][ix] * fac[1][iz]) * fac[2][iy], 0)
    return idx, w


def rotate_rigid(vol, prm, weights='f64'):
    """vol [NX][NZ][NY][C] -> the rotated object in the device's row order, [NZ][NX][NY][C] (float64; float32 with weights='f32')."""
    NX, NZ, NY, C = vol.shape
    idx, w = taps(prm, (NX, NZ, NY), weights)
    flat = np.asarray(vol, dtype=w.dtype).reshape(-1, C)
    out = np.zeros((NX, NZ, NY, C), dtype=w.dtype)
    for i in range(8):
        out += w[i][..., None] * flat[idx[i]]
    return out.transpose(1, 0, 2, 3)


def rotate_rigid_adjoint(g, prm, weights='f64'):
    """g [NZ][NX][NY][C], a rotated-frame array -> [NX][NZ][NY][C]: the scatter-add with rotate_rigid's weights."""
    NZ, NX, NY, C = g.shape
    idx, w = taps(prm, (NX, NZ, NY), weights)
    gg = np.asarray(g, dtype=w.dtype).transpose(1, 0, 2, 3)
    out = np.zeros((NX * NZ * NY, C), dtype=w.dtype)
    for i in range(8):
        np.add.at(out, idx[i].reshape(-1), (w[i][..., None] * gg).reshape(-1, C))
    return out.reshape(NX, NZ, NY, C)


def rotate_volume(obj, prm, weights='f64'):
    """obj (Y, X, Z, C) -> rotated (Y, X, Z, C): oracle.rotate_bilinear's interface."""
    return rotate_rigid(np.asarray(obj).transpose(1, 2, 0, 3), prm, weights).transpose(2, 1, 0, 3)


def rotate_volume_adjoint(g_rot, prm, weights='f64'):
    """g_rot (Y, X, Z, C) in the rotated frame -> (Y, X, Z, C) in the volume's."""
    return rotate_rigid_adjoint(np.asarray(g_rot).transpose(2, 1, 0, 3), prm, weights).transpose(2, 0, 1, 3)


# ---- the per-element bound of the device against the float64 restatement --------------------------------------------------------------
# A device weight is a product of three float32 factors in [0, 1], each within 2^-25 of its float64 value, multiplied twice in
# float32: absolute error <= 6 * 2^-24 (generously).  n <= 8 fused products are then added in float32, each step rounding the
# running sum (<= 2^-24 sum |w_i| |g_i|); `scale` and, when accumulating, the prior value add one rounding each (the "+ 4").  Hence
#     |device - reference| <= 2^-24 (6 sum |g_i| + (n + 4) sum |w_i| |g_i|),   times scale, + 2^-24 |prior| when accumulating.
# At zero tilt and roll the y factor is exactly 0 or 1, n <= 4 and a weight has two inexact factors: 4 sum |g_i| (weight_terms=4).
def forward_terms(vol, prm):
    """vol [NX][NZ][NY][C] -> (reference, sum |g_i|, sum |w_i| |g_i|, n), the first three [NZ][NX][NY][C], n [NZ][NX][NY][1]"""
    NX, NZ, NY, C = vol.shape
    idx, w = taps(prm, (NX, NZ, NY))
    flat = np.asarray(vol, dtype=f64).reshape(-1, C)
    ref, sg, swg = np.zeros((3, NX, NZ, NY, C))
    n = np.zeros((NX, NZ, NY, 1))
    for i in range(8):
        v = flat[idx[i]]
        live = (w[i] != 0)[..., None]
        ref += w[i][..., None] * v
        sg += live * np.abs(v)
        swg += w[i][..., None] * np.abs(v)
        n += live
    return tuple(a.transpose(1, 0, 2, 3) for a in (ref, sg, swg, n))


def adjoint_terms(g, prm):
    """g [NZ][NX][NY][C] -> (reference, sum |g_i|, sum |w_i| |g_i|, n), the first three [NX][NZ][NY][C], n [NX][NZ][NY][1]"""
    NZ, NX, NY, C = g.shape
    idx, w = taps(prm, (NX, NZ, NY))
    gg = np.asarray(g, dtype=f64).transpose(1, 0, 2, 3)
    ref, sg, swg = np.zeros((3, NX * NZ * NY, C))
    n = np.zeros((NX * NZ * NY, 1))
    for i in range(8):
        live = (w[i] != 0)[..., None]
        k = idx[i].reshape(-1)
        np.add.at(ref, k, (w[i][..., None] * gg).reshape(-1, C))
        np.add.at(sg, k, (live * np.abs(gg)).reshape(-1, C))
        np.add.at(swg, k, (w[i][..., None] * np.abs(gg)).reshape(-1, C))
        np.add.at(n, k, live.reshape(-1, 1).astype(f64))
    return ref.reshape(NX, NZ, NY, C), sg.reshape(NX, NZ, NY, C), swg.reshape(NX, NZ, NY, C), n.reshape(NX, NZ, NY, 1)


def element_bound(sg, swg, n, weight_terms=6):
    return 2.0 ** -24 * (weight_terms * sg + (n + 4) * swg)


# ---- geometries written by hand ---------------------------------------------------------------------------------------------------------
def hand_written(X, Z, Y):
    """[(keywords of util.rigid_geometry, M, t)]: matrices worked out on paper from the issue's three factor maps."""
    cx, cz, cy = (X - 1) / 2., (Z - 1) / 2., (Y - 1) / 2.
    h = np.pi / 2

    def t_of(M, c_o):
        return np.array([cx, cz, cy]) - np.asarray(M, dtype=f64) @ np.asarray(c_o)
    eye = [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
    turn = [[0, 1, 0], [-1, 0, 0], [0, 0, 1]]            # theta = pi / 2: x' = z, z' = -x
    tilt = [[1, 0, 0], [0, 0, 1], [0, -1, 0]]            # axis_tilt = pi / 2: z' = y, y' = -z
    roll = [[0, 0, 1], [0, 1, 0], [-1, 0, 0]]            # axis_roll = pi / 2: x' = y, y' = -x
    turn_tilt = [[0, 0, 1], [-1, 0, 0], [0, -1, 0]]      # M0(pi / 2) T(pi / 2): x' = z'' = y, z' = -x, y' = -z
    tilt_roll = [[0, 0, 1], [-1, 0, 0], [0, -1, 0]]      # T(pi / 2) R(pi / 2): x' = y, z' = y'' = -x, y' = -z
    return [
        (dict(theta=0.), eye, np.zeros(3)),
        (dict(theta=0., center=2.25), eye, np.array([cx - 2.25, 0., 0.])),
        (dict(theta=h), turn, t_of(turn, [cx, cz, cy])),
        (dict(theta=0., axis_tilt=h), tilt, t_of(tilt, [cx, cz, cy])),
        (dict(theta=0., axis_roll=h), roll, t_of(roll, [cx, cz, cy])),
        (dict(theta=h, axis_tilt=h), turn_tilt, t_of(turn_tilt, [cx, cz, cy])),
        (dict(theta=0., axis_tilt=h, axis_roll=h, center=1.5), tilt_roll, t_of(tilt_roll, [1.5, cz, cy])),
    ]


def signed_permutations():
    """The 24 proper rotations of the cube as integer matrices: the quarter turns about each axis and their products."""
    gens = [np.array(m) for m in ([[0, 1, 0], [-1, 0, 0], [0, 0, 1]], [[1, 0, 0], [0, 0, 1], [0, -1, 0]], [[0, 0, 1], [0, 1, 0], [-1, 0, 0]])]
    found = {tuple(np.eye(3, dtype=int).reshape(-1)): np.eye(3, dtype=int)}
    grew = True
    while grew:
        grew = False
        for m in list(found.values()):
            for g in gens:
                p = g @ m
                if tuple(p.reshape(-1)) not in found:
                    found[tuple(p.reshape(-1))] = p
                    grew = True
    out = [found[k] for k in sorted(found)]
    assert len(out) == 24 and all(round(float(np.linalg.det(m))) == 1 for m in out)
    return out


def random_rigid(rng):
    """A proper rotation drawn uniformly (QR of a gaussian matrix, sign-fixed)."""
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


# ---- the solver-level case: geometry, data, and where its gradient bound comes from ---------------------------------------------------
N, N_THETA, MB = 64, 7, 3
IDX = (1, 3, 6)
TILT, ROLL, CENTER = 0.5, 0.03, 30.4
E_EV, PSIZE_CM = 5000., 1e-7
# The bound of the solver-level gradient test by the rule of tests/gradient_cases.py (bound_rule): 2e-5 unless the float32 /
# complex64 restatement of the composed case (composed_figure) exceeds half of it.  tests/test_rigid_reference.py recomputes the
# figure on the CPU and holds this constant to the rule; no device figure enters.
SOLVER_GRADIENT_BOUND = 2e-5


def solver_theta():
    return -np.linspace(0, 2 * np.pi, N_THETA).astype(f32).astype(f64)          # as rotation='bilinear' (tests/test_gpu_bilinear.py)


def solver_geometry():
    from beyond_dof_amd import util
    return util.rigid_geometry(solver_theta(), (N, N, N), TILT, ROLL, CENTER)


@functools.lru_cache(maxsize=None)
def solver_problem(fp):
    """The 64^3 case of tests/test_gpu_rigid.py: a float32 object inside a margin, the three angles IDX under the tilted, rolled
    and off-centre axis, a plane wave, amplitudes |ref| U(0, 2) (reference_model.measurement_wide); float64 loss and gradient
    through the restatement composed with the oracle.  Computed once, shared, read only."""
    from oracle import bdof_oracle as orc
    import reference_model as ref_model
    rng = np.random.default_rng(7)
    od = np.zeros((N, N, N))
    od[:, 8:-8, 8:-8] = rng.uniform(0, 2e-6, size=(N, N - 16, N - 16))
    od = od.astype(f32).astype(f64)
    ob = (f32(0.1) * od.astype(f32)).astype(f64)
    prm = solver_geometry()[list(IDX)]
    one, zero = np.ones((N, N)), np.zeros((N, N))
    obj = np.stack([od, ob], axis=3)
    rot = np.stack([rotate_volume(obj, p) for p in prm])
    wave, _ = orc.multislice_propagate_batch_numpy(rot[..., 0], rot[..., 1], one, zero, E_EV, PSIZE_CM, fp, rot[..., 0].shape,
                                                   return_probe_array=False)
    meas = ref_model.measurement_wide(wave, 0).astype(f32).astype(f64)
    loss, gd, gb = orc.multislice_loss_and_grad(rot[..., 0], rot[..., 1], one, zero, E_EV, PSIZE_CM, meas, fp)
    g = sum(rotate_volume_adjoint(np.stack([gd[b], gb[b]], axis=3), p) for b, p in enumerate(prm))
    out = dict(od=od, ob=ob, prm=prm, rot=rot, wave=wave, meas=meas, loss=loss, gd=g[..., 0], gb=g[..., 1])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def composed_figure(fp):
    """The worst gradient error of the composed case in float32: rotation with float32 weights and sums, then
    modulation_reference.c64_loss_and_grad, then the float32 adjoint, against solver_problem's float64 gradient."""
    import modulation_reference as mref
    p = solver_problem(fp)
    obj = np.stack([p['od'], p['ob']], axis=3).astype(f32)
    rot = np.stack([rotate_volume(obj, q, 'f32') for q in p['prm']])
    assert rot.dtype == f32
    one, zero = np.ones((N, N)), np.zeros((N, N))
    _, loss, gd, gb = mref.c64_loss_and_grad(rot[..., 0], rot[..., 1], one, zero, p['meas'], fp)
    g = np.zeros((N, N, N, 2), f32)
    for b, q in enumerate(p['prm']):
        g = g + rotate_volume_adjoint(np.stack([gd[b], gb[b]], axis=3), q, 'f32')
    assert g.dtype == f32
    rel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))
    return max(rel(g[..., 0], p['gd']), rel(g[..., 1], p['gb']))


# ---- the ptychography case: one angle under a tilted axis, windows, far field -----------------------------------------------------------
PTY_SHAPE = (64, 64, 32)                                  # (Y, X, Z)
PTY_N_THETA, PTY_THETA, PTY_TILT = 4, 2, 0.5
PTY_POS = np.array([(16, 16), (16, 32), (16, 48), (32, 16), (32, 32), (32, 48), (48, 16), (10, 50), (60, 8)])   # the last two overhang
# By the same rule as SOLVER_GRADIENT_BOUND, per probe size, from ptycho_composed_figure on the CPU (test_rigid_reference.py).
# The float64 first step rotates in float32 like every other step: it is held to the same bound.
# The restatement reaches 1.6e-5 (32^2 probe) and 1.3e-5 (64^2): above half of 2e-5, so the rule gives twice the figure rounded
# up to one significant digit.
PTYCHO_GRADIENT_BOUND = {32: 4e-5, 64: 3e-5}


def ptycho_theta():
    return -np.linspace(0, 2 * np.pi, PTY_N_THETA).astype(f32).astype(f64)


def ptycho_windows(rot, psz):
    """rot (Y, X, Z, C) -> the windows [n_pos][psz][psz][Z][C] at PTY_POS, zeros beyond the volume"""
    half = psz // 2
    pad = np.pad(rot, ((psz, psz), (psz, psz), (0, 0), (0, 0)), mode='constant')
    return np.stack([pad[p[0] + psz - half:p[0] + psz - half + psz, p[1] + psz - half:p[1] + psz - half + psz] for p in PTY_POS])


def ptycho_windows_adjoint(g_sub, psz, dtype=f64):
    """[n_pos][psz][psz][Z][C] -> (Y, X, Z, C): overlap-add of the windows, what falls beyond the volume dropped"""
    Y, X, Z = PTY_SHAPE
    half = psz // 2
    pad = np.zeros((Y + 2 * psz, X + 2 * psz, Z, g_sub.shape[-1]), dtype=dtype)
    for b, p in enumerate(PTY_POS):
        pad[p[0] + psz - half:p[0] + psz - half + psz, p[1] + psz - half:p[1] + psz - half + psz] += g_sub[b]
    return pad[psz:psz + Y, psz:psz + X]


@functools.lru_cache(maxsize=None)
def ptycho_problem(psz):
    """A (64, 64, 32) float32 object, angle PTY_THETA of 4 under axis_tilt = 0.5, a psz^2 gaussian probe at 9 positions, far-field
    amplitudes |ref| U(0, 2): float64 waves, loss and volume-frame gradient through the restatement, the windows and the model."""
    from beyond_dof_amd import util
    from oracle import bdof_oracle as orc
    import reference_model as ref_model
    Y, X, Z = PTY_SHAPE
    rng = np.random.default_rng(17)
    od = np.zeros(PTY_SHAPE)
    od[:, 6:-6, 4:-4] = rng.uniform(0, 2e-6, size=(Y, X - 12, Z - 8))
    od = od.astype(f32).astype(f64)
    ob = (f32(0.1) * od.astype(f32)).astype(f64)
    prm = util.rigid_geometry(ptycho_theta(), PTY_SHAPE, PTY_TILT)[PTY_THETA]
    pr, pi = [np.asarray(v).astype(f32).astype(f64) for v in orc.gaussian_probe((psz, psz), psz / 10., psz / 10., 0.5)]
    subs = ptycho_windows(rotate_volume(np.stack([od, ob], axis=3), prm), psz)
    wave, _ = ref_model.forward(subs[..., 0], subs[..., 1], pr, pi, E_EV, PSIZE_CM, 'inf')
    meas = ref_model.measurement_wide(wave, 0).astype(f32).astype(f64)
    loss, gd, gb, _, _ = ref_model.loss_and_grad(subs[..., 0], subs[..., 1], pr, pi, E_EV, PSIZE_CM, meas, 'inf')
    g = rotate_volume_adjoint(ptycho_windows_adjoint(np.stack([gd, gb], axis=-1), psz), prm)
    out = dict(od=od, ob=ob, prm=prm, pr=pr, pi=pi, wave=wave, meas=meas, loss=float(loss), gd=g[..., 0], gb=g[..., 1])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def ptycho_composed_figure(psz):
    """The worst gradient error of the ptychography case in float32 / complex64: rotation, windows, c64_loss_and_grad, overlap-add,
    adjoint, against ptycho_problem's float64 gradient."""
    import modulation_reference as mref
    p = ptycho_problem(psz)
    rot = rotate_volume(np.stack([p['od'], p['ob']], axis=3).astype(f32), p['prm'], 'f32')
    subs = ptycho_windows(rot, psz)
    _, loss, gd, gb = mref.c64_loss_and_grad(subs[..., 0], subs[..., 1], p['pr'], p['pi'], p['meas'], 'inf')
    g = rotate_volume_adjoint(ptycho_windows_adjoint(np.stack([gd, gb], axis=-1), psz, f32), p['prm'], 'f32')
    assert rot.dtype == f32 and g.dtype == f32
    rel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))
    return max(rel(g[..., 0], p['gd']), rel(g[..., 1], p['gb']))
