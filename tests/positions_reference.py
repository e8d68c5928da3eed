"""Ptychography windows at fractional origins restated in numpy float64 — test side, shared by tests/test_positions_reference.py
(no GPU), tests/test_gpu_window_ops.py and tests/test_gpu_positions.py.

Device layouts (include/bdof.h, bdof_window_stack): rotated frame R [S][volNX][volNY][C], windows and their gradients
[B][S][NX][NY][C], origin[b] = (u, v), the pixel coordinate of window b's first voxel along x and along y:

    i0 = floor(u), fx = u - i0;  j0 = floor(v), fy = v - j0;  wx = (1 - fx, fx), wy = (1 - fy, fy)
    W_b[z][i][j]   = sum_{a,c} wx_a wy_c R[z][i0 + i + a][j0 + j + c]                          (window_cut)
    pad[z][xg][y]  = sum_b sum_{a,c} wx_a wy_c g_b[z][xg - i0_b - a][y - j0_b - c]             (window_cut_adjoint)
    dL/du_b        = sum g_b[z][i][j] sum_c wy_c (R[z][i0+i+1][j0+j+c] - R[z][i0+i][j0+j+c])   (position_terms; v: x and y exchanged)

a tap outside the frame counting 0, the derivative taken inside the cell floor gives (the right-hand derivative on a lattice line).

The bounds of the device results, derived here and not measured (the argument of rigid_reference.element_bound and
geometry_reference.entry_bound):
  * forward and adjoint: a device weight is the float32 product of two float32 factors in [0, 1], each within 2^-25 of its float64
    value: absolute error <= 2 * 2^-25 + 2^-25 (the product's rounding) < 4 * 2^-24 (generously) on every live tap: 4 * 2^-24 on
    SG = sum |v_i|; n live taps are added as fused products in float32, each step rounding the running sum (<= 2^-24 sum |w_i| |v_i|),
    `scale` and the accumulation add one rounding each ("+ 4", generously): (n + 4) * 2^-24 on SWG = sum |w_i| |v_i|.
        |device - reference| <= 2^-24 (4 SG + (n + 4) SWG)                                                   (element_bound)
    Through a rotation table the adjoint adds the pad rows that feed one volume row in float32: the rows' own bounds add, and the
    m rows cost m more roundings of the running sum: n := sum n + m (table_adjoint_terms).
  * derivative: a coefficient is ONE float32 factor, within 2^-25 of its float64 value: 1 * 2^-24 on SG = sum |g| |V| over live
    taps; n <= 4 fused products in float32 and the product and fused product of the two channels with g: (n + 4) * 2^-24 on
    SWG = sum |coefficient| |g| |V|; the sums over voxels are float64 (2^-53 per step: covered by the generosity above).
        |device - reference| <= 2^-24 (SG + (n + 4)-weighted SWG)                                             (entry_bound)
Nothing a device returned enters."""
import numpy as np

f64 = np.float64


def cells(origin):
    """origin (B, 2) -> (i0 (B, 2) int, w (B, 2, 2)): per window the lower corner (i0, j0) and the factors w[b][axis] = (1 - f, f)"""
    o = np.asarray(origin, dtype=f64).reshape(-1, 2)
    fl = np.floor(o)
    fr = o - fl
    return fl.astype(np.int64), np.stack([1.0 - fr, fr], axis=-1)


def _tap(R, i0, NX, NY, a, c):
    """R[z][i0 + i + a][j0 + j + c] as [S][NX][NY][C] with 0 outside the frame, and the mask [NX][NY] of the taps inside"""
    S, VX, VY, C = R.shape
    xs, ys = i0[0] + np.arange(NX) + a, i0[1] + np.arange(NY) + c
    mask = ((xs >= 0) & (xs < VX))[:, None] & ((ys >= 0) & (ys < VY))[None, :]
    v = R[:, np.clip(xs, 0, VX - 1)][:, :, np.clip(ys, 0, VY - 1)]
    return v * mask[None, :, :, None], mask


def forward_terms(R, origin, NX, NY):
    """(reference, sum |v_i|, sum |w_i| |v_i|, n): the first three [B][S][NX][NY][C], n [B][1][NX][NY][1], over the live taps"""
    R = np.asarray(R, dtype=f64)
    i0, w = cells(origin)
    B, (S, VX, VY, C) = len(i0), R.shape
    ref, sg, swg = np.zeros((3, B, S, NX, NY, C))
    n = np.zeros((B, 1, NX, NY, 1))
    for b in range(B):
        for a in range(2):
            for c in range(2):
                wt = w[b, 0, a] * w[b, 1, c]
                v, mask = _tap(R, i0[b], NX, NY, a, c)
                live = mask & (wt != 0)
                ref[b] += wt * v
                sg[b] += live[None, :, :, None] * np.abs(v)
                swg[b] += wt * np.abs(v)
                n[b, 0, :, :, 0] += live
    return ref, sg, swg, n


def window_cut(R, origin, NX, NY):
    return forward_terms(R, origin, NX, NY)[0]


def adjoint_terms(g, origin, VX, VY):
    """g [B][S][NX][NY][C] -> (reference, sum |g_i|, sum |w_i| |g_i|, n): [S][VX][VY][C], n [1][VX][VY][1]; windows in ascending b"""
    g = np.asarray(g, dtype=f64)
    B, S, NX, NY, C = g.shape
    i0, w = cells(origin)
    ref, sg, swg = np.zeros((3, S, VX, VY, C))
    n = np.zeros((1, VX, VY, 1))
    for b in range(B):
        for a in range(2):
            for c in range(2):
                wt = w[b, 0, a] * w[b, 1, c]
                x0, y0 = i0[b, 0] + a, i0[b, 1] + c                  # frame position of the window's (0, 0) under this tap
                xl, xh = max(0, -x0), min(NX, VX - x0)
                yl, yh = max(0, -y0), min(NY, VY - y0)
                if xl >= xh or yl >= yh:
                    continue
                src = g[b][:, xl:xh, yl:yh]
                dst = (slice(None), slice(x0 + xl, x0 + xh), slice(y0 + yl, y0 + yh))
                ref[dst] += wt * src
                if wt != 0:
                    sg[dst] += np.abs(src)
                    swg[dst] += wt * np.abs(src)
                    n[0, x0 + xl:x0 + xh, y0 + yl:y0 + yh, 0] += 1
    return ref, sg, swg, n


def window_cut_adjoint(g, origin, VX, VY):
    return adjoint_terms(g, origin, VX, VY)[0]


def element_bound(sg, swg, n):
    return 2.0 ** -24 * (4 * sg + (n + 4) * swg)


def table_adjoint_terms(terms, tab, n_dest):
    """adjoint_terms' four arrays taken through a rotation table tab [S][VX] (-> volume row): [n_dest][VY][C] each, with
    n = sum of the rows' n + the number of rows added (the float32 running sum of k_rot_adjoint)"""
    ref, sg, swg, n = terms
    S, VX, VY, C = ref.shape
    dest = np.asarray(tab).reshape(-1)
    out = []
    for a in (ref, sg, swg):
        o = np.zeros((n_dest, VY, C))
        np.add.at(o, dest, a.reshape(S * VX, VY, C))
        out.append(o)
    cnt = np.zeros((n_dest, VY, 1))
    np.add.at(cnt, dest, np.broadcast_to(n, (S, VX, VY, 1)).reshape(S * VX, VY, 1) + 1.0)
    return out[0], out[1], out[2], cnt


def position_terms(R, g, origin):
    """R [S][VX][VY][C], g [B][S][NX][NY][C] -> (d, SG, SWG, T), each (B, 2) = (d/du, d/dv): the derivative and, over its live
    taps, SG = sum |g| |V|, SWG = sum (n + 4) |coefficient| |g| |V| and T = sum |coefficient| |g| |V|"""
    R, g = np.asarray(R, dtype=f64), np.asarray(g, dtype=f64)
    B, S, NX, NY, C = g.shape
    i0, w = cells(origin)
    d, SG, SWG, T = np.zeros((4, B, 2))
    for b in range(B):
        for k in range(2):                               # 0: d/du (the x tap's bit decides the sign, the y factor weighs), 1: d/dv
            dv = np.zeros((S, NX, NY, C))
            sabs, wabs = np.zeros((2, S, NX, NY, C))
            cnt = np.zeros((1, NX, NY, 1))
            for a in range(2):
                for c in range(2):
                    bit, coef = (a, w[b, 1, c]) if k == 0 else (c, w[b, 0, a])
                    v, mask = _tap(R, i0[b], NX, NY, a, c)
                    live = mask & (coef != 0)
                    dv += (coef if bit else -coef) * v
                    sabs += live[None, :, :, None] * np.abs(v)
                    wabs += coef * np.abs(v)
                    cnt[0, :, :, 0] += live
            ag = np.abs(g[b])
            d[b, k] = np.sum(g[b] * dv)
            SG[b, k] = np.sum(ag * sabs)
            SWG[b, k] = np.sum((cnt + 4) * ag * wabs)
            T[b, k] = np.sum(ag * wabs)
    return d, SG, SWG, T


def entry_bound(SG, SWG):
    return 2.0 ** -24 * (SG + SWG)


# ---- the composed model: rotate, cut at fractional origins, far-field loss and gradient, adjoints --------------------------------------
def to_frame(obj_rot):
    """rotated object (Y, X, Z, C) -> R [Z][X][Y][C]"""
    return np.asarray(obj_rot).transpose(2, 1, 0, 3)


def from_frame(R):
    """(a contiguous copy: the oracle's rotation adjoint writes through a reshaped view of an array laid out like its argument)"""
    return np.ascontiguousarray(np.asarray(R).transpose(2, 1, 0, 3))


def origins(probe_pos, offsets, probe_size):
    """(u, v) per window: probe_pos and offsets in (y, x) order, half = probe_size // 2 as the solver's"""
    at = np.asarray(probe_pos, dtype=f64) + np.asarray(offsets, dtype=f64)
    half = (np.array(probe_size) / 2).astype(int)
    return np.stack([at[:, 1] - half[1], at[:, 0] - half[0]], axis=1)


def nearest(coord):
    from oracle import bdof_oracle as orc
    return (lambda obj: orc.apply_rotation(obj, coord)), (lambda g: orc.apply_rotation_adjoint(g, coord))


def ptycho_loss_and_grad(obj_delta, obj_beta, rotation, probe_pos, offsets, probe_size, probe_real, probe_imag, energy_ev, psize_cm, meas_abs,
                         want_positions=True):
    """rotation = (rotate, rotate_adjoint) on (Y, X, Z, C) arrays (nearest(coord), or rigid_reference's pair under a map).
    Returns dict(loss, gd, gb — the volume-frame gradient —, dpos (B, 2) in (y, x) order with its term sums SG, SWG, T, wave)."""
    import reference_model as ref_model
    rotate, rotate_adjoint = rotation
    py, px = int(probe_size[0]), int(probe_size[1])
    R = to_frame(rotate(np.stack([obj_delta, obj_beta], axis=3)))
    org = origins(probe_pos, offsets, probe_size)
    subs = window_cut(R, org, px, py).transpose(0, 3, 2, 1, 4)                      # (B, py, px, Z, C)
    loss, gd, gb, _, wave = ref_model.loss_and_grad(subs[..., 0], subs[..., 1], probe_real, probe_imag, energy_ev, psize_cm, meas_abs, 'inf')
    g = np.stack([gd, gb], axis=-1).transpose(0, 3, 2, 1, 4)                        # [B][S][NX][NY][C]
    g_vol = rotate_adjoint(from_frame(window_cut_adjoint(g, org, R.shape[1], R.shape[2])))
    out = dict(loss=float(loss), gd=g_vol[..., 0], gb=g_vol[..., 1], wave=wave)
    if want_positions:
        d, SG, SWG, T = position_terms(R, g, org)
        out.update(dpos=d[:, ::-1], SG=SG[:, ::-1], SWG=SWG[:, ::-1], T=T[:, ::-1])
    return out


def ptycho_loss(obj_delta, obj_beta, rotation, probe_pos, offsets, probe_size, probe_real, probe_imag, energy_ev, psize_cm, meas_abs):
    import reference_model as ref_model
    py, px = int(probe_size[0]), int(probe_size[1])
    R = to_frame(rotation[0](np.stack([obj_delta, obj_beta], axis=3)))
    subs = window_cut(R, origins(probe_pos, offsets, probe_size), px, py).transpose(0, 3, 2, 1, 4)
    return ref_model.loss_only(subs[..., 0], subs[..., 1], probe_real, probe_imag, energy_ev, psize_cm, meas_abs, 'inf')


def ptycho_forward(obj_delta, obj_beta, rotation, probe_pos, offsets, probe_size, probe_real, probe_imag, energy_ev, psize_cm):
    import reference_model as ref_model
    py, px = int(probe_size[0]), int(probe_size[1])
    R = to_frame(rotation[0](np.stack([obj_delta, obj_beta], axis=3)))
    subs = window_cut(R, origins(probe_pos, offsets, probe_size), px, py).transpose(0, 3, 2, 1, 4)
    return ref_model.forward(subs[..., 0], subs[..., 1], probe_real, probe_imag, energy_ev, psize_cm, 'inf')[0]


# ---- the solver-level cases (tests/test_gpu_positions.py) and where their bounds come from -----------------------------------------------
# Object, probe (32^2) and the 9 positions of rigid_reference.ptycho_problem with offsets U(-0.9, 0.9) on every position, under the
# lookup-table rotation ('nearest') and the rigid map of that problem ('trilinear'); amplitudes |ref| U(0, 2).
# LOSS_BOUND on the loss.  GRADIENT_BOUND on rel(g, g_ref) of the volume gradient and, per entry, on |d - d_ref| / T of the position
# gradient (T the sum of the absolute values of the entry's terms): the project's 2e-5 (geometry_reference.PTYCHO_GEOMETRY_GRADIENT_BOUND)
# unless the float32 / complex64 restatement of the case (composed_figure, on the CPU) says the float32 path cannot hold it — then
# three times that figure.  tests/test_positions_reference.py recomputes the figures and holds these constants to the rule; no
# device figure enters.  Figures reached by the restatement: see COMPOSED_FIGURE below.
PSZ = 32
LOSS_BOUND = 1e-5
GRADIENT_BOUND = 2e-5
COMPOSED_FIGURE = {'nearest': (1.57e-5, 7.4e-7), 'trilinear': (1.55e-5, 4.1e-7)}        # composed_figure(kind), as computed on the CPU
f32 = np.float32


def solver_rotation(kind):
    import rigid_reference as rr
    from beyond_dof_amd import util
    if kind == 'nearest':
        return nearest(util.rotation_lookup(rr.PTY_SHAPE, rr.PTY_N_THETA)[rr.PTY_THETA])
    prm = rr.ptycho_problem(PSZ)['prm']
    return (lambda obj: rr.rotate_volume(obj, prm)), (lambda g: rr.rotate_volume_adjoint(g, prm))


def solver_offsets():
    import rigid_reference as rr
    return np.random.default_rng(41).uniform(-0.9, 0.9, size=(len(rr.PTY_POS), 2))


_problems = {}


def solver_problem(kind, zero=False):
    """float64 data, loss, volume gradient and position gradient of the case; computed once, shared, read only"""
    import rigid_reference as rr
    import reference_model as ref_model
    if (kind, zero) not in _problems:
        p = rr.ptycho_problem(PSZ)
        off = np.zeros((len(rr.PTY_POS), 2)) if zero else solver_offsets()
        rot = solver_rotation(kind)
        args = (p['od'], p['ob'], rot, rr.PTY_POS, off, (PSZ, PSZ), p['pr'], p['pi'], rr.E_EV, rr.PSIZE_CM)
        meas = ref_model.measurement_wide(ptycho_forward(*args), 0).astype(f32).astype(f64)
        out = dict(ptycho_loss_and_grad(*args, meas), meas=meas, off=off)
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _problems[kind, zero] = out
    return _problems[kind, zero]


def window_cut32(R, origin, NX, NY):
    """window_cut as the kernel forms it: float32 factors, their float32 product, float32 sums"""
    R = np.asarray(R, dtype=f32)
    i0, w = cells(origin)
    w = w.astype(f32)
    out = np.zeros((len(i0), R.shape[0], NX, NY, R.shape[3]), dtype=f32)
    for b in range(len(i0)):
        for a in range(2):
            for c in range(2):
                out[b] += (w[b, 0, a] * w[b, 1, c]) * _tap(R, i0[b], NX, NY, a, c)[0].astype(f32)
    return out


def window_cut_adjoint32(g, origin, VX, VY):
    g = np.asarray(g, dtype=f32)
    B, S, NX, NY, C = g.shape
    i0, w = cells(origin)
    w = w.astype(f32)
    pad = np.zeros((S, VX, VY, C), dtype=f32)
    for b in range(B):
        for a in range(2):
            for c in range(2):
                x0, y0 = i0[b, 0] + a, i0[b, 1] + c
                xl, xh, yl, yh = max(0, -x0), min(NX, VX - x0), max(0, -y0), min(NY, VY - y0)
                if xl < xh and yl < yh:
                    pad[:, x0 + xl:x0 + xh, y0 + yl:y0 + yh] += (w[b, 0, a] * w[b, 1, c]) * g[b][:, xl:xh, yl:yh]
    return pad


def position32(R, g, origin):
    """the derivative with float32 coefficients, tap sums and products (the sums over voxels float64), (B, 2) = (d/du, d/dv)"""
    R, g = np.asarray(R, dtype=f32), np.asarray(g, dtype=f32)
    B, S, NX, NY, C = g.shape
    i0, w = cells(origin)
    w = w.astype(f32)
    d = np.zeros((B, 2))
    for b in range(B):
        for k in range(2):
            dv = np.zeros((S, NX, NY, C), dtype=f32)
            for a in range(2):
                for c in range(2):
                    bit, coef = (a, w[b, 1, c]) if k == 0 else (c, w[b, 0, a])
                    dv += (coef if bit else -coef) * _tap(R, i0[b], NX, NY, a, c)[0].astype(f32)
            q = g[b][..., 0] * dv[..., 0] + g[b][..., 1] * dv[..., 1]
            d[b, k] = np.sum(q.astype(f64))
    return d


def composed_figure(kind):
    """The worst errors of the case in float32 / complex64 — rotation with float32 weights, float32 cut,
    modulation_reference.c64_loss_and_grad, float32 adjoints and derivative — against solver_problem's float64 figures:
    (volume gradient: the larger rel of g_delta, g_beta; position gradient: the largest |d - d_ref| / T)"""
    import modulation_reference as mref
    import rigid_reference as rr
    from beyond_dof_amd import util
    p, ref = rr.ptycho_problem(PSZ), solver_problem(kind)
    obj = np.stack([p['od'], p['ob']], axis=3).astype(f32)
    if kind == 'nearest':
        rotate, back = nearest(util.rotation_lookup(rr.PTY_SHAPE, rr.PTY_N_THETA)[rr.PTY_THETA])
    else:
        rotate, back = (lambda o: rr.rotate_volume(o, p['prm'], 'f32')), (lambda g: rr.rotate_volume_adjoint(g, p['prm'], 'f32'))
    R = to_frame(rotate(obj))
    org = origins(rr.PTY_POS, ref['off'], (PSZ, PSZ))
    subs = window_cut32(R, org, PSZ, PSZ).transpose(0, 3, 2, 1, 4)
    _, loss, gd, gb = mref.c64_loss_and_grad(subs[..., 0], subs[..., 1], p['pr'], p['pi'], ref['meas'], 'inf')
    g = np.stack([gd, gb], axis=-1).astype(f32).transpose(0, 3, 2, 1, 4)
    g_vol = back(from_frame(window_cut_adjoint32(g, org, R.shape[1], R.shape[2])))
    assert g_vol.dtype == f32 and subs.dtype == f32
    rel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))
    d = position32(R, g, org)[:, ::-1]
    return max(rel(g_vol[..., 0], ref['gd']), rel(g_vol[..., 1], ref['gb'])), float(np.max(np.abs(d - ref['dpos']) / ref['T']))
