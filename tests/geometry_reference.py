"""The derivative of a loss with respect to the rigid map of rotation='trilinear', restated in numpy float64 — test side, shared by
tests/test_geometry_reference.py (no GPU), tests/test_gpu_geometry_ops.py and tests/test_gpu_geometry.py.

With rigid_reference's conventions (volume [NX][NZ][NY][C], rotated-frame arrays [NZ][NX][NY][C], prm = the 12 numbers of (M | t),
output voxel o = (x, z, y) sampling the volume at p = M o + t) and o~ = (x, z, y, 1):

    dL/d prm[a][j] = sum_o q_a(o) o~_j,        q_a(o) = sum_c g_c(o) dV_c/dp_a (p(o)),

dV/dp_a taken inside the cell floor(p): over the cell's 8 corners, -1 or +1 by the corner's bit along a, times the product of the
OTHER two axes' factors, times V(corner); a corner outside the volume counts 0 as in rigid_reference.taps.  A point on a lattice
plane belongs to the cell floor gives it (the right-hand derivative).

param_terms returns the 12 entries together with the sums of absolute values of their terms, from which the bounds come.

The per-entry bound of the device (entry_bound), by the argument of rigid_reference.element_bound:
  * the device's weight along a is the float32 product of two float32 factors in [0, 1], each within 2^-25 of its float64 value:
    absolute error <= 2 * 2^-25 + 2^-25 (the product's rounding) < 4 * 2^-24 (generously), on every live corner: 4 * 2^-24 on
    SG = sum_o sum_c sum_i |g_c| |V_c(i)| |o~_j|;
  * per channel n <= 8 fused products are added in float32, each step rounding the running sum (<= 2^-24 sum_i |w_i| |V_c(i)|),
    and q_a is a product and a fused product of the two channels with g (two more roundings, "+ 4" generously):
    (n + 4) * 2^-24 on SWG = sum_o sum_c sum_i |w_i| |g_c| |V_c(i)| |o~_j|;
  * q_a o~_j and the sums over voxels are float64: 2^-53 per step against 2^-24, negligible (and covered by the generosity above).
Hence |device - reference| <= 2^-24 (4 SG + (n + 4)-weighted SWG) per entry.  Nothing a device returned enters."""
import functools

import numpy as np

import rigid_reference as rr

f32, f64 = np.float32, np.float64


def cell(prm, dims):
    """(i0, fr): per axis the lower corner [NX][NZ][NY] of every output voxel's cell and the fraction in it, as rigid_reference.taps"""
    m = np.asarray(prm, dtype=f64).reshape(3, 4)
    NX, NZ, NY = dims
    x, z, y = np.meshgrid(np.arange(NX, dtype=f64), np.arange(NZ, dtype=f64), np.arange(NY, dtype=f64), indexing='ij')
    i0, fr = [], []
    for a in range(3):
        p = ((m[a, 0] * x + m[a, 3]) + m[a, 1] * z) + m[a, 2] * y
        fl = np.floor(p)
        i0.append(fl.astype(np.int64))
        fr.append(p - fl)
    return i0, fr, (x, z, y, np.ones_like(x))


def param_terms(vol, g, prm, weights='f64'):
    """vol [NX][NZ][NY][C], g [NZ][NX][NY][C] -> (d, SG, SWG, T), each (3, 4): the entries dL/d prm[a][j], and per entry
    SG = sum |g| |V| |o~_j| over live corners, SWG = sum (n + 4) |w| |g| |V| |o~_j| and T = sum |w| |g| |V| |o~_j| (the sum of the
    absolute values of the entry's terms).  weights='f32': factors, two-factor weights, tap sums and q_a in float32 as the
    kernel forms them (the sums over voxels stay float64)."""
    NX, NZ, NY, C = vol.shape
    i0, fr, ot = cell(prm, (NX, NZ, NY))
    wt = f32 if weights == 'f32' else f64
    fac = [((1.0 - f).astype(wt), f.astype(wt)) for f in fr]
    flat = np.asarray(vol, dtype=wt).reshape(-1, C)
    gg = np.asarray(g, dtype=wt).transpose(1, 0, 2, 3)
    n = (NX, NZ, NY)
    d, SG, SWG, T = np.zeros((4, 3, 4))
    for a in range(3):
        o1, o2 = [k for k in range(3) if k != a]
        dv = np.zeros((NX, NZ, NY, C), dtype=wt)
        sabs, wabs = np.zeros((2, NX, NZ, NY, C))
        cnt = np.zeros((NX, NZ, NY))
        for i in range(8):
            bit = (i >> 2, (i >> 1) & 1, i & 1)
            pos = [i0[k] + bit[k] for k in range(3)]
            inside = np.ones((NX, NZ, NY), dtype=bool)
            for k in range(3):
                inside &= (pos[k] >= 0) & (pos[k] < n[k])
            idx = np.where(inside, (pos[0] * NZ + pos[1]) * NY + pos[2], 0)
            w = np.where(inside, fac[o1][bit[o1]] * fac[o2][bit[o2]], 0).astype(wt)
            v = flat[idx]
            dv = dv + ((w if bit[a] else -w)[..., None] * v).astype(wt)
            live = inside & (w != 0)
            sabs += live[..., None] * np.abs(v).astype(f64)
            wabs += w.astype(f64)[..., None] * np.abs(v).astype(f64)
            cnt += live
        q = (gg[..., 0] * dv[..., 0]).astype(wt)
        for c in range(1, C):
            q = (q + gg[..., c] * dv[..., c]).astype(wt)
        ag = np.abs(gg).astype(f64)
        for j in range(4):
            d[a, j] = np.sum(q.astype(f64) * ot[j])
            SG[a, j] = np.sum((ag * sabs).sum(axis=-1) * np.abs(ot[j]))
            SWG[a, j] = np.sum((cnt + 4) * (ag * wabs).sum(axis=-1) * np.abs(ot[j]))
            T[a, j] = np.sum((ag * wabs).sum(axis=-1) * np.abs(ot[j]))
    return d, SG, SWG, T


def entry_bound(SG, SWG):
    return 2.0 ** -24 * (4 * SG + SWG)


def pairing(vol, g, prm):
    """L(prm) = sum rotate_rigid(V, prm) g in float64: what param_terms differentiates"""
    return float(np.sum(rr.rotate_rigid(np.asarray(vol, dtype=f64), prm) * np.asarray(g, dtype=f64)))


def to_rows(a):
    """(Y, X, Z) pairs of arrays -> [NX][NZ][NY][C] of the volume"""
    return np.stack(a, axis=3).transpose(1, 2, 0, 3)


def to_rotated(a):
    """(Y, X, Z) pairs of rotated-frame arrays -> [NZ][NX][NY][C]"""
    return np.stack(a, axis=3).transpose(2, 1, 0, 3)


# ---- the solver-level cases --------------------------------------------------------------------------------------------------------------
# |device - float64| per entry of dL/d(M | t), relative to the entry's sum of |terms| T (the entries cancel to about 1 % of T, so a
# bound relative to the entry itself would say nothing about the arithmetic).  By gradient_cases.bound_rule on the float32 /
# complex64 restatement (geometry_composed_figure, ptycho_geometry_composed_figure): tests/test_geometry_reference.py recomputes
# the figures on the CPU and holds these constants to the rule.  No device figure enters.
GEOMETRY_GRADIENT_BOUND = 2e-5
PTYCHO_GEOMETRY_GRADIENT_BOUND = 2e-5
FP = 1e-4                         # the full-field case's free_prop_cm


def _rotated_gradients(p, fp):
    from oracle import bdof_oracle as orc
    one, zero = np.ones((rr.N, rr.N)), np.zeros((rr.N, rr.N))
    rot = p['rot']
    _, gd, gb = orc.multislice_loss_and_grad(rot[..., 0], rot[..., 1], one, zero, rr.E_EV, rr.PSIZE_CM, p['meas'], fp)
    return gd, gb


def chain(prm_terms, index, theta, shape, tilt, roll, center):
    """(d, T) stacks (B, 3, 4) -> the geometry gradient and, by the same linear map applied to T through absolute values, the
    term sum every geometry entry is held against"""
    from beyond_dof_amd import util
    d = np.stack([t[0] for t in prm_terms])
    return util.rigid_geometry_gradient(theta, shape, tilt, roll, center, None, d.reshape(len(index), 12), index)


@functools.lru_cache(maxsize=None)
def solver_geometry_problem(fp=FP):
    """rigid_reference.solver_problem's three angles: float64 dL/d(M | t) (3, 3, 4) with its term sums from the model's rotated-frame
    gradient, and the geometry gradient the chain rule makes of it"""
    p = rr.solver_problem(fp)
    gd, gb = _rotated_gradients(p, fp)
    vol = to_rows([p['od'], p['ob']])
    terms = [param_terms(vol, to_rotated([gd[b], gb[b]]), q) for b, q in enumerate(p['prm'])]
    out = dict(d=np.stack([t[0] for t in terms]), T=np.stack([t[3] for t in terms]),
               geometry=chain(terms, np.array(rr.IDX), rr.solver_theta(), (rr.N, rr.N, rr.N), rr.TILT, rr.ROLL, rr.CENTER))
    for v in (out['d'], out['T']):
        v.setflags(write=False)
    return out


def geometry_composed_figure(fp=FP):
    """The worst error of dL/d(M | t) in float32 / complex64 — rotation with float32 weights, modulation_reference.c64_loss_and_grad,
    the restatement with 'f32' weights — against solver_geometry_problem's, relative to the entry's sum of |terms|"""
    import modulation_reference as mref
    p, ref = rr.solver_problem(fp), solver_geometry_problem(fp)
    obj = np.stack([p['od'], p['ob']], axis=3).astype(f32)
    rot = np.stack([rr.rotate_volume(obj, q, 'f32') for q in p['prm']])
    one, zero = np.ones((rr.N, rr.N)), np.zeros((rr.N, rr.N))
    _, loss, gd, gb = mref.c64_loss_and_grad(rot[..., 0], rot[..., 1], one, zero, p['meas'], fp)
    vol = to_rows([p['od'], p['ob']]).astype(f32)
    d = np.stack([param_terms(vol, to_rotated([gd[b], gb[b]]).astype(f32), q, 'f32')[0] for b, q in enumerate(p['prm'])])
    return float(np.max(np.abs(d - ref['d']) / ref['T']))


@functools.lru_cache(maxsize=None)
def ptycho_geometry_problem(psz=32):
    """rigid_reference.ptycho_problem's one angle: the same from the windows' gradient, overlap-added into the rotated frame"""
    import reference_model as ref_model
    p = rr.ptycho_problem(psz)
    vol = to_rows([p['od'], p['ob']])
    subs = rr.ptycho_windows(rr.rotate_volume(np.stack([p['od'], p['ob']], axis=3), p['prm']), psz)
    _, gd, gb, _, _ = ref_model.loss_and_grad(subs[..., 0], subs[..., 1], p['pr'], p['pi'], rr.E_EV, rr.PSIZE_CM, p['meas'], 'inf')
    g_rot = rr.ptycho_windows_adjoint(np.stack([gd, gb], axis=-1), psz)                  # (Y, X, Z, C)
    t = param_terms(vol, g_rot.transpose(2, 1, 0, 3), p['prm'])
    return dict(d=t[0][None], T=t[3][None],
                geometry=chain([t], np.array([rr.PTY_THETA]), rr.ptycho_theta(), rr.PTY_SHAPE, rr.PTY_TILT, 0., None))


def ptycho_geometry_composed_figure(psz=32):
    import modulation_reference as mref
    p, ref = rr.ptycho_problem(psz), ptycho_geometry_problem(psz)
    rot = rr.rotate_volume(np.stack([p['od'], p['ob']], axis=3).astype(f32), p['prm'], 'f32')
    subs = rr.ptycho_windows(rot, psz)
    _, loss, gd, gb = mref.c64_loss_and_grad(subs[..., 0], subs[..., 1], p['pr'], p['pi'], p['meas'], 'inf')
    g_rot = rr.ptycho_windows_adjoint(np.stack([gd, gb], axis=-1), psz, f32)
    vol = to_rows([p['od'], p['ob']]).astype(f32)
    d = param_terms(vol, g_rot.transpose(2, 1, 0, 3), p['prm'], 'f32')[0]
    return float(np.max(np.abs(d - ref['d'][0]) / ref['T'][0]))


def geometry_term_sums(T, index, theta, shape, tilt, roll, center):
    """What a geometry entry is held against: the chain rule's linear map with every coefficient and every term sum taken in
    absolute value — |d geometry| <= sum |coefficient| * bound * T.  Computed by differentiating with unit rows."""
    from beyond_dof_amd import util
    T = np.asarray(T).reshape(len(index), 12)
    out = None
    for k in range(len(index)):
        for e in range(12):
            unit = np.zeros((len(index), 12))
            unit[k, e] = 1.0
            g = util.rigid_geometry_gradient(theta, shape, tilt, roll, center, None, unit, index)
            if out is None:
                out = {name: np.zeros_like(np.asarray(v, dtype=f64)) for name, v in g.items()}
            for name, v in g.items():
                out[name] = out[name] + np.abs(v) * T[k, e]
    return out
