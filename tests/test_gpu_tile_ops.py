"""The four tile operators of the tiled propagator — cut, cut^H, put, put^H (csrc/bdof_field.h) — through each of the ten
bdof_tiles_* entry points, against a float64 numpy restatement written here: periodic window, raised-cosine taper, cores, and the
drop of core pixels beyond the field's edge.  Geometries (non-square, so an x / y swap shows):
  A  field 24 x 20, tiles 16 x 12, halo (4, 2), taper 2: negative origins, windows that wrap past the high edge, last y-cores that
     overhang the field by 4 pixels;
  B  field 12 x 20, tiles 16 x 12, halo (5, 2), taper 3: tiles wider than the field — a tile row maps onto a field row twice;
both also with taper 0.  In both every field pixel has exactly one core writer."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GEOMETRIES = {'A': dict(FX=24, FY=20, TX=16, TY=12, hx=4, hy=2, taper=2), 'B': dict(FX=12, FY=20, TX=16, TY=12, hx=5, hy=2, taper=3)}
CASES = [(g, t) for g in 'AB' for t in ('taper', 'taper0')]
# float arithmetic (__cosf taper, float products and sums): the parent commit's build measured 8.33e-08 (largest component error
# relative to max |reference| over A and B, bdof_tiles_gather and bdof_tiles_gather_adjoint); 4 x that, one significant digit up
FLOAT_BOUND = 4e-7


class Geometry(object):
    def __init__(self, FX, FY, TX, TY, hx, hy, taper):
        self.FX, self.FY, self.TX, self.TY, self.hx, self.hy, self.taper = FX, FY, TX, TY, hx, hy, taper
        cx, cy = TX - 2 * hx, TY - 2 * hy
        ox = [i * cx - hx for i in range(-(-FX // cx))]
        oy = [i * cy - hy for i in range(-(-FY // cy))]
        self.x0 = np.repeat(np.array(ox, dtype=np.int32), len(oy))
        self.y0 = np.tile(np.array(oy, dtype=np.int32), len(ox))
        self.B = len(self.x0)

    def weights(self):
        def w(n):
            e = np.minimum(np.arange(n), n - 1 - np.arange(n))
            return np.where(e < self.taper, 0.5 - 0.5 * np.cos(np.pi * (e + 0.5) / max(self.taper, 1)), 1.0)
        return w(self.TX)[:, None] * w(self.TY)[None, :]

    def window(self, b):
        """field indices (periodic) of tile b's pixels"""
        return np.mod(self.x0[b] + np.arange(self.TX), self.FX)[:, None], np.mod(self.y0[b] + np.arange(self.TY), self.FY)[None, :]

    def core(self, b):
        """mask [TX][TY] of tile b's core pixels that lie in the field, and their (unwrapped) field indices"""
        x, y = np.arange(self.TX), np.arange(self.TY)
        xg, yg = self.x0[b] + x, self.y0[b] + y
        mx = (x >= self.hx) & (x < self.TX - self.hx) & (xg >= 0) & (xg < self.FX)
        my = (y >= self.hy) & (y < self.TY - self.hy) & (yg >= 0) & (yg < self.FY)
        return mx[:, None] & my[None, :], np.clip(xg, 0, self.FX - 1)[:, None], np.clip(yg, 0, self.FY - 1)[None, :]

    # ---- the four operators, float64 ----
    def cut(self, f):
        return np.stack([f[self.window(b)] for b in range(self.B)]) * self.weights()

    def cut_adjoint(self, t):
        out = np.zeros((self.FX, self.FY), dtype=np.complex128)
        for b in range(self.B):
            np.add.at(out, self.window(b), t[b] * self.weights())
        return out

    def put(self, t, field):
        out = field.copy()
        for b in range(self.B):
            m, xg, yg = self.core(b)
            out[np.broadcast_to(xg, m.shape)[m], np.broadcast_to(yg, m.shape)[m]] = t[b][m]
        return out

    def put_adjoint(self, f):
        out = np.zeros((self.B, self.TX, self.TY), dtype=f.dtype)
        for b in range(self.B):
            m, xg, yg = self.core(b)
            out[b][m] = f[np.broadcast_to(xg, m.shape)[m], np.broadcast_to(yg, m.shape)[m]]
        return out


def _geometry(name, taper):
    kw = dict(GEOMETRIES[name])
    if taper == 'taper0':
        kw['taper'] = 0
    return Geometry(**kw)


def test_the_restatement_itself():
    """No device: one core writer per field pixel, and the two adjoint pairs of the numpy restatement."""
    for name, t in CASES:
        g = _geometry(name, t)
        rng = np.random.default_rng(1)
        writers = np.zeros((g.FX, g.FY), dtype=np.int64)
        for b in range(g.B):
            m, xg, yg = g.core(b)
            np.add.at(writers, (np.broadcast_to(xg, m.shape)[m], np.broadcast_to(yg, m.shape)[m]), 1)
        assert np.all(writers == 1)
        f = rng.normal(size=(g.FX, g.FY)) + 1j * rng.normal(size=(g.FX, g.FY))
        u = rng.normal(size=(g.B, g.TX, g.TY)) + 1j * rng.normal(size=(g.B, g.TX, g.TY))
        assert abs(np.vdot(u, g.cut(f)) - np.vdot(g.cut_adjoint(u), f)) <= 1e-15 * abs(np.vdot(u, g.cut(f))) + 1e-13
        zero = np.zeros_like(f)
        assert abs(np.vdot(f, g.put(u, zero)) - np.vdot(g.put_adjoint(f), u)) <= 1e-13


class Device(object):
    """One context and the buffers of one geometry; the ten entry points with the geometry's argument tail filled in."""

    def __init__(self, g):
        from beyond_dof_amd import _lib
        self.g, self._lib = g, _lib
        self.ctx = _lib.Context(0)
        self.lib, self.h = self.ctx.lib, self.ctx.handle
        self.bufs = []
        self.x0, self.y0 = self.up(g.x0), self.up(g.y0)

    def up(self, arr):
        self.bufs.append(self._lib.DeviceBuffer.from_host(self.ctx, np.ascontiguousarray(arr)))
        return self.bufs[-1]

    def close(self):
        self.ctx.sync()
        for b in self.bufs:
            b.free()
        self.ctx.close()

    def from_field(self, name, field, tile_dtype, fill=None):
        """cut / put^H entry point `name`: field (host) -> tiles (host)"""
        g = self.g
        f = self.up(field)
        t = self.up(np.full((g.B, g.TX, g.TY), np.nan if fill is None else fill, dtype=tile_dtype))
        edge = (g.hx, g.hy) if 'scatter' in name else (g.taper,)
        self.ctx.check(getattr(self.lib, name)(self.h, f.ptr, g.FX, g.FY, t.ptr, g.B, g.TX, g.TY, self.x0.ptr, self.y0.ptr, *edge))
        self.ctx.sync()
        return t.download()

    def into_field(self, name, tiles, field, minus=None, accumulate=None):
        """cut^H / put entry point `name`: tiles (host) -> the field (host; `field`: its content before the call)"""
        g = self.g
        t, f = self.up(tiles), self.up(field)
        edge = (g.hx, g.hy) if 'scatter' in name else (g.taper,)
        src = (t.ptr,) if accumulate is None else (t.ptr, None if minus is None else self.up(minus).ptr)
        tail = () if accumulate is None else (int(accumulate),)
        self.ctx.check(getattr(self.lib, name)(self.h, *src, f.ptr, g.FX, g.FY, g.B, g.TX, g.TY, self.x0.ptr, self.y0.ptr, *edge, *tail))
        self.ctx.sync()
        return f.download()


@pytest.fixture(scope='module')
def built():
    import __graft_entry__ as entry
    entry.build()


@pytest.fixture(scope='module', params=CASES, ids=['-'.join(c) for c in CASES])
def case(request, built):
    g = _geometry(*request.param)
    rng = np.random.default_rng(7)
    cn = lambda shape: rng.normal(size=shape) + 1j * rng.normal(size=shape)
    data = dict(f64=cn((g.FX, g.FY)), t64=cn((g.B, g.TX, g.TY)), b64=cn((g.B, g.TX, g.TY)), g64=cn((g.FX, g.FY)))
    data.update({k.replace('64', '32'): v.astype(np.complex64) for k, v in list(data.items())})
    dev = Device(g)
    yield g, dev, data
    dev.close()


def comp_err(a, b):
    """largest difference per real component"""
    d = np.asarray(a, dtype=np.complex128) - np.asarray(b, dtype=np.complex128)
    return float(max(np.abs(d.real).max(), np.abs(d.imag).max()))


def comp_max(a):
    return float(max(np.abs(a.real).max(), np.abs(a.imag).max()))


SENTINEL = -777.25 + 333.5j


def test_put_is_exact(case):
    """put in all three pairings, with tiles_b and accumulate; a sentinel-filled field is overwritten everywhere."""
    g, dev, d = case
    sent32, sent64 = np.full((g.FX, g.FY), SENTINEL, np.complex64), np.full((g.FX, g.FY), SENTINEL, np.complex128)
    out = dev.into_field('bdof_tiles_scatter', d['t32'], sent32)
    assert np.array_equal(out, g.put(d['t32'], sent32)) and not np.any(out == SENTINEL)
    out = dev.into_field('bdof_tiles_scatter_f64', d['t64'], sent64)
    assert np.array_equal(out, g.put(d['t64'], sent64)) and not np.any(out == SENTINEL)
    ta, tb = d['t32'].astype(np.complex128), d['b32'].astype(np.complex128)
    out = dev.into_field('bdof_tiles_scatter_diff64', d['t32'], sent64, None, 0)
    assert np.array_equal(out, g.put(ta, sent64)) and not np.any(out == SENTINEL)
    out = dev.into_field('bdof_tiles_scatter_diff64', d['t32'], sent64, d['b32'], 0)
    assert np.array_equal(out, g.put(ta - tb, sent64)) and not np.any(out == SENTINEL)
    start = d['g64']                                                    # accumulate: from a non-zero field
    for minus, diff in ((None, ta), (d['b32'], ta - tb)):
        out = dev.into_field('bdof_tiles_scatter_diff64', d['t32'], start, minus, 1)
        assert np.array_equal(out, g.put(diff + g.put_adjoint(start), start))


def test_put_adjoint_is_exact(case):
    """put^H in both pairings, zeros on halos and overhang included (the tiles start as NaN)."""
    g, dev, d = case
    assert np.array_equal(dev.from_field('bdof_tiles_scatter_adjoint', d['f32'], np.complex64), g.put_adjoint(d['f32']))
    assert np.array_equal(dev.from_field('bdof_tiles_scatter_adjoint_mixed', d['f64'], np.complex64), g.put_adjoint(d['f64']).astype(np.complex64))


def test_cut(case):
    """cut in all three pairings: exact with taper 0; double arithmetic to a few ulps of the weight product, float arithmetic to
    FLOAT_BOUND with a taper."""
    g, dev, d = case
    got32 = dev.from_field('bdof_tiles_gather', d['f32'], np.complex64)
    got64 = dev.from_field('bdof_tiles_gather_f64', d['f64'], np.complex128)
    gotmx = dev.from_field('bdof_tiles_gather_mixed', d['f64'], np.complex64)
    ref32, ref64 = g.cut(d['f32'].astype(np.complex128)), g.cut(d['f64'])
    if g.taper == 0:
        assert np.array_equal(got32, ref32.astype(np.complex64)) and np.array_equal(got64, ref64)
        assert np.array_equal(gotmx, ref64.astype(np.complex64))
        return
    refmx = ref64.astype(np.complex64)
    dm = gotmx - refmx
    ulps = max(np.max(np.abs(dm.real) / np.spacing(np.abs(refmx.real))), np.max(np.abs(dm.imag) / np.spacing(np.abs(refmx.imag))))
    e = (comp_err(got32, ref32) / comp_max(ref32), comp_err(got64, ref64) / comp_max(d['f64']), float(ulps))
    print('cut: float', e[0], 'double', e[1], 'mixed, in float32 ulps', e[2])
    assert e[0] <= FLOAT_BOUND
    assert e[1] <= 1e-14
    assert e[2] <= 1.0


def test_cut_adjoint(case):
    """cut^H: float sums to FLOAT_BOUND, double sums (with and without tiles_b, with and without accumulate) to 1e-13."""
    g, dev, d = case
    junk32, junk64 = np.full((g.FX, g.FY), SENTINEL, np.complex64), np.full((g.FX, g.FY), SENTINEL, np.complex128)
    ref = g.cut_adjoint(d['t32'].astype(np.complex128))
    e = comp_err(dev.into_field('bdof_tiles_gather_adjoint', d['t32'], junk32), ref) / comp_max(ref)
    print('cut^H: float', e)
    assert e <= FLOAT_BOUND
    ta, tb = d['t32'].astype(np.complex128), d['b32'].astype(np.complex128)
    for minus, diff in ((None, ta), (d['b32'], ta - tb)):
        for acc, start in ((0, junk64), (1, d['g64'])):
            ref = g.cut_adjoint(diff) + (start if acc else 0)
            e = comp_err(dev.into_field('bdof_tiles_gather_adjoint_diff64', d['t32'], start, minus, acc), ref) / comp_max(ref)
            print('cut^H: double, tiles_b', minus is not None, 'accumulate', acc, e)
            assert e <= 1e-13


def test_adjoint_pairs(case):
    """<Op u, v> = <u, Op^H v> on the device outputs, complex64 and mixed pairs.  Each side's inner product inherits its operator's
    bound: a component error of at most eps * max |reference| in each of n complex values moves <w, .> by at most
    eps * max |reference| * sqrt(2 n) * |w|; the two sides' allowances add (plus 1e-14 |u| |v| for the host's own sums)."""
    g, dev, d = case
    dot = lambda a, b: np.vdot(np.asarray(a, np.complex128), np.asarray(b, np.complex128))
    norm = lambda a: float(np.linalg.norm(np.asarray(a, np.complex128)))
    zero32, zero64 = np.zeros((g.FX, g.FY), np.complex64), np.zeros((g.FX, g.FY), np.complex128)
    t32 = d['t32']
    ulp32 = 2.0 ** -23                        # one float32 ulp of a value, relative to it (<= relative to the largest)
    exact_cut = g.taper == 0
    pairs = {   # name: (Op u on the device, v, bound of Op, Op^H v on the device, u, bound of Op^H)
        'cut c64': (dev.from_field('bdof_tiles_gather', d['f32'], np.complex64), t32, 0. if exact_cut else FLOAT_BOUND,
                    dev.into_field('bdof_tiles_gather_adjoint', t32, zero32), d['f32'], FLOAT_BOUND),
        'cut mixed': (dev.from_field('bdof_tiles_gather_mixed', d['f64'], np.complex64), t32, ulp32,
                      dev.into_field('bdof_tiles_gather_adjoint_diff64', t32, zero64, None, 0), d['f64'], 1e-13),
        'put c64': (dev.into_field('bdof_tiles_scatter', t32, zero32), d['g32'], 0.,
                    dev.from_field('bdof_tiles_scatter_adjoint', d['g32'], np.complex64), t32, 0.),
        'put mixed': (dev.into_field('bdof_tiles_scatter_diff64', t32, zero64, None, 0), d['g64'], 0.,
                      dev.from_field('bdof_tiles_scatter_adjoint_mixed', d['g64'], np.complex64), t32, ulp32),
    }
    for name, (op_u, v, e_op, adj_v, u, e_adj) in pairs.items():
        lhs, rhs = dot(v, op_u), dot(adj_v, u)
        bound = e_op * comp_max(op_u) * np.sqrt(2 * op_u.size) * norm(v) + e_adj * comp_max(adj_v) * np.sqrt(2 * adj_v.size) * norm(u) + \
            1e-14 * norm(u) * norm(v)
        print('adjoint pair', name, abs(lhs - rhs), 'bound', bound)
        assert abs(lhs - rhs) <= bound, name
