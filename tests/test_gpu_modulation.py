"""The table of modulation factors c - 1 = exp(i k delta) exp(-k beta) - 1 on the device, entry by entry, and every engine that
reads it at strong phase.

Part 1 — the table itself (bdof_modulation_table, MultisliceEngine.modulation_table): both producers (k_modulation_table,
k_rot_bilinear<MOD>) against tests/modulation_reference.py: |device - reference| <= bound for every entry of every case
(all four quadrants of the reduction for both signs of n, both expm1 branches, both sides of each switch, |x| up to 1e5,
y from -100 to 10), exact zeros for vacuum, bit-identical rebuilds, and the mean the host forms the carrier scalars from.

Part 2 — the consumers: objects with phases of +-pi per voxel, phases wrapped 8 turns and k beta up to 0.6 through the
streaming, resident and generic engines, the float64 adjoint sweep, the float64 twin, the tape-free adjoint, slice binning, the
real-space propagator and the two solvers, against the float64 oracle at the effective values k delta_eff = x32,
-k beta_eff = y32 (modulation_reference.oracle_inputs), at the bounds of the weak-phase tests of each path.  Every test prints
what it measured before it asserts (MEASUREMENTS.md)."""
import ctypes
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import bdof_oracle as orc

import reference_model as ref_model
import modulation_reference as mref

E, PS = mref.E_EV, mref.PSIZE_CM
B, S = mref.B, mref.S
rel = mref.rel
BDOF_ERR_STATE = -2


@pytest.fixture(scope='module')
def engine_mod():
    import __graft_entry__ as entry
    entry.build()
    from beyond_dof_amd import engine
    return engine


# =====================================================================================================================================
# Part 1: the table
# =====================================================================================================================================
def _table_engine(engine_mod, n_slice=1, **kw):
    """64 x 64 wavefields; a probe with a plane-wave part, so that the mean of the table is formed (want_cbar)."""
    eng = engine_mod.MultisliceEngine(64, 64, n_slice, 1, with_grad=False, **kw)
    eng.set_physics(E, PS, None)
    eng.set_probe(*mref.probe('structured', 64, 64))
    assert eng.k == mref.K64
    return eng


def _bind(eng, delta32, beta32):
    """n (delta, beta) pairs as one raw row of n entries (bdof_set_object with a rotation table, which the table pass never reads)."""
    from beyond_dof_amd._lib import DeviceBuffer
    rows = np.ascontiguousarray(np.stack([delta32, beta32], axis=-1).astype(np.float32))
    eng.set_volume(DeviceBuffer.from_host(eng.ctx, rows), 1, len(delta32), DeviceBuffer.zeros(eng.ctx, (1,), np.int32), 1, 1)


def _check_mean(tag, table, mean, D):
    """mean == fsum(entries) / n within (D + 2) 2^-53 mean|entry|: D roundings of additions on the longest chain from an entry to
    the sum, one of 1 / n and one of the product with it."""
    n = table.size
    ref = complex(math.fsum(table.real.astype(np.float64)), math.fsum(table.imag.astype(np.float64))) / n
    tol = (D + 2) * 2. ** -53 * float(np.abs(table.astype(np.complex128)).mean())
    print('mean of the table', tag, 'n', n, ': |device - fsum / n|', abs(mean - ref), 'bound', tol, 'mean', mean)
    assert abs(mean - ref) <= tol, (tag, mean, ref, tol)


# D, the longest chain of float64 additions from a table entry to the sum, counted in the kernels (csrc/bdof_kernels.h) for the
# launch the host makes (ensure_modulation / bdof_set_object_bilinear, csrc/bdof_capi.hip; ncu compute units).
# k_modulation_table, grid = min(ceil(n / 256), 16 ncu) workgroups of 256: T = ceil(n / (256 grid)) additions in a thread's
# grid-stride loop, 6 in the wave's shuffle tree, 3 over the four waves.  k_sum_mean: ceil(grid / 256) per thread, 8 in the tree over
# its 256 threads.  On the MI355X's 256 CUs: n <= 65536: D = 1 + 6 + 3 + 1 + 8 = 19; n = 65537: 257 partial sums, thread 0 of k_sum_mean
# adds two, D = 20; the 2^21 + 77 sweep: T = 3, grid = 4096, D = 3 + 9 + 16 + 8 = 36.
# k_rot_bilinear<MOD>, grid = min(ceil(rows / 4), 16 ncu), one wave per row, a lane's float4 holds two entries: 2 additions per row
# and per 64 float4 columns of it, then the same 6 + 3 and k_sum_mean.  6 x 5 x 64, B = 1 or 2: one row per wave, one float4 per
# lane: D = 2 + 6 + 3 + 1 + 8 = 20.
NCU = 256           # MI355X, which the gpu mark asks for; with fewer CUs T (and D) can only grow where ceil(n / 256) > 16 ncu


def _D(n, ncu=NCU):
    need = -(-n // 256)
    grid = min(need, 16 * ncu)
    return -(-need // grid) + 6 + 3 + -(-grid // 256) + 8


def _D_bilinear(rows, NYv, ncu=NCU):
    grid = min(-(-rows // 4), 16 * ncu)
    return 2 * -(-rows // (4 * grid)) * -(-(NYv // 2) // 64) + 6 + 3 + -(-grid // 256) + 8


@pytest.mark.parametrize('name', ['sweep', 'switches', 'special'])
def test_table_entry_by_entry(engine_mod, name):
    eng = _table_engine(engine_mod)
    k32 = np.float32(eng.k)
    d, b = {'sweep': mref.sweep, 'switches': lambda k: mref.switches(k)[:2], 'special': mref.special}[name](k32)
    _bind(eng, d, b)
    table, mean = eng.modulation_table()
    assert table.shape == d.shape and table.dtype == np.complex64
    ratio, where = mref.worst(table, d, b, k32)
    print('modulation table,', name, ', n =', d.size, ': worst |device - reference| / bound', ratio, 'at', where)
    assert ratio <= 1.0, (ratio, where)
    _check_mean('k_modulation_table, ' + name, table, mean, _D(d.size))
    if name == 'special':
        assert np.all(table[mref.SPECIAL_ZERO] == 0), table[mref.SPECIAL_ZERO]         # vacuum: a factor of exactly 1
        x, y = mref.arguments(d, b, k32)
        assert np.all(np.abs(table[mref.SPECIAL_OPAQUE] + 1) <= mref.bound(x, y)[mref.SPECIAL_OPAQUE])
    # a second build gives the same bits: another object in between forces it
    _bind(eng, np.zeros(300, np.float32), np.zeros(300, np.float32))
    other, m0 = eng.modulation_table()
    assert other.size == 300 and np.all(other == 0) and m0 == 0
    _bind(eng, d, b)
    again, mean2 = eng.modulation_table()
    assert np.array_equal(again.view(np.uint32), table.view(np.uint32))
    assert (mean.real, mean.imag) == (mean2.real, mean2.imag)


@pytest.mark.parametrize('n', [1, 255, 256, 257, 65536 + 1])
def test_table_mean(engine_mod, n):
    """65536 + 1 entries make 257 partial sums: k_sum_mean strides."""
    eng = _table_engine(engine_mod)
    k32 = np.float32(eng.k)
    d, b = mref.sweep(k32, n=n, seed=n)
    _bind(eng, d, b)
    table, mean = eng.modulation_table()
    assert mref.worst(table, d, b, k32)[0] <= 1.0
    _check_mean('k_modulation_table', table, mean, _D(n))
    _bind(eng, d[::-1].copy(), b[::-1].copy())
    eng.modulation_table()
    _bind(eng, d, b)
    table2, mean2 = eng.modulation_table()
    assert np.array_equal(table2.view(np.uint32), table.view(np.uint32)) and (mean.real, mean.imag) == (mean2.real, mean2.imag)


def test_table_mean_of_a_bin(engine_mod):
    """slice_binning = 2: the carrier of a step picks up the mean factor of its bin, (1 + m)^2 - 1 of the unbinned mean m."""
    k32 = np.float32(mref.K64)
    d, b = mref.regime('absorbing', (2 * 64 * 64,))
    means = []
    for bin_ in (1, 2):
        eng = _table_engine(engine_mod, n_slice=2, slice_binning=bin_)
        eng.set_object_batch(d.reshape(1, 64, 64, 2), b.reshape(1, 64, 64, 2))
        table, mean = eng.modulation_table()
        assert table.size == d.size and mref.worst(table, *[v.reshape(1, 64, 64, 2).transpose(0, 3, 2, 1).ravel() for v in (d, b)], k32)[0] <= 1.0
        means.append(mean)
    print('mean of a bin of 2:', means[1], 'unbinned', means[0], 'difference from (1 + m)^2 - 1:', abs(means[1] - ((1 + means[0]) ** 2 - 1)))
    assert abs(means[0]) > 0.1 and abs(means[1] - ((1 + means[0]) ** 2 - 1)) <= 1e-15


def test_table_mean_is_zero_without_a_plane_wave_part(engine_mod):
    eng = _table_engine(engine_mod)
    eng.set_probe(*mref.probe('gaussian', 64, 64))                                     # a carrier field: no mean rides on it
    d, b = mref.regime('absorbing', (1000,))
    _bind(eng, d, b)
    table, mean = eng.modulation_table()
    assert mean == 0 and mref.worst(table, d, b, np.float32(eng.k))[0] <= 1.0


def _bilinear_engine(engine_mod, NXv, NZv, NYv, Bmax):
    eng = engine_mod.MultisliceEngine(NYv, NXv, NZv, Bmax, with_grad=False, engine='generic')
    eng.set_physics(E, PS, None)
    eng.set_probe(*mref.probe('structured', NYv, NXv))
    return eng


def test_second_producer_bilinear_rotation(engine_mod):
    """bdof_set_object_bilinear (k_rot_bilinear<MOD>) writes the same table: bit for bit k_modulation_table's under the identity
    rotation, and within the bound of the reference at the rows bdof_rotate_bilinear (the MOD = false instance of the same
    interpolation) returns at two real angles."""
    from beyond_dof_amd._lib import DeviceBuffer
    NXv, NZv, NYv = 6, 5, 64
    eng = _bilinear_engine(engine_mod, NXv, NZv, NYv, 2)
    lib, h, k32 = eng.lib, eng.h, np.float32(eng.k)
    d, b = mref.regime('pi', (NXv, NZv, NYv), seed=5)
    vol = DeviceBuffer.from_host(eng.ctx, np.ascontiguousarray(np.stack([d, b], axis=-1)))            # [x][z][y] pairs
    # identity: output rows [z][x] are volume rows [x][z]
    prm = DeviceBuffer.from_host(eng.ctx, np.array([[1., 0., 0., 0.]]))
    eng.ctx.check(lib.bdof_set_object_bilinear(h, vol.ptr, NXv, NZv, NYv, prm.ptr, 1, 0))
    t_bil, m_bil = eng.modulation_table()
    eng.set_volume(vol, NXv * NZv, NYv, None, 0, 0)
    t_tab, m_tab = eng.modulation_table()
    assert t_bil.size == t_tab.size == d.size
    assert np.array_equal(t_bil.reshape(NZv, NXv, NYv).transpose(1, 0, 2).view(np.uint32), t_tab.reshape(NXv, NZv, NYv).view(np.uint32))
    assert mref.worst(t_tab, d.ravel(), b.ravel(), k32)[0] <= 1.0
    _check_mean('k_rot_bilinear<MOD>, identity', t_bil, m_bil, _D_bilinear(NZv * NXv, NYv))
    _check_mean('k_modulation_table, same volume', t_tab, m_tab, _D(d.size))
    # two real angles
    H, W = NXv, NZv
    prm_h = np.array([orc.rotate_bilinear_params(th, H, W) for th in (0.3, -2.0)], dtype=np.float64)
    prm = DeviceBuffer.from_host(eng.ctx, np.ascontiguousarray(prm_h))
    rows = DeviceBuffer(eng.ctx, 2 * d.size * 8, np.float32, (2, NZv, NXv, NYv, 2))
    eng.ctx.check(lib.bdof_rotate_bilinear(h, vol.ptr, NXv, NZv, NYv, prm.ptr, 2, rows.ptr))
    eng.ctx.sync()
    r = rows.download()
    assert np.any(r[0] != 0) and not np.array_equal(r[0], r[1])
    eng.ctx.check(lib.bdof_set_object_bilinear(h, vol.ptr, NXv, NZv, NYv, prm.ptr, 2, 0))
    table, mean = eng.modulation_table()
    ratio, where = mref.worst(table, r[..., 0].ravel(), r[..., 1].ravel(), k32)
    print('modulation table, bilinear rotation by 0.3 and -2.0 rad: worst |device - reference| / bound', ratio, 'at', where)
    assert ratio <= 1.0, (ratio, where)
    _check_mean('k_rot_bilinear<MOD>, two angles', table, mean, _D_bilinear(2 * NZv * NXv, NYv))


def test_accessor_is_refused_without_object_or_physics(engine_mod):
    def call(eng):
        t, n = ctypes.c_void_p(), ctypes.c_size_t(0)
        return eng.lib.bdof_modulation_table(eng.h, ctypes.byref(t), ctypes.byref(n), None)
    eng = engine_mod.MultisliceEngine(64, 64, 1, 1, with_grad=False)
    eng.set_physics(E, PS, None)
    assert call(eng) == BDOF_ERR_STATE and b'bdof_set_object' in eng.lib.bdof_last_error(eng.h)
    eng = engine_mod.MultisliceEngine(64, 64, 1, 1, with_grad=False)
    eng.set_object_batch(np.zeros((1, 64, 64, 1)), np.zeros((1, 64, 64, 1)))
    assert call(eng) == BDOF_ERR_STATE and b'bdof_set_physics' in eng.lib.bdof_last_error(eng.h)
    eng.set_physics(E, PS, None)
    assert call(eng) == 0                                                              # no probe needed: the mean is then (0, 0)


# =====================================================================================================================================
# Part 2: every consumer at strong phase
# =====================================================================================================================================
def _engine(engine_mod, key, engine, **kw):
    Y, X, name, fp = key
    c = mref.engine_case(*key)
    eng = engine_mod.MultisliceEngine(Y, X, S, B, with_grad=True, engine=engine, **kw)
    eng.set_physics(E, PS, fp)
    eng.set_probe(c['pr'], c['pi'])
    eng.set_object_batch(c['delta32'], c['beta32'])
    return eng, c


def _run_and_check(engine_mod, tag, key, engine, **kw):
    eng, c = _engine(engine_mod, key, engine, **kw)
    cbar_m1 = eng.modulation_table()[1]
    # the structured plane wave rides on a scalar carrier that the table's mean modulates; the gaussian probe of 'inf' on a field
    assert eng.probe_stack == (key[3] == 'inf') and (cbar_m1 != 0) == (key[3] != 'inf')
    wave = eng.forward(B)
    loss = eng.loss_grad(B, c['meas'])
    gd, gb = eng.grad_batch_to_host(B)
    if key[2] == 'wrapped' and key[3] != 'inf':
        assert eng.meas_ref > 0                  # amplitudes near |a0|: the residual stays split
    e = mref.errors(c, wave, loss, gd, gb)
    print('strong phase', tag, key, 'cbar - 1', cbar_m1, 'wave / intensity / loss / g_delta / g_beta rel err', e)
    assert np.all(np.isfinite(wave)) and mref.within(e), e
    return eng, c, (loss, gd, gb)


@pytest.mark.parametrize('key', mref.STREAMING_CASES, ids=str)
def test_streaming_engine(engine_mod, key):
    """k_row_fwd / k_row_bwd."""
    _run_and_check(engine_mod, 'streaming', key, 'streaming')


@pytest.mark.parametrize('key', mref.RESIDENT_CASES, ids=str)
def test_resident_engine(engine_mod, key):
    """EpiMod, EpiBwd, ResPoint of the LDS-resident kernel."""
    _run_and_check(engine_mod, 'resident', key, 'resident')


@pytest.mark.parametrize('key', mref.GENERIC_CASES, ids=str)
def test_generic_engine(engine_mod, key):
    """k_g_modulate / k_g_bwd."""
    _run_and_check(engine_mod, 'generic', key, 'generic')


def test_generic_engine_float64_adjoint(engine_mod):
    """k_g_bwd64."""
    _run_and_check(engine_mod, 'generic, float64 adjoint sweep', (72, 72, 'pi', 1e-4), 'generic', adjoint64=True)


def test_float64_twin(engine_mod):
    """k_f64_modulate evaluates c from the (delta, beta) rows in float64: regime 'pi' at the bounds of
    test_gpu_parity.py::test_float64_transfer_function_path_vs_oracle (loss 1e-8, gradients 2e-7); as there the oracle is given
    the float32-rounded (delta, beta), probe and measurement."""
    key = (64, 64, 'pi', 1e-4)
    eng, c = _engine(engine_mod, key, 'auto')
    delta, beta = c['delta32'].astype(np.float64), c['beta32'].astype(np.float64)
    p64 = (np.asarray(c['pr']) + 1j * np.asarray(c['pi'])).astype(np.complex64)
    pr, pi = p64.real.astype(np.float64), p64.imag.astype(np.float64)
    # ... and the measurement as the device holds it: float32(m - meas_ref), where meas_ref is |a0| under residual splitting and 0
    # without it (choose_residual_split decides on the amplitudes; here |d| ~ 0.4 under |a0| = 1).  Rounding m itself where the device
    # rounds m - |a0| moves the oracle's loss by 4.6e-8 and its gradients by 7.3e-7 / 7.9e-7 — more than these bounds.
    eng.choose_residual_split(c['meas'])                                               # what loss_grad will decide for them
    meas = eng.meas_ref + (c['meas'] - eng.meas_ref).astype(np.float32).astype(np.float64)
    rl, rgd, rgb = orc.multislice_loss_and_grad(delta, beta, pr, pi, E, PS, meas, key[3])
    eng.enable_tf_f64()
    loss = eng.loss_grad(B, meas, f64=True)
    gd, gb = eng.grad_batch_to_host(B)
    e = (abs(loss - rl) / abs(rl), rel(gd, rgd), rel(gb, rgb))
    print('strong phase float64 twin', key, 'loss / g_delta / g_beta rel err', e)
    assert e[0] <= 1e-8 and e[1] <= 2e-7 and e[2] <= 2e-7, e


@pytest.mark.parametrize('name', ['pi', 'absorbing'])
def test_tape_free_adjoint(engine_mod, name):
    """recompute=True: unmodulate_eps divides the marched-back wave by c.  Against the taped engine and the oracle at
    test_gpu_recompute.py's bounds: the same loss, gradients within 2e-5 of the taped ones and 2e-4 of the oracle's."""
    key = (64, 128, name, 1e-4)
    _, c, (l0, gd0, gb0) = _run_and_check(engine_mod, 'taped', key, 'streaming')
    eng, _ = _engine(engine_mod, key, 'streaming', recompute=True)
    l1 = eng.loss_grad(B, c['meas'])
    gd1, gb1 = eng.grad_batch_to_host(B)
    e = (rel(gd1, gd0), rel(gb1, gb0), abs(l1 - c['loss']) / abs(c['loss']), rel(gd1, c['gd']), rel(gb1, c['gb']))
    print('strong phase tape-free adjoint', key, 'g_delta / g_beta vs taped; loss / g_delta / g_beta vs oracle', e)
    assert l1 == l0
    assert e[0] <= 2e-5 and e[1] <= 2e-5, e
    assert e[2] <= 1e-5 and e[3] <= 2e-4 and e[4] <= 2e-4, e


@pytest.mark.parametrize('engine,Y,X', [('streaming', 64, 64), ('generic', 72, 72)])
@pytest.mark.parametrize('b', [2, 3])
def test_slice_binning(engine_mod, engine, Y, X, b):
    """The binning product of the table's factors, against tests/reference_model.py at test_gpu_binning.py's bounds."""
    fp = 1e-4
    c = mref.engine_case(Y, X, 'pi', fp)
    de, be, pr, pi = c['delta_eff'], c['beta_eff'], c['pr'], c['pi']
    ref, _ = ref_model.forward(de, be, pr, pi, E, PS, fp, 'numpy_skip_last', b)
    meas = mref.measurement(ref)
    rl, rgd, rgb, _, _ = ref_model.loss_and_grad(de, be, pr, pi, E, PS, meas, fp, 'numpy_skip_last', b)
    eng = engine_mod.MultisliceEngine(Y, X, S, B, with_grad=True, engine=engine, slice_binning=b)
    eng.set_physics(E, PS, fp)
    eng.set_probe(pr, pi)
    eng.set_object_batch(c['delta32'], c['beta32'])
    wave = eng.forward(B)
    loss = eng.loss_grad(B, meas)
    gd, gb = eng.grad_batch_to_host(B)
    e = (rel(wave, ref), rel(np.abs(wave) ** 2, np.abs(ref) ** 2), abs(loss - rl) / abs(rl), rel(gd, rgd), rel(gb, rgb))
    print('strong phase binning', engine, (Y, X), 'b', b, 'wave / intensity / loss / g_delta / g_beta rel err', e)
    assert mref.within(e), e


@pytest.mark.parametrize('ks,probe', [(17, 'plane'), (5, 'structured')])
def test_convolution_propagator(engine_mod, ks, probe):
    """Both convolution kernels' tap counts; k from numpy's pi (the same float32 as the transfer-function path's at 5 keV / 1 nm; the table is built again for it).  Against orc.cnn_loss_and_grad at
    test_gpu_conv.py's bounds: intensity 1e-5, wave 5e-6, loss 2e-5, gradients 2e-4 away from the corner block that the
    renormalisation of propagation.py:109-110 feeds, 2e-2 inside it."""
    Y, X, fp, k = 64, 128, 1e-4, mref.K64_CONV
    d32, b32 = mref.regime('pi', (B, Y, X, S), k64=k)
    de, be = mref.oracle_inputs(d32, b32, k64=k)
    pr, pi = (np.ones((Y, X)), np.zeros((Y, X))) if probe == 'plane' else mref.probe('structured', Y, X)
    pr32, pi32 = pr.astype(np.float32), pi.astype(np.float32)
    psize = [PS] * 3
    eng = engine_mod.MultisliceEngine(Y, X, S, B, with_grad=True)
    eng.set_physics(E, PS, fp)
    eng.set_conv(E, psize, ks)
    assert eng._conv_k64 == k
    eng.set_probe(pr, pi)
    eng.set_object_batch(d32, b32)
    wave = eng.forward(B, conv=True)
    ref = orc.multislice_propagate_cnn(de, be, pr32, pi32, E, psize, kernel_size=ks, free_prop_cm=fp)
    meas = mref.measurement(ref)
    loss = eng.loss_grad(B, meas, conv=True)
    gd, gb = eng.grad_batch_to_host(B)
    rl, rgd, rgb = orc.cnn_loss_and_grad(de, be, pr32, pi32, E, psize, meas, kernel_size=ks, free_prop_cm=fp)
    away = np.ones(gd.shape, dtype=bool)
    away[0, :ks, :ks, :] = False
    e = (rel(wave, ref), rel(np.abs(wave) ** 2, np.abs(ref) ** 2), abs(loss - rl) / abs(rl), rel(gd[away], rgd[away]), rel(gb[away], rgb[away]),
         rel(gd[~away], rgd[~away]), rel(gb[~away], rgb[~away]))
    print('strong phase conv', ks, probe, 'wave / intensity / loss / g_delta, g_beta away from the corner / in it rel err', e)
    assert e[0] <= 5e-6 and e[1] <= 1e-5 and e[2] <= 2e-5, e
    assert e[3] <= 2e-4 and e[4] <= 2e-4 and e[5] <= 2e-2 and e[6] <= 2e-2, e


def _volume(n, seed):
    d32, b32 = mref.regime('pi', (n, n, n), seed=seed)
    return (d32, b32) + mref.oracle_inputs(d32, b32)


def test_fullfield_solver(engine_mod):
    """64^3, two angles through the rotation tables, regime 'pi': loss and volume gradient against orc.fullfield_loss_and_grad at
    test_gpu_parity.py's bounds (loss 1e-5, gradients 2e-4)."""
    from beyond_dof_amd.solver import FullfieldSolver
    n, n_theta, fp = 64, 4, 1e-4
    d32, b32, de, be = _volume(n, 3)
    coords = orc.rotation_lookup([n, n, n], n_theta)
    idx = np.array([1, 3])
    one, zero = np.ones((n, n)), np.zeros((n, n))
    rot = np.stack([orc.apply_rotation(np.stack([de, be], axis=3), coords[j]) for j in idx])
    ref, _ = orc.multislice_propagate_batch_numpy(rot[..., 0], rot[..., 1], one, zero, E, PS, fp, rot[..., 0].shape, return_probe_array=False)
    prj = np.zeros((n_theta, n, n))
    prj[idx] = mref.measurement(ref)
    s = FullfieldSolver(n, n, n, n_theta, len(idx), E, PS, free_prop_cm=fp, coord_ls=coords)
    s.set_volume(d32, b32)
    s.set_measurements(prj)
    assert s.eng.meas_ref == 0                   # amplitudes of 1e-4 |a0|: float32(m - |a0|) would cost them three digits
    w = s.forward_angles(idx)
    loss = s.loss_and_grad(idx)
    gd, gb = s.gradient_to_host()
    rl, rgd, rgb = orc.fullfield_loss_and_grad(de, be, coords, idx, prj[idx], one, zero, E, PS, free_prop_cm=fp, with_reg=False)
    e = (rel(w, ref), rel(np.abs(w) ** 2, np.abs(ref) ** 2), abs(loss - rl) / abs(rl), rel(gd, rgd), rel(gb, rgb))
    print('strong phase FullfieldSolver 64^3 wave / intensity / loss / g_delta / g_beta rel err', e)
    assert e[2] <= 1e-5 and e[3] <= 2e-4 and e[4] <= 2e-4, e


def test_ptycho_solver(engine_mod):
    """64^3 object, 64-pixel probe, four positions, regime 'pi'.  Only the centred window lies inside a volume of the probe's own
    size: the other three hang over its edges, so rows and columns of exact-zero table entries (a factor of exactly 1) sit beside
    strong ones.  Against orc.ptycho_loss_and_grad at test_gpu_ptycho.py's bounds for a wave that no carrier holds — intensity
    1.2e-5, loss 5e-5, gradients 1e-3: its tighter set (5e-7, 2e-6, 1e-4) is for a weak object, where the scattered wave that
    runs through the float32 transforms is a small part of the whole; here it is all of it, and the oracle's model in plain
    complex64 (modulation_reference.c64_loss_and_grad on these windows) reaches 6.0e-6, 1.7e-5 and 1.1e-4 / 7.3e-4."""
    from beyond_dof_amd.solver import PtychoSolver
    n, n_theta, psz, i_theta = 64, 4, (64, 64), 2
    d32, b32, de, be = _volume(n, 3)
    coords = orc.rotation_lookup([n, n, n], n_theta)
    pos = np.array([(32, 32), (32, 33), (10, 50), (60, 8)])
    sel = np.arange(len(pos))
    prr, pii = orc.gaussian_probe(psz, 6., 6., 0.5)
    pad, half = orc.ptycho_pad_amounts(pos, psz, (n, n, n))
    rot = orc.apply_rotation(np.stack([de, be], axis=3), coords[i_theta])
    obj_pad = np.pad(rot, ((pad[0, 0], pad[0, 1]), (pad[1, 0], pad[1, 1]), (0, 0), (0, 0)), mode='constant')
    subs = np.stack([obj_pad[p[0] + pad[0, 0] - half[0]:p[0] + pad[0, 0] - half[0] + psz[0],
                             p[1] + pad[1, 0] - half[1]:p[1] + pad[1, 0] - half[1] + psz[1]] for p in pos])
    assert np.all(subs[0] != 0) and all(np.any(np.all(subs[i] == 0, axis=(1, 2, 3))) or np.any(np.all(subs[i] == 0, axis=(0, 2, 3))) for i in (1, 2, 3))
    ref, _ = orc.multislice_propagate_batch_numpy(subs[..., 0], subs[..., 1], prr, pii, E, PS, 'inf', subs[..., 0].shape, return_probe_array=False)
    meas = mref.measurement(ref)
    s = PtychoSolver((n, n, n), psz, pos, n_theta, len(pos), E, PS, prr, pii, coord_ls=coords)
    s.set_volume(d32, b32)
    w = s.forward(i_theta, sel)
    loss = s.loss_and_grad(i_theta, sel, meas)
    gd, gb = s.gradient_to_host()
    rl, rgd, rgb = orc.ptycho_loss_and_grad(de, be, coords[i_theta], pos, pos[sel], meas, prr, pii, psz, E, PS)
    e = (rel(w, ref), rel(np.abs(w) ** 2, np.abs(ref) ** 2), abs(loss - rl) / abs(rl), rel(gd, rgd), rel(gb, rgb))
    print('strong phase PtychoSolver 64^3 wave / intensity / loss / g_delta / g_beta rel err', e)
    assert e[1] <= 1.2e-5 and e[2] <= 5e-5 and e[3] <= 1e-3 and e[4] <= 1e-3, e
