"""bdof_shell_correlation (csrc/bdof_shells.h) and beyond_dof_amd.resolution on the device against the float64 numpy restatement
tests/fsc_reference.py: both sides compute in float64 from the same float32 volumes, so the bounds are those of two double
transforms (about eps log2 N ~ 4e-15 of the spectrum's rms per bin; white inputs keep every shell's power near that rms) with
four orders of margin for rocFFT's constant: 1e-10.  Inputs have the volumes' real magnitudes, delta ~ 1e-6 and beta ~ 1e-7,
so an absolute epsilon anywhere would show."""
import ctypes
import functools
import os

import numpy as np
import pytest

import fsc_reference as fr

pytestmark = pytest.mark.gpu

BDOF_ERR_SIZE = -3
CASES = ('same', 'noisy', 'independent')


@pytest.fixture(scope='module')
def ctx():
    import __graft_entry__ as entry
    entry.build()
    from beyond_dof_amd import _lib
    return _lib.Context(0)


def _white_rows(shape, seed):
    """[X][Z][Y][2] float32: white noise, delta scaled by 1e-6 and beta by 1e-7"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(tuple(shape) + (2,)) * np.array([1e-6, 1e-7])).astype(np.float32)


def _pair(rows):
    return rows[..., 0].astype(np.float64), rows[..., 1].astype(np.float64)


@functools.lru_cache(maxsize=None)
def _case(shape, case):
    """(rows_a, rows_b, reference sums over all shells) of one shape and case; computed once, never written"""
    a = _white_rows(shape, 10)
    if case == 'same':
        b = a.copy()
    elif case == 'noisy':
        b = (a + 0.7 * _white_rows(shape, 11)).astype(np.float32)
    else:
        b = _white_rows(shape, 12)
    ref = fr.shell_sums(_pair(a), _pair(b))
    for arr in (a, b, ref):
        arr.setflags(write=False)
    return a, b, ref


def _device_sums(ctx, bufs, shape, n_shells):
    out = np.full((max(n_shells, 1), 7), np.nan)
    rc = ctx.lib.bdof_shell_correlation(ctx.handle, bufs[0].ptr, bufs[1].ptr, shape[0], shape[1], shape[2], n_shells,
                                        out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    return rc, out


def _upload(ctx, *rows):
    from beyond_dof_amd._lib import DeviceBuffer
    return [DeviceBuffer.from_host(ctx, r) for r in rows]


def _compare(dev, ref, label):
    """the bounds of the module docstring; prints the worst figures before it asserts"""
    assert np.array_equal(dev[:, 0], ref[:, 0])
    worst = {'power': 0.0, 'cross': 0.0, 'curve': 0.0}
    for j in (1, 4):
        for col in (j + 1, j + 2):
            ok = ref[:, col] > 0
            worst['power'] = max(worst['power'], float(np.max(np.abs(dev[ok, col] - ref[ok, col]) / ref[ok, col])))
            assert np.all(dev[~ok, col] == 0)
        scale = np.sqrt(ref[:, j + 1] * ref[:, j + 2])
        ok = scale > 0
        worst['cross'] = max(worst['cross'], float(np.max(np.abs(dev[ok, j] - ref[ok, j]) / scale[ok])))
    for cd, cr in zip(fr.curves(dev), fr.curves(ref)):
        worst['curve'] = max(worst['curve'], float(np.max(np.abs(cd - cr))))
    print('shell correlation {}: worst relative power error {power:.3e}, cross error / sqrt(Pa Pb) {cross:.3e}, curve error {curve:.3e}'.format(
        label, **worst))
    assert worst['power'] <= 1e-10 and worst['cross'] <= 1e-10 and worst['curve'] <= 1e-10, worst


@pytest.mark.parametrize('case', CASES)
@pytest.mark.parametrize('shape', fr.SHAPES)
def test_sums_and_curves_against_the_restatement(ctx, shape, case):
    a, b, ref = _case(shape, case)
    rc, dev = _device_sums(ctx, _upload(ctx, a, b), shape, len(ref))
    assert rc == 0
    _compare(dev, ref, '{} {}'.format(shape, case))
    # Parseval on the device sums: sum_s P(s) = N sum x^2
    n = float(np.prod(shape))
    for col, vol in ((2, a[..., 0]), (3, b[..., 0]), (5, a[..., 1]), (6, b[..., 1])):
        want = n * np.sum(vol.astype(np.float64) ** 2)
        assert abs(dev[:, col].sum() - want) <= 1e-12 * want
    assert dev[:, 0].sum() == n


def test_shells_beyond_n_shells_are_dropped(ctx):
    shape = (16, 12, 20)
    a, b, ref = _case(shape, 'noisy')
    rc, dev = _device_sums(ctx, _upload(ctx, a, b), shape, 4)
    assert rc == 0
    _compare(dev, ref[:4], '{} first four shells'.format(shape))


def test_more_shells_than_one_table_holds(ctx):
    """A ring correlation with more shells than one wave's table in LDS holds (65536 / 56 = 1170): the call makes two passes."""
    shape = (1700, 1, 1700)
    a, b, ref = _case(shape, 'noisy')
    assert len(ref) > 1170
    rc, dev = _device_sums(ctx, _upload(ctx, a, b), shape, len(ref))
    assert rc == 0
    _compare(dev, ref, str(shape))


@pytest.mark.parametrize('shape', [(32, 32, 32), (16, 12, 20)])
def test_channels_do_not_mix(ctx, shape):
    a, b, _ = _case(shape, 'independent')
    n_shells = fr.n_shells_all(shape)
    # delta_b = delta_a, beta_b independent
    mixed = np.stack([a[..., 0], b[..., 1]], axis=-1)
    rc, dev = _device_sums(ctx, _upload(ctx, a, mixed), shape, n_shells)
    assert rc == 0
    assert np.all(dev[:, 0] > 0)                                     # every shell up to the corner holds points
    bound = 4 / np.sqrt(dev[:, 0])
    cd, cb = fr.curves(dev)
    assert np.abs(cd - 1).max() <= 1e-12 and np.all(np.abs(cb) <= bound)
    # b = (beta_a, delta_a): the channels swapped
    swapped = np.ascontiguousarray(a[..., ::-1])
    rc, dev = _device_sums(ctx, _upload(ctx, a, swapped), shape, n_shells)
    assert rc == 0
    # the swapped pair has other magnitudes than a: white and independent, each curve within 4 / sqrt(n) of 0
    assert all(np.all(np.abs(c) <= bound) for c in fr.curves(dev))


def test_bits(ctx):
    shape = (18, 10, 14)
    a, b, ref = _case(shape, 'noisy')
    bufs = _upload(ctx, a, b)
    rc1, first = _device_sums(ctx, bufs, shape, len(ref))
    rc2, second = _device_sums(ctx, bufs, shape, len(ref))
    assert rc1 == 0 and rc2 == 0 and first.tobytes() == second.tobytes()
    assert bufs[0].download().tobytes() == a.tobytes() and bufs[1].download().tobytes() == b.tobytes()
    # one pointer for both volumes
    rc, same = _device_sums(ctx, [bufs[0], bufs[0]], shape, len(ref))
    assert rc == 0 and np.array_equal(same[:, 0], ref[:, 0]) and np.all(ref[:, 0] > 0)
    for c in fr.curves(same):
        assert np.abs(c - 1).max() <= 4e-16
    assert bufs[0].download().tobytes() == a.tobytes()


def test_refusals(ctx):
    from beyond_dof_amd import resolution
    from beyond_dof_amd._lib import DeviceBuffer
    buf = DeviceBuffer.zeros(ctx, (8, 8, 8, 2), np.float32)
    assert _device_sums(ctx, [buf, buf], (3, 8, 8), 4)[0] == BDOF_ERR_SIZE            # Nref < 4
    assert _device_sums(ctx, [buf, buf], (8, 8, 8), 0)[0] == BDOF_ERR_SIZE            # n_shells = 0
    assert _device_sums(ctx, [buf, buf], (1, 16, 1), 4)[0] == BDOF_ERR_SIZE           # one long axis only
    assert _device_sums(ctx, [buf, buf], (8, 8, 8), 4)[0] == 0
    z = np.zeros((8, 8, 8))
    with pytest.raises(ValueError):
        resolution.fourier_shell_correlation((z, z), (z[:, :, :6], z[:, :, :6]), ctx=ctx)
    with pytest.raises(ValueError):
        resolution.fourier_shell_correlation(buf, DeviceBuffer.zeros(ctx, (8, 6, 8, 2), np.float32), ctx=ctx)


def test_module_functions(ctx):
    """fourier_shell_correlation on host (y, x, z) pairs and fourier_ring_correlation on (y, x) images: the record's shells,
    frequencies and curves are those of the restatement on the same arrays."""
    from beyond_dof_amd import resolution
    a, b, _ = _case((16, 12, 20), 'noisy')                          # rows [X][Z][Y] -> (y, x, z)
    host = lambda r: (r[..., 0].transpose(2, 0, 1), r[..., 1].transpose(2, 0, 1))
    rec = resolution.fourier_shell_correlation(host(a), host(b), psize_cm=1e-7, ctx=ctx)
    assert rec.nref == 12 and np.array_equal(rec.shell, np.arange(1, 6)) and np.array_equal(rec.frequency, np.arange(1, 6) / 12.0)
    ref = fr.shell_sums(_pair(a), _pair(b), 6)[1:]
    assert np.array_equal(rec.n_points, ref[:, 0]) and np.array_equal(rec.sums[:, 0], ref[:, 0])
    for got, want in zip((rec.fsc_delta, rec.fsc_beta), fr.curves(ref)):
        assert np.abs(got - want).max() <= 1e-10
    for r in resolution.resolution(rec, 'half-bit').values():
        assert r is None or (1 <= r.shell <= 5 and abs(r.half_period - 1e-7 * 12 / (2 * r.shell)) < 1e-20)
    a2, b2, _ = _case((24, 1, 16), 'noisy')
    img = lambda r: (r[:, 0, :, 0].T, r[:, 0, :, 1].T)
    ring = resolution.fourier_ring_correlation(img(a2), img(b2), ctx=ctx)
    ref2 = fr.shell_sums(_pair(a2), _pair(b2), 8)[1:]
    assert ring.nref == 16 and np.array_equal(ring.n_points, ref2[:, 0])
    for got, want in zip((ring.fsc_delta, ring.fsc_beta), fr.curves(ref2)):
        assert np.abs(got - want).max() <= 1e-10


def test_solver_compares_its_resident_volume():
    import __graft_entry__ as entry
    entry.build()
    from beyond_dof_amd import resolution
    from beyond_dof_amd.solver import FullfieldSolver
    from oracle import bdof_oracle as orc
    n, n_theta = 16, 4
    rng = np.random.default_rng(3)
    d, b = rng.normal(8.7e-7, 1e-7, (n, n, n)).astype(np.float32), rng.normal(5.1e-8, 1e-8, (n, n, n)).astype(np.float32)
    other = (d + rng.normal(0, 1e-7, d.shape).astype(np.float32), b + rng.normal(0, 1e-8, b.shape).astype(np.float32))
    s = FullfieldSolver(n, n, n, n_theta, 2, 5000., 1e-7, free_prop_cm=1e-4, coord_ls=orc.rotation_lookup([n, n, n], n_theta))
    s.set_volume(d, b)
    rec = s.shell_correlation(other)
    want = resolution.fourier_shell_correlation((d, b), other, ctx=s.ctx)
    assert rec.sums.tobytes() == want.sums.tobytes() and rec.fsc_delta.tobytes() == want.fsc_delta.tobytes()
    ref = fr.shell_sums(tuple(v.astype(np.float64) for v in (d, b)), tuple(v.astype(np.float64) for v in other), n // 2)[1:]
    for got, curve in zip((rec.fsc_delta, rec.fsc_beta), fr.curves(ref)):
        assert np.abs(got - curve).max() <= 1e-10
    got = s.get_volume()
    assert got[0].tobytes() == d.tobytes() and got[1].tobytes() == b.tobytes()
    # against another solver's resident volume: the same bits again
    s2 = FullfieldSolver(n, n, n, n_theta, 2, 5000., 1e-7, free_prop_cm=1e-4, coord_ls=orc.rotation_lookup([n, n, n], n_theta))
    s2.set_volume(*other)
    assert s.shell_correlation(s2).sums.tobytes() == want.sums.tobytes()


def _spheres(n, rng):
    """hard-edged spheres: a phantom with power in every shell"""
    z, y, x = np.mgrid[:n, :n, :n]
    d = np.zeros((n, n, n))
    for _ in range(5):
        c = rng.uniform(n * 0.3, n * 0.7, size=3)
        d[(z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2 <= rng.uniform(n * 0.1, n * 0.2) ** 2] += 1e-6
    return d.astype(np.float32), (0.1 * d).astype(np.float32)


def test_reconstruct_fullfield_reports_the_resolution(tmp_path, monkeypatch):
    """the end-to-end pattern of tests/test_gpu_fullfield.py at 16^3, one epoch, with fsc_reference = the phantom"""
    import __graft_entry__ as entry
    entry.build()
    from beyond_dof_amd import h5io
    from beyond_dof_amd.fullfield import reconstruct_fullfield
    from oracle import bdof_oracle as orc
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(0)
    n, n_theta, mb, fp = 16, 4, 2, 1e-4
    true_d, true_b = _spheres(n, rng)
    coords = orc.rotation_lookup([n, n, n], n_theta)
    one, zero = np.ones((n, n)), np.zeros((n, n))
    rot = np.stack([orc.apply_rotation(np.stack([true_d, true_b], axis=3).astype(np.float64), c) for c in coords])
    prj, _ = orc.multislice_propagate_batch_numpy(rot[..., 0], rot[..., 1], one, zero, 5000., 1e-7, fp, rot[..., 0].shape,
                                                  return_probe_array=False)
    os.makedirs('case')
    h5io.write_dataset('case/data.h5', 'exchange/data', prj.astype(np.complex64))
    init = [np.clip(rng.normal(8.7e-7, 1e-7, size=(n, n, n)), 0, None), np.clip(rng.normal(5.1e-8, 1e-8, size=(n, n, n)), 0, None)]
    kw = dict(theta_st=0, theta_end=2 * np.pi, n_epochs=1, learning_rate=1e-7, minibatch_size=mb, energy_ev=5000, psize_cm=1e-7,
              free_prop_cm=fp, save_path='case', initial_guess=init, shrink_cycle=None, seed=7, alpha_d=1.5e-8, alpha_b=1.5e-9, gamma=1e-11)
    with pytest.raises(ValueError):                                  # before any device work
        reconstruct_fullfield('data.h5', output_folder='bad', fsc_reference=(true_d[:, :, :8], true_b[:, :, :8]), **kw)
    assert not os.path.exists(os.path.join('case', 'bad'))
    d, b = reconstruct_fullfield('data.h5', output_folder='with', fsc_reference=(true_d, true_b), **kw)
    d0, b0 = reconstruct_fullfield('data.h5', output_folder='without', **kw)
    assert d.tobytes() == d0.tobytes() and b.tobytes() == b0.tobytes()
    out = os.path.join('case', 'with')
    rec = np.load(os.path.join(out, 'fsc.npy'), allow_pickle=True).item()
    ref = fr.shell_sums((d.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)),
                        (true_d.astype(np.float64), true_b.astype(np.float64)), n // 2)[1:]
    assert np.array_equal(rec['shell'], np.arange(1, n // 2)) and np.array_equal(rec['n_points'], ref[:, 0])
    for name, want in zip(('fsc_delta', 'fsc_beta'), fr.curves(ref)):
        print(name, rec[name], 'worst error', np.abs(rec[name] - want).max())
        assert np.abs(rec[name] - want).max() <= 1e-10
    lines = open(os.path.join(out, 'summary.txt')).read().splitlines()
    assert sum(l.startswith('resolution_delta') for l in lines) == 1 and sum(l.startswith('resolution_beta') for l in lines) == 1
    assert not os.path.exists(os.path.join('case', 'without', 'fsc.npy'))
    assert 'resolution_' not in open(os.path.join('case', 'without', 'summary.txt')).read()
    # the reference as two .npy paths: the same curves
    np.save('ref_d.npy', true_d)
    np.save('ref_b.npy', true_b)
    reconstruct_fullfield('data.h5', output_folder='paths', fsc_reference=('ref_d.npy', 'ref_b.npy'), fsc_threshold=0.5, **kw)
    rec2 = np.load(os.path.join('case', 'paths', 'fsc.npy'), allow_pickle=True).item()
    assert rec2['fsc_delta'].tobytes() == rec['fsc_delta'].tobytes()


def test_reconstruct_ptychography_reports_the_resolution(tmp_path, monkeypatch):
    """fsc_reference= of the second entry point: a one-epoch run on made-up far-field amplitudes (the fit is not the subject), the
    report against the restatement on the returned volume."""
    import __graft_entry__ as entry
    entry.build()
    from beyond_dof_amd import h5io
    from beyond_dof_amd.ptychography import reconstruct_ptychography
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(1)
    n, n_theta, psz = 32, 2, (32, 32)
    pos = [(y, x) for y in (8, 24) for x in (8, 24)]
    data = (psz[0] * np.abs(rng.normal(1.0, 0.1, size=(n_theta, len(pos)) + psz))).astype(np.complex64)
    os.makedirs('case')
    h5io.write_dataset('case/data.h5', 'exchange/data', data)
    ref = tuple((s * rng.random((n, n, n))).astype(np.float32) for s in (1e-6, 1e-7))
    init = [np.clip(rng.normal(8.7e-7, 1e-7, size=(n, n, n)), 0, None), np.clip(rng.normal(5.1e-8, 1e-8, size=(n, n, n)), 0, None)]
    kw = dict(theta_st=0, theta_end=2 * np.pi, n_epochs=1, learning_rate=1e-7, minibatch_size=2, energy_ev=5000, psize_cm=1e-7,
              save_path='case', initial_guess=init, probe_type='gaussian', seed=3, probe_mag_sigma=6., probe_phase_sigma=6.,
              probe_phase_max=0.5, adjoint_precision='float32')
    with pytest.raises(ValueError):
        reconstruct_ptychography('data.h5', pos, psz, (n, n, n), output_folder='bad', fsc_reference=(ref[0][:16], ref[1][:16]), **kw)
    d, b = reconstruct_ptychography('data.h5', pos, psz, (n, n, n), output_folder='with', fsc_reference=ref, fsc_threshold=0.143, **kw)
    d0, b0 = reconstruct_ptychography('data.h5', pos, psz, (n, n, n), output_folder='without', **kw)
    assert d.tobytes() == d0.tobytes() and b.tobytes() == b0.tobytes()
    rec = np.load(os.path.join('case', 'with', 'fsc.npy'), allow_pickle=True).item()
    want = fr.shell_sums((d.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)),
                         tuple(v.astype(np.float64) for v in ref), n // 2)[1:]
    assert np.array_equal(rec['n_points'], want[:, 0])
    for name, curve in zip(('fsc_delta', 'fsc_beta'), fr.curves(want)):
        assert np.abs(rec[name] - curve).max() <= 1e-10
    text = open(os.path.join('case', 'with', 'summary.txt')).read()
    assert text.count('resolution_delta') == 1 and text.count('resolution_beta') == 1 and '0.143 threshold' in text
    assert not os.path.exists(os.path.join('case', 'without', 'fsc.npy'))
    assert 'resolution_' not in open(os.path.join('case', 'without', 'summary.txt')).read()
