"""The free-space step of the rocFFT paths, fields <- F^-1(h * F fields) (bdof_fields_free_step, include/bdof.h), and what is built
on it: the step on the auxiliary stream, the float64 range sweep and the float64 twin of the transfer-function model.  Non-square
fields (B = 3, NX = 24, NY = 40, the generic engine's kind of shape), so that a table read in the wrong order cannot pass."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, NX, NY, S = 3, 24, 40, 3

# Relative L2 error of one step against numpy in complex128 at these shapes, on inputs rounded to the step's precision, as
# measured before the step became one function and reproduced to the digit after (MEASUREMENTS.md, "rocFFT paths"): complex64
# 1.63e-7 (h) / 1.64e-7 (conj h), complex128 4.53e-16 / 4.58e-16.  The bounds are four times the larger of each pair: room for
# another plan choice in another rocFFT release, not for another algorithm.
MEASURED = {0: 1.64e-7, 1: 4.58e-16}
BOUND = {p: 4 * e for p, e in MEASURED.items()}


@pytest.fixture(scope='module')
def eng():
    """A generic-engine ctx of the shape, bound to an all-vacuum object, with a unit wave."""
    import __graft_entry__ as entry
    entry.build()
    from beyond_dof_amd import engine
    e = engine.MultisliceEngine(NY, NX, S, B, with_grad=True)
    e.set_physics(5000., 1e-7, None)
    e.set_probe(np.ones((NY, NX)), np.zeros((NY, NX)))
    e.set_object_batch(np.zeros((B, NY, NX, S)), np.zeros((B, NY, NX, S)))
    return e


@pytest.fixture(scope='module')
def problem():
    """Fields [B][NX][NY] and a unit-modulus table H[kx][ky], in float64; the library's table carries 1 / (NX NY)."""
    rng = np.random.default_rng(7)
    f = rng.normal(size=(B, NX, NY)) + 1j * rng.normal(size=(B, NX, NY))
    H = np.exp(2j * np.pi * rng.random((NX, NY)))
    return f, H


def _ctype(is_double):
    return np.complex128 if is_double else np.complex64


def _step(eng, f, H, conj_h, is_double, aux=None):
    """One step of the device on f with the table H / (NX NY), both rounded to the precision; aux: None for the ctx's stream, else
    'src' / 'inplace' for the auxiliary stream (with / without a source to copy from first) and the join."""
    from beyond_dof_amd._lib import DeviceBuffer
    ct = _ctype(is_double)
    h = DeviceBuffer.from_host(eng.ctx, (H / (NX * NY)).astype(ct))
    if aux == 'src':
        src, d = DeviceBuffer.from_host(eng.ctx, f.astype(ct)), DeviceBuffer.zeros(eng.ctx, f.shape, ct)
    else:
        src, d = None, DeviceBuffer.from_host(eng.ctx, f.astype(ct))
    if aux is None:
        eng.ctx.check(eng.lib.bdof_fields_free_step(eng.h, d.ptr, B, NX, NY, h.ptr, conj_h, is_double))
    else:
        eng.ctx.check(eng.lib.bdof_fields_free_step_aux(eng.h, d.ptr, src.ptr if src else None, B, NX, NY, h.ptr, conj_h, is_double))
        # one auxiliary step in flight at a time
        assert eng.lib.bdof_fields_free_step_aux(eng.h, d.ptr, None, B, NX, NY, h.ptr, conj_h, is_double) != 0
        assert eng.lib.bdof_last_error(eng.h) == b'an auxiliary step is in flight: bdof_aux_join first'
        eng.ctx.check(eng.lib.bdof_aux_join(eng.h))
    eng.ctx.sync()
    return d.download()


@pytest.fixture(scope='module')
def plain(eng, problem):
    """The plain step's result for (is_double, conj_h): computed once, compared against by the tests below."""
    f, H = problem
    return {(p, cj): _step(eng, f, H, cj, p) for p in (0, 1) for cj in (0, 1)}


@pytest.mark.parametrize('conj_h', [0, 1])
@pytest.mark.parametrize('is_double', [0, 1])
def test_free_step_vs_numpy(problem, plain, is_double, conj_h):
    f, H = problem
    ct = _ctype(is_double)
    f_in, h_in = f.astype(ct).astype(np.complex128), (H / (NX * NY)).astype(ct).astype(np.complex128) * (NX * NY)
    ref = np.fft.ifft2(np.fft.fft2(f_in, axes=(1, 2)) * (np.conj(h_in) if conj_h else h_in), axes=(1, 2))
    err = np.linalg.norm(plain[is_double, conj_h] - ref) / np.linalg.norm(ref)
    print('free step, is_double', is_double, 'conj_h', conj_h, ': relative L2 error', err, 'bound', BOUND[is_double])
    assert err <= BOUND[is_double]


@pytest.mark.parametrize('aux', ['src', 'inplace'])
@pytest.mark.parametrize('is_double', [0, 1])
def test_aux_step_equals_the_plain_step(eng, problem, plain, is_double, aux):
    f, H = problem
    for conj_h in (0, 1):
        assert np.array_equal(_step(eng, f, H, conj_h, is_double, aux), plain[is_double, conj_h])


@pytest.mark.parametrize('prop_last', [0, 1])
def test_forward_range_f64_through_vacuum_is_plain_steps(eng, problem, prop_last):
    """In vacuum the modulation writes nothing: nz = 3 slices are 2 steps, or 3 with a step after the last."""
    from beyond_dof_amd._lib import DeviceBuffer
    f, H = problem
    h = DeviceBuffer.from_host(eng.ctx, H / (NX * NY))
    d = DeviceBuffer.from_host(eng.ctx, f)
    eng.ctx.check(eng.lib.bdof_forward_range_f64(eng.h, B, None, None, None, 0, S, d.ptr, h.ptr, float(eng.k), prop_last))
    ref = DeviceBuffer.from_host(eng.ctx, f)
    for _ in range(S - 1 + prop_last):
        eng.ctx.check(eng.lib.bdof_fields_free_step(eng.h, ref.ptr, B, NX, NY, h.ptr, 0, 1))
    eng.ctx.sync()
    assert np.array_equal(d.download(), ref.download())


def test_tf_f64_twin_vacuum_unit_wave_non_square(eng):
    """|psi| stays 1 through vacuum, on the generic engine's kind of shape (test_gpu_parity.py asserts it on 64 x 64)."""
    eng.enable_tf_f64()
    assert abs(eng.loss_grad(B, np.ones((B, NY, NX)), f64=True)) <= 1e-20
