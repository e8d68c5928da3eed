"""The C library's admission check (csrc/bdof_capi.hip: MODEL_OPTIONS, admit) on the device: every entry point that does not
carry slice binning, or several detector planes, refuses a ctx that runs with the option — BDOF_ERR_STATE and the text below
through bdof_last_error, before it touches anything — and the ctx goes on as it was."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BDOF_ERR_STATE = -2
Y = X = 64
S, B = 4, 1
E, PS = 5000., 1e-7
BINNING = ' does not carry slice binning: it would run the unbinned model (bdof_set_slice_binning)'
PLANES = ' does not carry detector planes: bdof_set_detector_planes(ctx, 1, NULL, NULL) first'
K = 0.025           # (any number: 2 pi dz / lambda of some step)


def _calls(lib, h, dev, host):
    """(the name the refusal begins with, the call) of every entry point that refuses an option, with well-formed arguments:
    dev — a zeroed device buffer, host — a zeroed host array, each larger than anything a call could read or write."""
    none3 = (None, None, None)
    return [
        ('bdof_forward_range', lambda: lib.bdof_forward_range(h, B, *none3, 0, 2, dev, dev, 1)),
        ('bdof_set_range_carrier', lambda: lib.bdof_set_range_carrier(h, dev, B, 0, 2)),
        ('bdof_forward_range_h', lambda: lib.bdof_forward_range_h(h, B, *none3, 0, 2, dev, dev, 1, dev)),
        ('bdof_adjoint_range', lambda: lib.bdof_adjoint_range(h, B, *none3, 0, 2, dev, dev, dev, dev)),
        ('bdof_range_carrier_build', lambda: lib.bdof_range_carrier_build(h, dev, dev, B, X, Y, dev, 2)),
        ('bdof_forward_range_f64', lambda: lib.bdof_forward_range_f64(h, B, *none3, 0, 2, dev, dev, K, 1)),
        ('bdof_set_conv_f64', lambda: lib.bdof_set_conv_f64(h, host, host, 5, 1.0, 0.0, K)),
        ('bdof_set_conv_f64_detector', lambda: lib.bdof_set_conv_f64_detector(h, host)),
        ('bdof_loss_grad_conv_f64', lambda: lib.bdof_loss_grad_conv_f64(h, B, *none3, dev, 0.0)),
        ('bdof_set_tf_f64', lambda: lib.bdof_set_tf_f64(h, host, host, host, K)),
        ('bdof_loss_grad_tf_f64', lambda: lib.bdof_loss_grad_tf_f64(h, B, *none3, dev, 0.0)),
        ('bdof_set_conv', lambda: lib.bdof_set_conv(h, host, host, 5, 1.0, 0.0, 1.0, 0.0, K)),
        ('bdof_set_conv_taps_f64', lambda: lib.bdof_set_conv_taps_f64(h, host, host, 1.0, 0.0)),
        ('bdof_set_conv_probe_stack', lambda: lib.bdof_set_conv_probe_stack(h, host, host, 1.0, 0.0, 1.0, 0.0)),
        ('bdof_forward_conv', lambda: lib.bdof_forward_conv(h, B, *none3, dev)),
        ('bdof_loss_grad_conv', lambda: lib.bdof_loss_grad_conv(h, B, *none3, dev, None)),
        ('bdof_set_object_bilinear', lambda: lib.bdof_set_object_bilinear(h, dev, X, S, Y, host, B, 0)),
        ('a carrier field (bdof_set_probe_stack)', lambda: lib.bdof_set_probe_stack(h, host, host)),
        ('a carrier field (bdof_set_probe_field)', lambda: lib.bdof_set_probe_field(h, host, host, host)),
    ]


# what carries the one option and not the other
CARRIES = {'binning': ('a carrier field (bdof_set_probe_stack)', 'a carrier field (bdof_set_probe_field)'), 'planes': ('bdof_set_object_bilinear',)}


@pytest.mark.parametrize('option', ['binning', 'planes'])
def test_entry_points_refuse_an_option_they_do_not_carry_and_leave_the_ctx_whole(option):
    import __graft_entry__ as entry
    entry.build()
    from beyond_dof_amd import _lib
    from beyond_dof_amd.engine import MultisliceEngine
    rng = np.random.default_rng(0)
    delta = rng.uniform(0, 2e-5, size=(B, Y, X, S))
    eng = MultisliceEngine(Y, X, S, B, with_grad=True, slice_binning=2 if option == 'binning' else 1)
    eng.set_physics(E, PS, 1e-4 if option == 'binning' else [5e-5, 1e-4])
    eng.set_probe(np.ones((Y, X)), np.zeros((Y, X)))
    eng.set_object_batch(delta, 0.1 * delta)
    meas = 1 + 0.05 * rng.normal(size=(B, Y, X) if option == 'binning' else (B, 2, Y, X))
    loss = eng.loss_grad(B, meas)
    assert np.isfinite(loss) and loss > 0
    dev = _lib.DeviceBuffer.zeros(eng.ctx, (1 << 22,), np.uint8)
    host_array = np.zeros(1 << 20, dtype=np.uint8)
    refused = [(name, call) for name, call in _calls(eng.lib, eng.h, dev.ptr, host_array.ctypes.data) if name not in CARRIES[option]]
    assert len(refused) == {'binning': 17, 'planes': 18}[option]
    for name, call in refused:
        assert call() == BDOF_ERR_STATE, name
        assert eng.lib.bdof_last_error(eng.h).decode() == name + (BINNING if option == 'binning' else PLANES)
        assert eng.loss_grad(B, meas) == loss, name
