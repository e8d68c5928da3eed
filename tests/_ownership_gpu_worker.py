"""Worker of tests/test_gpu_ownership.py: drives one bdof_ctx through re-configuration, repeated setters and refused calls in a
process of its own (the test gives it a time limit) and prints what it saw as one JSON line; the test asserts.

  reconfigure N_CTX N_ROUNDS   N_CTX contexts one after another; each visits every entry of CONFIGS N_ROUNDS times
  errors                       the refused calls of test_error_return_leaves_the_context_usable, and the same run without them
"""
import gc
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from beyond_dof_amd import _lib, util                    # noqa: E402
from beyond_dof_amd._lib import DeviceBuffer              # noqa: E402
from beyond_dof_amd.engine import MultisliceEngine        # noqa: E402

G, GEN, NORES, RES, RECOMP, A64 = _lib.CFG_GRAD, _lib.CFG_GENERIC, _lib.CFG_NO_RESIDENT, _lib.CFG_ALWAYS_RESIDENT, _lib.CFG_RECOMPUTE, \
    _lib.CFG_ADJOINT64
# one entry per owner of the workspace: (NY, NX, S, Bmax, flags, detector distance, float64 twin, real-space propagator)
CONFIGS = {
    'streaming': (256, 256, 32, 16, G | NORES, None, True, True),
    'resident': (64, 64, 32, 256, G | RES, None, False, False),
    'adjoint64': (192, 200, 48, 16, G | A64, 1e-4, True, False),         # no fused plan for 200: the generic engine (rocFFT)
    'recompute': (128, 512, 32, 32, G | NORES | RECOMP, 'inf', False, False),      # (the real-space sweep keeps a tape of S fields)
}
B = 2           # wavefields of the small loss_grad


def workspace_bytes(name):
    """A lower bound of what bdof_configure allocates for CONFIGS[name]: the gradient rows [Bmax][S] and the tape ([Bmax][S],
    three fields with the tape-free adjoint) of complex64 / float2 fields; the tables and the two work fields come on top."""
    ny, nx, s, bmax, flags = CONFIGS[name][:5]
    field = 8 * bmax * ny * nx
    return field * s + field * (min(s, 3) if flags & RECOMP else s)


def reconfigure(eng, ny, nx, s, bmax, flags):
    """bdof_configure on the engine's OWN context (MultisliceEngine configures once, in its constructor), host side reset to match"""
    eng.ctx.check(eng.lib.bdof_configure(eng.h, ny, nx, s, bmax, flags))
    eng.ny, eng.nx, eng.n_slice, eng.batch_max = ny, nx, s, bmax
    eng.adjoint64, eng.recompute = bool(flags & A64), bool(flags & RECOMP)
    eng._reset_host_state()


def inputs(ny, nx, s, seed):
    rng = np.random.default_rng(seed)
    delta = rng.uniform(0, 2e-5, size=(B, ny, nx, s)).astype(np.float32)
    meas = (1 + 0.05 * rng.normal(size=(B, ny, nx))).astype(np.float32)
    return delta, 0.1 * delta, meas, util.gaussian_probe((ny, nx), ny / 6., ny / 6., 0.5)


def visit(eng, name, data, tables):
    """Configure for CONFIGS[name], call every setter that allocates, run the small loss_grad after each: the losses by name."""
    ny, nx, s, bmax, flags, fp, f64, conv = CONFIGS[name]
    delta, beta, meas, gauss = data
    reconfigure(eng, ny, nx, s, bmax, flags)
    eng.set_physics(5000., 1e-7, fp)                       # bdof_set_physics, bdof_set_transfer_f64, (bdof_set_physics_f64)
    eng.set_rotation_adjoint(tables[0], tables[1], 7)      # bdof_set_rotation_adjoint sizes its row list; the tables are not read here
    eng.set_object_batch(delta, beta)
    out = {}
    eng.set_probe(*gauss)                                  # a localised probe: bdof_set_probe_field
    eng.enable_probe_grad(True)
    out['field'] = eng.loss_grad(B, meas)
    eng.enable_probe_grad(False)
    eng.set_probe(np.ones((ny, nx)), np.zeros((ny, nx)))   # a plane wave: bdof_set_probe, the carrier field goes
    out['plane'] = eng.loss_grad(B, meas)
    if f64:
        eng.enable_tf_f64()                                # bdof_set_tf_f64
        out['tf64'] = eng.loss_grad(B, meas, f64=True)
    if conv:
        eng.set_conv(5000., 1e-7, 17)                      # bdof_set_conv, bdof_set_conv_taps_f64
        out['conv'] = eng.loss_grad(B, meas, conv=True)
        eng.set_probe(*gauss)                              # bdof_set_conv_probe_stack
        out['conv_field'] = eng.loss_grad(B, meas, conv=True)
        if nx == ny:
            eng.enable_conv_f64()                          # bdof_set_conv_f64, bdof_set_conv_f64_detector
            out['conv64'] = eng.loss_grad(B, meas, conv=True, f64=True)
    eng.sync()
    return out


def run_reconfigure(n_ctx, n_rounds):
    meter = _lib.Context(0)                                # never configured: only reads the device's memory in use
    data = {name: inputs(c[0], c[1], c[2], i) for i, (name, c) in enumerate(sorted(CONFIGS.items()))}
    first, mismatches, used = {}, [], []
    for _ in range(n_ctx):
        eng = MultisliceEngine(64, 64, 1, 1, with_grad=False)
        tables = [DeviceBuffer.zeros(eng.ctx, (64,), np.int32) for _ in range(2)]
        for _ in range(n_rounds):
            for name in sorted(CONFIGS):
                losses = visit(eng, name, data[name], tables)
                if first.setdefault(name, losses) != losses:
                    mismatches.append((name, first[name], losses))
        eng._keep = {}
        eng.ctx.close()                                    # bdof_ctx_destroy
        del eng, tables
        gc.collect()
        used.append(meter.mem_used())
    print(json.dumps({'first': first, 'mismatches': mismatches, 'used': used,
                      'workspace': {name: workspace_bytes(name) for name in CONFIGS}}))


def run_errors():
    """The same sequence of valid calls on two fresh contexts; the second one has a refused call in front of each of them."""
    ny = nx = 128
    s, bmax, fp = 8, B, 1e-4                               # a near-field detector
    delta, beta, meas, gauss = inputs(ny, nx, s, 11)
    junk = np.zeros((s + 1, nx, ny), dtype=np.complex128)   # a host array large enough for any argument that is refused unread
    res = {}
    for inject in (False, True):
        eng = MultisliceEngine(ny, nx, s, bmax, with_grad=True, engine='streaming')
        lib, h, codes, losses = eng.lib, eng.h, {}, {}
        if inject:
            codes['configure_zero_size'] = lib.bdof_configure(h, 0, nx, s, bmax, G | NORES)
        eng.set_physics(5000., 1e-7, fp)
        eng.set_object_batch(delta, beta)
        if inject:
            codes['probe_stack_one_array'] = lib.bdof_set_probe_stack(h, junk.ctypes.data, None)
        eng.set_probe(*gauss)
        losses['field'] = eng.loss_grad(B, meas)
        if inject:
            codes['conv_probe_stack_without_conv'] = lib.bdof_set_conv_probe_stack(h, junk.ctypes.data, junk.ctypes.data, 1., 0., 1., 0.)
            losses['field_again'] = eng.loss_grad(B, meas)
        eng.set_conv(5000., 1e-7, 17)
        losses['conv'] = eng.loss_grad(B, meas, conv=True)
        if inject:
            codes['conv_f64_even_kernel'] = lib.bdof_set_conv_f64(h, junk.ctypes.data, junk.ctypes.data, 16, 1., 0., 1.)
        eng.enable_conv_f64()
        if inject:
            eng.ctx.check(lib.bdof_set_conv_f64_detector(h, None))      # a valid call: the detector step's table goes
            m = eng._meas_to_device(meas)
            codes['conv_f64_near_without_detector'] = lib.bdof_loss_grad_conv_f64(h, B, None, None, None, m.ptr, 0.0)
            eng.enable_conv_f64()
        losses['conv64'] = eng.loss_grad(B, meas, conv=True, f64=True)
        eng.sync()
        res['injected' if inject else 'fresh'] = {'codes': codes, 'losses': losses}
        eng.ctx.close()
    print(json.dumps(res))


if __name__ == '__main__':
    if sys.argv[1] == 'reconfigure':
        run_reconfigure(int(sys.argv[2]), int(sys.argv[3]))
    else:
        run_errors()
