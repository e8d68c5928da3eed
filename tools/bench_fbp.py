"""Time of the analytic start (FullfieldSolver.analytic_volume: bdof_ctf_retrieve + bdof_backproject per batch of angles) at n^3
with n_theta angles, beside one epoch of Adam steps of the same solver from the same job.  Per case: retrieve_ms — contrast,
transforms and ramp of all angles (stream-ordered stamps around the calls); backproject_ms — the back-projection of all angles;
analytic_s — the whole call from the host, uploads of the amplitudes included; first_s — the first call, which creates the rocFFT
plans and takes the complex128 work area; epoch_s — n_theta / minibatch steps.  Recorded, not asserted.  Prints one JSON line.

usage: python tools/bench_fbp.py [--cases 256:50,512:200] [--minibatch 10] [--rotation nearest]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one_case(n, n_theta, mb, rotation):
    from beyond_dof_amd import analytic
    from beyond_dof_amd._lib import DeviceBuffer
    from beyond_dof_amd.solver import FullfieldSolver
    rng = np.random.default_rng(n)
    theta = -np.linspace(0, 2 * np.pi, n_theta)
    s = FullfieldSolver(n, n, n, n_theta, mb, 5000., 1e-7, free_prop_cm=1e-3, rotation=rotation, theta=theta)
    prj = (1 + 0.01 * rng.standard_normal((n_theta, n, n), dtype=np.float32))
    s.set_measurements(prj)
    out = {}
    for key in ('first_s', 'analytic_s'):
        s.ctx.sync()
        t0 = time.perf_counter()
        s.analytic_volume(prj)
        out[key] = round(time.perf_counter() - t0, 3)
    # the two device stages alone, on resident inputs: all angles in batches of the minibatch size
    lib, h, ctx = s.ctx.lib, s.ctx.handle, s.ctx
    rows, angles = s.analytic_rows()
    filters = DeviceBuffer.from_host(ctx, analytic.ctf_filters(n, n, 5000., 1e-7, 1e-3, n))
    meas = DeviceBuffer.from_host(ctx, np.ascontiguousarray(prj[:mb]))
    q = DeviceBuffer(ctx, mb * n * n * 4, np.float32)
    prm = DeviceBuffer.from_host(ctx, np.ascontiguousarray(rows[:mb]))
    w = DeviceBuffer.from_host(ctx, analytic.angle_weights(angles)[:mb].astype(np.float32))
    vol = DeviceBuffer.zeros(ctx, (n, n, n, 2), np.float32)
    batches = n_theta // mb

    def timed(call):
        ms = ctypes.c_double(0)
        ctx.check(lib.bdof_timer_mark(h, 2))
        for i in range(batches):
            call(i)
        ctx.check(lib.bdof_timer_mark(h, 3))
        ctx.sync()
        ctx.check(lib.bdof_timer_elapsed(h, 2, 3, ctypes.byref(ms)))
        return round(ms.value, 2)

    out['retrieve_ms'] = timed(lambda i: ctx.check(lib.bdof_ctf_retrieve(h, meas.ptr, None, 1.0, filters.ptr, mb, 1, n, n, q.ptr)))
    out['backproject_ms'] = timed(lambda i: ctx.check(lib.bdof_backproject(h, q.ptr, n, n, prm.ptr, w.ptr, mb, vol.ptr, n, n, n, 0, n * n, int(i > 0), 10., 1.)))
    s.reset_moments()
    idx = np.arange(n_theta)
    s.step(0, idx[:mb], 1e-8)                    # first step: set-up
    s.ctx.sync()
    t0 = time.perf_counter()
    for i in range(batches):
        s.step(i, idx[i * mb:(i + 1) * mb], 1e-8)
    s.ctx.sync()
    out['epoch_s'] = round(time.perf_counter() - t0, 3)
    out['steps_per_epoch'] = batches
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='256:50,512:200', help='n:n_theta, separated by commas')
    ap.add_argument('--minibatch', type=int, default=10)
    ap.add_argument('--rotation', default='nearest')
    args = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    res = {}
    for case in args.cases.split(','):
        n, n_theta = (int(v) for v in case.split(':'))
        res[case] = one_case(n, n_theta, args.minibatch, args.rotation)
        print('[bench_fbp] {}^3, {} angles: {}'.format(n, n_theta, res[case]), file=sys.stderr, flush=True)
    print(json.dumps({'metric': 'analytic start (CTF retrieval + filtered back-projection) beside one epoch', 'minibatch': args.minibatch,
                      'rotation': args.rotation, **res}))
    return 0


if __name__ == '__main__':
    sys.exit(main())
