"""The materialised rotations at the cfg2 shape (256^3 volume, 50 of 50 angles per Adam step, 5 keV, 1 nm voxels,
free_prop_cm = 1e-4, plane probe): ms of the forward binding (bdof_set_object_bilinear / bdof_set_object_rigid), of the adjoint
(bdof_rotate_bilinear_adjoint / bdof_rotate_rigid_adjoint) and of the whole FullfieldSolver.step, for
    bilinear       rotation='bilinear' (the yardstick, same run)
    trilinear0     rotation='trilinear' at zero tilt (the same geometry as bilinear)
    trilinear30    rotation='trilinear' with the axis tilted 30 degrees towards the beam.
--geometry: trilinear30 against trilinear30_refined, the same step with refine_geometry on all five names (per step: the
parameter-gradient kernels, the download of B * 12 doubles, which waits for the stream, the chain rule and Adam on the host); both
also time the kernels alone (param_grad_kernel_ms: launches only, one wait at the end) and with the download (param_grad_host_ms).
Every mode runs in a child process of its own under `timeout`, one after another; the first one that fails ends the script with
its status.  Prints one JSON line.

usage: python tools/bench_rigid.py [--geometry] [--size 256] [--angles 50] [--steps 10] [--warmup 2] [--limit 240]
       python tools/bench_rigid.py --mode trilinear30 ...      (one mode, in this process)"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = {'bilinear': dict(rotation='bilinear'), 'trilinear0': dict(rotation='trilinear'),
         'trilinear30': dict(rotation='trilinear', axis_tilt=np.pi / 6),
         'trilinear30_refined': dict(rotation='trilinear', axis_tilt=np.pi / 6, refine_geometry=('center', 'axis_tilt', 'axis_roll', 'theta', 'shifts'))}


def one_mode(mode, n, mb, steps, warmup):
    import __graft_entry__ as entry
    entry.build()
    from beyond_dof_amd.solver import FullfieldSolver
    rng = np.random.default_rng(3)
    theta = -np.linspace(0, 2 * np.pi, mb).astype(np.float32)
    idx = np.arange(mb)
    true_d = np.zeros((n, n, n), dtype=np.float32)
    m = n // 8
    true_d[:, m:-m, m:-m] = rng.random((n, n - 2 * m, n - 2 * m), dtype=np.float32) * np.float32(2e-6)
    s = FullfieldSolver(n, n, n, mb, mb, 5000., 1e-7, free_prop_cm=1e-4, theta=theta, **MODES[mode])
    s.set_volume(true_d, 0.1 * true_d)
    s.set_measurements(np.abs(s.forward_angles(idx)).astype(np.float32))
    s.set_volume(0.9 * true_d, 0.09 * true_d)
    s.set_mask(np.ones((n, n, n), dtype=np.float32))
    hyper = dict(learning_rate=1e-8, alpha_d=1.5e-8, alpha_b=1.5e-9, gamma=1e-11)

    def timed(call, reps):
        s.ctx.sync()
        t0 = time.perf_counter()
        for i in range(reps):
            call(i)
        s.ctx.sync()
        return 1e3 * (time.perf_counter() - t0) / reps

    for i in range(warmup):
        s.step(i, idx, **hyper)
    out = {'step_ms': timed(lambda i: s.step(warmup + i, idx, **hyper), steps)}
    out['bind_ms'] = timed(lambda i: s.rot.stage(s.eng, s.x[s.cur], idx, mb, s.conv), steps)
    s._rot_loss_grad(idx)                       # a rotated-frame gradient for the adjoint to take back
    out['adjoint_ms'] = timed(lambda i: s._produce()(0, n), steps)
    if MODES[mode]['rotation'] == 'trilinear':
        from beyond_dof_amd._lib import DeviceBuffer
        dprm = DeviceBuffer.zeros(s.ctx, (mb, 12), np.float64)
        launch = lambda i: s.ctx.check(s.ctx.lib.bdof_rotate_rigid_param_grad(s.ctx.handle, s.x[s.cur].ptr, None, n, n, n, s.rot.prm_buf.ptr, mb, dprm.ptr, 0))
        launch(0)
        out['param_grad_kernel_ms'] = timed(launch, steps)
        out['param_grad_host_ms'] = timed(lambda i: s.rot.param_gradient(s.x[s.cur]), steps)
    return {k: round(v, 3) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--angles', type=int, default=50)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--limit', type=int, default=240, help='seconds a mode may take')
    ap.add_argument('--mode', choices=sorted(MODES))
    ap.add_argument('--geometry', action='store_true', help='the trilinear30 step without and with refine_geometry')
    args = ap.parse_args()
    if args.mode:
        print(json.dumps(one_mode(args.mode, args.size, args.angles, args.steps, args.warmup)))
        return 0
    res = {}
    for mode in (('trilinear30', 'trilinear30_refined') if args.geometry else ('bilinear', 'trilinear0', 'trilinear30')):
        cmd = ['timeout', '-k', '10', str(args.limit), sys.executable, os.path.abspath(__file__), '--mode', mode, '--size', str(args.size),
               '--angles', str(args.angles), '--steps', str(args.steps), '--warmup', str(args.warmup)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE)
        if r.returncode != 0:
            print('[bench_rigid] {} ended with status {}: stopping'.format(mode, r.returncode), file=sys.stderr)
            return r.returncode
        res[mode] = json.loads(r.stdout.decode().strip().splitlines()[-1])
    for mode, v in res.items():
        v['rest_of_step_ms'] = round(v['step_ms'] - v['adjoint_ms'], 3)
    print(json.dumps({'metric': 'ms per call at {0}^3, {1} angles per step'.format(args.size, args.angles), 'steps': args.steps, **res}))
    return 0


if __name__ == '__main__':
    sys.exit(main())
