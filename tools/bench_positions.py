"""Sub-pixel probe positions at the cfg5 shape (256^3 object, 72^2 gaussian probe, 20 x 20 scan positions, far field, all positions
of one angle per Adam step — tools/bench_ptycho.py): ms of the whole PtychoSolver.step for
    plain          neither keyword: the windows by index math (the yardstick, same run)
    offsets        position_offsets: the window stack path alone (bdof_window_stack, the modulation table of the stack,
                   bdof_window_stack_adjoint)
    refined        refine_positions='per_angle': the same with bdof_window_position_grad, the download of B * 2 doubles (which waits
                   for the stream) and the host Adam
and, in the modes that run them, of the three new calls by themselves (launches only, one wait at the end): stack_ms, adjoint_ms,
position_grad_ms.  Every mode runs in a child process of its own under `timeout`, one after another; the first one that fails
ends the script with its status.  Prints one JSON line.  No time is a pass condition.

usage: python tools/bench_positions.py [--probe 72] [--side 20] [--steps 5] [--warmup 2] [--limit 240]
       python tools/bench_positions.py --mode offsets ...      (one mode, in this process)"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = ('plain', 'offsets', 'refined')


def one_mode(mode, ps, side, steps, warmup):
    import __graft_entry__ as entry
    entry.build()
    from beyond_dof_amd import util
    from beyond_dof_amd.solver import PtychoSolver
    n, n_theta = 256, 8
    rng = np.random.default_rng(5)
    pos = np.array([(y, x) for y in np.arange(side) * 12 + 14 for x in np.arange(side) * 12 + 14])
    mb = len(pos)
    pr, pi = util.gaussian_probe((ps, ps), 6., 6., 0.5)
    kw = {'plain': {}, 'offsets': dict(position_offsets=rng.uniform(-0.9, 0.9, size=(mb, 2))),
          'refined': dict(position_offsets=rng.uniform(-0.9, 0.9, size=(mb, 2)), refine_positions='per_angle')}[mode]
    s = PtychoSolver([n, n, n], [ps, ps], pos, n_theta, mb, 5000., 1e-7, pr, pi, coord_ls=util.rotation_lookup([n, n, n], n_theta), **kw)
    d = rng.random((n, n, n), dtype=np.float32) * 1e-6
    s.set_volume(d, 0.1 * d)
    s.set_measurements(np.abs(rng.normal(1.0, 0.1, size=(n_theta, mb, ps, ps))).astype(np.float32) * ps)
    idx = np.arange(mb)

    def timed(call, reps):
        s.ctx.sync()
        t0 = time.perf_counter()
        for i in range(reps):
            call(i)
        s.ctx.sync()
        return 1e3 * (time.perf_counter() - t0) / reps

    s.reset_moments()
    for i in range(warmup):
        s.step(i, i % n_theta, idx, None, 1e-7)
    out = {'step_ms': timed(lambda i: s.step(warmup + i, (warmup + i) % n_theta, idx, None, 1e-7), steps)}
    if mode != 'plain':
        lib, h = s.ctx.lib, s.ctx.handle
        s.loss_and_grad(0, idx)                   # origins, a stack and a window-frame gradient for the calls to take
        vol, tab = s._source
        out['stack_ms'] = timed(lambda i: s.ctx.check(lib.bdof_window_stack(h, vol, n, n, tab, s.origin_buf.ptr, mb, s.stack.ptr)), steps)
        out['adjoint_ms'] = timed(lambda i: s.ctx.check(lib.bdof_window_stack_adjoint(h, None, 0, s.origin_buf.ptr, mb, s.g.ptr, 0, 1.0)), steps)
        out['position_grad_ms'] = timed(lambda i: s.ctx.check(lib.bdof_window_position_grad(h, vol, n, n, tab, None, s.origin_buf.ptr, mb,
                                                                                          s.dpos_buf.ptr, 0)), steps)
        out['stack_gb'] = round(mb * n * ps * ps * 8 / 1e9, 3)
    return {k: round(v, 3) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--probe', type=int, default=72)
    ap.add_argument('--side', type=int, default=20)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--limit', type=int, default=240, help='seconds a mode may take')
    ap.add_argument('--mode', choices=MODES)
    args = ap.parse_args()
    if args.mode:
        print(json.dumps(one_mode(args.mode, args.probe, args.side, args.steps, args.warmup)))
        return 0
    res = {}
    for mode in MODES:
        cmd = ['timeout', '-k', '10', str(args.limit), sys.executable, os.path.abspath(__file__), '--mode', mode, '--probe', str(args.probe),
               '--side', str(args.side), '--steps', str(args.steps), '--warmup', str(args.warmup)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE)
        if r.returncode != 0:
            print('[bench_positions] {} ended with status {}: stopping'.format(mode, r.returncode), file=sys.stderr)
            return r.returncode
        res[mode] = json.loads(r.stdout.decode().strip().splitlines()[-1])
    print(json.dumps({'metric': 'ms per call at 256^3, {0}^2 probe, {1} positions per step'.format(args.probe, args.side ** 2), 'steps': args.steps, **res}))
    return 0


if __name__ == '__main__':
    sys.exit(main())
