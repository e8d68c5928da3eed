"""Probe modes at the cfg5 shape (256^3 object, 72^2 gaussian probe, 20 x 20 scan positions, 256 slices, far field, all positions of
one angle per Adam step — tools/bench_ptycho.py, tools/bench_positions.py): ms of the whole PtychoSolver.step for
    plain          one (py, px) probe: the single-probe path (the yardstick, same run)
    modes1 .. 3    (M, py, px) probes, M = 1, 2, 3: the modes path — per mode one forward and one seeded launch of the resident
                   kernel, the coupling kernel between them and, for M > 1, the sum of the per-mode gradient rows
and, in the modes runs, of the coupling kernel alone — couple_ms: bdof_forward with an output buffer (forward launches + the
coupling kernel writing M B detector waves) minus bdof_forward without one (forward_ms: the forward launches alone); launches
only, one wait at the end — and the tape's size (tape_gb).
--parent-tree DIR: a built checkout of the parent commit; its own `tools/bench_positions.py --mode plain` — the same workload on
the single-probe path — is run from there as parent_plain, in the same job.
Every mode runs in a child process of its own under `timeout`, one after another; the first one that fails ends the script with
its status.  Prints one JSON line.  No time is a pass condition: the expectation to read the numbers against is
t(M) = M t(1) + small (the resident engine is bound per wavefield) and t(modes1) = t(plain) + two launches.

usage: python tools/bench_modes.py [--probe 72] [--side 20] [--steps 5] [--warmup 2] [--limit 240] [--parent-tree DIR]
       python tools/bench_modes.py --mode modes2 ...      (one mode, in this process)"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = ('plain', 'modes1', 'modes2', 'modes3')


def one_mode(mode, ps, side, steps, warmup):
    import __graft_entry__ as entry
    entry.build()
    from beyond_dof_amd import modes, util
    from beyond_dof_amd._lib import DeviceBuffer
    from beyond_dof_amd.solver import PtychoSolver
    n, n_theta = 256, 8
    rng = np.random.default_rng(5)
    pos = np.array([(y, x) for y in np.arange(side) * 12 + 14 for x in np.arange(side) * 12 + 14])
    mb = len(pos)
    pr, pi = util.gaussian_probe((ps, ps), 6., 6., 0.5)
    M = 0 if mode == 'plain' else int(mode[-1])
    if M:
        p = modes.initial_modes(pr + 1j * pi, M, 0.1)
        pr, pi = p.real, p.imag
    s = PtychoSolver([n, n, n], [ps, ps], pos, n_theta, mb, 5000., 1e-7, pr, pi, coord_ls=util.rotation_lookup([n, n, n], n_theta))
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
    out = {'step_ms': timed(lambda i: s.step(warmup + i, (warmup + i) % n_theta, idx, None, 1e-7), steps),
           'tape_gb': round(max(M, 1) * mb * n * ps * ps * 8 / 1e9, 3)}
    if M:
        lib, h = s.ctx.lib, s.ctx.handle
        a, xo, yo = s._stage(0, idx, None)
        s.rot.stage(s.eng, s.x[s.cur], [0], 1, False)
        waves = DeviceBuffer(s.ctx, M * mb * ps * ps * 8, np.complex64, (M * mb, ps, ps))
        with_waves = timed(lambda i: s.ctx.check(lib.bdof_forward(h, mb, a, xo, yo, waves.ptr, 0)), steps)
        without = timed(lambda i: s.ctx.check(lib.bdof_forward(h, mb, a, xo, yo, None, 0)), steps)
        out.update(forward_ms=without, couple_ms=with_waves - without)
    return {k: round(v, 3) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--probe', type=int, default=72)
    ap.add_argument('--side', type=int, default=20)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--limit', type=int, default=240, help='seconds a mode may take')
    ap.add_argument('--mode', choices=MODES)
    ap.add_argument('--parent-tree', help='a built checkout of the parent commit: its bench_positions.py --mode plain runs as parent_plain')
    args = ap.parse_args()
    if args.mode:
        print(json.dumps(one_mode(args.mode, args.probe, args.side, args.steps, args.warmup)))
        return 0
    shape = ['--probe', str(args.probe), '--side', str(args.side), '--steps', str(args.steps), '--warmup', str(args.warmup)]
    runs = [(mode, [os.path.abspath(__file__), '--mode', mode], ROOT) for mode in MODES]
    if args.parent_tree:
        tree = os.path.abspath(args.parent_tree)
        runs.insert(0, ('parent_plain', [os.path.join(tree, 'tools', 'bench_positions.py'), '--mode', 'plain'], tree))
    res = {}
    for name, script, cwd in runs:
        r = subprocess.run(['timeout', '-k', '10', str(args.limit), sys.executable] + script + shape, stdout=subprocess.PIPE, cwd=cwd)
        if r.returncode != 0:
            print('[bench_modes] {} ended with status {}: stopping'.format(name, r.returncode), file=sys.stderr)
            return r.returncode
        res[name] = json.loads(r.stdout.decode().strip().splitlines()[-1])
    print(json.dumps({'metric': 'ms per call at 256^3, {0}^2 probe, {1} positions per step'.format(args.probe, args.side ** 2), 'steps': args.steps, **res}))
    return 0


if __name__ == '__main__':
    sys.exit(main())
