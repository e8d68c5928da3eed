"""Detector planes at the cfg2 shape (256^3 volume, 50 of 50 angles per Adam step, 5 keV, 1 nm voxels, plane probe): ms per
FullfieldSolver.step with free_prop_cm a scalar, a sequence of one (the scalar's code path: the comparison shows the spread
between two runs of the same code) and sequences of 2 and 4 distances, the settings built once in one process and timed in
alternation (round-robin blocks, so drift of the device hits all alike).  Each block is timed with the library's stream-ordered
events (bdof_timer_mark / bdof_timer_elapsed, slots 2 / 3) around its steps.  Beside the measured cost of the planes the byte model of
DESIGN §3: the stage between the exit wave and the adjoint seed moves 36 D + 16 B per pixel per wavefield with D > 1 planes
(fan-out 8 (1 + D), loss 20 D, fan-in 8 (D + 1)), 52 B with one, against 104 S B for the sweep.  Prints one JSON line;
--profile adds the split per kernel class of one profiled step per setting (bdof_profile_enable), taken after the timing.

usage: python tools/bench_multidistance.py [--size 256] [--angles 50] [--n-theta 50] [--steps 24] [--warmup 3] [--block 4] [--profile]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

entry.build()
from beyond_dof_amd import _lib, util  # noqa: E402
from beyond_dof_amd.solver import FullfieldSolver  # noqa: E402

DISTANCES = (5e-5, 1e-4, 2e-4, 4e-4)
SETTINGS = [('scalar', 1e-4), ('D1', [1e-4]), ('D2', [5e-5, 1e-4]), ('D4', list(DISTANCES))]


def stage_bytes(D):
    """B per pixel per wavefield of the stage between the exit wave and the adjoint seed."""
    return 36.0 * D + 16.0 if D > 1 else 16.0 + 20.0 + 16.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--angles', type=int, default=50)
    ap.add_argument('--n-theta', type=int, default=50)
    ap.add_argument('--steps', type=int, default=24, help='timed steps per setting (>= 20 for a figure to record)')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--block', type=int, default=4, help='consecutive steps of one setting before the next takes its turn')
    ap.add_argument('--profile', action='store_true')
    args = ap.parse_args()
    n, mb, n_theta = args.size, args.angles, args.n_theta
    rng = np.random.default_rng(3)
    t0 = time.time()
    coords = util.rotation_lookup([n, n, n], n_theta)
    batches = [np.sort(rng.choice(n_theta, mb, replace=False)) for _ in range(4)]
    true_d = rng.random((n, n, n), dtype=np.float32) * np.float32(2e-6)
    init_d = np.clip(rng.normal(8.7e-7, 1e-7, size=(n, n, n)), 0, None).astype(np.float32)
    hyper = dict(learning_rate=1e-7, alpha_d=1.5e-8, alpha_b=1.5e-9, gamma=1e-11)
    solvers, planes = {}, {}
    for name, fp in SETTINGS:
        s = FullfieldSolver(n, n, n, n_theta, mb, 5000., 1e-7, free_prop_cm=fp, coord_ls=coords)
        s.set_volume(true_d, 0.1 * true_d)
        s.set_measurements(np.abs(s.forward_angles(np.arange(n_theta))).astype(np.float32))      # each setting fits its own data
        s.set_volume(init_d, 0.1 * init_d)
        s.set_mask(np.ones((n, n, n), dtype=np.float32))
        s.tune_tail()
        solvers[name], planes[name] = s, s.n_planes
    print('[bench_multidistance] setup %.1f s' % (time.time() - t0), file=sys.stderr, flush=True)

    def run(name, i):
        solvers[name].step(i % len(batches), batches[i % len(batches)], want_loss=False, **hyper)

    def timed(name, first, k):
        s = solvers[name]
        lib, h = s.ctx.lib, s.ctx.handle
        s.ctx.sync()
        s.ctx.check(lib.bdof_timer_mark(h, 2))
        for i in range(k):
            run(name, first + i)
        s.ctx.check(lib.bdof_timer_mark(h, 3))
        s.ctx.sync()
        ms = ctypes.c_double(0)
        s.ctx.check(lib.bdof_timer_elapsed(h, 2, 3, ctypes.byref(ms)))
        return ms.value

    names = [name for name, _ in SETTINGS]
    for name in names:
        for i in range(args.warmup):
            run(name, i)
        solvers[name].ctx.sync()
    blocks = {name: [] for name in names}
    done = 0
    while done < args.steps:
        k = min(args.block, args.steps - done)
        for name in names:
            blocks[name].append(timed(name, args.warmup + done, k) / k)
        done += k
    ms = {name: float(np.mean(blocks[name])) for name in names}
    S = n
    out = {'metric': 'ms per Adam step by detector planes', 'size': n, 'angles_per_step': mb, 'n_theta': n_theta, 'steps': args.steps,
           'ms_per_step': {name: round(ms[name], 3) for name in names},
           'ms_per_step_block_min_max': {name: [round(min(blocks[name]), 3), round(max(blocks[name]), 3)] for name in names},
           'D1_over_scalar': round(ms['D1'] / ms['scalar'], 4),
           'measured_ratio_to_scalar': {name: round(ms[name] / ms['scalar'], 4) for name in names},
           'byte_model_stage_B_per_px': {name: stage_bytes(planes[name]) for name in names},
           'byte_model_ratio_to_scalar': {name: round((104.0 * S + stage_bytes(planes[name])) / (104.0 * S + stage_bytes(1)), 4) for name in names}}
    if args.profile:
        prof = {}
        for name in names:
            s = solvers[name]
            lib, h = s.ctx.lib, s.ctx.handle
            s.ctx.check(lib.bdof_profile_enable(h, 1))
            run(name, 0)
            s.ctx.sync()
            row = {}
            for cls, cname in enumerate(_lib.KERNEL_CLASS_NAMES):
                cnt, tot = ctypes.c_int(0), ctypes.c_double(0)
                s.ctx.check(lib.bdof_profile_read(h, cls, ctypes.byref(cnt), ctypes.byref(tot)))
                row[cname] = [cnt.value, round(tot.value, 3)]
            s.ctx.check(lib.bdof_profile_enable(h, 0))
            prof[name] = row
        out['profiled_step_launches_ms_by_class'] = prof
    print(json.dumps(out))


if __name__ == '__main__':
    main()
