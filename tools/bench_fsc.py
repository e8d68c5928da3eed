"""Time of one Fourier shell correlation of two resident volumes (bdof_shell_correlation through resolution.shell_sums, every shell
up to the corner) at n^3, beside numpy float64 on the host doing the same hard shells (tests/fsc_reference.py: two real
transforms per volume, one bincount per sum).  Per size: first_ms — the first call, which creates the rocFFT plan and takes the
complex128 workspace; call_ms — the mean of the following calls, two transforms and one pass over the spectra each, the sums
copied back; host_s — the numpy restatement, once; worst_curve_diff — the largest difference of the two curves between them.
Recorded, not asserted.  Prints one JSON line.

usage: python tools/bench_fsc.py [--sizes 256,512] [--reps 5] [--no-host]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def one_size(n, reps, host):
    from beyond_dof_amd import _lib, resolution
    from beyond_dof_amd._lib import DeviceBuffer
    ctx = _lib.Context(0)
    rng = np.random.default_rng(n)
    rows = []
    for _ in range(2):
        r = rng.standard_normal((n, n, n, 2), dtype=np.float32)
        r *= np.array([1e-6, 1e-7], dtype=np.float32)
        rows.append(r)
    rows[1] += rows[0]                                               # b = a + noise
    bufs = [DeviceBuffer.from_host(ctx, r) for r in rows]

    def call():
        ctx.sync()
        t0 = time.perf_counter()
        sums = resolution.shell_sums(bufs[0], bufs[1], ctx=ctx)
        return 1e3 * (time.perf_counter() - t0), sums

    first_ms, sums = call()
    times = [call()[0] for _ in range(reps)]
    out = {'first_ms': round(first_ms, 2), 'call_ms': round(float(np.mean(times)), 2), 'call_ms_min': round(min(times), 2), 'shells': len(sums)}
    print('[bench_fsc] {}^3 device: {}'.format(n, out), file=sys.stderr, flush=True)
    if host:
        import fsc_reference as fr
        pairs = [(r[..., 0].astype(np.float64), r[..., 1].astype(np.float64)) for r in rows]
        t0 = time.perf_counter()
        ref = fr.shell_sums(pairs[0], pairs[1], len(sums))
        out['host_s'] = round(time.perf_counter() - t0, 2)
        out['worst_curve_diff'] = float(max(np.abs(c - r).max() for c, r in zip(resolution.curves(sums), fr.curves(ref))))
        out['n_points_equal'] = bool(np.array_equal(sums[:, 0], ref[:, 0]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='256,512')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no-host', action='store_true', help='skip the numpy restatement (minutes and tens of GB at 512^3)')
    args = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    res = {}
    for n in (int(v) for v in args.sizes.split(',')):
        res[str(n)] = one_size(n, args.reps, not args.no_host)
        print('[bench_fsc] {}^3: {}'.format(n, res[str(n)]), file=sys.stderr, flush=True)
    print(json.dumps({'metric': 'Fourier shell correlation of two n^3 volumes, all shells', 'reps': args.reps, **res}))
    return 0


if __name__ == '__main__':
    sys.exit(main())
