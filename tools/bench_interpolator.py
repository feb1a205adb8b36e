#!/usr/bin/env python
"""Time the device-resident Interpolator on the 4 M-particle cube of bench.py (GPU only; fails without a device).

    python tools/bench_interpolator.py --out OUTDIR [--n1 159] [--window 0.3]

For 125 000 grid points and for as many points as particles: `update()`, and `interpolate_many` with 1, W and 2 W
properties for 'shepard' and 'order1' (results left on the device: pull=False), each as the mean over a
device-synchronised window of at least `--window` seconds after a warm-up.  For comparison, in the same run over the
same arrays and grid: SummationDensity(dest='interpolate', sources=['fluid']) -- the same neighbour sweep with one
accumulator -- through the AccelerationEval that SPHEvaluator wraps, with device-resident state (sync='manual').
Writes OUTDIR/bench_interpolator.json and prints it.

(SPHEvaluator itself keeps the host arrays authoritative -- it pushes the inputs and pulls the outputs of 4 M particles
around every evaluate -- so its compiled evaluator is used with the state left on the device: the same kernel launches.)

Kernel statistics of the pair launches come from a separate run under the kernel-trace profiler, counters off:

    rocprofv3 --kernel-trace --stats -d OUTDIR/prof -o interp -- python tools/bench_interpolator.py --window 0.05 --out OUTDIR/prof
"""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def timed(ctx, fn, window, warmup=2):
    for _ in range(warmup):
        fn()
    ctx.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        if n % 2 == 0 or n == 1:
            ctx.synchronize()
            if time.perf_counter() - t0 >= window:
                break
    ctx.synchronize()
    return dict(ms=1e3 * (time.perf_counter() - t0) / n, reps=n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n1', type=int, default=159, help='lattice side of the cube (bench.py: 159 -> 4.02 M particles)')
    ap.add_argument('--window', type=float, default=0.3)
    ap.add_argument('--out', default='.')
    args = ap.parse_args()
    import bench
    from pysph_amd import device as dev
    from pysph_amd.acceleration_eval import AccelerationEval, SPHCompiler
    from pysph_amd.equations import Group, SummationDensity
    from pysph_amd.interpolator import WIDTH
    from pysph_amd.kernels import WendlandQuintic
    from pysph_amd.tools import Interpolator
    ctx = dev.HipContext(0)         # raises without a GPU
    pa, dx = bench.make_cube(args.n1)
    n = pa.get_number_of_particles()
    pa.p[:] = pa.rho - 1000.0
    dev.attach(pa, ctx).push('x', 'y', 'z', 'h', 'm', 'rho', 'u', 'v', 'w', 'p', 'au', 'av', 'aw', 'cs')
    kernel = WendlandQuintic(dim=3)
    fields = ['p', 'u', 'v', 'w', 'rho', 'au', 'av', 'aw']
    assert len(fields) >= 2 * WIDTH
    result = dict(particles=n, width=WIDTH, kernel='WendlandQuintic', window_s=args.window, cases=[])
    for label in ('grid125000', 'points=particles'):
        for method in ('shepard', 'order1'):
            kw = dict(num_points=125000) if label == 'grid125000' else dict(x=pa.x.copy(), y=pa.y.copy(), z=pa.z.copy())
            interp = Interpolator([pa], kernel=kernel, method=method, ctx=ctx, sync=False, **kw)
            interp.invalidate = False       # nothing else evaluates on this context between the calls
            row = dict(points=label, npoints=int(interp.pa.get_number_of_particles()), method=method)
            row['update'] = timed(ctx, interp.update, args.window)
            for k in (1, WIDTH, 2 * WIDTH):
                row['interpolate_many_%d' % k] = timed(ctx, lambda: interp.interpolate_many(fields[:k], pull=False), args.window)
            if method == 'order1':
                def first_call():
                    interp.update()
                    interp.interpolate_many(fields[:1], pull=False)
                row['update+first_call_1'] = timed(ctx, first_call, args.window)
            if method == 'shepard':
                a_eval = AccelerationEval([pa, interp.pa], [Group(equations=[SummationDensity(dest='interpolate', sources=['fluid'])])], kernel)
                SPHCompiler(a_eval, ctx=ctx, sync='manual').compile()
                a_eval.set_nnps(interp.nnps)
                row['summation_density'] = timed(ctx, lambda: a_eval.compute(0.0, 0.1), args.window)
                del a_eval
            result['cases'].append(row)
            print(json.dumps(row), flush=True)
            del interp
            gc.collect()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, 'bench_interpolator.json'), 'w') as f:
        json.dump(result, f, indent=1)
    ctx.close()


if __name__ == '__main__':
    main()
