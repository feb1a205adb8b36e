"""What one evaluation of WCSPHScheme(delta_sph=True, nu > 0) costs next to the plain set.

A jittered cube of n1^3 particles (default 100: 1 M), one fluid array, WendlandQuintic, device-resident
(sync='manual'); per equation set

  eval_ms   device events around windows of `--batch` evaluations issued back to back, per-evaluation time =
            interval / batch, median over `--reps` windows after `--warmup` evaluations (the timers off);
  split     the same evaluations once more with the library's timers on (sph_timer_get: event pairs around every
            launch group, which cost a few per cent): ms per evaluation of the EOS launch, the record packing and the
            pair launches per family -- "pair_delta_sph_pre" is the moment pass plus the gradient pass,
            "pair_wcsph_options" the rates sweep with the extra terms, "pair_wcsph" the plain rates sweep.

    python tools/wcsph_options_time.py [--n1 100 --reps 7 --batch 50 --warmup 60] [--out profiles/wcsph_options_time.json]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

KEYS = ('eos', 'pack', 'pair_wcsph', 'pair_wcsph_options', 'pair_delta_sph_pre')


def make_cube(n1, seed=11):
    from pysph_amd.particle_array import get_particle_array_wcsph
    rng = np.random.default_rng(seed)
    dx = 1.0 / n1
    g = (np.arange(n1) + 0.5) * dx
    x, y, z = [a.ravel() for a in np.meshgrid(g, g, g, indexing='ij')]
    n = x.size
    pa = get_particle_array_wcsph(
        name='fluid', x=x + 0.1 * dx * rng.uniform(-1, 1, n), y=y + 0.1 * dx * rng.uniform(-1, 1, n),
        z=z + 0.1 * dx * rng.uniform(-1, 1, n), u=rng.uniform(-1, 1, n), v=rng.uniform(-1, 1, n),
        w=rng.uniform(-1, 1, n), h=1.3 * dx * np.ones(n), m=1000.0 * dx ** 3 * np.ones(n),
        rho=1000.0 * (1 + 0.02 * rng.uniform(-1, 1, n)))
    return pa, dx


def measure(options, args, torch, stream):
    from pysph_amd import device as dev
    from pysph_amd import kernels as K
    from pysph_amd.acceleration_eval import AccelerationEval, SPHCompiler
    from pysph_amd.nnps import HipNNPS
    from pysph_amd.scheme import WCSPHScheme
    pa, dx = make_cube(args.n1)
    s = WCSPHScheme(['fluid'], [], dim=3, rho0=1000.0, c0=10.0, h0=1.3 * dx, hdx=1.3, gz=-9.81, alpha=0.2, beta=0.0,
                    **options)
    s.setup_properties([pa])
    kernel = K.WendlandQuintic(dim=3)
    ctx = dev.HipContext(0, stream.cuda_stream)
    dev.attach(pa, ctx).push()
    a_eval = AccelerationEval([pa], s.get_equations(), kernel)
    SPHCompiler(a_eval, ctx=ctx, sync='manual').compile()
    nnps = HipNNPS(3, [pa], radius_scale=kernel.radius_scale, ctx=ctx, sync=False)
    a_eval.set_nnps(nnps)
    nnps.update()
    for _ in range(args.warmup):
        a_eval.compute(0.0, 1e-4)
    ctx.synchronize()
    runs = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.batch):
            a_eval.compute(0.0, 1e-4)
        e1.record(stream)
        ctx.synchronize()
        runs.append(e0.elapsed_time(e1) / args.batch)
    ctx.timer_enable(True)
    ctx.timer_reset()
    for _ in range(args.batch):
        a_eval.compute(0.0, 1e-4)
    ctx.synchronize()
    split = {}
    for k in KEYS:
        ms, count = ctx.timer_get(k)
        if count:
            split[k] = dict(ms_per_eval=ms / args.batch, launches_per_eval=count / args.batch)
    ctx.timer_enable(False)
    pa.gpu.pull('arho', 'au')
    out = dict(particles=pa.get_number_of_particles(), options=options, eval_ms=float(np.median(runs)),
               all_ms=[round(x, 4) for x in runs], split=split,
               checksum=[float(np.abs(pa.arho).sum()), float(np.abs(pa.au).sum())])
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n1', type=int, default=100)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--batch', type=int, default=50, help='evaluations between one pair of events')
    ap.add_argument('--warmup', type=int, default=60)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    result = dict(n1=args.n1, reps=args.reps, batch=args.batch, warmup=args.warmup)
    for name, options in (('plain', {}), ('delta_sph_nu', dict(delta_sph=True, nu=0.01)),
                          ('nu', dict(nu=0.01))):
        result[name] = measure(options, args, torch, stream)
    result['delta_sph_nu_over_plain'] = result['delta_sph_nu']['eval_ms'] / result['plain']['eval_ms']
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()
