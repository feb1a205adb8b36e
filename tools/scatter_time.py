"""What the transposed launch of a source-store family costs.

A jittered lattice of about a million fluid particles over a slab of about
fifty thousand body particles, one group with AkinciRigidFluidCoupling
(pysph_amd/rigid_body.py): the fluid's acceleration in the forward launch, the
force on the body particles in the transposed one.  One pair of device events
around a BATCH of back-to-back calls (default 20) of the forward unit alone,
of the transposed unit alone and of the whole group, so that the stream stays
busy and the host path to the first launch is amortised; per-call time = the
interval / batch; medians over the repetitions after a warm-up and a burst of
device work for the clock.  Device-resident, neighbour grid built once.

What a call contains (everything `sph_eval_generated` enqueues for the unit):
  forward     packing the body's records and the fluid's own position records,
              then the pair launch over the fluid's rows;
  transposed  packing the FLUID's records (about a million) and the body's own,
              then the pair launch over the body's rows;
  group       both, through `AccelerationEval.compute`.

    python tools/scatter_time.py [--n 102 --layers 5 --reps 15 --batch 20] [--varh 0.0] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def particles(n1, layers, varh, seed=1):
    from pysph_amd.particle_array import get_particle_array
    rng = np.random.default_rng(seed)
    dx = 1.0 / n1
    g = (np.arange(n1) + 0.5) * dx
    x, y, z = [a.ravel() for a in np.meshgrid(g, g, g, indexing='ij')]
    body = y < layers * dx
    arrays = []
    for name, msk in (('fluid', ~body), ('body', body)):
        n = int(msk.sum())
        pa = get_particle_array(
            name=name, x=x[msk] + 0.1 * dx * rng.uniform(-1, 1, n), y=y[msk] + 0.1 * dx * rng.uniform(-1, 1, n),
            z=z[msk] + 0.1 * dx * rng.uniform(-1, 1, n), h=1.3 * dx * (1 + varh * rng.uniform(-1, 1, n)),
            m=dx ** 3 * np.ones(n), rho=1 + 0.1 * rng.uniform(-1, 1, n), p=rng.uniform(1, 2, n),
            additional_props=['V', 'fx', 'fy', 'fz', 'au', 'av', 'aw'])
        pa.V[:] = dx ** 3
        arrays.append(pa)
    return arrays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=102)
    ap.add_argument('--layers', type=int, default=5)
    ap.add_argument('--varh', type=float, default=0.0)
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--batch', type=int, default=20, help='calls between one pair of events')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from pysph_amd import device as dev
    from pysph_amd import kernels as K
    from pysph_amd.acceleration_eval import AccelerationEval, SPHCompiler
    from pysph_amd.equations import Group
    from pysph_amd.nnps import HipNNPS
    from pysph_amd.rigid_body import AkinciRigidFluidCoupling
    arrays = particles(args.n, args.layers, args.varh)
    eqs = [Group(equations=[AkinciRigidFluidCoupling('fluid', ['body'], fluid_rho=1.0)])]
    kernel = K.CubicSpline(dim=3)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = dev.HipContext(0, stream.cuda_stream)
    a_eval = AccelerationEval(arrays, eqs, kernel)
    SPHCompiler(a_eval, ctx=ctx, sync='manual').compile()
    nnps = HipNNPS(3, arrays, radius_scale=kernel.radius_scale, ctx=ctx)
    a_eval.set_nnps(nnps)
    for pa in arrays:
        pa.gpu.push()
    nnps.update()
    ev = a_eval.c_acceleration_eval
    (group, cg), = ev.plan
    forward, transposed = cg.units
    assert transposed.fam.transposed == 'fluid'
    cg.refresh_range()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.batch):
            fn()
        e1.record(stream)
        ctx.synchronize()
        return e0.elapsed_time(e1) / args.batch
    parts = dict(forward=lambda: forward.run(ev, 0.0, 1e-4), transposed=lambda: transposed.run(ev, 0.0, 1e-4),
                 group=lambda: a_eval.compute(0.0, 1e-4))
    for _ in range(40):             # warm-up: code objects, record buffers, and the clock
        for fn in parts.values():
            fn()
    ctx.synchronize()
    runs = dict((k, []) for k in parts)
    for _ in range(args.reps):
        for k, fn in parts.items():
            runs[k].append(timed(fn))
    med = dict((k, float(np.median(v))) for k, v in runs.items())
    result = dict(particles=dict((pa.name, pa.get_number_of_particles()) for pa in arrays), varh=args.varh,
                  kernel='CubicSpline', reps=args.reps, batch=args.batch, median_ms=med,
                  all_ms=dict((k, [round(x, 4) for x in v]) for k, v in runs.items()),
                  transposed_share_of_forward=med['transposed'] / med['forward'])
    print(json.dumps(result))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)
    ctx.close()


if __name__ == '__main__':
    main()
