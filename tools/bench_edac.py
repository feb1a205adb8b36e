#!/usr/bin/env python
"""Time the EDAC internal-branch force group next to the TVF force group (GPU only; fails without a device).

    python tools/bench_edac.py --out OUTDIR [--n1 100] [--reps 60]

A periodic cube of n1^3 particles (100 -> 1 M), QuinticSpline, hdx = 1, jittered lattice, random velocities and
pressures.  One evaluation of the whole EDAC group list first sets rho, V and pavg on every row (images included);
then, on the same context, arrays and neighbour grid:

    edac_force   [MomentumEquationPressureGradient, MomentumEquationViscosity, MomentumEquationArtificialStress,
                 EDACEquation] of pysph_amd.edac -- FamEDAC_T, the flag set compiled as a constant
    tvf_force    [MomentumEquationPressureGradient, MomentumEquationViscosity, MomentumEquationArtificialStress] of the
                 TVF scheme -- FamTVF_T on its own records (no StateEquation group before it: p and V gathered)

are evaluated alternately after a warm-up of at least a second, each evaluation timed by the host clock around a
device synchronise; the medians, their ratio and the quartiles go to OUTDIR/bench_edac.json and to stdout.  The TVF
group is the yardstick because it is the same sweep minus the pressure-rate term, the gather of m and the pavg read.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n1', type=int, default=100)
    ap.add_argument('--reps', type=int, default=60)
    ap.add_argument('--out', default='.')
    ap.add_argument('--f32', action='store_true', help='option arith_f32')
    args = ap.parse_args()
    from pysph_amd import device as dev
    from pysph_amd.acceleration_eval import AccelerationEval, SPHCompiler
    from pysph_amd.domain import HipDomainManager
    from pysph_amd.edac import EDACScheme
    from pysph_amd.kernels import QuinticSpline
    from pysph_amd.nnps import HipNNPS
    from pysph_amd.particle_array import get_particle_array
    from pysph_amd.scheme import TVFScheme
    ctx = dev.HipContext(0)         # raises without a GPU
    if args.f32:
        ctx.set_option('arith_f32', 1)
    n1 = args.n1
    rng = np.random.default_rng(5)
    dx = 1.0 / n1
    g = (np.arange(n1) + 0.5) * dx
    x, y, z = [a.ravel() + 0.1 * dx * rng.uniform(-1, 1, n1 ** 3) for a in np.meshgrid(g, g, g, indexing='ij')]
    n = x.size
    rho0, c0, nu = 1.0, 10.0, 0.01
    pa = get_particle_array(name='fluid', x=x, y=y, z=z, h=dx * np.ones(n), m=rho0 * dx ** 3 * np.ones(n),
                            rho=rho0 * np.ones(n), u=rng.uniform(-1, 1, n), v=rng.uniform(-1, 1, n),
                            w=rng.uniform(-1, 1, n), p=0.05 * rho0 * c0 * c0 * rng.uniform(-1, 1, n))
    edac = EDACScheme(['fluid'], [], dim=3, c0=c0, nu=nu, rho0=rho0, pb=rho0 * c0 * c0, h=dx)
    tvf = TVFScheme(['fluid'], [], dim=3, rho0=rho0, c0=c0, nu=nu, p0=rho0 * c0 * c0, pb=rho0 * c0 * c0, h0=dx)
    edac.setup_properties([pa])
    tvf.setup_properties([pa])
    for a, b in zip(('uhat', 'vhat', 'what'), 'uvw'):
        pa.properties[a][:] = pa.properties[b] + 0.1 * rng.uniform(-1, 1, n)
    kernel = QuinticSpline(dim=3)
    dev.attach(pa, ctx).push(*[p for p in pa.properties if pa.properties[p].dtype == np.float64])
    evals = {}
    for name, eqs in (('all', edac.get_equations()), ('edac_force', edac.get_equations()[-1:]),
                      ('tvf_force', tvf.get_equations()[-1:])):
        evals[name] = AccelerationEval([pa], eqs, kernel)
        SPHCompiler(evals[name], ctx=ctx, sync='manual').compile()
    dom = HipDomainManager(ctx=ctx, xmin=0, xmax=1, ymin=0, ymax=1, zmin=0, zmax=1, periodic_in_x=True,
                           periodic_in_y=True, periodic_in_z=True)
    nnps = HipNNPS(3, [pa], radius_scale=kernel.radius_scale, ctx=ctx, sync=False, domain=dom)
    for ev in evals.values():
        ev.set_nnps(nnps)
    nnps.update()
    evals['all'].compute(0.0, 1e-4)
    ctx.synchronize()

    def once(name):
        t0 = time.perf_counter()
        evals[name].compute(0.0, 1e-4)
        ctx.synchronize()
        return 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 1.0:           # clocks and code objects settle
        once('edac_force')
        once('tvf_force')
    times = dict(edac_force=[], tvf_force=[])
    for _ in range(args.reps):
        for name in ('edac_force', 'tvf_force'):
            times[name].append(once(name))
    result = dict(particles=n, rows_with_images=int(pa.gpu.get_number_of_particles()), kernel='QuinticSpline',
                  reps=args.reps, arith='fp32' if args.f32 else 'fp64')
    for name, v in times.items():
        q = np.percentile(v, [25, 50, 75])
        result[name] = dict(median_ms=float(q[1]), q25_ms=float(q[0]), q75_ms=float(q[2]))
    result['ratio'] = result['edac_force']['median_ms'] / result['tvf_force']['median_ms']
    os.makedirs(args.out, exist_ok=True)
    tag = '_f32' if args.f32 else ''
    with open(os.path.join(args.out, 'bench_edac%s.json' % tag), 'w') as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
    ctx.close()


if __name__ == '__main__':
    main()
