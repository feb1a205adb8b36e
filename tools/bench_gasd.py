#!/usr/bin/env python
"""Time the gas-dynamics evaluation of GasDScheme (GPU only; fails without a device).

    python tools/bench_gasd.py --out OUTDIR [--n1 100] [--reps 60] [--f32] [--adke]

A periodic cube of n1^3 particles (100 -> 1 M), QuinticSpline, kernel_factor 1, jittered lattice, masses +-10 % (the
density noise the smoothing lengths have to follow), random velocities and energies.  On one context, one array and
one neighbour grid, after a warm-up of at least a second, each evaluation timed by the host clock around a device
synchronise, medians and quartiles of `reps`:

    tvf_force       the TVF force group of DESIGN.md section 7f on the same box (uniform h), the yardstick for "a sweep
                    of this record size"; measured first, before the smoothing lengths vary
    density         the iterated density group from the initial h (pushed again and the stepper's initialize run before
                    every repetition, outside the clock): iterations per evaluation, ms per evaluation and per iteration
                    (one neighbour update with its periodic images and one sweep each), and the sweep alone from the
                    timer pair_gasd_density -- with option gasd_skip 0 and 1 alternately
    force           [IdealGasEOS | MPMUpdateGhostProps | MPMAccelerations] at the converged state, and the sweep alone
                    from the timer pair_gasd_mpm
    pec_step        whole PEC steps with GasDFluidStep (dt = 1e-4 of the box)
    gsph            GSPHScheme on the same box at the same converged state: the gradient group
                    [GSPHGradients] and its sweep alone (timer pair_gsph_gradients); per Riemann solver exact, hllc and
                    roe the force group [GSPHUpdateGhostProps | GSPHAcceleration], its sweep alone (timer pair_gsph),
                    its ratio to the MPM force group above and the solves that failed; after the PEC steps, whole Euler
                    steps with GSPHStep (exact)

    --adke          instead of everything but the MPM force group (re-measured as the yardstick of the session): ADKEScheme
                     on the same box at the same converged state with a three-layer wall array
                    of 3 n1^2 particles next to the fluid, k = 1, eps = 0.5, g1 = 0.2: the density group
                    [SummationDensityADKE] (h = h0, packing, sweep, reduction, the h launch) and sweep + reduction alone (timer
                    pair_adke_density), the wall group [WallBoundary] (timer pair_gasd_wall), the force group
                    [IdealGasEOS | ADKEUpdateGhostProps | ADKEAccelerations] (timer pair_adke) and whole PEC steps with
                    ADKEStep; writes bench_gasd_adke.json

The equation classes of pysph_amd.gas_dynamics are parameter holders without Python bodies, so the same group list
cannot be forced through run-time-generated families: there is no generated comparison.
Results go to OUTDIR/bench_gasd.json and to stdout.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def quartiles(v):
    q = np.percentile(v, [25, 50, 75])
    return dict(median_ms=float(q[1]), q25_ms=float(q[0]), q75_ms=float(q[2]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n1', type=int, default=100)
    ap.add_argument('--reps', type=int, default=60)
    ap.add_argument('--out', default='.')
    ap.add_argument('--f32', action='store_true', help='option arith_f32')
    ap.add_argument('--adke', action='store_true', help='the ADKE rows and the MPM force group only')
    args = ap.parse_args()
    from pysph_amd import device as dev
    from pysph_amd.acceleration_eval import AccelerationEval, SPHCompiler
    from pysph_amd.domain import HipDomainManager
    from pysph_amd.gas_dynamics import ADKEScheme, GasDScheme, GSPHScheme
    from pysph_amd.integrator import setup_integrator
    from pysph_amd.kernels import QuinticSpline
    from pysph_amd.nnps import HipNNPS
    from pysph_amd.particle_array import get_particle_array_gasd
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
    h_init = dx * np.ones(n)
    pa = get_particle_array_gasd(name='fluid', x=x, y=y, z=z, h=h_init.copy(),
                                 m=dx ** 3 * (1 + 0.1 * rng.uniform(-1, 1, n)), rho=np.ones(n),
                                 u=0.3 * rng.uniform(-1, 1, n), v=0.3 * rng.uniform(-1, 1, n),
                                 w=0.3 * rng.uniform(-1, 1, n), e=rng.uniform(1.0, 3.0, n), p=rng.uniform(0.5, 1.5, n))
    pa.alpha1[:] = 1.0
    pa.alpha2[:] = 0.1
    pa.omega[:] = 1.0
    gas = GasDScheme(['fluid'], [], dim=3, gamma=1.4, kernel_factor=1.0, has_ghosts=True, max_density_iterations=50)
    gas.setup_properties([pa])
    tvf = TVFScheme(['fluid'], [], dim=3, rho0=1.0, c0=10.0, nu=0.01, p0=100.0, pb=100.0, h0=dx)
    tvf.setup_properties([pa])
    for a, b in zip(('uhat', 'vhat', 'what'), 'uvw'):
        pa.properties[a][:] = pa.properties[b]
    solvers = (('exact', 2), ('hllc', 3), ('roe', 6))
    gsph = dict((name, GSPHScheme(['fluid'], [], dim=3, gamma=1.4, kernel_factor=1.0, has_ghosts=True, rsolver=rs))
                for name, rs in solvers)
    gsph['exact'].setup_properties([pa])
    kernel = QuinticSpline(dim=3)
    arrays = [pa]
    if args.adke:
        from pysph_amd.particle_array import ParticleArray
        gw = (np.arange(n1) + 0.5) * dx
        wx, wy, wz = [a.ravel() for a in np.meshgrid(gw, gw, (np.arange(3) + 1.0) * dx, indexing='ij')]
        wall = ParticleArray(name='wall', x=wx, y=wy, z=wz, h=dx * np.ones(wx.size))
        adke = ADKEScheme(['fluid'], ['wall'], dim=3, gamma=1.4, alpha=1.0, beta=2.0, k=1.0, eps=0.5, g1=0.2, g2=0.4,
                          has_ghosts=True)
        adke.setup_properties([pa, wall])
        wall.properties['h0'][:] = dx
        dev.attach(wall, ctx).push(*[p for p in wall.properties if wall.properties[p].dtype == np.float64])
        arrays.append(wall)
    dev.attach(pa, ctx).push(*[p for p in pa.properties if pa.properties[p].dtype == np.float64])
    groups = gas.get_equations()
    lists = dict(tvf_all=tvf.get_equations(), tvf_force=tvf.get_equations()[-1:], all=groups, density=groups[:1],
                 force=groups[1:])
    gsph_eqs = dict((name, sch.get_equations()) for name, sch in gsph.items())
    lists['gsph_all'] = gsph_eqs['exact']
    lists['gsph_grad'] = gsph_eqs['exact'][5:6]
    for name, eqs in gsph_eqs.items():
        assert [e.name for grp in eqs[5:] for e in grp.equations] == ['GSPHGradients', 'GSPHUpdateGhostProps', 'GSPHAcceleration']
        lists['gsph_force_' + name] = eqs[6:]
    if args.adke:
        aeqs = adke.get_equations()
        names = [[e.name for e in grp.equations] for grp in aeqs]
        assert names == [['WallBoundary'], ['SummationDensityADKE'], ['WallBoundary'], ['SummationDensity'], ['WallBoundary'],
                         ['IdealGasEOS', 'IdealGasEOS'], ['ADKEUpdateGhostProps'], ['ADKEAccelerations']]
        lists = dict(all=groups, force=groups[1:], adke_all=aeqs, adke_density=aeqs[1:2], adke_wall=aeqs[2:3],
                     adke_force=aeqs[5:])
    evals = {}
    for name, eqs in lists.items():
        evals[name] = AccelerationEval(arrays, eqs, kernel)
        SPHCompiler(evals[name], ctx=ctx, sync='manual').compile()
    dom = HipDomainManager(ctx=ctx, xmin=0, xmax=1, ymin=0, ymax=1, zmin=0, zmax=1, periodic_in_x=True,
                           periodic_in_y=True, periodic_in_z=True)
    nnps = HipNNPS(3, arrays, radius_scale=kernel.radius_scale, ctx=ctx, sync=False, domain=dom)
    for ev in evals.values():
        ev.set_nnps(nnps)
    aid = pa.gpu.array_id

    def clocked(fn):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    def warm(fn, seconds=1.0):
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < seconds:           # clocks and code objects settle
            fn()

    def timer(key):
        ms, cnt = C.c_double(), C.c_long()
        dev._check(ctx.lib.sph_timer_get(ctx._h, key.encode(), C.byref(ms), C.byref(cnt)))
        return ms.value, cnt.value

    result = dict(particles=n, kernel='QuinticSpline', kernel_factor=1.0, reps=args.reps,
                  arith='fp32' if args.f32 else 'fp64')
    if args.adke:
        return bench_adke(args, ctx, pa, wall, adke, evals, nnps, kernel, h_init, result, clocked, warm, timer)
    # -- the yardstick, on the uniform-h box ----------------------------------------------------------------------
    nnps.update_domain()
    nnps.update()
    evals['tvf_all'].compute(0.0, 1e-4)
    warm(lambda: clocked(lambda: evals['tvf_force'].compute(0.0, 1e-4)))
    result['tvf_force'] = quartiles([clocked(lambda: evals['tvf_force'].compute(0.0, 1e-4)) for _ in range(args.reps)])
    result['rows_with_images'] = int(pa.gpu.get_number_of_particles())

    # -- the density iteration from the initial h -------------------------------------------------------------------
    def reset():
        pa.properties['h'][:n] = h_init
        nreal = pa.gpu.get_number_of_particles(True)
        dev._check(ctx.lib.sph_array_push(ctx._h, aid, dev.prop_id('h'), h_init.ctypes.data_as(C.POINTER(C.c_double)), 0, nreal))
        dev._check(ctx.lib.sph_array_mark_written(ctx._h, aid, dev.prop_id('h')))
        dev._check(ctx.lib.sph_integrate_stage(ctx._h, aid, 8, 0, C.c_double(1e-4)))     # converged = 0, omega = 1, h0 = h
        nnps.update_domain()
        nnps.update()

    def density():
        evals['density'].compute(0.0, 1e-4)

    def its_of(name):
        return list(evals[name].c_acceleration_eval.iteration_counts.values())[0]

    def warm_density():
        reset()
        density()
    warm(warm_density)
    ctx.lib.sph_timer_enable(ctx._h, 1)
    for skip in (0, 1):
        result['density_skip%d' % skip] = dict(ms=[], its=[])
    sweep = {}
    for rep in range(args.reps):
        for skip in (0, 1):
            ctx.set_option('gasd_skip', skip)
            reset()
            ms0, c0 = timer('pair_gasd_density')
            s0 = timer('n_gasd_skipped')[1]
            r = result['density_skip%d' % skip]
            r['ms'].append(clocked(density))
            r['its'].append(its_of('density'))
            ms1, c1 = timer('pair_gasd_density')
            sweep.setdefault(skip, []).append(((ms1 - ms0), c1 - c0, timer('n_gasd_skipped')[1] - s0))
    ctx.lib.sph_timer_enable(ctx._h, 0)
    for skip in (0, 1):
        r = result['density_skip%d' % skip]
        ms, its = np.array(r.pop('ms')), np.array(r.pop('its'))
        r.update(per_evaluation=quartiles(ms), per_iteration=quartiles(ms / its), iterations=sorted(set(int(v) for v in its)),
                 sweeps_per_evaluation_ms=float(np.median([s[0] for s in sweep[skip]])),
                 sweep_alone_ms=float(np.median([s[0] / max(s[1], 1) for s in sweep[skip]])),
                 wavefronts_skipped_per_evaluation=int(np.median([s[2] for s in sweep[skip]])))
    ctx.set_option('gasd_skip', 0)

    # -- the force group at the converged state -----------------------------------------------------------------------
    reset()
    evals['all'].compute(0.0, 1e-4)
    warm(lambda: clocked(lambda: evals['force'].compute(0.0, 1e-4)))
    result['force'] = quartiles([clocked(lambda: evals['force'].compute(0.0, 1e-4)) for _ in range(args.reps)])
    ctx.lib.sph_timer_enable(ctx._h, 1)
    ms0, c0 = timer('pair_gasd_mpm')
    for _ in range(10):
        evals['force'].compute(0.0, 1e-4)
    ms1, c1 = timer('pair_gasd_mpm')
    ctx.lib.sph_timer_enable(ctx._h, 0)
    result['force']['sweep_alone_ms'] = (ms1 - ms0) / max(c1 - c0, 1)
    result['force_over_tvf_force'] = result['force']['median_ms'] / result['tvf_force']['median_ms']

    # -- GSPH at the same state: the gradient group, then the force group per Riemann solver ---------------------------
    def timed_group(name, key):
        fn = lambda: evals[name].compute(0.0, 1e-4)
        warm(lambda: clocked(fn))
        r = quartiles([clocked(fn) for _ in range(args.reps)])
        ctx.lib.sph_timer_enable(ctx._h, 1)
        ms0, c0 = timer(key)
        for _ in range(10):
            fn()
        ms1, c1 = timer(key)
        ctx.lib.sph_timer_enable(ctx._h, 0)
        r['sweep_alone_ms'] = (ms1 - ms0) / max(c1 - c0, 1)
        return r
    result['gsph'] = dict(gradients=timed_group('gsph_grad', 'pair_gsph_gradients'))
    for name, _ in solvers:
        r = timed_group('gsph_force_' + name, 'pair_gsph')
        r['solver_failures'] = gsph_eqs[name][-1].equations[0].solver_failures()
        r['over_mpm_force'] = r['median_ms'] / result['force']['median_ms']
        r['sweep_over_mpm_sweep'] = r['sweep_alone_ms'] / result['force']['sweep_alone_ms']
        result['gsph']['force_' + name] = r

    # -- whole PEC steps ------------------------------------------------------------------------------------------------
    integ = gas.configure_solver(kernel=kernel)
    setup_integrator(integ, evals['all'], nnps)
    state = dict(t=0.0)

    def step():
        integ.step(state['t'], 1e-4 * dx / 0.01)
        state['t'] += 1e-4 * dx / 0.01
    warm(lambda: clocked(step))
    ms, its = [], []
    for _ in range(args.reps):
        ms.append(clocked(step))
        its.append(its_of('all'))
    result['pec_step'] = dict(quartiles(ms), iterations=sorted(set(int(v) for v in its)))

    # -- whole Euler steps of GSPHScheme (exact) ----------------------------------------------------------------------
    ginteg = gsph['exact'].configure_solver(kernel=kernel)
    setup_integrator(ginteg, evals['gsph_all'], nnps)

    def gstep():
        ginteg.step(state['t'], 1e-4 * dx / 0.01)
        state['t'] += 1e-4 * dx / 0.01
    warm(lambda: clocked(gstep))
    result['gsph']['euler_step'] = quartiles([clocked(gstep) for _ in range(args.reps)])
    result['gsph']['euler_step']['solver_failures'] = gsph_eqs['exact'][-1].equations[0].solver_failures()
    os.makedirs(args.out, exist_ok=True)
    tag = '_f32' if args.f32 else ''
    with open(os.path.join(args.out, 'bench_gasd%s.json' % tag), 'w') as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
    ctx.close()


def bench_adke(args, ctx, pa, wall, adke, evals, nnps, kernel, h_init, result, clocked, warm, timer):
    """--adke: the MPM force group as yardstick, then the three ADKE groups and whole PEC steps, at the state the density
    iteration of GasDScheme converges to; h0 of the fluid is that h over 1.1, so that the h the reduction writes stays
    within the cells of the last neighbour update"""
    from pysph_amd import device as dev
    from pysph_amd.integrator import setup_integrator
    aid = pa.gpu.array_id
    n = h_init.size
    dx = 1.0 / args.n1
    dev._check(ctx.lib.sph_integrate_stage(ctx._h, aid, 8, 0, C.c_double(1e-4)))       # converged = 0, omega = 1, h0 = h
    nnps.update_domain()
    nnps.update()
    evals['all'].compute(0.0, 1e-4)
    result['rows_with_images'] = int(pa.gpu.get_number_of_particles())
    result['wall_rows'] = int(wall.get_number_of_particles())

    def timed_group(name, key):
        fn = lambda: evals[name].compute(0.0, 1e-4)
        warm(lambda: clocked(fn))
        r = quartiles([clocked(fn) for _ in range(args.reps)])
        ctx.lib.sph_timer_enable(ctx._h, 1)
        ms0, c0 = timer(key)
        for _ in range(10):
            fn()
        ms1, c1 = timer(key)
        ctx.lib.sph_timer_enable(ctx._h, 0)
        r['sweep_alone_ms'] = (ms1 - ms0) / max(c1 - c0, 1)
        return r
    result['force'] = timed_group('force', 'pair_gasd_mpm')
    pa.gpu.pull('h')
    pa.properties['h0'][:n] = pa.properties['h'][:n] / 1.1
    nreal = pa.gpu.get_number_of_particles(True)
    h0 = np.ascontiguousarray(pa.properties['h0'][:nreal])
    dev._check(ctx.lib.sph_array_push(ctx._h, aid, dev.prop_id('h0'), h0.ctypes.data_as(C.POINTER(C.c_double)), 0, nreal))
    nnps.update_domain()                   # the images take the new h0
    nnps.update()
    evals['adke_all'].compute(0.0, 1e-4)
    result['adke'] = dict(density=timed_group('adke_density', 'pair_adke_density'),
                          wall=timed_group('adke_wall', 'pair_gasd_wall'),
                          force=timed_group('adke_force', 'pair_adke'))
    for r in result['adke'].values():
        r['over_mpm_force'] = r['median_ms'] / result['force']['median_ms']
        r['sweep_over_mpm_sweep'] = r['sweep_alone_ms'] / result['force']['sweep_alone_ms']
    integ = adke.configure_solver(kernel=kernel)
    setup_integrator(integ, evals['adke_all'], nnps)
    state = dict(t=0.0)

    def step():
        integ.step(state['t'], 1e-4 * dx / 0.01)
        state['t'] += 1e-4 * dx / 0.01
    warm(lambda: clocked(step))
    result['adke']['pec_step'] = quartiles([clocked(step) for _ in range(args.reps)])
    pa.gpu.pull('h', 'h0')
    lam = pa.properties['h'][:n] / pa.properties['h0'][:n]
    result['adke']['lambda'] = [float(lam.min()), float(lam.max())]
    os.makedirs(args.out, exist_ok=True)
    tag = '_f32' if args.f32 else ''
    with open(os.path.join(args.out, 'bench_gasd_adke%s.json' % tag), 'w') as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
    ctx.close()


if __name__ == '__main__':
    main()
