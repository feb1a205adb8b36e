"""1-D Sod shock tube with ``GSPHScheme`` -- the set-up of examples/shock_tube.py under Godunov SPH.

Same particles (left state rho, p = 1, 1, right state 0.125, 0.1, gamma = 1.4, equal masses, Gaussian kernel, free
ends); the scheme's defaults (exact Riemann solver, linear interpolation, I02 limiter), Euler steps with ``GSPHStep``
at a fixed time step: ``GSPHAcceleration`` writes no ``dt_cfl``, and the reference's shock-tube example runs GSPH at a
fixed step too.

``__main__`` prints the mean state of the plateau between the contact discontinuity and the shock next to the exact
Riemann solution, and the number of Riemann solves that failed (none is expected).
"""
import numpy as np

from ..gas_dynamics import GSPHScheme
from ..kernels import Gaussian
from . import shock_tube as ST

KERNEL_FACTOR = ST.KERNEL_FACTOR
EXACT = ST.EXACT


def create_scheme(**kw):
    opts = dict(fluids=['fluid'], solids=[], dim=1, gamma=ST.GAMMA, kernel_factor=KERNEL_FACTOR, g1=0.0, g2=0.0,
                rsolver=2, interpolation=1, monotonicity=1, interface_zero=True, niter=40, tol=1e-6)
    opts.update(kw)
    return GSPHScheme(**opts)


def create_particles(n=900):
    pa = ST.create_particles(n)
    create_scheme().setup_properties([pa])
    return pa


def run(n=900, tf=0.15, dt=1e-4, ctx=None, quiet=False, **scheme_kw):
    from .. import device as dev
    from ..acceleration_eval import AccelerationEval, SPHCompiler
    from ..integrator import setup_integrator
    from ..nnps import HipNNPS
    own = ctx is None
    ctx = ctx or dev.HipContext(0)
    pa = create_particles(n)
    m_initial = pa.m.copy()
    s = create_scheme(**scheme_kw)
    kernel = Gaussian(dim=1)
    floats = [p for p in pa.properties if pa.properties[p].dtype == np.float64]
    dev.attach(pa, ctx).push(*floats)
    groups = s.get_equations()
    a_eval = AccelerationEval([pa], groups, kernel)
    SPHCompiler(a_eval, ctx=ctx, sync='manual').compile()
    nnps = HipNNPS(1, [pa], radius_scale=kernel.radius_scale, ctx=ctx, sync=False)
    a_eval.set_nnps(nnps)
    integ = s.configure_solver(kernel=kernel, tf=tf, dt=dt)
    setup_integrator(integ, a_eval, nnps)
    acc = groups[-1].equations[0]
    t, steps, failed = 0.0, 0, 0
    while t < tf - 1e-12:
        step = min(dt, tf - t)
        integ.step(t, step)
        t += step
        steps += 1
        if steps % 100 == 0:                 # the failure word is read now and then, not every step
            failed += acc.solver_failures()
    if steps % 100:
        failed += acc.solver_failures()
    pa.gpu.pull(*floats)
    if own:
        ctx.close()
    res = dict(array=pa, t=t, steps=steps, m_initial=m_initial, solver_failures=failed)
    if not quiet:
        print(report(res))
    return res


def report(res):
    pa, t = res['array'], res['t']
    got, count = ST.plateau(pa, t)
    lines = ['%d particles, %d Euler steps to t = %.4f; Riemann solves that failed in the sampled evaluations: %d'
             % (pa.get_number_of_particles(True), res['steps'], t, res['solver_failures']),
             'plateau between contact and shock (%d particles):' % count]
    for k in ('p', 'u', 'rho'):
        lines.append('  %-3s %.5f   exact %.5f   (%+.2f %%)' % (k, got[k], EXACT[k], 100 * (got[k] / EXACT[k] - 1)))
    return '\n'.join(lines)


if __name__ == '__main__':
    import argparse
    ap = argparse.ArgumentParser(description='1-D Sod shock tube (GSPHScheme) on one MI355X')
    ap.add_argument('--n', type=int, default=900)
    ap.add_argument('--tf', type=float, default=0.15)
    ap.add_argument('--dt', type=float, default=1e-4)
    ap.add_argument('--rsolver', default='exact')
    args = ap.parse_args()
    choices = create_scheme().rsolver_choices
    run(n=args.n, tf=args.tf, dt=args.dt, rsolver=choices[args.rsolver])
