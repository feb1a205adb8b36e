"""1-D Sod shock tube with ``ADKEScheme`` -- the particles of examples/shock_tube.py under ADKE.

The parameters are those of the reference's ``sod_shocktube.py``: ``alpha=1, beta=1, k=0.3, eps=0.5, g1=0.2, g2=0.4``
(of which ``ADKEAccelerations`` keeps ``g1`` for both), one pilot smoothing length ``h0 = 1.2 dx_right`` for every
particle, Gaussian kernel, PEC steps with ``ADKEStep`` at the fixed time step 1e-4.  Every evaluation sums the pilot
density with ``h = h0``, reduces ``logrho`` on the device and scales every ``h`` from it; nothing crosses to the host
between the push before the first step and the pull behind the last.

``__main__`` prints the mean state of the plateau between the contact discontinuity and the shock next to the exact
Riemann solution.
"""
import numpy as np

from ..gas_dynamics import ADKEScheme
from ..kernels import Gaussian
from . import shock_tube as ST

HDX = 1.2
EXACT = ST.EXACT


def create_scheme(**kw):
    opts = dict(fluids=['fluid'], solids=[], dim=1, gamma=ST.GAMMA, alpha=1.0, beta=1.0, k=0.3, eps=0.5, g1=0.2, g2=0.4)
    opts.update(kw)
    return ADKEScheme(**opts)


def create_particles(n=900):
    pa = ST.create_particles(n)
    create_scheme().setup_properties([pa])
    dxr = float(pa.x[-1] - pa.x[-2])
    pa.h0[:] = HDX * dxr
    pa.h[:] = pa.h0
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
    a_eval = AccelerationEval([pa], s.get_equations(), kernel)
    SPHCompiler(a_eval, ctx=ctx, sync='manual').compile()
    nnps = HipNNPS(1, [pa], radius_scale=kernel.radius_scale, ctx=ctx, sync=False)
    a_eval.set_nnps(nnps)
    integ = s.configure_solver(kernel=kernel, tf=tf, dt=dt)
    setup_integrator(integ, a_eval, nnps)
    t, steps = 0.0, 0
    while t < tf - 1e-12:
        step = min(dt, tf - t)
        integ.step(t, step)
        t += step
        steps += 1
    pa.gpu.pull(*floats)
    if own:
        ctx.close()
    res = dict(array=pa, t=t, steps=steps, m_initial=m_initial, k=s.k, eps=s.eps)
    if not quiet:
        print(report(res))
    return res


def report(res):
    pa, t = res['array'], res['t']
    got, count = ST.plateau(pa, t)
    lines = ['%d particles, %d PEC steps to t = %.4f; h / h0 between %.3f and %.3f'
             % (pa.get_number_of_particles(True), res['steps'], t, float(np.min(pa.h / pa.h0)), float(np.max(pa.h / pa.h0))),
             'plateau between contact and shock (%d particles):' % count]
    for k in ('p', 'u', 'rho'):
        lines.append('  %-3s %.5f   exact %.5f   (%+.2f %%)' % (k, got[k], EXACT[k], 100 * (got[k] / EXACT[k] - 1)))
    return '\n'.join(lines)


if __name__ == '__main__':
    import argparse
    ap = argparse.ArgumentParser(description='1-D Sod shock tube (ADKEScheme) on one MI355X')
    ap.add_argument('--n', type=int, default=900)
    ap.add_argument('--tf', type=float, default=0.15)
    ap.add_argument('--dt', type=float, default=1e-4)
    args = ap.parse_args()
    run(n=args.n, tf=args.tf, dt=args.dt)
