"""1-D Sod shock tube with ``GasDScheme`` -- problem set-up and a device-resident time loop.

Left state rho, p = 1, 1, right state 0.125, 0.1, gamma = 1.4, particles of equal mass (spacing ratio 8), Gaussian
kernel, PEC steps with ``GasDFluidStep`` and the time step from ``dt_cfl`` (``Integrator.compute_time_step``).  The tube
is [-1, 1] with the diaphragm at 0 and free ends: by t = 0.2 what the ends send inwards has not reached the waves.
Every evaluation solves the smoothing lengths by the iterated density group (``adaptive_h_scheme='mpm'``).

``__main__`` prints the mean state of the plateau between the contact discontinuity and the shock next to the exact
Riemann solution p* = 0.30313, u* = 0.92745, rho = 0.26557.
"""
import numpy as np

from ..gas_dynamics import GasDScheme
from ..kernels import Gaussian
from ..particle_array import get_particle_array_gasd

GAMMA = 1.4
RHO_L, P_L, RHO_R, P_R = 1.0, 1.0, 0.125, 0.1
KERNEL_FACTOR = 1.5
EXACT = dict(p=0.30313, u=0.92745, rho=0.26557)     # between contact and shock
U_CONTACT, U_SHOCK = 0.92745, 1.75216


def create_scheme(**kw):
    opts = dict(fluids=['fluid'], solids=[], dim=1, gamma=GAMMA, kernel_factor=KERNEL_FACTOR, alpha1=1.0, alpha2=1.0,
                beta=2.0, update_alpha1=True, update_alpha2=True, max_density_iterations=50,
                density_iteration_tolerance=1e-3)
    opts.update(kw)
    return GasDScheme(**opts)


def create_particles(n=900):
    """about n particles: eight on the left for every one on the right"""
    nr = max(int(round(n / 9.0)), 4)
    nl = 8 * nr
    dxl, dxr = 1.0 / nl, 1.0 / nr
    x = np.concatenate([-1.0 + (np.arange(nl) + 0.5) * dxl, (np.arange(nr) + 0.5) * dxr])
    left = x < 0
    rho = np.where(left, RHO_L, RHO_R)
    p = np.where(left, P_L, P_R)
    pa = get_particle_array_gasd(
        name='fluid', x=x, m=RHO_L * dxl * np.ones_like(x), rho=rho, p=p, e=p / ((GAMMA - 1.0) * rho),
        h=KERNEL_FACTOR * np.where(left, dxl, dxr), cs=np.sqrt(GAMMA * p / rho))
    pa.alpha1[:] = 1.0
    pa.alpha2[:] = 1.0
    pa.omega[:] = 1.0
    create_scheme().setup_properties([pa])
    return pa


def run(n=900, tf=0.2, cfl=0.3, dt0=1e-4, ctx=None, quiet=False):
    from .. import device as dev
    from ..acceleration_eval import AccelerationEval, SPHCompiler
    from ..integrator import setup_integrator
    from ..nnps import HipNNPS
    own = ctx is None
    ctx = ctx or dev.HipContext(0)
    pa = create_particles(n)
    m_initial = pa.m.copy()
    s = create_scheme()
    kernel = Gaussian(dim=1)
    dev.attach(pa, ctx).push(*[p for p in pa.properties if pa.properties[p].dtype == np.float64])
    a_eval = AccelerationEval([pa], s.get_equations(), kernel)
    SPHCompiler(a_eval, ctx=ctx, sync='manual').compile()
    nnps = HipNNPS(1, [pa], radius_scale=kernel.radius_scale, ctx=ctx, sync=False)
    a_eval.set_nnps(nnps)
    integ = s.configure_solver(kernel=kernel)
    setup_integrator(integ, a_eval, nnps)
    group = a_eval.equation_groups[0]                  # the iterated density group
    t, dt, steps, its = 0.0, dt0, 0, []
    while t < tf:
        dt = min(dt, tf - t)
        integ.step(t, dt)
        its.append(a_eval.c_acceleration_eval.iteration_counts[group.name])
        t += dt
        steps += 1
        new = integ.compute_time_step(dt, cfl)         # cfl h_min / max(dt_cfl), reduced on the device
        if new is not None:
            dt = min(new, 1.1 * dt)                    # the first steps grow from dt0
    pa.gpu.pull(*[p for p in pa.properties if pa.properties[p].dtype == np.float64])
    if own:
        ctx.close()
    res = dict(array=pa, t=t, steps=steps, iterations=its, m_initial=m_initial,
               max_density_iterations=s.max_density_iterations)
    if not quiet:
        print(report(res))
    return res


def plateau(pa, t):
    """mean p, u, rho of the particles in the middle half of the region between contact and shock"""
    lo, hi = U_CONTACT * t, U_SHOCK * t
    sel = (pa.x > lo + 0.25 * (hi - lo)) & (pa.x < hi - 0.25 * (hi - lo))
    return dict((k, float(np.mean(pa.properties[k][sel]))) for k in ('p', 'u', 'rho')), int(np.sum(sel))


def report(res):
    pa, t = res['array'], res['t']
    got, count = plateau(pa, t)
    its = res['iterations']
    lines = ['%d particles, %d PEC steps to t = %.4f; density iterations per evaluation %d..%d (mean %.2f)'
             % (pa.get_number_of_particles(True), res['steps'], t, min(its), max(its), float(np.mean(its))),
             'plateau between contact and shock (%d particles):' % count]
    for k in ('p', 'u', 'rho'):
        lines.append('  %-3s %.5f   exact %.5f   (%+.2f %%)' % (k, got[k], EXACT[k], 100 * (got[k] / EXACT[k] - 1)))
    return '\n'.join(lines)


if __name__ == '__main__':
    import argparse
    ap = argparse.ArgumentParser(description='1-D Sod shock tube (GasDScheme, mpm) on one MI355X')
    ap.add_argument('--n', type=int, default=900)
    ap.add_argument('--tf', type=float, default=0.2)
    args = ap.parse_args()
    run(n=args.n, tf=args.tf)
