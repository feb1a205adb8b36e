"""2-D Taylor-Green vortex with the EDAC scheme, internal-flow branch -- problem
set-up and a device-resident time loop.

The set-up of ``examples/taylor_green.py`` (unit periodic box, U = 1, rho0 = 1,
c0 = 10, Re = 100, hdx = 1, QuinticSpline) with ``EDACScheme(pb = c0^2 rho0)``:
the pressure is integrated state, so it starts from the exact field
p = -U^2 rho0 (cos 4 pi x + cos 4 pi y) / 4, and the steps are EPEC with
``EDACTVFStep`` (pysph/examples/taylor_green.py with ``--scheme edac``
configures ``EDACScheme`` the same way).  The exact solution decays as
exp(-8 pi^2 nu t / L^2); ``__main__`` prints the measured rate next to it.
"""
import numpy as np

from ..edac import EDACScheme
from ..kernels import QuinticSpline
from ..particle_array import get_particle_array

L, U, rho0 = 1.0, 1.0, 1.0
c0 = 10 * U
p0 = c0 ** 2 * rho0
hdx = 1.0


def create_scheme(nx=50, re=100.0):
    dx = L / nx
    return EDACScheme(['fluid'], [], dim=2, c0=c0, nu=U * L / re, rho0=rho0, pb=p0, h=hdx * dx)


def create_particles(nx=50, re=100.0):
    dx = L / nx
    g = (np.arange(nx) + 0.5) * dx
    x, y = [a.ravel().copy() for a in np.meshgrid(g, g, indexing='ij')]
    pa = get_particle_array(
        name='fluid', x=x, y=y, h=hdx * dx * np.ones_like(x),
        m=rho0 * dx * dx * np.ones_like(x), rho=rho0 * np.ones_like(x),
        u=-U * np.cos(2 * np.pi * x) * np.sin(2 * np.pi * y),
        v=U * np.sin(2 * np.pi * x) * np.cos(2 * np.pi * y),
        p=-0.25 * U * U * rho0 * (np.cos(4 * np.pi * x) + np.cos(4 * np.pi * y)))
    create_scheme(nx, re).setup_properties([pa])
    pa.V[:] = 1.0 / (dx * dx)
    pa.uhat[:] = pa.u
    pa.vhat[:] = pa.v
    return [pa], dx


def run(nx=50, re=100.0, n_steps=200, ctx=None):
    """EPEC steps, device-resident incl. the periodic images."""
    import time

    from .. import device as dev
    from ..acceleration_eval import AccelerationEval, SPHCompiler
    from ..domain import HipDomainManager
    from ..integrator import EPECIntegrator, setup_integrator
    from ..nnps import HipNNPS
    ctx = ctx or dev.HipContext(0)
    arrays, dx = create_particles(nx, re)
    s = create_scheme(nx, re)
    kernel = QuinticSpline(dim=2)
    h0 = hdx * dx
    dt = min(0.25 * h0 / (c0 + U), 0.125 * h0 * h0 / s.nu)
    for a in arrays:
        dev.attach(a, ctx).push(*[p for p in a.properties if a.properties[p].dtype == np.float64])
    a_eval = AccelerationEval(arrays, s.get_equations(), kernel)
    SPHCompiler(a_eval, ctx=ctx, sync='manual').compile()
    dom = HipDomainManager(ctx=ctx, xmin=0, xmax=L, ymin=0, ymax=L, periodic_in_x=True,
                           periodic_in_y=True)
    nnps = HipNNPS(2, arrays, radius_scale=kernel.radius_scale, ctx=ctx, sync=False,
                   domain=dom)
    a_eval.set_nnps(nnps)
    integ = s.configure_solver(kernel=kernel, integrator_cls=EPECIntegrator)
    setup_integrator(integ, a_eval, nnps)
    t, t0 = 0.0, time.perf_counter()
    for _ in range(n_steps):
        integ.step(t, dt)
        t += dt
    ctx.synchronize()
    wall = time.perf_counter() - t0
    arrays[0].gpu.pull('x', 'y', 'u', 'v', 'p', 'rho')
    return arrays, dict(steps=n_steps, t=t, dt=dt, nu=s.nu, wall_s=wall,
                        steps_per_s=n_steps / wall)


def decay_rate(pa, t):
    """-ln(max|v| / U) / t: the exact field gives 8 pi^2 nu / L^2"""
    n = pa.get_number_of_particles(True)
    return -np.log(np.sqrt(pa.u[:n] ** 2 + pa.v[:n] ** 2).max() / U) / t


if __name__ == '__main__':
    import argparse
    ap = argparse.ArgumentParser(description='2-D Taylor-Green vortex (EDAC, internal branch) on one MI355X')
    ap.add_argument('--nx', type=int, default=100)
    ap.add_argument('--steps', type=int, default=2000)
    args = ap.parse_args()
    arrs, st = run(nx=args.nx, n_steps=args.steps)
    pa = arrs[0]
    print('%d particles, %d EPEC steps to t = %.4f in %.2f s wall (%.0f steps/s); decay rate of max|v| %.4f, '
          'exact %.4f' % (pa.get_number_of_particles(True), st['steps'], st['t'], st['wall_s'],
                          st['steps_per_s'], decay_rate(pa, st['t']), 8 * np.pi ** 2 * st['nu'] / L ** 2))
