"""Flow through an open channel: inlet -> WCSPH fluid between walls -> outlet.

A minimal open-boundary problem in the spirit of the reference's
``pysph/examples/trivial_inlet_outlet.py``: particles enter the fluid from an
inlet block that moves with the prescribed velocity, are integrated as weakly
compressible fluid between two wall rows (``nz == 1``: a 2-D channel; ``nz > 1``:
a 3-D duct with four walls) and leave through an outlet block.  Everything
stays on the device: EPEC integrator, ``WCSPHStep`` for the fluid, generated
stage families for the inlet and the outlet, and
``InletBase.update`` / ``OutletBase.update`` (pysph_amd/inlet_outlet.py) after
the integrator stages through ``set_post_stage_callback``.

The lattice rows are staggered along x in ``phases`` groups, so that particles
cross the two interfaces in bursts with quiet updates in between instead of a
whole lattice plane at once.

gid: every particle gets a unique gid, mirrored on the device so that it
travels with its row.  A particle that enters the fluid carries the gid of the
inlet row it was copied from (that row wraps back and enters again one inlet
length later).
"""
import numpy as np

from ..inlet_outlet import InletInfo, InletOutletManager, InletStep, OutletInfo
from ..kernels import WendlandQuintic
from ..particle_array import get_particle_array_wcsph
from ..scheme import WCSPHScheme

rho0 = 1000.0
u0 = 1.0
c0 = 10.0 * u0
hdx = 1.2
gamma = 7.0
alpha = 0.1


class CarriedStep(InletStep):
    """``InletStep`` for updates after EVERY stage.  It keeps all the
    start-of-step copies WCSPHStep reads (y0 ... rho0) current, so that a
    particle handed to the fluid after stage 1 is integrated through stage 2
    from its own start-of-step state; and its second stage advances x from where
    the particle IS, not from x0: an inlet row that wrapped back after stage 1
    must not return to x0 + dt u, across the interface, and enter twice."""

    def initialize(self, d_idx, d_x0, d_y0, d_z0, d_u0, d_v0, d_w0, d_rho0, d_x, d_y, d_z, d_u,
                   d_v, d_w, d_rho):
        d_x0[d_idx] = d_x[d_idx]
        d_y0[d_idx] = d_y[d_idx]
        d_z0[d_idx] = d_z[d_idx]
        d_u0[d_idx] = d_u[d_idx]
        d_v0[d_idx] = d_v[d_idx]
        d_w0[d_idx] = d_w[d_idx]
        d_rho0[d_idx] = d_rho[d_idx]

    def stage2(self, d_idx, d_x, d_u, dt):
        d_x[d_idx] += 0.5 * dt * d_u[d_idx]


def create_particles(dx=0.02, nx=100, ny=25, nz=1, n_io=4, phases=4, wall_layers=2, outlet_filled=False):
    """[fluid, inlet, outlet, wall]; the fluid fills 0 <= x < nx dx, the inlet
    the n_io lattice planes before it, the outlet (empty unless outlet_filled)
    the n_io planes behind it."""
    dim = 2 if nz == 1 else 3
    jj, kk = [a.ravel() for a in np.meshgrid(np.arange(ny), np.arange(nz), indexing='ij')]
    stagger = ((jj + kk) % phases) / float(phases) * 0.5 * dx    # per lattice row along x, below half a spacing
    ys, zs = (jj + 0.5) * dx, ((kk + 0.5) * dx if dim == 3 else 0.0 * kk)

    def block(i0, i1):
        ii = np.arange(i0, i1)
        x = ((ii[:, None] + 0.5) * dx + stagger[None, :]).ravel()
        y = np.broadcast_to(ys, (ii.size, ys.size)).ravel()
        z = np.broadcast_to(zs, (ii.size, zs.size)).ravel()
        return x, y, z

    out = []
    for name, (i0, i1) in (('fluid', (0, nx)), ('inlet', (-n_io, 0)),
                           ('outlet', (nx, nx + n_io if outlet_filled else nx))):
        x, y, z = block(i0, i1)
        out.append(get_particle_array_wcsph(name=name, x=x, y=y, z=z, u=u0 * np.ones_like(x)))
    # walls: `wall_layers` lattice rows around the cross-section, along the whole length
    wi = np.arange(-n_io - 2, nx + n_io + 3)
    wj = np.arange(-wall_layers, ny + wall_layers)
    wk = np.arange(-wall_layers, nz + wall_layers) if dim == 3 else np.arange(1)
    I, J, K = [a.ravel() for a in np.meshgrid(wi, wj, wk, indexing='ij')]
    outside = (J < 0) | (J >= ny)
    if dim == 3:
        outside |= (K < 0) | (K >= nz)
    I, J, K = I[outside], J[outside], K[outside]
    out.append(get_particle_array_wcsph(name='wall', x=(I + 0.5) * dx, y=(J + 0.5) * dx,
                                        z=(K + 0.5) * dx if dim == 3 else 0.0 * K))
    gid0 = 0
    for pa in out:
        n = pa.get_number_of_particles()
        pa.m[:] = rho0 * dx ** dim
        pa.h[:] = hdx * dx
        pa.rho[:] = rho0
        pa.gid[:] = np.arange(gid0, gid0 + n)
        gid0 += n
        for prop in ('ioid', 'disp'):
            pa.add_property(prop)
    return out


def create_manager(dx, nx):
    """interfaces at x = 0 (inlet) and x = nx dx (outlet), normals out of the fluid"""
    iom = InletOutletManager(
        ['fluid'], [InletInfo('inlet', normal=[-1.0, 0.0, 0.0], refpoint=[0.0, 0.0, 0.0], has_ghost=False)],
        [OutletInfo('outlet', normal=[1.0, 0.0, 0.0], refpoint=[nx * dx, 0.0, 0.0])])
    iom.update_dx(dx)
    return iom


class ChannelFlow(object):
    """The device-resident run.  ``make_updates(sim)`` may supply other objects
    with ``update(t, dt, stage)`` than the manager's (tests drive the same run
    through the host-side structural helpers for comparison)."""

    def __init__(self, dx=0.02, nx=100, ny=25, nz=1, n_io=4, phases=4, active_stages=(1, 2),
                 dt=None, ctx=None, make_updates=None):
        from .. import device as dev
        from ..acceleration_eval import AccelerationEval, SPHCompiler
        from ..integrator import EPECIntegrator, WCSPHStep, setup_integrator
        from ..nnps import HipNNPS
        self.dim = 2 if nz == 1 else 3
        self.dx, self.nx, self.n_io = dx, nx, n_io
        self.ctx = ctx or dev.HipContext(0)
        self.arrays = create_particles(dx, nx, ny, nz, n_io, phases)
        self.by_name = dict((pa.name, pa) for pa in self.arrays)
        self.kernel = WendlandQuintic(dim=self.dim)
        self.iom = create_manager(dx, nx)
        self.iom.setup_iom(self.dim, self.kernel)
        self.iom.active_stages = list(active_stages)
        scheme = WCSPHScheme(['fluid'], ['wall', 'inlet', 'outlet'], dim=self.dim, rho0=rho0, c0=c0,
                             h0=hdx * dx, hdx=hdx, gamma=gamma, alpha=alpha)
        dev.prop_register('gid')                  # travels with its row, as in a slab migration
        for pa in self.arrays:
            dev.attach(pa, self.ctx).push()
        # (the outlet starts empty: its length is that of the inlet block, not of its particles)
        self.iom.outletinfo[0].length = n_io * dx
        self.ios = self.iom.get_inlet_outlet(self.by_name)
        if make_updates is not None:
            self.ios = make_updates(self)
        a_eval = AccelerationEval(self.arrays, scheme.get_equations(), self.kernel)
        SPHCompiler(a_eval, ctx=self.ctx, sync='manual').compile()
        self.nnps = HipNNPS(self.dim, self.arrays, radius_scale=self.kernel.radius_scale, ctx=self.ctx, sync=False)
        a_eval.set_nnps(self.nnps)
        self.integrator = EPECIntegrator(fluid=WCSPHStep(), inlet=CarriedStep(), outlet=CarriedStep())
        setup_integrator(self.integrator, a_eval, self.nnps)
        self.integrator.set_post_stage_callback(
            lambda t, dt_, stage: [io.update(t, dt_, stage) for io in self.ios])
        self.dt = dt if dt is not None else 0.25 * hdx * dx / (c0 + u0)
        self.t = 0.0
        self.steps = 0

    def step(self):
        self.integrator.step(self.t, self.dt)
        self.t += self.dt
        self.steps += 1

    def sizes(self):
        return dict((pa.name, pa.gpu.get_number_of_particles()) for pa in self.arrays)

    def sync_host(self):
        self.ctx.synchronize()
        for pa in self.arrays:
            pa.gpu.sync_host()


def run(n_steps=100, log=None, **kw):
    sim = ChannelFlow(**kw)
    for _ in range(n_steps):
        sim.step()
        if log and sim.steps % log == 0:
            print('step %d  t = %.5f  %s' % (sim.steps, sim.t, sim.sizes()))
    sim.sync_host()
    return sim


if __name__ == '__main__':
    import argparse
    ap = argparse.ArgumentParser(description='open channel flow on one MI355X')
    ap.add_argument('--dx', type=float, default=0.01)
    ap.add_argument('--nx', type=int, default=200)
    ap.add_argument('--ny', type=int, default=50)
    ap.add_argument('--nz', type=int, default=1)
    ap.add_argument('--steps', type=int, default=200)
    args = ap.parse_args()
    s = run(n_steps=args.steps, log=50, dx=args.dx, nx=args.nx, ny=args.ny, nz=args.nz)
    print('t = %.4f: %s' % (s.t, s.sizes()))
