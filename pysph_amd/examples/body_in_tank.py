"""A fixed block in a settling water column: the force the fluid puts on it.

An illustration of ``pysph_amd.rigid_body`` (nothing here is validated
against an experiment): a closed tank of WCSPH boundary particles, a column of
water at rest that settles under gravity, and a block of body particles
standing on the floor.  The fluid feels the block through Akinci's pressure
and friction forces; the same pair loop adds the reaction to ``fx, fy, fz`` of
the block's particles (``s_fx[s_idx] += ...``: the transposed launch of
DESIGN.md section 7c).  By default the block is held fixed and the run prints
the total force on it per step: the weight of the block plus, once the column
has settled, the buoyancy.  With ``--free`` the block is a rigid body lighter
than water (``get_particle_array_rigid_body``): ``RigidBodyMoments`` sums the
force and torque on it, ``RigidBodyMotion`` gives its particles the body's
velocity and ``RK2StepRigidBody`` moves it; the run then
prints its centre of mass and velocity, from one small pull of the body state.

The coupling equations sit in a group of their own behind the hand-written
WCSPH rates: they continue from the accelerations in memory, and a store to a
source property may not depend on what a hand-written unit of the same group
writes.

    python -m pysph_amd.examples.body_in_tank [--dx 0.05 --steps 50 --free]
"""
import numpy as np

from ..equations import (ContinuityEquation, Group, MomentumEquation, TaitEOS,
                         XSPHCorrection)
from ..kernels import CubicSpline
from ..particle_array import (get_particle_array_rigid_body,
                              get_particle_array_wcsph)
from ..rigid_body import (BodyForce, NumberDensity, PressureRigidBody,
                          RigidBodyMoments, RigidBodyMotion, RK2StepRigidBody,
                          ViscosityRigidBody)

dim = 3
hdx = 1.3
rho0 = 1000.0
gamma = 7.0
depth = 0.6
c0 = 10.0 * np.sqrt(2.0 * 9.81 * depth)
g = -9.81
body_rho = 2000.0
free_body_rho = 500.0           # --free: lighter than the water, so that it rises
BODY_PROPS = ['V', 'fx', 'fy', 'fz']


def create_particles(dx=0.05, free=False):
    """tank 1 x 1 x 1 with two layers of walls, water up to `depth`, a 0.3^3 block on the floor in the middle
    (free: the block is one rigid body of density `free_body_rho`)"""
    n = int(round(1.0 / dx))
    c = (np.arange(-2, n + 2) + 0.5) * dx
    x, y, z = [a.ravel() for a in np.meshgrid(c, c, c, indexing='ij')]
    inside = (x > 0) & (x < 1) & (y > 0) & (z > 0) & (z < 1)
    wall = ~inside & (y < 1.0)
    half = 0.15 + 1e-6 * dx         # (a lattice point at exactly 0.15 from the axis is in on both sides)
    block = inside & (abs(x - 0.5) < half) & (abs(z - 0.5) < half) & (y < 0.3)
    water = inside & ~block & (y < depth)
    # a gap of one spacing around the block: the body particles stand for the fluid there
    near = inside & (abs(x - 0.5) < half + dx) & (abs(z - 0.5) < half + dx) & (y < 0.3 + dx)
    water &= ~near
    arrays = []
    for name, msk in (('fluid', water), ('tank', wall), ('block', block)):
        k = int(msk.sum())
        if free and name == 'block':
            pa = get_particle_array_rigid_body(name=name, x=x[msk], y=y[msk], z=z[msk], h=hdx * dx * np.ones(k),
                                               m=free_body_rho * dx ** 3 * np.ones(k), rho=rho0 * np.ones(k))
        else:
            pa = get_particle_array_wcsph(name=name, x=x[msk], y=y[msk], z=z[msk], h=hdx * dx * np.ones(k),
                                          m=(body_rho if name == 'block' else rho0) * dx ** 3 * np.ones(k),
                                          rho=rho0 * np.ones(k))
        for p in BODY_PROPS:
            if p not in pa.properties:
                pa.add_property(p)
        arrays.append(pa)
    return arrays


def create_equations(dx=0.05, nu=0.05, free=False):
    everyone = ['fluid', 'tank']
    # free: the force and torque on the body from the forces on its particles, then the particles' velocities
    dynamics = [Group(equations=[RigidBodyMoments(dest='block', sources=None)]),
                Group(equations=[RigidBodyMotion(dest='block', sources=None)])] if free else []
    return [
        Group(real=False, equations=[TaitEOS(dest=a, sources=None, rho0=rho0, c0=c0, gamma=gamma) for a in everyone]),
        # the weight of the block's particles and their number density (V: what a body particle stands for is 1 / V)
        Group(equations=[BodyForce(dest='block', sources=None, gy=g),
                         NumberDensity(dest='block', sources=['block'])]),
        Group(equations=[ContinuityEquation(dest='tank', sources=['fluid']),
                         ContinuityEquation(dest='fluid', sources=everyone),
                         MomentumEquation(dest='fluid', sources=everyone, c0=c0, alpha=0.25, beta=0.0, gy=g),
                         XSPHCorrection(dest='fluid', sources=['fluid'], eps=0.5)]),
        # fluid <- block, and the reaction on the block in the same pair loop
        Group(equations=[PressureRigidBody(dest='fluid', sources=['block'], rho0=rho0),
                         ViscosityRigidBody(dest='fluid', sources=['block'], rho0=rho0, nu=nu)]),
    ] + dynamics


def run(dx=0.05, n_steps=50, ctx=None, log=True, free=False):
    """EPEC steps, device-resident; per step the total force on the block (three small pulls).  free: the block
    moves; per step the force on it, its centre of mass and velocity (one pull of the body state: 9 doubles)."""
    from .. import device as dev
    from ..acceleration_eval import AccelerationEval, SPHCompiler
    from ..integrator import EPECIntegrator, WCSPHStep, setup_integrator
    from ..nnps import HipNNPS
    ctx = ctx or dev.HipContext(0)
    arrays = create_particles(dx, free)
    kernel = CubicSpline(dim=dim)
    for a in arrays:
        dev.attach(a, ctx).push()
    a_eval = AccelerationEval(arrays, create_equations(dx, free=free), kernel)
    SPHCompiler(a_eval, ctx=ctx, sync='manual').compile()
    nnps = HipNNPS(dim, arrays, radius_scale=kernel.radius_scale, ctx=ctx, sync=False)
    a_eval.set_nnps(nnps)
    steppers = dict(fluid=WCSPHStep(), tank=WCSPHStep())
    if free:
        steppers['block'] = RK2StepRigidBody()
    integ = EPECIntegrator(**steppers)
    setup_integrator(integ, a_eval, nnps)
    dt = 0.125 * hdx * dx / (1.1 * c0)
    block = arrays[2]
    weight = float(block.m.sum()) * g
    forces, t = [], 0.0
    for step in range(n_steps):
        integ.step(t, dt)
        t += dt
        if free:
            block.gpu.pull('force', 'cm', 'vc')
            forces.append(tuple(float(v) for v in block.force))
            if log:
                print('step %3d  t = %.5f  cm = (%.5f, %.5f, %.5f)  vc = (%+.4e, %+.4e, %+.4e)  force y = %+.4e'
                      % ((step + 1, t) + tuple(block.cm) + tuple(block.vc) + (forces[-1][1],)))
            continue
        block.gpu.pull('fx', 'fy', 'fz')
        f = (float(block.fx.sum()), float(block.fy.sum()), float(block.fz.sum()))
        forces.append(f)
        if log:
            print('step %3d  t = %.5f  force on the block = (%+.4e, %+.4e, %+.4e)  [weight %+.4e]'
                  % (step + 1, t, f[0], f[1], f[2], weight))
    return arrays, forces


if __name__ == '__main__':
    import argparse
    ap = argparse.ArgumentParser(description='force of a settling water column on a fixed block, one MI355X')
    ap.add_argument('--dx', type=float, default=0.05)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--free', action='store_true', help='the block is a rigid body lighter than water and moves')
    args = ap.parse_args()
    run(dx=args.dx, n_steps=args.steps, free=args.free)
