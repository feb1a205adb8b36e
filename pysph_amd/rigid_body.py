"""Forces between a fluid and the particles of an immersed body.

Every class here computes, in ONE pair loop over (fluid particle, body
particle), the acceleration the body gives the fluid particle and the
reaction on the body particle, ``s_fx[s_idx] += ...``: action and reaction are
the same term.  ``pysph_amd.codegen`` turns the second half into a transposed
launch of its own, so the classes have no hand-written
kernel.  Class names, constructor arguments and the array names in the method
signatures are the interface of pysph/sph/rigid_body.py (``BodyForce`` :232,
``NumberDensity`` :260, ``ViscosityRigidBody`` :280, ``PressureRigidBody``
:311, ``AkinciRigidFluidCoupling`` :338, ``LiuFluidForce`` :378); the bodies
are written from the papers' formulae:

* Akinci, Ihmsen, Akinci, Solenthaler & Teschner, "Versatile rigid-fluid
  coupling for incompressible SPH", ACM TOG 31(4), 2012.  A body particle b
  stands for the fluid mass ``psi_b = rho0 vol_b`` (eq. 5); the pressure force
  on fluid particle i is ``F_i<-b = -m_i psi_b (p_i / rho_i^2) grad W_ib``
  (eq. 9), the friction force ``-m_i psi_b Pi_ib grad W_ib`` with the
  artificial-viscosity term ``Pi_ib = -nu min(v_ib . x_ib, 0) / (rho_i (|x_ib|^2
  + eps))`` (eqs. 11-14), and the body particle takes ``-F_i<-b`` (eq. 10).
  Every body below forms that force on the fluid particle first, divides it by
  ``m_i`` for the acceleration and subtracts it from the body particle.
  ``PressureRigidBody`` / ``ViscosityRigidBody`` read ``V`` as a NUMBER density
  (``vol_b = 1 / V_b``, what ``NumberDensity`` computes);
  ``AkinciRigidFluidCoupling`` reads it as the volume itself and mirrors the
  fluid pressure onto the body particle (the factor 2).
* Liu, Xie, Xu & Shao (doi 10.1155/2017/3174904): the symmetric pressure term
  ``-m_b (p_b / rho_b^2 + p_i / rho_i^2) grad W_ib`` with the body particles
  carrying a pressure and density of their own (``LiuFluidForce``).

The bodies move, too.  ``RigidBodyMoments`` (:69) sums mass, centre of mass,
inertia, force and torque of every body and solves Euler's equation for the
angular acceleration; ``RigidBodyMotion`` (:215) gives every body particle the
velocity ``vc + omega x (r - cm)``; ``RK2StepRigidBody`` (:718) and
``EulerStepRigidBody`` (:695) advance the particles and the bodies' ``vc`` and
``omega``.  On the device these four are hand-written kernels over a block of
per-body state (csrc/sph_rigid.hip) that
``AccelerationEval`` and ``HipIntegrator`` call through the C-ABI; the method
bodies below are their host twins -- plain Python over the arrays and constants
of ``get_particle_array_rigid_body`` -- written from the formulae:

* ``M = sum m``, ``cm = sum m r / M``; inertia about the origin ``sum m (|r|^2 1
  - r r^T)`` moved to ``cm`` by the parallel-axis theorem ``I = I_0 - M (|cm|^2
  1 - cm cm^T)``; ``F = sum f``, ``tau = sum r x f - cm x F``;
* Euler's equation ``I omega_dot = tau - omega x (I omega)``, solved with the
  adjugate of the symmetric ``I`` over its determinant.

The collisions of the bodies (``RigidBodyCollision``, ``RigidBodyWallCollision``,
``RigidBodyForceGPUGems``) are not part of this module.
"""
import numpy as np

from .equations import Equation
from .integrator import IntegratorStep

def body_index(body_id, nbody):
    """(order, start): the rows sorted by body id, stable in row order, and where each body's rows begin in
    `order` (start[nbody] = n).  An id outside [0, nbody) or a body without particles is a ValueError (in the
    reference: an index error or a division by zero)."""
    ids = np.asarray(body_id)
    nbody = int(nbody)
    if ids.size and (np.any(ids < 0) or np.any(ids >= nbody) or np.any(ids != np.floor(ids))):
        bad = ids[(ids < 0) | (ids >= nbody) | (ids != np.floor(ids))][0]
        raise ValueError('body_id %r is outside [0, %d)' % (bad, nbody))
    ids = ids.astype(np.int64)
    counts = np.bincount(ids, minlength=nbody)
    if nbody < 1 or np.any(counts == 0):
        empty = int(np.nonzero(counts == 0)[0][0]) if nbody >= 1 else 0
        raise ValueError('body %d of %d has no particles' % (empty, nbody))
    order = np.argsort(ids, kind='stable').astype(np.uint32)
    start = np.zeros(nbody + 1, dtype=np.uint32)
    start[1:] = np.cumsum(counts)
    return order, start


def solve_symmetric3(ixx, iyy, izz, ixy, ixz, iyz, rx, ry, rz):
    """``I^-1 r`` for the symmetric ``I``: adjugate over determinant"""
    a00 = iyy * izz - iyz * iyz
    a01 = ixz * iyz - ixy * izz
    a02 = ixy * iyz - ixz * iyy
    a11 = ixx * izz - ixz * ixz
    a12 = ixy * ixz - ixx * iyz
    a22 = ixx * iyy - ixy * ixy
    rdet = 1.0 / (ixx * a00 + ixy * a01 + ixz * a02)
    return ((a00 * rx + a01 * ry + a02 * rz) * rdet,
            (a01 * rx + a11 * ry + a12 * rz) * rdet,
            (a02 * rx + a12 * ry + a22 * rz) * rdet)


class RigidBodyMoments(Equation):
    """total_mass, cm, mi (the inertia tensor about cm in mi[0..8]), force, ac, torque and omega_dot of every body,
    from x y z m fx fy fz of ALL rows of the array and the bodies' omega.  On the device: ``sph_rigid_moments``, run
    where this ``reduce`` would run (the hook itself is then not called)."""

    def reduce(self, dst, t, dt):
        nbody = int(dst.num_body[0])
        order, start = body_index(dst.body_id, nbody)
        mi = dst.mi
        for b in range(nbody):
            rows = order[start[b]:start[b + 1]]
            m, x, y, z = dst.m[rows], dst.x[rows], dst.y[rows], dst.z[rows]
            fx, fy, fz = dst.fx[rows], dst.fy[rows], dst.fz[rows]
            mass = np.sum(m)
            cx, cy, cz = np.sum(m * x) / mass, np.sum(m * y) / mass, np.sum(m * z) / mass
            # about the origin, then to the centre of mass (parallel-axis theorem)
            ixx = np.sum(m * (y * y + z * z)) - (cy * cy + cz * cz) * mass
            iyy = np.sum(m * (x * x + z * z)) - (cx * cx + cz * cz) * mass
            izz = np.sum(m * (x * x + y * y)) - (cx * cx + cy * cy) * mass
            myz = np.sum(m * y * z)
            ixy = cx * cy * mass - np.sum(m * x * y)
            ixz = cx * cz * mass - np.sum(m * x * z)
            iyz = cy * cz * mass - myz
            force = (np.sum(fx), np.sum(fy), np.sum(fz))
            origin = (np.sum(y * fz - z * fy), np.sum(z * fx - x * fz), np.sum(x * fy - y * fx))
            torque = (origin[0] - (cy * force[2] - cz * force[1]),
                      origin[1] - (cz * force[0] - cx * force[2]),
                      origin[2] - (cx * force[1] - cy * force[0]))
            dst.total_mass[b] = mass
            dst.cm[3 * b:3 * b + 3] = (cx, cy, cz)
            mi[16 * b:16 * b + 9] = (ixx, ixy, ixz, ixy, iyy, iyz, ixz, iyz, izz)
            # (slots 9..15: what the reference's temporaries leave there)
            mi[16 * b + 9] = -myz
            mi[16 * b + 10:16 * b + 13] = force
            mi[16 * b + 13:16 * b + 16] = origin
            dst.force[3 * b:3 * b + 3] = force
            dst.ac[3 * b:3 * b + 3] = (force[0] / mass, force[1] / mass, force[2] / mass)
            dst.torque[3 * b:3 * b + 3] = torque
            wx, wy, wz = dst.omega[3 * b:3 * b + 3]
            lx = ixx * wx + ixy * wy + ixz * wz
            ly = ixy * wx + iyy * wy + iyz * wz
            lz = ixz * wx + iyz * wy + izz * wz
            dst.omega_dot[3 * b:3 * b + 3] = solve_symmetric3(
                ixx, iyy, izz, ixy, ixz, iyz,
                torque[0] - (wy * lz - wz * ly), torque[1] - (wz * lx - wx * lz), torque[2] - (wx * ly - wy * lx))


class RigidBodyMotion(Equation):
    """``(u, v, w) = vc + omega x (r - cm)`` of the particle's body.  On the device: ``sph_rigid_motion``."""

    def initialize(self, d_idx, d_x, d_y, d_z, d_u, d_v, d_w,
                   d_cm, d_vc, d_ac, d_omega, d_body_id):
        base = 3 * int(d_body_id[d_idx])
        wx = d_omega[base]
        wy = d_omega[base + 1]
        wz = d_omega[base + 2]
        rx = d_x[d_idx] - d_cm[base]
        ry = d_y[d_idx] - d_cm[base + 1]
        rz = d_z[d_idx] - d_cm[base + 2]
        d_u[d_idx] = d_vc[base] + wy * rz - wz * ry
        d_v[d_idx] = d_vc[base + 1] + wz * rx - wx * rz
        d_w[d_idx] = d_vc[base + 2] + wx * ry - wy * rx


def _advance_bodies(d_idx, d_num_body, new, old, rate, f):
    """``new = old + f rate`` for the 3 nb components of a per-body vector, once per stage (particle 0)"""
    if d_idx == 0:
        for k in range(3 * int(d_num_body[0])):
            new[k] = old[k] + f * rate[k]


class EulerStepRigidBody(IntegratorStep):
    """forward Euler for the bodies and their particles (one stage; for tests)"""

    def initialize(self):
        pass

    def stage1(self, d_idx, d_u, d_v, d_w, d_x, d_y, d_z,
               d_omega, d_omega_dot, d_vc, d_ac, d_num_body,
               dt=0.0):
        _advance_bodies(d_idx, d_num_body, d_vc, d_vc, d_ac, dt)
        _advance_bodies(d_idx, d_num_body, d_omega, d_omega, d_omega_dot, dt)
        d_x[d_idx] += dt * d_u[d_idx]
        d_y[d_idx] += dt * d_v[d_idx]
        d_z[d_idx] += dt * d_w[d_idx]


class RK2StepRigidBody(IntegratorStep):
    """midpoint rule: positions, vc and omega from their values at the start of the step (x0, vc0, omega0) and the
    velocities / accelerations of the latest evaluation -- half a step in stage 1, the whole step in stage 2"""

    def initialize(self, d_idx, d_x, d_y, d_z, d_x0, d_y0, d_z0,
                   d_omega, d_omega0, d_vc, d_vc0, d_num_body):
        if d_idx == 0:
            for k in range(3 * int(d_num_body[0])):
                d_vc0[k] = d_vc[k]
                d_omega0[k] = d_omega[k]
        d_x0[d_idx] = d_x[d_idx]
        d_y0[d_idx] = d_y[d_idx]
        d_z0[d_idx] = d_z[d_idx]

    def _advance(self, f, d_idx, d_u, d_v, d_w, d_x, d_y, d_z, d_x0, d_y0, d_z0,
                 d_omega, d_omega_dot, d_vc, d_ac, d_omega0, d_vc0, d_num_body):
        _advance_bodies(d_idx, d_num_body, d_vc, d_vc0, d_ac, f)
        _advance_bodies(d_idx, d_num_body, d_omega, d_omega0, d_omega_dot, f)
        d_x[d_idx] = d_x0[d_idx] + f * d_u[d_idx]
        d_y[d_idx] = d_y0[d_idx] + f * d_v[d_idx]
        d_z[d_idx] = d_z0[d_idx] + f * d_w[d_idx]

    def stage1(self, d_idx, d_u, d_v, d_w, d_x, d_y, d_z, d_x0, d_y0, d_z0,
               d_omega, d_omega_dot, d_vc, d_ac, d_omega0, d_vc0, d_num_body,
               dt=0.0):
        self._advance(0.5 * dt, d_idx, d_u, d_v, d_w, d_x, d_y, d_z, d_x0, d_y0, d_z0,
                      d_omega, d_omega_dot, d_vc, d_ac, d_omega0, d_vc0, d_num_body)

    def stage2(self, d_idx, d_u, d_v, d_w, d_x, d_y, d_z, d_x0, d_y0, d_z0,
               d_omega, d_omega_dot, d_vc, d_ac, d_omega0, d_vc0, d_num_body,
               dt=0.0):
        self._advance(dt, d_idx, d_u, d_v, d_w, d_x, d_y, d_z, d_x0, d_y0, d_z0,
                      d_omega, d_omega_dot, d_vc, d_ac, d_omega0, d_vc0, d_num_body)


class BodyForce(Equation):
    """the weight of every body particle: the value the coupling forces of the evaluation are added to"""

    def __init__(self, dest, sources, gx=0.0, gy=0.0, gz=0.0):
        self.gx = gx
        self.gy = gy
        self.gz = gz
        super(BodyForce, self).__init__(dest, sources)

    def initialize(self, d_idx, d_m, d_fx, d_fy, d_fz):
        mass = d_m[d_idx]
        d_fx[d_idx] = mass * self.gx
        d_fy[d_idx] = mass * self.gy
        d_fz[d_idx] = mass * self.gz


class NumberDensity(Equation):
    """``V = sum_b W_ab`` over the body particles: the inverse of the volume a body particle stands for"""

    def initialize(self, d_idx, d_V):
        d_V[d_idx] = 0.0

    def loop(self, d_idx, d_V, WIJ):
        d_V[d_idx] += WIJ


class PressureRigidBody(Equation):
    """Akinci eq. 9 / 10.  ``V`` of the body is a number density, so a body particle takes the volume ``1 / V_b``
    and stands for the fluid mass ``psi_b = rho0 / V_b``.  Destination: the fluid; sources: the bodies."""

    def __init__(self, dest, sources, rho0):
        self.rho0 = rho0
        super(PressureRigidBody, self).__init__(dest, sources)

    def loop(self, d_idx, d_m, d_rho, d_au, d_av, d_aw, d_p,
             s_idx, s_V, s_fx, s_fy, s_fz, DWIJ):
        m_i = d_m[d_idx]
        rho_i = d_rho[d_idx]
        vol_b = 1.0 / s_V[s_idx]
        # F_i<-b = -m_i psi_b (p_i / rho_i^2) grad W_ib: the force on the fluid particle, in newtons
        strength = m_i * (self.rho0 * vol_b) * d_p[d_idx] / (rho_i * rho_i)
        fx = -strength * DWIJ[0]
        fy = -strength * DWIJ[1]
        fz = -strength * DWIJ[2]
        d_au[d_idx] += fx / m_i
        d_av[d_idx] += fy / m_i
        d_aw[d_idx] += fz / m_i
        # eq. 10: the body particle takes the opposite force
        s_fx[s_idx] -= fx
        s_fy[s_idx] -= fy
        s_fz[s_idx] -= fz


class ViscosityRigidBody(Equation):
    """Akinci eqs. 11-14 with ``psi_b = rho0 / V_b``: friction acts only while the two particles approach."""

    def __init__(self, dest, sources, rho0, nu):
        self.nu = nu
        self.rho0 = rho0
        super(ViscosityRigidBody, self).__init__(dest, sources)

    def loop(self, d_idx, d_m, d_au, d_av, d_aw, d_rho,
             s_idx, s_V, s_fx, s_fy, s_fz,
             EPS, VIJ, XIJ, R2IJ, DWIJ):
        closing = VIJ[0] * XIJ[0] + VIJ[1] * XIJ[1] + VIJ[2] * XIJ[2]
        if closing >= 0.0:
            return                      # separating (or at rest): Pi_ib = 0
        m_i = d_m[d_idx]
        psi_b = self.rho0 / s_V[s_idx]
        # Pi_ib = -nu min(v_ib . x_ib, 0) / (rho_i (|x_ib|^2 + eps)),  F_i<-b = -m_i psi_b Pi_ib grad W_ib
        pi_ib = -self.nu * closing / (d_rho[d_idx] * (R2IJ + EPS))
        strength = m_i * psi_b * pi_ib
        fx = -strength * DWIJ[0]
        fy = -strength * DWIJ[1]
        fz = -strength * DWIJ[2]
        d_au[d_idx] += fx / m_i
        d_av[d_idx] += fy / m_i
        d_aw[d_idx] += fz / m_i
        s_fx[s_idx] -= fx
        s_fy[s_idx] -= fy
        s_fz[s_idx] -= fz


class AkinciRigidFluidCoupling(Equation):
    """Akinci eq. 9 / 10 in its symmetric form ``p_i / rho_i^2 + p_b / rho_b^2`` with the fluid particle's pressure
    and density mirrored onto the body particle, and ``V`` of the body read as the volume itself:
    ``psi_b = fluid_rho V_b``.  Apply it once: it gives both the fluid's acceleration and the body's force."""

    def __init__(self, dest, sources, fluid_rho=1000):
        self.fluid_rho = fluid_rho
        super(AkinciRigidFluidCoupling, self).__init__(dest, sources)

    def loop(self, d_idx, d_m, d_rho, d_au, d_av, d_aw, d_p,
             s_idx, s_V, s_fx, s_fy, s_fz, DWIJ, s_m, s_p, s_rho):
        m_i = d_m[d_idx]
        rho_i = d_rho[d_idx]
        own = d_p[d_idx] / (rho_i * rho_i)
        mirrored = own                  # p_b := p_i, rho_b := rho_i
        strength = m_i * (self.fluid_rho * s_V[s_idx]) * (own + mirrored)
        fx = -strength * DWIJ[0]
        fy = -strength * DWIJ[1]
        fz = -strength * DWIJ[2]
        d_au[d_idx] += fx / m_i
        d_av[d_idx] += fy / m_i
        d_aw[d_idx] += fz / m_i
        s_fx[s_idx] -= fx
        s_fy[s_idx] -= fy
        s_fz[s_idx] -= fz


class LiuFluidForce(Equation):
    """Liu et al.: the symmetric SPH pressure force between a fluid particle and a body particle that carries a
    mass, a pressure and a density of its own."""

    def __init__(self, dest, sources):
        super(LiuFluidForce, self).__init__(dest, sources)

    def loop(self, d_idx, d_m, d_rho, d_au, d_av, d_aw, d_p,
             s_idx, s_V, s_fx, s_fy, s_fz, DWIJ, s_m, s_p, s_rho):
        m_i = d_m[d_idx]
        rho_i = d_rho[d_idx]
        rho_b = s_rho[s_idx]
        # F_i<-b = -m_i m_b (p_i / rho_i^2 + p_b / rho_b^2) grad W_ib
        strength = m_i * s_m[s_idx] * (d_p[d_idx] / (rho_i * rho_i) + s_p[s_idx] / (rho_b * rho_b))
        fx = -strength * DWIJ[0]
        fy = -strength * DWIJ[1]
        fz = -strength * DWIJ[2]
        d_au[d_idx] += fx / m_i
        d_av[d_idx] += fy / m_i
        d_aw[d_idx] += fz / m_i
        s_fx[s_idx] -= fx
        s_fy[s_idx] -= fy
        s_fz[s_idx] -= fz
