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

The moments, the motion and the collisions of the bodies are not part of this
module.
"""
from .equations import Equation


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
