"""Entropically damped artificial compressibility (EDAC) for the HIP backend.

Mirrors the interface of pysph/sph/wc/edac.py (Ramachandran & Puri, "Entropically
damped artificial compressibility for SPH", Computers & Fluids 179 (2019) 579):

* ``EDACScheme`` (:543-978): ``get_equations()`` gives the reference's group list
  for both branches -- external flow (``pb == 0``, :882-978) and internal flow
  with the transport velocity (``|pb| > 1e-14``, :774-880) -- in the same order,
  with the same ``real`` flags, sources and parameters;
* the fluid equations ``ComputeAveragePressure`` (:62-79), ``MomentumEquation``
  (:301-351), ``MomentumEquationPressureGradient`` (:389-488) and ``EDACEquation``
  (:354-386) are parameter holders: their bodies are the hand-written families
  ``FamEDAC_T`` / ``FamAvgP_T`` of csrc/sph_fam_tvf.h (DESIGN.md, section EDAC).
  ``MomentumEquation`` and ``MomentumEquationPressureGradient`` share their names
  with the WCSPH / TVF classes; ``equations.resolve_equation`` tells them apart by
  the module name (``'edac' in type(eq).__module__``), for these classes and for
  the reference's own;
* the wall equations ``SourceNumberDensity`` (:177-183), ``SolidWallPressureBC``
  (:136-166), ``SetWallVelocity`` (:186-233), ``ClampWallPressure`` (:169-174),
  ``NoSlipVelocityExtrapolation`` (:236-265) and
  ``NoSlipAdvVelocityExtrapolation`` (:268-298) have Python bodies that
  ``pysph_amd.codegen`` translates, like those of ``pysph_amd/wall_bc.py``.  The
  bodies are written from the formulae of Adami, Hu & Adams, J. Comput. Phys. 231
  (2012) 7057: the kernel sum ``sum_f W`` of a wall particle over the fluid, the
  Shepard mean of the fluid velocity (eq. 22) mirrored about the wall's own
  velocity (eq. 23), the wall pressure (eq. 27), and for a free-slip wall the
  Shepard mean reflected about the wall normal, ``v - 2 (v . n) n``;
* the steppers ``EDACStep`` / ``EDACTVFStep`` live in ``pysph_amd.integrator``,
  ``EDAC_PROPS`` / ``get_particle_array_edac*`` in ``pysph_amd.particle_array``.
"""
from .equations import (Equation, Group, TVFSummationDensity as SummationDensity,
                        MomentumEquationViscosity,
                        MomentumEquationArtificialViscosity,
                        MomentumEquationArtificialStress, XSPHCorrection)
from .integrator import EDACStep, EDACTVFStep, PECIntegrator
from .particle_array import (DEFAULT_PROPS, EDAC_PROPS, EDAC_SOLID_PROPS,  # noqa: F401
                             get_particle_array_edac,
                             get_particle_array_edac_solid)
from .wall_bc import VolumeSummation, SolidWallNoSlipBC


# --------------------------------------------------------------------------
# fluid equations: parameter holders of the hand-written kernels
# --------------------------------------------------------------------------
class ComputeAveragePressure(Equation):
    """wc/edac.py:62-79: ``pavg`` = mean of the neighbours' pressure, ``nnbr``
    their number (Basa, Quinlan & Lastiwka 2009)."""


class MomentumEquation(Equation):
    """wc/edac.py:301-351: number-density pressure gradient, body force behind
    the ``tdamp`` ramp."""

    def __init__(self, dest, sources, c0, gx=0.0, gy=0.0, gz=0.0, tdamp=0.0):
        self.gx = gx
        self.gy = gy
        self.gz = gz
        self.c0 = c0
        self.tdamp = tdamp
        super(MomentumEquation, self).__init__(dest, sources)


class MomentumEquationPressureGradient(Equation):
    """wc/edac.py:389-488: the TVF pressure gradient with the destination's
    average pressure taken off both pressures."""

    def __init__(self, dest, sources, pb, gx=0., gy=0., gz=0., tdamp=0.0):
        self.pb = pb
        self.gx = gx
        self.gy = gy
        self.gz = gz
        self.tdamp = tdamp
        super(MomentumEquationPressureGradient, self).__init__(dest, sources)


class EDACEquation(Equation):
    """wc/edac.py:354-386: the pressure rate ``ap``."""

    def __init__(self, dest, sources, cs, nu, rho0):
        self.cs = cs
        self.nu = nu
        self.rho0 = rho0
        super(EDACEquation, self).__init__(dest, sources)


# --------------------------------------------------------------------------
# wall equations: Python bodies for the generated-family path
# --------------------------------------------------------------------------
class SourceNumberDensity(Equation):
    """``wij = sum_f W``: the denominator of every Shepard mean below."""

    def initialize(self, d_idx, d_wij):
        d_wij[d_idx] = 0.0

    def loop(self, d_idx, d_wij, WIJ):
        d_wij[d_idx] += WIJ


class SolidWallPressureBC(Equation):
    """Adami et al. 2012, eq. 27; ``d_au, d_av, d_aw`` are the prescribed
    accelerations of the wall, ``d_wij`` comes from ``SourceNumberDensity``."""

    def __init__(self, dest, sources, gx=0.0, gy=0.0, gz=0.0):
        self.gx = gx
        self.gy = gy
        self.gz = gz
        super(SolidWallPressureBC, self).__init__(dest, sources)

    def initialize(self, d_idx, d_p):
        d_p[d_idx] = 0.0

    def loop(self, d_idx, s_idx, d_p, d_au, d_av, d_aw, s_p, s_rho, WIJ, XIJ):
        # (g - a_w) . r_wf: the hydrostatic head between fluid and wall particle
        head = (self.gx - d_au[d_idx]) * XIJ[0] + \
            (self.gy - d_av[d_idx]) * XIJ[1] + \
            (self.gz - d_aw[d_idx]) * XIJ[2]
        d_p[d_idx] += s_p[s_idx] * WIJ + s_rho[s_idx] * head * WIJ

    def post_loop(self, d_idx, d_p, d_wij):
        ksum = d_wij[d_idx]
        if ksum > 1e-14:
            d_p[d_idx] = d_p[d_idx] / ksum


class ClampWallPressure(Equation):
    """No suction at the wall: a negative wall pressure becomes zero."""

    def post_loop(self, d_idx, d_p):
        if d_p[d_idx] < 0.0:
            d_p[d_idx] = 0.0


class SetWallVelocity(Equation):
    """Adami et al. 2012, eqs. 22-23: ``uf`` the Shepard mean of the fluid
    velocity, ``ug = 2 u_wall - uf``."""

    def initialize(self, d_idx, d_uf, d_vf, d_wf):
        d_uf[d_idx] = 0.0
        d_vf[d_idx] = 0.0
        d_wf[d_idx] = 0.0

    def loop(self, d_idx, s_idx, d_uf, d_vf, d_wf, s_u, s_v, s_w, WIJ):
        d_uf[d_idx] += s_u[s_idx] * WIJ
        d_vf[d_idx] += s_v[s_idx] * WIJ
        d_wf[d_idx] += s_w[s_idx] * WIJ

    def post_loop(self, d_idx, d_uf, d_vf, d_wf, d_wij, d_u, d_v, d_w,
                  d_ug, d_vg, d_wg):
        ksum = d_wij[d_idx]
        um = d_uf[d_idx]
        vm = d_vf[d_idx]
        wm = d_wf[d_idx]
        if ksum > 1e-12:
            # a wall particle with no fluid in reach keeps a zero mean
            um = um / ksum
            vm = vm / ksum
            wm = wm / ksum
        d_uf[d_idx] = um
        d_vf[d_idx] = vm
        d_wf[d_idx] = wm
        d_ug[d_idx] = 2 * d_u[d_idx] - um
        d_vg[d_idx] = 2 * d_v[d_idx] - vm
        d_wg[d_idx] = 2 * d_w[d_idx] - wm


class NoSlipVelocityExtrapolation(Equation):
    """Free-slip (inviscid) wall: the Shepard mean of the fluid velocity with
    its wall-normal part reversed, written into the wall's own ``u, v, w``;
    ``xn, yn, zn`` is the unit normal."""

    def initialize(self, d_idx, d_u, d_v, d_w):
        d_u[d_idx] = 0.0
        d_v[d_idx] = 0.0
        d_w[d_idx] = 0.0

    def loop(self, d_idx, s_idx, d_u, d_v, d_w, s_u, s_v, s_w, WIJ):
        d_u[d_idx] += s_u[s_idx] * WIJ
        d_v[d_idx] += s_v[s_idx] * WIJ
        d_w[d_idx] += s_w[s_idx] * WIJ

    def post_loop(self, d_idx, d_wij, d_u, d_v, d_w, d_xn, d_yn, d_zn):
        ksum = d_wij[d_idx]
        um = d_u[d_idx]
        vm = d_v[d_idx]
        wm = d_w[d_idx]
        if ksum > 1e-14:
            um = um / ksum
            vm = vm / ksum
            wm = wm / ksum
        vn = um * d_xn[d_idx] + vm * d_yn[d_idx] + wm * d_zn[d_idx]
        d_u[d_idx] = um - 2 * vn * d_xn[d_idx]
        d_v[d_idx] = vm - 2 * vn * d_yn[d_idx]
        d_w[d_idx] = wm - 2 * vn * d_zn[d_idx]


class NoSlipAdvVelocityExtrapolation(Equation):
    """The same for the transport (advection) velocity ``uhat, vhat, what``."""

    def initialize(self, d_idx, d_uhat, d_vhat, d_what):
        d_uhat[d_idx] = 0.0
        d_vhat[d_idx] = 0.0
        d_what[d_idx] = 0.0

    def loop(self, d_idx, s_idx, d_uhat, d_vhat, d_what, s_uhat, s_vhat, s_what,
             WIJ):
        d_uhat[d_idx] += s_uhat[s_idx] * WIJ
        d_vhat[d_idx] += s_vhat[s_idx] * WIJ
        d_what[d_idx] += s_what[s_idx] * WIJ

    def post_loop(self, d_idx, d_wij, d_uhat, d_vhat, d_what, d_xn, d_yn, d_zn):
        ksum = d_wij[d_idx]
        um = d_uhat[d_idx]
        vm = d_vhat[d_idx]
        wm = d_what[d_idx]
        if ksum > 1e-14:
            um = um / ksum
            vm = vm / ksum
            wm = wm / ksum
        vn = um * d_xn[d_idx] + vm * d_yn[d_idx] + wm * d_zn[d_idx]
        d_uhat[d_idx] = um - 2 * vn * d_xn[d_idx]
        d_vhat[d_idx] = vm - 2 * vn * d_yn[d_idx]
        d_what[d_idx] = wm - 2 * vn * d_zn[d_idx]


# --------------------------------------------------------------------------
# the scheme
# --------------------------------------------------------------------------
TVF_FLUID_PROPS = ('uhat', 'vhat', 'what', 'ap', 'auhat', 'avhat', 'awhat', 'V',
                   'p0', 'u0', 'v0', 'w0', 'x0', 'y0', 'z0', 'pavg', 'nnbr')
TVF_SOLID_PROPS = ('V', 'wij', 'ax', 'ay', 'az', 'uf', 'vf', 'wf', 'ug', 'vg', 'wg')
INVISCID_SOLID_PROPS = ('xn', 'yn', 'zn', 'uhat', 'vhat', 'what')


class EDACScheme(object):
    """wc/edac.py:543-978."""

    def __init__(self, fluids, solids, dim, c0, nu, rho0, pb=0.0, gx=0.0,
                 gy=0.0, gz=0.0, tdamp=0.0, eps=0.0, h=0.0, edac_alpha=0.5,
                 alpha=0.0, bql=True, clamp_p=False, inlet_outlet_manager=None,
                 inviscid_solids=None):
        self.c0 = c0
        self.nu = nu
        self.rho0 = rho0
        self.gx = gx
        self.gy = gy
        self.gz = gz
        self.tdamp = tdamp
        self.dim = dim
        self.eps = eps
        self.fluids = list(fluids)
        self.solids = list(solids)
        self.pb = pb
        self.solver = None
        self.integrator = None
        self.kernel = None
        self.bql = bql
        self.clamp_p = clamp_p
        self.edac_alpha = edac_alpha
        self.alpha = alpha
        self.h = h
        self.inlet_outlet_manager = inlet_outlet_manager
        self.inviscid_solids = [] if inviscid_solids is None else list(inviscid_solids)
        self.attributes_changed()

    # -- public protocol ---------------------------------------------------
    def attributes_changed(self):
        """:647-651."""
        if self.pb is not None:
            self.use_tvf = abs(self.pb) > 1e-14
        if self.h is not None and self.c0 is not None:
            self.art_nu = self.edac_alpha * self.h * self.c0 / 8

    def configure(self, **kw):
        for k, v in kw.items():
            if not hasattr(self, k):
                raise RuntimeError('Parameter %s not defined for %s.' % (k, type(self).__name__))
            setattr(self, k, v)
        self.attributes_changed()

    def get_timestep(self, cfl=0.25):
        """the acoustic and the viscous limit of the explicit steppers"""
        dt = cfl * self.h / self.c0
        nu = max(self.nu, self._get_edac_nu())
        if nu > 0.0:
            dt = min(dt, 0.125 * self.h * self.h / nu)
        return dt

    def get_stepper_class(self):
        return EDACTVFStep if self.use_tvf else EDACStep

    def configure_solver(self, kernel=None, integrator_cls=None,
                         extra_steppers=None, **kw):
        """:653-703: the kernel (QuinticSpline by default), one
        ``EDACTVFStep`` / ``EDACStep`` per fluid by the branch, the inlet/outlet
        manager's steppers, a PEC integrator unless another class is given.
        The integrator is kept in ``self.integrator`` (this package has no
        ``Solver``; ``integrator.setup_integrator`` installs it)."""
        from .kernels import QuinticSpline
        if kernel is None:
            kernel = QuinticSpline(dim=self.dim)
        steppers = {}
        if extra_steppers is not None:
            steppers.update(extra_steppers)
        step_cls = self.get_stepper_class()
        cls = integrator_cls if integrator_cls is not None else PECIntegrator
        for fluid in self.fluids:
            if fluid not in steppers:
                steppers[fluid] = step_cls()
        iom = self.inlet_outlet_manager
        if iom is not None:
            iom_stepper = iom.get_stepper(self, cls, self.use_tvf)
            for name in iom_stepper:
                steppers[name] = iom_stepper[name]
        self.kernel = kernel
        self.integrator = cls(**steppers)
        self.solver_args = dict(kw)
        if iom is not None:
            iom.setup_iom(dim=self.dim, kernel=kernel)
        return self.integrator

    def get_equations(self):
        if self.use_tvf:
            return self._get_internal_flow_equations()
        return self._get_external_flow_equations()

    def setup_properties(self, particles, clean=True):
        """:714-762 (properties are added; none is removed)."""
        arrays = dict((pa.name, pa) for pa in particles)
        extra = TVF_FLUID_PROPS if self.use_tvf else EDAC_PROPS
        iom = self.inlet_outlet_manager
        fluids_with_io = self.fluids
        if iom is not None:
            fluids_with_io = self.fluids + list(iom.get_io_names(ghost=True))
        for fluid in fluids_with_io:
            pa = arrays[fluid]
            _ensure(pa, tuple(DEFAULT_PROPS) + tuple(extra))
            pa.set_output_arrays(['x', 'y', 'z', 'u', 'v', 'w', 'rho', 'p', 'm', 'h', 'V']
                                 + (['pavg'] if 'pavg' in pa.properties else []))
            if iom is not None:
                iom.add_io_properties(pa, self)
        solid_props = tuple(TVF_SOLID_PROPS)
        if self.inviscid_solids:
            solid_props += INVISCID_SOLID_PROPS
        extra = solid_props if self.use_tvf else EDAC_SOLID_PROPS
        if not self.use_tvf and self.inviscid_solids:
            extra = tuple(extra) + ('xn', 'yn', 'zn')      # the normals NoSlipVelocityExtrapolation reads
        for solid in self.solids + self.inviscid_solids:
            pa = arrays[solid]
            _ensure(pa, tuple(DEFAULT_PROPS) + tuple(extra))
            pa.set_output_arrays(['x', 'y', 'z', 'u', 'v', 'w', 'rho', 'p', 'm', 'h', 'V'])

    # -- private protocol --------------------------------------------------
    def _get_edac_nu(self):
        """:765-772, without the printing."""
        return self.art_nu if self.art_nu > 0 else self.nu

    def _wall_group(self, fluids_with_io, everyone, internal):
        eqs = []
        for solid in self.solids:
            eqs.extend([
                SourceNumberDensity(dest=solid, sources=fluids_with_io),
                VolumeSummation(dest=solid, sources=everyone),
                SolidWallPressureBC(dest=solid, sources=fluids_with_io,
                                    gx=self.gx, gy=self.gy, gz=self.gz),
                SetWallVelocity(dest=solid, sources=fluids_with_io),
            ])
            if not internal and self.clamp_p:
                eqs.append(ClampWallPressure(dest=solid, sources=None))
        for solid in self.inviscid_solids:
            eqs.append(SourceNumberDensity(dest=solid, sources=fluids_with_io))
            eqs.append(NoSlipVelocityExtrapolation(dest=solid, sources=fluids_with_io))
            if internal:
                eqs.append(NoSlipAdvVelocityExtrapolation(dest=solid, sources=fluids_with_io))
            eqs.append(VolumeSummation(dest=solid, sources=everyone))
            eqs.append(SolidWallPressureBC(dest=solid, sources=fluids_with_io,
                                           gx=self.gx, gy=self.gy, gz=self.gz))
        return eqs

    def _viscous_terms(self, fluid, fluids_with_io):
        eqs = []
        if self.alpha > 0.0:
            eqs.append(MomentumEquationArtificialViscosity(
                dest=fluid, sources=fluids_with_io + self.solids, alpha=self.alpha, c0=self.c0))
        if self.nu > 0.0:
            eqs.append(MomentumEquationViscosity(dest=fluid, sources=fluids_with_io, nu=self.nu))
        if len(self.solids) > 0 and self.nu > 0.0:
            eqs.append(SolidWallNoSlipBC(dest=fluid, sources=self.solids, nu=self.nu))
        return eqs

    def _io(self):
        iom = self.inlet_outlet_manager
        fluids_with_io = self.fluids
        all_solids = self.solids + self.inviscid_solids
        if iom is not None:
            fluids_with_io = self.fluids + list(iom.get_io_names())
        return iom, fluids_with_io, all_solids, fluids_with_io + all_solids

    def _get_internal_flow_equations(self):
        """:774-880."""
        edac_nu = self._get_edac_nu()
        iom, fluids_with_io, all_solids, everyone = self._io()
        equations = []
        if iom is not None:
            equations.extend(iom.get_equations(self, self.use_tvf))
        group1, avg_p_group = [], []
        has_solids = len(all_solids) > 0
        for fluid in fluids_with_io:
            group1.append(SummationDensity(dest=fluid, sources=everyone))
            if self.bql:
                eq = ComputeAveragePressure(dest=fluid, sources=everyone)
                (avg_p_group if has_solids else group1).append(eq)
        group1.extend(self._wall_group(fluids_with_io, everyone, True))
        equations.append(Group(equations=group1, real=False))
        # the average pressure AFTER the wall pressure is set
        if self.bql and has_solids:
            equations.append(Group(equations=avg_p_group, real=True))
        group2 = []
        for fluid in self.fluids:
            group2.append(MomentumEquationPressureGradient(
                dest=fluid, sources=everyone, pb=self.pb, gx=self.gx, gy=self.gy, gz=self.gz,
                tdamp=self.tdamp))
            group2.extend(self._viscous_terms(fluid, fluids_with_io))
            group2.extend([
                MomentumEquationArtificialStress(dest=fluid, sources=fluids_with_io),
                EDACEquation(dest=fluid, sources=everyone, nu=edac_nu, cs=self.c0, rho0=self.rho0),
            ])
        equations.append(Group(equations=group2))
        if iom is not None:
            equations.extend(iom.get_equations_post_compute_acceleration())
        return equations

    def _get_external_flow_equations(self):
        """:882-978."""
        iom, fluids_with_io, all_solids, everyone = self._io()
        edac_nu = self._get_edac_nu()
        equations = []
        if iom is not None:
            equations.extend(iom.get_equations(self, self.use_tvf))
        group1 = [SummationDensity(dest=fluid, sources=everyone) for fluid in fluids_with_io]
        group1.extend(self._wall_group(fluids_with_io, everyone, False))
        equations.append(Group(equations=group1, real=False))
        group2 = []
        for fluid in self.fluids:
            group2.append(MomentumEquation(
                dest=fluid, sources=everyone, gx=self.gx, gy=self.gy, gz=self.gz, c0=self.c0,
                tdamp=self.tdamp))
            group2.extend(self._viscous_terms(fluid, fluids_with_io))
            group2.extend([
                EDACEquation(dest=fluid, sources=everyone, nu=edac_nu, cs=self.c0, rho0=self.rho0),
                XSPHCorrection(dest=fluid, sources=[fluid], eps=self.eps),
            ])
        equations.append(Group(equations=group2))
        if iom is not None:
            equations.extend(iom.get_equations_post_compute_acceleration())
        return equations


def _ensure(pa, props):
    for p in props:
        if p not in pa.properties:
            pa.add_property(p)
