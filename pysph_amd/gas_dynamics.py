"""Compressible gas dynamics for the HIP backend.

Mirrors the interface of pysph/sph/gas_dynamics/basic.py and ``GasDScheme`` of pysph/sph/scheme.py:884-1141
(Sod tubes, blast waves, Sedov, Kelvin-Helmholtz):

* the equation classes ``SummationDensity`` (basic.py:74-219), ``IdealGasEOS`` (:222-230), ``MPMAccelerations``
  (:356-483), ``ScaleSmoothingLength`` (:13-19) and ``UpdateSmoothingLengthFromVolume`` (:22-29) are parameter
  holders with the reference's constructor signatures and defaults: their bodies are the hand-written families
  ``FamGasSD_T`` / ``FamMPM_T`` (csrc/sph_fam_gas.h) and three cases of ``k_nosrc`` in csrc/sph_eval.hip.
  ``SummationDensity`` is the third class of that name next to basic_equations' and transport_velocity's;
  ``equations.resolve_equation`` finds it by the module name (``'gas_dynamics' in type(eq).__module__``), for this
  class and for the reference's own;
* ``SummationDensity(density_iterations=True)`` under ``Group(update_nnps=True, iterate=True)`` solves the smoothing
  length of every particle by Newton-Raphson, one neighbour update and one sweep per iteration.  The sweep leaves one
  device word, which the evaluator turns into ``equation_has_converged`` (-1 / 1) behind every launch: ``converged()``
  is what the iterated group asks, as in the reference;
* ``MPMUpdateGhostProps`` (:486-497), which ``GasDScheme(has_ghosts=True)`` puts in a ``real=False`` group, copies
  ``p`` and ``cs`` of every row behind the real ones from the row ``orig_idx`` names.  ``orig_idx`` gets a device
  column when the evaluator is set up; the periodic / mirror images of ``HipDomainManager`` are copies of their rows,
  so they carry the right value, and every domain update hands them the current ``h, rho, omega, alpha*, e``;
* ``GasDScheme`` gives the reference's group list for ``adaptive_h_scheme='mpm'`` and ``'gsph'``; ``solids`` are
  refused at construction (running the reference's ``WallBoundary`` through the translator was not attempted);
* ``GasDFluidStep`` lives in ``pysph_amd.integrator``, ``get_particle_array_gasd`` in ``pysph_amd.particle_array``.

Godunov SPH (pysph/sph/gas_dynamics/gsph.py, riemann_solver.py, ``GSPHScheme`` of scheme.py:1144-1458; DESIGN.md,
section 7h):

* ``GSPHGradients`` (gsph.py:61-101), ``GSPHUpdateGhostProps`` (:104-145) and ``GSPHAcceleration`` (:148-541) are
  parameter holders too: ``FamGSPHGrad_T``, a case of ``k_nosrc`` and ``FamGSPH_T``.  The force sweep holds the eleven
  Riemann solvers; which one runs, the limiter, the interpolation, ``hybrid`` and the conduction switch are launch
  parameters.  A pair whose solve fails where the reference's returns 1 without a result enters with
  ``pstar = ustar = 0`` and is counted: ``eq.solver_failures()`` of a ``GSPHAcceleration`` the evaluator has compiled
  reads the count of the last evaluation from the device (nothing is read unless it is called);
* the images of a periodic / mirror domain get what ``GSPHAcceleration`` reads from them -- the twelve gradients,
  ``grhox..z``, ``dwdh``, ``rho``, ``div``, ``p``, ``cs`` -- from ``GSPHUpdateGhostProps``, the ghost kernel, right
  before the force group (``has_ghosts=True``), not from the domain update.  The reference's list has that group only
  behind ``GSPHGradients``, which then sums over images whose ``p`` and ``rho`` date from the last domain update; the
  evaluator runs the ghost group in front of the gradient group as well, so that a periodic box equals its explicit
  tiling -- a deliberate difference from the reference, for arrays with images only (the group list is the reference's);
* ``GSPHScheme`` gives the reference's group list (including that it does not hand ``tf`` to ``GSPHAcceleration``);
  ``configure_solver`` takes ``tf`` from its keywords as the reference's does.  ``GSPHStep`` lives in
  ``pysph_amd.integrator``.

ADKE (gas_dynamics/basic.py:32-71, :274-353, :500-512, boundary_equations.py, ``ADKEScheme`` of scheme.py:1461-1644;
DESIGN.md, section 7i):

* ``SummationDensityADKE``, ``ADKEAccelerations``, ``ADKEUpdateGhostProps`` and ``WallBoundary`` are parameter holders:
  ``FamADKESD_T``, ``FamADKE_T``, a case of ``k_nosrc`` and ``FamGasWall_T``.  The ``reduce`` hook of
  ``SummationDensityADKE`` is replaced by a device reduction in a fixed order and one element-wise launch behind the
  sweep: no value crosses to the host.  ``ADKEAccelerations`` drops the ``g2`` it is given, as the reference does;
* ``ADKEScheme`` gives the reference's group list, ``solids`` included (``GasDScheme`` and ``GSPHScheme`` still refuse
  them).  ``ADKEStep`` lives in ``pysph_amd.integrator``.
"""
import numpy as np

from .equations import Equation, Group
from .integrator import ADKEStep, EulerIntegrator, GasDFluidStep, GSPHStep, PECIntegrator
from .particle_array import GASD_PROPS, get_npy, get_particle_array_gasd  # noqa: F401


class ScaleSmoothingLength(Equation):
    """gas_dynamics/basic.py:13-19: ``h *= factor``."""

    def __init__(self, dest, sources, factor=2.0):
        super(ScaleSmoothingLength, self).__init__(dest, sources)
        self.factor = factor


class UpdateSmoothingLengthFromVolume(Equation):
    """gas_dynamics/basic.py:22-29: ``h = k (m / rho)^(1 / dim)``."""

    def __init__(self, dest, sources, dim, k=1.2):
        super(UpdateSmoothingLengthFromVolume, self).__init__(dest, sources)
        self.k = k
        self.dim1 = 1. / dim


class SummationDensity(Equation):
    """gas_dynamics/basic.py:74-219: density, its rate, its gradient and dW/dh with the destination's own h, and
    with ``density_iterations`` one Newton-Raphson step for h per evaluation of the group."""

    def __init__(self, dest, sources, dim, density_iterations=False,
                 iterate_only_once=False, k=1.2, htol=1e-6):
        self.density_iterations = density_iterations
        self.iterate_only_once = iterate_only_once
        self.dim = dim
        self.k = k
        self.htol = htol
        # 1: converged; the evaluator writes -1 behind a sweep that left a particle unconverged
        self.equation_has_converged = 1
        super(SummationDensity, self).__init__(dest, sources)

    def converged(self):
        return self.equation_has_converged


class IdealGasEOS(Equation):
    """gas_dynamics/basic.py:222-230: ``p = (gamma - 1) rho e``, ``cs = sqrt(gamma p / rho)``."""

    def __init__(self, dest, sources, gamma):
        self.gamma = gamma
        self.gamma1 = gamma - 1.0
        super(IdealGasEOS, self).__init__(dest, sources)


class MPMAccelerations(Equation):
    """gas_dynamics/basic.py:356-483: grad-h momentum and energy rates with artificial viscosity, artificial
    conduction and the sources of the two switches."""

    def __init__(self, dest, sources, beta=2.0, update_alpha1=False,
                 update_alpha2=False, alpha1_min=0.1, alpha2_min=0.1,
                 sigma=0.1):
        self.beta = beta
        self.sigma = sigma
        self.update_alpha1 = update_alpha1
        self.update_alpha2 = update_alpha2
        self.alpha1_min = alpha1_min
        self.alpha2_min = alpha2_min
        super(MPMAccelerations, self).__init__(dest, sources)


class MPMUpdateGhostProps(Equation):
    """gas_dynamics/basic.py:486-497: ``p`` and ``cs`` of an image row from the row it mirrors (``orig_idx``)."""

    def __init__(self, dest, sources=None, dim=2):
        super(MPMUpdateGhostProps, self).__init__(dest, sources)
        self.dim = dim


class GasDScheme(object):
    """scheme.py:884-1141."""

    def __init__(self, fluids, solids, dim, gamma, kernel_factor, alpha1=1.0,
                 alpha2=0.1, beta=2.0, adaptive_h_scheme='mpm',
                 update_alpha1=False, update_alpha2=False,
                 max_density_iterations=250,
                 density_iteration_tolerance=1e-3, has_ghosts=False):
        if list(solids):
            raise NotImplementedError(
                'GasDScheme(solids=%r): the WallBoundary equation of gas_dynamics/boundary_equations.py has '
                'not been run through this backend (not attempted); stale wall values are not computed with' % (list(solids),))
        if adaptive_h_scheme not in ('mpm', 'gsph'):
            raise ValueError("adaptive_h_scheme must be 'mpm' or 'gsph', not %r" % (adaptive_h_scheme,))
        self.fluids = list(fluids)
        self.solids = list(solids)
        self.dim = dim
        self.solver = None
        self.integrator = None
        self.kernel = None
        self.gamma = gamma
        self.alpha1 = alpha1
        self.alpha2 = alpha2
        self.update_alpha1 = update_alpha1
        self.update_alpha2 = update_alpha2
        self.beta = beta
        self.kernel_factor = kernel_factor
        self.adaptive_h_scheme = adaptive_h_scheme
        self.density_iteration_tolerance = density_iteration_tolerance
        self.max_density_iterations = max_density_iterations
        self.has_ghosts = has_ghosts

    def configure(self, **kw):
        for k, v in kw.items():
            if not hasattr(self, k):
                raise RuntimeError('Parameter %s not defined for %s.' % (k, type(self).__name__))
            setattr(self, k, v)

    def get_stepper_class(self):
        return GasDFluidStep

    def configure_solver(self, kernel=None, integrator_cls=None,
                         extra_steppers=None, **kw):
        """:985-1024: the kernel (Gaussian by default), one ``GasDFluidStep`` per fluid, a PEC integrator unless
        another class is given.  The integrator is kept in ``self.integrator`` (this package has no ``Solver``;
        ``integrator.setup_integrator`` installs it)."""
        from .kernels import Gaussian
        if kernel is None:
            kernel = Gaussian(dim=self.dim)
        steppers = {}
        if extra_steppers is not None:
            steppers.update(extra_steppers)
        cls = integrator_cls if integrator_cls is not None else PECIntegrator
        step_cls = self.get_stepper_class()
        for name in self.fluids:
            if name not in steppers:
                steppers[name] = step_cls()
        self.kernel = kernel
        self.integrator = cls(**steppers)
        self.solver_args = dict(kw)
        return self.integrator

    def get_integrator(self):
        if self.integrator is None:
            self.configure_solver()
        return self.integrator

    def get_equations(self):
        """:1026-1120."""
        equations = []
        if self.adaptive_h_scheme == 'mpm':
            g1 = [SummationDensity(dest=fluid, sources=self.fluids, k=self.kernel_factor,
                                   density_iterations=True, dim=self.dim,
                                   htol=self.density_iteration_tolerance) for fluid in self.fluids]
            equations.append(Group(equations=g1, update_nnps=True, iterate=True,
                                   max_iterations=self.max_density_iterations))
        else:
            equations.append(Group(
                equations=[ScaleSmoothingLength(dest=fluid, sources=None, factor=2.0) for fluid in self.fluids],
                update_nnps=True))
            equations.append(Group(
                equations=[SummationDensity(dest=fluid, sources=self.fluids, dim=self.dim) for fluid in self.fluids],
                update_nnps=False))
            equations.append(Group(
                equations=[UpdateSmoothingLengthFromVolume(dest=fluid, sources=None, k=self.kernel_factor,
                                                           dim=self.dim) for fluid in self.fluids],
                update_nnps=True))
            equations.append(Group(
                equations=[SummationDensity(dest=fluid, sources=self.fluids, dim=self.dim) for fluid in self.fluids],
                update_nnps=False))
        equations.append(Group(equations=[IdealGasEOS(dest=fluid, sources=None, gamma=self.gamma)
                                          for fluid in self.fluids]))
        equations.append(Group(equations=[]))          # the (empty) wall group of the reference's list
        if self.has_ghosts:
            equations.append(Group(equations=[MPMUpdateGhostProps(dest=fluid, sources=None) for fluid in self.fluids],
                                   real=False))
        equations.append(Group(equations=[
            MPMAccelerations(dest=fluid, sources=self.fluids + self.solids, alpha1_min=self.alpha1,
                             alpha2_min=self.alpha2, beta=self.beta, update_alpha1=self.update_alpha1,
                             update_alpha2=self.update_alpha2) for fluid in self.fluids]))
        return equations

    def setup_properties(self, particles, clean=True):
        """:1122-1141 (properties are added; none is removed)."""
        arrays = dict((pa.name, pa) for pa in particles)
        for fluid in self.fluids:
            pa = arrays[fluid]
            for p in GASD_PROPS:
                if p not in pa.properties:
                    pa.add_property(p)
            if 'orig_idx' not in pa.properties:
                pa.add_property('orig_idx', type='int')
            get_npy(pa, 'orig_idx')[:] = np.arange(pa.get_number_of_particles())
            pa.set_output_arrays(['x', 'y', 'u', 'v', 'rho', 'm', 'h', 'cs', 'p', 'e', 'au', 'av', 'ae', 'pid', 'gid',
                                  'tag', 'dwdh', 'alpha1', 'alpha2'])


# Riemann solver types, interpolation types (gsph.py:11-27)
NonDiffusive, VanLeer, Exact, HLLC, Ducowicz, HLLE, Roe, LLXF, HLLCBall, HLLBall, HLLSY = range(11)
Delta, Linear, Cubic = range(3)
GSPH_GRADIENT_PROPS = ('px', 'py', 'pz', 'ux', 'uy', 'uz', 'vx', 'vy', 'vz', 'wx', 'wy', 'wz')


class GSPHGradients(Equation):
    """gsph.py:61-101: the gradients of ``p, u, v, w`` with ``DWI``: twelve sums, one sweep."""


class GSPHUpdateGhostProps(Equation):
    """gsph.py:104-145: the twenty columns ``GSPHAcceleration`` reads from an image row, from the row it mirrors
    (``orig_idx``)."""

    def __init__(self, dest, sources=None):
        super(GSPHUpdateGhostProps, self).__init__(dest, sources)


class GSPHAcceleration(Equation):
    """gsph.py:148-541: Inutsuka's GSPH accelerations with the monotonicity constraints of I02 / IwIn, the
    specific-volume interpolations and the Riemann solvers of riemann_solver.py."""

    def __init__(self, dest, sources, g1=0.0, g2=0.0,
                 monotonicity=0, rsolver=Exact,
                 interpolation=Linear, interface_zero=True, hybrid=False,
                 blend_alpha=5.0, tf=1.0,
                 gamma=1.4, niter=20, tol=1e-6):
        self.gamma = gamma
        self.niter = niter
        self.tol = tol
        self.g1 = g1
        self.g2 = g2
        self.monotonicity = monotonicity
        self.interpolation = interpolation
        self.rsolver = rsolver
        self.sstar = 0.0
        if (g1 == 0 and g2 == 0):
            self.thermal_conduction = 0
        else:
            self.thermal_conduction = 1
        self.interface_zero = interface_zero
        self.hybrid = hybrid
        self.blend_alpha = blend_alpha
        self.tf = tf
        super(GSPHAcceleration, self).__init__(dest, sources)

    def solver_failures(self):
        """Pairs of the last evaluation whose Riemann solve failed; the evaluator that compiles this equation
        replaces the method with one that reads the device word."""
        return 0


class GSPHScheme(object):
    """scheme.py:1144-1458."""

    def __init__(self, fluids, solids, dim, gamma, kernel_factor, g1=0.0,
                 g2=0.0, rsolver=2, interpolation=1, monotonicity=1,
                 interface_zero=True, hybrid=False, blend_alpha=5.0, tf=1.0,
                 niter=20, tol=1e-6, has_ghosts=False):
        if list(solids):
            raise NotImplementedError(
                'GSPHScheme(solids=%r): the WallBoundary equation of gas_dynamics/boundary_equations.py has '
                'not been run through this backend (not attempted); stale wall values are not computed with' % (list(solids),))
        self.fluids = list(fluids)
        self.solids = list(solids)
        self.dim = dim
        self.solver = None
        self.integrator = None
        self.kernel = None
        self.gamma = gamma
        self.kernel_factor = kernel_factor
        self.g1 = g1
        self.g2 = g2
        self.rsolver = rsolver
        self.interpolation = interpolation
        self.monotonicity = monotonicity
        self.interface_zero = interface_zero
        self.hybrid = hybrid
        self.blend_alpha = blend_alpha
        self.tf = tf
        self.niter = niter
        self.tol = tol
        self.has_ghosts = has_ghosts
        self.rsolver_choices = {'non_diffusive': 0,
                                'van_leer': 1,
                                'exact': 2,
                                'hllc': 3,
                                'ducowicz': 4,
                                'hlle': 5,
                                'roe': 6,
                                'llxf': 7,
                                'hllc_ball': 8,
                                'hll_ball': 9,
                                'hllsy': 10}
        self.interpolation_choices = {'delta': 0,
                                      'linear': 1,
                                      'cubic': 2}
        self.monotonicity_choices = {'first_order': 0,
                                     'i02': 1,
                                     'iwin': 2}

    def configure(self, **kw):
        for k, v in kw.items():
            if not hasattr(self, k):
                raise RuntimeError('Parameter %s not defined for %s.' % (k, type(self).__name__))
            setattr(self, k, v)

    def configure_solver(self, kernel=None, integrator_cls=None,
                         extra_steppers=None, **kw):
        """:1294-1335: the kernel (Gaussian by default), one ``GSPHStep`` per fluid, an Euler integrator unless
        another class is given; ``tf`` of the keywords becomes the scheme's.  The integrator is kept in
        ``self.integrator`` (this package has no ``Solver``; ``integrator.setup_integrator`` installs it)."""
        from .kernels import Gaussian
        if kernel is None:
            kernel = Gaussian(dim=self.dim)
        steppers = {}
        if extra_steppers is not None:
            steppers.update(extra_steppers)
        cls = integrator_cls if integrator_cls is not None else EulerIntegrator
        for name in self.fluids:
            if name not in steppers:
                steppers[name] = GSPHStep()
        self.kernel = kernel
        self.integrator = cls(**steppers)
        self.solver_args = dict(kw)
        if 'tf' in kw:
            self.tf = kw['tf']
        return self.integrator

    def get_integrator(self):
        if self.integrator is None:
            self.configure_solver()
        return self.integrator

    def get_equations(self):
        """:1337-1435 (the wall groups exist with ``solids`` only, which are refused)."""
        all_pa = self.fluids + self.solids
        equations = []
        equations.append(Group(
            equations=[ScaleSmoothingLength(dest=fluid, sources=None, factor=2.0) for fluid in self.fluids],
            update_nnps=True))
        equations.append(Group(
            equations=[SummationDensity(dest=fluid, sources=all_pa, dim=self.dim) for fluid in self.fluids],
            update_nnps=False))
        equations.append(Group(
            equations=[UpdateSmoothingLengthFromVolume(dest=fluid, sources=None, k=self.kernel_factor,
                                                       dim=self.dim) for fluid in self.fluids],
            update_nnps=True))
        equations.append(Group(
            equations=[SummationDensity(dest=fluid, sources=all_pa, dim=self.dim) for fluid in self.fluids],
            update_nnps=False))
        equations.append(Group(equations=[IdealGasEOS(dest=fluid, sources=None, gamma=self.gamma)
                                          for fluid in self.fluids]))
        equations.append(Group(equations=[GSPHGradients(dest=fluid, sources=all_pa) for fluid in self.fluids]))
        if self.has_ghosts:
            equations.append(Group(equations=[GSPHUpdateGhostProps(dest=fluid, sources=None) for fluid in self.fluids],
                                   update_nnps=False, real=False))
        equations.append(Group(equations=[
            GSPHAcceleration(dest=fluid, sources=all_pa, g1=self.g1, g2=self.g2, monotonicity=self.monotonicity,
                             rsolver=self.rsolver, interpolation=self.interpolation,
                             interface_zero=self.interface_zero, hybrid=self.hybrid, blend_alpha=self.blend_alpha,
                             gamma=self.gamma, niter=self.niter, tol=self.tol) for fluid in self.fluids]))
        return equations

    def setup_properties(self, particles, clean=True):
        """:1437-1458 (properties are added; none is removed)."""
        arrays = dict((pa.name, pa) for pa in particles)
        for fluid in self.fluids:
            pa = arrays[fluid]
            for p in GASD_PROPS + GSPH_GRADIENT_PROPS:
                if p not in pa.properties:
                    pa.add_property(p)
            if 'orig_idx' not in pa.properties:
                pa.add_property('orig_idx', type='int')
            get_npy(pa, 'orig_idx')[:] = np.arange(pa.get_number_of_particles())
            pa.set_output_arrays(['x', 'y', 'u', 'v', 'rho', 'm', 'h', 'cs', 'p', 'e', 'au', 'av', 'ae', 'pid', 'gid',
                                  'tag', 'dwdh', 'alpha1', 'alpha2'])


# -- ADKE (pysph/sph/gas_dynamics/basic.py:32-71, :274-353, :500-512; boundary_equations.py; scheme.py:1461-1644) -------
ADKE_PROPS = ('x', 'y', 'z', 'u', 'v', 'w', 'rho', 'h', 'm', 'cs', 'p', 'e', 'au', 'av', 'aw', 'arho', 'ae', 'am', 'ah',
              'x0', 'y0', 'z0', 'u0', 'v0', 'w0', 'rho0', 'e0', 'h0', 'div', 'wij', 'htmp', 'logrho')


class SummationDensityADKE(Equation):
    """gas_dynamics/basic.py:32-71: the pilot density with ``h = h0``, ``div`` and ``logrho``; the ``reduce`` of the
    reference -- ``h = k (exp(mean logrho) / rho)^eps h0`` over every row -- runs on the device behind the sweep, so
    this holder has no ``reduce`` method (a reference object's is not called either)."""

    def __init__(self, dest, sources, k=1.0, eps=0.0):
        self.k = k
        self.eps = eps
        super(SummationDensityADKE, self).__init__(dest, sources)


class ADKEAccelerations(Equation):
    """gas_dynamics/basic.py:274-353.  As the reference's constructor does (:287-288), ``g2`` becomes ``g1``: the value
    given for ``g2`` is dropped."""

    def __init__(self, dest, sources, alpha, beta, g1, g2, k, eps):
        self.alpha = alpha
        self.g1 = g1
        self.g2 = g1
        self.alpha = alpha
        self.beta = beta
        self.k = k
        self.eps = eps
        super(ADKEAccelerations, self).__init__(dest, sources)


class ADKEUpdateGhostProps(Equation):
    """gas_dynamics/basic.py:500-512: ``p``, ``cs`` and ``rho`` of an image row from the row it mirrors."""

    def __init__(self, dest, sources=None, dim=2):
        super(ADKEUpdateGhostProps, self).__init__(dest, sources)
        self.dim = dim


class WallBoundary(Equation):
    """gas_dynamics/boundary_equations.py:5-48: a wall row takes the kernel average of the fluid's
    ``p, -u, -v, -w, m, rho, e, cs, div, h`` at its own ``h0``; a row no fluid particle reaches keeps the raw (zero)
    sums and ``h = h0``."""


class ADKEScheme(object):
    """scheme.py:1461-1644."""

    def __init__(self, fluids, solids, dim, gamma=1.4, alpha=1.0, beta=2.0,
                 k=1.0, eps=0.0, g1=0, g2=0, has_ghosts=False):
        self.fluids = list(fluids)
        self.solids = list(solids)
        self.dim = dim
        self.solver = None
        self.integrator = None
        self.kernel = None
        self.gamma = gamma
        self.alpha = alpha
        self.beta = beta
        self.k = k
        self.eps = eps
        self.g1 = g1
        self.g2 = g2
        self.has_ghosts = has_ghosts

    def configure(self, **kw):
        for k, v in kw.items():
            if not hasattr(self, k):
                raise RuntimeError('Parameter %s not defined for %s.' % (k, type(self).__name__))
            setattr(self, k, v)

    def get_equations(self):
        """:1504-1572, group for group."""
        from .equations import SummationDensity as BasicSummationDensity
        all_pa = self.fluids + self.solids
        equations = []

        def wall_group():
            return Group(equations=[WallBoundary(solid, sources=self.fluids) for solid in self.solids])
        if self.solids:
            equations.append(wall_group())
        equations.append(Group(
            equations=[SummationDensityADKE(fluid, sources=all_pa, k=self.k, eps=self.eps) for fluid in self.fluids],
            update_nnps=False, iterate=False))
        if self.solids:
            equations.append(wall_group())
        equations.append(Group(equations=[BasicSummationDensity(fluid, all_pa) for fluid in self.fluids],
                               update_nnps=True))
        if self.solids:
            equations.append(wall_group())
        equations.append(Group(equations=[IdealGasEOS(elem, sources=None, gamma=self.gamma) for elem in all_pa]))
        if self.has_ghosts:
            equations.append(Group(equations=[ADKEUpdateGhostProps(dest=fluid, sources=None) for fluid in self.fluids],
                                   real=False))
        equations.append(Group(equations=[
            ADKEAccelerations(dest=fluid, sources=all_pa, alpha=self.alpha, beta=self.beta, g1=self.g1, g2=self.g2,
                              k=self.k, eps=self.eps) for fluid in self.fluids]))
        return equations

    def configure_solver(self, kernel=None, integrator_cls=None,
                         extra_steppers=None, **kw):
        """:1574-1612: the kernel (Gaussian by default), one ``ADKEStep`` per fluid, a PEC integrator unless another
        class is given.  The integrator is kept in ``self.integrator`` (this package has no ``Solver``;
        ``integrator.setup_integrator`` installs it)."""
        from .kernels import Gaussian
        if kernel is None:
            kernel = Gaussian(dim=self.dim)
        steppers = {}
        if extra_steppers is not None:
            steppers.update(extra_steppers)
        cls = integrator_cls if integrator_cls is not None else PECIntegrator
        for name in self.fluids:
            if name not in steppers:
                steppers[name] = ADKEStep()
        self.kernel = kernel
        self.integrator = cls(**steppers)
        self.solver_args = dict(kw)
        return self.integrator

    def get_integrator(self):
        if self.integrator is None:
            self.configure_solver()
        return self.integrator

    def setup_properties(self, particles, clean=True):
        """:1614-1644 (properties are added; none is removed)."""
        arrays = dict((pa.name, pa) for pa in particles)
        out = ['x', 'y', 'u', 'v', 'rho', 'm', 'h', 'cs', 'p', 'e', 'au', 'av', 'ae', 'pid', 'gid', 'tag']
        for name in self.solids + self.fluids:
            pa = arrays[name]
            for p in ADKE_PROPS:
                if p not in pa.properties:
                    pa.add_property(p)
            pa.set_output_arrays(out)
        for fluid in self.fluids:
            pa = arrays[fluid]
            if 'orig_idx' not in pa.properties:
                pa.add_property('orig_idx', type='int')
            get_npy(pa, 'orig_idx')[:] = np.arange(pa.get_number_of_particles())
