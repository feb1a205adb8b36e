"""Open boundaries that stay on the device: inlets and outlets.

The surface of the reference's ``pysph/sph/bc/inlet_outlet_manager.py``
(``InletInfo`` / ``OutletInfo`` :13-64, ``InletOutletManager`` :67-346,
``IOEvaluate`` :349-406, ``InletStep`` / ``OutletStep`` /
``OutletStepWithUhat`` :469-494, ``InletBase`` :497-621, ``OutletBase``
:624-743), written against that surface for the HIP backend.

What differs is where the structural step runs.  The reference classifies
the particles with an ``IOEvaluate`` evaluator, pulls ``ioid`` to the host,
builds index lists with numpy and moves whole rows through host particle
arrays.  Here ``update`` asks the device for the class of every row
(``pa.gpu.classify_plane``: the fused form of ``IOEvaluate``), moves the rows
between the device arrays (``transfer_selected`` / ``shift_selected`` /
``remove_selected``) and reads ONE small table of counts per update; no
property value crosses PCIe in either direction.  The arrays must be
device-attached (``pysph_amd.device.attach``) and the run device-resident
(``sync='manual'``): the host arrays keep the right LENGTH, their float
values are stale until ``pa.gpu.sync_host()``.

Ordering contract.  Rows appended to a destination arrive in ascending index
of their source array.  Removal is STABLE: the rows that stay keep their
order, as this package's ``pa.gpu.remove_particles`` does.  The reference's
``ParticleArray.remove_particles`` fills the holes with rows from the end, so
results agree with the reference as SETS of particles and with this package's
host path row for row.

Arrays that carry device ghosts behind their real rows (a slab halo, a device
domain manager: ``pa.gpu.ghost_owner``) are refused with an error: open
boundaries on decomposed or periodic arrays are not supported.

Wiring into a run set up with ``setup_integrator``::

    ios = manager.get_inlet_outlet(arrays_by_name)
    integrator.set_post_stage_callback(
        lambda t, dt, stage: [io.update(t, dt, stage) for io in ios])
"""
import numpy as np

from . import device as dev
from .equations import Equation
from .integrator import IntegratorStep
from .particle_array import get_particle_array


class InletInfo(object):
    """What is known of one inlet before the particles exist (:13-50): the
    array's name, the interface plane (a point on it and its normal, pointing
    out of the fluid), whether a mirrored ghost array goes with it, the class
    that performs the update, optional equations, a velocity scale and the
    properties an update copies.  ``length`` and ``dx`` are filled in by the
    manager once the particles are there."""

    def __init__(self, pa_name, normal, refpoint, has_ghost=True, update_cls=None,
                 equations=None, umax=1.0, props_to_copy=None):
        self.pa_name = pa_name
        self.normal = normal
        self.refpoint = refpoint
        self.has_ghost = has_ghost
        self.update_cls = update_cls if update_cls is not None else InletBase
        self.equations = list(equations) if equations is not None else []
        self.umax = umax
        self.props_to_copy = props_to_copy
        self.length = 0.0
        self.dx = 0.1


class OutletInfo(InletInfo):
    """The same record for an outlet (:53-64): no ghost by default, updated by
    ``OutletBase``."""

    def __init__(self, pa_name, normal, refpoint, has_ghost=False, update_cls=None,
                 equations=None, umax=1.0, props_to_copy=None):
        super(OutletInfo, self).__init__(pa_name, normal, refpoint, has_ghost, update_cls,
                                         equations, umax, props_to_copy)
        if update_cls is None:
            self.update_cls = OutletBase


class InletOutletManager(object):
    """Book-keeping of the inlets and outlets of a problem (:67-346): names,
    ghost pairing, sizes, and the ``InletBase`` / ``OutletBase`` objects."""

    def __init__(self, fluid_arrays, inletinfo, outletinfo, extraeqns=None):
        self.fluids = fluid_arrays
        self.inletinfo = list(inletinfo) if inletinfo is not None else []
        self.outletinfo = list(outletinfo) if outletinfo is not None else []
        self.inlets = [info.pa_name for info in self.inletinfo]
        self.outlets = [info.pa_name for info in self.outletinfo]
        self.extraeqns = dict(extraeqns) if extraeqns is not None else {}
        self.dim = None
        self.kernel = None
        self.active_stages = []
        self.inlet_pairs, self.outlet_pairs = {}, {}
        self.ghost_inlets, self.ghost_outlets = [], []
        self._create_ghost_names()

    def _create_ghost_names(self):
        for infos, pairs, names in ((self.inletinfo, self.inlet_pairs, self.ghost_inlets),
                                    (self.outletinfo, self.outlet_pairs, self.ghost_outlets)):
            for info in infos:
                if info.has_ghost:
                    pairs[info.pa_name] = 'ghost_' + info.pa_name
                    names.append(pairs[info.pa_name])

    def _info_of(self, name, inlet):
        for info in (self.inletinfo if inlet else self.outletinfo):
            if info.pa_name == name:
                return info
        return None

    def create_ghost(self, pa_arr, inlet=True):
        """The mirror image of an inlet / outlet array about its interface
        plane, as a particle array named ``ghost_<name>`` (None when the info
        asks for no ghost).  Row i of the ghost is the image of row i."""
        info = self._info_of(pa_arr.name, inlet)
        if info is not None and not info.has_ghost:
            return None
        ref = info.refpoint if info is not None else (0.0, 0.0, 0.0)
        nrm = info.normal if info is not None else (0.0, 0.0, 0.0)
        dist = ((pa_arr.x - ref[0]) * nrm[0] + (pa_arr.y - ref[1]) * nrm[1] +
                (pa_arr.z - ref[2]) * nrm[2])
        pairs = self.inlet_pairs if inlet else self.outlet_pairs
        return get_particle_array(
            name=pairs[pa_arr.name], x=pa_arr.x - 2.0 * dist * nrm[0],
            y=pa_arr.y - 2.0 * dist * nrm[1], z=pa_arr.z - 2.0 * dist * nrm[2],
            m=pa_arr.m, h=pa_arr.h, u=pa_arr.u, rho=pa_arr.rho, p=0.0)

    def update_dx(self, dx):
        for info in self.inletinfo + self.outletinfo:
            info.dx = dx

    def _update_inlet_outlet_info(self, pa):
        """``length`` of the inlet / outlet `pa`: its extent along the normal,
        half a spacing added on either side (host values: call it before the
        run goes device-resident)."""
        for info in self.inletinfo + self.outletinfo:
            if info.pa_name != pa.name or pa.get_number_of_particles() == 0:
                continue            # (an array that starts empty keeps the length it was given)
            ext = [(np.max(c) + 0.5 * info.dx) - (np.min(c) - 0.5 * info.dx)
                   for c in (pa.x, pa.y, pa.z)]
            info.length = abs(sum(e * n for e, n in zip(ext, info.normal)))

    # hooks a scheme-specific manager overrides
    def add_io_properties(self, pa, scheme=None):
        pass

    def get_stepper(self, scheme, integrator, **kw):
        raise NotImplementedError()

    def setup_iom(self, dim, kernel):
        self.dim = dim
        self.kernel = kernel

    def get_equations(self, scheme, **kw):
        return []

    def get_equations_post_compute_acceleration(self):
        return []

    def get_io_names(self, ghost=False):
        names = self.inlets + self.outlets
        return names + self.ghost_inlets + self.ghost_outlets if ghost else names

    def get_inlet_outlet(self, particle_array):
        """One update object per inlet and per outlet; `particle_array` maps
        names to arrays."""
        out = []
        for infos, pairs in ((self.inletinfo, self.inlet_pairs), (self.outletinfo, self.outlet_pairs)):
            for info in infos:
                pa = particle_array[info.pa_name]
                self._update_inlet_outlet_info(pa)
                ghost = particle_array[pairs[info.pa_name]] if info.pa_name in pairs else None
                obj = None
                for fluid in self.fluids:
                    obj = info.update_cls(pa, particle_array[fluid], info, self.kernel, self.dim,
                                          self.active_stages, ghost_pa=ghost)
                out.append(obj)
        return out


class IOEvaluate(Equation):
    """``ioid`` of every particle of `dest` from its signed distance ``disp``
    to the interface plane through (x, y, z) with outward normal (xn, yn, zn):
    0 on the fluid side, 1 inside the inlet / outlet (up to `maxdist` deep), 2
    beyond it (:349-406).  Python bodies: runs as a generated family.
    ``pa.gpu.classify_plane`` is the same arithmetic fused with the count of
    each class.  A particle within rounding of a threshold must get the same
    class from both, so neither may depend on which multiply-adds a compiler
    chooses to fuse: the body is generated with contraction off
    (``_fp_contract_``), the fused kernel is compiled the same way, and disp is
    the plain left-to-right binary64 expression on both sides."""
    _fp_contract_ = False

    def __init__(self, dest, sources, x, y, z, xn, yn, zn, maxdist=1000.0):
        self.x, self.y, self.z = x, y, z
        self.xn, self.yn, self.zn = xn, yn, zn
        self.maxdist = maxdist
        super(IOEvaluate, self).__init__(dest, sources)

    def loop(self, d_idx, d_x, d_y, d_z, d_ioid, d_disp):
        dist = (d_x[d_idx] - self.x) * self.xn + (d_y[d_idx] - self.y) * self.yn + \
            (d_z[d_idx] - self.z) * self.zn
        beyond = dist - self.maxdist
        d_disp[d_idx] = dist
        if dist > 1e-6 and beyond < 1e-6:
            d_ioid[d_idx] = 1.0
        elif beyond > 1e-6:
            d_ioid[d_idx] = 2.0
        else:
            d_ioid[d_idx] = 0.0


class InletStep(IntegratorStep):
    """Inlet particles are carried along x with their own velocity (:469-478);
    the stage bodies run as generated stage families."""

    def initialize(self, d_idx, d_x0, d_x):
        d_x0[d_idx] = d_x[d_idx]

    def stage1(self, d_idx, d_x, d_x0, d_u, dt):
        d_x[d_idx] = d_x0[d_idx] + 0.5 * dt * d_u[d_idx]

    def stage2(self, d_idx, d_x, d_x0, d_u, dt):
        d_x[d_idx] = d_x0[d_idx] + dt * d_u[d_idx]


class OutletStep(InletStep):
    """:493-494."""


class OutletStepWithUhat(IntegratorStep):
    """Outlet particles carried by the transport velocity (:481-490)."""

    def initialize(self, d_idx, d_x0, d_x):
        d_x0[d_idx] = d_x[d_idx]

    def stage1(self, d_idx, d_x, d_x0, d_uhat, dt):
        d_x[d_idx] = d_x0[d_idx] + 0.5 * dt * d_uhat[d_idx]

    def stage2(self, d_idx, d_x, d_x0, d_uhat, dt):
        d_x[d_idx] = d_x0[d_idx] + dt * d_uhat[d_idx]


def _device(pa, who):
    gpu = getattr(pa, 'gpu', None)
    if not isinstance(gpu, dev.HipDeviceHelper):
        raise RuntimeError("%s: particle array '%s' has no device mirror (pysph_amd.device.attach); "
                           "open boundaries run on device-attached arrays only" % (who, pa.name))
    return gpu


def _wants_ioid(gpu):
    """does the array hold ioid or disp on the device (classifying it only to
    write them is skipped otherwise)"""
    have = set(gpu.device_props())
    return dev.prop_id('ioid') in have or dev.prop_id('disp') in have


class _IOBase(object):
    def _setup(self, info, kernel, dim, active_stages, callback):
        self.kernel = kernel
        self.dim = dim
        self.callback = callback
        self.active_stages = active_stages
        self.x = self.y = self.z = 0.0
        self.xn = self.yn = self.zn = 0.0
        self.length = 0.0
        self.dx = 0.0
        self.io_eval = None          # (the reference's evaluator: classify_plane takes its place)
        self.gpu = True
        self._init = False
        self._info = info
        self.last_counts = None      # what the last active update read from the device

    def initialize(self):
        """take the plane and the length from the info object (the manager
        fills them in after the particles were created)"""
        info = self._info
        self.x, self.y, self.z = info.refpoint[0], info.refpoint[1], info.refpoint[2]
        self.xn, self.yn, self.zn = info.normal[0], info.normal[1], info.normal[2]
        self.length = info.length
        self.dx = info.dx

    def _active(self, stage):
        if not self._init:
            self.initialize()
            self._init = True
        return stage in self.active_stages


class InletBase(_IOBase):
    """Feeds `dest_pa` from `inlet_pa` (:497-621).  After an active stage every
    inlet particle that crossed the interface (ioid 0) is COPIED to the end of
    the destination, in ascending inlet index, with every property the two
    arrays share; the original wraps back by ``length`` along the normal to the
    inlet's far end, and row i of the index-aligned ghost array moves by the
    opposite vector.  ``callback(dest_pa, inlet_pa)`` follows every active
    update.  All of it on the device; see the module docstring."""

    def __init__(self, inlet_pa, dest_pa, inletinfo, kernel, dim, active_stages=[1],
                 callback=None, ghost_pa=None):
        self.inlet_pa = inlet_pa
        self.dest_pa = dest_pa
        self.ghost_pa = ghost_pa
        self.inletinfo = inletinfo
        self._setup(inletinfo, kernel, dim, active_stages, callback)

    def update(self, time, dt, stage):
        if not self._active(stage):
            return
        g_in = _device(self.inlet_pa, 'InletBase.update')
        g_dst = _device(self.dest_pa, 'InletBase.update')
        g_ghost = _device(self.ghost_pa, 'InletBase.update') if self.ghost_pa is not None else None
        ref, nrm = (self.x, self.y, self.z), (self.xn, self.yn, self.zn)
        g_in.classify_plane(ref, nrm, maxdist=self.length, read=False)
        if _wants_ioid(g_dst):       # the reference's evaluator leaves ioid / disp on the fluid too
            g_dst.classify_plane(ref, nrm, read=False)
        counts, = dev.HipDeviceHelper.read_io_counts(g_in)
        self.last_counts = counts
        if counts[0]:
            g_in.transfer_selected(g_dst, 0, props=None, keep=True)
            shift = (self.length * self.xn, self.length * self.yn, self.length * self.zn)
            g_in.shift_selected(0, shift[0], shift[1], shift[2])
            if g_ghost is not None:
                g_ghost.shift_selected(0, -shift[0], -shift[1], -shift[2], flags=g_in)
        if self.callback is not None:
            self.callback(self.dest_pa, self.inlet_pa)


class OutletBase(_IOBase):
    """Drains `source_pa` into `outlet_pa` (:624-743).  After an active stage
    the source particles inside the outlet (ioid 1) MOVE to the end of the
    outlet array -- the properties of ``outletinfo.props_to_copy`` travel
    (None: all shared ones), every other outlet property reads 0 on the new
    rows -- and then the outlet particles that were beyond its far end (ioid 2)
    are deleted.  Both removals are stable.  ``callback(source_pa, outlet_pa)``
    follows every active update."""

    def __init__(self, outlet_pa, source_pa, outletinfo, kernel, dim, active_stages=[1],
                 callback=None, ghost_pa=None):
        self.outlet_pa = outlet_pa
        self.source_pa = source_pa
        self.ghost_pa = ghost_pa
        self.outletinfo = outletinfo
        self.props_to_copy = None
        self._setup(outletinfo, kernel, dim, active_stages, callback)

    def initialize(self):
        super(OutletBase, self).initialize()
        self.props_to_copy = self.outletinfo.props_to_copy

    def update(self, time, dt, stage):
        if not self._active(stage):
            return
        g_out = _device(self.outlet_pa, 'OutletBase.update')
        g_src = _device(self.source_pa, 'OutletBase.update')
        ref, nrm = (self.x, self.y, self.z), (self.xn, self.yn, self.zn)
        g_out.classify_plane(ref, nrm, maxdist=self.length, read=False)
        g_src.classify_plane(ref, nrm, read=False)
        c_out, c_src = dev.HipDeviceHelper.read_io_counts(g_out, g_src)
        self.last_counts = (c_out, c_src)
        if c_src[1]:
            g_src.transfer_selected(g_out, 1, props=self.props_to_copy, keep=False)
        if c_out[2]:
            g_out.remove_selected(2)
        if self.callback is not None:
            self.callback(self.source_pa, self.outlet_pa)
