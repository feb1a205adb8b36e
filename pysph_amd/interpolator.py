"""``Interpolator``: particle fields onto a uniform grid or a given set of
points, the reference's post-processing tool
(pysph/tools/interpolator.py:225-511) on the HIP backend.

Same constructor arguments, methods and attributes (``interpolate``,
``update``, ``update_particle_arrays``, ``set_domain``,
``set_interpolation_points``, ``METHODS``, ``x y z shape pa nnps``) and the
module functions ``get_bounding_box`` / ``get_nx_ny_nz``.  The interpolation
itself is ``sph_interpolate`` of the C-ABI (csrc/sph_interp.h): one neighbour
sweep of the pair kernel carries ``WIDTH`` = 4 properties, the sources stay on
the device, and the moment matrices of ``'order1'`` are kept until the next
``update()``.

New here:

* ``interpolate_many(props, comp=0, pull=True)``: a list of arrays from
  ceil(len(props) / 4) sweeps; ``interpolate(prop)`` is its one-property case.
  With ``pull=False`` nothing comes back to the host: the results stay on the
  device as properties of ``self.pa`` named ``ip0, ip1, ...`` (user property
  slots, of which a process has 128 -- ``pull=True`` takes none) -- property k of
  the list is ``ip<k>``, for ``'order1'`` its value and gradient are
  ``ip<4k> .. ip<4k+3>`` -- and their names are returned.
* ``ctx=`` shares a ``HipContext`` with a running simulation.  ``sync=True``
  (the drop-in behaviour) pushes x, y, z, h, m, rho and the requested
  properties of the sources from the host before each use; ``sync=False`` reads
  what is on the device and never touches the sources' host arrays.  A context
  holds ONE neighbour grid: in a shared context every ``interpolate`` call
  rebuilds the interpolator's grid first and invalidates it afterwards (option
  ``invalidate_nnps``), so that an evaluation of the simulation that forgot its
  own neighbour update fails instead of using this grid (attribute
  ``invalidate``; False keeps the grid between calls).
* ``equations=`` is not supported (``NotImplementedError``): ``SPHEvaluator``
  runs arbitrary equations onto a destination array.

Deliberate deviations from the reference:

1. ``'order1'`` leaves the sources' ``rho`` untouched (the reference overwrites
   it with the summation density it computes first); the summation density
   lives in a private device buffer.
2. Every accumulator is zeroed on every call (the reference's ``initialize`` of
   the first-order equation zeroes three of the four ``p_sph`` components, so
   its second call accumulates into the fourth).

With ``sync=True`` the positions, h and (for ``'order1'``, whose moment
matrices are all that reads it) m are pushed by ``update()``, as the
reference's neighbour search sees moved particles only after ``update()``; the
requested properties -- and m, rho for the methods that weight with m / rho --
are pushed by every ``interpolate`` call.
"""
import ctypes as C

import numpy as np

from . import device as dev
from .kernels import Gaussian, kernel_id
from .particle_array import get_npy, get_particle_array

WIDTH = 4      # properties per neighbour sweep (INTERP_W of csrc/sph_interp.h)
_METHOD_IDS = {'shepard': 0, 'sph': 1, 'order1': 2, 'splash': 3, 'splash_norm': 4}


def get_bounding_box(particle_arrays, tight=False, stretch=0.05):
    """(xmin, xmax, ymin, ymax, zmin, zmax) over a sequence of particle arrays;
    unless `tight`, every axis is widened on both sides by `stretch` times its
    length (interpolator.py:175-202)."""
    lo = np.full(3, 1e20)
    hi = np.full(3, -1e20)
    for pa in particle_arrays:
        for k, name in enumerate('xyz'):
            v = get_npy(pa, name)
            lo[k] = min(lo[k], v.min())
            hi[k] = max(hi[k], v.max())
    return _stretched(lo, hi, tight, stretch)


def _stretched(lo, hi, tight, stretch):
    bounds = np.empty(6)
    bounds[0::2] = lo
    bounds[1::2] = hi
    if not tight:
        pad = stretch * (bounds[1::2] - bounds[0::2])
        bounds[0::2] -= pad
        bounds[1::2] += pad
    return bounds


def get_nx_ny_nz(num_points, bounds):
    """Points per axis of a uniform mesh with about `num_points` points in
    `bounds`: the spacing is the one at which the axes that count as dimensions
    (longer than 1e-3 of the summed lengths) hold `num_points` cells; an axis
    shorter than 1e-4 of the summed lengths gets a single point
    (interpolator.py:205-222)."""
    b = np.asarray(bounds, dtype=float).reshape(3, 2)
    length = b[:, 1] - b[:, 0]
    share = length / length.sum()
    extent = length[share > 1e-3]
    spacing = pow(np.prod(extent) / num_points, 1.0 / extent.size)
    return np.array([int(round(ln / spacing)) if sh > 1e-4 else 1 for ln, sh in zip(length, share)], dtype=int)


class Interpolator(object):
    METHODS = ['shepard', 'sph', 'order1', 'splash', 'splash_norm']

    def __init__(self, particle_arrays, num_points=125000, kernel=None,
                 x=None, y=None, z=None, domain_manager=None,
                 equations=None, method='shepard', ctx=None, sync=True):
        # argument checks first: none of them needs a device
        if equations is not None:
            raise NotImplementedError(
                'pysph_amd Interpolator: custom equations are not supported; '
                'pysph_amd.tools.SPHEvaluator runs arbitrary equations onto a destination array')
        if method not in self.METHODS:
            raise RuntimeError('%s method is not implemented' % (method))
        particle_arrays = list(particle_arrays)
        if len(particle_arrays) > dev.MAX_ARRAYS - 1:
            raise ValueError('Interpolator: at most %d source arrays (SPH_MAX_ARRAYS - 1), got %d'
                             % (dev.MAX_ARRAYS - 1, len(particle_arrays)))
        self.method = method
        self.equations = None
        self.sync = bool(sync)
        self.domain_manager = domain_manager
        # a context holds ONE neighbour grid: after interpolating in a shared context invalidate it (set False when nothing
        # else evaluates on the context between two calls: repeated calls then reuse this object's grid and moments)
        self.invalidate = ctx is not None
        self._own_ctx = ctx is None
        self.ctx = ctx if ctx is not None else dev.HipContext(0)
        self.pa = None
        self.nnps = None
        self._mine = None           # the context's neighbour-update number this object's grid belongs to
        self._set_particle_arrays(particle_arrays)
        bounds = self._bounding_box()
        shape = get_nx_ny_nz(num_points, bounds)
        self.dim = 3 - list(shape).count(1)
        self.kernel = Gaussian(dim=self.dim) if kernel is None else kernel
        self._ck = dev.SphKernel(kernel_id(self.kernel), int(self.kernel.dim), float(self.kernel.fac),
                                 float(self.kernel.radius_scale), float(self.kernel.get_deltap()))
        if x is None and y is None and z is None:
            self.set_domain(bounds, shape)
        else:
            self.set_interpolation_points(x=x, y=y, z=z)

    # -- Interpolator protocol -------------------------------------------
    def set_interpolation_points(self, x=None, y=None, z=None):
        """The points to interpolate onto; a coordinate that is not given is 0."""
        given = [t for t in (x, y, z) if t is not None]
        if not given:
            raise RuntimeError('At least one non-None array must be given.')
        first = np.asarray(given[0])
        x, y, z = [np.asarray(t, dtype=float) if t is not None else np.zeros(first.shape) for t in (x, y, z)]
        self.shape = x.shape
        self.x, self.y, self.z = x.squeeze(), y.squeeze(), z.squeeze()
        xr = x.ravel()
        hmax = self._max_h()
        if self.pa is not None and self.pa.get_number_of_particles() != xr.size:
            helper = dev.attach(self.pa, self.ctx)
            helper.managed = False
            self.pa.resize(xr.size)
            self.pa.set_num_real_particles(xr.size)
        if self.pa is None:
            self.pa = get_particle_array(name='interpolate', x=xr, y=y.ravel(), z=z.ravel(), h=hmax * np.ones_like(xr))
        else:
            self.pa.x[:] = xr
            self.pa.y[:] = y.ravel()
            self.pa.z[:] = z.ravel()
            self.pa.h[:] = hmax
        self._npoints = xr.size
        self.update_particle_arrays(self.particle_arrays)

    def set_domain(self, bounds, shape):
        """A uniform mesh of `shape` = (nx, ny, nz) points in `bounds` =
        (xmin, xmax, ymin, ymax, zmin, zmax)."""
        self.bounds = np.asarray(bounds)
        self.shape = np.asarray(shape)
        b, n = self.bounds, self.shape
        x, y, z = np.mgrid[b[0]:b[1]:n[0] * 1j, b[2]:b[3]:n[1] * 1j, b[4]:b[5]:n[2] * 1j]
        self.set_interpolation_points(x, y, z)

    def interpolate(self, prop, comp=0):
        """Property `prop` at the points, shaped like them; `comp` 1..3: a
        component of its gradient ('order1' only)."""
        return self.interpolate_many([prop], comp=comp)[0]

    def interpolate_many(self, props, comp=0, pull=True):
        """The properties of `props` at the points in ceil(len / 4) neighbour
        sweeps (plus, for 'order1', the moment pass after an `update()`).
        pull=True: a list of arrays shaped like the points (component `comp`).
        pull=False: the results stay on the device as properties of `self.pa`;
        returns their names -- one per property, or for 'order1' a tuple of
        four (value, d/dx, d/dy, d/dz)."""
        props = list(props)
        order1 = self.method == 'order1'
        if not isinstance(comp, (int, np.integer)) or not 0 <= comp <= 3:
            raise RuntimeError('comp must be one of 0 (value), 1, 2, 3 (d/dx, d/dy, d/dz), got %r' % (comp,))
        if comp and not order1:
            raise RuntimeError("a gradient component needs method 'order1' (this interpolator uses %r)" % self.method)
        if not props:
            return []
        lib, ctx = self.ctx.lib, self.ctx
        need_update = self._add_image_props(props)
        if self.sync:
            # ('order1' reads m through its moment matrices only: pushed with the geometry by update())
            vol = ('m', 'rho') if self.method in ('sph', 'splash', 'splash_norm') else ()
            geometry = ('x', 'y', 'z', 'h', 'm') if order1 else ('x', 'y', 'z', 'h')    # as of the last update()
            for pa, h in zip(self.particle_arrays, self._helpers):
                names = [p for p in vol + tuple(props) if p in pa.properties and p not in geometry]
                if names:
                    h.push(*names)
            # device-made periodic images are copies taken by the last update: they do not carry what was just pushed
            need_update = need_update or isinstance(self.domain_manager, _device_domain_type())
        if need_update or self._mine is None or getattr(ctx, '_nnps_updates', None) != self._mine:
            self.update()
        pids = [dev.prop_id(p) if dev.prop_id(p) >= 0 else dev.prop_register(p) for p in props]
        nout = 4 if order1 else 1
        names = ['ip%d' % k for k in range(len(props) * nout)]
        src = (C.c_int * len(self._helpers))(*[h.array_id for h in self._helpers])
        if pull:
            # no destination property per result (user property slots are a small process-wide table): the library
            # keeps the results in a block of its own and copies them out
            host = np.empty((len(props) * nout, self._npoints))
            outs, hp, npull = None, host.ctypes.data_as(dev._PD), self._npoints
        else:
            outs, hp, npull = (C.c_int * len(names))(*[dev.prop_register(n) for n in names]), None, 0
        dev._check(lib.sph_interpolate(ctx._h, C.byref(self._ck), _METHOD_IDS[self.method], self._ph.array_id,
                                       len(self._helpers), src, len(pids), (C.c_int * len(pids))(*pids),
                                       outs, hp, npull))
        if self.invalidate:
            # one grid per context: the simulation's next evaluation must rebuild its own
            ctx.set_option('invalidate_nnps', 1)
            self._mine = None
        if not pull:
            return [tuple(names[4 * k:4 * k + 4]) for k in range(len(props))] if order1 else names
        return [host[nout * k + comp].copy().reshape(self.shape).squeeze() for k in range(len(props))]

    def update(self, update_domain=True):
        """The particles moved (same arrays): rebuild the neighbour structure
        (and, with `update_domain`, the periodic images)."""
        self._push_geometry()
        if update_domain:
            self.nnps.update_domain()
            if self.domain_manager is not None:
                self._push_geometry()       # a host domain manager changed the arrays' lengths
        self.nnps.update()
        self._mine = self.ctx._nnps_updates

    def update_particle_arrays(self, particle_arrays):
        """A new set of particle arrays with the same properties."""
        self._set_particle_arrays(list(particle_arrays))
        from .nnps import HipNNPS
        arrays = self.particle_arrays + [self.pa]
        self._helpers = [dev.attach(pa, self.ctx) for pa in self.particle_arrays]
        self._ph = dev.attach(self.pa, self.ctx)
        self._push_geometry()
        # (this object pushes what `sync` asks for itself: the points are always host-owned, the sources may not be)
        self.nnps = HipNNPS(dim=self.kernel.dim, particles=arrays, radius_scale=self.kernel.radius_scale,
                            domain=self.domain_manager, cache=True, ctx=self.ctx, sync=False)
        if self.domain_manager is not None:
            self._push_geometry()
            self.nnps.update()
        self._mine = self.ctx._nnps_updates

    def close(self):
        """Release the context this object created (one that was passed in
        as ``ctx=`` belongs to its owner and is left alone).  Also the exit of
        ``with Interpolator(...) as interp:``."""
        if self._own_ctx and self.ctx is not None:
            self.ctx.close()
        self.ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- private -----------------------------------------------------------
    def _set_particle_arrays(self, particle_arrays):
        if len(particle_arrays) > dev.MAX_ARRAYS - 1:
            raise ValueError('Interpolator: at most %d source arrays (SPH_MAX_ARRAYS - 1), got %d'
                             % (dev.MAX_ARRAYS - 1, len(particle_arrays)))
        self.particle_arrays = particle_arrays

    def _push_geometry(self):
        if self.sync:
            names = ('x', 'y', 'z', 'h', 'm') if self.method == 'order1' else ('x', 'y', 'z', 'h')
            for pa in self.particle_arrays:
                dev.attach(pa, self.ctx).push(*[p for p in names if p in pa.properties])
        if self.pa is not None:
            dev.attach(self.pa, self.ctx).push('x', 'y', 'z', 'h')

    def _device_minmax(self):
        helpers = [dev.attach(pa, self.ctx) for pa in self.particle_arrays]
        ids = (C.c_int * len(helpers))(*[h.array_id for h in helpers])
        out = (C.c_double * 8)()
        dev._check(self.ctx.lib.sph_nnps_minmax(self.ctx._h, len(helpers), ids, out))
        return np.array(out[0:4]), np.array(out[4:8])

    def _bounding_box(self):
        if self.sync:
            return get_bounding_box(self.particle_arrays)
        lo, hi = self._device_minmax()      # the host arrays of a device-resident simulation are stale
        return _stretched(lo[:3], hi[:3], False, 0.05)

    def _max_h(self):
        if self.sync:
            return max([-1.0] + [float(get_npy(pa, 'h').max()) for pa in self.particle_arrays
                                 if pa.get_number_of_particles()])
        return float(self._device_minmax()[1][3])

    def _add_image_props(self, props):
        """a domain manager that restricts the properties its images carry must carry what is read here"""
        dm = self.domain_manager
        if dm is None or getattr(dm, 'image_props', None) is None:
            return False
        changed = False
        want = set(('x', 'y', 'z', 'h', 'm', 'rho')) | set(props)
        for pa in self.particle_arrays:
            have = set(dm.image_props.get(pa.name, ()))
            if pa.name in dm.image_props and not want <= have:
                dm.image_props[pa.name] = sorted(have | want)
                changed = True
        return changed


def _device_domain_type():
    from .domain import HipDomainManager
    return HipDomainManager
