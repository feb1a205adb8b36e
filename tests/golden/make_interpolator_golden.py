#!/usr/bin/env python
"""Generate tests/golden/interpolator.npz from the REFERENCE's interpolator.

Run in the build container only (needs /root/reference; a couple of minutes):

    python tests/golden/make_interpolator_golden.py

The equation classes of ``pysph.tools.interpolator`` (and ``SummationDensity``,
``gj_solve``) are the reference's own code, executed as plain Python through
``oracle/ref_driver.py`` like the cases of ``make_golden.py``; the equation
lists are those ``Interpolator._compile_acceleration_eval`` builds, and one
property is interpolated per evaluation as ``Interpolator.interpolate`` does
(``temp_prop`` <- the property, 0.0 where an array lacks it).  The expected
outputs of 'order1' follow this project's two stated deviations: the
summation density feeds V_j without being judged as an output, and every
accumulator starts from zero for every property.

Case c6 is an addition to the issue's list.

Stored: the source arrays and points of every case, the expected values per
method and field (4 per point for 'order1': value, gradient), and recorded
outputs of ``get_bounding_box`` / ``get_nx_ny_nz``.

Asserted here, so that the tests need no exclusions: the neighbour search
equals brute force, and in every 'order1' case a point either has no neighbour
at all or every pivot of the elimination has magnitude >= 1e-3.

The 1-D case uses CubicSpline: the reference's WendlandQuintic (like this
project's) does not exist in one dimension.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

from oracle.ref_driver import (REFERENCE, setup_reference_imports, ListPA,  # noqa: E402
                               PyLinkedListNNPS, RefEval)

HAVE_REFERENCE = os.path.isdir(REFERENCE)
OUT = os.path.join(HERE, 'interpolator.npz')
SUM_METHODS = ('shepard', 'sph', 'splash', 'splash_norm')


def _declare(kind, n=1):
    """stand-in for compyle's ``declare`` when the bodies run as plain Python"""
    if kind.startswith('matrix'):
        return [0.0] * int(kind[kind.index('(') + 1:kind.index(')')])
    return 0 if n == 1 else (0,) * n


def import_reference():
    """pysph.tools.interpolator with stand-ins for the modules that need the
    compiled parts of the reference"""
    setup_reference_imports()

    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    for name, attrs in (('pysph.base.utils', dict(get_particle_array=None)),
                        ('pysph.base.nnps', dict(LinkedListNNPS=None)),
                        ('pysph.sph.sph_compiler', dict(SPHCompiler=None))):
        if name not in sys.modules:
            try:
                __import__(name)
            except Exception:
                mod(name, **attrs)
    import pysph.sph.wc.linalg as linalg
    import pysph.tools.interpolator as ri
    linalg.declare = _declare
    ri.declare = _declare
    return ri


def field_values(k, x, y, z):
    """smooth, non-trivial fields; every one depends on x and on y also where z (or y and z) vanish, so that no
    gradient component inside the case's dimension is identically zero"""
    return [1 + np.sin(3 * x) - 2 * y ** 2 + x * z,
            np.cos(2 * x + y) + 0.5 * z,
            x * y - z ** 2 + 0.3 + 0.5 * x,
            np.exp(-x) * (1 + y) + np.sin(2 * z),
            2.0 - x + 3 * y * z + 0.7 * y,
            0.7 + x ** 2 - np.sin(y + z)][k]


def equations_for(ri, method, names, dim):
    from pysph.sph.equation import Group
    from pysph.sph.basic_equations import SummationDensity
    if method == 'shepard':
        return [ri.InterpolateFunction(dest='interpolate', sources=names)]
    if method == 'sph':
        return [ri.InterpolateSPH(dest='interpolate', sources=names)]
    if method == 'splash':
        return [ri.SPLASHInterpolateProperty(dest='interpolate', sources=names)]
    if method == 'splash_norm':
        return [ri.SPLASHInterpolatePropertyNormalized(dest='interpolate', sources=names)]
    return [Group(equations=[SummationDensity(dest=n, sources=names) for n in names], real=False),
            Group(equations=[ri.SPHFirstOrderApproximationPreStep(dest='interpolate', sources=names, dim=dim)], real=True),
            Group(equations=[ri.SPHFirstOrderApproximation(dest='interpolate', sources=names, dim=dim)], real=True)]


def check_pivots(moment, npts, dim, has_nbr):
    """every point: no neighbour at all, or all elimination pivots (no row exchange) >= 1e-3"""
    n = dim + 1
    for i in range(npts):
        if not has_nbr[i]:
            continue
        m = np.array(moment[16 * i:16 * i + 16]).reshape(4, 4)[:n, :n].copy()
        for col in range(n):
            assert abs(m[col, col]) >= 1e-3, ('small pivot', i, col, m[col, col])
            for r in range(col + 1, n):
                m[r] -= m[r, col] / m[col, col] * m[col]


def ref_interpolate(ri, kernel, dim, sources, pts, fields, methods):
    """sources: [(name, {prop: array})]; fields: names present in (some of) the sources.
    -> {method: {field: values}}"""
    from pysph.sph.acceleration_eval import AccelerationEval
    hmax = max(float(np.max(p['h'])) for _, p in sources)
    npts = len(pts[0])
    names = [n for n, _ in sources]
    out = {}
    for method in methods:
        pas = []
        for name, props in sources:
            q = {k: np.asarray(props[k], dtype=float) for k in ('x', 'y', 'z', 'h', 'm', 'rho')}
            q['temp_prop'] = np.zeros(len(q['x']))
            q['extra_'] = np.zeros(len(q['x']))      # (the reference's property check wants a strict superset)
            pas.append(ListPA(name, q))
        z1 = np.zeros(npts)
        dp = dict(x=pts[0], y=pts[1], z=pts[2], h=hmax * np.ones(npts), number_density=z1, unity=z1, extra_=z1,
                  prop=np.zeros(npts * (4 if method == 'order1' else 1)), moment=np.zeros(16 * npts), p_sph=np.zeros(4 * npts),
                  m=z1, rho=z1)
        dst = ListPA('interpolate', dp)
        dst.n = npts
        dst.n_real = npts
        pas.append(dst)
        a_eval = AccelerationEval(pas, equations_for(ri, method, names, dim), kernel)
        nnps = PyLinkedListNNPS(dim, pas, radius_scale=kernel.radius_scale)
        nnps.update()
        di = len(pas) - 1
        dests = [di] + (list(range(di)) if method == 'order1' else [])
        has_nbr = np.zeros(npts, dtype=bool)
        for d in dests:
            for s in range(di):
                for i in range(pas[d].n):
                    a = sorted(nnps.neighbors(s, d, i))
                    assert a == nnps.brute_force(s, d, i), (s, d, i)
                    if d == di and a:
                        has_nbr[i] = True
        ev = RefEval(a_eval, nnps)
        groups = a_eval.mega_groups
        if method == 'order1':      # density and moments once: they do not depend on the property
            ev._do_group(groups[0], 0.0, 0.1)
            ev._do_group(groups[1], 0.0, 0.1)
            check_pivots(dst.properties['moment'], npts, dim, has_nbr)
        res = {}
        for f in fields:
            for pa, (name, props) in zip(pas, sources):
                data = props[f] if f in props else np.zeros(pa.n)
                pa.properties['temp_prop'] = [float(v) for v in data]
            if method == 'order1':
                dst.properties['p_sph'] = [0.0] * (4 * npts)     # every accumulator starts from zero (deviation 2)
                dst.properties['prop'] = [0.0] * (4 * npts)
                ev._do_group(groups[2], 0.0, 0.1)
            else:
                ev.compute(0.0, 0.1)
            res[f] = np.array(dst.properties['prop'])
            assert np.all(np.isfinite(res[f]))
            assert np.all(res[f].reshape(npts, -1)[~has_nbr] == 0.0)
        out[method] = res
        out['has_nbr'] = has_nbr
    return out


def lattice(rng, n, dx, dim, jitter=0.2):
    ax = [dx * (np.arange(k) + 0.5) for k in n] + [np.zeros(1)] * (3 - dim)
    g = np.meshgrid(*ax, indexing='ij')
    p = [a.ravel().copy() for a in g]
    for k in range(dim):
        p[k] += jitter * dx * rng.uniform(-1, 1, p[k].size)
    return p


def source_props(rng, x, y, z, h, rho0, dx, dim, nfields):
    n = x.size
    props = dict(x=x, y=y, z=z, h=h * np.ones(n), m=rho0 * dx ** dim * (1 + 0.05 * rng.uniform(-1, 1, n)),
                 rho=rho0 * (1 + 0.03 * rng.uniform(-1, 1, n)))
    for k in range(nfields):
        props['f%d' % k] = field_values(k, x, y, z)
    return props


def store(out, case, kernel, dim, sources, pts, fields, res):
    out['%s/kernel' % case] = np.array(type(kernel).__name__)
    out['%s/dim' % case] = np.array(dim)
    out['%s/sources' % case] = np.array([n for n, _ in sources])
    out['%s/fields' % case] = np.array(fields)
    out['%s/has_nbr' % case] = res.pop('has_nbr')
    for name, props in sources:
        for k, v in props.items():
            out['%s/src/%s/%s' % (case, name, k)] = np.asarray(v, dtype=float)
    for k, v in zip('xyz', pts):
        out['%s/pts/%s' % (case, k)] = np.asarray(v, dtype=float)
    for method, r in res.items():
        for f, v in r.items():
            out['%s/out/%s/%s' % (case, method, f)] = v


def main():
    ri = import_reference()
    from pysph.base.kernels import CubicSpline, Gaussian, QuinticSpline, WendlandQuintic
    out = {}

    # 1. 3-D, uniform h, Gaussian, all five methods, one source array, 130 scattered points
    rng = np.random.default_rng(20261017)
    dx = 0.1
    x, y, z = lattice(rng, (10, 10, 10), dx, 3)
    h = 1.0 * dx
    src = [('fluid', source_props(rng, x, y, z, h, 1000.0, dx, 3, 5))]
    L = 10 * dx
    interior = rng.uniform(0.35, 0.65, (3, 87))
    face = rng.uniform(0.3, 0.7, (3, 30))
    for k in range(30):                      # within one h of a free face (inside the particles)
        face[k % 3, k] = (0.4 * h + 0.5 * dx) if (k // 3) % 2 else L - 0.5 * dx - 0.4 * h
    far = rng.uniform(0.2, 0.8, (3, 12))
    for k in range(12):                      # farther than 3 hmax from every particle
        far[k % 3, k] = -3.2 * h - 0.3 * dx if (k // 3) % 2 else L + 3.2 * h + 0.3 * dx
    on = np.array([[x[555]], [y[555]], [z[555]]])   # exactly on a particle
    pts = np.concatenate([interior, face, far, on], axis=1)
    assert pts.shape[1] == 130
    fields = ['f%d' % k for k in range(5)]
    res = ref_interpolate(ri, Gaussian(dim=3), 3, src, pts, fields, ('shepard', 'sph', 'order1', 'splash', 'splash_norm'))
    assert int((~res['has_nbr']).sum()) == 12
    store(out, 'c1', Gaussian(dim=3), 3, src, pts, fields, res)
    print('case 1 done')

    # 2. 3-D, variable h (+- 20 %), CubicSpline: WIJ, WI and WJ differ
    rng = np.random.default_rng(20261018)
    x, y, z = lattice(rng, (10, 10, 10), dx, 3)
    hv = 1.3 * dx * (1 + 0.2 * rng.uniform(-1, 1, x.size))
    src = [('fluid', source_props(rng, x, y, z, hv, 1000.0, dx, 3, 5))]
    pts = np.concatenate([rng.uniform(0.1, 0.9, (3, 110)), rng.uniform(-0.3, 1.3, (3, 20))], axis=1)
    res = ref_interpolate(ri, CubicSpline(dim=3), 3, src, pts, fields, ('shepard', 'splash', 'splash_norm'))
    store(out, 'c2', CubicSpline(dim=3), 3, src, pts, fields, res)
    print('case 2 done')

    # 3. 2-D, QuinticSpline, shepard and order1 (3 x 3 system)
    rng = np.random.default_rng(20261019)
    dx2 = 0.05
    x, y, z = lattice(rng, (30, 30), dx2, 2)
    src = [('fluid', source_props(rng, x, y, z, 1.2 * dx2, 1000.0, dx2, 2, 5))]
    p2 = np.concatenate([rng.uniform(0.3, 1.2, (2, 100)), rng.uniform(0.03, 1.47, (2, 20)),
                         np.array([[-0.5, 2.0, 0.7], [0.7, 0.7, 2.1]])], axis=1)
    pts = np.concatenate([p2, np.zeros((1, p2.shape[1]))], axis=0)
    res = ref_interpolate(ri, QuinticSpline(dim=2), 2, src, pts, fields, ('shepard', 'order1'))
    store(out, 'c3', QuinticSpline(dim=2), 2, src, pts, fields, res)
    print('case 3 done')

    # 4. 1-D, CubicSpline, shepard, sph and order1 (2 x 2 system)
    rng = np.random.default_rng(20261020)
    dx1 = 0.01
    x, y, z = lattice(rng, (200,), dx1, 1)
    src = [('fluid', source_props(rng, x, y, z, 1.5 * dx1, 1.0, dx1, 1, 5))]
    p1 = np.concatenate([rng.uniform(0.1, 1.9, 110), rng.uniform(0.006, 0.03, 8), [-0.2, 2.3, x[77]]])
    pts = np.stack([p1, np.zeros_like(p1), np.zeros_like(p1)])
    res = ref_interpolate(ri, CubicSpline(dim=1), 1, src, pts, fields, ('shepard', 'sph', 'order1'))
    store(out, 'c4', CubicSpline(dim=1), 1, src, pts, fields, res)
    print('case 4 done')

    # 5. three source arrays from the wcsph_dam_dx0.1 inputs (sub-sampled); 'f1' exists on the fluid only
    rng = np.random.default_rng(20261021)
    g = np.load(os.path.join(HERE, 'wcsph_dam_dx0.1.npz'))
    src = []
    for name, keep in (('fluid', 500), ('boundary', 600), ('obstacle', None)):
        n = g['in/%s/x' % name].size
        idx = np.arange(n) if keep is None else np.sort(rng.choice(n, keep, replace=False))
        props = {k: g['in/%s/%s' % (name, k)][idx] for k in ('x', 'y', 'z', 'h', 'm', 'rho')}
        props['f0'] = field_values(0, props['x'], props['y'], props['z'])
        if name == 'fluid':
            props['f1'] = field_values(1, props['x'], props['y'], props['z'])
        for k in (2, 3, 4):
            props['f%d' % k] = field_values(k, props['x'], props['y'], props['z'])
        src.append((name, props))
    pts = np.stack([rng.uniform(-0.1, 3.3, 100), rng.uniform(-0.6, 0.6, 100), rng.uniform(-0.1, 1.1, 100)])
    res = ref_interpolate(ri, WendlandQuintic(dim=3), 3, src, pts, fields, ('shepard', 'sph'))
    store(out, 'c5', WendlandQuintic(dim=3), 3, src, pts, fields, res)
    print('case 5 done')

    # 6. 3-D, variable h, TWO source arrays, WendlandQuintic, order1 (and shepard): the density pass over every source
    # as destination, the variable-h first-order kernels
    rng = np.random.default_rng(20261023)
    dx6 = 0.1
    x, y, z = lattice(rng, (9, 9, 9), dx6, 3)
    hv = 1.4 * dx6 * (1 + 0.2 * rng.uniform(-1, 1, x.size))
    allp = source_props(rng, x, y, z, hv, 1000.0, dx6, 3, 5)
    pick = rng.uniform(0, 1, x.size) < 0.6
    src = [('fluid', {k: v[pick] for k, v in allp.items()}), ('solid', {k: v[~pick] for k, v in allp.items()})]
    pts = np.concatenate([rng.uniform(0.3, 0.6, (3, 50)), np.array([[-1.0, 2.0], [0.4, 0.4], [0.4, 0.4]])], axis=1)
    res = ref_interpolate(ri, WendlandQuintic(dim=3), 3, src, pts, fields, ('shepard', 'order1'))
    store(out, 'c6', WendlandQuintic(dim=3), 3, src, pts, fields, res)
    print('case 6 done')

    # 7. get_bounding_box / get_nx_ny_nz: recorded outputs
    class _PA(object):
        def __init__(self, x, y, z):
            self.x, self.y, self.z = x, y, z
    rng = np.random.default_rng(20261022)
    n = 0

    def cloud(ext):
        return _PA(*[e * rng.uniform(0, 1, 50) + 0.1 * k for k, e in enumerate(ext)])
    # 1-D, 2-D and 3-D extents; a degenerate axis just above / below the 1e-4 and 1e-3 relative-length thresholds
    for ext, tight, stretch, npnt in (((1.0, 0.0, 0.0), False, 0.05, 100), ((2.0, 1.0, 0.0), False, 0.05, 5000),
                                      ((1.0, 2.0, 0.5), False, 0.05, 125000), ((1.0, 2.0, 0.5), True, 0.05, 1000),
                                      ((1.0, 1.0, 0.5), False, 0.1, 777), ((1.0, 1.0, 2.4e-3), True, 0.05, 10000),
                                      ((1.0, 1.0, 1.7e-3), True, 0.05, 10000), ((1.0, 1.0, 2.4e-4), True, 0.05, 10000),
                                      ((1.0, 1.0, 1.7e-4), True, 0.05, 10000)):
        arrays = [cloud(ext), cloud(ext)]
        bounds = ri.get_bounding_box(arrays, tight=tight, stretch=stretch)
        dims = ri.get_nx_ny_nz(npnt, bounds)
        for k, a in enumerate(arrays):
            for c in 'xyz':
                out['bb/%d/in/%d/%s' % (n, k, c)] = getattr(a, c)
        out['bb/%d/tight' % n] = np.array(tight)
        out['bb/%d/stretch' % n] = np.array(stretch)
        out['bb/%d/num_points' % n] = np.array(npnt)
        out['bb/%d/bounds' % n] = np.array(bounds)
        out['bb/%d/dims' % n] = np.array(dims)
        n += 1
    out['bb/n'] = np.array(n)
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT) // 1024, 'KiB')


if __name__ == '__main__':
    main()
