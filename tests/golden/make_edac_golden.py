#!/usr/bin/env python
"""Golden vectors for the EDAC scheme, from the REFERENCE's own ``EDACScheme`` and its
own equation and stepper classes (pysph/sph/wc/edac.py), in the manner of
make_wcsph_options_golden.py (same driver, same stored layout):

    python tests/golden/make_edac_golden.py

    edac_ext3d.npz          external branch, 3-D 6^3 fluid (last 20 rows ghosts) over two wall layers (`solids`),
                            a free-slip patch with unit normals (`inviscid_solids`) and one wall particle far from
                            everything; alpha, nu, eps, clamp_p, gz, 0 < t < tdamp; QuinticSpline; out/ after one
                            evaluation, out2/ + nnps2/ after moving the fluid by dt u, a neighbour update and a second
    edac_int2d.npz          internal branch, 2-D 16 x 12 fluid over three wall layers, h +-10 %, pb > 0, bql,
                            WendlandQuinticC4
    edac_int3d_nosolid.npz  internal branch without solids (ComputeAveragePressure shares group 1 with the density),
                            edac_alpha = 0 (the real nu), CubicSpline
    edac_kernels.npz        per smoothing kernel class one tiny external-branch case without walls, stored under the
                            class name as prefix
    edac_steppers.npz       EDACStep and EDACTVFStep, initialize / stage1 / stage2 on random columns
    edac_steps.npz          the edac_ext3d particles through three PEC steps (dt = 1e-4)
    edac_structures.npz     group lists only, for further option combinations

Every output property starts as random garbage, so that a missing write shows.  Conditions asserted on the reference
alone (re-seeded until met, results under meta/): no wall row with 0 < wij < 1e-8 max(wij) (the wall equations divide
by wij behind the thresholds 1e-14 / 1e-12) and at least one with wij == 0 exactly; a tenth of the fluid-fluid pairs
with vijdotrij < 0 and a tenth without; with clamp_p one wall pressure clamped and one not; nnbr >= 1 on every fluid row.
"""
import json
import os
import sys
import types
from inspect import getfullargspec

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402  (sets up the reference imports)

from oracle.ref_driver import ListPA, PyLinkedListNNPS, RefEval  # noqa: E402

if 'pysph.base.utils' not in sys.modules:
    # wc/edac.py imports pysph.base.utils (-> cyarray, absent) for a particle-array factory and the default names only
    _m = types.ModuleType('pysph.base.utils')
    _m.get_particle_array = lambda *a, **k: None
    sys.modules['pysph.base.utils'] = _m
sys.modules['pysph.base.utils'].DEFAULT_PROPS = set(
    ('x', 'y', 'z', 'u', 'v', 'w', 'm', 'h', 'rho', 'p', 'au', 'av', 'aw', 'gid', 'pid', 'tag'))

from pysph.sph.acceleration_eval import AccelerationEval  # noqa: E402
from pysph.sph.wc import edac as RE  # noqa: E402
from pysph.base import kernels as RK  # noqa: E402

RE.print = lambda *a, **k: None          # (_get_edac_nu reports its choice on stdout)

SKIP_ATTRS = ('dest', 'sources', 'name', 'var_name', 'no_source')
KERNELS = ('CubicSpline', 'WendlandQuintic', 'QuinticSpline', 'Gaussian', 'WendlandQuinticC2_1D', 'WendlandQuinticC4',
           'WendlandQuinticC4_1D', 'WendlandQuinticC6', 'WendlandQuinticC6_1D', 'SuperGaussian')

FLUID_OUT_EXT = ('rho', 'V', 'au', 'av', 'aw', 'ap', 'ax', 'ay', 'az')
FLUID_OUT_INT = ('rho', 'V', 'au', 'av', 'aw', 'ap', 'auhat', 'avhat', 'awhat', 'pavg', 'nnbr')
WALL_OUT = ('wij', 'V', 'p', 'uf', 'vf', 'wf', 'ug', 'vg', 'wg')
SLIP_OUT_EXT = ('wij', 'V', 'p', 'u', 'v', 'w')
SLIP_OUT_INT = SLIP_OUT_EXT + ('uhat', 'vhat', 'what')


def structure(groups):
    out = []
    for g in groups:
        eqs = []
        for eq in g.equations:
            par = dict((k, (bool(v) if isinstance(v, bool) else float(v))) for k, v in vars(eq).items()
                       if k not in SKIP_ATTRS and not k.startswith('_') and isinstance(v, (bool, int, float)))
            eqs.append(dict(cls=type(eq).__name__, dest=eq.dest, sources=list(eq.sources or []), params=par))
        out.append(dict(real=bool(g.real), equations=eqs))
    return out


def _nnps_out(out, nnps, prefix):
    out[prefix + '/cell_size'] = np.array(nnps.cell_size)
    out[prefix + '/xmin'] = np.array(nnps.xmin)
    out[prefix + '/xmax'] = np.array(nnps.xmax)
    out[prefix + '/ncells_per_dim'] = np.array(nnps.nc)
    out[prefix + '/n_cells'] = np.array(nnps.n_cells)


def _store(out, pas, which):
    for pa in pas:
        for k, v in pa.properties.items():
            out['%s/%s/%s' % (which, pa.name, k)] = np.array(v)


def conditions(pas, nnps, kw, need_zero_wij):
    """the conditions of the module docstring, on the reference's results; returns what goes under meta/"""
    arrays = dict((pa.name, pa) for pa in pas)
    names = [pa.name for pa in pas]
    meta = {}
    walls = list(kw.get('solids') or []) + list(kw.get('inviscid_solids') or [])
    if walls:
        wij = np.concatenate([np.array(arrays[w].properties['wij']) for w in walls])
        big = wij.max()
        tiny = (wij > 0) & (wij < 1e-8 * big)
        assert not tiny.any(), ('wij next to a threshold', wij[tiny])
        meta['n_wij_zero'] = int(np.sum(wij == 0.0))
        meta['min_wij_nonzero'] = float(wij[wij > 0].min() / big)
        if need_zero_wij:
            assert meta['n_wij_zero'] >= 1
    if kw.get('alpha', 0.0) > 0.0:
        f = arrays[kw['fluids'][0]]
        fi = names.index(f.name)
        P = dict((k, np.array(f.properties[k])) for k in 'xyzuvw')
        neg = tot = 0
        for i in range(f.n_real):
            nb = np.array(nnps.neighbors(fi, fi, i))
            nb = nb[nb != i]
            d = sum((P[a][i] - P[a][nb]) * (P[b][i] - P[b][nb]) for a, b in zip('uvw', 'xyz'))
            neg += int(np.sum(d < 0))
            tot += nb.size
        assert neg * 10 >= tot and (tot - neg) * 10 >= tot, (neg, tot)
        meta['n_pairs'], meta['n_approaching'] = tot, neg
    if kw.get('clamp_p') and kw.get('solids'):
        p = np.concatenate([np.array(arrays[w].properties['p']) for w in kw['solids']])
        w_ = np.concatenate([np.array(arrays[w].properties['wij']) for w in kw['solids']])
        meta['n_clamped'] = int(np.sum((p == 0.0) & (w_ > 0)))
        meta['n_unclamped'] = int(np.sum(p > 0.0))
        assert meta['n_clamped'] >= 1 and meta['n_unclamped'] >= 1, meta
    if abs(kw.get('pb', 0.0)) > 1e-14 and kw.get('bql', True):
        for fl in kw['fluids']:
            f = arrays[fl]
            nn = np.array(f.properties['nnbr'])[:f.n_real]
            assert np.all(nn >= 1.0)
            meta['min_nnbr'] = float(nn.min())
    return meta


def evaluate(arrays, kw, kernel, t, dt, second=False, need_zero_wij=False, steps=0, prefix=''):
    """arrays: [(name, props, n_real)].  Returns the dictionary of what is stored."""
    dim = kw['dim']
    s = RE.EDACScheme(**kw)
    groups = s.get_equations()
    pas = [ListPA(name, props, n_real) for name, props, n_real in arrays]
    out = {}
    _store(out, pas, 'in')
    for pa in pas:
        out['nreal/%s' % pa.name] = np.array(pa.n_real)
    a_eval = AccelerationEval(pas, groups, kernel)
    nnps = PyLinkedListNNPS(dim, pas, radius_scale=kernel.radius_scale)
    ev = RefEval(a_eval, nnps)
    meta = {}
    fluid = [pa for pa in pas if pa.name == kw['fluids'][0]][0]
    if steps:
        # pysph/sph/integrator.py:227-246 (PECIntegrator.one_timestep): initialize; stage1; update_domain;
        # compute_accelerations (neighbours rebuilt); stage2; update_domain
        step = RE.EDACTVFStep() if s.use_tvf else RE.EDACStep()

        def sweep(meth, dt_):
            f = getattr(step, meth)
            args = [a for a in getfullargspec(f).args if a != 'self']
            ns = dict(('d_' + k, v) for k, v in fluid.properties.items())
            ns.update(dt=dt_, t=t)
            for i in range(fluid.n_real):
                ns['d_idx'] = i
                f(*[ns[a] for a in args])
        tt = t
        for k in range(steps):
            sweep('initialize', dt)
            sweep('stage1', dt)
            nnps.update()
            ev.compute(tt + 0.5 * dt, dt)
            sweep('stage2', dt)
            tt += dt
        _store(out, pas, 'out')
        meta['steps'] = steps
    else:
        nnps.update()
        MG.check_nnps(nnps)
        ev.compute(t, dt)
        _store(out, pas, 'out')
        _nnps_out(out, nnps, 'nnps')
        meta.update(conditions(pas, nnps, kw, need_zero_wij))
        if second:
            P = fluid.properties
            for a, b in zip('xyz', 'uvw'):
                P[a] = [x + dt * u for x, u in zip(P[a], P[b])]
            nnps.update()
            MG.check_nnps(nnps)
            ev.compute(t + dt, dt)
            _store(out, pas, 'out2')
            _nnps_out(out, nnps, 'nnps2')
            meta.update(('second_' + k, v) for k, v in conditions(pas, nnps, kw, need_zero_wij).items())
    out['t'] = np.array(t)
    out['dt'] = np.array(dt)
    out['structure'] = np.array(json.dumps(structure(groups)))
    out['scheme'] = np.array(json.dumps(kw))
    out['kernel'] = np.array(type(kernel).__name__)
    for k, v in meta.items():
        out['meta/' + k] = np.array(v)
    return dict((prefix + k, v) for k, v in out.items()), meta


def save(fname, out, note=''):
    path = os.path.join(HERE, fname)
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path) // 1024, 'KiB', note)


def _garbage(props, rng, n, names):
    for k in names:
        props[k] = rng.uniform(-1, 1, n)          # garbage: must be overwritten


def _fluid3d(n1, rng, rho0, c0, hfac=1.2, varh=0.0, internal=False):
    dx = 1.0 / n1
    g = (np.arange(n1) + 0.5) * dx
    x, y, z = [a.ravel() for a in np.meshgrid(g, g, g, indexing='ij')]
    n = x.size
    props = dict(
        x=x + 0.2 * dx * rng.uniform(-1, 1, n), y=y + 0.2 * dx * rng.uniform(-1, 1, n),
        z=z + 0.2 * dx * rng.uniform(-1, 1, n),
        u=rng.uniform(-1, 1, n), v=rng.uniform(-1, 1, n), w=rng.uniform(-1, 1, n),
        h=hfac * dx * (1 + varh * rng.uniform(-1, 1, n)), m=rho0 * dx ** 3 * np.ones(n),
        p=0.05 * rho0 * c0 * c0 * rng.uniform(-1, 1, n))
    if internal:
        for a in 'uvw':
            props[a + 'hat'] = props[a] + 0.1 * rng.uniform(-1, 1, n)
    _garbage(props, rng, n, FLUID_OUT_INT if internal else FLUID_OUT_EXT)
    return props, n, dx


def _wall(x, y, z, rng, dx, hfac, rho0, mass, jitter=0.1, varh=0.0, out=WALL_OUT, moving=True):
    n = x.size
    props = dict(x=x + jitter * dx * rng.uniform(-1, 1, n), y=y + jitter * dx * rng.uniform(-1, 1, n),
                 z=z + jitter * dx * rng.uniform(-1, 1, n) * (1.0 if np.any(z != 0) else 0.0),
                 h=hfac * dx * (1 + varh * rng.uniform(-1, 1, n)), m=mass * np.ones(n),
                 rho=rho0 * (1 + 0.05 * rng.uniform(-1, 1, n)),
                 au=0.3 * rng.uniform(-1, 1, n), av=0.3 * rng.uniform(-1, 1, n), aw=0.3 * rng.uniform(-1, 1, n))
    if 'u' not in out:
        for a in 'uvw':
            props[a] = 0.5 * rng.uniform(-1, 1, n) if moving else np.zeros(n)
    _garbage(props, rng, n, out)
    return props, n


def _with_far(x, y, z, far):
    return np.append(x, far[0]), np.append(y, far[1]), np.append(z, far[2])


EXT3D_KW = dict(fluids=['fluid'], solids=['wall'], inviscid_solids=['slip'], dim=3, c0=10.0, nu=0.01, rho0=1000.0,
                pb=0.0, gz=-9.81, tdamp=1.0, eps=0.5, alpha=0.2, clamp_p=True)


def _ext3d_arrays(seed):
    rng = np.random.default_rng(seed)
    rho0, c0 = 1000.0, 10.0
    fluid, n, dx = _fluid3d(6, rng, rho0, c0)
    g = (np.arange(8) - 0.5) * dx
    x, y, z = [a.ravel() for a in np.meshgrid(g, g, (np.arange(-2, 0) + 0.5) * dx, indexing='ij')]
    x, y, z = _with_far(x, y, z, (5.0, 5.0, 5.0))
    wall, nw = _wall(x, y, z, rng, dx, 1.2, rho0, rho0 * dx ** 3)
    x, z, y = [a.ravel() for a in np.meshgrid((np.arange(6) + 0.5) * dx, (np.arange(4) + 0.5) * dx, [-0.5 * dx],
                                              indexing='ij')]
    slip, ns = _wall(x, y, z, rng, dx, 1.2, rho0, rho0 * dx ** 3, out=SLIP_OUT_EXT)
    nrm = np.stack([0.2 * rng.uniform(-1, 1, ns), np.ones(ns), 0.2 * rng.uniform(-1, 1, ns)])
    nrm /= np.sqrt((nrm ** 2).sum(axis=0))
    slip['xn'], slip['yn'], slip['zn'] = nrm
    kw = dict(EXT3D_KW, h=1.2 * dx)
    return [('fluid', fluid, n - 20), ('wall', wall, nw), ('slip', slip, ns)], kw, dx


def case_ext3d():
    for seed in range(200, 240):
        arrays, kw, dx = _ext3d_arrays(seed)
        try:
            out, meta = evaluate(arrays, kw, RK.QuinticSpline(dim=3), t=0.3, dt=1e-4, second=True, need_zero_wij=True)
        except AssertionError as e:
            print('seed', seed, 'rejected:', e)
            continue
        out['meta/seed'], out['meta/dx'] = np.array(seed), np.array(dx)
        save('edac_ext3d.npz', out, meta)
        # the same particles through three PEC steps
        arrays, kw, dx = _ext3d_arrays(seed)
        fl = arrays[0][1]
        rng = np.random.default_rng(seed + 1000)
        _garbage(fl, rng, len(fl['x']), ('x0', 'y0', 'z0', 'u0', 'v0', 'w0', 'p0'))
        out, meta = evaluate(arrays, kw, RK.QuinticSpline(dim=3), t=0.3, dt=1e-4, steps=3)
        out['meta/seed'] = np.array(seed)
        save('edac_steps.npz', out, meta)
        return
    raise RuntimeError('no seed met the conditions')


def case_int2d():
    for seed in range(300, 340):
        rng = np.random.default_rng(seed)
        dx, rho0, c0 = 1.0 / 16, 1000.0, 10.0
        gx, gy = (np.arange(16) + 0.5) * dx, (np.arange(12) + 0.5) * dx
        x, y = [a.ravel() for a in np.meshgrid(gx, gy, indexing='ij')]
        n = x.size
        fluid = dict(x=x + 0.2 * dx * rng.uniform(-1, 1, n), y=y + 0.2 * dx * rng.uniform(-1, 1, n), z=np.zeros(n),
                     u=rng.uniform(-1, 1, n), v=rng.uniform(-1, 1, n), w=np.zeros(n),
                     h=1.3 * dx * (1 + 0.1 * rng.uniform(-1, 1, n)), m=rho0 * dx ** 2 * np.ones(n),
                     p=0.05 * rho0 * c0 * c0 * rng.uniform(-1, 1, n))
        fluid['uhat'] = fluid['u'] + 0.1 * rng.uniform(-1, 1, n)
        fluid['vhat'] = fluid['v'] + 0.1 * rng.uniform(-1, 1, n)
        fluid['what'] = np.zeros(n)
        _garbage(fluid, rng, n, FLUID_OUT_INT)
        bx, by = (np.arange(-3, 19) + 0.5) * dx, (np.arange(-3, 0) + 0.5) * dx
        x, y = [a.ravel() for a in np.meshgrid(bx, by, indexing='ij')]
        x, y, z = _with_far(x, y, np.zeros(x.size), (4.0, 4.0, 0.0))
        wall, nw = _wall(x, y, z, rng, dx, 1.3, rho0, rho0 * dx ** 2, jitter=0.2, varh=0.1)
        wall['w'] = np.zeros(nw)
        wall['aw'] = np.zeros(nw)
        kw = dict(fluids=['fluid'], solids=['wall'], dim=2, c0=c0, nu=0.02, rho0=rho0, pb=rho0 * c0 * c0, gy=-9.81,
                  h=1.3 * dx, alpha=0.3, bql=True)
        try:
            out, meta = evaluate([('fluid', fluid, n), ('wall', wall, nw)], kw, RK.WendlandQuinticC4(dim=2), t=0.0,
                                 dt=1e-4, need_zero_wij=True)
        except AssertionError as e:
            print('seed', seed, 'rejected:', e)
            continue
        out['meta/seed'], out['meta/dx'] = np.array(seed), np.array(dx)
        save('edac_int2d.npz', out, meta)
        return
    raise RuntimeError('no seed met the conditions')


def case_int3d_nosolid():
    rng = np.random.default_rng(401)
    fluid, n, dx = _fluid3d(6, rng, 1000.0, 10.0, internal=True)
    kw = dict(fluids=['fluid'], solids=[], dim=3, c0=10.0, nu=0.05, rho0=1000.0, pb=1.0e5, gx=0.4, tdamp=0.5,
              h=1.2 * dx, edac_alpha=0.0, alpha=0.1)
    out, meta = evaluate([('fluid', fluid, n - 20)], kw, RK.CubicSpline(dim=3), t=0.2, dt=1e-4)
    out['meta/dx'] = np.array(dx)
    save('edac_int3d_nosolid.npz', out, meta)


def case_kernels():
    allout = {}
    for k, name in enumerate(KERNELS):
        rng = np.random.default_rng(500 + k)
        cls = getattr(RK, name)
        if name.endswith('_1D'):
            dim, n = 1, 40
            dx, rho0, c0 = 1.0 / n, 1000.0, 10.0
            fluid = dict(x=(np.arange(n) + 0.5) * dx + 0.2 * dx * rng.uniform(-1, 1, n), y=np.zeros(n), z=np.zeros(n),
                         u=rng.uniform(-1, 1, n), v=np.zeros(n), w=np.zeros(n), h=1.3 * dx * np.ones(n),
                         m=rho0 * dx * np.ones(n), p=0.05 * rho0 * c0 * c0 * rng.uniform(-1, 1, n))
            _garbage(fluid, rng, n, FLUID_OUT_EXT)
            hh = 1.3 * dx
        else:
            dim = 3
            fluid, n, dx = _fluid3d(4, rng, 1000.0, 10.0)
            hh = 1.2 * dx
        kw = dict(fluids=['fluid'], solids=[], dim=dim, c0=10.0, nu=0.01, rho0=1000.0, gx=0.3, eps=0.3, h=hh, alpha=0.1)
        out, meta = evaluate([('fluid', fluid, n)], kw, cls(dim=dim), t=0.0, dt=1e-4, prefix=name + '/')
        allout.update(out)
    allout['kernels'] = np.array(json.dumps(list(KERNELS)))
    save('edac_kernels.npz', allout)


def case_steppers():
    """the reference's stepper methods executed as plain Python on 24 random particles (as make_golden.case_steppers)"""
    rng = np.random.default_rng(611)
    n = 24
    names = ['x', 'y', 'z', 'u', 'v', 'w', 'p', 'x0', 'y0', 'z0', 'u0', 'v0', 'w0', 'p0', 'au', 'av', 'aw', 'ax', 'ay',
             'az', 'ap', 'uhat', 'vhat', 'what', 'auhat', 'avhat', 'awhat']
    base = dict((k, rng.uniform(-1, 1, n)) for k in names)
    out = dict(('in/' + k, v.copy()) for k, v in base.items())
    dt = 0.0123
    out['dt'] = np.array(dt)
    for step, tag in ((RE.EDACStep(), 'edac'), (RE.EDACTVFStep(), 'edac_tvf')):
        st = dict((k, [float(x) for x in v]) for k, v in base.items())
        for meth in ('initialize', 'stage1', 'stage2'):
            f = getattr(step, meth)
            args = [a for a in getfullargspec(f).args if a != 'self']
            for i in range(n):
                ns = dict(('d_' + k, v) for k, v in st.items())
                ns.update(d_idx=i, dt=dt, t=0.0)
                f(*[ns[a] for a in args])
            for k, v in st.items():
                out['%s/%s/%s' % (tag, meth, k)] = np.array(v)
    save('edac_steppers.npz', out)


STRUCTURES = dict(
    bql_false=dict(fluids=['fluid'], solids=['wall'], dim=2, c0=10.0, nu=0.01, rho0=1.0, pb=100.0, h=0.1, bql=False),
    alpha0_nu0=dict(fluids=['fluid'], solids=['wall'], dim=2, c0=10.0, nu=0.0, rho0=1.0, pb=100.0, h=0.1, alpha=0.0),
    ext_alpha0_nu0=dict(fluids=['fluid'], solids=['wall'], dim=3, c0=10.0, nu=0.0, rho0=1.0, h=0.1, eps=0.2),
    no_solids_ext=dict(fluids=['fluid'], solids=[], dim=3, c0=10.0, nu=0.01, rho0=1.0, h=0.1, alpha=0.2, gz=-1.0),
    no_solids_int=dict(fluids=['f1', 'f2'], solids=[], dim=3, c0=10.0, nu=0.01, rho0=1.0, pb=50.0, h=0.1),
    clamp_p_with_pb=dict(fluids=['fluid'], solids=['wall'], inviscid_solids=['slip'], dim=2, c0=10.0, nu=0.01,
                         rho0=1.0, pb=100.0, h=0.1, clamp_p=True, alpha=0.1, tdamp=0.5, gx=1.0),
    edac_alpha0=dict(fluids=['fluid'], solids=['wall'], dim=2, c0=10.0, nu=0.03, rho0=1.0, h=0.1, edac_alpha=0.0,
                     clamp_p=True),
)


def case_structures():
    out = {}
    for name, kw in STRUCTURES.items():
        out[name + '/scheme'] = np.array(json.dumps(kw))
        out[name + '/structure'] = np.array(json.dumps(structure(RE.EDACScheme(**kw).get_equations())))
    out['names'] = np.array(json.dumps(sorted(STRUCTURES)))
    save('edac_structures.npz', out)


if __name__ == '__main__':
    which = sys.argv[1:] or ['ext3d', 'int2d', 'int3d_nosolid', 'kernels', 'steppers', 'structures']
    for name in which:
        globals()['case_' + name]()
