"""``pysph_amd.interpolator.Interpolator`` (pysph/tools/interpolator.py on the
HIP backend) and the C-ABI entry ``sph_interpolate`` behind it.

Reference values: tests/golden/interpolator.npz (make_interpolator_golden.py:
the reference's interpolation equations run as plain Python), a brute force
written here, and invariants that need no reference.  No point is excluded
from any comparison."""
import ctypes as C
import functools
import importlib.util
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
from helpers import rel_err

TOL = 1e-10      # the project's golden tolerance (BASELINE.json)
# The fields f0..f4 of the fixtures travel under the names of built-in properties: a property without a built-in id takes
# one of the 96 user property slots of the process-wide table, which the whole test session shares.
AS = {'f0': 'u', 'f1': 'v', 'f2': 'w', 'f3': 'p', 'f4': 'cs'}
ALL = ['shepard', 'sph', 'order1', 'splash', 'splash_norm']


@functools.lru_cache(maxsize=None)
def golden():
    g = load_golden('interpolator.npz')
    return {k: g[k] for k in g.files}


def case_arrays(case):
    from pysph_amd.particle_array import ParticleArray
    g = golden()
    out = []
    for name in g[case + '/sources']:
        name = str(name)
        pre = '%s/src/%s/' % (case, name)
        out.append(ParticleArray(name=name, **{AS.get(k[len(pre):], k[len(pre):]): g[k].copy() for k in g if k.startswith(pre)}))
    return out


def case_setup(case):
    from pysph_amd import kernels as K
    g = golden()
    kernel = getattr(K, str(g[case + '/kernel']))(dim=int(g[case + '/dim']))
    pts = [g['%s/pts/%s' % (case, c)] for c in 'xyz']
    fields = [str(f) for f in g[case + '/fields']]
    methods = [m for m in ALL if '%s/out/%s/%s' % (case, m, fields[0]) in g]
    return kernel, pts, fields, methods


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_bounding_box_and_mesh_counts_match_the_recorded_reference_outputs():
    from pysph_amd.particle_array import ParticleArray
    from pysph_amd.tools import get_bounding_box, get_nx_ny_nz
    g = golden()
    n = int(g['bb/n'])
    assert n >= 6
    for i in range(n):
        arrays = [ParticleArray(name='a%d' % k, **{c: g['bb/%d/in/%d/%s' % (i, k, c)] for c in 'xyz'}) for k in (0, 1)]
        bounds = get_bounding_box(arrays, tight=bool(g['bb/%d/tight' % i]), stretch=float(g['bb/%d/stretch' % i]))
        want = g['bb/%d/bounds' % i]
        assert np.all(np.abs(bounds - want) <= 1e-15 * np.abs(want)), (i, bounds, want)
        dims = get_nx_ny_nz(int(g['bb/%d/num_points' % i]), want)
        assert list(dims) == list(g['bb/%d/dims' % i]), (i, dims)


def small_arrays(n):
    from pysph_amd.particle_array import get_particle_array
    rng = np.random.default_rng(1)
    return [get_particle_array(name='a%d' % k, x=rng.random(5), y=rng.random(5), z=rng.random(5), h=0.5 * np.ones(5))
            for k in range(n)]


def test_unknown_method_raises_runtime_error_before_any_device_call():
    from pysph_amd.tools import Interpolator
    with pytest.raises(RuntimeError, match='nearest method is not implemented'):
        Interpolator(small_arrays(1), num_points=10, method='nearest')


def test_custom_equations_are_refused_with_a_pointer_to_sph_evaluator():
    from pysph_amd.tools import Interpolator
    with pytest.raises(NotImplementedError, match='SPHEvaluator'):
        Interpolator(small_arrays(1), num_points=10, equations=[object()])


def test_too_many_source_arrays_raise_value_error():
    from pysph_amd import device as dev
    from pysph_amd.tools import Interpolator
    with pytest.raises(ValueError):
        Interpolator(small_arrays(dev.MAX_ARRAYS), num_points=10)


def test_golden_generator_imports_cleanly():
    if not os.path.isdir('/root/reference'):
        pytest.skip('the generator needs the reference (build container only)')
    spec = importlib.util.spec_from_file_location('make_interpolator_golden',
                                                  os.path.join(GOLDEN, 'make_interpolator_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert callable(mod.main) and mod.OUT.endswith('interpolator.npz')


# ---------------------------------------------------------------------------
# A. golden parity
# ---------------------------------------------------------------------------
def check_against_golden(case, method, interp, fields):
    g = golden()
    no_nbr = ~g[case + '/has_nbr']
    assert interp.shape == g[case + '/pts/x'].shape
    for comp in (range(4) if method == 'order1' else (0,)):
        many = interp.interpolate_many([AS[f] for f in fields], comp=comp)
        for f, got in zip(fields, many):
            want = g['%s/out/%s/%s' % (case, method, f)]
            want = want[comp::4] if method == 'order1' else want     # every component against its own magnitude
            err = rel_err(got, want)
            print(case, method, f, comp, 'rel_err %.3e' % err)
            assert err < TOL, (case, method, f, comp, err)
            assert np.all(got[no_nbr] == 0.0)
            one = interp.interpolate(AS[f], comp=comp)
            assert np.array_equal(one, got), (case, method, f, comp)      # to the bit


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['c1', 'c2', 'c3', 'c4', 'c5', 'c6'])
def test_golden_parity(case):
    from pysph_amd.tools import Interpolator
    kernel, pts, fields, methods = case_setup(case)
    assert len(fields) > 4 and methods
    for method in methods:
        interp = Interpolator(case_arrays(case), kernel=kernel, x=pts[0], y=pts[1], z=pts[2], method=method)
        assert interp.pa.name == 'interpolate'
        check_against_golden(case, method, interp, fields)
        interp.close()


# ---------------------------------------------------------------------------
# B. brute force written here
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def brute_sources():
    rng = np.random.default_rng(4097)
    dx = 1.0 / 16
    g = np.meshgrid(*[dx * (np.arange(16) + 0.5)] * 3, indexing='ij')
    p = [np.append(a.ravel(), 0.5 + 0.01 * k) for k, a in enumerate(g)]           # 16^3 + 1 = 4097
    n = p[0].size
    x, y, z = [a + 0.2 * dx * rng.uniform(-1, 1, n) for a in p]
    props = dict(x=x, y=y, z=z, h=1.2 * dx * (1 + 0.15 * rng.uniform(-1, 1, n)),
                 m=dx ** 3 * (1 + 0.05 * rng.uniform(-1, 1, n)), rho=1 + 0.03 * rng.uniform(-1, 1, n))
    props['f0'] = 1 + np.sin(3 * x) - 2 * y ** 2 + x * z
    props['f1'] = np.cos(2 * x + y) + 0.5 * z
    props['f2'] = x * y - z ** 2 + 0.3
    props['f3'] = np.exp(-x) * (1 + y)
    props['f4'] = 2.0 - x + 3 * y * z
    return props


@functools.lru_cache(maxsize=None)
def brute_points(kind):
    rng = np.random.default_rng(37)
    s = brute_sources()
    if kind == 'sparse37':
        return tuple(rng.uniform(0.1, 0.9, (3, 37)))
    if kind == 'scattered130':
        return tuple(rng.uniform(0.05, 0.95, (3, 130)))
    if kind == 'outside130':
        return tuple(rng.uniform(-0.3, 1.3, (3, 130)))
    return (s['x'].copy(), s['y'].copy(), s['z'].copy())       # 'dense4097': the particle positions (r = 0 pairs)


@functools.lru_cache(maxsize=None)
def brute_force(kind, method):
    """O(M N) with numpy and the host kernel functions of pysph_amd.kernels"""
    from pysph_amd import kernels as K
    kernel = K.CubicSpline(dim=3)
    s, (px, py, pz) = brute_sources(), brute_points(kind)
    hp = s['h'].max()
    out = {f: np.zeros(px.size) for f in ('f0', 'f1', 'f2', 'f3', 'f4')}
    rs = kernel.radius_scale
    for a in range(0, px.size, 256):
        sl = slice(a, a + 256)
        dxx, dyy, dzz = [p[sl, None] - s[c][None, :] for p, c in zip((px, py, pz), 'xyz')]
        r2 = (dxx * dxx + dyy * dyy) + dzz * dzz
        nbr = (r2 < (rs * hp) ** 2) | (r2 < (rs * s['h'][None, :]) ** 2)
        r = np.sqrt(r2)
        hh = {'shepard': 0.5 * (hp + s['h'])[None, :], 'sph': 0.5 * (hp + s['h'])[None, :],
              'splash': hp * np.ones((1, s['h'].size)), 'splash_norm': s['h'][None, :]}[method]
        w = np.where(nbr, kernel.kernel(rij=r, h=hh), 0.0)
        if method != 'shepard':
            w = w * (s['m'] / s['rho'])[None, :]
        den = w.sum(axis=1)
        for f in out:
            v = (w * s[f][None, :]).sum(axis=1)
            if method in ('shepard', 'splash_norm'):
                v = np.where(den > 1e-12, v / np.where(den > 1e-12, den, 1.0), v)
            out[f][sl] = v
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('method', ['shepard', 'sph', 'splash', 'splash_norm'])
def test_sum_methods_equal_brute_force(method):
    from pysph_amd import kernels as K
    from pysph_amd.particle_array import ParticleArray
    from pysph_amd.tools import Interpolator
    pa = ParticleArray(name='fluid', **{AS.get(k, k): v.copy() for k, v in brute_sources().items()})
    fields = ['f0', 'f1', 'f2', 'f3', 'f4']
    interp = None
    for kind in ('sparse37', 'scattered130', 'dense4097', 'outside130'):
        px, py, pz = brute_points(kind)
        if interp is None:
            interp = Interpolator([pa], kernel=K.CubicSpline(dim=3), x=px, y=py, z=pz, method=method)
        else:
            interp.set_interpolation_points(px, py, pz)
        want = brute_force(kind, method)
        for f, got in zip(fields, interp.interpolate_many([AS[f] for f in fields])):
            err = rel_err(got, want[f])
            print(method, kind, f, 'rel_err %.3e' % err)
            assert got.shape == px.shape and err < TOL, (method, kind, f, err)
    interp.close()


# ---------------------------------------------------------------------------
# C. invariants
# ---------------------------------------------------------------------------
def lattice_array(n=10, seed=3):
    from pysph_amd.particle_array import get_particle_array
    rng = np.random.default_rng(seed)
    dx = 1.0 / n
    g = np.meshgrid(*[dx * (np.arange(n) + 0.5)] * 3, indexing='ij')
    x, y, z = [a.ravel() + 0.2 * dx * rng.uniform(-1, 1, n ** 3) for a in g]
    pa = get_particle_array(name='fluid', x=x, y=y, z=z, h=1.0 * dx * np.ones(n ** 3),
                            m=dx ** 3 * (1 + 0.05 * rng.uniform(-1, 1, n ** 3)),
                            rho=1 + 0.03 * rng.uniform(-1, 1, n ** 3))
    return pa, rng


@pytest.mark.gpu
def test_invariants_constant_and_linear_fields():
    from pysph_amd.kernels import Gaussian
    from pysph_amd.tools import Interpolator
    pa, rng = lattice_array()
    c, a, b = 3.7, 1.25, -2.5
    pa.p[:] = c                     # a constant field
    pa.u[:] = a + b * pa.x          # a linear one
    pts = np.concatenate([rng.uniform(0.35, 0.65, (3, 60)), rng.uniform(-1.0, -0.5, (3, 4))], axis=1)
    sh = Interpolator([pa], x=pts[0], y=pts[1], z=pts[2], method='shepard')
    assert isinstance(sh.kernel, Gaussian) and sh.kernel.dim == 3 and sh.dim == 3      # the default kernel
    got = sh.interpolate('p')
    # <= ~2000 terms x 2^-53 in numerator and denominator
    assert np.all(np.abs(got[:60] - c) <= 1e-12 * abs(c)) and np.all(got[60:] == 0.0)
    sh.close()
    o1 = Interpolator([pa], x=pts[0, :60], y=pts[1, :60], z=pts[2, :60], method='order1')
    val, gx, gy, gz = [o1.interpolate('u', comp=k) for k in range(4)]
    want = a + b * pts[0, :60]
    print('order1 linear: value %.3e gradient %.3e' % (rel_err(val, want), np.max(np.abs(gx - b)) / abs(b)))
    assert rel_err(val, want) < TOL and np.max(np.abs(gx - b)) < TOL * abs(b)
    assert np.max(np.abs(gy)) < TOL * abs(b) and np.max(np.abs(gz)) < TOL * abs(b)
    assert rel_err(o1.interpolate('x'), pts[0, :60]) < TOL
    with pytest.raises(RuntimeError):
        o1.interpolate('u', comp=4)
    o1.close()


# ---------------------------------------------------------------------------
# D. device-resident sources
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('method', ALL)
def test_device_resident_sources_are_not_touched(method):
    from pysph_amd import device as dev
    from pysph_amd.tools import Interpolator
    kernel, pts, fields, _ = case_setup('c1')
    arrays = case_arrays('c1')
    ctx = dev.HipContext(0)
    for pa in arrays:
        dev.attach(pa, ctx).push(*[k for k, v in pa.properties.items() if v.dtype == np.float64])
    n = arrays[0].get_number_of_particles()
    rho0 = arrays[0].gpu.pull_into('rho', np.empty(n))
    for pa in arrays:
        for v in pa.properties.values():
            if v.dtype == np.float64:
                v[:] = np.nan
    interp = Interpolator(arrays, kernel=kernel, x=pts[0], y=pts[1], z=pts[2], method=method, ctx=ctx, sync=False)
    g = golden()
    for comp in (range(4) if method == 'order1' else (0,)):
        for f, got in zip(fields, interp.interpolate_many([AS[f] for f in fields], comp=comp)):
            want = g['c1/out/%s/%s' % (method, f)]
            err = rel_err(got, want[comp::4] if method == 'order1' else want)
            assert err < TOL, (method, f, comp, err)
    for pa in arrays:
        for v in pa.properties.values():
            if v.dtype == np.float64:
                assert np.all(np.isnan(v))
    assert np.array_equal(arrays[0].gpu.pull_into('rho', np.empty(n)), rho0)      # 'order1' keeps its density to itself
    names = interp.interpolate_many([AS[fields[2]]], pull=False)       # stays on the device, as properties of interp.pa
    assert names == ([('ip0', 'ip1', 'ip2', 'ip3')] if method == 'order1' else ['ip0'])
    want = g['c1/out/%s/%s' % (method, fields[2])]
    for k, name in enumerate(names[0] if method == 'order1' else names):
        got = interp.pa.gpu.pull_into(name, np.empty(pts[0].size))
        assert rel_err(got, want[k::4] if method == 'order1' else want) < TOL, name
    ctx.close()


# ---------------------------------------------------------------------------
# E. moment cache and update()
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_order1_moment_cache_and_update():
    from pysph_amd.tools import Interpolator
    kernel, pts, fields, _ = case_setup('c1')
    arrays = case_arrays('c1')
    interp = Interpolator(arrays, kernel=kernel, x=pts[0], y=pts[1], z=pts[2], method='order1')
    count = lambda key: interp.ctx.timer_get(key)[1]
    m0, s0 = count('n_interp_moment'), count('n_interp_sweep')
    fields = [AS[f] for f in fields]
    first = interp.interpolate_many(fields, comp=1)
    assert count('n_interp_moment') == m0 + 1 and count('n_interp_sweep') == s0 + 2     # 5 properties: 2 sweeps
    second = interp.interpolate_many(fields, comp=1)
    assert count('n_interp_moment') == m0 + 1 and count('n_interp_sweep') == s0 + 4
    for a, b in zip(first, second):
        assert np.array_equal(a, b)
    rng = np.random.default_rng(8)
    pa = arrays[0]
    for c in 'xyz':
        pa.properties[c] += 0.01 * rng.uniform(-1, 1, pa.get_number_of_particles())
    interp.update()
    moved = interp.interpolate_many(fields, comp=0)
    assert count('n_interp_moment') == m0 + 2
    fresh = Interpolator(case_arrays_like(pa), kernel=kernel, x=pts[0], y=pts[1], z=pts[2], method='order1')
    for f, a, b in zip(fields, moved, fresh.interpolate_many(fields, comp=0)):
        assert rel_err(a, b) < TOL, f
    interp.close()
    fresh.close()


def case_arrays_like(pa):
    from pysph_amd.particle_array import ParticleArray
    return [ParticleArray(name=pa.name, **{k: v.copy() for k, v in pa.properties.items() if v.dtype == np.float64})]


@pytest.mark.gpu
def test_methods_alternate_on_one_context_without_a_neighbour_update():
    """order1, then sph (which writes its own m / rho), then order1 again from the kept moments: every call gives the
    golden values -- through the C-ABI with one grid, and through one Interpolator whose method is switched"""
    from pysph_amd.tools import Interpolator
    kernel, pts, fields, _ = case_setup('c1')
    g = golden()
    from pysph_amd import device as dev
    arrays = case_arrays('c1')
    ctx = dev.HipContext(0)
    for pa in arrays:       # device-resident sources: nothing is pushed between the calls (a push of m ends the cache)
        dev.attach(pa, ctx).push(*[k for k, v in pa.properties.items() if v.dtype == np.float64])
    interp = Interpolator(arrays, kernel=kernel, x=pts[0], y=pts[1], z=pts[2], method='order1', ctx=ctx, sync=False)
    interp.invalidate = False       # nothing else evaluates on this context: the grid stays
    count = lambda: ctx.timer_get('n_interp_moment')[1]
    m0 = count()
    for method in ('order1', 'sph', 'splash_norm', 'order1', 'shepard', 'order1'):
        interp.method = method
        for comp in ((0, 2) if method == 'order1' else (0,)):
            for f, got in zip(fields, interp.interpolate_many([AS[f] for f in fields], comp=comp)):
                want = g['c1/out/%s/%s' % (method, f)]
                err = rel_err(got, want[comp::4] if method == 'order1' else want)
                assert err < TOL, (method, f, comp, err)
    assert count() == m0 + 1            # the moments were made once and survived the other methods
    interp.close()
    ctx.close()


# ---------------------------------------------------------------------------
# F. periodic domain
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_periodic_shepard_equals_minimum_image_brute_force():
    from pysph_amd import device as dev
    from pysph_amd import kernels as K
    from pysph_amd.domain import HipDomainManager
    from pysph_amd.particle_array import get_particle_array
    from pysph_amd.tools import Interpolator
    rng = np.random.default_rng(12)
    n, dx = 40, 1.0 / 40
    g = np.meshgrid(*[dx * (np.arange(n) + 0.5)] * 2, indexing='ij')
    x, y = [a.ravel() + 0.2 * dx * rng.uniform(-1, 1, n * n) for a in g]
    h = 1.2 * dx
    f = np.sin(2 * np.pi * x) * np.cos(2 * np.pi * y) + 0.3 * rng.uniform(-1, 1, n * n)
    pa = get_particle_array(name='fluid', x=x, y=y, h=h * np.ones(n * n), m=dx * dx * np.ones(n * n), rho=np.ones(n * n))
    pa.p[:] = f
    kernel = K.QuinticSpline(dim=2)
    # points within one h of the periodic faces (and a few inside)
    edge = np.concatenate([rng.uniform(0.0, h, 30), rng.uniform(1.0 - h, 1.0, 30)])
    px = np.concatenate([edge, rng.uniform(0, 1, 60), rng.uniform(0.2, 0.8, 10)])
    py = np.concatenate([rng.uniform(0, 1, 60), edge, rng.uniform(0.2, 0.8, 10)])
    ctx = dev.HipContext(0)
    dev.attach(pa, ctx).push('x', 'y', 'z', 'h', 'm', 'rho', 'p')
    dom = HipDomainManager(ctx=ctx, xmin=0.0, xmax=1.0, ymin=0.0, ymax=1.0, periodic_in_x=True, periodic_in_y=True)
    interp = Interpolator([pa], kernel=kernel, x=px, y=py, domain_manager=dom, method='shepard', ctx=ctx, sync=False)
    got = interp.interpolate('p')
    ddx = px[:, None] - x[None, :]
    ddy = py[:, None] - y[None, :]
    ddx -= np.round(ddx)
    ddy -= np.round(ddy)
    r = np.sqrt(ddx * ddx + ddy * ddy)
    w = np.where(r < kernel.radius_scale * h, kernel.kernel(rij=r, h=h), 0.0)
    want = (w * f[None, :]).sum(axis=1) / w.sum(axis=1)
    err = rel_err(got, want)
    print('periodic shepard rel_err %.3e' % err)
    assert err < TOL
    ctx.close()


# ---------------------------------------------------------------------------
# G. a probe does not disturb the simulation it looks at
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_probe_in_a_shared_context_does_not_change_the_dam_break():
    from pysph_amd.examples import dam_break_3d as db
    from pysph_amd.tools import Interpolator
    rng = np.random.default_rng(5)
    pts = np.stack([rng.uniform(0.0, 3.2, 500), rng.uniform(-0.5, 0.5, 500), rng.uniform(0.0, 1.0, 500)])
    seen = []

    def probe(step, t, arrays, ctx):
        if step % 2:
            return
        if not seen:
            seen.append(Interpolator(arrays, kernel=db.create_kernel(), x=pts[0], y=pts[1], z=pts[2], method='shepard',
                                     ctx=ctx, sync=False))
        p, u = seen[0].interpolate_many(['p', 'u'])
        assert p.shape == (500,) and np.all(np.isfinite(p)) and np.all(np.isfinite(u))
        seen.append(p)

    plain, _ = db.run(dx=0.1, n_steps=6, adaptive=False)
    probed, _ = db.run(dx=0.1, n_steps=6, adaptive=False, probe=probe)
    assert len(seen) == 4 and np.abs(seen[-1]).max() > 0
    for a, b in zip(plain, probed):
        assert a.name == b.name
        for key, va in a.properties.items():
            if va.dtype == np.float64:
                err = rel_err(b.properties[key], va)
                assert err < TOL, (a.name, key, err)


# ---------------------------------------------------------------------------
# H. C-ABI errors
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_cabi_errors():
    from pysph_amd import device as dev
    from pysph_amd import kernels as K
    from pysph_amd.nnps import HipNNPS
    from pysph_amd.particle_array import get_particle_array
    pa, rng = lattice_array(6)
    pts = get_particle_array(name='interpolate', x=rng.random(20), y=rng.random(20), z=rng.random(20), h=pa.h[0] * np.ones(20))
    ctx = dev.HipContext(0)
    lib = ctx.lib
    hs, hd = dev.attach(pa, ctx), dev.attach(pts, ctx)
    hs.push()
    hd.push('x', 'y', 'z', 'h')
    k = K.CubicSpline(dim=3)
    ck = dev.SphKernel(K.kernel_id(k), 3, k.fac, k.radius_scale, k.get_deltap())
    src = (C.c_int * 1)(hs.array_id)
    prop = (C.c_int * 1)(dev.prop_id('rho'))
    out = (C.c_int * 1)(dev.prop_register('ip0'))

    def call(method=0, dest=None, nsrc=1):
        return lib.sph_interpolate(ctx._h, C.byref(ck), method, hd.array_id if dest is None else dest, nsrc, src, 1, prop, out,
                                   None, 0)
    assert call() == -6 and b'sph_nnps_update' in lib.sph_last_error()          # SPH_ERR_STATE: no neighbour update yet
    HipNNPS(3, [pa, pts], radius_scale=k.radius_scale, ctx=ctx, sync=False)
    assert call() == 0
    assert call(method=5) == -2 and b'method' in lib.sph_last_error()           # SPH_ERR_ARG
    assert call(dest=7) == -2 and b'destination' in lib.sph_last_error()
    assert call(dest=hs.array_id) == -2 and lib.sph_last_error()               # a source as destination
    assert call(nsrc=dev.MAX_ARRAYS) == -2 and lib.sph_last_error()
    # results straight to the host, no destination property: the same values
    host = np.empty((1, 20))
    assert lib.sph_interpolate(ctx._h, C.byref(ck), 0, hd.array_id, 1, src, 1, prop, None, host.ctypes.data_as(dev._PD), 20) == 0
    assert np.array_equal(host[0], hd.pull_into('ip0', np.empty(20)))
    assert lib.sph_interpolate(ctx._h, C.byref(ck), 0, hd.array_id, 1, src, 1, prop, None, host.ctypes.data_as(dev._PD), 21) == -2
    ctx.close()
