"""The EDAC scheme on the GPU against the reference's own classes (tests/golden/edac_*.npz, made by
tests/golden/make_edac_golden.py): the hand-written force family and average pressure, the generated wall equations
behind and before them, both steppers, three device-resident PEC steps, the name clash with the WCSPH / TVF classes,
periodic images and the refusal of slab-decomposed arrays."""
import json

import numpy as np
import pytest

from conftest import load_golden
from helpers import rel_err
import test_edac as TE

TOL = 1e-10            # BASELINE.json north_star, as tests/test_hip_parity.py
TOL_F32 = 5e-5         # test_fp32_arithmetic_vs_golden
EVAL_CASES = TE.EVAL_CASES


class _View(object):
    """the keys of one prefix of a golden file (edac_kernels.npz holds one case per kernel class)"""

    def __init__(self, g, prefix):
        self._g, self._p = g, prefix
        self.files = [k[len(prefix):] for k in g.files if k.startswith(prefix)]

    def __getitem__(self, key):
        return self._g[self._p + key]


def arrays_of(g, which='in'):
    from pysph_amd.particle_array import ParticleArray
    names = []
    for key in g.files:
        parts = key.split('/')
        if parts[0] == which and parts[1] not in names:
            names.append(parts[1])
    out = []
    for name in names:
        props = dict((key.split('/')[2], g[key].copy()) for key in g.files if key.startswith('%s/%s/' % (which, name)))
        pa = ParticleArray(name=name, **props)
        pa.set_num_real_particles(int(g['nreal/%s' % name]))
        out.append(pa)
    return out


def kernel_of(g):
    from pysph_amd import kernels as K
    return getattr(K, str(g['kernel']))(dim=int(json.loads(str(g['scheme']))['dim']))


def stored_props(g, pa, which='in'):
    return [key.split('/')[2] for key in g.files if key.startswith('%s/%s/' % (which, pa.name))]


def push_all(g, arrays):
    for pa in arrays:
        pa.gpu.push(*stored_props(g, pa))           # the user properties (ap, pavg, wij, ...) by name


def pull_all(g, arrays):
    """outputs AND inputs: nothing but the outputs may have changed"""
    for pa in arrays:
        pa.gpu.pull(*stored_props(g, pa))


def evaluator(g, arrays, equations=None, variant=6, f32=False):
    from pysph_amd import device as dev
    from pysph_amd.acceleration_eval import AccelerationEval, SPHCompiler
    from pysph_amd.nnps import HipNNPS
    kernel = kernel_of(g)
    ctx = dev.HipContext(0)
    ctx.set_option('pair_variant', variant)
    if f32:
        ctx.set_option('arith_f32', 1)
    a_eval = AccelerationEval(arrays, TE.equations_of(g) if equations is None else equations, kernel)
    SPHCompiler(a_eval, ctx=ctx, sync='manual').compile()
    push_all(g, arrays)
    nnps = HipNNPS(kernel.dim, arrays, radius_scale=kernel.radius_scale, ctx=ctx, sync=False)
    a_eval.set_nnps(nnps)
    return a_eval, nnps, ctx


def check_nnps(nnps, g, prefix):
    assert nnps.cell_size == float(g[prefix + '/cell_size'])
    assert np.array_equal(nnps.xmin, g[prefix + '/xmin'])
    assert np.array_equal(nnps.xmax, g[prefix + '/xmax'])
    assert np.array_equal(nnps.ncells_per_dim, g[prefix + '/ncells_per_dim'])
    assert nnps.n_cells == int(g[prefix + '/n_cells'])


def check_all(case, g, arrays, which, tol, what):
    """EVERY stored property of every array, every element"""
    worst, n = 0.0, 0
    for pa in arrays:
        keys = [k for k in g.files if k.startswith('%s/%s/' % (which, pa.name))]
        assert keys
        for key in keys:
            prop = key.split('/')[2]
            want, got = g[key], pa.properties[prop]
            assert got.shape == want.shape, (case, key)
            e = rel_err(got, want)
            print('%s %s %s/%s: %.3e' % (case, what, pa.name, prop, e))
            worst = max(worst, e)
            assert e < tol, (case, what, pa.name, prop, e)
            n += want.size
    print('%s %s: max rel err %.3e over %d elements' % (case, what, worst, n))
    return worst


def run_case(case, g, variant=6, f32=False, equations=None, tol=TOL):
    arrays = arrays_of(g)
    a_eval, nnps, ctx = evaluator(g, arrays, equations, variant, f32)
    nnps.update()
    check_nnps(nnps, g, 'nnps')
    t, dt = float(g['t']), float(g['dt'])
    a_eval.compute(t, dt)
    pull_all(g, arrays)
    what = 'arith_f32' if f32 else 'variant %d' % variant
    worst = check_all(case, g, arrays, 'out', tol, what)
    if 'nnps2/cell_size' in g.files:
        fluid = arrays[0]
        for a, b in zip('xyz', 'uvw'):      # as the generator: the fluid moves by dt u
            fluid.properties[a][:] = g['in/fluid/' + a] + dt * g['in/fluid/' + b]
        fluid.gpu.push('x', 'y', 'z')
        nnps.update()
        check_nnps(nnps, g, 'nnps2')
        a_eval.compute(t + dt, dt)
        pull_all(g, arrays)
        worst = max(worst, check_all(case, g, arrays, 'out2', tol, what + ', second evaluation'))
    ctx.close()
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize('variant', [6, 0])
@pytest.mark.parametrize('case', EVAL_CASES)
def test_edac_parity_with_reference_golden(case, variant):
    """fp64, both schedules: NNPS scalars equal, every property of every array within 1e-10 of the field maximum
    after the first evaluation and, for edac_ext3d, after the update and the second one; inputs unchanged"""
    run_case(case, load_golden(case + '.npz'), variant)


@pytest.mark.gpu
@pytest.mark.parametrize('case', EVAL_CASES)
def test_edac_fp32_arithmetic(case):
    """option arith_f32 against the fp64 vectors at the project's fp32 bound, every element; really in float"""
    worst = run_case(case, load_golden(case + '.npz'), 6, f32=True, tol=TOL_F32)
    assert worst > 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize('kname', json.loads(str(load_golden('edac_kernels.npz')['kernels'])))
def test_edac_every_smoothing_kernel(kname):
    """all ten kernel ids, fp64: the external branch without walls on a 4^3 block (a 40-particle line for the 1-D
    classes)"""
    g = _View(load_golden('edac_kernels.npz'), kname + '/')
    assert str(g['kernel']) == kname
    run_case('edac_kernels ' + kname, g)


@pytest.mark.gpu
@pytest.mark.parametrize('tag,kind', [('edac', 6), ('edac_tvf', 7)])
def test_edac_steppers_vs_reference_golden(tag, kind):
    """both stage kernels against the reference's stepper methods, stage by stage; fma contraction may move the last
    bit (1e-15 relative, as tests/test_reference_integrators.py holds the other steppers to)"""
    import ctypes as C
    from pysph_amd import device as dev
    from pysph_amd.particle_array import ParticleArray
    g = load_golden('edac_steppers.npz')
    dt = float(g['dt'])
    props = dict((k[3:], g[k].copy()) for k in g.files if k.startswith('in/'))
    pa = ParticleArray(name='fluid', **props)
    ctx = dev.HipContext(0)
    dev.attach(pa, ctx).push(*sorted(props))
    for stage, meth in ((0, 'initialize'), (1, 'stage1'), (2, 'stage2')):
        dev._check(ctx.lib.sph_integrate_stage(ctx._h, pa.gpu.array_id, kind, stage, C.c_double(dt)))
        pa.gpu.pull(*sorted(props))
        for k in sorted(props):
            ref = g['%s/%s/%s' % (tag, meth, k)]
            assert np.allclose(pa.properties[k], ref, rtol=1e-15, atol=1e-16), (tag, meth, k)
    ctx.close()


@pytest.mark.gpu
def test_edac_three_device_resident_pec_steps():
    """the edac_ext3d particles through three PEC steps with EDACStep on the device (neighbours rebuilt before every
    evaluation), every property of every array within 1e-10 of the field maximum of the reference's three steps"""
    from pysph_amd.integrator import PECIntegrator, EDACStep, setup_integrator
    g = load_golden('edac_steps.npz')
    arrays = arrays_of(g)
    a_eval, nnps, ctx = evaluator(g, arrays)
    integ = PECIntegrator(fluid=EDACStep())
    setup_integrator(integ, a_eval, nnps)
    t, dt = float(g['t']), float(g['dt'])
    for _ in range(int(g['meta/steps'])):
        integ.step(t, dt)
        t += dt
    pull_all(g, arrays)
    worst = check_all('edac_steps', g, arrays, 'out', TOL, 'three PEC steps')
    print('edac_steps: worst figure %.3e' % worst)
    assert not np.array_equal(arrays[0].x, g['in/fluid/x'])
    ctx.close()


def reference_named(groups):
    """the same equation objects as instances of classes NAMED like the reference's and living in a module NAMED
    like the reference's -- what a user who passes pysph's own EDAC objects hands over"""
    from pysph_amd import edac as ED
    clones = {}
    for grp in groups:
        for eq in grp.equations:
            cls = type(eq)
            if cls.__module__ == ED.__name__:
                if cls not in clones:
                    clone = type(cls.__name__, (cls,), {})
                    clone.__module__ = 'pysph.sph.wc.edac'
                    clones[cls] = clone
                eq.__class__ = clones[cls]
    return groups


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['edac_ext3d', 'edac_int3d_nosolid'])
def test_reference_named_classes_select_the_edac_kernels(case):
    """MomentumEquation / MomentumEquationPressureGradient of a module called pysph.sph.wc.edac are EDAC's, not the
    WCSPH / TVF namesakes: the EDAC kinds are selected and the golden is met"""
    from pysph_amd.equations import resolve_equation
    g = load_golden(case + '.npz')
    groups = reference_named(TE.equations_of(g))
    kinds = [resolve_equation(eq)[0] for eq in groups[-1].equations if type(eq).__name__.startswith('MomentumEquation')
             and type(eq).__module__ == 'pysph.sph.wc.edac']
    assert kinds == [31 if case == 'edac_ext3d' else 32]
    run_case(case + ' (reference-named classes)', g, equations=groups)


def _periodic_tiles(n1=16):
    """internal branch, no solids, on the unit square: the box, and its explicit 3 x 3 tiling with the central tile
    first"""
    rng = np.random.default_rng(71)
    dx = 1.0 / n1
    c = (np.arange(n1) + 0.5) * dx
    x, y = [a.ravel() for a in np.meshgrid(c, c, indexing='ij')]
    n = x.size
    rho0, c0 = 1.0, 10.0
    base = dict(x=x + 0.2 * dx * rng.uniform(-1, 1, n), y=y + 0.2 * dx * rng.uniform(-1, 1, n), z=np.zeros(n),
                u=rng.uniform(-1, 1, n), v=rng.uniform(-1, 1, n), w=np.zeros(n), h=1.0 * dx * np.ones(n),
                m=rho0 * dx * dx * np.ones(n), p=0.05 * rho0 * c0 * c0 * rng.uniform(-1, 1, n))
    base['uhat'] = base['u'] + 0.1 * rng.uniform(-1, 1, n)
    base['vhat'] = base['v'] + 0.1 * rng.uniform(-1, 1, n)
    base['what'] = np.zeros(n)
    shifts = [(0, 0)] + [(i, j) for i in (-1, 0, 1) for j in (-1, 0, 1) if (i, j) != (0, 0)]
    tiled = dict((k, np.tile(v, 9)) for k, v in base.items())
    tiled['x'] = np.concatenate([base['x'] + i for i, j in shifts])
    tiled['y'] = np.concatenate([base['y'] + j for i, j in shifts])
    kw = dict(fluids=['fluid'], solids=[], dim=2, c0=c0, nu=0.02, rho0=rho0, pb=rho0 * c0 * c0, h=dx, alpha=0.1, gx=0.5)
    return base, tiled, kw, n


OUT_INT = ('rho', 'V', 'pavg', 'nnbr', 'au', 'av', 'aw', 'auhat', 'avhat', 'awhat', 'ap')


def _run_box(props, kw, periodic):
    from pysph_amd import device as dev
    from pysph_amd import kernels as K
    from pysph_amd.acceleration_eval import AccelerationEval, SPHCompiler
    from pysph_amd.domain import HipDomainManager
    from pysph_amd.edac import EDACScheme
    from pysph_amd.nnps import HipNNPS
    from pysph_amd.particle_array import ParticleArray
    pa = ParticleArray(name='fluid', **props)
    s = EDACScheme(**kw)
    s.setup_properties([pa])
    kernel = K.QuinticSpline(dim=2)
    assert 1.0 > 2 * kernel.radius_scale * kw['h']         # the box is wider than twice the kernel radius
    ctx = dev.HipContext(0)
    dev.attach(pa, ctx).push(*[p for p in pa.properties if pa.properties[p].dtype == np.float64])
    a_eval = AccelerationEval([pa], s.get_equations(), kernel)
    SPHCompiler(a_eval, ctx=ctx, sync='manual').compile()
    dkw = {}
    if periodic:
        dkw = dict(domain=HipDomainManager(ctx=ctx, xmin=0, xmax=1, ymin=0, ymax=1, periodic_in_x=True,
                                           periodic_in_y=True))
    nnps = HipNNPS(2, [pa], radius_scale=kernel.radius_scale, ctx=ctx, sync=False, **dkw)
    a_eval.set_nnps(nnps)
    nnps.update()
    a_eval.compute(0.0, 1e-4)
    if periodic:
        assert pa.gpu.get_number_of_particles() > pa.gpu.get_number_of_particles(True)
    pa.gpu.pull(*OUT_INT)
    ctx.close()
    return pa


@pytest.mark.gpu
def test_edac_periodic_box_equals_its_explicit_tiling():
    """internal branch without solids on a periodic 16 x 16 box under HipDomainManager against the same equations on
    the explicit 3 x 3 tiling without periodicity: the central tile's rows within 1e-10 of the field maximum (the
    sums associate differently: not bit-equal).  rho, V, pavg of the image rows come from the real=False group."""
    base, tiled, kw, n = _periodic_tiles()
    box = _run_box(base, kw, True)
    ref = _run_box(tiled, kw, False)
    for p in OUT_INT:
        want, got = ref.properties[p][:n], box.properties[p][:n]
        e = rel_err(got, want)
        print('periodic %s: %.3e' % (p, e))
        assert e < TOL, (p, e)
        if p not in ('aw', 'awhat'):
            assert np.abs(want).max() > 0.0, p
    assert np.all(ref.properties['nnbr'][:n] >= 1.0)


@pytest.mark.gpu
def test_edac_on_a_slab_decomposed_array_is_refused():
    """p is integrated state and the halo messages carry no p / V / uhat set for it: NotImplementedError naming the
    reason before anything is launched -- nothing is written"""
    g = load_golden('edac_int3d_nosolid.npz')
    arrays = arrays_of(g)
    a_eval, nnps, ctx = evaluator(g, arrays)
    arrays[0].slab_decomposed = True         # what a slab HipParallelManager marks its array with (parallel.py)
    nnps.update()
    with pytest.raises(NotImplementedError, match='integrated state'):
        a_eval.compute(float(g['t']), float(g['dt']))
    pull_all(g, arrays)
    for p in stored_props(g, arrays[0]):
        assert np.array_equal(arrays[0].properties[p], g['in/fluid/' + p]), p
    ctx.close()


def prebuild():
    """the generated families of this module (the wall equations of the two cases with walls, both precisions),
    built without a GPU"""
    from pysph_amd import codegen
    from pysph_amd import kernels as K
    from pysph_amd.acceleration_eval import AccelerationEval, _CGroup

    def every():
        count = 0
        for case in ('edac_ext3d', 'edac_int2d'):
            g = load_golden(case + '.npz')
            arrays = arrays_of(g)
            kernel = kernel_of(g)
            a = AccelerationEval(arrays, TE.equations_of(g), kernel)
            ids = dict((pa.name, i) for i, pa in enumerate(arrays))
            amap = dict((pa.name, pa) for pa in arrays)
            for grp in a.equation_groups:
                for u in _CGroup(grp, ids, amap, K.kernel_id(kernel)).units:
                    if hasattr(u, 'fam'):
                        f32 = u.fam.flavour_f32() if (u.fam.sources and u.fam.bodies['loop'] and not u.fam.abs_src_pos) else None
                        if f32 is not None:
                            f32.load()
                        count += 1
        return count
    codegen.DEFERRED = []
    every()
    codegen.build_deferred()
    return every()
