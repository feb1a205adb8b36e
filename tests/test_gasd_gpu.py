"""Gas dynamics on the GPU against the reference's own classes (tests/golden/gasd_*.npz, made by
tests/golden/make_gasd_golden.py): the iterated density sweep with its Newton step for h, the ideal-gas EOS, the MPM
force sweep, the gsph list, the stage kernel, three device-resident PEC steps, all ten smoothing kernels, fp32
arithmetic, the name clash of the three SummationDensity classes and the refusal of slab-decomposed arrays.

Measured on an MI355X (the figures the bounds below come from are in DESIGN.md, section 7g)."""
import ctypes as C
import json

import numpy as np
import pytest

from conftest import load_golden
from helpers import rel_err
import test_gasd as TG

TOL = 1e-10            # BASELINE.json north_star, as tests/test_hip_parity.py and tests/test_edac_gpu.py
TOL_F32 = 5e-5         # test_fp32_arithmetic_vs_golden
EVAL_CASES = TG.EVAL_CASES
# max |h_f32 - h_golden| / h0 of the density iteration in fp32 arithmetic, measured per case;
# the tests assert four times these.  (A convergence decision may fall the other way in fp32: h then differs by up to
# one Newton step of a nearly converged particle, below htol.)
H_F32_MEASURED = {'gasd_1d': 1.383e-06, 'gasd_2d': 3.732e-07, 'gasd_3d': 2.869e-07}


class _View(object):
    """the keys of one prefix of a golden file (gasd_kernels.npz holds one case per kernel class)"""

    def __init__(self, g, prefix):
        self._g, self._p = g, prefix
        self.files = [k[len(prefix):] for k in g.files if k.startswith(prefix)]

    def __getitem__(self, key):
        return self._g[self._p + key]


def arrays_of(g, which='in'):
    from pysph_amd.particle_array import ParticleArray
    props = dict((key.split('/')[2], g[key].copy()) for key in g.files if key.startswith('%s/fluid/' % which))
    pa = ParticleArray(name='fluid', **props)
    pa.set_num_real_particles(int(g['nreal/fluid']))
    return [pa]


def scheme_kw(g):
    return json.loads(str(g['scheme']))


def kernel_of(g):
    from pysph_amd import kernels as K
    return getattr(K, str(g['kernel']))(dim=int(scheme_kw(g)['dim']))


def stored_props(g, pa, which='in'):
    return [key.split('/')[2] for key in g.files if key.startswith('%s/%s/' % (which, pa.name))]


def push_all(g, arrays):
    for pa in arrays:
        pa.gpu.push(*stored_props(g, pa))           # the user properties (omega, alpha1, dwdh, ...) by name


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
    a_eval = AccelerationEval(arrays, TG.equations_of(g) if equations is None else equations, kernel)
    SPHCompiler(a_eval, ctx=ctx, sync='manual').compile()
    push_all(g, arrays)
    nnps = HipNNPS(kernel.dim, arrays, radius_scale=kernel.radius_scale, ctx=ctx, sync=False)
    a_eval.set_nnps(nnps)
    return a_eval, nnps, ctx


def check_nnps(nnps, g, prefix):
    """the grid behind the last neighbour update of the evaluation: built from the h the iteration ended with, which
    equals the reference's to rounding, not to the bit"""
    assert nnps.cell_size == pytest.approx(float(g[prefix + '/cell_size']), rel=1e-12)
    assert np.allclose(nnps.xmin, g[prefix + '/xmin'], rtol=1e-12, atol=1e-14)
    assert np.allclose(nnps.xmax, g[prefix + '/xmax'], rtol=1e-12, atol=1e-14)
    assert np.array_equal(nnps.ncells_per_dim, g[prefix + '/ncells_per_dim'])
    assert nnps.n_cells == int(g[prefix + '/n_cells'])


def check_all(case, g, arrays, which, tol, what, skip=()):
    """EVERY stored property of every array, every element"""
    worst, n = 0.0, 0
    for pa in arrays:
        keys = [k for k in g.files if k.startswith('%s/%s/' % (which, pa.name))]
        assert keys
        for key in keys:
            prop = key.split('/')[2]
            if prop in skip:
                continue
            want, got = g[key], pa.properties[prop]
            assert got.shape == want.shape, (case, key)
            e = rel_err(got, want)
            print('%s %s %s/%s: %.3e' % (case, what, pa.name, prop, e))
            worst = max(worst, e)
            assert e < tol, (case, what, pa.name, prop, e)
            n += want.size
    print('%s %s: max rel err %.3e over %d elements' % (case, what, worst, n))
    return worst


def iterations(a_eval):
    counts = list(a_eval.c_acceleration_eval.iteration_counts.values())
    assert len(counts) == 1
    return counts[0]


def run_case(case, g, variant=6, equations=None, tol=TOL):
    from pysph_amd import device as dev
    arrays = arrays_of(g)
    a_eval, nnps, ctx = evaluator(g, arrays, equations, variant)
    nnps.update()
    t, dt = float(g['t']), float(g['dt'])
    a_eval.compute(t, dt)
    pull_all(g, arrays)
    what = 'variant %d' % variant
    worst = check_all(case, g, arrays, 'out', tol, what)
    check_nnps(nnps, g, 'nnps')
    mpm = scheme_kw(g).get('adaptive_h_scheme', 'mpm') == 'mpm'
    if mpm:
        assert iterations(a_eval) == int(g['meta/iterations']), (case, iterations(a_eval))
        assert np.all(arrays[0].properties['converged'] == 1.0)
    if 'nnps2/cell_size' in g.files:
        fluid = arrays[0]
        for a, b in zip('xyz', 'uvw'):      # as the generator: the particles move by dt u, then the stepper's initialize
            fluid.properties[a][:] = g['in/fluid/' + a] + dt * g['in/fluid/' + b]
        fluid.gpu.push('x', 'y', 'z')
        dev._check(ctx.lib.sph_integrate_stage(ctx._h, fluid.gpu.array_id, 8, 0, C.c_double(dt)))
        nnps.update()
        a_eval.compute(t + dt, dt)
        pull_all(g, arrays)
        worst = max(worst, check_all(case, g, arrays, 'out2', tol, what + ', second evaluation'))
        check_nnps(nnps, g, 'nnps2')
        assert iterations(a_eval) == int(g['meta/second_iterations'])
    ctx.close()
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize('variant', [6, 0])
@pytest.mark.parametrize('case', EVAL_CASES)
def test_gasd_parity_with_reference_golden(case, variant):
    """fp64, both schedules: every property of every particle within 1e-10 of the field maximum after the whole
    evaluation -- the density iteration with the SAME number of iterations as the reference, the EOS and the force
    sweep -- and, for gasd_3d, after moving, the stage kernel's initialize and a second evaluation.  The particles
    that converged before the last iteration leave with the raw arho, those of the last with arho * omega: both are
    in the vectors (meta/n_converged_early, meta/n_converged_last)."""
    g = load_golden(case + '.npz')
    assert int(g['meta/n_converged_early']) * 10 >= int(g['nreal/fluid']) and int(g['meta/n_converged_last']) >= 1
    run_case(case, g, variant)


@pytest.mark.gpu
def test_gasd_gsph_group_list():
    """adaptive_h_scheme='gsph': scale h, sum, h from the volume, sum again -- the two no-source h kernels and the
    density sweep without iteration, then the EOS and the forces"""
    g = load_golden('gasd_gsph_h.npz')
    run_case('gasd_gsph_h', g)


@pytest.mark.gpu
@pytest.mark.parametrize('kname', json.loads(str(load_golden('gasd_kernels.npz')['kernels'])))
def test_gasd_every_smoothing_kernel(kname):
    """all ten kernel ids, fp64, WI / DWI / GHI / DWJ and DWIJ of each: a 4^3 block (a 40-particle line for the 1-D
    classes) with h +-10 %, both switches updating"""
    g = _View(load_golden('gasd_kernels.npz'), kname + '/')
    assert str(g['kernel']) == kname
    run_case('gasd_kernels ' + kname, g)


@pytest.mark.gpu
@pytest.mark.parametrize('case', EVAL_CASES)
def test_gasd_fp32_force_group(case):
    """option arith_f32, EOS and force group at the golden's converged state (h, rho, omega pushed): every property
    within the project's fp32 bound of 5e-5 of the field maximum; really in float"""
    g = load_golden(case + '.npz')
    arrays = arrays_of(g, 'out')
    groups = TG.equations_of(g)[-3:]
    assert [e.name for grp in groups for e in grp.equations] == ['IdealGasEOS', 'MPMAccelerations']
    a_eval, nnps, ctx = evaluator(g, arrays, groups, f32=True)
    nnps.update()
    a_eval.compute(float(g['t']), float(g['dt']))
    pull_all(g, arrays)
    worst = check_all(case, g, arrays, 'out', TOL_F32, 'arith_f32 force group')
    assert worst > 1e-9
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize('case', EVAL_CASES)
def test_gasd_fp32_density_iteration(case):
    """option arith_f32, the whole evaluation: the iteration converges below max_iterations, and h ends within four
    times the measured distance from the fp64 vectors (in units of h0)"""
    g = load_golden(case + '.npz')
    kw = scheme_kw(g)
    arrays = arrays_of(g)
    a_eval, nnps, ctx = evaluator(g, arrays, f32=True)
    nnps.update()
    a_eval.compute(float(g['t']), float(g['dt']))
    pull_all(g, arrays)
    n_it = iterations(a_eval)
    err = float(np.max(np.abs(arrays[0].properties['h'] - g['out/fluid/h']) / g['in/fluid/h0']))
    htol = kw.get('density_iteration_tolerance', 1e-3)
    print('%s arith_f32 density iteration: %d iterations (fp64 %d), max |h - h_golden| / h0 = %.3e (htol %.1e)'
          % (case, n_it, int(g['meta/iterations']), err, htol))
    ctx.close()
    assert n_it < kw['max_density_iterations']
    assert np.all(arrays[0].properties['converged'] == 1.0)
    assert err < 10 * htol                       # beyond this it is a defect, whatever was measured
    assert err < 4 * H_F32_MEASURED[case], (case, err)


@pytest.mark.gpu
def test_gasd_stepper_vs_reference_golden():
    """the stage kernel against the reference's stepper methods, stage by stage; fma contraction may move the last
    bit (1e-15 relative, as tests/test_reference_integrators.py holds the other steppers to)"""
    from pysph_amd import device as dev
    from pysph_amd.particle_array import ParticleArray
    g = load_golden('gasd_steppers.npz')
    dt = float(g['dt'])
    props = dict((k[3:], g[k].copy()) for k in g.files if k.startswith('in/'))
    pa = ParticleArray(name='fluid', **props)
    ctx = dev.HipContext(0)
    dev.attach(pa, ctx).push(*sorted(props))
    for stage, meth in ((0, 'initialize'), (1, 'stage1'), (2, 'stage2')):
        dev._check(ctx.lib.sph_integrate_stage(ctx._h, pa.gpu.array_id, 8, stage, C.c_double(dt)))
        pa.gpu.pull(*sorted(props))
        for k in sorted(props):
            ref = g['gasd/%s/%s' % (meth, k)]
            assert np.allclose(pa.properties[k], ref, rtol=1e-15, atol=1e-16), (meth, k)
    assert np.all(g['gasd/initialize/converged'] == 0.0) and np.all(g['gasd/initialize/omega'] == 1.0)
    ctx.close()


@pytest.mark.gpu
def test_gasd_three_device_resident_pec_steps():
    """the gasd_3d particles through three PEC steps with GasDFluidStep on the device -- no host pull between the
    steps, neighbours rebuilt before every evaluation and inside every density iteration -- every property of every
    particle within 1e-10 of the field maximum of the reference's three steps, the same iterations per step"""
    from pysph_amd.integrator import PECIntegrator, GasDFluidStep, setup_integrator
    g = load_golden('gasd_steps.npz')
    arrays = arrays_of(g)
    a_eval, nnps, ctx = evaluator(g, arrays)
    integ = PECIntegrator(fluid=GasDFluidStep())
    setup_integrator(integ, a_eval, nnps)
    t, dt = float(g['t']), float(g['dt'])
    its = []
    for _ in range(int(g['meta/steps'])):
        integ.step(t, dt)
        its.append(iterations(a_eval))
        t += dt
    pull_all(g, arrays)
    worst = check_all('gasd_steps', g, arrays, 'out', TOL, 'three PEC steps')
    print('gasd_steps: worst figure %.3e, iterations %s' % (worst, its))
    assert its == [int(v) for v in g['meta/iterations_per_step']]
    assert not np.array_equal(arrays[0].x, g['in/fluid/x'])
    ctx.close()


def reference_named(groups):
    """the same equation objects as instances of classes NAMED like the reference's and living in a module NAMED
    like the reference's -- what a user who passes pysph's own gas-dynamics objects hands over"""
    from pysph_amd import gas_dynamics as GD
    clones = {}
    for grp in groups:
        for eq in grp.equations:
            cls = type(eq)
            if cls.__module__ == GD.__name__:
                if cls not in clones:
                    clone = type(cls.__name__, (cls,), {})
                    clone.__module__ = 'pysph.sph.gas_dynamics.basic'
                    clones[cls] = clone
                eq.__class__ = clones[cls]
    return groups


@pytest.mark.gpu
def test_reference_named_classes_select_the_gas_dynamics_kernels():
    """SummationDensity of a module called pysph.sph.gas_dynamics.basic is the gas-dynamics one, not one of its two
    namesakes: kind 34 is selected, its convergence flag drives the iteration, and the golden is met"""
    from pysph_amd.equations import resolve_equation
    g = load_golden('gasd_2d.npz')
    groups = reference_named(TG.equations_of(g))
    assert [type(eq).__module__ for eq in groups[0].equations] == ['pysph.sph.gas_dynamics.basic']
    assert resolve_equation(groups[0].equations[0])[0] == 34
    run_case('gasd_2d (reference-named classes)', g, equations=groups)


@pytest.mark.gpu
def test_max_iterations_stops_an_iteration_that_has_not_converged():
    """max_density_iterations below what the case needs: the group stops there, some particle is left unconverged
    and the convergence word said so every time"""
    g = load_golden('gasd_1d.npz')
    kw = dict(scheme_kw(g), max_density_iterations=int(g['meta/iterations']) - 2)
    from pysph_amd.gas_dynamics import GasDScheme
    groups = GasDScheme(**kw).get_equations()
    arrays = arrays_of(g)
    a_eval, nnps, ctx = evaluator(g, arrays, groups)
    nnps.update()
    a_eval.compute(float(g['t']), float(g['dt']))
    arrays[0].gpu.pull('converged')
    assert iterations(a_eval) == kw['max_density_iterations']
    assert groups[0].equations[0].converged() == -1
    assert np.any(arrays[0].properties['converged'] == 0.0) and np.any(arrays[0].properties['converged'] == 1.0)
    ctx.close()


@pytest.mark.gpu
def test_gasd_on_a_slab_decomposed_array_is_refused():
    """h is an unknown of the evaluation and the halo messages carry nothing between the density iterations:
    NotImplementedError before anything is launched -- nothing is written"""
    g = load_golden('gasd_2d.npz')
    arrays = arrays_of(g)
    a_eval, nnps, ctx = evaluator(g, arrays)
    arrays[0].slab_decomposed = True         # what a slab HipParallelManager marks its array with (parallel.py)
    nnps.update()
    with pytest.raises(NotImplementedError, match='slab-decomposed'):
        a_eval.compute(float(g['t']), float(g['dt']))
    pull_all(g, arrays)
    for p in stored_props(g, arrays[0]):
        assert np.array_equal(arrays[0].properties[p], g['in/fluid/' + p]), p
    ctx.close()


@pytest.mark.gpu
def test_pair_timers_of_the_two_families():
    """sph_timer_get keys pair_gasd_density (one launch per iteration) and pair_gasd_mpm (one per evaluation)"""
    g = load_golden('gasd_2d.npz')
    arrays = arrays_of(g)
    a_eval, nnps, ctx = evaluator(g, arrays)
    ctx.lib.sph_timer_enable(ctx._h, 1)
    nnps.update()
    a_eval.compute(float(g['t']), float(g['dt']))
    counts = {}
    for key in ('pair_gasd_density', 'pair_gasd_mpm'):
        ms, n = C.c_double(), C.c_long()
        assert ctx.lib.sph_timer_get(ctx._h, key.encode(), C.byref(ms), C.byref(n)) == 0
        counts[key] = n.value
        assert ms.value > 0.0
    assert counts == {'pair_gasd_density': int(g['meta/iterations']), 'pair_gasd_mpm': 1}
    ctx.close()


def _counter(ctx, key):
    ms, n = C.c_double(), C.c_long()
    assert ctx.lib.sph_timer_get(ctx._h, key.encode(), C.byref(ms), C.byref(n)) == 0
    return n.value


@pytest.mark.gpu
def test_skipping_converged_wavefronts_changes_nothing():
    """option gasd_skip: wavefronts whose 64 destinations have all converged leave before their neighbour work and only
    restore the raw arho and div.  gasd_1d (two wavefronts, six iterations): every column identical to the sweep that
    skips nothing, bit for bit, the same iterations (whether one of its two wavefronts converges early is the case's
    business: the next test makes sure some do)"""
    g = load_golden('gasd_1d.npz')
    cols = {}
    for skip in (0, 1):
        arrays = arrays_of(g)
        a_eval, nnps, ctx = evaluator(g, arrays)
        ctx.set_option('gasd_skip', skip)
        nnps.update()
        a_eval.compute(float(g['t']), float(g['dt']))
        pull_all(g, arrays)
        assert iterations(a_eval) == int(g['meta/iterations'])
        skipped = _counter(ctx, 'n_gasd_skipped')
        print('gasd_skip %d: %d wavefronts skipped' % (skip, skipped))
        assert skip or skipped == 0
        check_all('gasd_1d', g, arrays, 'out', TOL, 'gasd_skip %d' % skip)
        cols[skip] = dict((p, arrays[0].properties[p].copy()) for p in stored_props(g, arrays[0]))
        ctx.close()
    for p in cols[0]:
        assert np.array_equal(cols[0][p], cols[1][p]), p


@pytest.mark.gpu
def test_wavefronts_are_skipped_where_a_region_converges_first():
    """the converged state of gasd_3d with `converged` cleared and the h of the six particles nearest one corner off by
    5 %: everybody else converges in the first iteration (WI / DWI / GHI read the destination's own h only), the six
    need more -- wavefronts without one of them leave early from the second iteration on, and every column equals the
    sweep that skips nothing bit for bit"""
    g = load_golden('gasd_3d.npz')
    cols, its = {}, {}
    for skip in (0, 1):
        arrays = arrays_of(g, 'out')
        pa = arrays[0]
        near = np.argsort(pa.x + pa.y + pa.z)[:6]
        pa.properties['h'][near] *= 1.05
        pa.properties['h0'][:] = pa.properties['h']
        pa.properties['converged'][:] = 0.0
        pa.properties['omega'][:] = 1.0
        a_eval, nnps, ctx = evaluator(g, arrays)
        ctx.set_option('gasd_skip', skip)
        nnps.update()
        a_eval.compute(float(g['t']), float(g['dt']))
        pull_all(g, arrays)
        its[skip] = iterations(a_eval)
        skipped = _counter(ctx, 'n_gasd_skipped')
        print('gasd_skip %d: %d iterations, %d wavefronts skipped' % (skip, its[skip], skipped))
        assert (skipped > 0) == bool(skip)
        assert np.all(pa.properties['converged'] == 1.0)
        cols[skip] = dict((p, pa.properties[p].copy()) for p in stored_props(g, pa))
        ctx.close()
    assert its[0] == its[1] >= 2
    for p in cols[0]:
        assert np.array_equal(cols[0][p], cols[1][p]), p


PERIODIC_OUT = ('h', 'rho', 'arho', 'grhox', 'grhoy', 'dwdh', 'div', 'omega', 'ah', 'converged', 'p', 'cs', 'au', 'av', 'ae',
                'del2e', 'dt_cfl', 'aalpha1', 'aalpha2', 'u', 'v', 'e', 'alpha1', 'alpha2')


def _periodic_tiles(n1=12):
    """the unit square with n1 x n1 particles, and its explicit 3 x 3 tiling with the central tile first"""
    rng = np.random.default_rng(83)
    dx = 1.0 / n1
    c = (np.arange(n1) + 0.5) * dx
    x, y = [a.ravel() for a in np.meshgrid(c, c, indexing='ij')]
    n = x.size
    base = dict(x=x + 0.2 * dx * rng.uniform(-1, 1, n), y=y + 0.2 * dx * rng.uniform(-1, 1, n), z=np.zeros(n),
                u=0.3 * rng.uniform(-1, 1, n), v=0.3 * rng.uniform(-1, 1, n), w=np.zeros(n),
                h=1.2 * dx * (1 + 0.1 * rng.uniform(-1, 1, n)), m=dx * dx * (1 + 0.1 * rng.uniform(-1, 1, n)),
                e=rng.uniform(1.0, 3.0, n), alpha1=rng.uniform(0.2, 1.5, n), alpha2=rng.uniform(0.05, 0.5, n))
    shifts = [(0, 0)] + [(i, j) for i in (-1, 0, 1) for j in (-1, 0, 1) if (i, j) != (0, 0)]
    tiled = dict((k, np.tile(v, 9)) for k, v in base.items())
    tiled['x'] = np.concatenate([base['x'] + i for i, j in shifts])
    tiled['y'] = np.concatenate([base['y'] + j for i, j in shifts])
    kw = dict(fluids=['fluid'], solids=[], dim=2, gamma=1.4, kernel_factor=1.2, update_alpha1=True, update_alpha2=True,
              alpha1=0.3, alpha2=0.2, max_density_iterations=40)
    return base, tiled, kw, n


def _run_box(props, kw, periodic, steps, caps=None):
    """one evaluation (steps = 0) or PEC steps; caps: the iterations every evaluation may take at most.  Returns the
    array and the iterations every evaluation ran."""
    from pysph_amd import device as dev
    from pysph_amd import kernels as K
    from pysph_amd.acceleration_eval import AccelerationEval, SPHCompiler
    from pysph_amd.domain import HipDomainManager
    from pysph_amd.gas_dynamics import GasDScheme
    from pysph_amd.integrator import setup_integrator
    from pysph_amd.nnps import HipNNPS
    from pysph_amd.particle_array import get_particle_array_gasd
    pa = get_particle_array_gasd(name='fluid', **dict((k, v.copy()) for k, v in props.items()))
    pa.omega[:] = 1.0
    s = GasDScheme(has_ghosts=periodic, **kw)
    s.setup_properties([pa])
    kernel = K.CubicSpline(dim=2)
    assert 1.0 > 2 * kernel.radius_scale * 1.5 * props['h'].max()     # the box is wider than twice the kernel radius
    ctx = dev.HipContext(0)
    dev.attach(pa, ctx).push(*[p for p in pa.properties if pa.properties[p].dtype == np.float64])
    groups = s.get_equations()
    a_eval = AccelerationEval([pa], groups, kernel)
    SPHCompiler(a_eval, ctx=ctx, sync='manual').compile()
    dkw = {}
    if periodic:
        dkw = dict(domain=HipDomainManager(ctx=ctx, xmin=0, xmax=1, ymin=0, ymax=1, periodic_in_x=True,
                                           periodic_in_y=True))
    nnps = HipNNPS(2, [pa], radius_scale=kernel.radius_scale, ctx=ctx, sync=False, **dkw)
    a_eval.set_nnps(nnps)
    its = []
    if steps == 0:
        if caps:
            groups[0].max_iterations = caps[0]
        nnps.update_domain()
        nnps.update()
        a_eval.compute(0.0, 1e-3)
        its.append(iterations(a_eval))
    else:
        integ = s.configure_solver(kernel=kernel)
        setup_integrator(integ, a_eval, nnps)
        t, dt = 0.0, 1e-3
        for k in range(steps):
            if caps:
                groups[0].max_iterations = caps[k]
            integ.step(t, dt)
            its.append(iterations(a_eval))
            t += dt
    if periodic:
        assert pa.gpu.get_number_of_particles() > pa.gpu.get_number_of_particles(True)
    pa.gpu.pull(*(PERIODIC_OUT + ('x', 'y')))
    ctx.close()
    return pa, its


@pytest.mark.gpu
@pytest.mark.parametrize('steps', [0, 2])
def test_gasd_periodic_box_equals_its_explicit_tiling(steps):
    """GasDScheme(has_ghosts=True) on a periodic 12 x 12 box under HipDomainManager against the same scheme on the
    explicit 3 x 3 tiling without periodicity, for one evaluation and for two PEC steps: the central tile's rows within
    1e-10 of the field maximum.  The images get h, rho, omega, alpha*, e from every domain update inside the density
    iteration and p, cs from MPMUpdateGhostProps through orig_idx.  The tiling's outer rim is a free surface whose
    particles need more iterations than the box; a particle that has converged is summed again in every further
    iteration and loses the factor omega of its arho (the reference's behaviour), so the tiling may iterate at most
    as often as the box did in the same evaluation -- its central tile and the ring of particles that tile reads have
    all their neighbours and converge exactly as the box does."""
    base, tiled, kw, n = _periodic_tiles()
    box, its = _run_box(base, kw, True, steps)
    ref, its_ref = _run_box(tiled, kw, False, steps, caps=its)
    assert its_ref == its and all(2 <= k < kw['max_density_iterations'] for k in its), (its, its_ref)
    worst = 0.0
    for p in PERIODIC_OUT + ('x', 'y'):
        want, got = ref.properties[p][:n], box.properties[p][:n]
        e = rel_err(got, want)
        worst = max(worst, e)
        print('periodic, %d steps, %s: %.3e' % (steps, p, e))
        assert e < TOL, (p, e)
        assert np.abs(want).max() > 0.0, p
    print('periodic, %d steps: worst %.3e, iterations %s' % (steps, worst, its))
    assert np.all(box.properties['converged'][:n] == 1.0)


@pytest.mark.gpu
def test_shock_tube_example_keeps_its_invariants():
    """the Sod tube of pysph_amd/examples/shock_tube.py with 200 particles to t = 0.02: masses untouched, every
    particle converged, all columns finite, no step at max_density_iterations, h > 0 (the plateau values it prints
    are not asserted: SPH's error there is a property of the method)"""
    from pysph_amd.examples import shock_tube
    res = shock_tube.run(n=200, tf=0.02, quiet=True)
    pa = res['array']
    assert np.array_equal(pa.m, res['m_initial'])
    assert np.all(pa.converged == 1.0)
    for p in ('x', 'u', 'rho', 'p', 'e', 'h', 'cs', 'au', 'ae', 'omega', 'alpha1', 'alpha2'):
        assert np.all(np.isfinite(pa.properties[p])), p
    assert res['steps'] >= 2 and max(res['iterations']) < res['max_density_iterations']
    assert np.all(pa.h > 0.0) and np.all(pa.rho > 0.0) and np.all(pa.e > 0.0)
