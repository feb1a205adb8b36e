"""Godunov SPH on the GPU against the reference's own classes (tests/golden/gsph_*.npz, made by
tests/golden/make_gsph_golden.py): the whole group list in one, two and three dimensions, every Riemann solver, every
combination of limiter, interpolation and interface position, hybrid, a coincident pair of two arrays, all ten smoothing
kernels, the stage kernel, three device-resident Euler steps, a periodic box against its tiling, the failure word and
fp32 arithmetic.

Measured on an MI355X (the figures the bounds below come from are in DESIGN.md, section 7h)."""
import ctypes as C
import json

import numpy as np
import pytest

from conftest import load_golden
from helpers import rel_err
import test_gsph as TS
from test_gasd_gpu import _View, check_nnps, kernel_of

TOL = 1e-10            # of the field maximum, as tests/test_gasd_gpu.py
TOL_F32 = 5e-5         # the project's fp32 bound (tests/test_gasd_gpu.py)
FORCE_OUT = ('au', 'av', 'aw', 'ae')
SOLVER_NAMES = ('non_diffusive', 'van_leer', 'exact', 'hllc', 'ducowicz', 'hlle', 'roe', 'llxf', 'hllc_ball', 'hll_ball',
                'hllsy')
# max over au av aw ae of |fp32 - golden| / max |golden|, force group in fp32 arithmetic on the converged 2-D state, per
# solver; the test asserts four times these, and TOL_F32 in any case.  `exact` iterates: its stop
# test compares a relative change with tol = 1e-6, which fp32 resolves (2^-24 = 6e-8), so a solve may stop one iteration
# earlier or later than in fp64; either way the change at the stop is below tol and the pressure moves by less than
# tol * p: the case gets the same bound as the others.
F32_MEASURED = {0: 1.204e-06, 2: 8.487e-07, 3: 7.812e-07, 4: 1.053e-06, 5: 7.478e-07, 6: 9.908e-07, 7: 8.848e-07,
                8: 8.107e-07, 9: 7.476e-07, 10: 8.020e-07}


def names_of(g, prefix=''):
    return sorted(set(k[len(prefix):].split('/')[1] for k in g.files if k.startswith(prefix + 'nreal/')))


def arrays_of(g, which='in', prefix=''):
    from pysph_amd.particle_array import ParticleArray
    out = []
    for name in names_of(g, prefix):
        head = '%s%s/%s/' % (prefix, which, name)
        props = dict((key[len(head):], g[key].copy()) for key in g.files if key.startswith(head))
        pa = ParticleArray(name=name, **props)
        pa.set_num_real_particles(int(g['%snreal/%s' % (prefix, name)]))
        out.append(pa)
    return out


def _floats(pa):
    return sorted(p for p in pa.properties if pa.properties[p].dtype == np.float64)


def evaluator(arrays, groups, kernel, variant=6, f32=False):
    from pysph_amd import device as dev
    from pysph_amd.acceleration_eval import AccelerationEval, SPHCompiler
    from pysph_amd.nnps import HipNNPS
    ctx = dev.HipContext(0)
    ctx.set_option('pair_variant', variant)
    if f32:
        ctx.set_option('arith_f32', 1)
    a_eval = AccelerationEval(arrays, groups, kernel)
    SPHCompiler(a_eval, ctx=ctx, sync='manual').compile()
    for pa in arrays:
        pa.gpu.push(*_floats(pa))
    nnps = HipNNPS(kernel.dim, arrays, radius_scale=kernel.radius_scale, ctx=ctx, sync=False)
    a_eval.set_nnps(nnps)
    return a_eval, nnps, ctx


def pull_all(arrays):
    """outputs AND inputs: nothing but the outputs may have changed"""
    for pa in arrays:
        pa.gpu.pull(*_floats(pa))


def check_all(case, g, arrays, which, tol, what, prefix=''):
    """EVERY stored property of every array, every element"""
    worst, n = 0.0, 0
    for pa in arrays:
        head = '%s%s/%s/' % (prefix, which, pa.name)
        keys = [k for k in g.files if k.startswith(head)]
        assert keys
        for key in keys:
            prop = key[len(head):]
            want, got = g[key], pa.properties[prop]
            assert got.shape == want.shape, (case, key)
            e = rel_err(got, want)
            print('%s %s %s/%s: %.3e' % (case, what, pa.name, prop, e))
            worst = max(worst, e)
            assert e < tol, (case, what, pa.name, prop, e)
            n += want.size
    print('%s %s: max rel err %.3e over %d elements' % (case, what, worst, n))
    return worst


def failures(groups):
    return groups[-1].equations[0].solver_failures()


def run_case(case, g, variant=6, groups=None, prefix=''):
    from pysph_amd import device as dev
    arrays = arrays_of(g, 'in', prefix)
    groups = TS.equations_of(g, prefix) if groups is None else groups
    a_eval, nnps, ctx = evaluator(arrays, groups, kernel_of(_View(g, prefix)), variant)
    nnps.update()
    t, dt = float(g[prefix + 't']), float(g[prefix + 'dt'])
    a_eval.compute(t, dt)
    pull_all(arrays)
    what = 'variant %d' % variant
    worst = check_all(case, g, arrays, 'out', TOL, what, prefix)
    check_nnps(nnps, _View(g, prefix), 'nnps')
    assert failures(groups) == 0
    if prefix + 'nnps2/cell_size' in g.files:
        for pa in arrays:                # as the generator: one GSPHStep, then a second evaluation
            dev._check(ctx.lib.sph_integrate_stage(ctx._h, pa.gpu.array_id, 9, 1, C.c_double(dt)))
        nnps.update()
        a_eval.compute(t + dt, dt)
        pull_all(arrays)
        worst = max(worst, check_all(case, g, arrays, 'out2', TOL, what + ', second evaluation', prefix))
        check_nnps(nnps, _View(g, prefix), 'nnps2')
        assert failures(groups) == 0
    ctx.close()
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize('variant', [6, 0])
@pytest.mark.parametrize('case', TS.EVAL_CASES)
def test_gsph_parity_with_reference_golden(case, variant):
    """fp64, both schedules: every stored column of every particle within 1e-10 of the field maximum after the whole
    list -- the two density sweeps around the h update, the EOS, the twelve gradients and the force sweep -- and, for
    gsph_3d (IwIn, cubic, interface position), after one GSPHStep on the device and a second evaluation; no solver
    failure is counted"""
    run_case(case, load_golden(case + '.npz'), variant)


@pytest.mark.gpu
@pytest.mark.parametrize('kname', json.loads(str(load_golden('gsph_kernels.npz')['kernels'])))
def test_gsph_every_smoothing_kernel(kname):
    """all ten kernel ids, fp64: DWI, DWJ and DWIJ of each in the gradient and the force sweep (g1, g2 non-zero)"""
    g = load_golden('gsph_kernels.npz')
    assert str(g[kname + '/kernel']) == kname
    run_case('gsph_kernels ' + kname, g, prefix=kname + '/')


def _force_group(params):
    from pysph_amd.equations import Group
    from pysph_amd.gas_dynamics import GSPHAcceleration
    return [Group(equations=[GSPHAcceleration(dest='fluid', sources=['fluid'], **params)])]


def run_force_case(g, key, name, variant=6, f32=False, tol=TOL):
    """GSPHAcceleration alone on the stored state: its four columns against the vectors, every other column unchanged"""
    from pysph_amd import kernels as K
    arrays = arrays_of(g)
    params = json.loads(str(g['%s/%s/params' % (key, name)]))
    groups = _force_group(params)
    a_eval, nnps, ctx = evaluator(arrays, groups, K.CubicSpline(dim=2), variant, f32)
    nnps.update()
    a_eval.compute(float(g['%s/%s/t' % (key, name)]), float(g['dt']))
    pull_all(arrays)
    pa = arrays[0]
    worst = 0.0
    for col in FORCE_OUT:
        want = g['%s/%s/fluid/%s' % (key, name, col)]
        e = rel_err(pa.properties[col], want)
        worst = max(worst, e)
        print('%s %s %s variant %d%s: %.3e' % (key, name, col, variant, ' fp32' if f32 else '', e))
        assert e < tol, (key, name, col, e)
    for key in g.files:
        col = key[len('in/fluid/'):]
        if key.startswith('in/fluid/') and col not in FORCE_OUT:
            assert np.array_equal(pa.properties[col], g[key]), (name, col)
    assert failures(groups) == 0
    ctx.close()
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize('variant', [6, 0])
@pytest.mark.parametrize('rsolver', range(11))
def test_gsph_every_riemann_solver(rsolver, variant):
    """the force group alone on the converged 2-D state (I02, linear, conduction on), once per solver"""
    g = load_golden('gsph_solvers.npz')
    assert json.loads(str(g['solver/%d/params' % rsolver]))['rsolver'] == rsolver
    run_force_case(g, 'solver', str(rsolver), variant)


@pytest.mark.gpu
@pytest.mark.parametrize('mono', [0, 1, 2])
@pytest.mark.parametrize('rsolver', [2, 3])
def test_gsph_limiter_interpolation_and_interface_position(rsolver, mono):
    """on exact and on hllc: the three limiters x the three interpolations x interface_zero both ways"""
    g = load_golden('gsph_options.npz')
    names = json.loads(str(g['names']))
    mine = [n for n in names if n.startswith('r%d_m%d_' % (rsolver, mono))]
    assert len(mine) == 6
    for name in mine:
        run_force_case(g, 'opt', name)


@pytest.mark.gpu
def test_gsph_hybrid_blends_with_hllsy_at_the_host_computed_factor():
    """hybrid=True at t = 0.3 tf with tf = 0.8 handed to the equation: exp(-blend_alpha t / tf) is computed once per
    launch from the evaluation's t"""
    g = load_golden('gsph_options.npz')
    params = json.loads(str(g['opt/hybrid/params']))
    assert params['hybrid'] and float(g['opt/hybrid/t']) == pytest.approx(0.3 * params['tf'])
    run_force_case(g, 'opt', 'hybrid')


@pytest.mark.gpu
@pytest.mark.parametrize('variant', [6, 0])
def test_gsph_two_fluids_with_a_coincident_pair(variant):
    """two arrays, each destination and source, one particle of f2 on one of f1 (RIJ = 0 between different arrays:
    eij = 0, sij = 1 / EPS, the limiter's and the interpolation's RIJ branches), IwIn and cubic: the whole list"""
    g = load_golden('gsph_options.npz')
    run_case('gsph_options coincident', g, variant, prefix='coincident/')


def reference_named(groups):
    """the same equation objects as instances of classes NAMED like the reference's and living in modules NAMED like
    the reference's -- what a user who passes pysph's own objects hands over"""
    from pysph_amd import gas_dynamics as GD
    clones = {}
    for grp in groups:
        for eq in grp.equations:
            cls = type(eq)
            if cls.__module__ == GD.__name__:
                if cls not in clones:
                    clone = type(cls.__name__, (cls,), {})
                    clone.__module__ = ('pysph.sph.gas_dynamics.gsph' if cls.__name__.startswith('GSPH')
                                        else 'pysph.sph.gas_dynamics.basic')
                    clones[cls] = clone
                eq.__class__ = clones[cls]
    return groups


@pytest.mark.gpu
def test_reference_named_classes_select_the_gsph_kernels():
    from pysph_amd.equations import resolve_equation
    g = load_golden('gsph_2d.npz')
    groups = reference_named(TS.equations_of(g))
    assert [type(grp.equations[0]).__module__ for grp in groups[-2:]] == ['pysph.sph.gas_dynamics.gsph'] * 2
    assert [resolve_equation(grp.equations[0])[0] for grp in groups] == [37, 34, 38, 34, 35, 40, 42]
    run_case('gsph_2d (reference-named classes)', g, groups=groups)


def _vacuum_pair(rsolver):
    """two particles receding at ur - ul = 20 > 2 (cl + cr) / (gamma - 1) = 11.8: the force group alone, first order"""
    from pysph_amd import kernels as K
    from pysph_amd.particle_array import get_particle_array_gasd
    from pysph_amd.gas_dynamics import GSPHScheme
    pa = get_particle_array_gasd(name='fluid', x=np.array([0.0, 0.1]), u=np.array([-10.0, 10.0]), h=0.1 * np.ones(2),
                                 m=0.1 * np.ones(2), rho=np.ones(2), p=np.ones(2), e=2.5 * np.ones(2),
                                 cs=np.sqrt(1.4) * np.ones(2))
    GSPHScheme(['fluid'], [], dim=1, gamma=1.4, kernel_factor=1.2).setup_properties([pa])
    for col in FORCE_OUT:
        pa.properties[col][:] = 7.0
    groups = _force_group(dict(rsolver=rsolver, monotonicity=0, gamma=1.4))
    a_eval, nnps, ctx = evaluator([pa], groups, K.Gaussian(dim=1))
    nnps.update()
    a_eval.compute(0.0, 1e-4)
    n = failures(groups)
    pa.gpu.pull(*FORCE_OUT)
    ctx.close()
    return pa, n


@pytest.mark.gpu
def test_failure_word_counts_a_vacuum_pair_and_the_pair_contributes_nothing():
    """`exact` on the vacuum test returns 1 without a result: both ordered pairs are counted, and with
    pstar = ustar = 0 they add nothing (the self pairs solve and carry DWI = 0); hllc on the same pair solves"""
    pa, n = _vacuum_pair(2)
    assert n == 2
    for col in FORCE_OUT:
        assert np.array_equal(pa.properties[col], np.zeros(2)), col
    pa, n = _vacuum_pair(3)
    assert n == 0
    assert np.all(np.abs(pa.au) > 0.0) and np.all(np.isfinite(pa.au)) and np.all(np.isfinite(pa.ae))


@pytest.mark.gpu
def test_gsph_stepper_vs_reference_golden():
    """the stage kernel against the reference's GSPHStep.stage1; every product is rounded on its own (no contraction)"""
    from pysph_amd import device as dev
    from pysph_amd.particle_array import ParticleArray
    g = load_golden('gsph_steppers.npz')
    dt = float(g['dt'])
    props = dict((k[3:], g[k].copy()) for k in g.files if k.startswith('in/'))
    pa = ParticleArray(name='fluid', **props)
    ctx = dev.HipContext(0)
    dev.attach(pa, ctx).push(*sorted(props))
    for stage in (0, 1, 2):                  # initialize and stage2 do nothing
        dev._check(ctx.lib.sph_integrate_stage(ctx._h, pa.gpu.array_id, 9, stage, C.c_double(dt)))
        pa.gpu.pull(*sorted(props))
        for k in sorted(props):
            ref = g['gsph/stage1/' + k] if stage else g['in/' + k]
            assert np.allclose(pa.properties[k], ref, rtol=1e-15, atol=0.0), (stage, k)
    assert not np.array_equal(pa.properties['e'], g['in/e'])
    ctx.close()


@pytest.mark.gpu
def test_gsph_three_device_resident_euler_steps():
    """the gsph_3d particles through three Euler steps with the reference-named GSPHStep on the device -- no host pull
    between the steps -- every column within 1e-10 of the field maximum of the reference's three steps"""
    from pysph_amd.integrator import EulerIntegrator, setup_integrator
    g = load_golden('gsph_steps.npz')
    arrays = arrays_of(g)
    groups = TS.equations_of(g)
    a_eval, nnps, ctx = evaluator(arrays, groups, kernel_of(g))
    ref_step = type('GSPHStep', (object,), {})()       # the reference's own stepper object selects the stage kernel
    integ = EulerIntegrator(fluid=ref_step)
    setup_integrator(integ, a_eval, nnps)
    assert [kind for _, _, _, kind, _ in integ.c_integrator._stages] == [9]
    t, dt = float(g['t']), float(g['dt'])
    for _ in range(int(g['meta/steps'])):
        integ.step(t, dt)
        t += dt
    assert failures(groups) == 0
    pull_all(arrays)
    worst = check_all('gsph_steps', g, arrays, 'out', TOL, 'three Euler steps')
    print('gsph_steps: worst figure %.3e' % worst)
    assert not np.array_equal(arrays[0].x, g['in/fluid/x'])
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize('rsolver', sorted(F32_MEASURED))
def test_gsph_fp32_force_group(rsolver):
    """option arith_f32, the force group at the golden state, the non-iterative solvers and exact: within four times the
    measured distance from the fp64 vectors and within the project's fp32 bound; really in float"""
    g = load_golden('gsph_solvers.npz')
    worst = run_force_case(g, 'solver', str(rsolver), f32=True, tol=TOL_F32)
    print('fp32 force group, %s: %.3e' % (SOLVER_NAMES[rsolver], worst))
    assert worst > 1e-9
    assert worst < 4 * F32_MEASURED[rsolver], (rsolver, worst)


PERIODIC_OUT = ('h', 'rho', 'arho', 'grhox', 'grhoy', 'dwdh', 'div', 'p', 'cs', 'px', 'py', 'ux', 'uy', 'vx', 'vy', 'au', 'av',
                'ae', 'u', 'v', 'e')


def _periodic_tiles(n1=12):
    """the unit square with n1 x n1 particles, and its explicit 3 x 3 tiling with the central tile first"""
    rng = np.random.default_rng(89)
    dx = 1.0 / n1
    c = (np.arange(n1) + 0.5) * dx
    x, y = [a.ravel() for a in np.meshgrid(c, c, indexing='ij')]
    n = x.size
    base = dict(x=x + 0.2 * dx * rng.uniform(-1, 1, n), y=y + 0.2 * dx * rng.uniform(-1, 1, n), z=np.zeros(n),
                u=0.3 * rng.uniform(-1, 1, n), v=0.3 * rng.uniform(-1, 1, n), w=np.zeros(n),
                h=1.2 * dx * (1 + 0.05 * rng.uniform(-1, 1, n)), m=dx * dx * (1 + 0.1 * rng.uniform(-1, 1, n)),
                e=rng.uniform(1.0, 3.0, n))
    shifts = [(0, 0)] + [(i, j) for i in (-1, 0, 1) for j in (-1, 0, 1) if (i, j) != (0, 0)]
    tiled = dict((k, np.tile(v, 9)) for k, v in base.items())
    tiled['x'] = np.concatenate([base['x'] + i for i, j in shifts])
    tiled['y'] = np.concatenate([base['y'] + j for i, j in shifts])
    kw = dict(fluids=['fluid'], solids=[], dim=2, gamma=1.4, kernel_factor=1.2, g1=0.2, g2=0.4, monotonicity=2)
    return base, tiled, kw, n


def _run_box(props, kw, periodic, steps):
    from pysph_amd import device as dev
    from pysph_amd import kernels as K
    from pysph_amd.acceleration_eval import AccelerationEval, SPHCompiler
    from pysph_amd.domain import HipDomainManager
    from pysph_amd.gas_dynamics import GSPHScheme
    from pysph_amd.integrator import setup_integrator
    from pysph_amd.nnps import HipNNPS
    from pysph_amd.particle_array import get_particle_array_gasd
    pa = get_particle_array_gasd(name='fluid', **dict((k, v.copy()) for k, v in props.items()))
    s = GSPHScheme(has_ghosts=periodic, **kw)
    s.setup_properties([pa])
    kernel = K.CubicSpline(dim=2)
    assert 1.0 > 2 * kernel.radius_scale * 2.0 * props['h'].max()     # wider than twice the kernel radius at the scaled h
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
    if steps == 0:
        nnps.update_domain()
        nnps.update()
        a_eval.compute(0.0, 1e-3)
    else:
        integ = s.configure_solver(kernel=kernel)
        setup_integrator(integ, a_eval, nnps)
        t, dt = 0.0, 1e-3
        for k in range(steps):
            integ.step(t, dt)
            t += dt
    assert failures(groups) == 0
    if periodic:
        assert pa.gpu.get_number_of_particles() > pa.gpu.get_number_of_particles(True)
    pa.gpu.pull(*(PERIODIC_OUT + ('x', 'y')))
    ctx.close()
    return pa


@pytest.mark.gpu
@pytest.mark.parametrize('steps', [0, 2])
def test_gsph_periodic_box_equals_its_explicit_tiling(steps):
    """GSPHScheme(has_ghosts=True) on a periodic 12 x 12 box under HipDomainManager against the same scheme on the
    explicit 3 x 3 tiling without periodicity, for one evaluation and for two Euler steps: the central tile's rows within
    1e-10 of the field maximum.  The images get h, rho, e and the velocities from the domain updates of the two
    update_nnps groups, and what the force sweep reads besides -- the gradients, grho, div, dwdh, rho, p, cs -- from
    GSPHUpdateGhostProps through orig_idx, right before it; the evaluator runs that group in front of the gradient
    group too, whose sums read p and rho of the images (with the reference's order alone px was off by 2.2 of its
    maximum)."""
    base, tiled, kw, n = _periodic_tiles()
    box = _run_box(base, kw, True, steps)
    ref = _run_box(tiled, kw, False, steps)
    worst = 0.0
    for p in PERIODIC_OUT + ('x', 'y'):
        want, got = ref.properties[p][:n], box.properties[p][:n]
        if steps and p in ('x', 'y'):          # the box wraps a particle that leaves it
            got, want = np.mod(got, 1.0), np.mod(want, 1.0)
        e = rel_err(got, want)
        worst = max(worst, e)
        print('periodic, %d steps, %s: %.3e' % (steps, p, e))
        assert e < TOL, (p, e)
        assert np.abs(want).max() > 0.0, p
    print('periodic, %d steps: worst %.3e' % (steps, worst))


@pytest.mark.gpu
def test_pair_timers_of_the_two_families():
    """sph_timer_get keys pair_gsph_gradients and pair_gsph: one launch each per evaluation"""
    g = load_golden('gsph_2d.npz')
    arrays = arrays_of(g)
    a_eval, nnps, ctx = evaluator(arrays, TS.equations_of(g), kernel_of(g))
    ctx.lib.sph_timer_enable(ctx._h, 1)
    nnps.update()
    a_eval.compute(float(g['t']), float(g['dt']))
    for key in ('pair_gsph_gradients', 'pair_gsph'):
        ms, n = C.c_double(), C.c_long()
        assert ctx.lib.sph_timer_get(ctx._h, key.encode(), C.byref(ms), C.byref(n)) == 0
        assert n.value == 1 and ms.value > 0.0, key
    ctx.close()


@pytest.mark.gpu
def test_gsph_shock_tube_example_reports_the_plateau():
    """the Sod tube of pysph_amd/examples/gsph_shock_tube.py with 200 particles to t = 0.02: masses untouched, all columns
    finite, no solver failure; at this time the star region is a few particles wide, so the plateau figures are
    printed, not asserted (DESIGN.md section 7h has them at t = 0.15)"""
    from pysph_amd.examples import gsph_shock_tube
    res = gsph_shock_tube.run(n=200, tf=0.02, quiet=True)
    pa = res['array']
    assert np.array_equal(pa.m, res['m_initial'])
    for p in ('x', 'u', 'rho', 'p', 'e', 'h', 'cs', 'au', 'ae', 'px', 'ux'):
        assert np.all(np.isfinite(pa.properties[p])), p
    assert res['steps'] >= 2 and res['solver_failures'] == 0
    assert np.all(pa.h > 0.0) and np.all(pa.rho > 0.0) and np.all(pa.e > 0.0)
