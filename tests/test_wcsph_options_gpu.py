"""WCSPHScheme options delta_sph / nu / update_h on the GPU against the reference's own classes
(tests/golden/opt_*.npz, made by tests/golden/make_wcsph_options_golden.py).

``GradientCorrection`` keeps or drops the corrected gradient of a pair by a threshold.  The generator asserted that
no pair of the fp64 cases lies within 1e-6 of it (two correct fp64 solves differ by ~1e-13) and none of the gap case
within 5e-4 (fp32 moments and solves are good to ~1e-5), so every element is compared: a flipped branch would show as
an error of the size of a whole pair term.
"""
import json

import numpy as np
import pytest

from conftest import load_golden
from helpers import rel_err
import test_wcsph_options as TO

TOL = 1e-10            # BASELINE.json north_star, as tests/test_hip_parity.py
TOL_F32 = 5e-5         # test_fp32_arithmetic_vs_golden
STRIDED = {'m_mat': 9, 'gradrho': 3}


def arrays_of(g, which='in'):
    """pysph_amd ParticleArrays of a stored state, the strided properties with their strides"""
    from pysph_amd.particle_array import ParticleArray
    names = []
    for key in g.files:
        parts = key.split('/')
        if parts[0] == which and parts[1] not in names:
            names.append(parts[1])
    out = []
    for name in names:
        props = dict((key.split('/')[2], g[key].copy()) for key in g.files if key.startswith('%s/%s/' % (which, name)))
        strided = dict((k, props.pop(k)) for k in list(props) if k in STRIDED)
        pa = ParticleArray(name=name, **props)
        pa.set_num_real_particles(int(g['nreal/%s' % name]))
        for k, v in strided.items():
            pa.add_property(k, stride=STRIDED[k], data=v)
        out.append(pa)
    return out


def kernel_of(g):
    from pysph_amd import kernels as K
    return getattr(K, str(g['kernel']))(dim=int(json.loads(str(g['scheme']))['dim']))


def evaluator(g, arrays, variant=6, f32=False):
    from pysph_amd import device as dev
    from pysph_amd.acceleration_eval import AccelerationEval, SPHCompiler
    from pysph_amd.nnps import HipNNPS
    kernel = kernel_of(g)
    ctx = dev.HipContext(0)
    ctx.set_option('pair_variant', variant)
    if f32:
        ctx.set_option('arith_f32', 1)
    a_eval = AccelerationEval(arrays, TO.equations_of(g), kernel)
    SPHCompiler(a_eval, ctx=ctx, sync='manual').compile()
    push_all(arrays)
    nnps = HipNNPS(kernel.dim, arrays, radius_scale=kernel.radius_scale, ctx=ctx, sync=False)
    a_eval.set_nnps(nnps)
    return a_eval, nnps, ctx


def push_all(arrays):
    for pa in arrays:
        pa.gpu.push()
        cols = ['%s__%d' % (k, j) for k, s in STRIDED.items() if k in pa.properties for j in range(s)]
        if cols:
            pa.gpu.push(*cols)


def check_nnps(nnps, g, prefix):
    assert nnps.cell_size == float(g[prefix + '/cell_size'])
    assert np.array_equal(nnps.xmin, g[prefix + '/xmin'])
    assert np.array_equal(nnps.xmax, g[prefix + '/xmax'])
    assert np.array_equal(nnps.ncells_per_dim, g[prefix + '/ncells_per_dim'])
    assert nnps.n_cells == int(g[prefix + '/n_cells'])


def check_all(case, g, arrays, which, tol, what):
    """EVERY stored property of every array, every element; the strided ones component by component"""
    worst, n = 0.0, 0
    for pa in arrays:
        keys = [k for k in g.files if k.startswith('%s/%s/' % (which, pa.name))]
        assert keys
        for key in keys:
            prop = key.split('/')[2]
            want, got = g[key], pa.properties[prop]
            assert got.shape == want.shape, (case, key)
            s = STRIDED.get(prop, 1)
            for j in range(s):
                e = rel_err(got[j::s], want[j::s])
                print('%s %s %s/%s[%d]: %.3e' % (case, what, pa.name, prop, j, e))
                worst = max(worst, e)
                assert e < tol, (case, what, pa.name, prop, j, e)
                n += want[j::s].size
    print('%s %s: max rel err %.3e over %d elements' % (case, what, worst, n))
    return worst


def pull_everything(a_eval, arrays):
    a_eval.c_acceleration_eval.pull_outputs()
    for pa in arrays:            # inputs too: nothing but the outputs may have changed
        pa.gpu.pull('x', 'y', 'z', 'u', 'v', 'w', 'h', 'm', 'rho')


@pytest.mark.gpu
@pytest.mark.parametrize('variant', [6, 0])
@pytest.mark.parametrize('case', ['opt_dsph3d', 'opt_dsph2d_tank', 'opt_lamvisc3d', 'opt_singular'])
def test_options_parity_with_reference_golden(case, variant):
    """fp64, both schedules: NNPS scalars equal, every property -- all components of m_mat and gradrho, and h --
    within 1e-10 of the field maximum after the first evaluation; opt_dsph3d (update_h) also after nnps.update() and a
    second evaluation: h has changed, so the cell size moves"""
    g = load_golden(case + '.npz')
    arrays = arrays_of(g)
    a_eval, nnps, ctx = evaluator(g, arrays, variant)
    nnps.update()
    check_nnps(nnps, g, 'nnps')
    t, dt = float(g['t']), float(g['dt'])
    a_eval.compute(t, dt)
    pull_everything(a_eval, arrays)
    check_all(case, g, arrays, 'out', TOL, 'variant %d' % variant)
    if 'nnps2/cell_size' in g.files:
        assert float(g['nnps2/cell_size']) != float(g['nnps/cell_size'])
        nnps.update()
        check_nnps(nnps, g, 'nnps2')
        a_eval.compute(t + dt, dt)
        pull_everything(a_eval, arrays)
        check_all(case, g, arrays, 'out2', TOL, 'variant %d, second evaluation' % variant)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['opt_dsph3d_gap', 'opt_lamvisc3d'])
def test_options_fp32_arithmetic(case):
    """option arith_f32 against the fp64 vectors at the project's fp32 bound, every element; really in float"""
    g = load_golden(case + '.npz')
    arrays = arrays_of(g)
    a_eval, nnps, ctx = evaluator(g, arrays, 6, f32=True)
    nnps.update()
    a_eval.compute(float(g['t']), float(g['dt']))
    pull_everything(a_eval, arrays)
    worst = check_all(case, g, arrays, 'out', TOL_F32, 'arith_f32')
    assert worst > 1e-9
    ctx.close()


@pytest.mark.gpu
def test_singular_moment_matrices_stay_uncorrected():
    """the isolated particle, the pair and the collinear triple have moment matrices without a usable pivot: their
    gradrho is the plain sum (rho_b - rho_a) DWIJ V_b"""
    from pysph_amd import kernels as K
    g = load_golden('opt_singular.npz')
    arrays = arrays_of(g)
    a_eval, nnps, ctx = evaluator(g, arrays)
    nnps.update()
    a_eval.compute(float(g['t']), float(g['dt']))
    pull_everything(a_eval, arrays)
    check_all('opt_singular', g, arrays, 'out', TOL, 'fp64')
    ctx.close()
    pa = arrays[0]
    kernel = K.QuinticSpline(dim=3)
    n, k = pa.get_number_of_particles(), int(g['meta/n_degenerate'])
    want = np.zeros((k, 3))
    for a, i in enumerate(range(n - k, n)):
        for j in range(n):
            xij = [pa.x[i] - pa.x[j], pa.y[i] - pa.y[j], pa.z[i] - pa.z[j]]
            r2 = xij[0] * xij[0] + xij[1] * xij[1] + xij[2] * xij[2]
            if r2 < (3.0 * pa.h[i]) ** 2 or r2 < (3.0 * pa.h[j]) ** 2:
                dw = [0.0, 0.0, 0.0]
                kernel.gradient(xij, np.sqrt(r2), 0.5 * (pa.h[i] + pa.h[j]), dw)
                want[a] += (pa.rho[j] - pa.rho[i]) * np.array(dw) * pa.m[j] / pa.rho[j]
    got = pa.gradrho.reshape(-1, 3)[n - k:]
    assert np.all(want[0] == 0.0) and np.abs(want[1:]).min() > 0.0       # alone: nothing but itself
    assert np.max(np.abs(got - want)) < TOL * np.abs(want).max(), (got, want)


@pytest.mark.gpu
def test_update_h_follows_the_density_through_epec_steps():
    """10 EPEC steps of the 3-D case, device-resident.  The corrector stage changes rho behind the step's last
    evaluation, so one more evaluation follows the steps; then h == hdx (m / rho)^(1/dim) from the pulled m and rho
    within 4 ulp (the bound tests/test_codegen_semantics.py holds pow to), and the next neighbour update has looked at
    the new values: cell_size == radius_scale max(h)."""
    from pysph_amd.integrator import EPECIntegrator, WCSPHStep, setup_integrator
    g = load_golden('opt_dsph3d.npz')
    arrays = arrays_of(g)
    for pa in arrays:
        for p in ('x0', 'y0', 'z0', 'u0', 'v0', 'w0', 'rho0'):
            pa.add_property(p)
    a_eval, nnps, ctx = evaluator(g, arrays)
    integ = EPECIntegrator(fluid=WCSPHStep())
    setup_integrator(integ, a_eval, nnps)
    t, dt = 0.0, 1e-4
    for _ in range(10):
        integ.step(t, dt)
        t += dt
    nnps.update()
    a_eval.compute(t, dt)
    pa = arrays[0]
    pa.gpu.pull('h', 'm', 'rho')
    hdx = json.loads(str(g['scheme']))['hdx']
    want = hdx * np.power(pa.m / pa.rho, 1.0 / 3.0)
    assert np.max(np.abs(pa.h - want) / np.spacing(want)) <= 4.0
    assert np.ptp(pa.h) > 0.0 and not np.array_equal(pa.h, g['in/fluid/h'])
    nnps.update()
    assert nnps.cell_size == nnps.radius_scale * pa.h.max()
    ctx.close()


def _small_block(n1=5, solid_rows=0):
    from pysph_amd.particle_array import get_particle_array_wcsph
    rng = np.random.default_rng(3)
    dx = 1.0 / n1
    c = (np.arange(n1) + 0.5) * dx
    x, y, z = [a.ravel() + 0.1 * dx * rng.uniform(-1, 1, n1 ** 3) for a in np.meshgrid(c, c, c, indexing='ij')]
    n = x.size
    fluid = get_particle_array_wcsph(name='fluid', x=x, y=y, z=z, h=1.2 * dx * np.ones(n), m=1000.0 * dx ** 3 * np.ones(n),
                                     rho=1000.0 * (1 + 0.02 * rng.uniform(-1, 1, n)), u=rng.uniform(-1, 1, n))
    return fluid, dx


def _delta_scheme(dx, solids=()):
    from pysph_amd.scheme import WCSPHScheme
    return WCSPHScheme(['fluid'], list(solids), dim=3, rho0=1000.0, c0=10.0, h0=1.2 * dx, hdx=1.2, alpha=0.2,
                       delta_sph=True, nu=0.01)


@pytest.mark.gpu
@pytest.mark.parametrize('ghosts', ['slab', 'periodic'])
def test_delta_sph_with_ghost_layers_is_refused(ghosts):
    """ghost rows would need gradrho carried to them: NotImplementedError naming the reason before any delta-SPH pass
    is launched"""
    from pysph_amd import device as dev
    from pysph_amd import kernels as K
    from pysph_amd.acceleration_eval import AccelerationEval, SPHCompiler
    from pysph_amd.domain import HipDomainManager
    from pysph_amd.nnps import HipNNPS
    from pysph_amd.parallel import DeviceHaloOps, WCSPH_HALO_PROPS
    fluid, dx = _small_block()
    s = _delta_scheme(dx)
    s.setup_properties([fluid])
    kernel = K.WendlandQuintic(dim=3)
    ctx = dev.HipContext(0)
    dev.attach(fluid, ctx).push()
    a_eval = AccelerationEval([fluid], s.get_equations(), kernel)
    SPHCompiler(a_eval, ctx=ctx, sync='manual').compile()
    if ghosts == 'slab':
        DeviceHaloOps(fluid, ctx, WCSPH_HALO_PROPS, 0)         # what a slab HipParallelManager puts on the array
        nnps = HipNNPS(3, [fluid], radius_scale=2.0, ctx=ctx, sync=False)
    else:
        dom = HipDomainManager(ctx=ctx, xmin=0, xmax=1, ymin=0, ymax=1, zmin=0, zmax=1, periodic_in_x=True)
        nnps = HipNNPS(3, [fluid], radius_scale=2.0, ctx=ctx, domain=dom, sync=False)
    a_eval.set_nnps(nnps)
    with pytest.raises(NotImplementedError, match='gradrho'):
        a_eval.compute(0.0, 1e-4)
    ctx.close()


@pytest.mark.gpu
def test_options_with_an_empty_solid_array():
    """a solid array without particles is a source and a destination of nothing: the option set runs and gives what
    the same set without the array gives"""
    from pysph_amd import device as dev
    from pysph_amd import kernels as K
    from pysph_amd.acceleration_eval import AccelerationEval, SPHCompiler
    from pysph_amd.nnps import HipNNPS
    from pysph_amd.particle_array import get_particle_array_wcsph
    kernel = K.WendlandQuintic(dim=3)
    results = []
    for solids in (('wall',), ()):
        fluid, dx = _small_block()
        arrays = [fluid]
        if solids:
            arrays.append(get_particle_array_wcsph(name='wall', x=np.zeros(0)))
        s = _delta_scheme(dx, solids)
        s.setup_properties(arrays)
        ctx = dev.HipContext(0)
        a_eval = AccelerationEval(arrays, s.get_equations(), kernel)
        SPHCompiler(a_eval, ctx=ctx).compile()
        nnps = HipNNPS(3, arrays, radius_scale=2.0, ctx=ctx)
        a_eval.set_nnps(nnps)
        nnps.update()
        a_eval.compute(0.0, 1e-4)
        results.append(dict((p, fluid.properties[p].copy()) for p in ('arho', 'au', 'av', 'aw', 'gradrho', 'm_mat')))
        ctx.close()
    for p, v in results[0].items():
        assert np.abs(v).max() > 0.0 and np.array_equal(v, results[1][p]), p
