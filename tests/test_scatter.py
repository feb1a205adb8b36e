"""Loop bodies that add to properties of their SOURCE array (``s_fx[s_idx] += ...``:
the force a fluid puts on the particles of an immersed body).  The translator
splits such a family into the forward launch and a transposed companion
(DESIGN.md section 7c); the checker is oracle/py_eval.py, which executes the
same Python bodies serially, source stores included."""
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import rel_err

TOL = 1e-10         # BASELINE.json: the project's parity tolerance
FORCES = ('fx', 'fy', 'fz')
SOLID_OUT = FORCES + ('tq',)
FLUID_OUT = ('au', 'av', 'aw', 'e')
N1 = 9
DX = 1.0 / N1
EXTRA = ['V', 'q', 'e', 'fx', 'fy', 'fz', 'au', 'av', 'aw', 'arho', 'p', 'cs', 'gsum']


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------
def _array(name, x, y, z, varh, rng):
    from pysph_amd.particle_array import get_particle_array
    n = x.size
    pa = get_particle_array(
        name=name, constants=dict(coef=np.array([1.25, -0.5])),
        x=x + 0.1 * DX * rng.uniform(-1, 1, n), y=y + 0.1 * DX * rng.uniform(-1, 1, n),
        z=z + 0.1 * DX * rng.uniform(-1, 1, n),
        u=rng.uniform(-1, 1, n), v=rng.uniform(-1, 1, n), w=rng.uniform(-1, 1, n),
        h=1.3 * DX * (1 + varh * rng.uniform(-1, 1, n)),
        m=DX ** 3 * rng.uniform(0.8, 1.2, n), rho=1 + 0.1 * rng.uniform(-1, 1, n),
        additional_props=EXTRA)
    for k in EXTRA:
        pa.properties[k][:] = rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n)   # random, never zero
    pa.V[:] = DX ** 3 * rng.uniform(0.8, 1.2, n)
    pa.p[:] = rng.uniform(1, 2, n)
    pa.add_property('nrm', stride=3, data=rng.uniform(-1, 1, 3 * n))
    pa.add_property('tq', stride=3, data=rng.uniform(0.5, 1.5, 3 * n))
    return pa


def base_case(varh, seed=11, solid_rows=None, split_solid=False):
    """9^3 jittered lattice, `solid` the layers y < 4.5 dx (324 rows: five full
    wave tiles and a partial one), `fluid` the rest (405 rows); every field
    random, the forces of the solid random and non-zero."""
    rng = np.random.default_rng(seed)
    g = (np.arange(N1) + 0.5) * DX
    x, y, z = [a.ravel() for a in np.meshgrid(g, g, g, indexing='ij')]
    wall = y < 4.5 * DX
    fluid = _array('fluid', x[~wall], y[~wall], z[~wall], varh, rng)
    idx = np.nonzero(wall)[0]
    if solid_rows is not None:
        idx = idx[solid_rows]
    if not split_solid:
        return [fluid, _array('solid', x[idx], y[idx], z[idx], varh, rng)]
    lo = idx[x[idx] < 0.5]
    hi = idx[x[idx] >= 0.5]
    return [fluid, _array('solid', x[lo], y[lo], z[lo], varh, rng), _array('solid2', x[hi], y[hi], z[hi], varh, rng)]


def clone(arrays):
    out = []
    for pa in arrays:
        q = pa.extract_particles(np.arange(pa.get_number_of_particles()))
        q.set_num_real_particles(pa.get_number_of_particles(True))
        out.append(q)
    return out


def pair_equations(sources=('solid',), which='both', **group_kw):
    from pysph_amd.equations import Group
    from scatter_equations import AkinciPair, ScatterSink
    eqs = []
    if which in ('both', 'akinci'):
        eqs.append(AkinciPair('fluid', list(sources), rho0=1.1))
    if which in ('both', 'sink'):
        eqs.append(ScatterSink('fluid', list(sources)[:1], a=0.3, cut=0.6))
    return [Group(equations=eqs, **group_kw)]


def mixed_equations(python):
    """the scatter equations next to a hand-written WCSPH equation on the same destination and group (for the
    checker: the same equation as a Python body)"""
    from pysph_amd.equations import ContinuityEquation, Group
    from custom_equations import PyContinuity
    cont = (PyContinuity if python else ContinuityEquation)(dest='fluid', sources=['fluid', 'solid'])
    return [Group(equations=[cont] + pair_equations()[0].equations)]


def self_equations():
    from pysph_amd.equations import Group
    from scatter_equations import SelfScatter
    return [Group(equations=[SelfScatter('fluid', ['fluid'])])]


def make_eval(arrays, eqs, kernel, sync='auto', options=()):
    from pysph_amd import device as dev
    from pysph_amd.acceleration_eval import AccelerationEval, SPHCompiler
    from pysph_amd.nnps import HipNNPS
    ctx = dev.HipContext(0)
    for key, val in options:
        ctx.set_option(key, val)
    a_eval = AccelerationEval(arrays, eqs, kernel)
    SPHCompiler(a_eval, ctx=ctx, sync=sync).compile()
    nnps = HipNNPS(3, arrays, radius_scale=kernel.radius_scale, ctx=ctx)
    a_eval.set_nnps(nnps)
    return a_eval, nnps, ctx


def run_checker(oracle, ref, eqs, kernel, t=0.25, dt=1e-3):
    from oracle.py_eval import PyEval
    onn = oracle.OracleNNPS(3, ref, radius_scale=kernel.radius_scale)
    onn.update()
    PyEval(ref, eqs, kernel, onn).compute(t, dt)
    return onn


def neighbour_counts(onn, src, dst):
    """per row of array `dst`: its number of neighbours in array `src` (the checker's lists)"""
    cs, _ = onn.get_csr(src, dst)
    return np.diff(np.asarray(cs, dtype=np.int64))


def compare(arrays, ref, fields):
    worst = 0.0
    for pa, pr in zip(arrays, ref):
        for prop in fields.get(pa.name, ()):
            e = rel_err(pa.properties[prop], pr.properties[prop])
            print('%s.%s rel_err %.3e' % (pa.name, prop, e))
            worst = max(worst, e)
            assert e < TOL, (pa.name, prop, e)
    return worst


def kernel_of(name):
    from pysph_amd import kernels as K
    return getattr(K, name)(dim=3)


# ---------------------------------------------------------------------------
# the families of the GPU tests, built without a GPU (__graft_entry__.build())
# ---------------------------------------------------------------------------
def prebuild():
    from pysph_amd import codegen
    from pysph_amd import kernels as K
    from pysph_amd.acceleration_eval import AccelerationEval, _CGroup

    def plan(arrays, eqs, kernel):
        count = 0
        a = AccelerationEval(arrays, eqs, kernel)
        ids = dict((pa.name, i) for i, pa in enumerate(arrays))
        amap = dict((pa.name, pa) for pa in arrays)
        for g in a.equation_groups:
            for u in _CGroup(g, ids, amap, K.kernel_id(kernel)).units:
                if hasattr(u, 'fam'):
                    u.fam.flavour_f32().load()      # option arith_f32 (and the translation test) take the float build
                    count += 2
        return count

    def every():
        n = 0
        two = base_case(0.0)
        three = base_case(0.0, split_solid=True)
        for kname in ('CubicSpline', 'WendlandQuintic'):
            n += plan(two, pair_equations(), kernel_of(kname))
        cubic = kernel_of('CubicSpline')
        n += plan(two, mixed_equations(False), cubic)
        n += plan(two, pair_equations(which='akinci'), cubic)
        n += plan(three, pair_equations(sources=('solid', 'solid2'), which='akinci'), cubic)
        n += plan(two[:1], self_equations(), cubic)
        n += plan(two, product_equations(), cubic)
        return n
    codegen.DEFERRED = []
    every()
    codegen.build_deferred()
    return every()


def product_equations():
    from pysph_amd.equations import Group
    from pysph_amd import rigid_body as rb
    return [Group(equations=[rb.BodyForce('solid', None, gy=-9.81), rb.NumberDensity('solid', ['solid'])]),
            Group(equations=[rb.AkinciRigidFluidCoupling('fluid', ['solid'], fluid_rho=1.2),
                             rb.PressureRigidBody('fluid', ['solid'], rho0=1.1),
                             rb.ViscosityRigidBody('fluid', ['solid'], rho0=1.1, nu=0.05),
                             rb.LiuFluidForce('fluid', ['solid'])])]


# ---------------------------------------------------------------------------
# CPU tests
# ---------------------------------------------------------------------------
def _families(arrays, eqs, kernel_name='CubicSpline'):
    from pysph_amd import kernels as K
    from pysph_amd.acceleration_eval import AccelerationEval, _CGroup
    kernel = kernel_of(kernel_name)
    a = AccelerationEval(arrays, eqs, kernel)
    ids = dict((pa.name, i) for i, pa in enumerate(arrays))
    amap = dict((pa.name, pa) for pa in arrays)
    units = []
    for g in a.equation_groups:
        units += _CGroup(g, ids, amap, K.kernel_id(kernel)).units
    return units


def _pair_text(source):
    """the body of FamGen::pair in a generated source"""
    start = source.index('static __device__ __forceinline__ void pair(')
    return source[start:source.index('template <class A> static __device__ __forceinline__ void finish(')]


@pytest.mark.parametrize('which', ['test equations', 'rigid_body'])
def test_translation_forward_and_companion_build(which):
    """Both test equations and the classes of pysph_amd/rigid_body.py translate into a forward family without a
    store to a source pointer and a companion whose pair() stores to no destination output, and both build for
    gfx950 in both precisions."""
    arrays = base_case(0.15)
    eqs = pair_equations() if which == 'test equations' else product_equations()
    units = [u for u in _families(arrays, eqs) if hasattr(u, 'fam')]
    fwd = [u for u in units if u.fam.transposed is None and u.fam.companions]
    comp = [u for u in units if u.fam.transposed is not None]
    assert len(fwd) == 1 and len(comp) == 1 and fwd[0].fam.companions == [comp[0].fam]
    assert units.index(comp[0]) == units.index(fwd[0]) + 1          # runs directly behind its forward unit
    f, c = fwd[0].fam, comp[0].fam
    assert f.dest == 'fluid' and c.dest == 'solid' and c.sources == ['fluid'] and c.transposed == 'fluid'
    assert set(f.dout) == ({'au', 'av', 'aw', 'e'} if which == 'test equations' else {'au', 'av', 'aw'})
    want = {'fx', 'fy', 'fz', 'tq__0', 'tq__2'} if which == 'test equations' else set(FORCES)
    assert set(c.dout) == want and not (set(c.din) & want)
    # forward: nothing of a source is stored (sources are read through the packed records only)
    assert 's_fx' not in f.source and 'd_fx' not in f.source and 'sperm' not in f.source
    # companion: pair() accumulates into the lane's registers of the scattered properties and nothing else
    pair = _pair_text(c.source)
    stores = set(ln.split('+=')[0].split('-=')[0].strip() for ln in pair.split('\n')
                 if ('+=' in ln or '-=' in ln) and 'D.d_' in ln.split('=')[0])
    assert stores == set('D.d_%s' % p for p in want), stores
    assert 'a.p.dout' not in pair and 'D.d_au' not in c.source and 'D.d_e ' not in c.source
    assert 'PAIR_INDEX = true' in c.source and 'a.p.sperm[jg - a.src[0].off]' in pair
    for fam in (f, c):
        assert os.path.exists(fam.build()) and os.path.exists(fam.flavour_f32().build())
    if which == 'test equations':
        assert c.strides == {'tq': 3, 'nrm': 3}
        assert '#pragma clang fp contract(off)' in pair          # _fp_contract_ = False carries over


def _refused(loop_src, match, sources=('solid',), arrays=None, extra=(), dest='fluid', methods=''):
    import importlib.util
    import tempfile
    from pysph_amd.codegen import CodegenError, GeneratedFamily
    from pysph_amd.equations import Group
    src = ('from pysph_amd.equations import Equation\n\n\nclass Bad(Equation):\n' + methods +
           '    def loop(self, d_idx, s_idx, d_au, d_m, d_fx, s_fx, s_m, s_coef, XIJ, WIJ):\n' +
           ''.join('        %s\n' % ln for ln in loop_src))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'bad_scatter.py')
        with open(path, 'w') as f:
            f.write(src)
        spec = importlib.util.spec_from_file_location('bad_scatter', path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        arrays = arrays or base_case(0.0)
        amap = dict((pa.name, pa) for pa in arrays)
        eq = mod.Bad(dest, list(sources))
        with pytest.raises(CodegenError, match=match) as ei:
            if extra:
                _families(arrays, [Group(equations=list(extra) + [eq])])
            else:
                GeneratedFamily(dest, [eq], amap, 1, 'bad')
    return str(ei.value)


def test_refusals():
    """What stays refused with today's message, and the stores whose value depends on the order of the reference's
    loops (each names the equation, the line and the property)."""
    ro = 'read-only'
    _refused(['s_m[s_idx] = 1.0'], ro)                                       # plain assignment
    _refused(['s_fx[s_idx] *= 2.0'], ro)
    _refused(['k = declare("int")', 'k = 3', 's_fx[k] += 1.0'], ro)          # a run-time index
    _refused(['s_coef[0] += 1.0'], ro)                                       # a constant
    _refused(['d_au[d_idx] += WIJ'], ro,
             methods='    def post_loop(self, d_idx, s_idx, s_fx):\n        s_fx[s_idx] += 1.0\n\n')
    _refused(['d_au[d_idx] += WIJ'], ro,
             methods='    def initialize(self, d_idx, s_idx, s_fx):\n        s_fx[s_idx] += 1.0\n\n')
    _refused(['d_au[d_idx] += WIJ'], ro,
             methods='    def loop_all(self, d_idx, s_fx, NBRS, N_NBRS):\n        s_fx[NBRS[0]] += 1.0\n\n')
    _refused(['d_au[d_idx] += WIJ'], ro,
             methods='    def initialize_pair(self, d_idx, s_fx):\n        s_fx[d_idx] += 1.0\n\n')
    # 1. the value depends on a destination property the family writes: directly, through a local, through a condition
    order = r'Bad\.loop line \d+: s_fx\[s_idx\] \+= \.\.\. depends on d_au, which .* order of its loops'
    _refused(['d_au[d_idx] += WIJ', 's_fx[s_idx] += d_au[d_idx]'], order)
    _refused(['tmp = 2.0 * d_au[d_idx]', 'd_au[d_idx] += WIJ', 's_fx[s_idx] += tmp * WIJ'], order)
    _refused(['d_au[d_idx] += WIJ', 'if d_au[d_idx] > 1.0:', '    return', 's_fx[s_idx] += WIJ'], order)
    _refused(['s_fx[s_idx] += d_au[d_idx]'], order,
             methods='    def post_loop(self, d_idx, d_au):\n        d_au[d_idx] = 0.5 * d_au[d_idx]\n\n')
    # ... or that a hand-written unit of the same destination and group writes (by its table of properties)
    from pysph_amd.equations import MomentumEquation
    mom = MomentumEquation(dest='fluid', sources=['fluid'], c0=10.0, alpha=0.1, beta=0.0)
    wc = base_case(0.0)
    for prop in ('dt_cfl', 'dt_force'):
        wc[0].add_property(prop)
    _refused(['s_fx[s_idx] += d_au[d_idx] * WIJ'], order, extra=[mom], arrays=wc)
    # ... or on an equation attribute the same loop assigns (state carried from pair to pair)
    _refused(['self.count = self.count + 1.0', 's_fx[s_idx] += WIJ'],
             r'Bad\.loop line \d+: s_fx\[s_idx\] \+= \.\.\.: the same loop assigns self\.count \(line \d+\)',
             methods='    count = 0.0\n\n')
    # a constant of the source array is a scalar parameter of the family: one source only
    _refused(['d_au[d_idx] += s_coef[0] * WIJ'], 'exactly one source', sources=('solid', 'fluid'))
    # 2. an equation of the family reads the scattered property as s_*
    _refused(['d_au[d_idx] += s_fx[s_idx]', 's_fx[s_idx] += WIJ'],
             r'Bad\.loop line \d+: s_fx\[s_idx\] \+= \.\.\.: s_fx is also read')
    _refused(['s_m[s_idx] -= WIJ', 'd_au[d_idx] += s_m[s_idx]'], r's_m\[s_idx\] -= \.\.\.: s_m is also read')
    # 3. destination and source are the same array and the property is touched through d_*
    _refused(['d_fx[d_idx] += WIJ', 's_fx[s_idx] += WIJ'],
             r'Bad\.loop line \d+: s_fx\[s_idx\] \+= \.\.\.: destination and source are the same array', sources=('fluid',))
    # more properties of the original destination than a record holds: the existing error
    names = ['q%d' % k for k in range(21)]
    arrays = base_case(0.0)
    for pa in arrays:
        for nm in names:
            pa.add_property(nm)
    import importlib.util
    import tempfile
    from pysph_amd.codegen import CodegenError, GeneratedFamily
    src = ('from pysph_amd.equations import Equation\n\n\nclass Wide(Equation):\n    def loop(self, d_idx, s_idx, s_fx, %s):\n'
           '        s_fx[s_idx] += %s\n' % (', '.join('d_' + nm for nm in names), ' + '.join('d_%s[d_idx]' % nm for nm in names)))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'wide_scatter.py')
        with open(path, 'w') as f:
            f.write(src)
        spec = importlib.util.spec_from_file_location('wide_scatter', path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        with pytest.raises(CodegenError, match='more than 20 source properties'):
            GeneratedFamily('fluid', [mod.Wide('fluid', ['solid'])], dict((pa.name, pa) for pa in arrays), 1, 'wide')


def test_scatter_unit_refuses_a_slab_decomposed_array():
    """what a rank adds to a Remote row never reaches its owner: the unit raises before it launches, for the array
    written to and for the one it takes its neighbours from (SlabHalo marks the arrays it manages)"""
    for marked in (0, 1):
        arrays = base_case(0.0)
        units = _families(arrays, pair_equations())
        scatter = [u for u in units if getattr(u, 'fam', None) is not None and u.fam.transposed is not None]
        assert len(scatter) == 1
        scatter[0]._check(None)                         # nothing marked: passes
        arrays[marked].slab_decomposed = True
        with pytest.raises(NotImplementedError, match='slab-decomposed'):
            scatter[0].run(None, 0.0, 1e-3)             # refused before anything of the evaluation is touched
        for u in units:
            if u is not scatter[0]:
                u._check(None) if hasattr(u, '_check') else None
    import inspect
    from pysph_amd import parallel
    assert 'pa.slab_decomposed = True' in inspect.getsource(parallel.SlabHalo.__init__)


def test_example_sets_up_and_translates():
    """pysph_amd/examples/body_in_tank.py on the CPU: a symmetric block, no water inside or next to it, and
    equations that translate into the forward family and its companion behind the hand-written rates"""
    from pysph_amd.examples import body_in_tank as B
    for dx in (0.1, 0.05):
        fluid, tank, block = B.create_particles(dx)
        assert block.get_number_of_particles() > 0 and fluid.get_number_of_particles() > block.get_number_of_particles()
        assert abs(block.x.mean() - 0.5) < 1e-12 and abs(block.z.mean() - 0.5) < 1e-12
        gap = np.sqrt((fluid.x[:, None] - block.x[None, :]) ** 2 + (fluid.y[:, None] - block.y[None, :]) ** 2
                      + (fluid.z[:, None] - block.z[None, :]) ** 2).min()
        assert gap > 1.5 * dx
    arrays = B.create_particles(0.1)
    units = _families(arrays, B.create_equations(0.1))
    kinds = [type(u).__name__ for u in units]
    assert kinds[-2:] == ['_GeneratedUnit', '_ScatterUnit'] and kinds.count('_ScatterUnit') == 1
    assert units[-1].fam.dest == 'block' and set(units[-1].fam.dout) == set(FORCES)


def test_reference_classes_translate():
    """the reference's own four classes (where its sources are present, as tests/reference_census.py does)"""
    import json
    import subprocess
    import sys
    from conftest import REPO
    if not os.path.isdir('/root/reference/pysph'):
        pytest.skip('reference sources not present')
    out = subprocess.run([sys.executable, os.path.join(REPO, 'tests', 'reference_census.py')], cwd=REPO,
                         stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
    res = json.loads(out.strip().split('\n')[-1])
    for name in ('AkinciRigidFluidCoupling', 'PressureRigidBody', 'ViscosityRigidBody', 'LiuFluidForce'):
        full = 'pysph.sph.rigid_body.' + name
        assert full in res['ok'], res['bad'].get(full)


def test_product_bodies_reproduce_the_reference_classes(oracle):
    """tests/golden/rigid_coupling.npz: the reference's own classes run by PyEval on the two-array case
    (tests/golden/make_rigid_coupling_golden.py); the bodies of pysph_amd/rigid_body.py, run the same way on the
    recorded inputs, give the recorded outputs."""
    import sys
    if GOLDEN not in sys.path:
        sys.path.append(GOLDEN)
    import make_rigid_coupling_golden as mk
    g = np.load(os.path.join(GOLDEN, 'rigid_coupling.npz'))
    arrays = mk.arrays_from(g, 'in')
    from pysph_amd import rigid_body as rb
    run_checker(oracle, arrays, mk.equations(rb), kernel_of('CubicSpline'))
    checked = 0
    for pa in arrays:
        for prop in mk.OUTPUTS[pa.name]:
            e = rel_err(pa.properties[prop], g['out/%s/%s' % (pa.name, prop)])
            print('%s.%s rel_err %.3e' % (pa.name, prop, e))
            assert e < TOL, (pa.name, prop, e)
            assert not np.array_equal(g['out/%s/%s' % (pa.name, prop)], g['in/%s/%s' % (pa.name, prop)])
            checked += 1
    assert checked == 7


# ---------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------
def _check_geometry(onn, arrays):
    """the case cannot pass vacuously: at least half of the solid rows have a fluid neighbour, at least one has
    none.  Returns the solid rows without one."""
    cnt = neighbour_counts(onn, 0, 1)       # per solid row: neighbours among the fluid
    assert cnt.size == arrays[1].get_number_of_particles()
    assert 2 * np.count_nonzero(cnt) >= cnt.size, (np.count_nonzero(cnt), cnt.size)
    assert (cnt == 0).any()
    return np.nonzero(cnt == 0)[0]


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['uniform-CubicSpline', 'uniform-WendlandQuintic', 'varh-CubicSpline',
                                  'varh-WendlandQuintic', 'uniform-CubicSpline-mixed'])
def test_scatter_parity(oracle, case):
    """A: forward outputs on the fluid and scattered outputs on the solid against PyEval; rows of the solid
    without a fluid neighbour come back bit-identical."""
    parts = case.split('-')
    arrays = base_case(0.15 if parts[0] == 'varh' else 0.0)
    assert arrays[1].get_number_of_particles() == 324 < arrays[0].get_number_of_particles()
    ref, before = clone(arrays), clone(arrays)
    kernel = kernel_of(parts[1])
    mixed = len(parts) == 3
    a_eval, nnps, ctx = make_eval(arrays, mixed_equations(False) if mixed else pair_equations(), kernel)
    a_eval.compute(0.25, 1e-3)
    onn = run_checker(oracle, ref, mixed_equations(True) if mixed else pair_equations(), kernel)
    alone = _check_geometry(onn, ref)
    compare(arrays, ref, {'fluid': FLUID_OUT + (('arho',) if mixed else ()), 'solid': SOLID_OUT})
    for prop in FORCES:
        assert (before[1].properties[prop] != 0).all()
        assert np.array_equal(arrays[1].properties[prop][alone], before[1].properties[prop][alone])
        assert not np.array_equal(arrays[1].properties[prop], before[1].properties[prop])
    tq, tq0 = arrays[1].tq.reshape(-1, 3), before[1].tq.reshape(-1, 3)
    assert np.array_equal(tq[alone], tq0[alone]) and np.array_equal(tq[:, 1], tq0[:, 1])


@pytest.mark.gpu
@pytest.mark.parametrize('how', ['real', 'start_stop'])
def test_scatter_range_filter(oracle, how):
    """B: the transposed launch takes neighbours from exactly the rows the forward loop visits -- not from the
    non-real rows of the fluid under Group(real=True), not from the rows outside [start_idx, stop_idx) -- although
    those rows have solid neighbours."""
    arrays = base_case(0.0)
    n = arrays[0].get_number_of_particles()
    if how == 'real':
        nreal = n - 60                      # the last 60 rows: the slab x = 8.5 dx and a part of the one before
        arrays[0].tag[nreal:] = 2
        arrays[0].set_num_real_particles(nreal)
        eqs = pair_equations(real=True)
        excluded = np.arange(nreal, n)
    else:
        eqs = pair_equations(real=False, start_idx=37, stop_idx=263)    # neither is a multiple of 64
        excluded = np.concatenate([np.arange(37), np.arange(263, n)])
    ref, unfiltered = clone(arrays), clone(arrays)
    kernel = kernel_of('CubicSpline')
    a_eval, nnps, ctx = make_eval(arrays, eqs, kernel)
    a_eval.compute(0.25, 1e-3)
    onn = run_checker(oracle, ref, eqs, kernel)
    _check_geometry(onn, ref)
    cnt = neighbour_counts(onn, 1, 0)       # per fluid row: neighbours among the solid
    assert cnt[excluded].sum() > 0 and cnt[np.setdiff1d(np.arange(n), excluded)].sum() > 0
    compare(arrays, ref, {'fluid': FLUID_OUT, 'solid': SOLID_OUT})
    # a missing filter changes the answer: the checker over ALL rows differs from it far beyond the tolerance
    unfiltered[0].set_num_real_particles(n)
    run_checker(oracle, unfiltered, pair_equations(real=False), kernel)
    assert max(rel_err(unfiltered[1].properties[p], ref[1].properties[p]) for p in FORCES) > 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize('shape', ['small', 'empty', 'two_sources', 'same_array'])
def test_scatter_shapes_at_the_edges(oracle, shape):
    """C: a source array of fewer than 64 rows, an empty one, two source arrays written to by one family, and
    destination = source with a property that is only ever added to."""
    kernel = kernel_of('CubicSpline')
    if shape == 'small':
        arrays, eqs = base_case(0.0, solid_rows=np.arange(284, 324)), pair_equations()    # 40 rows next to the fluid
        fields = {'fluid': FLUID_OUT, 'solid': SOLID_OUT}
        assert arrays[1].get_number_of_particles() == 40
    elif shape == 'empty':
        arrays, eqs = base_case(0.0, solid_rows=np.arange(0)), pair_equations()
        fields = {'fluid': FLUID_OUT, 'solid': SOLID_OUT}
        assert arrays[1].get_number_of_particles() == 0
    elif shape == 'two_sources':
        arrays = base_case(0.0, split_solid=True)
        eqs = pair_equations(sources=('solid', 'solid2'), which='akinci')
        fields = {'fluid': FLUID_OUT[:3], 'solid': FORCES, 'solid2': FORCES}
    else:
        arrays, eqs = base_case(0.0)[:1], self_equations()
        fields = {'fluid': ('gsum',)}
    ref, before = clone(arrays), clone(arrays)
    a_eval, nnps, ctx = make_eval(arrays, eqs, kernel)
    a_eval.compute(0.25, 1e-3)
    run_checker(oracle, ref, eqs, kernel)
    compare(arrays, ref, fields)
    if shape != 'empty':
        for pa, pb in zip(arrays[-1:], before[-1:]):
            for prop in fields[pa.name]:
                assert not np.array_equal(pa.properties[prop], pb.properties[prop])


@pytest.mark.gpu
def test_scatter_action_equals_reaction(oracle):
    """D (fp64, the Akinci pair alone): |sum_d m_d a_d + sum_s (f_s - f0_s)| <= 2^-52 (n_max + n_rows + 4) T per
    component, T = the sum of |m_d term| over all pairs evaluated by the checker, n_max the largest neighbour count,
    n_rows the rows of the two host sums.

    Derivation (u = 2^-53): both launches form the SAME rounded ax for a pair (one operation order, no contraction,
    symmetric geometry).  Forward sum of a row: (n_d - 1) u sum|ax|; the host's m_d a_d: u m_d sum|ax|; the
    device's m_d ax per pair: u |m_d ax|; the transposed sum of a row: (n_s - 1) u sum|m_d ax|; the read-modify-write
    and the host's f - f0: u (|f0| + 2 |acc|) per row, with sum|f0| <= T (asserted) at most 3 u T; the host sums are
    exactly rounded (math.fsum): u |result| each.  Together less than u T (2 n_max + 5) < 2^-52 (n_max + 3) T."""
    from pysph_amd.equations import Group
    from scatter_equations import AkinciPair

    class AkinciAbs(AkinciPair):            # checker only: T per component, into the fluid's gsum / q / e
        def loop(self, d_idx, s_idx, d_m, d_rho, d_p, d_gsum, d_q, d_e, s_V, DWIJ):
            psi = self.rho0 * s_V[s_idx]
            coef = -psi * d_p[d_idx] / (d_rho[d_idx] * d_rho[d_idx])
            d_gsum[d_idx] += abs(d_m[d_idx] * (coef * DWIJ[0]))
            d_q[d_idx] += abs(d_m[d_idx] * (coef * DWIJ[1]))
            d_e[d_idx] += abs(d_m[d_idx] * (coef * DWIJ[2]))
    kernel = kernel_of('CubicSpline')
    arrays = base_case(0.15)
    fluid, solid = arrays
    tarr = clone(arrays)
    for k in ('gsum', 'q', 'e'):
        tarr[0].properties[k][:] = 0.0
    onn = run_checker(oracle, tarr, [Group(equations=[AkinciAbs('fluid', ['solid'], rho0=1.1)])], kernel)
    _check_geometry(onn, tarr)
    T = [math.fsum(tarr[0].properties[k]) for k in ('gsum', 'q', 'e')]
    n_max = int(max(neighbour_counts(onn, 0, 1).max(), neighbour_counts(onn, 1, 0).max()))
    n_rows = fluid.get_number_of_particles() + solid.get_number_of_particles()
    rng = np.random.default_rng(3)
    for c, (a, f) in enumerate(zip(('au', 'av', 'aw'), FORCES)):
        fluid.properties[a][:] = 0.0
        solid.properties[f][:] = rng.uniform(0.25, 0.5, solid.x.size) * rng.choice([-1.0, 1.0], solid.x.size) \
            * T[c] / solid.x.size
        assert (solid.properties[f] != 0).all() and np.abs(solid.properties[f]).sum() <= T[c]
    f0 = clone(arrays)[1]
    a_eval, nnps, ctx = make_eval(arrays, pair_equations(which='akinci'), kernel)
    a_eval.compute(0.25, 1e-3)
    for c, (a, f) in enumerate(zip(('au', 'av', 'aw'), FORCES)):
        action = math.fsum(fluid.m * fluid.properties[a])
        reaction = math.fsum(solid.properties[f] - f0.properties[f])
        bound = 2.0 ** -52 * (n_max + n_rows + 4) * T[c]
        print('%s: action %.17g reaction %.17g sum %.3e bound %.3e (T %.6g, n_max %d, n_rows %d)'
              % (f, action, reaction, action + reaction, bound, T[c], n_max, n_rows))
        assert abs(action) > 1e3 * bound
        assert abs(action + reaction) <= bound, (f, action + reaction, bound)


SCHEDULES = [(), (('row_mod3', 3),), (('row_mod3', 4),), (('norm_masks', 0),)]


@pytest.mark.gpu
def test_scatter_is_deterministic_under_every_schedule():
    """E: two evaluations from the same restored state give bit-identical scattered (and forward) fields -- with
    the default schedule and with the context options row_mod3 and norm_masks toggled.  Between the settings the
    launches behave as every launch of the skeleton does (tests/test_schedules.py): norm_masks on / off is
    bit-identical; row_mod3 changes the order in which a lane meets its neighbours, that is the order of its sum and
    nothing else, so those results agree to rounding (held to the parity tolerance; measured on an MI355X: row_mod3 = 3 came out
    bit-identical on this case, row_mod3 = 4 within 3.3e-16 of each field's maximum)."""
    kernel = kernel_of('CubicSpline')
    start = base_case(0.15)
    first = {}
    for options in SCHEDULES:
        arrays = clone(start)
        a_eval, nnps, ctx = make_eval(arrays, pair_equations(), kernel, options=options)
        a_eval.compute(0.25, 1e-3)
        once = clone(arrays)
        for pa, p0 in zip(arrays, start):           # the host arrays are authoritative (sync='auto'): restore, again
            for k in pa.properties:
                pa.properties[k][:] = p0.properties[k]
        a_eval.compute(0.25, 1e-3)
        for pa, pb, fields in zip(arrays, once, (FLUID_OUT, SOLID_OUT)):
            for prop in fields:
                assert np.array_equal(pa.properties[prop], pb.properties[prop]), (options, pa.name, prop)
        first[options] = once
    base = first[()]
    assert not np.array_equal(base[1].fx, start[1].fx)
    for options in SCHEDULES[1:]:
        for pa, pb, fields in zip(first[options], base, (FLUID_OUT, SOLID_OUT)):
            for prop in fields:
                same = np.array_equal(pa.properties[prop], pb.properties[prop])
                e = rel_err(pa.properties[prop], pb.properties[prop])
                print('%s vs default: %s.%s %s (rel_err %.3e)' % (options, pa.name, prop,
                                                                 'bit-identical' if same else 'differs', e))
                if options[0][0] == 'norm_masks':
                    assert same, (options, pa.name, prop)
                else:
                    assert e < TOL, (options, pa.name, prop, e)


@pytest.mark.gpu
def test_scatter_float_builds(oracle):
    """F: option arith_f32 runs the float builds of both launches; judged as
    test_generated_families_fp32_arithmetic_vs_python judges the same kind of sum: 5e-5 of each field's maximum,
    and it must really be another precision."""
    kernel = kernel_of('CubicSpline')
    arrays = base_case(0.0)
    ref = clone(arrays)
    a_eval, nnps, ctx = make_eval(arrays, pair_equations(), kernel, options=(('arith_f32', 1),))
    a_eval.compute(0.25, 1e-3)
    run_checker(oracle, ref, pair_equations(), kernel)
    for pa, pr, fields in zip(arrays, ref, (FLUID_OUT, SOLID_OUT)):
        worst = 0.0
        for prop in fields:
            got, want = pa.properties[prop], pr.properties[prop]
            e = np.abs(got - want).max() / max(np.abs(want).max(), 1e-300)
            print('arith_f32 %s.%s: %.3e of the field maximum' % (pa.name, prop, e))
            worst = max(worst, e)
            assert e <= 5e-5, (pa.name, prop, e)
        # each launch on its own: the forward one writes the fluid, the transposed one the solid
        assert worst > 1e-10, 'the float build of the launch that writes %s was not the one that ran' % pa.name


@pytest.mark.gpu
def test_scatter_sync_modes(oracle):
    """G: with sync='auto' the host arrays of the solid hold the new forces after compute; device-resident
    (sync='manual') they do not until they are pulled."""
    kernel = kernel_of('CubicSpline')
    arrays = base_case(0.0)
    ref, before = clone(arrays), clone(arrays)
    run_checker(oracle, ref, pair_equations(), kernel)
    a_eval, nnps, ctx = make_eval(arrays, pair_equations(), kernel, sync='manual')
    # device-resident: the caller moves the data -- every input of the plan by name (pa.gpu.push() without names
    # takes the built-in properties only), the scattered properties of the solid among them
    hip_eval = a_eval.c_acceleration_eval
    assert set(SOLID_OUT[:3]) | {'tq__0', 'tq__2'} <= hip_eval.inputs['solid'] & hip_eval.outputs_exact['solid']
    hip_eval.push_inputs()
    nnps.update()
    a_eval.compute(0.25, 1e-3)
    ctx.synchronize()
    for prop in SOLID_OUT:
        assert np.array_equal(arrays[1].properties[prop], before[1].properties[prop])
    arrays[1].gpu.pull(*(FORCES + ('tq__0', 'tq__2')))       # a strided property travels as its components
    arrays[0].gpu.pull(*FLUID_OUT)
    compare(arrays, ref, {'fluid': FLUID_OUT, 'solid': SOLID_OUT})
    auto = clone(before)
    a_eval, nnps, ctx = make_eval(auto, pair_equations(), kernel, sync='auto')
    a_eval.compute(0.25, 1e-3)
    compare(auto, ref, {'fluid': FLUID_OUT, 'solid': SOLID_OUT})
    for prop in SOLID_OUT:
        assert np.array_equal(auto[1].properties[prop], arrays[1].properties[prop])
