"""The front of the WCSPH step: the Tait EOS absorbed by record packing (sph_group.src_eos = 3, option eos_absorb)
against the EOS kernel followed by packing (eos_absorb 0: the host keeps the EOS group and promises src_eos = 1).

Both forms run ONE device function for p and cs and the same expression for p / rho^2, so every comparison here is
bit for bit (the doubles as uint64: NaN and the sign of zero count).  The cases that cannot absorb the equation --
several arrays, h and m that vary, an exponent other than 7, the HG-corrected EOS, a split evaluation -- must fall
back to the EOS kernel, with the same bits again and counter n_eos_absorbed unchanged."""
import ctypes as C
import functools

import numpy as np
import pytest

from helpers import WC_OUT
from test_hip_parity import make_eval, cube_equations

pytestmark = pytest.mark.gpu

OUT = sorted(set(WC_OUT) | {'p', 'cs'})
RHO0 = 1000.0


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def lattice_array(n, n_ghost=0, varh=0.0, varm=0.0, seed=5):
    """the first n points of a jittered cubic lattice; rho[0] = rho0 exactly, rho[1] = 0 (n >= 3: the p / rho^2
    guard); the last n_ghost rows are ghosts (no destinations, but the EOS covers them)"""
    from pysph_amd.particle_array import get_particle_array_wcsph
    rng = np.random.default_rng(seed + n)
    m1 = int(np.ceil(n ** (1.0 / 3.0) - 1e-9))
    dx = 1.0 / 16
    g = np.arange(m1) * dx
    c = np.array([a.ravel() for a in np.meshgrid(g, g, g, indexing='ij')]).T[:n].copy()
    c += 0.1 * dx * rng.uniform(-1, 1, c.shape)
    rho = RHO0 * (1 + 0.02 * rng.uniform(-1, 1, n))
    rho[0] = RHO0
    if n >= 3:
        rho[1] = 0.0
    pa = get_particle_array_wcsph(
        name='fluid', x=c[:, 0].copy(), y=c[:, 1].copy(), z=c[:, 2].copy(),
        h=1.3 * dx * (1 + varh * rng.uniform(-1, 1, n)), m=RHO0 * dx ** 3 * (1 + varm * rng.uniform(-1, 1, n)),
        rho=rho, u=rng.uniform(-1, 1, n), v=rng.uniform(-1, 1, n), w=rng.uniform(-1, 1, n))
    if n_ghost:
        pa.set_num_real_particles(n - n_ghost)
    return pa, dx


def two_evaluations(make, absorb, opts=(), nupdates=2):
    """[outputs after the first evaluation, ... after the second], the counters.  Device-resident (sync='manual': a
    host that pushed m before every evaluation would never see the uniform-mass records); the second evaluation
    follows a second neighbour update, as those records only engage then."""
    from pysph_amd import kernels as K
    arrays, eqs = make()
    for pa in arrays:                    # whatever the evaluation leaves in p and cs, it computed
        pa.p[:] = -1.0
        pa.cs[:] = -1.0
    a_eval, nnps, ctx = make_eval(arrays, eqs, K.WendlandQuintic(dim=3), 3, 6, sync='manual')
    try:
        ctx.set_option('eos_absorb', absorb)
        ctx.timer_enable(True)           # (timer 'eos' counts the launches of the EOS kernel only while timing is on)
        for k, v in opts:
            ctx.set_option(k, v)
        for pa in arrays:
            pa.gpu.push()
        nnps.sync = False
        got = []
        for rep in range(nupdates):
            nnps.update()
            a_eval.compute(0.0, 1e-5)
            a_eval.c_acceleration_eval.pull_outputs()
            for pa in arrays:
                pa.gpu.pull('p', 'cs')
            got.append({(pa.name, k): np.array(pa.properties[k]) for pa in arrays for k in OUT if k in pa.properties})
            for pa in arrays:
                pa.p[:] = -1.0
                pa.cs[:] = -1.0
                pa.gpu.push('p', 'cs')
        cnt = {k: ctx.timer_get(k)[1] for k in ('n_eos_absorbed', 'n_eos_fused', 'n_mass_fused', 'n_merged', 'eos')}
    finally:
        ctx.close()
    return got, cnt


def assert_same_bits(on, off, what):
    assert len(on) == len(off)
    for rep, (a, b) in enumerate(zip(on, off)):
        assert sorted(a) == sorted(b)
        for key in a:
            same = _bits(a[key]) == _bits(b[key])
            assert same.all(), (what, 'evaluation %d' % rep, key, int((~same).sum()), np.flatnonzero(~same)[:4])


@pytest.mark.parametrize('f32', [0, 1], ids=['fp64', 'fp32'])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 255, 256, 257, 513])
def test_absorbed_eos_matches_the_eos_kernel(n, f32):
    """counts around the wavefront and around the whole-block LDS store path of emit_pieces and its per-lane tail;
    rho = rho0 exactly and rho = 0; trailing ghosts (n >= 63); layout 6 (fp64) and 7 (arith_f32)"""
    n_ghost = n // 8

    def make():
        pa, dx = lattice_array(n, n_ghost)
        return [pa], cube_equations(dx)
    opts = (('arith_f32', 1),) if f32 else ()
    on, c_on = two_evaluations(make, 1, opts)
    off, c_off = two_evaluations(make, 0, opts)
    assert c_on['n_eos_absorbed'] == 2 and c_off['n_eos_absorbed'] == 0, (c_on, c_off)
    assert c_on['n_eos_fused'] == 2 and c_off['n_eos_fused'] == 2, (c_on, c_off)
    assert c_on['n_mass_fused'] == 1 and c_off['n_mass_fused'] == 1, (c_on, c_off)    # the second evaluation's records
    assert_same_bits(on, off, (n, f32))
    # ... and the EOS did cover the ghosts and the density 0: p0 = 0, so p(0) = -B exactly and cs(0) = 0
    from pysph_amd.examples import dam_break_3d as db
    for res in on:
        p, cs = res[('fluid', 'p')], res[('fluid', 'cs')]
        assert not np.any(cs == -1.0) and np.all(cs[2:] > 0.5 * db.c0)
        if n >= 3:
            assert p[1] == -(RHO0 * db.c0 * db.c0 / db.gamma) and cs[1] == 0.0


def _fallback(make, opts=()):
    on, c_on = two_evaluations(make, 1, opts)
    off, c_off = two_evaluations(make, 0, opts)
    assert c_on['n_eos_absorbed'] == 0 and c_off['n_eos_absorbed'] == 0, (c_on, c_off)
    assert c_on['eos'] == c_off['eos'] > 0, (c_on, c_off)     # as many EOS launches as the kept group makes
    return on, off, c_on


def test_fallback_variable_h_and_mixed_masses():
    def make():
        pa, dx = lattice_array(513, 64, varh=0.15, varm=0.2)
        return [pa], cube_equations(dx)
    on, off, cnt = _fallback(make)
    assert cnt['n_eos_fused'] == 0
    assert_same_bits(on, off, 'variable h, mixed masses')


def test_fallback_three_arrays_on_the_merged_order():
    from pysph_amd.examples import dam_break_3d as db

    def make():
        dx = 0.1
        arrays = db.create_particles(dx)
        rng = np.random.default_rng(3)
        for pa in arrays:
            pa.rho[:] = db.ro * (1 + 0.02 * rng.uniform(-1, 1, pa.get_number_of_particles()))
        return arrays, db.create_scheme(dx).get_equations()
    on, off, cnt = _fallback(make)
    assert cnt['n_merged'] > 0
    assert_same_bits(on, off, 'dam break, three arrays')


def test_fallback_exponent_three():
    from pysph_amd.scheme import WCSPHScheme
    from pysph_amd.examples import dam_break_3d as db

    def make():
        pa, dx = lattice_array(257, 32)
        s = WCSPHScheme(['fluid'], [], dim=3, rho0=db.ro, c0=db.c0, h0=1.3 * dx, hdx=1.3, gz=-9.81, alpha=db.alpha,
                        beta=db.beta, gamma=3.0)
        return [pa], s.get_equations()
    on, off, cnt = _fallback(make)
    assert cnt['n_eos_fused'] == 2
    assert_same_bits(on, off, 'gamma = 3')


def test_fallback_hg_corrected_eos():
    def make():
        pa, dx = lattice_array(257, 32)
        return [pa], _hg_equations(dx)
    on, off, cnt = _fallback(make)
    assert_same_bits(on, off, 'HG-corrected EOS')
    assert on[0][('fluid', 'rho')].min() >= RHO0          # the correction wrote rho


def _hg_equations(dx):
    from pysph_amd.equations import Group, TaitEOSHGCorrection
    from pysph_amd.examples import dam_break_3d as db
    eqs = cube_equations(dx)
    assert [type(e).__name__ for e in eqs[0].equations] == ['TaitEOS']
    eqs[0] = Group(real=False, equations=[TaitEOSHGCorrection(dest='fluid', sources=None, rho0=db.ro, c0=db.c0,
                                                              gamma=db.gamma)])
    return eqs


def _split_evaluation(absorb):
    """compute_begin / compute_end around the arrival of trailing ghosts, one array, device-resident"""
    from pysph_amd import device as dev
    from pysph_amd import kernels as K
    nreal, ng = 400, 113
    n = nreal + ng
    pa, dx = lattice_array(n)
    order = np.argsort(pa.x, kind='stable')               # the ghosts: the slab of largest x
    for k in list(pa.properties):
        pa.properties[k][:] = pa.properties[k][order]
    cut = 0.5 * (pa.x[nreal - 1] + pa.x[nreal])
    pa.set_num_real_particles(nreal)
    a_eval, nnps, ctx = make_eval([pa], cube_equations(dx), K.WendlandQuintic(dim=3), 3, 6, sync='manual')
    try:
        ctx.set_option('eos_absorb', absorb)
        ctx.timer_enable(True)
        ce = a_eval.c_acceleration_eval
        assert ce.can_split()
        pa.gpu.push()
        nnps.sync = False
        for rep in range(2):
            dev._check(ctx.lib.sph_array_resize(ctx._h, pa.gpu.array_id, nreal, nreal))
            nnps.set_ghost_faces(0, -1e30, cut)
            nnps.update()
            ce.compute_begin(0.0, 1e-5)
            dev._check(ctx.lib.sph_array_resize(ctx._h, pa.gpu.array_id, n, nreal))
            nnps.update_ghosts(0, -1e30, cut)
            ce.compute_end(0.0, 1e-5)
        ce.pull_outputs()
        pa.gpu.pull('p', 'cs')
        cnt = {k: ctx.timer_get(k)[1] for k in ('n_eos_absorbed', 'n_phase2', 'eos')}
        got = {('fluid', k): np.array(pa.properties[k]) for k in OUT}
    finally:
        ctx.close()
    return [got], cnt


def test_fallback_split_evaluation():
    on, c_on = _split_evaluation(1)
    off, c_off = _split_evaluation(0)
    assert c_on['n_eos_absorbed'] == 0 and c_off['n_eos_absorbed'] == 0, (c_on, c_off)
    assert c_on['n_phase2'] == 2 and c_on['eos'] == c_off['eos'] > 0, (c_on, c_off)
    assert_same_bits(on, off, 'compute_begin / compute_end')


def _step_around_fp64_calls(n, opts=(), middle=True, lacking=None):
    """One array of n jittered-lattice points, device-resident: evaluate the TaitEOS + Continuity / Momentum step, then
    (`middle`) the calls that are fp64 by contract on the same context -- neighbour lists, a Shepard and an order-1
    interpolation -- then update and evaluate again.  `lacking`: a property the pair loop requires, left off the device
    for the first evaluation -- which must fail with SPH_ERR_MISSING_PROP once its records are chosen -- and pushed
    before the second.  -> {'out': outputs of the second evaluation, 'lists': (start, nbrs), 'interp': [values]}"""
    from pysph_amd import device as dev
    from pysph_amd import kernels as K
    from pysph_amd.interpolator import _METHOD_IDS
    from pysph_amd.nnps import HipNNPS
    from pysph_amd.particle_array import get_particle_array
    pa, dx = lattice_array(n)
    pa.p[:] = -1.0
    pa.cs[:] = -1.0
    kernel = K.WendlandQuintic(dim=3)
    a_eval, nnps, ctx = make_eval([pa], cube_equations(dx), kernel, 3, 6, sync='manual')
    res = {}
    try:
        for k, v in opts:
            ctx.set_option(k, v)
        pa.gpu.push(*[k for k in pa.properties if dev.prop_id(k) >= 0 and k != lacking])
        nnps.sync = False
        nnps.update()
        if lacking:
            with pytest.raises(dev.SphError, match='error -5'):
                a_eval.compute(0.0, 1e-5)
            assert ctx.timer_get('n_eos_absorbed')[1] == 1      # the records that absorb the EOS were chosen already
        else:
            a_eval.compute(0.0, 1e-5)
        if middle:
            res['lists'] = nnps.get_csr(0, 0)
            m1 = int(np.ceil(n ** (1.0 / 3.0) - 1e-9))
            pts = np.random.default_rng(11).uniform(-0.5 * dx, (m1 - 0.5) * dx, (3, 24))
            # (through the C-ABI: the Interpolator class sizes a default mesh from the sources' extent, which one point lacks)
            pts_pa = get_particle_array(name='interpolate', x=pts[0], y=pts[1], z=pts[2], h=pa.h[0] * np.ones(24))
            hd = dev.attach(pts_pa, ctx)
            hd.push('x', 'y', 'z', 'h')
            HipNNPS(3, [pa, pts_pa], radius_scale=kernel.radius_scale, ctx=ctx, sync=False)
            ck = dev.SphKernel(K.kernel_id(kernel), 3, kernel.fac, kernel.radius_scale, kernel.get_deltap())
            src, prop = (C.c_int * 1)(pa.gpu.array_id), (C.c_int * 1)(dev.prop_id('u'))
            res['interp'] = []
            for method, nout in (('shepard', 1), ('order1', 4)):
                host = np.empty((nout, 24))
                dev._check(ctx.lib.sph_interpolate(ctx._h, C.byref(ck), _METHOD_IDS[method], hd.array_id, 1, src, 1, prop, None,
                                                   host.ctypes.data_as(dev._PD), 24))
                res['interp'] += list(host)
        if lacking:
            pa.gpu.push(lacking)
        nnps.update()
        a_eval.compute(0.0, 1e-5)
        a_eval.c_acceleration_eval.pull_outputs()
        pa.gpu.pull('p', 'cs')
        res['out'] = {('fluid', k): np.array(pa.properties[k]) for k in OUT}
        res['x'] = np.stack([pa.x, pa.y, pa.z], axis=1)
        res['hr'] = kernel.radius_scale * pa.h[0]
    finally:
        ctx.close()
    return res


@functools.lru_cache(maxsize=None)
def _fp64_reference(n):
    """the same sequence on a context whose options arith_f32 and record_f32 are 0"""
    return _step_around_fp64_calls(n)


def _assert_fp64_calls_same_bits(got, want, what):
    for a, b in zip(got['lists'], want['lists']):
        assert np.array_equal(a, b), (what, 'neighbour lists')
    assert len(got['interp']) == len(want['interp']) == 5
    for k, (a, b) in enumerate(zip(got['interp'], want['interp'])):
        assert np.array_equal(_bits(a), _bits(b)), (what, 'interpolation', k)


# below, at and above one wavefront, and above one 256-thread pack block
SMALL_N = [1, 64, 65, 257]


@pytest.mark.parametrize('option', ['arith_f32', 'record_f32'])
@pytest.mark.parametrize('n', SMALL_N)
def test_precision_options_do_not_leak_into_fp64_calls(n, option):
    """neighbour lists and the interpolator are fp64 whatever arith_f32 / record_f32 say, and leave both options and
    the records of the evaluation around them as they were"""
    opts = ((option, 1),)
    with_calls = _step_around_fp64_calls(n, opts)
    without = _step_around_fp64_calls(n, opts, middle=False)
    assert_same_bits([with_calls['out']], [without['out']], (n, option, 'second evaluation'))
    _assert_fp64_calls_same_bits(with_calls, _fp64_reference(n), (n, option))
    if n > 1:       # the option is in force: the outputs are not those of the fp64 context
        assert any((_bits(with_calls['out'][k]) != _bits(_fp64_reference(n)['out'][k])).any() for k in with_calls['out'])


@pytest.mark.parametrize('n', SMALL_N)
def test_failed_evaluation_leaves_nothing_behind(n):
    """the absorbable group on an array whose device copy lacks w: SPH_ERR_MISSING_PROP after the EOS-absorbing records
    were chosen; the fp64 calls behind it, and the same group once w is there, are those of a context that never failed"""
    failed = _step_around_fp64_calls(n, lacking='w')
    x, (start, nbrs) = failed['x'], failed['lists']
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2)
    near = d2 < failed['hr'] ** 2
    assert np.array_equal(start, np.concatenate([[0], np.cumsum(near.sum(axis=1))]))
    assert np.array_equal(nbrs, np.nonzero(near)[1])            # (rows in ascending order, as get_csr returns them)
    _assert_fp64_calls_same_bits(failed, _fp64_reference(n), n)
    assert_same_bits([failed['out']], [_fp64_reference(n)['out']], (n, 'evaluation after the failed one'))


def test_plan_marks_the_absorbable_group_only():
    """the host side: which EOS group annotate_plan hands to the pair group after it (no launch involved)"""
    from pysph_amd import kernels as K
    pa, dx = lattice_array(65)
    for hg in (False, True):
        eqs = _hg_equations(dx) if hg else cube_equations(dx)
        a_eval, nnps, ctx = make_eval([pa], eqs, K.WendlandQuintic(dim=3), 3, 6)
        try:
            plan = a_eval.c_acceleration_eval.plan
            (g0, cg0), (g1, cg1) = plan[0], plan[1]
            assert cg1.units[0].cg.src_eos == 1            # the promise itself is what it was
            assert (cg0.eos_absorbed_by is cg1) == (not hg) and cg1.absorbs_eos == (not hg)
            ce = a_eval.c_acceleration_eval
            assert cg1.will_absorb(ce) == (not hg)
            ctx.set_option('eos_absorb', 0)
            assert not cg1.will_absorb(ce)
        finally:
            ctx.close()
