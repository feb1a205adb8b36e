"""The neighbour search and the pair kernel at geometric edges: domains scaled by powers of two, translated far from
the origin, very elongated and sparse, particles far outside fixed grid bounds, pairs exactly ON the neighbour cutoff
and lattices whose points lie on cell faces -- against the CPU oracle on the same doubles.

Every case runs pair variant 0 (per-particle 27-cell walk, no fp32 prefilter: the in-product cross-check) and
variant 6 (the wave-tile kernel with its fp32 prefilter).  Bounds: the neighbour CSR is IDENTICAL to the oracle's
(start array, and the indices sorted per row); fp64 fields within 1e-10 of the field maximum (rel_err) and within the
element-wise 1e-8 of tests/test_baseline_sizes.py (bench.field_error); fp32 arithmetic within the 5e-5 of
test_hip_parity.test_fp32_arithmetic_vs_golden."""
import numpy as np
import pytest

from helpers import rel_err, WC_OUT
from test_hip_parity import make_eval, _copy_arrays, make_cube
from test_baseline_sizes import ELEMENTWISE_BOUND

pytestmark = pytest.mark.gpu

TOL = 1e-10
TOL_F32 = 5e-5
KERNELS = ['CubicSpline', 'WendlandQuintic', 'QuinticSpline', 'Gaussian']


def _kernel(name, dim=3):
    from pysph_amd import kernels as K
    return getattr(K, name)(dim=dim)


def sd_equations():
    from pysph_amd.equations import Group, SummationDensity
    return [Group(equations=[SummationDensity(dest='fluid', sources=['fluid'])])]


def wcsph_equations(dx, hdx=1.3, s=1.0, dim=3):
    """cube_equations with lengths scaled by s (h0 by s, gravity by 1/s) in `dim` dimensions"""
    from pysph_amd.scheme import WCSPHScheme
    from pysph_amd.examples import dam_break_3d as db
    g = {1: 'gx', 2: 'gy', 3: 'gz'}[dim]
    return WCSPHScheme(['fluid'], [], dim=dim, rho0=db.ro, c0=db.c0, h0=hdx * dx * s, hdx=hdx, alpha=db.alpha,
                       beta=db.beta, gamma=db.gamma, **{g: -9.81 / s}).get_equations()


def sorted_csr(start, idx):
    idx = np.array(idx, dtype=np.int64)
    for i in range(len(start) - 1):
        idx[start[i]:start[i + 1]].sort()
    return np.asarray(start, dtype=np.int64), idx


def oracle_run(oracle, arrays, eqs, kernel, dim, t=0.0, dt=1e-5):
    """(copies of `arrays` after the oracle's evaluation, its CSR of array 0 <- array 0)"""
    ref = _copy_arrays(arrays)
    onn = oracle.OracleNNPS(dim, ref, radius_scale=kernel.radius_scale)
    onn.update()
    oev = oracle.OracleEval(ref, eqs, kernel, nthreads=8)
    oev.set_nnps(onn)
    oev.compute(t, dt)
    return ref, sorted_csr(*onn.get_csr(0, 0, nthreads=8))


def device_run(arrays, eqs, kernel, dim, variant, f32=False, t=0.0, dt=1e-5):
    dev = _copy_arrays(arrays)
    a_eval, nnps, ctx = make_eval(dev, eqs, kernel, dim, variant)
    if f32:
        ctx.set_option('arith_f32', 1)
    a_eval.compute(t, dt)
    csr = sorted_csr(*nnps.get_csr(0, 0))
    ctx.close()
    return dev, csr


def assert_csr_equal(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, 'neighbour counts differ for %d destinations'
                                             % np.count_nonzero(np.diff(got[0]) != np.diff(want[0])))
    assert np.array_equal(got[1], want[1]), (what, 'neighbour indices differ')


def assert_fields(dev, ref, outs, what, f32=False):
    import bench
    worst = 0.0
    for pa, pr in zip(dev, ref):
        for f in outs:
            a, b = pa.properties[f], pr.properties[f]
            e = rel_err(a, b)
            worst = max(worst, e)
            if f32:
                assert e < TOL_F32, (what, f, e)
                continue
            assert e < TOL, (what, f, e)
            _, ew = bench.field_error(a, b, [pr.properties[g] for g in bench._scale_group(f) if g in pr.properties],
                                      elementwise=True)
            assert ew < ELEMENTWISE_BOUND, (what, f, 'element-wise', ew)
    if f32:
        assert worst > 1e-9, (what, 'the fp32 path did not run')
    return worst


def check_case(oracle, arrays, eqs, kernel, dim, outs, what, f32=False, ref=None):
    """variants 0 and 6 against the oracle; returns (oracle result, {variant: device arrays}, {variant: csr})"""
    if ref is None:
        ref = oracle_run(oracle, arrays, eqs, kernel, dim)
    devs, csrs = {}, {}
    for variant in (0, 6):
        dev, csr = device_run(arrays, eqs, kernel, dim, variant, f32=f32)
        assert_csr_equal(csr, ref[1], (what, variant))
        assert_fields(dev, ref[0], outs, (what, variant), f32=f32)
        devs[variant], csrs[variant] = dev, csr
    return ref, devs, csrs


# ---------------------------------------------------------------------------
# 1. power-of-two scaling
# ---------------------------------------------------------------------------
SCALES = [2.0 ** -7, 2.0 ** 3, 2.0 ** 10, 2.0 ** 40]
SCALES_F32 = SCALES[:2]          # m s^3 leaves the float range beyond


def scaled_cube(pa, s):
    q = _copy_arrays([pa])[0]
    for k in ('x', 'y', 'z', 'h'):
        q.properties[k] *= s
    q.properties['m'] *= s ** 3
    return q


@pytest.mark.parametrize('varh', [0.0, 0.2], ids=['uniform-h', 'variable-h'])
@pytest.mark.parametrize('kname', KERNELS)
def test_power_of_two_scaling(oracle, kname, varh):
    """A 10^3 jittered cube under the WCSPH set with x, y, z, h scaled by s, m by s^3, gravity by 1/s: every quantity
    of the evaluation is then the unscaled one times a power of two, and since a multiplication by a power of two is
    exact, every output field is the unscaled field times ONE power of two per field, bit for bit (2^-20 is left out:
    the reference's cell_size < 1e-6 -> 1.0 rule changes the cells there and with them the summation order).

    Asserted: the oracle IS covariant like that (the premise), the device's CSR is the same at every scale, the
    scaled run matches the scaled oracle, and the device's own fields are covariant bit for bit, in fp64 for both
    variants and in fp32 arithmetic (variant 6, s = 2^-7 and 2^3)."""
    kernel = _kernel(kname)
    pa, dx = make_cube(10, varh=varh)
    base_ref, base_dev, base_csr = check_case(oracle, [pa], wcsph_equations(dx), kernel, 3, WC_OUT, (kname, varh, 1.0))
    base_f32 = device_run([pa], wcsph_equations(dx), kernel, 3, 6, f32=True)[0]     # arith_f32 is variant 6 only
    not_covariant = []
    for s in SCALES:
        eqs = wcsph_equations(dx, s=s)
        ps = scaled_cube(pa, s)
        ref = oracle_run(oracle, [ps], eqs, kernel, 3)
        assert_csr_equal(ref[1], base_ref[1], (kname, varh, s, 'oracle'))
        factor = {}
        for f in WC_OUT:
            a, b = ref[0][0].properties[f], base_ref[0][0].properties[f]
            nz = b != 0
            factor[f] = (a[nz] / b[nz])[0] if nz.any() else 1.0
            assert np.log2(factor[f]) == np.round(np.log2(factor[f])), (f, factor[f])
            assert np.array_equal(a, b * factor[f]), ('the oracle is not covariant', kname, varh, s, f)
        _, devs, csrs = check_case(oracle, [ps], eqs, kernel, 3, WC_OUT, (kname, varh, s), ref=ref)
        runs = [('f64', v, devs[v], base_dev[v]) for v in (0, 6)]
        if s in SCALES_F32:
            d32, c32 = device_run([ps], eqs, kernel, 3, 6, f32=True)
            assert_csr_equal(c32, base_ref[1], (kname, varh, s, 'f32'))
            assert_fields(d32, ref[0], WC_OUT, (kname, varh, s, 'f32'), f32=True)
            runs.append(('f32', 6, d32, base_f32))
        for v in (0, 6):
            assert_csr_equal(csrs[v], base_csr[v], (kname, varh, s, v, 'device across scales'))
        for prec, v, d, b in runs:
            for f in WC_OUT:
                if not np.array_equal(d[0].properties[f], b[0].properties[f] * factor[f]):
                    not_covariant.append((prec, v, s, f, rel_err(d[0].properties[f], b[0].properties[f] * factor[f])))
    assert not not_covariant, not_covariant


# ---------------------------------------------------------------------------
# 2. translation
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('shift', [(1e3, -1e5, 1e6), (-1e6, -1e6, -1e6)], ids=['mixed', 'minus-1e6'])
@pytest.mark.parametrize('kname,varh', [('WendlandQuintic', 0.0), ('WendlandQuintic', 0.2), ('Gaussian', 0.0),
                                        ('QuinticSpline', 0.2)])
def test_translated_cube(oracle, kname, varh, shift):
    """the same cube far from the origin: positions carry ~1e-10 of rounding, 1e-9 h -- the same doubles go to the
    oracle, and both take differences of them"""
    pa, dx = make_cube(10, varh=varh)
    for k, d in zip('xyz', shift):
        pa.properties[k] += d
    check_case(oracle, [pa], wcsph_equations(dx), _kernel(kname), 3, WC_OUT, (kname, varh, shift))


# ---------------------------------------------------------------------------
# 3. long sparse domains
# ---------------------------------------------------------------------------
def _wcsph_array(x, y, z, h, dx, dim, rng):
    from pysph_amd.particle_array import get_particle_array_wcsph
    from pysph_amd.examples import dam_break_3d as db
    n = x.size
    vel = {k: 0.1 * db.c0 * rng.uniform(-1, 1, n) * (i < dim) for i, k in enumerate('uvw')}
    return get_particle_array_wcsph(name='fluid', x=x, y=y, z=z, h=h * np.ones(n), m=db.ro * dx ** dim * np.ones(n),
                                    rho=db.ro * (1 + 0.01 * rng.uniform(-1, 1, n)), **vel)


def line_clusters():
    """1-D: 2000 particles in 20 clusters of 100 over L / h = 10^6"""
    rng = np.random.default_rng(31)
    dx = 1e-3
    h = 1.3 * dx
    x = np.concatenate([k * (1e6 * h / 19) + (np.arange(100) + 0.1 * rng.uniform(-1, 1, 100)) * dx for k in range(20)])
    z = np.zeros_like(x)
    return _wcsph_array(x, z, z.copy(), h, dx, 1, rng), dx


def strip_clusters():
    """2-D: 3000 particles in 30 clusters of 10 x 10 in a strip 4 cells wide and 10^4 cells long"""
    rng = np.random.default_rng(32)
    dx = 1e-2
    h = 1.3 * dx
    cell = 2 * h
    gx, gy = [a.ravel() for a in np.meshgrid(np.arange(10), np.arange(10), indexing='ij')]
    xs, ys = [], []
    for k in range(30):
        xs.append(k * (1e4 * cell / 29) + (gx + 0.1 * rng.uniform(-1, 1, 100)) * dx)
        ys.append((gy + 0.1 * rng.uniform(-1, 1, 100)) * dx * (3.9 * cell / (9.2 * dx)))
    x, y = np.concatenate(xs), np.concatenate(ys)
    return _wcsph_array(x, y, np.zeros_like(x), h, dx, 2, rng), dx


@pytest.mark.parametrize('eqset', ['density', 'wcsph'])
@pytest.mark.parametrize('dim', [1, 2])
def test_long_sparse_domain(oracle, dim, eqset):
    """here the prefilter's slack (1.5e-6 of the extent) exceeds h: everything rests on the exact criterion"""
    pa, dx = line_clusters() if dim == 1 else strip_clusters()
    kernel = _kernel('CubicSpline' if dim == 1 else 'WendlandQuintic', dim)     # no 1-D WendlandQuintic
    eqs, outs = (sd_equations(), ['rho']) if eqset == 'density' else (wcsph_equations(dx, dim=dim), WC_OUT)
    ref, devs, csrs = check_case(oracle, [pa], eqs, kernel, dim, outs, (dim, eqset))
    extent = pa.x.max() - pa.x.min()
    assert np.diff(ref[1][0]).min() > 1          # sparse, yet everybody has neighbours
    if dim == 1:
        assert 1.5e-6 * extent > pa.h[0]


# ---------------------------------------------------------------------------
# 4. clusters outside fixed bounds
# ---------------------------------------------------------------------------
EXTENTS_OUT = [(15, (1, 0, 0)), (50, (0, -1, 0)), (100, (0, 0, 1)), (1000, (1, 1, 1))]


def cube_with_far_clusters():
    """a 12^3 cube inside bounds (-0.2 .. 1.2)^3 and, 15 / 50 / 100 / 1000 grid extents outside them along +x, -y, +z
    and the diagonal, four clusters of 64 anchors (a 4^3 lattice of spacing 3 h: no anchor is another's neighbour),
    each with one partner at r = 2 h (1 - U(0, 1e-4)) and one at 2 h (1 + U(0, 1e-4)) in a random direction"""
    pa, dx = make_cube(12)
    rng = np.random.default_rng(44)
    h = pa.h[0]
    n0 = pa.get_number_of_particles()
    extent = 1.4
    pos, kind = [], []
    gx = np.array(np.meshgrid(*[np.arange(4)] * 3, indexing='ij')).reshape(3, -1).T * 3 * h
    for k, d in EXTENTS_OUT:
        origin = np.where(np.array(d) > 0, 1.2, -0.2) * np.abs(d) + np.array(d) * k * extent + 0.1 * (1 - np.abs(d))
        anchors = origin + gx
        u = rng.normal(size=(64, 3))
        u /= np.linalg.norm(u, axis=1)[:, None]
        r_in = 2 * h * (1 - rng.uniform(0, 1e-4, 64))
        r_out = 2 * h * (1 + rng.uniform(0, 1e-4, 64))
        pos += [anchors, anchors + u * r_in[:, None], anchors + u * r_out[:, None]]
        kind += [np.zeros(64, int), np.ones(64, int), 2 * np.ones(64, int)]
    pos, kind = np.concatenate(pos), np.concatenate(kind)
    return pa, dx, pos, kind, n0


@pytest.mark.parametrize('variant', [0, 6])
def test_clusters_outside_fixed_bounds(oracle, variant):
    """HipNNPS(fixed_h=True) with fixed bounds: particles outside the grid are clamped into its outermost cells and
    found by the distance criterion (sph_nnps.hip).  The oracle's brute-force search -- no grid at all -- decides
    who is a neighbour; the device's lists must be identical, for the cube and for every cluster."""
    from pysph_amd import device as dev
    from pysph_amd.acceleration_eval import AccelerationEval, SPHCompiler
    from pysph_amd.nnps import HipNNPS
    from pysph_amd.particle_array import get_particle_array_wcsph
    cube, dx, pos, kind, n0 = cube_with_far_clusters()
    n = n0 + len(pos)
    props = {k: np.concatenate([cube.properties[k], np.full(len(pos), cube.properties[k][0])])
             for k in ('h', 'm', 'rho')}
    inside = np.concatenate([[cube.x, cube.y, cube.z], np.full((3, len(pos)), 0.5)], axis=1)
    pa = get_particle_array_wcsph(name='fluid', x=inside[0].copy(), y=inside[1].copy(), z=inside[2].copy(), **props)
    kernel = _kernel('WendlandQuintic')
    ctx = dev.HipContext(0)
    ctx.set_option('pair_variant', variant)
    a_eval = AccelerationEval([pa], sd_equations(), kernel)
    SPHCompiler(a_eval, ctx=ctx).compile()
    nnps = HipNNPS(3, [pa], radius_scale=2.0, ctx=ctx, fixed_h=True)     # first update: everybody inside
    a_eval.set_nnps(nnps)
    nnps.bounds = (-0.2, -0.2, -0.2, 1.2, 1.2, 1.2)
    for k, c in enumerate('xyz'):
        pa.properties[c][n0:] = pos[:, k]
    nnps.update()
    assert np.all(nnps.xmin > -1) and np.all(nnps.xmax < 2)        # the grid is the bounds', the clusters are outside
    a_eval.compute(0.0, 1e-5)
    start, idx = sorted_csr(*nnps.get_csr(0, 0))
    ctx.close()
    # the oracle: brute force over all particles
    ref = _copy_arrays([pa])
    onn = oracle.OracleNNPS(3, ref, radius_scale=2.0)
    want = [np.sort(onn.brute_force_neighbors(0, 0, i)) for i in range(n)]
    # the condition that keeps the test from being vacuous: the margins (2e-6) are far above a position ulp (2e-13)
    anchors = n0 + np.flatnonzero(kind == 0)
    for c in range(4):
        a = anchors[64 * c:64 * (c + 1)]
        has_in = np.mean([a[i] + 64 in want[a[i]] for i in range(64)])
        has_out = np.mean([a[i] + 128 in want[a[i]] for i in range(64)])
        assert has_in >= 0.95 and has_out <= 0.05, (EXTENTS_OUT[c], has_in, has_out)
    missing = np.zeros(5, int)
    extra = np.zeros(5, int)
    where = np.concatenate([np.zeros(n0, int), 1 + np.repeat(np.arange(4), 192)])
    for i in range(n):
        got = idx[start[i]:start[i + 1]]
        missing[where[i]] += len(np.setdiff1d(want[i], got))
        extra[where[i]] += len(np.setdiff1d(got, want[i]))
    print('variant %d: neighbours missing (cube, 15, 50, 100, 1000 extents out) %s, extra %s' % (variant, missing, extra))
    assert not missing.any() and not extra.any(), (missing, extra)
    # ... and the density the pair kernel sums over them
    hh = pa.h[0]
    sigma = 21.0 / (16 * np.pi) / hh ** 3
    P = np.array([pa.x, pa.y, pa.z]).T
    rho = np.empty(n)
    for i in range(n):
        q = np.sqrt(((P[want[i]] - P[i]) ** 2).sum(axis=1)) / hh
        rho[i] = np.sum(pa.m[want[i]] * sigma * (1 - 0.5 * q) ** 4 * (2 * q + 1) * (q < 2))
    assert rel_err(pa.rho, rho) < TOL


# ---------------------------------------------------------------------------
# 5. pairs exactly on the cutoff
# ---------------------------------------------------------------------------
def cutoff_pairs(radius, mode):
    """Pairs at r = radius * h exactly and one step of the partner's x to either side: axis-aligned, face-diagonal
    and 3-4-5 separations, h = 0.5 and 0.25; anchors on a lattice of spacing 8 that starts at 0 (for anchors with
    x = 0 the step is one ulp of the separation itself).  mode 'h0.5' / 'h0.25': every particle has that h;
    'variable': anchor and partner differ (0.5 / 0.25 both ways) -- the rule r2 < hi^2 OR r2 < hj^2 -- and the
    fillers carry either.  200 filler particles fill the wave tiles."""
    rng = np.random.default_rng(55)
    if mode == 'variable':
        hs = [(0.5, 0.25), (0.25, 0.5)]
    else:
        hs = [(float(mode[1:]),) * 2]
    seps = []
    for hi, hj in hs:
        R = radius * max(hi, hj)
        a = R / np.sqrt(2.0)
        for v in ((R, 0, 0), (0, R, 0), (0, 0, -R), (a, a, 0), (a, 0, -a), (0.6 * R, 0.8 * R, 0), (0.8 * R, 0, 0.6 * R),
                  (-R, 0, 0), (-a, 0, a)):
            for step in (0, -1, 1):
                seps.append((np.array(v, dtype=float), step, hi, hj))
    lattice = np.array(np.meshgrid(*[np.arange(4)] * 3, indexing='ij')).reshape(3, -1).T * 8.0
    assert len(seps) <= len(lattice)
    pos, h = [], []
    for (v, step, hi, hj), anchor in zip(seps, lattice):
        p = anchor + v
        if step:
            k = 0 if v[0] != 0 else (1 if v[1] != 0 else 2)
            p[k] = np.nextafter(p[k], p[k] + step * 10.0)
        pos += [anchor, p]
        h += [hi, hj]
    nf = 200
    pos = np.concatenate([np.array(pos), rng.uniform(-1, 25, (nf, 3))])
    hf = rng.choice([0.5, 0.25], nf) if mode == 'variable' else np.full(nf, hs[0][0])
    h = np.concatenate([h, hf])
    from pysph_amd.particle_array import get_particle_array_wcsph
    n = len(h)
    return get_particle_array_wcsph(name='fluid', x=pos[:, 0].copy(), y=pos[:, 1].copy(), z=pos[:, 2].copy(), h=h,
                                    m=1.0 + rng.uniform(0, 1, n), rho=np.ones(n)), 2 * len(seps)


@pytest.mark.parametrize('mode', ['h0.5', 'h0.25', 'variable'])
@pytest.mark.parametrize('kname', KERNELS)
def test_pairs_on_the_cutoff(oracle, kname, mode):
    """r2 == (radius h)^2 is NOT a neighbour (the criterion is <), one ulp less is; the CSR must be the oracle's, and
    the summed density too -- the Gaussian is cut off where it is still 1.2e-4 of its peak, so a tie pair that is in
    on one side and out on the other shows in rho."""
    kernel = _kernel(kname)
    pa, npair = cutoff_pairs(kernel.radius_scale, mode)
    ref, devs, csrs = check_case(oracle, [pa], sd_equations(), kernel, 3, ['rho'], (kname, mode))
    # the cases do straddle: of the paired particles some have their partner as a neighbour and some do not
    start, idx = ref[1]
    has = np.array([(i ^ 1) in idx[start[i]:start[i + 1]] for i in range(npair)])
    assert 0.2 < has.mean() < 0.8, has.mean()


# ---------------------------------------------------------------------------
# 6. lattice on cell faces
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('kname', ['QuinticSpline', 'Gaussian'])
def test_lattice_on_cell_faces(oracle, kname):
    """an unjittered lattice with dx = 1/8 and h = dx: positions are exact multiples of dx, separations of 3 dx --
    exactly the support radius of both kernels -- abound"""
    pa, dx = make_cube(8, hdx=1.0, jitter=0.0)
    assert dx == 0.125 and np.all(pa.h == dx) and np.all(pa.x * 8 == np.round(pa.x * 8))
    kernel = _kernel(kname)
    ref, _, _ = check_case(oracle, [pa], wcsph_equations(dx, hdx=1.0), kernel, 3, WC_OUT, kname)
    # ties exist and are excluded: an interior particle has the 3 dx neighbours along the axes at r2 == (3 h)^2
    P = np.array([pa.x, pa.y, pa.z]).T
    i = int(np.argmin(((P - 0.5) ** 2).sum(axis=1)))
    start, idx = ref[1]
    r2 = ((P[idx[start[i]:start[i + 1]]] - P[i]) ** 2).sum(axis=1)
    assert r2.max() < (3 * dx) ** 2 and np.any(((P - P[i]) ** 2).sum(axis=1) == (3 * dx) ** 2)
