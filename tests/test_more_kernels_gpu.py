"""The smoothing kernels 5..10 (WendlandQuinticC2_1D, WendlandQuinticC4, WendlandQuinticC4_1D, WendlandQuinticC6,
WendlandQuinticC6_1D, SuperGaussian) on the device: one value per thread through
tests/probes/device_functions_more.hip, lattice moments through the pair loop, every hand-written family against
golden vectors of the reference's own Python classes (tests/golden/make_more_kernels_golden.py), the generated path,
the interpolator, and the C-ABI's answer to a kernel it does not have.

Error budgets of the device functions, by the counting rule of tests/test_device_functions.py:
|device - reference| <= C u S, u the unit roundoff of the type, S the absolute value of the term as the device writes
it, C the roundings the term goes through.  A rounding in a factor that appears n times counts n times; a
multiplication by a power of two counts nothing; a coefficient that is no fp number (35/12, 14/3) counts one.
Where a power of t underflows (fp32, within a few ulp of the support radius) the budget gets the absolute term
C fmin |factor| (see _budgets).

All five Wendlands are one product t^n P(q) (w), c q D(q) t^(n-1) (dw), c D(q) t^(n-1) (dwq), t = 1 - 0.5 q, with P and
D in Horner form (sph_kernels.h).
  * t^n: t carries one rounding and appears n times: n; the n - 1 multiplications that form the power, by squaring
    or one by one, count n - 1 (t2 = t t appears n/2 times with one rounding each, and so on): 2 n - 1.
  * a Horner polynomial of degree k with positive coefficients and q >= 0: every partial result is below the value,
    so each of its 2 k operations (minus the multiplications by 2 or 4) counts one.
  * the multiplications that join the factors count one each.

  C2_1D  w   t t t (1.5 q + 1)                       t^3: 5, P: 2,      join 1            =  8
         dw  -3 q t t                                t^2: 3,            -3 q, (.) t t: 2  =  5
         dwq -3 t t                                  t^2: 3,            join 1            =  4
  C4     w   t^6 ((35/12 q + 3) q + 1)               t^6: 11, P: 4 + 1 (35/12), join 1    = 17
         dw  -14/3 q (1 + 2.5 q) t^5                 t^5: 9, D: 2, 14/3: 1, join 3        = 15
         dwq -14/3 (1 + 2.5 q) t^5                   as dw without the multiplication by q = 14
  C4_1D  w   t^5 ((2 q + 2.5) q + 1)                 t^5: 9, P: 3 (2 q exact), join 1     = 13
         dw  -3.5 q (2 q + 1) t^4                    t^4: 7, D: 1, join 3                 = 11
         dwq -3.5 (2 q + 1) t^4                                                           = 10
  C6     w   t^8 (((4 q + 6.25) q + 4) q + 1)        t^8: 15, P: 5 (4 q exact), join 1    = 21
         dw  -5.5 q t^7 ((4 q + 3.5) q + 1)          t^7: 13, D: 3, join 3                = 19
         dwq -5.5 t^7 ((4 q + 3.5) q + 1)                                                 = 18
  C6_1D  w   t^7 (((2.625 q + 4.75) q + 3.5) q + 1)  t^7: 13, P: 6, join 1                = 20
         dw  -0.5 q ((26.25 q + 27) q + 9) t^6       t^6: 11, D: 4, join 2 (-0.5 q exact) = 17
         dwq -0.5 ((26.25 q + 27) q + 9) t^6         -0.5 (.) exact: join 1               = 16

SuperGaussian: the Gaussian's exp-plus-polynomial form.  exp(-q2) with q2 = q q: 4 ulp of exp, and the rounding of
its argument moves it by q^2 u relative.  The polynomial factors are differences, so they are judged by the sum S of
the absolute values of their terms, not by their value (w changes sign at q^2 = 1 + dim/2):
  w   exp(-q2) (1 + 0.5 dim - q2)      S = 1 + dim/2 + q^2;      q2, the subtraction, the product: 3
  dw  q (2 q2 - (dim + 4)) exp(-q2)    S = q (2 q^2 + dim + 4);  q2, the subtraction, two products: 4
  dwq (2 q2 - (dim + 4)) exp(-q2)      S = 2 q^2 + dim + 4;      3
  |device - reference| <= 4 ulp(exp) S + (q^2 + C) u exp(-q^2) S

Worst C seen on an MI355X (fp64 / fp32), w, dw, dwq: C2_1D 3.56 / 5.71, 3.17 / 3.42, 2.80 / 3.04; C4 8.45 / 10.13,
6.94 / 8.34, 6.62 / 8.56; C4_1D 5.64 / 6.70, 5.09 / 6.04, 4.78 / 5.23; C6 9.37 / 11.75, 8.58 / 10.05, 8.29 / 10.55;
C6_1D 8.77 / 11.67, 8.12 / 9.50, 9.02 / 9.38 -- about half of each count, as for the first four kernels.  The
SuperGaussian uses 0.38 of its budget at the most; pair_w / pair_gradfac / pair_gradh at the most 0.48 of theirs.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden, arrays_from_golden
import helpers as H
from helpers import rel_err
import more_kernels as MK
import test_kernel_moments as KM
import test_more_kernels as TM

DPS = 50
U = {np.float64: 2.0 ** -53, np.float32: 2.0 ** -24}
DTYPES = [np.float64, np.float32]
TOL = 1e-10            # BASELINE.json north_star, as tests/test_hip_parity.py
TOL_F32 = 5e-5         # test_fp32_arithmetic_vs_golden


def _mp():
    import mpmath as mp
    mp.mp.dps = DPS
    return mp


def _abs_err(dev, ref):
    mp = _mp()
    return np.array([float(abs(mp.mpf(float(d)) - r)) for d, r in zip(dev, ref)])


def _bits(a):
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def _spacing(x, dtype):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(dtype)).astype(np.float64)


def edge_q(kk, dim, dtype):
    """q = 0, the support radius with its neighbours on both sides, the SuperGaussian's sign change q^2 = 1 + dim/2 with
    its neighbours, 2048 log-spaced q in [2^-60, support], 2048 uniform q, and a few beyond the support"""
    sup = MK.SUPPORT[kk]
    rng = np.random.default_rng(200 + 10 * kk + dim)
    knots = [sup] + ([np.sqrt(1 + 0.5 * dim)] if kk == 10 else [])
    pts = [0.0]
    for k in knots:
        k = dtype(k)
        pts += [np.nextafter(k, dtype(0)), k, np.nextafter(k, dtype(10))]
    return np.concatenate([np.array(pts, dtype=dtype),
                           (2.0 ** np.linspace(-60, np.log2(sup), 2048)).astype(dtype),
                           rng.uniform(0, sup, 2048).astype(dtype),
                           np.array([sup * 1.0001, sup * 1.5, 10.0, 1e6, 1e30], dtype=dtype)])


def _budgets(kk, dim, q, rw, dtype):
    """(bound_w, bound_dw, bound_dwq, S_w, S_dw, S_dwq) at the arguments q (float64 array); rw: the reference's w as
    mpf, used for exp(-q^2) of the SuperGaussian"""
    u = U[dtype]
    sw, sd, sq = MK.term_sums(kk, q, dim)
    if kk != 10:
        # underflow: next to the support radius t^n falls below the smallest normal number of the type (fp32: t^6 at
        # t = 2^-24 is 2^-144), where the format has no relative precision -- a partial product there is rounded
        # absolutely (gradual underflow) or flushed, by less than fmin, and then multiplied by at most the rest of
        # the product, which the polynomial factor bounds (t <= 1): C fmin factor on top of C u S
        fmin = float(np.finfo(dtype).tiny)
        spec = MK.WENDLAND[kk]
        c = abs(spec['c'])
        fw, fd, fq = MK._poly(spec['P'], q), c * q * MK._poly(spec['D'], q), c * MK._poly(spec['D'], q)
        return (MK.C_W[kk] * (u * sw + fmin * fw * (sw > 0)), MK.C_DW[kk] * (u * sd + fmin * fd * (sd > 0)),
                MK.C_DWQ[kk] * (u * sq + fmin * fq * (sq > 0)), sw, sd, sq)
    e = np.where(q < 3, np.exp(-q * q), 0.0)
    ulp_e = _spacing(e, dtype) * (q < 3)
    return (4 * ulp_e * sw + (q * q + 3) * u * e * sw, 4 * ulp_e * sd + (q * q + 4) * u * e * sd,
            4 * ulp_e * sq + (q * q + 3) * u * e * sq, e * sw, e * sd, e * sq)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES, ids=['f64', 'f32'])
@pytest.mark.parametrize('kk,dim', MK.KIND_DIMS)
def test_kernel_functions_within_rounding_budget(kk, dim, dtype):
    """SphKernel<kk>::w / dw / dwq, INSUP both ways, against the reference's formulas at 50 digits, within the budgets
    of the module docstring; exactly 0 from the support radius on; INSUP changes no bit inside."""
    mp = _mp()
    q = edge_q(kk, dim, dtype)
    q64 = q.astype(np.float64)
    ref = [MK.mp_kernel(kk, mp.mpf(float(x)), dim) for x in q]
    rw, rdw = [a for a, b in ref], [b for a, b in ref]
    sup = MK.SUPPORT[kk]
    w, dw, dwq = MK.probe_kernel(kk, False, q, dim)
    wi, dwi, dwqi = MK.probe_kernel(kk, True, q, dim)
    for a in (w, dw, dwq):
        assert np.all(np.isfinite(a))
    for a in (wi, dwi, dwqi):
        assert np.all(np.isfinite(a[q <= sup]))
    bw, bdw, bdwq, sw, sd, sq = _budgets(kk, dim, q64, rw, dtype)
    # dw / q: the reference's dw over q; at q = 0 the limit c D(0) (Wendlands), -(dim + 4) (SuperGaussian)
    lim = mp.mpf(MK.WENDLAND[kk]['c'] * MK.WENDLAND[kk]['D'][0]) if kk != 10 else mp.mpf(-(dim + 4))
    rdwq = [b / mp.mpf(float(x)) if x > 0 else lim for b, x in zip(rdw, q)]
    worst = {}
    for name, dev, r, bound, s in (('w', w, rw, bw, sw), ('dw', dw, rdw, bdw, sd), ('dwq', dwq, rdwq, bdwq, sq)):
        err = _abs_err(dev, r)
        live = bound > 0
        assert live.sum() > 4000
        worst[name] = float(np.max(err[live] / bound[live]))
        assert np.all(err[~live] == 0), name
        assert np.all(err <= bound), (name, worst[name], q[np.argmax(np.where(live, err / np.where(live, bound, 1), 0))])
    cs = {'w': MK.C_W, 'dw': MK.C_DW, 'dwq': MK.C_DWQ}
    print('%s dim %d %s: worst %s' % (MK.NAMES[kk], dim, dtype.__name__, ', '.join(
        '%s %.2f' % (k, v * cs[k][kk]) if kk != 10 else '%s %.2f of the budget' % (k, v) for k, v in sorted(worst.items()))))
    # exactly 0 at and beyond the support radius (the Wendlands: t is an exact zero at q == 2; INSUP has no test, so
    # at q == 2 it returns the zero of the product, sign included, and the tested path returns the same bits)
    out = q >= sup
    assert out.sum() >= 6
    for a in (w, dw, dwq):
        assert np.all(a[out] == 0)
    at = q == sup
    if kk != 10:
        for a, b in ((w, wi), (dw, dwi), (dwq, dwqi)):
            assert np.all(b[at] == 0) and np.array_equal(_bits(a[at]), _bits(b[at]))
    else:       # cut off where it is not zero: the support test stays whatever the caller guarantees
        for b in (wi, dwi, dwqi):
            assert np.all(b[out] == 0)
        assert np.all(w[(q64 * q64 > 1 + 0.5 * dim + 1e-3) & (q < 3)] < 0) and np.all(w[q64 * q64 < 1 + 0.5 * dim - 1e-3] > 0)
    ins = q <= sup
    for a, b in ((w, wi), (dw, dwi), (dwq, dwqi)):
        assert np.array_equal(_bits(a[ins]), _bits(b[ins]))


H_VALUES = {np.float64: [2.0 ** -30, 1.1 * 2.0 ** -3, 1.3, 2.0 ** 40], np.float32: [2.0 ** -10, 0.013, 1.3, 2.0 ** 10]}
FAST_REL = {np.float64: 1e-14, np.float32: 2 * 2.0 ** -23}      # sph_pair.h, as tests/test_device_functions.py


def _pair_inputs(kk, dim, dtype, hij):
    sup = MK.SUPPORT[kk]
    tiny = np.finfo(dtype).smallest_subnormal
    g2 = dtype(1e-12) * dtype(1e-12)
    edge = [0.0, tiny, 1000 * tiny, np.nextafter(g2, dtype(0)), g2, np.nextafter(g2, dtype(1)), 4 * g2]
    knots = (sup,) + ((np.sqrt(1 + 0.5 * dim),) if kk == 10 else ())
    qs = np.concatenate([2.0 ** np.linspace(-20, np.log2(sup), 192), np.array(knots + (1.01 * sup, 2 * sup)),
                         np.array(knots) * (1 - 1e-6)])
    r = (qs * float(hij)).astype(dtype)
    return np.concatenate([np.array(edge, dtype=dtype), r * r])


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES, ids=['f64', 'f32'])
@pytest.mark.parametrize('kk,dim', MK.KIND_DIMS)
def test_pair_geometry_and_gradient_factors(kk, dim, dtype):
    """pair_geom / pair_w / pair_gradfac / pair_gradh for the new ids, UH both ways, as
    test_device_functions.test_pair_geometry_and_gradient_factors: the geometry against numpy in the same type (bit
    for bit on the SuperGaussian's exact-q path, within the fast paths' documented accuracy otherwise), the kernel
    functions against mpmath AT the device's own geometry: the kernel's budget, u S per further multiplication, and
    u q times the function's slope (more_kernels.slope_sums) for the rounding of q = rij h1 itself."""
    mp = _mp()
    u, fast, sup = U[dtype], FAST_REL[dtype], MK.SUPPORT[kk]
    exact_q = kk == 10
    guard = dtype(1e-12)
    clamp = dtype(1e-300) if dtype is np.float64 else dtype(1e-35)
    tiny = float(np.finfo(dtype).smallest_subnormal)
    sigma = 0.3183098861837907
    worst = {'w': 0.0, 'gradfac': 0.0, 'gradh': 0.0}
    n_guarded = 0
    for h in H_VALUES[dtype]:
        for uh in (False, True):
            h = dtype(h)
            hi, hj = (h, h) if uh else (dtype(h * 1.1), dtype(h * 0.9))
            hij = dtype(0.5) * (hi + hj)
            r2 = _pair_inputs(kk, dim, dtype, hij)
            if uh:
                r2 = r2[r2 < (dtype(sup) * hij) ** 2]
            one = dtype(1)
            h1u = one / hij
            facu = dtype(sigma) * h1u
            for _ in range(dim - 1):
                facu = facu * h1u
            epsu = dtype(0.01) * hij * hij
            o = MK.probe_pair(kk, uh, r2, np.full(r2.size, hi), np.full(r2.size, hj), sigma, dim,
                              uniform=(hij, h1u, facu, epsu))
            ctx = (kk, dtype.__name__, dim, float(h), uh)
            for k, a in o.items():
                assert np.all(np.isfinite(a)), (k,) + ctx
            assert np.array_equal(o['hij'], np.full(r2.size, hij)), ctx
            assert np.array_equal(o['eps'], np.full(r2.size, epsu)), ctx
            assert np.array_equal(_bits(o['q']), _bits(o['rij'] * o['h1'])), ctx
            if uh or exact_q:
                assert np.array_equal(o['h1'], np.full(r2.size, h1u)), ctx
                assert np.array_equal(o['fac'], np.full(r2.size, facu)), ctx
            else:
                assert np.all(np.abs(o['h1'].astype(np.float64) * float(hij) - 1) <= fast), ctx
            if exact_q:
                rij = np.sqrt(r2)
                with np.errstate(divide='ignore'):
                    rinv = np.where(rij > 0, one / rij, dtype(0)).astype(dtype)
                assert np.array_equal(_bits(o['rij']), _bits(rij)), ctx
                assert np.array_equal(_bits(o['rinv']), _bits(rinv)), ctx
            else:
                rc = [mp.sqrt(mp.mpf(float(max(v, clamp)))) for v in r2]
                e1 = _abs_err(o['rij'], rc) / np.array([float(v) for v in rc])
                assert e1.max() <= fast, ctx + (e1.max(),)
            q, fac, h1d, rij = (o[k].astype(np.float64) for k in ('q', 'fac', 'h1', 'rij'))
            ref = [MK.mp_kernel(kk, mp.mpf(v), dim) for v in q]
            rw, rdw = [a for a, b in ref], [b for a, b in ref]
            if uh and not exact_q:
                assert np.all(q <= sup), ctx
            bw, bdw, bdwq, sw, sdw, sdwq = _budgets(kk, dim, q, rw, dtype)
            dq = u * q
            lw, ldw, ldwq = (np.maximum.reduce(c) for c in zip(*[MK.slope_sums(kk, np.maximum(q + sg * dq, 0), dim)
                                                                 for sg in (-1, 0, 1)]))
            bw, bdw, bdwq = bw + dq * lw, bdw + dq * ldw, bdwq + dq * ldwq
            # pair_w = w(q) fac
            err = _abs_err(o['w'], [a * mp.mpf(f) for a, f in zip(rw, fac)])
            bound = (bw + u * sw) * fac + tiny
            assert np.all(err <= bound), ('pair_w',) + ctx + (np.max(err / bound),)
            worst['w'] = max(worst['w'], np.max(err / bound))
            # pair_gradfac = dwq(q) (fac h1 h1), 0 for rij <= 1e-12
            live = o['rij'] > guard
            n_guarded += int(np.count_nonzero(~live))
            assert np.all(o['gradfac'][~live] == 0), ctx
            gref = [b / mp.mpf(qq) * mp.mpf(f) * mp.mpf(a) ** 2 if lv else mp.mpf(0)
                    for b, qq, f, a, lv in zip(rdw, q, fac, h1d, live)]
            err = _abs_err(o['gradfac'], gref)
            bound = (bdwq + 3 * u * sdwq) * fac * h1d * h1d + tiny
            assert np.all(err[live] <= bound[live]), ('pair_gradfac',) + ctx + (np.max(err[live] / bound[live]),)
            worst['gradfac'] = max(worst['gradfac'], np.max(err[live] / bound[live]))
            # pair_gradh = -+ fac h1 (dw q + w dim); the SuperGaussian's carries the reference's own sign (:1027-1047)
            sign = 1 if kk == 10 else -1
            href = [sign * mp.mpf(f) * mp.mpf(a) * (b * mp.mpf(qq) + w_ * dim) for f, a, b, qq, w_ in zip(fac, h1d, rdw, q, rw)]
            err = _abs_err(o['gradh'], href)
            sh = sdw * q + sw * dim
            bound = (bdw * q + bw * dim + 4 * u * sh) * fac * h1d + tiny
            assert np.all(err <= bound), ('pair_gradh',) + ctx + (np.max(err / bound),)
            worst['gradh'] = max(worst['gradh'], np.max(err / bound))
    assert n_guarded >= len(H_VALUES[dtype]) * 2 * 4
    print('%s dim %d %s: worst fraction of the budget %s' % (MK.NAMES[kk], dim, dtype.__name__,
                                                            ', '.join('%s %.2f' % kv for kv in sorted(worst.items()))))


@pytest.mark.gpu
def test_supergaussian_gradh_sign_is_the_references():
    """the reference's SuperGaussian.gradient_h against the device's pair_gradh at the fixture's samples: the stored
    values (of opposite sign to -fac h1 (dw q + w dim)) within 1e-10 of the largest"""
    g = load_golden('kernels_more.npz')
    for dim in (1, 2, 3):
        key = 'SuperGaussian/%d/' % dim
        h, r, sigma = g[key + 'h'], g[key + 'r'], float(g[key + 'fac'])
        o = MK.probe_pair(10, False, r * r, h, h, sigma, dim)
        assert np.count_nonzero(g[key + 'gradh']) > 16
        assert rel_err(o['gradh'], g[key + 'gradh']) < TOL, dim


# ---------------------------------------------------------------------------
# lattice moments through the pair loop
# ---------------------------------------------------------------------------
def _evaluator(arrays, eqs, kernel, dim, variant=6, sync='auto'):
    from pysph_amd import device as dev
    from pysph_amd.acceleration_eval import AccelerationEval, SPHCompiler
    from pysph_amd.nnps import HipNNPS
    ctx = dev.HipContext(0)
    ctx.set_option('pair_variant', variant)
    a_eval = AccelerationEval(arrays, eqs, kernel)
    SPHCompiler(a_eval, ctx=ctx, sync=sync).compile()
    nnps = HipNNPS(dim, arrays, radius_scale=kernel.radius_scale, ctx=ctx)
    a_eval.set_nnps(nnps)
    return a_eval, nnps, ctx


@pytest.mark.gpu
@pytest.mark.parametrize('name,dim', sorted(TM.PLACES))
def test_lattice_moments_device_pair_loop(name, dim):
    """the GPU half of tests/test_kernel_moments.py for the new 2-D / 3-D kernels: a probe particle in a unit lattice,
    a generated equation sums WIJ and DWIJ; places as pysph/base/tests/test_kernel.py asks (test_more_kernels.PLACES)"""
    from pysph_amd import kernels as K
    kernel = getattr(K, name)(dim=dim)
    p0, p1, p2 = TM.PLACES[(name, dim)]
    probe, lat = KM.moment_arrays(dim)
    got = {}
    for lmn in ((0, 0, 0), (1, 0, 0), (0, 1, 0)) + (((0, 0, 1),) if dim == 3 else ()):
        a_eval, nnps, ctx = _evaluator([probe, lat], KM.moment_equations(*lmn), kernel, dim)
        a_eval.compute(0.0, 0.1)
        got[lmn] = (probe.mom[0], probe.gx[0], probe.gy[0], probe.gz[0])
        ctx.close()
    mom, gx, gy, gz = got[(0, 0, 0)]
    print(name, dim, got)
    assert abs(mom - 1.0) < 0.5 * 10.0 ** -p0
    assert max(abs(gx), abs(gy), abs(gz)) < 0.5e-7
    for axis, lmn in enumerate(((1, 0, 0), (0, 1, 0), (0, 0, 1))[:dim]):
        mom, *g = got[lmn]
        assert abs(mom) < 0.5e-7
        for other in range(3):
            if other == axis:
                assert abs(g[other] + 1.0) < 0.5 * 10.0 ** -p1, (lmn, g)
            else:
                assert abs(g[other]) < 0.5 * 10.0 ** -p2, (lmn, g)


# ---------------------------------------------------------------------------
# every hand-written family against the reference's golden vectors
# ---------------------------------------------------------------------------
def _check_outputs(case, g, arrays, outs, tol, what):
    worst = 0.0
    for pa in arrays:
        for prop in outs:
            key = 'out/%s/%s' % (pa.name, prop)
            if key in g.files and prop in pa.properties:
                e = rel_err(pa.properties[prop], g[key])
                worst = max(worst, e)
                assert e < tol, (case, what, pa.name, prop, e)
    print('%s %s: max rel err %.3e' % (case, what, worst))
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize('variant', [6, 0])
@pytest.mark.parametrize('case', MK.GOLDEN_CASES)
def test_family_parity_with_reference_golden(case, variant):
    """fp64, both schedules: NNPS scalars equal, every output field within 1e-10 of the field maximum -- after the
    first evaluation and after a second one on device-resident state (the fused record layouts engage there, as in
    test_hip_parity.test_golden_parity_on_fused_records; the equation sets are idempotent on their inputs)."""
    g = load_golden(case + '.npz')
    arrays = arrays_from_golden(g, 'in')
    eqs, kernel, dim, outs = MK.golden_case(case, g)
    a_eval, nnps, ctx = _evaluator(arrays, eqs, kernel, dim, variant, sync='manual')
    for pa in arrays:
        pa.gpu.push()
    nnps.sync = False
    nnps.update()
    assert nnps.cell_size == float(g['nnps/cell_size'])
    assert np.array_equal(nnps.xmin, g['nnps/xmin'])
    assert np.array_equal(nnps.xmax, g['nnps/xmax'])
    assert np.array_equal(nnps.ncells_per_dim, g['nnps/ncells_per_dim'])
    assert nnps.n_cells == int(g['nnps/n_cells'])
    t, dt = float(g['t']), float(g['dt'])
    a_eval.compute(t, dt)
    a_eval.c_acceleration_eval.pull_outputs()
    _check_outputs(case, g, arrays, outs, TOL, 'variant %d' % variant)
    nnps.update()
    a_eval.compute(t, dt)
    a_eval.c_acceleration_eval.pull_outputs()
    _check_outputs(case, g, arrays, outs, TOL, 'variant %d, second evaluation' % variant)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize('case', MK.GOLDEN_CASES)
def test_family_parity_fp32_arithmetic(case):
    """option arith_f32 against the fp64 golden vectors at the existing fp32 bound (5e-5 of the field maximum), after
    the first evaluation and after a second one on device-resident state (the fp32 fused record layouts)"""
    g = load_golden(case + '.npz')
    arrays = arrays_from_golden(g, 'in')
    eqs, kernel, dim, outs = MK.golden_case(case, g)
    a_eval, nnps, ctx = _evaluator(arrays, eqs, kernel, dim, 6, sync='manual')
    ctx.set_option('arith_f32', 1)
    for pa in arrays:
        pa.gpu.push()
    nnps.sync = False
    t, dt = float(g['t']), float(g['dt'])
    for what in ('arith_f32', 'arith_f32, second evaluation'):
        nnps.update()
        a_eval.compute(t, dt)
        a_eval.c_acceleration_eval.pull_outputs()
        worst = _check_outputs(case, g, arrays, outs, TOL_F32, what)
        assert worst > 1e-9           # really fp32 arithmetic
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize('case', [c for c in MK.GOLDEN_CASES if 'elastic' not in c])
def test_neighbour_sets_match_reference(case):
    """neighbour counts and sets of the device's lists equal to the reference's (stored with the golden vectors).
    The elastic case is absent: make_golden._elastic_case, which made its fixture, stores no neighbour lists (nor does
    it for the existing elastic goldens); its NNPS grid values are compared in the parity test above."""
    from pysph_amd import device as dev
    from pysph_amd.nnps import HipNNPS
    g = load_golden(case + '.npz')
    arrays = arrays_from_golden(g, 'in')
    eqs, kernel, dim, outs = MK.golden_case(case, g)
    ctx = dev.HipContext(0)
    nnps = HipNNPS(dim, arrays, radius_scale=kernel.radius_scale, ctx=ctx)
    nnps.update()
    start, idx = nnps.get_csr(0, 0)
    gs, gi = g['nbrs/fluid/fluid/start'], g['nbrs/fluid/fluid/idx']
    assert np.array_equal(start, gs)
    assert np.diff(gs.astype(int)).min() >= 2
    assert np.array_equal(idx, np.concatenate([np.sort(gi[gs[i]:gs[i + 1]]) for i in range(len(gs) - 1)]))
    ctx.close()


# ---------------------------------------------------------------------------
# generated path
# ---------------------------------------------------------------------------
def generated_setup(dim, seed=5):
    """tests/test_hip_parity._custom_setup in 2 or 3 dimensions with h +-15 %: PowerLawState, KitchenSink (WIJ, DWIJ and
    the KERNEL / GRADIENT symbols WI, WJ, DWI, DWJ) and WallPush of tests/custom_equations.py"""
    from pysph_amd.equations import Group
    from pysph_amd.particle_array import get_particle_array
    from custom_equations import KitchenSink, PowerLawState, WallPush
    rng = np.random.default_rng(seed)
    n1 = 9 if dim == 3 else 20
    dx = 1.0 / n1
    g = (np.arange(n1) + 0.5) * dx
    if dim == 3:
        x, y, z = [a.ravel() for a in np.meshgrid(g, g, g, indexing='ij')]
    else:
        x, y = [a.ravel() for a in np.meshgrid(g, g, indexing='ij')]
        z = np.zeros_like(x)
    wall = y < 2.5 * dx
    arrays = []
    for name, msk in (('fluid', ~wall), ('solid', wall)):
        n = int(msk.sum())
        pa = get_particle_array(
            name=name, constants=dict(coef=np.array([1.25, -0.5])),
            x=x[msk] + 0.1 * dx * rng.uniform(-1, 1, n), y=y[msk] + 0.1 * dx * rng.uniform(-1, 1, n),
            z=z[msk] + (0.1 * dx * rng.uniform(-1, 1, n) if dim == 3 else 0.0),
            u=rng.uniform(-1, 1, n), v=rng.uniform(-1, 1, n), w=rng.uniform(-1, 1, n) * (dim == 3),
            h=1.3 * dx * (1 + 0.15 * rng.uniform(-1, 1, n)), m=dx ** dim * np.ones(n),
            rho=1 + 0.1 * rng.uniform(-1, 1, n), additional_props=['q', 'gx', 'gy', 'gz', 'e'])
        for k in ('q', 'gx', 'gy', 'gz', 'e', 'p'):
            pa.properties[k][:] = rng.uniform(1, 2, n)
        arrays.append(pa)
    eqs = [Group(real=False, equations=[PowerLawState('fluid', None, k=1.5, n=1.4),
                                        PowerLawState('solid', None, k=0.5, n=2.0)]),
           Group(equations=[KitchenSink('fluid', ['fluid', 'solid'], a=0.3, b=0.05, flag=True),
                            WallPush('fluid', ['solid'], c=0.7),
                            KitchenSink('solid', ['fluid'], a=0.1, b=2.0, flag=False)])]
    return arrays, eqs


GENERATED = [('WendlandQuinticC4', 3), ('SuperGaussian', 2)]


@pytest.mark.gpu
@pytest.mark.parametrize('kname,dim', GENERATED)
def test_generated_equations_vs_python(oracle, kname, dim):
    """user equations through the generated-family path with a new kernel against the same Python bodies run by
    oracle/py_eval.py with the host kernel object (pinned to the reference by test_more_kernels.py), at the 1e-10
    test_hip_parity.test_generated_custom_equations_vs_python holds that comparison to"""
    from oracle.py_eval import PyEval
    from pysph_amd import kernels as K
    import test_hip_parity as T
    arrays, eqs = generated_setup(dim)
    ref = T._copy_arrays(arrays)
    for r, a in zip(ref, arrays):
        r.constants = dict((k, v.copy()) for k, v in a.constants.items())
    kernel = getattr(K, kname)(dim=dim)
    t, dt = 0.25, 1e-3
    a_eval, nnps, ctx = _evaluator(arrays, eqs, kernel, dim)
    a_eval.compute(t, dt)
    onn = oracle.OracleNNPS(dim, ref, radius_scale=kernel.radius_scale)
    onn.update()
    PyEval(ref, eqs, kernel, onn).compute(t, dt)
    worst = 0.0
    for pa, pr in zip(arrays, ref):
        for prop in ('p', 'e', 'q', 'gx', 'gy', 'gz'):
            e = rel_err(pa.properties[prop], pr.properties[prop])
            worst = max(worst, e)
            assert e < TOL, (pa.name, prop, e)
    print('generated equations %s dim %d: max rel err %.3e' % (kname, dim, worst))
    ctx.close()


# ---------------------------------------------------------------------------
# interpolator
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('method', ['shepard', 'sph'])
def test_interpolator_equals_brute_force(method):
    """one scalar from 8^3 + 1 particles onto 101 points with WendlandQuinticC4(dim=3) against an O(M N) numpy sum with
    the host kernel class, at 1e-10 of the field maximum (the brute force of tests/test_interpolator.py)"""
    from pysph_amd import kernels as K
    from pysph_amd.particle_array import ParticleArray
    from pysph_amd.tools import Interpolator
    kernel = K.WendlandQuinticC4(dim=3)
    rng = np.random.default_rng(513)
    dx = 1.0 / 8
    g = np.meshgrid(*[dx * (np.arange(8) + 0.5)] * 3, indexing='ij')
    p = [np.append(a.ravel(), 0.5 + 0.01 * k) for k, a in enumerate(g)]
    n = p[0].size
    x, y, z = [a + 0.2 * dx * rng.uniform(-1, 1, n) for a in p]
    s = dict(x=x, y=y, z=z, h=1.2 * dx * (1 + 0.15 * rng.uniform(-1, 1, n)), m=dx ** 3 * (1 + 0.05 * rng.uniform(-1, 1, n)),
             rho=1 + 0.03 * rng.uniform(-1, 1, n))
    s['u'] = 1 + np.sin(3 * x) - 2 * y ** 2 + x * z
    px, py, pz = rng.uniform(-0.1, 1.1, (3, 101))
    hp = s['h'].max()
    d = [a[:, None] - s[c][None, :] for a, c in zip((px, py, pz), 'xyz')]
    r2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    nbr = (r2 < (2.0 * hp) ** 2) | (r2 < (2.0 * s['h'][None, :]) ** 2)
    w = np.where(nbr, kernel.kernel(rij=np.sqrt(r2), h=0.5 * (hp + s['h'])[None, :]), 0.0)
    if method == 'sph':
        w = w * (s['m'] / s['rho'])[None, :]
    den = w.sum(axis=1)
    want = (w * s['u'][None, :]).sum(axis=1)
    if method == 'shepard':
        want = np.where(den > 1e-12, want / np.where(den > 1e-12, den, 1.0), want)
    assert np.count_nonzero(want) > 60
    interp = Interpolator([ParticleArray(name='fluid', **{k: v.copy() for k, v in s.items()})], kernel=kernel,
                          x=px, y=py, z=pz, method=method)
    got = interp.interpolate('u')
    err = rel_err(got, want)
    print(method, 'rel_err %.3e' % err)
    assert got.shape == px.shape and err < TOL
    interp.close()


# ---------------------------------------------------------------------------
# the C-ABI and a kernel it does not have
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('kind,dim', [(99, 1), (5, 3), (6, 1), (0, 1)])
def test_unknown_kernel_is_an_error_and_nothing_is_written(kind, dim):
    """sph_eval_group through ctypes with a kind outside 1..10, and with a kind in a dimension its class does not have:
    SPH_ERR_UNSUPPORTED, a message in the library's error text, the destination array as it was"""
    from pysph_amd import device as dev
    g = load_golden('more_sd1d_WendlandQuinticC2_1D.npz')
    arrays = arrays_from_golden(g, 'in')
    eqs, kernel, d1, outs = MK.golden_case('more_sd1d_WendlandQuinticC2_1D', g)
    a_eval, nnps, ctx = _evaluator(arrays, eqs, kernel, d1, sync='manual')
    pa = arrays[0]
    pa.rho[:] = -7.25
    pa.gpu.push()
    nnps.sync = False
    nnps.update()
    ev = a_eval.c_acceleration_eval
    unit = [u for leaf in ev._leaves(ev.plan) for u in leaf.units if hasattr(u, 'cg')][0]
    unit.refresh(0, -1)
    bad = dev.SphKernel(kind, dim, float(kernel.fac), float(kernel.radius_scale), float(kernel.get_deltap()))
    rc = ev.lib.sph_eval_group(ctx._h, C.byref(bad), C.byref(unit.cg), 0.0, 1e-4)
    assert rc == -4                                       # SPH_ERR_UNSUPPORTED (include/sphhip.h)
    msg = ev.lib.sph_last_error().decode()
    assert 'kernel' in msg and str(kind) in msg, msg
    pa.rho[:] = 0.0
    pa.gpu.pull('rho')
    assert np.all(pa.rho == -7.25)
    # ... and the same call with the kernel it was built for does run
    rc = ev.lib.sph_eval_group(ctx._h, C.byref(ev.ckernel), C.byref(unit.cg), 0.0, 1e-4)
    assert rc == 0, ev.lib.sph_last_error()
    pa.gpu.pull('rho')
    assert rel_err(pa.rho, g['out/fluid/rho']) < TOL
    ctx.close()


# ---------------------------------------------------------------------------
# what __graft_entry__.build() compiles ahead of the GPU run
# ---------------------------------------------------------------------------
def prebuild():
    """the generated families of this module and the probe library, built without a GPU"""
    from pysph_amd import codegen
    from pysph_amd import kernels as K
    from pysph_amd.acceleration_eval import AccelerationEval, _CGroup

    def plan(arrays, eqs, kernel):
        count = 0
        a = AccelerationEval(arrays, eqs, kernel)
        ids = dict((pa.name, i) for i, pa in enumerate(arrays))
        amap = dict((pa.name, pa) for pa in arrays)
        for g in a.equation_groups:
            count += sum(hasattr(u, 'fam') for u in _CGroup(g, ids, amap, K.kernel_id(kernel)).units)
        return count

    def every():
        n = 0
        for name, dim in sorted(TM.PLACES):
            n += plan(list(KM.moment_arrays(2)), KM.moment_equations(), getattr(K, name)(dim=dim))
        for kname, dim in GENERATED:
            arrays, eqs = generated_setup(dim)
            n += plan(arrays, eqs, getattr(K, kname)(dim=dim))
        return n
    codegen.DEFERRED = []
    every()
    codegen.build_deferred()
    return every(), MK.build_probe_library()
