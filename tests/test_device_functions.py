"""The device functions every neighbour pair goes through -- fast_rcp, fast_sqrt_rsqrt, pair_geom, pair_w,
pair_gradfac, pair_gradh (pysph_amd/csrc/sph_pair.h) and SphKernel<1..4>::w/dw/dwq (sph_kernels.h), INSUP / UH both
ways, fp64 and fp32 -- one value per thread through tests/probes/device_functions.hip, against the reference's
formulas (pysph/base/kernels.py) evaluated with mpmath at 50 digits (helpers.mp_kernel).

The parity tests see these functions only through sums over ~100 neighbours judged at 1e-10 of a field maximum; here a
wrong ulp fails.

Error budgets.  u = unit roundoff of the type (2^-53 / 2^-24).  For the polynomial kernels
    |device - reference| <= C u S
with S the sum of the absolute values of the polynomial's terms as the device code writes them (the differences
t_k = k - q count as factors, not as sums) and C the number of roundings the longest term goes through plus the
additions between terms.  A rounding of relative size u in a factor that appears n times moves the term by n u, so
the subtraction that forms t_k counts once per appearance of t_k; a multiplication by a power of two (0.5 q, 2 q,
0.25 x) is exact and counts nothing:

  CubicSpline      w   q > 1:  0.25 t2 t2 t2                 3 (t2) + 2 mul                                = 5
                       q <= 1: 1 - 1.5 q q (1 - 0.5 q)       1.5q, q, 1 (inner sub), () = 4, + 1 addition  = 5
                   dw  q > 1:  -0.75 t2 t2                   2 (t2) + 2 mul                                = 4
                       q <= 1: -3 q (1 - 0.75 q)             0.75q, sub, 3q, ()                            = 4
  WendlandQuintic  t = 1 - 0.5 q: one rounding
                   w   t t t t (2 q + 1)                     4 (t) + 1 (+1) + 4 mul                        = 9
                   dw  -5 q t t t                            3 (t) + 4 mul                                 = 7
                   dwq -5 t t t                              3 (t) + 3 mul                                 = 6
  QuinticSpline    w   t3^5 - 6 t2^5 + 15 t1^5               longest 6 t2^5: 5 (t2) + 5 mul, + 2 additions = 12,
                                                             held to the 10 this suite allows the quintic  = 10
                   dw  -5 t3^4 + 30 t2^4 - 75 t1^4           longest 30 t2^4: 4 (t2) + 4 mul, + 2 additions = 10
  Gaussian         exp(-q q): 4 ulp of exp, plus the polynomial part: the argument's one multiplication moves the
                   result by q^2 u relative, the factors -2 q (dw: 2 mul) and -2 (dwq: 1 mul) by u each:
                   |device - reference| <= 4 ulp(exp) |factor| + (q^2 + mul) u |reference|

(Counting every operation of the longest term once, t_k included -- 6/4, 8/6/5, 8/7 -- is NOT a bound: on an MI355X
WendlandQuintic dwq in fp32 reaches 5.11 u S against that count's 5.)  Worst C seen on an MI355X, fp64 / fp32:
CubicSpline w 1.82 / 1.83, dw 2.21 / 2.30; WendlandQuintic w 4.23 / 5.68, dw 5.05 / 5.02, dwq 4.14 / 5.11; QuinticSpline
w 5.37 / 6.39, dw 4.33 / 4.48; the Gaussian uses 0.65 of its budget at the most.
"""
import functools

import numpy as np
import pytest

from conftest import load_golden
import helpers as H

DPS = 50
U = {np.float64: 2.0 ** -53, np.float32: 2.0 ** -24}
DTYPES = [np.float64, np.float32]
# documented accuracy of the fast paths (sph_pair.h: "one step leaves ~1e-14 relative"; fp32: the hardware
# instructions are 1-ulp, s = a * rs adds a rounding: 2 ulp = 2 * 2^-23 relative at the most)
FAST_REL = {np.float64: 1e-14, np.float32: 2 * 2.0 ** -23}
C_W = {1: 5, 2: 9, 3: 10}
C_DW = {1: 4, 2: 7, 3: 10}
C_DWQ = {2: 6}
HAS_DWQ = {1: False, 2: True, 3: False, 4: True}


def _mp():
    import mpmath as mp
    mp.mp.dps = DPS
    return mp


def term_sums(kk, q):
    """S of the module docstring for w, dw, dwq (float64 arrays; 0 where the kernel is identically 0)"""
    q = np.asarray(q, dtype=np.float64)
    if kk == 1:
        t2 = np.abs(2 - q)
        sw = np.where(q > 1, 0.25 * t2 ** 3, 1 + 1.5 * q * q * np.abs(1 - 0.5 * q))
        sd = np.where(q > 1, 0.75 * t2 ** 2, 3 * q * np.abs(1 - 0.75 * q))
        return np.where(q > 2, 0, sw), np.where(q > 2, 0, sd), np.zeros_like(q)
    if kk == 2:
        t = np.abs(1 - 0.5 * q)
        ins = q < 2
        return ins * t ** 4 * (2 * q + 1), ins * 5 * q * t ** 3, ins * 5 * t ** 3
    if kk == 3:
        t3, t2, t1 = np.abs(3 - q), np.maximum(2 - q, 0), np.maximum(1 - q, 0)
        ins = q <= 3
        return ins * (t3 ** 5 + 6 * t2 ** 5 + 15 * t1 ** 5), ins * (5 * t3 ** 4 + 30 * t2 ** 4 + 75 * t1 ** 4), np.zeros_like(q)
    raise KeyError(kk)


def slope_sums(kk, q):
    """sum of the absolute values of the terms of d/dq of w, dw, dwq, term by term as in term_sums (Gaussian
    included): how far each function moves per unit of q.  The pair functions receive q = rij * h1, a product rounded
    to u q -- and under the product's -ffp-contract=fast the compiler folds that product into the polynomial's first
    operation (t_k = k - rij h1 becomes one fma), so the polynomial sees the UNROUNDED product while the stored q and
    every comparison see the rounded one.  Either way the argument is within u q of the stored q."""
    q = np.asarray(q, dtype=np.float64)
    z = np.zeros_like(q)
    if kk == 1:
        t2 = np.abs(2 - q)
        dw = np.where(q > 1, 0.75 * t2 ** 2, 3 * q * np.abs(1 - 0.5 * q) + 0.75 * q * q)
        ddw = np.where(q > 1, 1.5 * t2, 3 * np.abs(1 - 0.75 * q) + 2.25 * q)
        return np.where(q > 2, 0, dw), np.where(q > 2, 0, ddw), z
    if kk == 2:
        t = np.abs(1 - 0.5 * q)
        ins = q < 2
        return ins * (2 * t ** 3 * (2 * q + 1) + 2 * t ** 4), ins * (5 * t ** 3 + 7.5 * q * t ** 2), ins * 7.5 * t ** 2
    if kk == 3:
        t3, t2, t1 = np.abs(3 - q), np.maximum(2 - q, 0), np.maximum(1 - q, 0)
        ins = q <= 3
        return ins * (5 * t3 ** 4 + 30 * t2 ** 4 + 75 * t1 ** 4), ins * (20 * t3 ** 3 + 120 * t2 ** 3 + 300 * t1 ** 3), z
    if kk == 4:
        e = np.where(q < 3, np.exp(-q * q), 0.0)
        return 2 * q * e, 2 * e * (1 + 2 * q * q), 4 * q * e
    raise KeyError(kk)


def edge_q(kk, dtype):
    """q = 0, every knot and the support radius with their neighbours on both sides, 4096 log-spaced q in
    [2^-60, support], 4096 uniform q, and a few beyond the support"""
    sup = H.KERNEL_SUPPORT[kk]
    rng = np.random.default_rng(100 + kk)
    pts = [0.0]
    for k in H.KERNEL_KNOTS[kk] + (sup,):
        k = dtype(k)
        pts += [np.nextafter(k, dtype(0)), k, np.nextafter(k, dtype(10))]
    q = np.concatenate([np.array(pts, dtype=dtype),
                        (2.0 ** np.linspace(-60, np.log2(sup), 4096)).astype(dtype),
                        rng.uniform(0, sup, 4096).astype(dtype),
                        np.array([sup * 1.0001, sup * 1.5, 10.0, 1e6, 1e30], dtype=dtype)])
    return q


@functools.lru_cache(maxsize=None)
def reference_at(kk, dtype):
    """(q, [W(q)], [dW/dq(q)]) as mpf lists -- computed once per kernel and type, shared by the tests"""
    mp = _mp()
    q = edge_q(kk, dtype)
    w, dw = [], []
    for x in q:
        a, b = H.mp_kernel(kk, mp.mpf(float(x)))
        w.append(a)
        dw.append(b)
    return q, w, dw


def _abs_err(dev, ref):
    """|device - reference| per element as float64, the subtraction in mpmath"""
    mp = _mp()
    return np.array([float(abs(mp.mpf(float(d)) - r)) for d, r in zip(dev, ref)])


def _bits(a):
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def _spacing(x, dtype):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(dtype)).astype(np.float64)


# ---------------------------------------------------------------------------
# the reference itself, pinned before anything is judged by it (no GPU)
# ---------------------------------------------------------------------------
GOLDEN_KERNELS = [(kk, dim) for kk in (1, 2, 3, 4) for dim in (1, 2, 3) if not (kk == 2 and dim == 1)]


def _golden_vs_mp(kk, dim):
    """per stored sample: (|golden - mp| for w, dwdq), the mp values, q and the normalisation"""
    mp = _mp()
    g = load_golden('kernels.npz')
    key = '%s/%d/' % (H.KERNEL_NAMES[kk], dim)
    h, r, sigma = g[key + 'h'], g[key + 'r'], float(g[key + 'fac'])
    rows = []
    for i in range(h.size):
        w, dw = H.mp_kernel_wdw(kk, r[i], h[i], sigma, dim)
        h1 = 1.0 / h[i]
        rows.append((float(abs(mp.mpf(float(g[key + 'w'][i])) - w)), float(abs(mp.mpf(float(g[key + 'dwdq'][i])) - dw)),
                     float(w), float(dw), r[i] * h1, sigma * h1 ** dim))
    return [np.array(c) for c in zip(*rows)]


@pytest.mark.parametrize('kk,dim', GOLDEN_KERNELS)
def test_mpmath_reference_reproduces_golden_kernels(kk, dim):
    """helpers.mp_kernel / mp_kernel_wdw reproduce tests/golden/kernels.npz (the reference's own Python classes in
    fp64: w, dwdq and the gradient) to 2 ulp of every stored value.

    The stored values carry the rounding of their own fp64 evaluation -- up to 154 ulp of the value where the quintic
    spline's dW/dq crosses zero, 8 ulp where exp(-q^2) amplifies the rounding of q^2 -- so no EXACT evaluation can be
    that close to them.  The reference's lines can: helpers.mp_kernel performs the reference's operations in the
    reference's order, and at a working precision of 53 bits mpmath rounds each of them to nearest as IEEE double
    does, so the same code that is run at 50 digits to judge the device retraces the file's evaluation rounding by
    rounding.  What is left is libm's exp against mpmath's correctly rounded one (below 1 ulp, carried through the
    normalisation's multiplications).  A wrong coefficient, knot, branch condition or guard in those lines shows at
    once; that they mean the same at 50 digits is test_mpmath_reference_within_rounding_budget_of_golden."""
    mp = _mp()
    g = load_golden('kernels.npz')
    key = '%s/%d/' % (H.KERNEL_NAMES[kk], dim)
    h, r, xij, sigma = g[key + 'h'], g[key + 'r'], g[key + 'xij'], float(g[key + 'fac'])
    worst = {'w': 0.0, 'dwdq': 0.0, 'grad': 0.0}
    inside = 0
    with mp.workprec(53):
        for i in range(h.size):
            w, dw, grad = H.mp_kernel_wdw(kk, r[i], h[i], sigma, dim, xij=xij[i])
            inside += w != 0
            stored = [('w', g[key + 'w'][i], w), ('dwdq', g[key + 'dwdq'][i], dw)]
            stored += [('grad', g[key + 'grad'][i][c], grad[c]) for c in range(3)]
            for name, got, ref in stored:
                ref = float(ref)            # exact: the mpf has 53 bits
                if ref == 0:
                    assert got == 0, (name, i, got)
                else:
                    worst[name] = max(worst[name], abs(got - ref) / np.spacing(abs(ref)))
    print('%s dim %d: max ulp %s' % (H.KERNEL_NAMES[kk], dim, ', '.join('%s %.2f' % kv for kv in sorted(worst.items()))))
    assert inside > 16                       # the samples do reach inside the support
    assert max(worst.values()) <= 2, worst


@pytest.mark.parametrize('kk,dim', GOLDEN_KERNELS)
def test_mpmath_reference_within_rounding_budget_of_golden(kk, dim):
    """The same comparison against the rounding budget of the fp64 evaluation that produced the stored values: the
    module's C u S for the kernel polynomial, plus dim + 1 multiplications of the normalisation (fac = sigma h1..h1,
    val * fac).  A wrong coefficient, knot or branch in helpers.mp_kernel is off by orders of magnitude more."""
    ew, ed, w, dw, q, fac = _golden_vs_mp(kk, dim)
    u = U[np.float64]
    if kk == 4:
        e = np.where(q < 3, np.exp(-q * q), 0.0)
        bw = (4 * np.spacing(e) + (q * q + dim + 1) * u * e) * fac
        bd = (4 * np.spacing(e) * 2 * q + (q * q + 2 + dim + 1) * u * 2 * q * e) * fac
    else:
        sw, sd, _ = term_sums(kk, q)
        bw = (C_W[kk] + dim + 1) * u * sw * fac
        bd = (C_DW[kk] + dim + 1) * u * sd * fac
    assert np.all(ew <= bw), np.max(ew / np.maximum(bw, 1e-300))
    assert np.all(ed <= bd), np.max(ed / np.maximum(bd, 1e-300))
    assert np.count_nonzero(w) > 16          # the samples do reach inside the support


# ---------------------------------------------------------------------------
# SphKernel<KK>::w / dw / dwq
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES, ids=['f64', 'f32'])
@pytest.mark.parametrize('kk', [1, 2, 3])
def test_polynomial_kernels_within_rounding_budget(kk, dtype):
    mp = _mp()
    q, rw, rdw = reference_at(kk, dtype)
    sup, u = H.KERNEL_SUPPORT[kk], U[dtype]
    w, dw, dwq = H.probe_kernel(kk, False, q)
    wi, dwi, dwqi = H.probe_kernel(kk, True, q)
    for a in (w, dw, dwq):
        assert np.all(np.isfinite(a))
    for a in (wi, dwi, dwqi):       # INSUP is the caller's promise that q is inside the support
        assert np.all(np.isfinite(a[q <= sup]))
    sw, sd, sq = term_sums(kk, q)
    worst = {}
    for name, dev, ref, s, c in (('w', w, rw, sw, C_W[kk]), ('dw', dw, rdw, sd, C_DW[kk])):
        err = _abs_err(dev, ref)
        seen = err / np.where(s > 0, u * s, 1.0)
        worst[name] = seen[s > 0].max()
        assert np.all(err[s == 0] == 0), name
        assert np.all(err <= c * u * s), (name, worst[name], q[np.argmax(seen)])
    if HAS_DWQ[kk]:
        pos = q > 0
        ref = [b / mp.mpf(float(x)) if x > 0 else mp.mpf(-5) for b, x in zip(rdw, q)]   # dw/q -> -5 at q = 0
        err = _abs_err(dwq, ref)
        worst['dwq'] = (err / np.where(sq > 0, u * sq, 1.0))[sq > 0].max()
        assert np.all(err <= C_DWQ[kk] * u * sq), worst['dwq']
        assert pos.any()
    else:
        assert np.all(dwq == 0)
    print('%s %s: worst C seen %s' % (H.KERNEL_NAMES[kk], dtype.__name__,
                                     ', '.join('%s %.2f' % kv for kv in sorted(worst.items()))))
    # exactly 0 outside the support without INSUP
    out = q >= sup if kk == 2 else q > sup
    assert out.sum() >= 5
    for a in (w, dw, dwq):
        assert np.all(a[out] == 0)
    # INSUP only drops the support test: bit for bit the same inside
    ins = q <= sup
    for a, b in ((w, wi), (dw, dwi), (dwq, dwqi)):
        assert np.array_equal(_bits(a[ins]), _bits(b[ins]))


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES, ids=['f64', 'f32'])
def test_gaussian_kernel_within_rounding_budget(dtype):
    mp = _mp()
    q, rw, rdw = reference_at(4, dtype)
    u = U[dtype]
    q64 = q.astype(np.float64)
    res = {}
    for insup in (False, True):
        w, dw, dwq = res[insup] = H.probe_kernel(4, insup, q)
        for a in (w, dw, dwq):
            assert np.all(np.isfinite(a))
            assert np.all(a[q >= 3] == 0)            # cut off at q = 3 whatever the caller guarantees
    assert (q >= 3).sum() >= 5 and np.all(res[False][0][q < 3] > 0)
    for a, b in zip(res[False], res[True]):
        assert np.array_equal(_bits(a), _bits(b))
    w, dw, dwq = res[False]
    e = np.array([float(x) for x in rw])
    ulp_e = _spacing(e, dtype) * (q < 3)
    rdwq = [-2 * x for x in rw]
    worst = {}
    for name, dev, ref, factor, nmul in (('w', w, rw, 1.0, 0), ('dw', dw, rdw, 2 * q64, 2), ('dwq', dwq, rdwq, 2.0, 1)):
        err = _abs_err(dev, ref)
        bound = 4 * ulp_e * factor + (q64 * q64 + nmul) * u * factor * e
        worst[name] = np.max(err / np.where(bound > 0, bound, 1.0))
        assert np.all(err <= bound), (name, worst[name])
    print('Gaussian %s: worst fraction of the budget %s' % (dtype.__name__,
                                                           ', '.join('%s %.2f' % kv for kv in sorted(worst.items()))))


# ---------------------------------------------------------------------------
# fast_rcp / fast_sqrt_rsqrt
# ---------------------------------------------------------------------------
def _wide_operands(dtype, n=16384):
    """random mantissas over [2^-200, 2^200] (fp64) / [2^-60, 2^60] (fp32: squares and reciprocals stay normal),
    and the exact powers of two"""
    e = 200 if dtype is np.float64 else 60
    rng = np.random.default_rng(77)
    x = (rng.uniform(1, 2, n) * 2.0 ** rng.integers(-e, e, n)).astype(dtype)
    return np.concatenate([x, (2.0 ** np.arange(-e, e + 1)).astype(dtype)])


# measured on an MI355X over _wide_operands (the maxima the test prints): fp64 relative error rcp 1.97e-15,
# rsqrt 3.94e-15, sqrt 3.99e-15; fp32 rcp 0.80 ulp, rsqrt 0.81 ulp, sqrt 1.84 ulp
@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES, ids=['f64', 'f32'])
def test_fast_rcp_and_sqrt_accuracy(dtype):
    """fp64: maximum relative error against mpmath below the figure sph_pair.h documents for one Newton step
    (1e-14); fp32: 2 ulp."""
    mp = _mp()
    x = _wide_operands(dtype)
    r = H.probe_rcp(x)
    s, rs = H.probe_sqrt_rsqrt(x)
    mx = [mp.mpf(float(v)) for v in x]
    refs = {'rcp': (r, [1 / v for v in mx]), 'sqrt': (s, [mp.sqrt(v) for v in mx]), 'rsqrt': (rs, [1 / mp.sqrt(v) for v in mx])}
    worst = {}
    for name, (dev, ref) in refs.items():
        assert np.all(np.isfinite(dev)), name
        err = _abs_err(dev, ref)
        reff = np.array([float(v) for v in ref])
        if dtype is np.float64:
            worst[name] = np.max(err / reff)
        else:
            worst[name] = np.max(err / _spacing(reff, dtype))
    print('fast paths %s: max %s %s' % (dtype.__name__, 'relative error' if dtype is np.float64 else 'ulp',
                                        ', '.join('%s %.3e' % kv for kv in sorted(worst.items()))))
    for name, v in worst.items():
        assert v <= (1e-14 if dtype is np.float64 else 2.0), (name, v)


# ---------------------------------------------------------------------------
# pair_geom / pair_w / pair_gradfac / pair_gradh
# ---------------------------------------------------------------------------
H_VALUES = {np.float64: [2.0 ** -30, 1.1 * 2.0 ** -3, 1.3, 2.0 ** 40], np.float32: [2.0 ** -10, 0.013, 1.3, 2.0 ** 10]}


def _pair_inputs(kk, dtype, hij):
    """r2 = 0, subnormal, both sides of (1e-12)^2, and (q hij)^2 for q = 0.., every knot, the support radius and 256
    log-spaced q in [2^-20, support]"""
    sup = H.KERNEL_SUPPORT[kk]
    tiny = np.finfo(dtype).smallest_subnormal
    g2 = dtype(1e-12) * dtype(1e-12)
    edge = [0.0, tiny, 1000 * tiny, np.nextafter(g2, dtype(0)), g2, np.nextafter(g2, dtype(1)), 4 * g2]
    qs = np.concatenate([2.0 ** np.linspace(-20, np.log2(sup), 256), np.array(H.KERNEL_KNOTS[kk] + (sup, 1.01 * sup, 2 * sup)),
                         np.array(H.KERNEL_KNOTS[kk] + (sup,)) * (1 - 1e-6)])
    r = (qs * float(hij)).astype(dtype)
    return np.concatenate([np.array(edge, dtype=dtype), r * r])


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES, ids=['f64', 'f32'])
@pytest.mark.parametrize('kk', [1, 2, 3, 4])
def test_pair_geometry_and_gradient_factors(kk, dtype):
    """pair_geom's outputs against numpy in the same type (bit for bit where the code is plain IEEE arithmetic --
    HIJ, EPS, the normalisation, q = rij * h1, and ALL of the Gaussian's EXACT_Q path -- within the documented
    accuracy where it goes through the fast reciprocal / square root), then pair_w, pair_gradfac and pair_gradh
    against mpmath AT the device's own geometry, so that each budget covers that function's arithmetic only: the
    kernel's C u S of the module docstring, u S per further multiplication, and u q times the function's slope for
    the rounding of q = rij * h1 itself (slope_sums)."""
    mp = _mp()
    u, fast, sup = U[dtype], FAST_REL[dtype], H.KERNEL_SUPPORT[kk]
    exact_q = kk == 4
    guard = dtype(1e-12)
    clamp = dtype(1e-300) if dtype is np.float64 else dtype(1e-35)
    tiny = float(np.finfo(dtype).smallest_subnormal)
    sigma = 0.3183098861837907          # any normalisation: 1/pi
    worst = {'w': 0.0, 'gradfac': 0.0, 'gradh': 0.0}
    n_guarded = 0
    for dim in (1, 2, 3):
        for h in H_VALUES[dtype]:
            for uh in (False, True):
                h = dtype(h)
                hi, hj = (h, h) if uh else (dtype(h * 1.1), dtype(h * 0.9))
                hij = dtype(0.5) * (hi + hj)
                r2 = _pair_inputs(kk, dtype, hij)
                if uh:          # the caller's guarantee of the uniform-h kernels: the pair passed r2 < (radius h)^2
                    r2 = r2[r2 < (dtype(sup) * hij) ** 2]
                one = dtype(1)
                h1u = one / hij
                facu = dtype(sigma) * h1u
                for _ in range(dim - 1):
                    facu = facu * h1u
                epsu = dtype(0.01) * hij * hij
                o = H.probe_pair(kk, uh, r2, np.full(r2.size, hi), np.full(r2.size, hj), sigma, dim,
                                 uniform=(hij, h1u, facu, epsu))
                ctx = (kk, dtype.__name__, dim, float(h), uh)
                for k, a in o.items():
                    assert np.all(np.isfinite(a)), (k,) + ctx
                # --- geometry
                assert np.array_equal(o['hij'], np.full(r2.size, hij)), ctx
                assert np.array_equal(o['eps'], np.full(r2.size, epsu)), ctx
                assert np.array_equal(_bits(o['q']), _bits(o['rij'] * o['h1'])), ctx
                if uh or exact_q:
                    assert np.array_equal(o['h1'], np.full(r2.size, h1u)), ctx
                    assert np.array_equal(o['fac'], np.full(r2.size, facu)), ctx
                else:
                    assert np.all(np.abs(o['h1'].astype(np.float64) * float(hij) - 1) <= fast), ctx
                    f = dtype(sigma) * o['h1']
                    for _ in range(dim - 1):
                        f = f * o['h1']
                    assert np.array_equal(_bits(o['fac']), _bits(f)), ctx
                if exact_q:
                    rij = np.sqrt(r2)
                    with np.errstate(divide='ignore'):
                        rinv = np.where(rij > 0, one / rij, dtype(0)).astype(dtype)
                    assert np.array_equal(_bits(o['rij']), _bits(rij)), ctx
                    assert np.array_equal(_bits(o['rinv']), _bits(rinv)), ctx
                else:
                    rc = [mp.sqrt(mp.mpf(float(max(v, clamp)))) for v in r2]
                    e1 = _abs_err(o['rij'], rc) / np.array([float(v) for v in rc])
                    e2 = _abs_err(o['rinv'], [1 / v for v in rc]) * np.array([float(v) for v in rc])
                    assert e1.max() <= fast and e2.max() <= fast, ctx + (e1.max(), e2.max())
                # --- the kernel functions at the device's geometry
                q, fac, h1d, rinv, rij = (o[k].astype(np.float64) for k in ('q', 'fac', 'h1', 'rinv', 'rij'))
                ref = [H.mp_kernel(kk, mp.mpf(v)) for v in q]
                rw, rdw = [a for a, b in ref], [b for a, b in ref]
                if uh and kk != 4:   # INSUP: no support test (inputs are inside; q may round onto the radius itself)
                    assert np.all(q <= sup), ctx
                if kk == 4:
                    e = np.array([float(v) for v in rw])
                    ulp_e = _spacing(e, dtype) * (q < 3)
                    sw = e
                    bw = 4 * ulp_e + (q * q) * u * e
                    bdw = 4 * ulp_e * 2 * q + (q * q + 2) * u * 2 * q * e          # dw = -2 q exp
                    bdwq = 4 * ulp_e * 2 + (q * q + 1) * u * 2 * e                 # dwq = -2 exp
                    sdw = 2 * q * e
                else:
                    sw, sdw, sdwq = term_sums(kk, q)
                    bw, bdw = C_W[kk] * u * sw, C_DW[kk] * u * sdw
                    bdwq = C_DWQ[kk] * u * sdwq if HAS_DWQ[kk] else None
                # ... each evaluated at an argument within dq = u q of the stored q: by the mean value theorem the
                # function moves by at most dq times the largest slope over [q - dq, q + dq], which slope_sums (terms
                # monotone in |t_k|) takes at an end of the interval -- next to the support radius dq is as large as
                # t_k itself, first order in dq is not enough there
                dq = u * q
                lw, ldw, ldwq = (np.maximum.reduce(c) for c in zip(*[slope_sums(kk, np.maximum(q + sg * dq, 0))
                                                                     for sg in (-1, 0, 1)]))
                bw, bdw = bw + dq * lw, bdw + dq * ldw
                if HAS_DWQ[kk]:
                    bdwq = bdwq + dq * ldwq
                # pair_w = w(q) * fac: one more multiplication
                err = _abs_err(o['w'], [a * mp.mpf(f) for a, f in zip(rw, fac)])
                bound = (bw + u * sw) * fac + tiny
                assert np.all(err <= bound), ('pair_w',) + ctx + (np.max(err / bound),)
                worst['w'] = max(worst['w'], np.max(err / bound))
                # pair_gradfac: the reference's dwdq * h1 / rij, 0 for rij <= 1e-12
                live = o['rij'] > guard
                n_guarded += int(np.count_nonzero(~live))
                assert np.all(o['gradfac'][~live] == 0), ctx
                if HAS_DWQ[kk]:     # dwq(q) (fac h1 h1): 3 more multiplications; dw(q)/q = dw(q) h1 / rij up to q's rounding
                    gref = [b / mp.mpf(qq) * mp.mpf(f) * mp.mpf(a) ** 2 if lv else mp.mpf(0)
                            for b, qq, f, a, lv in zip(rdw, q, fac, h1d, live)]
                    sdq = 5 * np.abs(1 - 0.5 * q) ** 3 * (q < 2) if kk == 2 else 2 * e
                    bound = (bdwq + 3 * u * sdq) * fac * h1d * h1d + tiny
                else:               # dw(q) (fac h1) rinv: 3 more multiplications
                    gref = [b * mp.mpf(f) * mp.mpf(a) * mp.mpf(ri) if lv else mp.mpf(0)
                            for b, f, a, ri, lv in zip(rdw, fac, h1d, rinv, live)]
                    bound = (bdw + 3 * u * sdw) * fac * h1d * rinv + tiny
                err = _abs_err(o['gradfac'], gref)
                assert np.all(err[live] <= bound[live]), ('pair_gradfac',) + ctx + (np.max(err[live] / bound[live]),)
                worst['gradfac'] = max(worst['gradfac'], np.max(err[live] / bound[live]))
                # pair_gradh = -fac h1 (dw q + w dim): per term one multiplication, one addition, two multiplications
                href = [-mp.mpf(f) * mp.mpf(a) * (b * mp.mpf(qq) + w_ * dim) for f, a, b, qq, w_ in zip(fac, h1d, rdw, q, rw)]
                err = _abs_err(o['gradh'], href)
                sh = sdw * q + sw * dim
                bound = (bdw * q + bw * dim + 4 * u * sh) * fac * h1d + tiny
                assert np.all(err <= bound), ('pair_gradh',) + ctx + (np.max(err / bound),)
                worst['gradh'] = max(worst['gradh'], np.max(err / bound))
    assert n_guarded >= 3 * len(H_VALUES[dtype]) * 2 * 4     # r2 = 0, subnormal and <= (1e-12)^2 did reach the guard
    print('%s %s: worst fraction of the budget %s' % (H.KERNEL_NAMES[kk], dtype.__name__,
                                                     ', '.join('%s %.2f' % kv for kv in sorted(worst.items()))))
