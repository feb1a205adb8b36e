"""Helpers of the tests of the smoothing kernels 5..10 (test_more_kernels.py, test_more_kernels_gpu.py): the
reference's formulas restated for mpmath, the term sums of the error budgets, the device probes
(tests/probes/device_functions_more.hip) and the equation sets of the golden cases of
tests/golden/make_more_kernels_golden.py."""
import os

import numpy as np

import helpers as H
from pysph_amd import kernels as K

NAMES = {5: 'WendlandQuinticC2_1D', 6: 'WendlandQuinticC4', 7: 'WendlandQuinticC4_1D', 8: 'WendlandQuinticC6',
         9: 'WendlandQuinticC6_1D', 10: 'SuperGaussian'}
DIMS = {5: (1,), 6: (2, 3), 7: (1,), 8: (2, 3), 9: (1,), 10: (1, 2, 3)}
SUPPORT = {5: 2.0, 6: 2.0, 7: 2.0, 8: 2.0, 9: 2.0, 10: 3.0}
KIND_DIMS = [(kk, dim) for kk in sorted(NAMES) for dim in DIMS[kk]]
PROBE_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'probes', 'device_functions_more.hip')

# The Wendlands as the DEVICE writes them (sph_kernels.h): w = t^n P(q), dw = c q D(q) t^(n-1), dwq = c D(q) t^(n-1),
# t = 1 - q/2; P and D lowest power first.  All coefficients of P and D are positive.
WENDLAND = {
    5: dict(n=3, P=(1.0, 1.5), c=-3.0, D=(1.0,)),
    6: dict(n=6, P=(1.0, 3.0, 35.0 / 12.0), c=-14.0 / 3.0, D=(1.0, 2.5)),
    7: dict(n=5, P=(1.0, 2.5, 2.0), c=-3.5, D=(1.0, 2.0)),
    8: dict(n=8, P=(1.0, 4.0, 6.25, 4.0), c=-5.5, D=(1.0, 3.5, 4.0)),
    9: dict(n=7, P=(1.0, 3.5, 4.75, 2.625), c=-0.5, D=(9.0, 27.0, 26.25)),
}
# C of |device - reference| <= C u S, derived in the docstring of test_more_kernels_gpu.py
C_W = {5: 8, 6: 17, 7: 13, 8: 21, 9: 20}
C_DW = {5: 5, 6: 15, 7: 11, 8: 19, 9: 17}
C_DWQ = {5: 4, 6: 14, 7: 10, 8: 18, 9: 16}


def mp_kernel(kk, q, dim):
    """(W(q), dW/dq(q)) without the normalisation from the formulas, branch conditions and operation order of the
    reference's pysph/base/kernels.py (WendlandQuinticC2_1D :208-233, C4_1D :427-452, C4 :536-563, C6_1D :650-677,
    C6 :761-788, SuperGaussian :986-1010) at mpmath's working precision -- see helpers.mp_kernel for why the order
    matters at 53 bits.  The rij > 1e-12 guard of dwdq belongs to the caller."""
    import mpmath as mp
    q = mp.mpf(q)
    f = mp.mpf
    if kk == 10:
        if q < 3:
            q2 = q * q
            return mp.exp(-q2) * (f(1) + dim * f(0.5) - q2), q * (f(2) * q2 - dim - 4) * mp.exp(-q2)
        return f(0), f(0)
    tmp = 1 - f(0.5) * q
    if not q < 2:
        return f(0), f(0)
    if kk == 5:
        return tmp * tmp * tmp * (f(1.5) * q + 1), f(-3) * q * tmp * tmp
    if kk == 7:
        return (tmp * tmp * tmp * tmp * tmp * (2 * q * q + f(2.5) * q + 1),
                f(-3.5) * q * (2 * q + 1) * tmp * tmp * tmp * tmp)
    if kk == 6:
        return (tmp * tmp * tmp * tmp * tmp * tmp * ((f(35) / f(12)) * q * q + f(3) * q + 1),
                (f(-14) / f(3)) * q * (1 + f(2.5) * q) * tmp * tmp * tmp * tmp * tmp)
    if kk == 9:
        return (tmp * tmp * tmp * tmp * tmp * tmp * tmp * (f(2.625) * q * q * q + f(4.75) * q * q + f(3.5) * q + 1),
                f(-0.5) * q * (f(26.25) * q * q + 27 * q + 9) * tmp * tmp * tmp * tmp * tmp * tmp)
    if kk == 8:
        return (tmp * tmp * tmp * tmp * tmp * tmp * tmp * tmp * (f(4) * q * q * q + f(6.25) * q * q + f(4) * q + 1),
                f(-5.5) * q * tmp * tmp * tmp * tmp * tmp * tmp * tmp * (1 + f(3.5) * q + 4 * q * q))
    raise KeyError(kk)


def mp_kernel_all(kk, r, h, sigma, dim, xij):
    """the reference's kernel, dwdq, gradient and gradient_h of (xij, rij, h), operation by operation (h1 = 1 / h and
    q = rij * h1 in the inputs' own arithmetic: the reference's definition of q)"""
    import mpmath as mp
    f = mp.mpf
    h1 = type(r)(1) / h
    q = r * h1
    w, dw = mp_kernel(kk, q, dim)
    fac = f(float(sigma))
    for _ in range(dim):
        fac = fac * f(h1)
    if kk == 10:     # :1044-1047, its own closed form
        val = f(0)
        if q < 3:
            q2 = f(q) * f(q)
            val = (-dim * dim * f(0.5) + f(2) * dim * q2 - dim - f(2) * q2 * q2 + 4 * q2) * mp.exp(-q2)
        gh = -fac * f(h1) * val
    else:
        gh = -fac * f(h1) * (dw * f(q) + w * dim)
    if not r > 1e-12:
        dw = f(0)
    w, dw = w * fac, dw * fac
    tmp = dw * f(h1) / f(r) if r > 1e-12 else f(0)
    return w, dw, [tmp * f(float(c)) for c in xij], gh


def _poly(c, q):
    return sum(a * q ** i for i, a in enumerate(c))


def _dpoly(c, q):
    return sum(i * a * q ** (i - 1) for i, a in enumerate(c) if i)


def term_sums(kk, q, dim):
    """S for w, dw, dwq: the absolute values of the terms as the device writes them (one product for the Wendlands;
    for the SuperGaussian the polynomial factor's |terms|, without exp)"""
    q = np.asarray(q, dtype=np.float64)
    if kk == 10:
        ins = q < 3
        return ins * (1 + 0.5 * dim + q * q), ins * q * (2 * q * q + dim + 4), ins * (2 * q * q + dim + 4)
    s = WENDLAND[kk]
    t, ins, c, n = np.abs(1 - 0.5 * q), q < 2, abs(s['c']), s['n']
    return ins * t ** n * _poly(s['P'], q), ins * c * q * _poly(s['D'], q) * t ** (n - 1), ins * c * _poly(s['D'], q) * t ** (n - 1)


def slope_sums(kk, q, dim):
    """sum of the absolute values of the terms of d/dq of w, dw, dwq (exp included for the SuperGaussian), as
    test_device_functions.slope_sums"""
    q = np.asarray(q, dtype=np.float64)
    if kk == 10:
        e = np.where(q < 3, np.exp(-q * q), 0.0)
        a, b = 1 + 0.5 * dim, dim + 4.0
        return (2 * q * e * (a + q * q) + 2 * q * e, (2 * q * q + b) * e + 4 * q * q * e + 2 * q * q * (2 * q * q + b) * e,
                4 * q * e + 2 * q * (2 * q * q + b) * e)
    s = WENDLAND[kk]
    t, ins, c, n = np.abs(1 - 0.5 * q), q < 2, abs(s['c']), s['n']
    P, dP, D, dD = _poly(s['P'], q), _dpoly(s['P'], q), _poly(s['D'], q), _dpoly(s['D'], q)
    tn1 = t ** (n - 1)
    tn2 = t ** (n - 2)
    return (ins * (0.5 * n * tn1 * P + t ** n * dP),
            ins * c * (D * tn1 + q * dD * tn1 + q * D * 0.5 * (n - 1) * tn2),
            ins * c * (dD * tn1 + D * 0.5 * (n - 1) * tn2))


# ---------------------------------------------------------------------------
# the probe library: built like helpers.build_probe_library, from its own source
# ---------------------------------------------------------------------------
def _probe_command(out):
    cmd = H._probe_command(out)
    return [PROBE_SRC if c == H.PROBE_SRC else c for c in cmd]


def probe_library_path():
    import hashlib
    import sys
    sys.path.insert(0, os.path.join(H._REPO, 'pysph_amd', 'csrc'))
    import srchash
    from pysph_amd import codegen
    h = hashlib.sha256()
    with open(PROBE_SRC, 'rb') as f:
        h.update(f.read())
    h.update(srchash.source_hash().encode())
    h.update(' '.join(_probe_command('')[1:]).encode())
    return os.path.join(codegen.GEN_DIR, 'probe_device_functions_more_%s.so' % h.hexdigest()[:16])


def build_probe_library():
    """next to the generated families' shared objects (so that it travels with the tree); compiled here when it is
    missing.  No hipcc and no library is an error, not a skip."""
    import shutil
    import subprocess
    so = probe_library_path()
    if os.path.exists(so):
        return so
    cmd = _probe_command(so + '.tmp%d' % os.getpid())
    if not (os.path.isfile(cmd[0]) or shutil.which(cmd[0])):
        raise RuntimeError('%s is missing and there is no hipcc (%s) to build it' % (so, cmd[0]))
    os.makedirs(os.path.dirname(so), exist_ok=True)
    subprocess.check_call(cmd)
    os.replace(cmd[-1], so)
    return so


_PROBE = []


def probe_library():
    import ctypes as C
    if not _PROBE:
        lib = C.CDLL(build_probe_library())
        vp, i, d = C.c_void_p, C.c_int, C.c_double
        lib.probe_more_kernel.argtypes = [i, i, i, i, i, vp, vp, vp, vp]
        lib.probe_more_pair.argtypes = [i, i, i, i, vp, vp, vp, d, i, d, d, d, d, vp]
        _PROBE.append(lib)
    return _PROBE[0]


def probe_kernel(kk, insup, q, dim):
    """device SphKernel<kk>::w/dw/dwq<insup>(q, dim); the dtype of q selects the arithmetic"""
    q = np.ascontiguousarray(q)
    out = [np.empty_like(q) for _ in range(3)]
    rc = probe_library().probe_more_kernel(kk, int(insup), int(q.dtype == np.float32), q.size, int(dim), H._vp(q),
                                           *map(H._vp, out))
    assert rc == 0, 'probe_more_kernel: HIP error %d' % rc
    return out


def probe_pair(kk, uh, r2, hi, hj, sigma, dim, uniform=(0.0, 0.0, 0.0, 0.0)):
    """device pair_geom<kk, uh> + pair_w / pair_gradfac / pair_gradh; dict of the helpers.PAIR_OUT arrays"""
    r2 = np.ascontiguousarray(r2)
    hi = np.ascontiguousarray(hi, dtype=r2.dtype)
    hj = np.ascontiguousarray(hj, dtype=r2.dtype)
    assert hi.size == r2.size and hj.size == r2.size
    out = np.empty((len(H.PAIR_OUT), r2.size), dtype=r2.dtype)
    rc = probe_library().probe_more_pair(kk, int(uh), int(r2.dtype == np.float32), r2.size, H._vp(r2), H._vp(hi),
                                         H._vp(hj), float(sigma), int(dim), *[float(u) for u in uniform], H._vp(out))
    assert rc == 0, 'probe_more_pair: HIP error %d' % rc
    return dict(zip(H.PAIR_OUT, out))


# ---------------------------------------------------------------------------
# the golden cases of tests/golden/make_more_kernels_golden.py
# ---------------------------------------------------------------------------
GOLDEN_CASES = ['more_wcsph_c4_varh', 'more_wcsph_c6', 'more_tvf2d_sg', 'more_tvf2d_sg_varh',
                'more_sd1d_WendlandQuinticC2_1D', 'more_sd1d_WendlandQuinticC4_1D', 'more_sd1d_WendlandQuinticC6_1D',
                'more_sd1d_SuperGaussian', 'more_elastic2d_c6']


def golden_case(name, g):
    """(equations, kernel, dim, output props) matching make_more_kernels_golden.py"""
    from pysph_amd.equations import Group, SummationDensity
    from pysph_amd.scheme import WCSPHScheme, TVFScheme
    if name.startswith('more_wcsph'):
        dx = float(g['meta/dx'])
        s = WCSPHScheme(['fluid'], [], dim=3, rho0=1000.0, c0=10.0, h0=1.2 * dx, hdx=1.2, gx=0.5, gy=-0.25, gz=-9.81,
                        alpha=1.0, beta=1.0, gamma=7.0, tensile_correction=True, summation_density=True)
        kernel = K.WendlandQuinticC4(dim=3) if 'c4' in name else K.WendlandQuinticC6(dim=3)
        return s.get_equations(), kernel, 3, H.WC_OUT
    if name.startswith('more_tvf2d'):
        dx = float(g['meta/dx'])
        s = TVFScheme(['fluid'], [], dim=2, rho0=1.0, c0=10.0, nu=0.01, p0=100.0, pb=100.0, h0=dx, gx=0.1, alpha=0.2)
        return s.get_equations(), K.SuperGaussian(dim=2), 2, H.TVF_OUT
    if name.startswith('more_sd1d_'):
        eqs = [Group(equations=[SummationDensity(dest='fluid', sources=['fluid'])])]
        return eqs, getattr(K, name[len('more_sd1d_'):])(dim=1), 1, ['rho']
    if name == 'more_elastic2d_c6':
        from pysph_amd.solid_mech import ElasticSolidsScheme
        s = ElasticSolidsScheme(['solid'], [], dim=2)
        return s.get_equations(), K.WendlandQuinticC6(dim=2), 2, H.EL_OUT
    raise KeyError(name)
