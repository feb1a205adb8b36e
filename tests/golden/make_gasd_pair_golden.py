#!/usr/bin/env python
"""The five gas-dynamics pair sweeps, cluster by cluster, from the REFERENCE's own classes -- ``SummationDensity``,
``MPMAccelerations``, ``SummationDensityADKE`` (with its ``reduce``), ``ADKEAccelerations`` (gas_dynamics/basic.py) and
``WallBoundary`` (boundary_equations.py) -- executed as plain Python, in the manner of make_gsph_riemann_golden.py:

    python tests/golden/make_gasd_pair_golden.py          ->  gasd_pair_edges.npz

Layout.  Every table is a row of isolated clusters along x, 1 apart (2^-24 apart in the scaled table of the fallback);
every h is in [2^-4, 2^-2] and a cluster is less than 1/4 across, so a particle's neighbours are its own cluster and
nothing else, also under Gaussian (radius 3).  Clusters are pairs (both orders: each particle is a destination), triples
(one destination between two sources) and, for the wall, one wall row with one or two fluid rows.  Every table exists
in 1-D under CubicSpline and Gaussian, in 2-D under CubicSpline and in 3-D under QuinticSpline, the partner offset
along (1, 0, 0), (3/4, -1/2, 0) and (1/2, -3/4, 1/4).  Every input is a dyadic number or a fixed-seed double.

A table runs ONE equation alone, one sweep: ``initialize`` over the destinations, ``loop`` over every destination and
its neighbours (the reference's criterion, r^2 < (radius h_i)^2 or r^2 < (radius h_j)^2 at the h of entry), ``post_loop``,
and for SummationDensityADKE its ``reduce``.  XIJ VIJ R2IJ RIJ HIJ EPS RHOIJ RHOIJ1 WIJ WI WJ DWIJ DWI DWJ GHI are formed
as pysph/sph/equation.py:185-300 forms them, the kernels by the reference's kernel classes.  A table runs twice:

    ref/<column>   in double, with ``sig``, the lines of ``loop`` (per source) and ``post_loop`` each destination ran
    mp/<column>    at 50 digits (mpmath; ``sqrt``, ``log``, ``exp`` of the module rebound, the kernels from
                   tests/helpers.mp_kernel with the reference's gradient and gradient_h lines around them), as a double
                   and a remainder per value; ``mpok`` where that run took the lines of the double run
    S/<column>     the scale of every element, kref/<column> = |double - 50 digits| / (u S), u = 2^-53

Scale.  A column the loop accumulates (``+=``, ``-=``): S = the sum over the cluster of |new - old| of every statement
that writes it, recorded at 50 digits by the list type the columns live in.  ``dt_cfl``, a running maximum, takes
|cij| + |beta| sum_k |VIJ_k XIJ_k| of the pair that set it.  A column ``post_loop`` (or ``reduce``) derives runs through
the reference's OWN post_loop on values that carry their scale, with first-order propagation plus the formula's own terms:

    a +- b : s_a + s_b + |a| + |b|          a b : s_a |b| + s_b |a| + |a b|         a / b : s_a / |b| + s_b |a| / b^2 + |a / b|
    a ^ p  : |p| s_a |a^p / a| + |a^p|      sqrt a : s_a / (2 sqrt a) + sqrt a      log a : s_a / |a| + |log a|
    exp a  : s_a exp a + exp a              sum of a list: sum s_i + sum |a_i|      an input or a constant: 0

so that, column by column (sums in capitals, their scales S_X):
    div     = -ARHO / RHO                              (all three density sweeps; ARHO omega where the row converged now)
    omega   = 1 / (1 + h DWDH / (dim RHO))
    h (SD)  = h - (m (k / h)^dim - RHO) / (omegai / dhdrho), or 1.2 h, 0.8 h (scale |1.2 h|), or k (m / RHO)^(1 / dim)
    arho    = ARHO omega, ah = arho dhdrho             (a row that converges in this sweep)
    logrho  = log RHO;  h (ADKE) = k (exp(sum logrho / n) / RHO)^eps h0
    aalpha1 = (alpha1_min - alpha1) / (h / (sigma cs)) + max(-div, 0)
    aalpha2 = (alpha2_min - alpha2) / tau + 0.01 h |DEL2E| / sqrt e
    wall    : Q / WIJ for the nine averaged columns, HTMP / WIJ for h
An element of scale 0 must be exact.

Conditions asserted here on the reference alone (tests/test_gasd_pair_edges.py asserts them again on the file):
  1. every branch of REQUIRED is taken at least twice over the main tables;
  2. no threshold decision within a relative 1e-3 of its threshold (diff against htol, hnew against 1.2 h, 0.8 h and
     1e-6, RIJ against 1e-8, wij against 1e-30 -- the two constructed wall rows a factor 8 -- |omegai| against 0, dot and
     XIJ.VIJ against 0 relative to |VIJ| (|XIJ| |VIJ|), div against 0); a value that is exactly zero by construction is
     exempt: both sides write the same there;
  3. every REQUIRED branch is observable: the method with that one comparison inverted (its source text patched in
     memory, MUTANTS below) leaves the bound of item 5 in at least two destinations that took the branch.  A mutant that
     raises where the reference does not (a division by RIJ = 0 or by wij = 0) counts as leaving it: the compiled
     reference writes no number there.  ``coincident_pair_unequal_h`` shares its comparison with ``rij_below_1e-8``;
     ``dt_cfl_*`` and the signs of ``div`` are choices of ``max`` and ``abs``, inverted as ``min`` and ``abs(.) + .``.
     Unobservable and therefore not REQUIRED: ``fallback_gradh`` (gradhi < 1e-6 needs omegai > 1e6) -- not built;
  4. per equation at most one destination in ten has K_ref > 64 in a column or another path at 50 digits;
  5. K_eq = the largest K_ref over the well-conditioned elements of an equation (K_ref <= 64, same path at 50 digits;
     meta/k_eq); a well-conditioned element is held to max(4, 4 K_eq) u S, any other to 4 K_ref of itself;
  6. the reference with beta (1 + 1e-13) (MPM, ADKE), k (1 + 1e-13) (both density sweeps) and the fluid's columns scaled
     by (1 + 1e-13) (wall) leaves that bound in at least one well-conditioned element per equation.
A state on which the reference raises is dropped and named under meta/dropped.
"""
import inspect
import json
import math
import os
import sys
import textwrap
from collections import Counter

import numpy as np
import mpmath as mp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as MG  # noqa: E402,F401  (sets up the reference imports)
import make_gasd_golden as GG  # noqa: E402,F401  (its module stubs)
import make_adke_golden as MA  # noqa: E402,F401  (the reduce helpers of gas_dynamics.basic)
import helpers as H  # noqa: E402  (mp_kernel)

from pysph.sph.gas_dynamics import basic as RB  # noqa: E402
from pysph.sph.gas_dynamics import boundary_equations as RW  # noqa: E402
from pysph.base import kernels as RK  # noqa: E402

OUT = os.path.join(HERE, 'gasd_pair_edges.npz')
U = 2.0 ** -53
WELL = 64.0
FACTOR = 4.0
MARGIN = 1e-3
CONFIGS = (('1d_cubic', 1, 'CubicSpline'), ('1d_gauss', 1, 'Gaussian'), ('2d_cubic', 2, 'CubicSpline'),
           ('3d_quintic', 3, 'QuinticSpline'))
KERNEL_IDS = {'CubicSpline': 1, 'QuinticSpline': 3, 'Gaussian': 4}
DIRS = {1: (1.0, 0.0, 0.0), 2: (0.75, -0.5, 0.0), 3: (0.5, -0.75, 0.25)}
EQUATIONS = ('SummationDensity', 'MPMAccelerations', 'SummationDensityADKE', 'ADKEAccelerations', 'WallBoundary')
CLASSES = {'SummationDensity': RB.SummationDensity, 'MPMAccelerations': RB.MPMAccelerations,
           'SummationDensityADKE': RB.SummationDensityADKE, 'ADKEAccelerations': RB.ADKEAccelerations,
           'WallBoundary': RW.WallBoundary}
OUTPUTS = {
    'SummationDensity': ('rho', 'arho', 'grhox', 'grhoy', 'grhoz', 'dwdh', 'div', 'omega', 'ah', 'h', 'converged'),
    'MPMAccelerations': ('au', 'av', 'aw', 'ae', 'del2e', 'dt_cfl', 'aalpha1', 'aalpha2'),
    'SummationDensityADKE': ('rho', 'arho', 'div', 'logrho', 'h'),
    'ADKEAccelerations': ('au', 'av', 'aw', 'ae'),
    'WallBoundary': ('p', 'u', 'v', 'w', 'm', 'rho', 'e', 'cs', 'div', 'wij', 'h', 'htmp'),
}
# columns a sweep may leave as they came (the branch decides): they start as chosen inputs, every other output as garbage
KEPT = {'SummationDensity': ('omega', 'ah', 'h', 'converged'), 'SummationDensityADKE': ('h',), 'WallBoundary': ('h',)}
REQUIRED = (
    'clamp_up', 'clamp_down', 'no_clamp', 'fallback_small_h', 'omega_reset', 'converged_now', 'not_converged',
    'already_converged', 'once', 'density_iterations_false',
    'approaching', 'receding', 'rij_below_1e-8', 'rij_above_1e-8', 'coincident_pair_unequal_h', 'dt_cfl_from_partner',
    'dt_cfl_from_self', 'dt_cfl_stays_zero', 'update_alpha1_div_negative', 'update_alpha1_div_positive', 'update_alpha2',
    'adke_approaching', 'adke_receding', 'adke_div_pp', 'adke_div_pn', 'adke_div_np', 'adke_div_nn',
    'reached', 'reached_tiny', 'below_threshold', 'not_reached')
# branch -> (method, text of the reference's line, replacement): the comparison inverted
MUTANTS = {
    'clamp_up': ('post_loop', '(hnew > 1.2 * hi)', '(hnew <= 1.2 * hi)'),
    'no_clamp': ('post_loop', '(hnew > 1.2 * hi)', '(hnew <= 1.2 * hi)'),
    'clamp_down': ('post_loop', '(hnew < 0.8 * hi)', '(hnew >= 0.8 * hi)'),
    'fallback_small_h': ('post_loop', '(hnew <= 1e-6)', '(hnew > 1e-6)'),
    'omega_reset': ('post_loop', 'if omegai < 0:', 'if omegai >= 0:'),
    'converged_now': ('post_loop', '(diff < self.htol)', '(diff >= self.htol)'),
    'not_converged': ('post_loop', '(diff < self.htol)', '(diff >= self.htol)'),
    'already_converged': ('post_loop', 'if not (d_converged[d_idx] == 1):', 'if (d_converged[d_idx] == 1):'),
    'once': ('post_loop', 'self.iterate_only_once):', '(not self.iterate_only_once)):'),
    'density_iterations_false': ('post_loop', 'if self.density_iterations:', 'if not self.density_iterations:'),
    'approaching': ('loop', 'if dot <= 0.0:', 'if dot > 0.0:'),
    'receding': ('loop', 'if dot <= 0.0:', 'if dot > 0.0:'),
    'rij_below_1e-8': ('loop', 'if RIJ < 1e-8:', 'if RIJ >= 1e-8:'),
    'rij_above_1e-8': ('loop', 'if RIJ < 1e-8:', 'if RIJ >= 1e-8:'),
    'coincident_pair_unequal_h': ('loop', 'if RIJ < 1e-8:', 'if RIJ >= 1e-8:'),
    'dt_cfl_from_partner': ('loop', 'd_dt_cfl[d_idx] = max(', 'd_dt_cfl[d_idx] = min('),
    'dt_cfl_from_self': ('loop', 'd_dt_cfl[d_idx] = max(', 'd_dt_cfl[d_idx] = min('),
    'dt_cfl_stays_zero': ('loop', 'd_dt_cfl[d_idx] = max(', 'd_dt_cfl[d_idx] = min('),
    'update_alpha1_div_negative': ('post_loop', 'S1 = max(', 'S1 = min('),
    'update_alpha1_div_positive': ('post_loop', 'S1 = max(', 'S1 = min('),
    'update_alpha2': ('post_loop', 'if self.update_alpha2:', 'if not self.update_alpha2:'),
    'adke_approaching': ('loop', 'if xijdotvij < 0:', 'if xijdotvij >= 0:'),
    'adke_receding': ('loop', 'if xijdotvij < 0:', 'if xijdotvij >= 0:'),
    'adke_div_pp': ('loop', '(abs(divi)-divi)', '(abs(divi)+divi)'),
    'adke_div_pn': ('loop', '(abs(divj)-divj)', '(abs(divj)+divj)'),
    'adke_div_np': ('loop', '(abs(divi)-divi)', '(abs(divi)+divi)'),
    'adke_div_nn': ('loop', '(abs(divj)-divj)', '(abs(divj)+divj)'),
    'reached': ('post_loop', 'if (d_wij[d_idx]>1e-30):', 'if (d_wij[d_idx]<=1e-30):'),
    'reached_tiny': ('post_loop', 'if (d_wij[d_idx]>1e-30):', 'if (d_wij[d_idx]<=1e-30):'),
    'below_threshold': ('post_loop', 'if (d_wij[d_idx]>1e-30):', 'if (d_wij[d_idx]<=1e-30):'),
    'not_reached': ('post_loop', 'if (d_wij[d_idx]>1e-30):', 'if (d_wij[d_idx]<=1e-30):'),
}
BRANCH_EQUATION = dict((b, 'SummationDensity') for b in REQUIRED[:10])
BRANCH_EQUATION.update((b, 'MPMAccelerations') for b in REQUIRED[10:21])
BRANCH_EQUATION.update((b, 'ADKEAccelerations') for b in REQUIRED[21:27])
BRANCH_EQUATION.update((b, 'WallBoundary') for b in REQUIRED[27:])


# -- values that carry their scale ---------------------------------------------------------------------------------------
class VS(object):
    """a 50-digit value and the scale of its rounding error (the rules of the docstring); compares as its value"""
    __slots__ = ('v', 's')

    def __init__(self, v, s=0):
        self.v, self.s = mp.mpf(v), mp.mpf(s)

    @staticmethod
    def of(o):
        if isinstance(o, VS):
            return o
        if isinstance(o, (int, float, mp.mpf, np.floating, np.integer)):
            return VS(o, 0)
        return None

    def _bin(self, o, fn):
        o = VS.of(o)
        return NotImplemented if o is None else fn(self, o)

    def __add__(self, o):
        return self._bin(o, lambda a, b: VS(a.v + b.v, a.s + b.s + abs(a.v) + abs(b.v)))
    __radd__ = __add__

    def __sub__(self, o):
        return self._bin(o, lambda a, b: VS(a.v - b.v, a.s + b.s + abs(a.v) + abs(b.v)))

    def __rsub__(self, o):
        return self._bin(o, lambda a, b: VS(b.v - a.v, a.s + b.s + abs(a.v) + abs(b.v)))

    def __mul__(self, o):
        return self._bin(o, lambda a, b: VS(a.v * b.v, a.s * abs(b.v) + b.s * abs(a.v) + abs(a.v * b.v)))
    __rmul__ = __mul__

    def __truediv__(self, o):
        return self._bin(o, lambda a, b: VS(a.v / b.v, a.s / abs(b.v) + b.s * abs(a.v) / (b.v * b.v) + abs(a.v / b.v)))

    def __rtruediv__(self, o):
        return self._bin(o, lambda a, b: VS(b.v / a.v, b.s / abs(a.v) + a.s * abs(b.v) / (a.v * a.v) + abs(b.v / a.v)))

    def __pow__(self, p):
        r = mp.power(self.v, p)
        return VS(r, abs(p) * self.s * abs(r / self.v) + abs(r))

    def __neg__(self):
        return VS(-self.v, self.s)

    def __abs__(self):
        return VS(abs(self.v), self.s)

    def __float__(self):
        return float(self.v)

    def __lt__(self, o):
        return self.v < VS.of(o).v

    def __le__(self, o):
        return self.v <= VS.of(o).v

    def __gt__(self, o):
        return self.v > VS.of(o).v

    def __ge__(self, o):
        return self.v >= VS.of(o).v

    def __eq__(self, o):
        return self.v == VS.of(o).v

    def __ne__(self, o):
        return self.v != VS.of(o).v
    __hash__ = None


def _vs_sqrt(x):
    if isinstance(x, VS):
        r = mp.sqrt(x.v)
        return VS(r, x.s / (2 * r) + r)
    return mp.sqrt(x)


def _vs_log(x):
    if isinstance(x, VS):
        r = mp.log(x.v)
        return VS(r, x.s / abs(x.v) + abs(r))
    return mp.log(x)


def _vs_exp(x):
    if isinstance(x, VS):
        r = mp.exp(x.v)
        return VS(r, x.s * r + r)
    return mp.exp(x)


def _vs_sum(arr, op='sum'):
    vals = [VS.of(a) for a in arr]
    return VS(sum(a.v for a in vals), sum(a.s + abs(a.v) for a in vals))


class RecList(list):
    """a column; while ``rec`` is a list, every write adds |new - old| to it"""
    rec = None

    def __setitem__(self, i, v):
        if self.rec is not None:
            self.rec[i] += abs(v - self[i])
        list.__setitem__(self, i, v)


# -- the two arithmetics -------------------------------------------------------------------------------------------------
class Double(object):
    name = 'double'
    conv = float

    def __init__(self, kname, dim):
        self.k = getattr(RK, kname)(dim=dim)

    def kern(self, xij, rij, h):
        grad = [0.0, 0.0, 0.0]
        self.k.gradient(xij, rij, h, grad)
        return self.k.kernel(xij, rij, h), grad, self.k.gradient_h(xij, rij, h)

    sqrt = staticmethod(math.sqrt)

    def bind(self):
        RB.sqrt, RB.log, RB.exp = math.sqrt, math.log, math.exp
        RB.serial_reduce_array = lambda arr, op='sum': np.sum(arr)


class Digits50(object):
    name = 'mp'
    conv = mp.mpf

    def __init__(self, kname, dim):
        self.kk, self.dim = KERNEL_IDS[kname], dim
        self.fac0 = mp.mpf(getattr(RK, kname)(dim=dim).fac)       # the double constant is the definition

    def kern(self, xij, rij, h):
        """kernel, gradient and gradient_h as the reference writes them (kernels.py:69-163 and alike)"""
        h1 = 1 / h
        q = rij * h1
        w, dw = H.mp_kernel(self.kk, q)
        fac = self.fac0
        for _ in range(self.dim):
            fac = fac * h1
        gh = -fac * h1 * (dw * q + w * self.dim)
        tmp = dw * fac * h1 / rij if rij > 1e-12 else mp.mpf(0)
        return w * fac, [tmp * c for c in xij], gh

    sqrt = staticmethod(mp.sqrt)

    def bind(self):
        RB.sqrt, RB.log, RB.exp = _vs_sqrt, _vs_log, _vs_exp
        RB.serial_reduce_array = _vs_sum


def unbind():
    Double.bind(None)


# -- the sweep -----------------------------------------------------------------------------------------------------------
_SPEC = {}


def _args(fn):
    code = fn.__code__
    if code not in _SPEC:
        _SPEC[code] = [a for a in inspect.getfullargspec(fn).args if a != 'self']
    return _SPEC[code]


class CallTrace(object):
    """the lines (relative to the ``def``) one call ran and its locals on return"""

    def __init__(self, code):
        self.code, self.lines, self.locals = code, set(), {}

    def __call__(self, frame, event, arg):
        return self.local if frame.f_code is self.code else None

    def local(self, frame, event, arg):
        if event == 'line':
            self.lines.add(frame.f_lineno - self.code.co_firstlineno)
        elif event == 'return':
            self.locals = dict((k, (list(v) if isinstance(v, list) and not isinstance(v, RecList) else v))
                               for k, v in frame.f_locals.items()
                               if isinstance(v, (int, float, mp.mpf, VS)) or (isinstance(v, list) and len(v) == 3))
        return self.local


def traced_call(fn, args):
    tr = CallTrace(fn.__code__)
    sys.settrace(tr)
    try:
        fn(*args)
    finally:
        sys.settrace(None)
    return tr


def neighbours(table):
    """per (destination array, source array): the lists of the reference's criterion at the h of entry, in double; every
    list is asserted to lie inside the destination's cluster"""
    rs = {'CubicSpline': 2.0, 'Gaussian': 3.0, 'QuinticSpline': 3.0}[table['kernel']]
    out = {}
    A = table['arrays']
    for dn in A:
        for sn in A:
            D, S = A[dn], A[sn]
            lists = []
            for i in range(len(D['x'])):
                d2 = sum((D[c][i] - S[c]) ** 2 for c in 'xyz')
                hit = (d2 < (rs * D['h'][i]) ** 2) | (d2 < (rs * S['h']) ** 2)
                assert np.all(S['cl'][hit] == D['cl'][i]), (table['key'], dn, sn, i, 'a neighbour outside the cluster')
                lists.append([int(j) for j in np.nonzero(hit)[0]])
            out[(dn, sn)] = lists
    return out


def sweep(table, N, cls=None, params=None, scale_cols=None):
    """one equation over one table in the arithmetic N.  Returns a dict: cols (destination columns after the sweep),
    S (scales, 50 digits only), recs (per destination: the CallTraces of its loop calls and its post_loop), flag"""
    eqname = table['equation']
    cls = cls or CLASSES[eqname]
    par = dict(table['params'], **(params or {}))
    dest, sources = table['dest'], table['sources']
    eq = cls(dest=dest, sources=list(sources), **par)
    N.bind()
    try:
        A = {}
        for name, cols in table['arrays'].items():
            A[name] = dict((c, RecList(N.conv(float(x)) * (scale_cols.get((name, c), 1) if scale_cols else 1) for x in v))
                           for c, v in cols.items() if c != 'cl')
        D = A[dest]
        n = len(D['x'])
        nb = table['nbrs']
        mpmode = N.name == 'mp'
        S = dict((c, [mp.mpf(0)] * n) for c in OUTPUTS[eqname]) if mpmode else None
        recs = [dict(loop=[], post=None) for _ in range(n)]

        def call(meth, i, extra=None, sn=None, j=None, trace=False):
            fn = getattr(eq, meth, None)
            if fn is None:
                return None
            ns = dict(d_idx=i, s_idx=j, t=0.0, dt=0.0)
            ns.update(extra or {})
            args = []
            for a in _args(fn):
                if a[:2] == 'd_' and a != 'd_idx':
                    args.append(D[a[2:]])
                elif a[:2] == 's_' and a != 's_idx':
                    args.append(A[sn][a[2:]])
                else:
                    args.append(ns[a])
            if trace:
                return traced_call(fn, args)
            fn(*args)
            return None

        for i in range(n):
            call('initialize', i)
        if hasattr(eq, 'loop'):
            need = set(_args(eq.loop))
            if mpmode:
                for c in S:
                    D[c].rec = S[c]
            for sn in sources:
                Sa = A[sn]
                for i in range(n):
                    for j in nb[(dest, sn)][i]:
                        sym = symbols(need, N, D, Sa, i, j)
                        old = D['dt_cfl'][i] if eqname == 'MPMAccelerations' else None
                        recs[i]['loop'].append((sn, j, call('loop', i, sym, sn, j, trace=True)))
                        if mpmode and old is not None and D['dt_cfl'][i] != old:
                            cij = (D['cs'][i] + Sa['cs'][j]) / 2
                            S['dt_cfl'][i] = abs(cij) + abs(eq.beta) * sum(abs(a * b) for a, b in zip(sym['VIJ'], sym['XIJ']))
            for c in D:
                D[c].rec = None
        if mpmode:          # every column of the destination carries a scale from here on: 0 for an input
            for c in D:
                for i in range(n):
                    D[c][i] = VS(D[c][i], S[c][i] if c in S else 0)
        for i in range(n):
            recs[i]['post'] = call('post_loop', i, trace=True)
        if hasattr(eq, 'reduce'):
            view = type('View', (object,), {})()
            for c in ('x', 'logrho', 'rho', 'h0', 'h'):
                setattr(view, c, np.array(list(D[c]), dtype=(object if mpmode else float)))
            eq.reduce(view, 0.0, 0.0)
            D['h'] = RecList(view.h)
        cols = {}
        for c in OUTPUTS[eqname]:
            vals = [VS.of(x) if mpmode else float(x) for x in D[c]]
            if mpmode:
                cols[c] = [x.v for x in vals]
                S[c] = [mp.mpf(float(np.float32(float(x.s)))) for x in vals]      # (stored as float32: a scale needs no more)
            else:
                cols[c] = np.array(vals, dtype=np.float64)
        inputs_same = all(all(float(a) == float(b) for a, b in zip(A[name][c], table['arrays'][name][c]))
                          for name in A for c in A[name] if not (name == dest and c in OUTPUTS[eqname])) if not scale_cols else True
        assert inputs_same, 'the reference wrote an input column'
        flag = eq.converged() if hasattr(eq, 'converged') else 1
        return dict(cols=cols, S=S, recs=recs, flag=flag, eq=eq)
    finally:
        unbind()


def symbols(need, N, D, S, i, j):
    """equation.py:185-300, in the arithmetic of the columns"""
    o = {}
    XIJ = [D[c][i] - S[c][j] for c in 'xyz']
    o['XIJ'] = XIJ
    o['VIJ'] = [D[c][i] - S[c][j] for c in 'uvw']
    R2IJ = XIJ[0] * XIJ[0] + XIJ[1] * XIJ[1] + XIJ[2] * XIJ[2]
    RIJ = N.sqrt(R2IJ)
    o['R2IJ'], o['RIJ'] = R2IJ, RIJ
    HIJ = 0.5 * (D['h'][i] + S['h'][j])
    o['HIJ'] = HIJ
    o['EPS'] = 0.01 * HIJ * HIJ
    if 'RHOIJ' in need or 'RHOIJ1' in need:
        o['RHOIJ'] = 0.5 * (D['rho'][i] + S['rho'][j])
        o['RHOIJ1'] = 1.0 / o['RHOIJ']
    if 'WIJ' in need or 'DWIJ' in need:
        o['WIJ'], o['DWIJ'], _ = N.kern(XIJ, RIJ, HIJ)
    if 'WI' in need or 'DWI' in need or 'GHI' in need:
        o['WI'], o['DWI'], o['GHI'] = N.kern(XIJ, RIJ, D['h'][i])
    if 'WJ' in need or 'DWJ' in need:
        o['WJ'], o['DWJ'], _ = N.kern(XIJ, RIJ, S['h'][j])
    return o


# -- branches and margins ------------------------------------------------------------------------------------------------
def _rel(fn, text, nth=0):
    src = inspect.getsourcelines(fn)[0]
    hits = [k for k, ln in enumerate(src) if text in ln]
    assert len(hits) > nth, (fn.__name__, text)
    return hits[nth]


_SD, _MPM, _ADKE, _WALL = RB.SummationDensity, RB.MPMAccelerations, RB.ADKEAccelerations, RW.WallBoundary
LINES = {
    'sd_block': _rel(_SD.post_loop, 'mi = d_m[d_idx]'),
    'sd_iter': _rel(_SD.post_loop, 'if not (d_converged[d_idx] == 1)'),
    'sd_up': _rel(_SD.post_loop, 'hnew = 1.2 * hi'),
    'sd_down': _rel(_SD.post_loop, 'hnew = 0.8 * hi'),
    'sd_fallback': _rel(_SD.post_loop, 'hnew = self.k * (mi/d_rho'),
    'sd_reset': _rel(_SD.post_loop, 'omegai = 1.0', 1),
    'sd_not': _rel(_SD.post_loop, 'd_converged[d_idx] = 0'),
    'sd_now': _rel(_SD.post_loop, 'd_converged[d_idx] = 1'),
    'mpm_zero': _rel(_MPM.loop, 'XIJ[0] = 0.0'),
    'mpm_norm': _rel(_MPM.loop, 'XIJ[0] /= RIJ'),
    'mpm_visc': _rel(_MPM.loop, 'alpha1 = 0.5 * (d_alpha1'),
    'mpm_a1': _rel(_MPM.post_loop, 'S1 = max('),
    'mpm_a2': _rel(_MPM.post_loop, 'S2 = 0.01'),
    'adke_visc': _rel(_ADKE.loop, 'muij = HIJ*xijdotvij'),
    'wall_reached': _rel(_WALL.post_loop, 'd_p[d_idx] = d_p[d_idx]/d_wij[d_idx]'),
}


def _val(x):
    return x.v if isinstance(x, VS) else x


def _norm(v):
    return math.sqrt(sum(float(_val(c)) ** 2 for c in v))


def decisions(table, run, i):
    """(branch names, smallest relative distance of a decision from its threshold) of destination i; a value that is
    zero by construction is exempt"""
    eqname = table['equation']
    rec = run['recs'][i]
    names, margin = set(), float('inf')

    def far(x, thr, rel=None):
        nonlocal margin
        x, thr = float(_val(x)), float(thr)
        margin = min(margin, abs(x - thr) / (abs(thr) if rel is None else rel))

    post = rec['post']
    L = post.locals if post is not None else {}
    D = table['arrays'][table['dest']]
    if eqname == 'SummationDensity':
        par = table['params']
        if LINES['sd_iter'] not in post.lines:
            names.add('density_iterations_false')
        elif LINES['sd_block'] not in post.lines:
            names.add('already_converged')
        else:
            hi = float(_val(L['hi']))
            raw = float(_val(L['hi'])) - float(_val(L['func'])) / float(_val(L['dfdh']))
            far(raw, 1.2 * hi)
            far(raw, 0.8 * hi)
            names.add('clamp_up' if LINES['sd_up'] in post.lines else 'clamp_down' if LINES['sd_down'] in post.lines else 'no_clamp')
            clamped = min(max(raw, 0.8 * hi), 1.2 * hi)
            far(clamped, 1e-6)
            far(L['gradhi'], 1e-6)
            if LINES['sd_fallback'] in post.lines:
                names.add('fallback_small_h' if clamped <= 1e-6 else 'fallback_gradh')
            om = 1.0 - float(_val(L['dhdrhoi'])) * float(_val(L['dwdhi']))
            far(om, 0.0, 1.0)
            if LINES['sd_reset'] in post.lines:
                names.add('omega_reset')
            far(L['diff'], par['htol'])
            if LINES['sd_not'] in post.lines:
                names.add('not_converged')
            else:
                names.add('converged_now' if float(_val(L['diff'])) < par['htol'] else 'once')
    elif eqname == 'MPMAccelerations':
        best, who = 0.0, None
        for sn, j, tr in rec['loop']:
            Lp = tr.locals
            self_pair = sn == table['dest'] and j == i
            rij = float(Lp['RIJ'])
            far(rij, 1e-8)
            vn = _norm(Lp['VIJ'])
            dot = float(Lp['dot'])
            if dot != 0.0:
                far(dot, 0.0, vn)
            if not self_pair:
                if LINES['mpm_zero'] in tr.lines:
                    if rij > 0:
                        names.add('rij_below_1e-8')
                    elif D['h'][i] != table['arrays'][sn]['h'][j]:
                        names.add('coincident_pair_unequal_h')
                else:
                    names.add('rij_above_1e-8')
                    names.add('approaching' if LINES['mpm_visc'] in tr.lines else 'receding')
            cfl = float(Lp['cij']) + table['params']['beta'] * dot
            if cfl > best:
                best, who = cfl, self_pair
        names.add('dt_cfl_stays_zero' if who is None else 'dt_cfl_from_self' if who else 'dt_cfl_from_partner')
        if LINES['mpm_a1'] in post.lines:
            far(D['div'][i], 0.0, 1.0)
            names.add('update_alpha1_div_negative' if D['div'][i] < 0 else 'update_alpha1_div_positive')
        if LINES['mpm_a2'] in post.lines:
            names.add('update_alpha2')
    elif eqname == 'ADKEAccelerations':
        for sn, j, tr in rec['loop']:
            Lp = tr.locals
            if sn == table['dest'] and j == i:
                continue
            xv = float(Lp['xijdotvij'])
            if xv != 0.0:
                far(xv, 0.0, _norm(Lp['VIJ']) * _norm(Lp['XIJ']))
            names.add('adke_approaching' if LINES['adke_visc'] in tr.lines else 'adke_receding')
            di, dj = float(Lp['divi']), float(Lp['divj'])
            far(di, 0.0, 1.0)
            far(dj, 0.0, 1.0)
            names.add('adke_div_' + ('p' if di > 0 else 'n') + ('p' if dj > 0 else 'n'))
    elif eqname == 'WallBoundary':
        wij = float(run['cols']['wij'][i]) if not isinstance(run['cols']['wij'], list) else float(run['cols']['wij'][i])
        if wij != 0.0:
            far(wij, 1e-30)
        if LINES['wall_reached'] in post.lines:
            names.add('reached_tiny' if wij < 1e-27 else 'reached')
        else:
            names.add('not_reached' if wij == 0.0 else 'below_threshold')
    return names, margin


def signature(rec):
    parts = ['%s:%d:%s' % (sn, j, ','.join(str(k) for k in sorted(tr.lines))) for sn, j, tr in rec['loop']]
    if rec['post'] is not None:
        parts.append('post:' + ','.join(str(k) for k in sorted(rec['post'].lines)))
    return ' '.join(parts)


def mutant_class(eqname, branch):
    meth, old, new = MUTANTS[branch]
    cls = CLASSES[eqname]
    src = textwrap.dedent(inspect.getsource(getattr(cls, meth)))
    assert src.count(old) == 1, (eqname, branch, src.count(old))
    ns = {}
    mod = sys.modules[cls.__module__]
    exec(compile(src.replace(old, new), '<%s %s inverted>' % (eqname, branch), 'exec'), mod.__dict__, ns)
    return type(cls.__name__, (cls,), {meth: ns[meth]})


# -- tables --------------------------------------------------------------------------------------------------------------
NEEDED = {
    'SummationDensity': ('x', 'y', 'z', 'u', 'v', 'w', 'h', 'h0', 'm', 'converged', 'omega', 'ah', 'rho', 'arho', 'grhox', 'grhoy',
                         'grhoz', 'dwdh', 'div'),
    'MPMAccelerations': ('x', 'y', 'z', 'u', 'v', 'w', 'h', 'm', 'rho', 'p', 'cs', 'e', 'omega', 'alpha1', 'alpha2', 'div', 'au', 'av',
                         'aw', 'ae', 'am', 'del2e', 'dt_cfl', 'aalpha1', 'aalpha2'),
    'SummationDensityADKE': ('x', 'y', 'z', 'u', 'v', 'w', 'h', 'h0', 'm', 'rho', 'arho', 'div', 'logrho'),
    'ADKEAccelerations': ('x', 'y', 'z', 'u', 'v', 'w', 'h', 'm', 'rho', 'p', 'cs', 'e', 'div', 'au', 'av', 'aw', 'ae'),
    'WallBoundary': ('x', 'y', 'z', 'u', 'v', 'w', 'h', 'h0', 'm', 'rho', 'p', 'cs', 'e', 'div', 'wij', 'htmp'),
}


def particle(rng, dim, arr, off, h, **kw):
    """fixed-seed doubles for every state column; ``kw`` overrides"""
    p = dict(arr=arr, off=off, h=h, h0=h, converged=0.0,
             m=float(rng.uniform(0.5, 2.0)) * 2.0 ** -6, rho=float(rng.uniform(0.5, 2.0)), p=float(rng.uniform(0.5, 2.0)),
             cs=float(rng.uniform(0.8, 1.5)), e=float(rng.uniform(1.0, 3.0)), omega=float(rng.uniform(0.7, 1.4)),
             alpha1=float(rng.uniform(0.2, 1.5)), alpha2=float(rng.uniform(0.05, 0.5)),
             div=float(rng.uniform(0.2, 1.0) * rng.choice([-1.0, 1.0])), ah=float(rng.uniform(-1, 1)))
    vel = rng.uniform(-1, 1, 3)
    for k, c in enumerate('uvw'):
        p[c] = float(vel[k]) if k < dim else 0.0
    p.update(kw)
    return p


def build_table(key, eqname, cfg, clusters, params, dest, sources, spacing=1.0, seed=0):
    cname, dim, kname = cfg
    rng = np.random.default_rng(seed + 991)
    names = []
    for cl in clusters:
        for q in cl:
            if q['arr'] not in names:
                names.append(q['arr'])
    names = [n for n in (dest,) + tuple(sources) if n in names] + [n for n in names if n not in (dest,) + tuple(sources)]
    arrays = {}
    for name in names:
        rows = [(c, q) for c, cl in enumerate(clusters) for q in cl if q['arr'] == name]
        cols = dict((k, np.zeros(len(rows))) for k in NEEDED[eqname])
        cols['cl'] = np.array([c for c, q in rows])
        for r, (c, q) in enumerate(rows):
            for k in cols:
                if k == 'cl':
                    continue
                if k in 'xyz':
                    cols[k][r] = (c if k == 'x' else 0.0) * spacing + q['off']['xyz'.index(k)]
                elif k in q:
                    cols[k][r] = q[k]
                else:
                    cols[k][r] = float(rng.uniform(-1, 1))        # garbage: must be overwritten
        arrays[name] = cols
    table = dict(key=key, equation=eqname, config=cname, dim=dim, kernel=kname, params=params, dest=dest, sources=tuple(sources),
                 arrays=arrays)
    table['nbrs'] = neighbours(table)
    return table


def _off(dim, r):
    return tuple(r * c for c in DIRS[dim])


def _h(rng):
    return 2.0 ** -4 * float(rng.uniform(1.0, 4.0))


SD_K = {'1d_cubic': 1.0625, '1d_gauss': 0.90625, '2d_cubic': 0.84375, '3d_quintic': 0.65625}


def sd_clusters(rng, dim, n_pairs, special=True):
    cl = []
    for k in range(n_pairs):
        hi, hj = _h(rng), _h(rng)
        r = min(float(rng.uniform(0.3, 1.5)) * min(hi, hj), 0.23)
        mi = float(rng.uniform(0.5, 2.0)) * 2.0 ** -6
        a = particle(rng, dim, 'fluid', _off(dim, 0.0), hi, m=mi, h0=hi * float(rng.choice([1.0, 0.5, 2.0])))
        b = particle(rng, dim, 'fluid', _off(dim, r), hj, m=mi * float(rng.uniform(0.1, 3.0)), h0=hj)
        cl.append([a, b])
    if special:
        for k in range(4):          # rows that come in converged
            hi, hj = _h(rng), _h(rng)
            r = min(float(rng.uniform(0.3, 1.5)) * min(hi, hj), 0.23)
            cl.append([particle(rng, dim, 'fluid', _off(dim, 0.0), hi, converged=1.0),
                       particle(rng, dim, 'fluid', _off(dim, r), hj, converged=float(k % 2))])
        for k in range(4):          # a partner of small negative mass: omegai < 0 with rho > 0 (the partner comes in converged)
            hi = _h(rng)
            mi = float(rng.uniform(0.5, 2.0)) * 2.0 ** -6
            r = min(float(rng.uniform(0.5, 1.2)) * hi, 0.23)
            cl.append([particle(rng, dim, 'fluid', _off(dim, 0.0), hi, m=mi),
                       particle(rng, dim, 'fluid', _off(dim, r), hi, m=-mi * 2.0 ** -(2 + k % 2), converged=1.0)])
    return cl


def mpm_clusters(rng, dim, two_fluids=False):
    other = 'f2' if two_fluids else 'fluid'
    first = 'f1' if two_fluids else 'fluid'
    cl = []

    def pair(r, hi=None, hj=None, kwa=None, kwb=None):
        hi, hj = hi or _h(rng), hj or _h(rng)
        cl.append([particle(rng, dim, first, _off(dim, 0.0), hi, **(kwa or {})), particle(rng, dim, other, _off(dim, r), hj, **(kwb or {}))])

    for k in range(8 if two_fluids else 14):
        hi, hj = _h(rng), _h(rng)
        pair(min(float(rng.uniform(0.3, 1.5)) * min(hi, hj), 0.23), hi, hj)
    d = DIRS[dim]
    for k in range(4):                  # strongly approaching (dt_cfl stays zero without a self pair) and strongly receding
        s = 3.0 if k < 2 else -3.0
        va = dict(zip('uvw', [-s * c for c in d]))
        vb = dict(zip('uvw', [s * c for c in d]))
        pair(0.125, kwa=va, kwb=vb)
    for k in range(2):
        pair(2.0 ** -27)
        pair(2.0 ** -26)
        pair(0.0, hi=2.0 ** -4 * (1.5 + k), hj=2.0 ** -4 * (2.5 + k))
        pair(0.1875, hi=2.0 ** -4, hj=2.0 ** -2)                   # h ratio 4: DWI = 0 for the small one, DWJ not
        pair(0.09375, kwa=dict(p=1.25), kwb=dict(p=1.25))           # vsig2 = 0
    for k in range(4):                  # one destination between two sources, one approaching, one receding
        hi = _h(rng)
        r1, r2 = float(rng.uniform(0.3, 0.9)) * 2.0 ** -4, float(rng.uniform(0.3, 0.9)) * 2.0 ** -4
        cl.append([particle(rng, dim, first, _off(dim, 0.0), hi, u=0.0, v=0.0, w=0.0),
                   particle(rng, dim, other, _off(dim, r1), _h(rng), **dict(zip('uvw', [0.5 * c for c in d]))),
                   particle(rng, dim, other, _off(dim, -r2), _h(rng), **dict(zip('uvw', [0.25 * c for c in d])))])
    return cl


def adkesd_clusters(rng, dim):
    cl = []
    for k in range(14):
        a0, b0 = 2.0 ** -4 * float(rng.uniform(1.0, 2.0)), 2.0 ** -4 * float(rng.uniform(1.0, 2.0))
        r = float(rng.uniform(0.3, 1.6)) * min(a0, b0)
        cl.append([particle(rng, dim, 'fluid', _off(dim, 0.0), 2 * a0, h0=a0), particle(rng, dim, 'fluid', _off(dim, r), 2 * b0, h0=b0)])
    for k in range(2):
        a0 = 2.0 ** -4 * float(rng.uniform(1.0, 2.0))
        cl.append([particle(rng, dim, 'fluid', _off(dim, 0.0), 2 * a0, h0=a0),
                   particle(rng, dim, 'fluid', _off(dim, 0.0625), 2.0 ** -3, h0=2.0 ** -4),
                   particle(rng, dim, 'fluid', _off(dim, -0.046875), 2.0 ** -3 * 1.5, h0=2.0 ** -4 * 1.5)])
    return cl


def adke_clusters(rng, dim):
    cl = []
    d = DIRS[dim]
    for k in range(16):
        hi, hj = _h(rng), _h(rng)
        r = min(float(rng.uniform(0.3, 1.5)) * min(hi, hj), 0.23)
        si, sj = (1.0, -1.0)[k % 2], (1.0, -1.0)[(k // 2) % 2]
        cl.append([particle(rng, dim, 'fluid', _off(dim, 0.0), hi, div=si * float(rng.uniform(0.2, 1.0))),
                   particle(rng, dim, 'fluid', _off(dim, r), hj, div=sj * float(rng.uniform(0.2, 1.0)))])
    for k in range(2):                  # e_i = e_j: no conduction
        cl.append([particle(rng, dim, 'fluid', _off(dim, 0.0), _h(rng), e=1.5), particle(rng, dim, 'fluid', _off(dim, 0.078125), _h(rng), e=1.5)])
    for k in range(4):
        cl.append([particle(rng, dim, 'fluid', _off(dim, 0.0), _h(rng), u=0.0, v=0.0, w=0.0),
                   particle(rng, dim, 'fluid', _off(dim, 0.0625), _h(rng), **dict(zip('uvw', [0.5 * c for c in d]))),
                   particle(rng, dim, 'fluid', _off(dim, -0.046875), _h(rng), **dict(zip('uvw', [0.25 * c for c in d])))])
    return cl


def wall_exponents(kname, dim, h):
    """e1: the largest e with W(2 - 2^-e) >= 8e-30; e2: the smallest with W <= 1e-30 / 8 (CubicSpline: W = fac / h^dim
    (2 - q)^3 / 4)"""
    pre = 0.25 * getattr(RK, kname)(dim=dim).fac / h ** dim
    e1 = max(e for e in range(20, 50) if pre * 2.0 ** (-3 * e) >= 8e-30)
    e2 = min(e for e in range(20, 50) if pre * 2.0 ** (-3 * e) <= 1e-30 / 8)
    return e1, e2


def wall_clusters(rng, dim, kname):
    cl = []

    def wall(h0):
        return particle(rng, dim, 'wall', (0.0, 0.0, 0.0), h0, h0=h0)

    for k in range(8):
        h0 = 2.0 ** -4 * float(rng.uniform(1.0, 3.0))
        cl.append([wall(h0), particle(rng, dim, 'fluid', _off(dim, min(float(rng.uniform(0.2, 1.6)) * h0, 0.23)), _h(rng))])
    for k in range(5):
        h0 = 2.0 ** -4 * float(rng.uniform(1.0, 2.0))
        cl.append([wall(h0), particle(rng, dim, 'fluid', _off(dim, float(rng.uniform(0.2, 1.6)) * h0 * 0.5), _h(rng)),
                   particle(rng, dim, 'fluid', _off(dim, -float(rng.uniform(0.2, 1.6)) * h0 * 0.5), _h(rng))])
    if kname == 'CubicSpline':
        e1, e2 = wall_exponents(kname, dim, 2.0 ** -3)
        for e in (e1, e1, e2, e2):
            cl.append([wall(2.0 ** -3), particle(rng, dim, 'fluid', (2.0 ** -3 * (2.0 - 2.0 ** -e), 0.0, 0.0), _h(rng))])
    for k in range(2):
        cl.append([wall(2.0 ** -4), particle(rng, dim, 'fluid', _off(1, 0.203125), 2.0 ** -4)])       # outside both radii
        cl.append([wall(2.0 ** -4), particle(rng, dim, 'fluid', _off(1, 0.203125), 2.0 ** -2)])       # a neighbour with W = 0
    return cl


def scaled(clusters, s, dim):
    out = []
    for cl in clusters:
        out.append([dict(q, off=tuple(c * s for c in q['off']), h=q['h'] * s, h0=q['h0'] * s, m=q['m'] * s ** dim) for q in cl])
    return out


def all_tables():
    """(table, counts towards the conditions)"""
    tables = []
    for ci, cfg in enumerate(CONFIGS):
        cname, dim, kname = cfg
        rng = np.random.default_rng(4100 + ci)
        sdp = dict(dim=dim, density_iterations=True, iterate_only_once=False, k=SD_K[cname], htol=0.125)
        tables.append(build_table('SummationDensity/main/' + cname, 'SummationDensity', cfg, sd_clusters(rng, dim, 22), sdp,
                                  'fluid', ['fluid'], seed=ci))
        tables.append(build_table('SummationDensity/once/' + cname, 'SummationDensity', cfg, sd_clusters(rng, dim, 8, False),
                                  dict(sdp, iterate_only_once=True), 'fluid', ['fluid'], seed=10 + ci))
        tables.append(build_table('SummationDensity/noiter/' + cname, 'SummationDensity', cfg, sd_clusters(rng, dim, 4, False),
                                  dict(sdp, density_iterations=False), 'fluid', ['fluid'], seed=20 + ci))
        tables.append(build_table('SummationDensity/small/' + cname, 'SummationDensity', cfg,
                                  scaled(sd_clusters(rng, dim, 6, False), 2.0 ** -24, dim), sdp, 'fluid', ['fluid'],
                                  spacing=2.0 ** -24, seed=30 + ci))
        mp_ = dict(beta=2.0, update_alpha1=True, update_alpha2=True, alpha1_min=0.1, alpha2_min=0.1, sigma=0.1)
        tables.append(build_table('MPMAccelerations/main/' + cname, 'MPMAccelerations', cfg, mpm_clusters(rng, dim), mp_,
                                  'fluid', ['fluid'], seed=40 + ci))
        two = mpm_clusters(rng, dim, two_fluids=True)
        mp2 = dict(mp_, update_alpha1=False, update_alpha2=False, beta=1.5)
        tables.append(build_table('MPMAccelerations/two_a/' + cname, 'MPMAccelerations', cfg, two, mp2, 'f1', ['f2'], seed=50 + ci))
        tables.append(build_table('MPMAccelerations/two_b/' + cname, 'MPMAccelerations', cfg, two, mp2, 'f2', ['f1'], seed=60 + ci))
        tables.append(build_table('SummationDensityADKE/main/' + cname, 'SummationDensityADKE', cfg, adkesd_clusters(rng, dim),
                                  dict(k=1.25, eps=0.5), 'fluid', ['fluid'], seed=70 + ci))
        tables.append(build_table('ADKEAccelerations/main/' + cname, 'ADKEAccelerations', cfg, adke_clusters(rng, dim),
                                  dict(alpha=1.0, beta=2.0, g1=0.5, g2=1.0, k=1.0, eps=0.5), 'fluid', ['fluid'], seed=80 + ci))
        tables.append(build_table('WallBoundary/main/' + cname, 'WallBoundary', cfg, wall_clusters(rng, dim, kname), {}, 'wall',
                                  ['fluid'], seed=90 + ci))
    return tables


# -- a table through both arithmetics ------------------------------------------------------------------------------------
def _split(x):
    hi = float(x)
    return hi, float(x - mp.mpf(hi))


SIGS = ['']


def _sig_id(s):
    if s not in SIGS:
        SIGS.append(s)
    return SIGS.index(s)


def kmeasure(got, mpv, S):
    """|got - truth| / (u S) per element; 0 where both are equal, inf where the scale is 0 and they differ"""
    k = np.zeros(len(mpv))
    for i in range(len(mpv)):
        g = float(got[i])
        if g != g:
            k[i] = np.inf
            continue
        d = abs(mp.mpf(g) - mpv[i])
        if d != 0:
            k[i] = float(d / (mp.mpf(U) * S[i])) if S[i] != 0 else np.inf
    with np.errstate(over='ignore'):
        return k.astype(np.float32).astype(np.float64)


def run_table(table, N2, Nmp):
    """the double and the 50-digit run of a table; None where the reference raises"""
    ref = sweep(table, N2)
    with mp.workdps(50):
        tru = sweep(table, Nmp)
        n = len(ref['recs'])
        res = dict(ref=ref, tru=tru, kref={}, names=[], margin=np.zeros(n), sig=np.zeros(n, np.int32), mpok=np.zeros(n, bool))
        for c in OUTPUTS[table['equation']]:
            res['kref'][c] = kmeasure(ref['cols'][c], tru['cols'][c], tru['S'][c])
        for i in range(n):
            names, margin = decisions(table, ref, i)
            res['names'].append(names)
            res['margin'][i] = margin
            s = signature(ref['recs'][i])
            res['sig'][i] = _sig_id(s)
            res['mpok'][i] = s == signature(tru['recs'][i])
    assert ref['flag'] == tru['flag']
    return res


def worst_k(res, eqname):
    return np.max(np.array([res['kref'][c] for c in OUTPUTS[eqname]]), axis=0)


def bound_of(res, eqname, k_eq):
    """per output column the bound in units of u S of every element (an element is well-conditioned where ITS K_ref is at
    most 64 and the 50-digit run took the path of the double run), and the destinations whose elements all are"""
    well = res['mpok'] & (worst_k(res, eqname) <= WELL)
    flat = max(FACTOR, FACTOR * k_eq)
    return dict((c, np.where(res['mpok'] & (res['kref'][c] <= WELL), flat, FACTOR * res['kref'][c])) for c in OUTPUTS[eqname]), well


def leaves_bound(table, res, other, k_eq, rows=None, only_well=False):
    """the destinations in which the columns of the run ``other`` (double) leave the bound around the 50-digit truth"""
    eqname = table['equation']
    bound, well = bound_of(res, eqname, k_eq)
    out = np.zeros(len(well), bool)
    with mp.workdps(50):
        for c in OUTPUTS[eqname]:
            k = kmeasure(other['cols'][c], res['tru']['cols'][c], res['tru']['S'][c])
            out |= ~(k <= bound[c])
    if only_well:
        out &= well
    return out if rows is None else out & rows


def build():
    out, dropped = {}, []
    tables = all_tables()
    nums = {}
    results = {}
    branches = Counter()
    keys = []
    for table in tables:
        cfg = (table['kernel'], table['dim'])
        if cfg not in nums:
            nums[cfg] = (Double(*cfg), Digits50(*cfg))
        results[table['key']] = run_table(table, *nums[cfg])
        keys.append(table['key'])
        print(table['key'], sum(len(v['x']) for v in table['arrays'].values()), 'particles', flush=True)
    # the lone particle: omegai = 1 - 1
    for ci, cfg in enumerate(CONFIGS):
        rng = np.random.default_rng(77 + ci)
        lone = build_table('SummationDensity/lone/' + cfg[0], 'SummationDensity', cfg,
                           [[particle(rng, cfg[1], 'fluid', (0.0, 0.0, 0.0), 2.0 ** -3)]],
                           dict(dim=cfg[1], density_iterations=True, iterate_only_once=False, k=SD_K[cfg[0]], htol=0.125), 'fluid', ['fluid'])
        try:
            with np.errstate(over='ignore'):          # (omegai of the order of u: the scale of 1 / omegai is beyond float32)
                r = run_table(lone, *nums[(cfg[2], cfg[1])])
            assert r['margin'][0] < MARGIN, 'the lone particle was expected to sit on omegai = 0'
            dropped.append(dict(table=lone['key'], state='a lone particle', error='omegai = 0 up to rounding'))
        except ZeroDivisionError:
            dropped.append(dict(table=lone['key'], state='a lone particle', error='ZeroDivisionError'))

    # 1, 2, 4, 5
    k_eq = {}
    for eqname in EQUATIONS:
        good, bad, total = [0.0], 0, 0
        for table in tables:
            if table['equation'] != eqname:
                continue
            res = results[table['key']]
            for names in res['names']:
                branches.update(names)
            assert np.all(res['margin'] >= MARGIN), (table['key'], 'a decision within 1e-3 of its threshold',
                                                     np.nonzero(res['margin'] < MARGIN)[0], res['margin'].min())
            w = worst_k(res, eqname)
            well = res['mpok'] & (w <= WELL)
            bad += int(np.sum(~well))
            total += well.size
            for c in OUTPUTS[eqname]:
                k = res['kref'][c][res['mpok']]
                good.extend(k[k <= WELL])
        assert bad * 10 <= total, (eqname, bad, total)
        k_eq[eqname] = float(max(good))
        print('K_eq %-22s %8.3f   (%d of %d destinations not well-conditioned)' % (eqname, k_eq[eqname], bad, total), flush=True)
    missing = dict((b, branches[b]) for b in REQUIRED if branches[b] < 2)
    assert not missing, ('taken fewer than twice', missing)
    for table in tables:           # the two constructed wall rows: a factor 8 from 1e-30
        if table['equation'] == 'WallBoundary':
            res = results[table['key']]
            wij = res['ref']['cols']['wij']
            for i, names in enumerate(res['names']):
                if 'reached_tiny' in names:
                    assert wij[i] >= 8e-30
                if 'below_threshold' in names:
                    assert 0 < wij[i] <= 1e-30 / 8

    # 3: observability
    observed = Counter()
    mutants = {}
    for b in REQUIRED:
        eqname = BRANCH_EQUATION[b]
        for table in tables:
            if table['equation'] != eqname:
                continue
            res = results[table['key']]
            rows = np.array([b in names for names in res['names']])
            if not rows.any():
                continue
            mk = (eqname, MUTANTS[b])
            if mk not in mutants:
                mutants[mk] = mutant_class(eqname, b)
            try:
                other = sweep(table, nums[(table['kernel'], table['dim'])][0], cls=mutants[mk])
                observed[b] += int(leaves_bound(table, res, other, k_eq[eqname], rows).sum())
            except ZeroDivisionError:
                observed[b] += int(rows.sum())           # the other side writes no number
    unobserved = dict((b, observed[b]) for b in REQUIRED if observed[b] < 2)
    assert not unobserved, ('not observable', unobserved)
    print('observable in', dict(observed), flush=True)

    # 6: sensitivity
    sensitive = Counter()
    for table in tables:
        eqname = table['equation']
        res = results[table['key']]
        N2 = nums[(table['kernel'], table['dim'])][0]
        if eqname in ('MPMAccelerations', 'ADKEAccelerations'):
            other = sweep(table, N2, params=dict(beta=table['params']['beta'] * (1 + 1e-13)))
        elif eqname in ('SummationDensity', 'SummationDensityADKE'):
            other = sweep(table, N2, params=dict(k=table['params']['k'] * (1 + 1e-13)))
        else:
            other = sweep(table, N2, scale_cols=dict((('fluid', c), 1 + 1e-13) for c in ('p', 'u', 'v', 'w', 'm', 'rho', 'e', 'cs', 'div')))
        sensitive[eqname] += int(leaves_bound(table, res, other, k_eq[eqname], only_well=True).sum())
    assert all(sensitive[e] >= 1 for e in EQUATIONS), sensitive
    print('sensitive to a part in 1e13:', dict(sensitive), flush=True)

    # the file
    for table in tables:
        key, eqname = table['key'], table['equation']
        res = results[key]
        # one entry per kind, the columns as rows (in the order of spec['in'] / OUTPUTS): an archive member costs more
        # than a short column holds
        incols = {}
        for name, cols in table['arrays'].items():
            # (a pure output column is garbage that the sweep overwrites: the test brings its own)
            incols[name] = [c for c in cols if not (name == table['dest'] and c in OUTPUTS[eqname] and c not in KEPT.get(eqname, ()))
                            and c != 'cl']
            out['%s/in/%s' % (key, name)] = np.array([cols[c] for c in incols[name]])
            out['%s/cl/%s' % (key, name)] = cols['cl'].astype(np.int16)
        out[key + '/spec'] = np.array(json.dumps({'equation': eqname, 'config': table['config'], 'dim': table['dim'],
                                                  'kernel': table['kernel'], 'params': table['params'], 'dest': table['dest'],
                                                  'sources': list(table['sources']), 'arrays': list(table['arrays']),
                                                  'in': incols, 'flag': int(res['ref']['flag'])}))
        for sn in table['sources']:
            lists = table['nbrs'][(table['dest'], sn)]
            out['%s/nbr_start/%s' % (key, sn)] = np.cumsum([0] + [len(v) for v in lists]).astype(np.int32)
            out['%s/nbr_idx/%s' % (key, sn)] = np.array([j for v in lists for j in v], dtype=np.int32)
        with mp.workdps(50):
            cs = OUTPUTS[eqname]
            pairs = [[_split(x) for x in res['tru']['cols'][c]] for c in cs]
            out[key + '/ref'] = np.array([res['ref']['cols'][c] for c in cs])
            out[key + '/mp'] = np.array([[p[0] for p in row] for row in pairs])
            out[key + '/mplo'] = np.array([[p[1] for p in row] for row in pairs])
            out[key + '/S'] = np.array([[float(s) for s in res['tru']['S'][c]] for c in cs]).astype(np.float32)
            out[key + '/kref'] = np.array([res['kref'][c] for c in cs]).astype(np.float32)
        out[key + '/sig'] = res['sig'].astype(np.int16)
        out[key + '/mpok'] = res['mpok']
        out[key + '/margin'] = res['margin'].astype(np.float32)
        out[key + '/names'] = np.array(json.dumps([sorted(n) for n in res['names']]))
    out['tables'] = np.array(json.dumps(keys))
    out['sigs'] = np.array(json.dumps(SIGS))
    out['meta/branches'] = np.array(json.dumps(dict((b, int(branches[b])) for b in sorted(branches))))
    out['meta/required'] = np.array(json.dumps(list(REQUIRED)))
    out['meta/observed'] = np.array(json.dumps(dict((b, int(observed[b])) for b in REQUIRED)))
    out['meta/sensitive'] = np.array(json.dumps(dict(sensitive)))
    out['meta/k_eq'] = np.array(json.dumps(k_eq))
    out['meta/dropped'] = np.array(json.dumps(dropped))
    out['meta/constants'] = np.array([WELL, FACTOR, MARGIN])
    return out


def main():
    out = build()
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size < 1024 * 1024, size
    print('wrote', OUT, size // 1024, 'KiB')


if __name__ == '__main__':
    main()
