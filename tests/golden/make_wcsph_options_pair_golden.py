#!/usr/bin/env python
"""The delta-SPH / laminar-viscosity rates and the delta-SPH pre-passes (``FamWCSPHX_T``, ``FamDSPre_T``), cluster by
cluster, from the REFERENCE's own classes -- ``GradientCorrectionPreStep``, ``GradientCorrection``
(wc/kernel_correction.py, with ``gj_solve`` of wc/linalg.py), ``ContinuityEquationDeltaSPHPreStep``,
``ContinuityEquationDeltaSPH``, ``MomentumEquation``, ``MomentumEquationDeltaSPH`` (wc/basic.py), ``LaminarViscosity``,
``LaminarViscosityDeltaSPH`` (wc/viscosity.py) and ``ContinuityEquation`` (basic_equations.py) -- executed as plain
Python by the group sweep of make_edac_pair_golden.py (which has the layout, the scale and the bound rule):

    python tests/golden/make_wcsph_options_pair_golden.py             ->  wcsph_options_pair_edges.npz
    python tests/golden/make_wcsph_options_pair_golden.py --mutants   ->  the list of tests/test_wcsph_options_pair_edges.py

Tables (every one in the four configurations, in a ``uh`` and a ``vh`` form; ``m_mat`` and ``gradrho`` are strided
properties, stored component by component):
    moment/n<k>       GradientCorrectionPreStep(dim = k) alone, k = 1, 2, 3 in every configuration: all nine components
                      are outputs, those outside the k x k block exactly 0, a pair at r <= 1e-12 adds exactly nothing
    gradient/*        [GradientCorrection(dim = k, tol), ContinuityEquationDeltaSPHPreStep], k = 1, 2, 3 in every
                      configuration (k is the equation's, whatever the kernel's dimension), WITH m_mat AN INPUT (a pair
                      or a triple has a rank-deficient moment matrix of its own: its last pivot would be rounding noise)
        well/n<k>     identity plus dyadic perturbations of at most 1/4, not symmetric, tol = 1/4; and the two matrices
                      with a last pivot of exactly 0 (below)
        built/n<k>    entries chosen so that the elimination is exact in double and the pivot is the number written,
                      tol = 2^50 (a tiny pivot gives a result of the order 2^40: only a large tol lets it act):
                      M00 = 2^-41 / 2^-39 (k >= 2), M11 = 2^-41 / 2^-39 behind a first column of zeros (k = 3),
                      M00 = 2^-41 under k = 1 (no pivot test: it divides), a last pivot of exactly 0 with a partner
                      along an axis on which that row's DWIJ is exactly 0 and with a partner off it (k <= dim >= 2;
                      with k > dim that row's DWIJ is 0 for every partner)
                      The entries outside the k x k block are 1/2: nothing may read them.
    order/alone       ContinuityEquationDeltaSPHPreStep alone
    order/behind      [ContinuityEquationDeltaSPHPreStep, GradientCorrection]: the correction behind corrects nothing;
                      the same inputs as order/alone, the same results bit for bit
    rates/*           ContinuityEquation + ContinuityEquationDeltaSPH; MomentumEquation (alpha = beta = 0, no tensile
                      correction, pressures of 2^-8) + MomentumEquationDeltaSPH, + LaminarViscosity, + LaminarViscosityDeltaSPH,
                      + both delta terms; the rates of WCSPHScheme(delta_sph=True, nu != 0) on the fluid alone and on
                      fluid <- {fluid, solid} with the delta terms on the fluid source only.  gradrho of destination and
                      source are independent inputs; one cluster per continuity table has fac XIJ = gradrho_i + gradrho_j
                      up to 2^-20 (ContinuityEquation's own term carries the scale of arho there, so these rows stay
                      well-conditioned, K_ref <= 19.3: the cancellation is seen at the column's scale, not at its own)
Conditions 1..6 as in make_edac_pair_golden.py.  Decisions: RIJ against 1e-12 (the kernel's guard and loop_all's), R2IJ
against 1e-12 (dt_cfl of MomentumEquation), every pivot but the last against 1e-12, |rhs| against 1e-12 where the last
pivot is exactly 0, ``change`` against ``tol``; gj_solve runs under a trace of its own, its lines are part of the path
that the 50-digit run must share (``float`` of wc/linalg.py is the identity there).  Inverted comparisons (MUTANTS): in
the text of gj_solve and of GradientCorrection.loop (the pivot test by moving 1e-12 across the pivot, to 1e-13 and to
1e-11: inverted as it stands it would leave at the first pivot of every matrix); the kernel's guard; ``rho_equal`` is rho_j + rho_i for
rho_j - rho_i; ``psi_cancelling`` is + s_gradrho for - s_gradrho.
"""
import inspect
import math
import os
import sys
import textwrap

import numpy as np
import mpmath as mp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as MG  # noqa: E402,F401  (sets up the reference imports)
import make_wcsph_options_golden as MW  # noqa: E402,F401  (``declare`` of the three modules that unpack it)
import make_edac_pair_golden as E  # noqa: E402  (the group sweep, the bound rule, the file)
import make_gasd_pair_golden as P  # noqa: E402

import pysph.sph.wc.kernel_correction as KC  # noqa: E402
import pysph.sph.wc.linalg as LA  # noqa: E402
from pysph.sph.wc import basic as RW  # noqa: E402
from pysph.sph.wc import viscosity as RV  # noqa: E402
from pysph.sph import basic_equations as RBE  # noqa: E402

OUT = os.path.join(HERE, 'wcsph_options_pair_edges.npz')
WELL, FACTOR, MARGIN = E.WELL, E.FACTOR, E.MARGIN
CONFIGS = E.CONFIGS
DIRS = E.DIRS
H0 = E.H0
GC_LOOP = MW._orig_loop            # (make_wcsph_options_golden.py wraps the method to record `change`: the reference's own)
CLASSES = {
    'GradientCorrectionPreStep': KC.GradientCorrectionPreStep, 'GradientCorrection': KC.GradientCorrection,
    'ContinuityEquationDeltaSPHPreStep': RW.ContinuityEquationDeltaSPHPreStep,
    'ContinuityEquationDeltaSPH': RW.ContinuityEquationDeltaSPH, 'MomentumEquation': RW.MomentumEquation,
    'MomentumEquationDeltaSPH': RW.MomentumEquationDeltaSPH, 'LaminarViscosity': RV.LaminarViscosity,
    'LaminarViscosityDeltaSPH': RV.LaminarViscosityDeltaSPH, 'ContinuityEquation': RBE.ContinuityEquation,
    'XSPHCorrection': RBE.XSPHCorrection,
}
LABELS = ('GradientCorrectionPreStep', 'GradientCorrection', 'ContinuityEquationDeltaSPHPreStep', 'ContinuityEquationDeltaSPH',
          'MomentumEquationDeltaSPH', 'LaminarViscosity', 'LaminarViscosityDeltaSPH', 'delta_terms', 'scheme_rates',
          'scheme_rates_solid')
COLUMNS = ('x', 'y', 'z', 'u', 'v', 'w', 'h', 'm', 'rho', 'p', 'cs', 'm_mat', 'gradrho', 'arho', 'au', 'av', 'aw', 'ax', 'ay', 'az',
           'dt_cfl', 'dt_force')
STRIDE = {'m_mat': 9, 'gradrho': 3}
OUTPUT_ORDER = tuple('m_mat__%d' % k for k in range(9)) + tuple('gradrho__%d' % k for k in range(3)) + (
    'arho', 'au', 'av', 'aw', 'ax', 'ay', 'az', 'dt_cfl', 'dt_force')
REQUIRED = ('corrected', 'uncorrected', 'pivot0_below', 'pivot0_above', 'pivot1_below', 'pivot1_above', 'n1_tiny_pivot',
            'last_zero_rhs_small', 'last_zero_rhs_large', 'rho_equal', 'rij_below_1e-12', 'rij_above_1e-12',
            'coincident_unequal_h', 'psi_cancelling')
UNOBSERVABLE = ()
# (the pivot test inverted as it stands leaves gj_solve at the FIRST pivot of every matrix, also where the reference leaves
# it at the second: the threshold is moved across the pivot instead, 2^-41 = 4.5e-13 < 1e-12 < 2^-39 = 1.8e-12)
_PIVB = ('gj', 'if abs(dnr) < 1e-12:', 'if abs(dnr) < 1e-13:')
_PIVA = ('gj', 'if abs(dnr) < 1e-12:', 'if abs(dnr) < 1e-11:')
MUTANTS = {
    'corrected': ('GradientCorrection', 'loop', 'if change < self.tol:', 'if change >= self.tol:'),
    'uncorrected': ('GradientCorrection', 'loop', 'if change < self.tol:', 'if change >= self.tol:'),
    'pivot0_below': _PIVB, 'pivot0_above': _PIVA, 'pivot1_below': _PIVB, 'pivot1_above': _PIVA,
    'n1_tiny_pivot': ('gj', 'if (m[nt*rb + rb] == 0):', 'if (abs(m[nt*rb + rb]) < 1e-12):'),
    'last_zero_rhs_small': ('gj', 'if (m[nt*rb + rb] == 0):', 'if (m[nt*rb + rb] != 0):'),
    'last_zero_rhs_large': ('gj', 'if abs(m[nt*rb + augCol - 1]) > tol:', 'if abs(m[nt*rb + augCol - 1]) <= tol:'),
    'rho_equal': ('ContinuityEquationDeltaSPHPreStep', 'loop', 'd_gradrho[d_idx*3 + 0] += (rhoj - rhoi)', 'd_gradrho[d_idx*3 + 0] += (rhoj + rhoi)'),
    'rij_below_1e-12': ('kernel',), 'rij_above_1e-12': ('kernel',), 'coincident_unequal_h': ('kernel',),
    'psi_cancelling': ('ContinuityEquationDeltaSPH', 'loop', '- s_gradrho[s_idx*3 + 0]', '+ s_gradrho[s_idx*3 + 0]'),
}
SENSITIVE = {
    'GradientCorrectionPreStep': ('column', 'm'), 'GradientCorrection': ('column', 'm'),
    'ContinuityEquationDeltaSPHPreStep': ('column', 'm'), 'ContinuityEquationDeltaSPH': ('ContinuityEquationDeltaSPH', 'delta'),
    'MomentumEquationDeltaSPH': ('MomentumEquationDeltaSPH', 'alpha'), 'LaminarViscosity': ('LaminarViscosity', 'nu'),
    'LaminarViscosityDeltaSPH': ('LaminarViscosityDeltaSPH', 'nu'), 'delta_terms': ('LaminarViscosityDeltaSPH', 'nu'),
    'scheme_rates': ('ContinuityEquationDeltaSPH', 'delta'), 'scheme_rates_solid': ('ContinuityEquationDeltaSPH', 'delta'),
}
ARITH = (
    ('gradrho_j dropped from psi', 'ContinuityEquationDeltaSPH', 'loop', '- s_gradrho[s_idx*3 + 1]', '- 0.0*s_gradrho[s_idx*3 + 1]'),
    ('gradrho_i dropped from psi', 'ContinuityEquationDeltaSPH', 'loop', '- d_gradrho[d_idx*3 + 0]', '- 0.0*d_gradrho[d_idx*3 + 0]'),
    ('fac = -2 (rho_j - rho_i) with the sign lost', 'ContinuityEquationDeltaSPH', 'loop', 'fac = -2.0 *', 'fac = 2.0 *'),
    ('HIJ replaced by h_i (continuity)', 'params', {'ContinuityEquationDeltaSPH': 'hi'}),
    ('HIJ replaced by h_i (momentum)', 'params', {'MomentumEquationDeltaSPH': 'hi'}),
    ('eta HIJ^2 replaced by EPS with eta = 1/64', 'params', {'LaminarViscosity': {'eta': 0.015625}}),
    ('eta HIJ^2 replaced by eta HIJ', 'LaminarViscosity', 'loop', 'self.eta*HIJ*HIJ', 'self.eta*HIJ'),
    ('2 (dim + 2) replaced by 2 dim', 'LaminarViscosityDeltaSPH', 'loop', '2 * (self.dim + 2)', '2 * (self.dim)'),
    ('m_j replaced by V_j in LaminarViscosity', 'LaminarViscosity', 'loop', 'mb = s_m[s_idx]', 'mb = s_m[s_idx]/rhob'),
    ('V_j replaced by m_j in MomentumEquationDeltaSPH', 'MomentumEquationDeltaSPH', 'loop', 'Vj = s_m[s_idx]/s_rho[s_idx]', 'Vj = s_m[s_idx]'),
    ('rho_i replaced by rho_j in MomentumEquationDeltaSPH', 'MomentumEquationDeltaSPH', 'loop', 'Vj/d_rho[d_idx]', 'Vj/s_rho[s_idx]'),
    ('moment matrix transposed', 'GradientCorrectionPreStep', 'loop_all', '9 * d_idx + 3 * i + j', '9 * d_idx + 3 * j + i'),
    ('moment matrix without V_b', 'GradientCorrectionPreStep', 'loop_all', '-= V * dwij[i] * xj', '-= dwij[i] * xj'),
    ('pivot threshold 1e-12 changed to 1e-11 (2^-39 = 1.8e-12)', 'gj', 'if abs(dnr) < 1e-12:', 'if abs(dnr) < 1e-11:'),
    ('pivot threshold 1e-12 changed to 1e-13 (2^-41 = 4.5e-13)', 'gj', 'if abs(dnr) < 1e-12:', 'if abs(dnr) < 1e-13:'),
    ('the zero last pivot eliminated above', 'gj', 'if (m[nt*rb + rb] == 0):', 'if (m[nt*rb + rb] == 12345.0):'),
    ('change relative to |DWIJ| without 1e-4 HIJ', 'GradientCorrection', 'loop', '(dwij_mag + eps)', '(dwij_mag)'),
    ('change < tol changed to change <= tol', 'GradientCorrection', 'loop', 'if change < self.tol:', 'if change <= self.tol:'),
    ('the corrected gradient applied to the first component only', 'GradientCorrection', 'loop', 'DWIJ[i] = res[i]', 'DWIJ[0] = res[0]'),
)
EQUIVALENT = ('change < tol changed to change <= tol',)


# -- gj_solve under a trace of its own -----------------------------------------------------------------------------------
GJ = [LA.gj_solve, inspect.getsource(LA.gj_solve).split('\n')]          # the function in use and the lines of its text
LAST = [None]


def _gj(m, n, nb, result):
    """the reference's gj_solve (or a mutant of it); records the lines it ran, ``dnr`` at every pivot test and, per
    back-substitution row, the diagonal and the right-hand side at the test of the diagonal"""
    fn, text = GJ
    code = fn.__code__
    log = dict(lines=set(), dnr=[], back=[])

    def local(frame, event, arg):
        if event == 'line':
            k = frame.f_lineno - code.co_firstlineno
            log['lines'].add(k)
            ln = text[k].strip()
            L = frame.f_locals
            if ln.startswith('if abs(dnr)'):
                log['dnr'].append((L['rrcol'], L['dnr']))
            elif ln.startswith('if') and 'm[nt*rb + rb]' in ln:
                nt, rb = L['nt'], L['rb']
                log['back'].append((rb, L['m'][nt * rb + rb], L['m'][nt * rb + L['augCol'] - 1]))
        return local

    def tracer(frame, event, arg):
        return local if frame.f_code is code else None

    old = sys.gettrace()
    sys.settrace(tracer)
    try:
        ret = fn(m, n, nb, result)
    finally:
        sys.settrace(old)
    log['ret'] = float(ret)
    LAST[0] = log
    return ret


def _attach(tr):
    tr.gj = LAST[0]
    tr.extra = ':gj%s' % ','.join(str(k) for k in sorted(tr.gj['lines']))


_NONE = object()


class _Bound(object):
    """what a sweep rebinds in the reference's modules, for the sweep only: the reference's own GradientCorrection.loop
    (make_wcsph_options_golden.py leaves a recording wrapper there), gj_solve under its trace, sqrt, and ``float`` of
    wc/linalg.py; ``unbind`` puts back what was there"""

    def _bind(self, sqrt, flt):
        self._saved = (KC.GradientCorrection.loop, KC.gj_solve, KC.sqrt, LA.__dict__.get('float', _NONE))
        KC.GradientCorrection.loop, KC.gj_solve, KC.sqrt, LA.float = GC_LOOP, _gj, sqrt, flt

    def unbind(self):
        E.unbind()
        KC.GradientCorrection.loop, KC.gj_solve, KC.sqrt, flt = self._saved
        if flt is _NONE:
            del LA.float
        else:
            LA.float = flt


class Double(_Bound, E.Double):
    def bind(self):
        E.Double.bind(self)
        self._bind(math.sqrt, float)


class Digits50(_Bound, E.Digits50):
    def bind(self):
        E.Digits50.bind(self)
        self._bind(mp.sqrt, lambda x: x)


class GuardInverted(_Bound, E.GuardInverted):
    bind = Double.bind


def numerics(tables):
    nums = {}
    for table in tables:
        cfg = (table['kernel'], table['dim'])
        if cfg not in nums:
            nums[cfg] = (Double(*cfg), Digits50(*cfg), GuardInverted(*cfg))
    return nums


# -- branches and margins ------------------------------------------------------------------------------------------------
def decisions(table, run, i):
    names, margin = set(), float('inf')

    def far(x, thr, rel=None):
        nonlocal margin
        margin = min(margin, abs(float(x) - thr) / (abs(thr) if rel is None else rel))

    A = table['arrays']
    D = A[table['dest']]
    group = dict((e['name'], e) for e in table['group'])
    seen = set()
    first = table['group'][0]['name']
    for sn, j, name, tr in run['recs'][i]['loop']:
        Sa = A[sn]
        if sn == table['dest'] and j == i:
            continue
        if (sn, j) not in seen:
            seen.add((sn, j))
            r2 = sum((D[c][i] - Sa[c][j]) ** 2 for c in 'xyz')
            rij = math.sqrt(r2)
            if rij == 0.0:
                if D['h'][i] != Sa['h'][j]:
                    names.add('coincident_unequal_h')
            else:
                far(rij, 1e-12)
                if 'MomentumEquation' in group:
                    far(r2, 1e-12)
                if rij <= 1e-12:
                    names.add('rij_below_1e-12')
                elif rij < 1e-9:
                    names.add('rij_above_1e-12')
            if Sa['rho'][j] == D['rho'][i] and ('ContinuityEquationDeltaSPHPreStep' in group or 'ContinuityEquationDeltaSPH' in group):
                names.add('rho_equal')
        if name == 'GradientCorrection':
            gj, L = tr.gj, tr.locals
            n = group[name]['params']['dim']
            far(L['change'], group[name]['params']['tol'])
            if first != 'GradientCorrection':
                continue                     # (behind the pre-step: its decisions are on the path, its result is not read)
            for col, dnr in gj['dnr']:
                far(abs(float(dnr)), 1e-12)
                if abs(float(dnr)) < 1e-9:
                    names.add('pivot%d_%s' % (col, 'below' if abs(float(dnr)) < 1e-12 else 'above'))
            for rb, diag, rhs in gj['back']:
                if float(diag) == 0.0:
                    assert rb == n - 1, 'a zero pivot that is not the last'
                    if float(rhs) != 0.0:
                        far(abs(float(rhs)), 1e-12)
                    names.add('last_zero_rhs_large' if abs(float(rhs)) > 1e-12 else 'last_zero_rhs_small')
                elif n == 1 and abs(float(diag)) < 1e-12:
                    names.add('n1_tiny_pivot')
            names.add('corrected' if float(L['change']) < group[name]['params']['tol'] else 'uncorrected')
    if i in table.get('cancelling', ()):
        names.add('psi_cancelling')
    return names, margin


def mutant_run(table, nums, spec):
    keep = KC.GradientCorrection.loop
    KC.GradientCorrection.loop = GC_LOOP          # (the text a mutant is made from)
    try:
        return _mutant_run(table, nums, spec)
    finally:
        KC.GradientCorrection.loop = keep


def _mutant_run(table, nums, spec):
    have = [e['name'] for e in table['group']]
    if spec[0] == 'gj':
        if 'GradientCorrection' not in have:
            return None
        src = textwrap.dedent(inspect.getsource(LA.gj_solve))
        assert src.count(spec[1]) == 1, spec
        ns = {}
        new = src.replace(spec[1], spec[2])
        exec(compile(new, '<gj_solve changed>', 'exec'), LA.__dict__, ns)
        keep = list(GJ)
        GJ[:] = [ns['gj_solve'], new.split('\n')]
        try:
            return E.gsweep(table, nums[(table['kernel'], table['dim'])][0], catch=True)
        finally:
            GJ[:] = keep
    if spec[0] == 'params' and 'hi' in spec[1].values():           # HIJ of one equation replaced by the destination's h
        hit = [n for n in spec[1] if n in have]
        if not hit:
            return None
        classes = {}
        for n in hit:
            cls = CLASSES[n]
            src = textwrap.dedent(inspect.getsource(cls.loop))
            head = src[:src.index('):') + 2]
            body = src[src.index('):') + 2:]
            assert 'd_h' not in head
            new = head.replace('(self, d_idx,', '(self, d_idx, d_h,') + body.replace('HIJ', 'd_h[d_idx]')
            ns = {}
            exec(compile(new, '<%s.loop with h_i>' % n, 'exec'), sys.modules[cls.__module__].__dict__, ns)
            classes[n] = type(cls.__name__, (cls,), {'loop': ns['loop']})
        return E.gsweep(table, nums[(table['kernel'], table['dim'])][0], classes=classes, catch=True)
    return E.mutant_run(table, nums, spec)


# -- tables --------------------------------------------------------------------------------------------------------------
def particle(rng, dim, arr, off, h, **kw):
    rho = float(rng.uniform(0.75, 1.5))
    q = dict(arr=arr, off=off, h=h, rho=rho, m=float(rng.uniform(0.75, 1.5)) * 2.0 ** -6, p=float(rng.uniform(0.5, 2.0)),
             cs=float(rng.uniform(0.8, 1.5)), gradrho=[float(x) if k < dim else 0.0 for k, x in enumerate(rng.uniform(-4, 4, 3))],
             m_mat=[0.5] * 9)
    vel = rng.uniform(-1, 1, 3)
    for k, c in enumerate('uvw'):
        q[c] = float(vel[k]) if k < dim else 0.0
    q.update(kw)
    return q


def _off(dim, r, axis=None):
    if axis is not None:
        return tuple(r if k == axis else 0.0 for k in range(3))
    return tuple(r * c for c in DIRS[dim])


def matrix(n, block):
    """the 3 x 3 row-major list with ``block`` (n x n) in its corner and 1/2 outside it"""
    m = [0.5] * 9
    for i in range(n):
        for j in range(n):
            m[3 * i + j] = block[i][j]
    return m


def well_matrix(rng, n):
    return matrix(n, [[(1.0 if i == j else 0.0) + float(rng.integers(-4, 5)) / 16.0 for j in range(n)] for i in range(n)])


def last_zero_matrix(n):
    """the last pivot exactly 0 without an elimination step touching it"""
    return matrix(n, [[0.0] if n == 1 else [1.0, 0.25], [0.0, 0.0]] if n < 3 else [[1.0, 0.25, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 0.0]])


def built_matrices(n):
    """(name of the branch, matrix): the pivot is the number written, every elimination step is exact in double"""
    out = []
    if n == 1:
        out.append(('n1_tiny_pivot', matrix(1, [[2.0 ** -41]])))
    if n == 2:
        out.append(('pivot0_below', matrix(2, [[2.0 ** -41, 0.25], [0.0, 1.0]])))
        out.append(('pivot0_above', matrix(2, [[2.0 ** -39, 0.25], [0.0, 1.0]])))
    if n == 3:
        out.append(('pivot0_below', matrix(3, [[2.0 ** -41, 0.25, 0.0], [0.0, 1.0, 0.125], [0.0, 0.0, 1.0]])))
        out.append(('pivot0_above', matrix(3, [[2.0 ** -39, 0.25, 0.0], [0.0, 1.0, 0.125], [0.0, 0.0, 1.0]])))
        out.append(('pivot1_below', matrix(3, [[1.0, 0.25, 0.0], [0.0, 2.0 ** -41, 0.125], [0.0, 0.0, 1.0]])))
        out.append(('pivot1_above', matrix(3, [[1.0, 0.25, 0.0], [0.0, 2.0 ** -39, 0.125], [0.0, 0.0, 1.0]])))
    return out


def clusters(rng, dim, uh, kind, n=None, other='fluid'):
    cl = []

    def hh():
        return H0 if uh else P._h(rng)

    def pair(r, hi=None, hj=None, kwa=None, kwb=None, arr=None, axis=None):
        hi, hj = hi or hh(), hj or hh()
        cl.append([particle(rng, dim, 'fluid', _off(dim, 0.0), hi, **(kwa or {})),
                   particle(rng, dim, arr or other, _off(dim, r, axis), hj, **(kwb or {}))])

    def sep(hi, hj):
        return min(float(rng.uniform(0.3, 1.5)) * min(hi, hj), 0.23)

    def mm():
        return dict(m_mat=well_matrix(rng, n)) if n else {}

    for k in range(5):
        hi, hj = hh(), hh()
        pair(sep(hi, hj), hi, hj, kwa=mm(), kwb=mm(), arr=('fluid' if k % 3 == 2 else None))
    for k in range(2):
        cl.append([particle(rng, dim, 'fluid', _off(dim, 0.0), hh(), **mm()), particle(rng, dim, other, _off(dim, 0.0625), hh(), **mm()),
                   particle(rng, dim, 'fluid', _off(dim, -0.046875), hh(), **mm())])
    for r in (2.0 ** -40, 2.0 ** -40, 2.0 ** -39, 2.0 ** -39):
        pair(r, kwa=mm(), kwb=mm())
    if uh:
        pair(0.0, kwa=mm(), kwb=mm())
    else:
        pair(0.0, hi=2.0 ** -4 * 1.5, hj=2.0 ** -4 * 2.5, kwa=mm(), kwb=mm())
        pair(0.0, hi=2.0 ** -4 * 3.5, hj=2.0 ** -4 * 2.0, kwa=mm(), kwb=mm())
        pair(0.1875, hi=2.0 ** -4, hj=2.0 ** -2, kwa=mm(), kwb=mm())
    if kind in ('pre', 'cont'):
        pair(0.078125, kwa=dict(rho=1.25, **mm()), kwb=dict(rho=1.25, **mm()))
        pair(0.0625, kwa=dict(rho=0.875, **mm()), kwb=dict(rho=0.875, **mm()))
    if kind in ('pre', 'built') and n and (dim >= 2 or n >= 2):
        # the last pivot exactly 0: a partner along the axis on which the last row's DWIJ is 0, and one off it (with
        # n > dim that row's DWIJ is 0 for every partner: in 1-D under n = 2, 3, in 2-D under n = 3 both are `small`)
        axis = 1 if n == 1 else 0
        for k in range(2):
            z = dict(m_mat=last_zero_matrix(n))
            pair(0.0625 + 0.015625 * k, kwa=dict(z), kwb=dict(z), axis=axis)
            pair(0.0625 + 0.015625 * k, kwa=dict(z), kwb=dict(z))
    if kind == 'mom':                   # the base equation's pressure term small next to the term under test
        for c in cl:
            for q in c:
                q['p'] *= 2.0 ** -8
    if kind == 'built':
        for name, m in built_matrices(n):
            for k in range(2):
                pair(0.0625 + 0.015625 * k, kwa=dict(m_mat=list(m)), kwb=dict(m_mat=list(m)))
    return cl


def build_table(key, label, cfg, form, cl, group, t=0.25, seed=0, cancelling=False):
    cname, dim, kname = cfg
    rng = np.random.default_rng(seed + 2777)
    dest = 'fluid'
    sources = []
    for e in group:
        for s in e['sources']:
            if s not in sources:
                sources.append(s)
    used = columns_of(group)
    cancel_rows = []
    if cancelling:
        # fac XIJ = gradrho_i + gradrho_j up to 2^-20 (wc/basic.py:404-408; the same for both orders of the pair)
        hi, hj = (H0, H0) if form == 'uh' else (2.0 ** -4 * 1.75, 2.0 ** -4 * 2.25)
        a = particle(rng, dim, 'fluid', _off(dim, 0.0), hi)
        b = particle(rng, dim, 'fluid', _off(dim, 0.09375), hj)
        xij = [-c for c in b['off']]
        hij = 0.5 * (hi + hj)
        fac = -2.0 * (b['rho'] - a['rho']) / (sum(c * c for c in xij) + 0.01 * hij * hij)
        b['gradrho'] = [fac * x * (1.0 - 2.0 ** -20) - g for x, g in zip(xij, a['gradrho'])]
        cl = cl + [[a, b]]
    names = [dest] + [s for s in sources if s != dest]
    arrays = {}
    for name in names:
        rows = [(c, q) for c, cluster in enumerate(cl) for q in cluster if q['arr'] == name]
        cols = dict((k, np.zeros(len(rows) * STRIDE.get(k, 1))) for k in used)
        cols['cl'] = np.array([c for c, q in rows])
        for r, (c, q) in enumerate(rows):
            if cancelling and name == dest and c == len(cl) - 1:
                cancel_rows.append(r)
            for k in used:
                s = STRIDE.get(k, 1)
                if k in 'xyz':
                    cols[k][r] = (c if k == 'x' else 0.0) + q['off']['xyz'.index(k)]
                elif k in q:
                    cols[k][r * s:(r + 1) * s] = q[k]
                else:
                    cols[k][r * s:(r + 1) * s] = rng.uniform(-1, 1, s)        # garbage: must be overwritten
        arrays[name] = cols
    table = dict(key=key, label=label, config=cname, dim=dim, kernel=kname, form=form, group=group, dest=dest,
                 sources=tuple(sources), arrays=arrays, t=t, decide=decisions, cancelling=tuple(cancel_rows),
                 classes=CLASSES, numerics=numerics, hooks={'GradientCorrection': _attach}, symbols=dict(WDP=1.0))          # (WDP: read by MomentumEquation.loop, used under tensile_correction only)
    table['outputs'] = writes(table)
    table['nbrs'] = E.neighbours(table)
    return table


def columns_of(group):
    used = set(('x', 'y', 'z', 'u', 'v', 'w', 'h', 'm', 'rho'))
    for e in group:
        for meth in ('initialize', 'loop', 'loop_all', 'post_loop'):
            fn = getattr(CLASSES[e['name']], meth, None)
            for a in (P._args(fn) if fn is not None else ()):
                if a[:2] in ('d_', 's_') and a not in ('d_idx', 's_idx'):
                    used.add(a[2:])
    return tuple(c for c in COLUMNS if c in used)


def writes(table):
    """the destination columns the group's methods assign, from the reference's text; a strided one by its components"""
    found = []
    for e in table['group']:
        cls = CLASSES[e['name']]
        for meth in ('initialize', 'loop', 'loop_all', 'post_loop'):
            fn = getattr(cls, meth, None)
            if fn is None:
                continue
            for ln in inspect.getsource(fn).split('\n'):
                ln = ln.strip()
                if ln.startswith('d_') and '[' in ln.split('=')[0] and '=' in ln and 'd_idx' in ln.split('=')[0]:
                    c = ln[2:ln.index('[')]
                    if c not in found:
                        found.append(c)
    out = []
    for c in found:
        out.extend([c] if c not in STRIDE else ['%s__%d' % (c, k) for k in range(STRIDE[c])])
    return tuple(c for c in OUTPUT_ORDER if c in out)


C0, RHO0, NU, DELTA, ALPHA = 1.5, 1.0, 0.375, 0.21875, 0.75
G3 = dict(gx=0.5, gy=-0.25, gz=0.125)


def _eq(name, sources, **params):
    return dict(name=name, sources=list(sources), params=params)


def all_tables():
    tables = []
    f, fs = ['fluid'], ['fluid', 'solid']
    mom = dict(c0=C0, alpha=0.0, beta=0.0, tensile_correction=False, **G3)
    for ci, cfg in enumerate(CONFIGS):
        cname, dim, kname = cfg
        for fi, form in enumerate(('uh', 'vh')):
            uh = form == 'uh'
            rng = np.random.default_rng(6300 + 10 * ci + fi)
            seed = [100 * ci + 50 * fi]

            def add(label, kind, cl, group, **kw):
                seed[0] += 1
                tables.append(build_table('%s/%s/%s/%s' % (label, kind, cname, form), label, cfg, form, cl, group, seed=seed[0], **kw))

            for n in (1, 2, 3):
                add('GradientCorrectionPreStep', 'moment_n%d' % n, clusters(rng, dim, uh, ''), [_eq('GradientCorrectionPreStep', f, dim=n)])
            for n in (1, 2, 3):          # (n is GradientCorrection.dim, whatever the kernel's: the scheme's 2 also in 1-D)
                add('GradientCorrection', 'well_n%d' % n, clusters(rng, dim, uh, 'pre', n),
                    [_eq('GradientCorrection', f, dim=n, tol=0.25), _eq('ContinuityEquationDeltaSPHPreStep', f)])
                add('GradientCorrection', 'built_n%d' % n, clusters(rng, dim, uh, 'built', n),
                    [_eq('GradientCorrection', f, dim=n, tol=2.0 ** 50), _eq('ContinuityEquationDeltaSPHPreStep', f)])
            order = clusters(np.random.default_rng(6400 + 10 * ci + fi), dim, uh, 'pre', dim)
            keep = seed[0]
            add('ContinuityEquationDeltaSPHPreStep', 'alone', order, [_eq('ContinuityEquationDeltaSPHPreStep', f)])
            seed[0] = keep           # (the same garbage too: the two tables differ in their group only)
            add('ContinuityEquationDeltaSPHPreStep', 'behind', order,
                [_eq('ContinuityEquationDeltaSPHPreStep', f), _eq('GradientCorrection', f, dim=dim, tol=0.25)])
            dcont = _eq('ContinuityEquationDeltaSPH', f, c0=C0, delta=DELTA)
            dmom = _eq('MomentumEquationDeltaSPH', f, rho0=RHO0, c0=C0, alpha=ALPHA)
            lamd = _eq('LaminarViscosityDeltaSPH', f, dim=dim, rho0=RHO0, nu=NU)
            add('ContinuityEquationDeltaSPH', 'continuity', clusters(rng, dim, uh, 'cont'), [_eq('ContinuityEquation', f), dcont], cancelling=True)
            add('MomentumEquationDeltaSPH', 'momentum', clusters(rng, dim, uh, 'mom'), [_eq('MomentumEquation', f, **mom), dmom])
            add('LaminarViscosity', 'momentum', clusters(rng, dim, uh, 'mom'), [_eq('MomentumEquation', f, **mom), _eq('LaminarViscosity', f, nu=NU, eta=0.01)])
            add('LaminarViscosityDeltaSPH', 'momentum', clusters(rng, dim, uh, 'mom'), [_eq('MomentumEquation', f, **mom), lamd])
            add('delta_terms', 'momentum', clusters(rng, dim, uh, 'mom'), [_eq('MomentumEquation', f, **mom), dmom, lamd])
            # pysph/sph/scheme.py WCSPHScheme.get_equations with delta_sph and nu: the rates group
            add('scheme_rates', 'fluid', clusters(rng, dim, uh, 'cont'),
                [_eq('ContinuityEquation', f), dcont, _eq('MomentumEquation', f, **mom), dmom, _eq('XSPHCorrection', f, eps=0.5), lamd],
                cancelling=True)
            add('scheme_rates_solid', 'solid', clusters(rng, dim, uh, 'cont', other='solid'),
                [_eq('ContinuityEquation', fs), dcont, _eq('MomentumEquation', fs, **mom), dmom, _eq('XSPHCorrection', f, eps=0.5), lamd],
                cancelling=True)
    return tables


def main():
    E.write(sys.modules[__name__], OUT)


if __name__ == '__main__':
    main()
