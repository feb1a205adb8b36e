#!/usr/bin/env python
"""The EDAC force group and the average pressure (``FamEDAC_T``, ``FamAvgP_T``), cluster by cluster, from the REFERENCE's
own classes -- ``ComputeAveragePressure``, ``MomentumEquation``, ``MomentumEquationPressureGradient``, ``EDACEquation``
(wc/edac.py), ``SummationDensity``, ``MomentumEquationViscosity``, ``MomentumEquationArtificialViscosity``,
``MomentumEquationArtificialStress`` (wc/transport_velocity.py) and ``XSPHCorrection`` (basic_equations.py) -- executed
as plain Python with the machinery of make_gasd_pair_golden.py (its number type that carries a scale, its recording
columns, its call traces, its pair symbols, its two arithmetics and its K measure):

    python tests/golden/make_edac_pair_golden.py             ->  edac_pair_edges.npz
    python tests/golden/make_edac_pair_golden.py --mutants   ->  the wrong-arithmetic list of tests/test_edac_pair_edges.py

Layout.  As gasd_pair_edges.npz: every table is a row of isolated clusters along x, 1 apart; every h is in
[2^-4, 2^-2], a cluster is less than 1/4 across.  Clusters are lone particles (the average pressure), pairs in both
orders and triples.  Every table exists in 1-D under CubicSpline, in 2-D under WendlandQuintic, in 3-D under
QuinticSpline and in 3-D under Gaussian, the partner offset along (1, 0, 0), (3/4, -1/2, 0) and (1/2, -3/4, 1/4), and
in two forms: ``uh`` (every h of every array is 2^-3) and ``vh`` (h unequal within clusters).  Every input is a dyadic
number or a fixed-seed double.  ``V`` is an input near rho / m.

A table runs ONE GROUP, the smallest the product takes into the family under test (``group`` of its spec): the equation
alone where the product accepts it alone, next to a base equation with plain parameters where it does not.  The sweep is
the reference's (acceleration_eval): ``initialize`` of every equation over the destinations; per source array, per
destination, per neighbour, ``loop`` of every equation that has the source; ``post_loop`` of every equation.  A table
runs twice, in double (``ref``) and at 50 digits (``mp`` + ``mplo``; ``mpok`` where that run took the lines of the
double run), at the stored time ``t`` (never 0).

Scale.  A column the loops accumulate: S = the sum over the cluster of |new - old| of every statement of every
equation of the group that writes it (50 digits).  ``post_loop`` runs on values that carry their scale with the rules of
make_gasd_pair_golden.py: pavg = PAVG / NNBR, a* += damping g, ax = AX + u.  An element of scale 0 must be exact.

Conditions asserted here on the reference alone (tests/test_edac_pair_edges.py asserts them again on the file):
  1. every branch of REQUIRED is taken at least twice;
  2. no decision within a relative 1e-3 of its threshold: t against tdamp, vijdotrij against 0 relative to |VIJ| |XIJ|,
     RIJ against 1e-12, nnbr against 0 (a count); a value that is exactly on it by construction (t == tdamp, RIJ == 0,
     vijdotrij == 0) is exempt;
  3. every REQUIRED branch but ``tdamp_equal`` is observable: the method with that one comparison inverted (MUTANTS;
     its source text patched in memory) leaves the bound of item 5 in at least two destinations that took the branch; a
     mutant that raises where the reference does not counts as leaving it.  Branches without a comparison of their own in
     an equation's text: the gradient guard ``rij > 1e-12`` is the KERNEL's (pysph/base/kernels.py) and is inverted
     there; ``nnbr_self_only`` is the sweep without the self pair; ``p_equal`` is p_i + p_j for p_i - p_j; ``eps_zero``
     is eps + 1 for eps.  ``tdamp_equal`` is NOT observable by any test of values and is exempt: the ramp
     0.5 (sin((-1/2 + t / tdamp) pi) + 1) is exactly 1.0 in double at t == tdamp, what the other side of ``t < tdamp``
     writes;
  4. per table label at most one destination in ten has K_ref > 64 in a column or another path at 50 digits;
  5. K_eq = the largest K_ref over the well-conditioned elements of a label (meta/k_eq), at most 64; a well-conditioned
     element is held to max(4, 4 K_eq) u S, any other to 4 K_ref of itself;
  6. a relative 1e-13 on one parameter per label (SENSITIVE: pb, nu, edac_nu through the group, cs, alpha, eps; the
     sources' p for the two equations without a parameter of their own in a pair term; rho for the artificial stress)
     leaves that bound in at least one well-conditioned element.
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
import make_edac_golden as MEG  # noqa: E402,F401  (the stub of pysph.base.utils that wc/edac.py imports)
import make_gasd_pair_golden as P  # noqa: E402  (VS, RecList, CallTrace, symbols, Double, Digits50, kmeasure)
import helpers as H  # noqa: E402  (mp_kernel)

from pysph.sph.wc import edac as RE  # noqa: E402
from pysph.sph.wc import transport_velocity as RT  # noqa: E402
from pysph.sph import basic_equations as RBE  # noqa: E402
from pysph.base import kernels as RK  # noqa: E402

OUT = os.path.join(HERE, 'edac_pair_edges.npz')
U = 2.0 ** -53
WELL, FACTOR, MARGIN = P.WELL, P.FACTOR, P.MARGIN
CONFIGS = (('1d_cubic', 1, 'CubicSpline'), ('2d_wendland', 2, 'WendlandQuintic'), ('3d_quintic', 3, 'QuinticSpline'),
           ('3d_gauss', 3, 'Gaussian'))
KERNEL_IDS = dict(P.KERNEL_IDS, WendlandQuintic=2)          # (tests/helpers.mp_kernel knows all four)
RADIUS = {'CubicSpline': 2.0, 'WendlandQuintic': 2.0, 'QuinticSpline': 3.0, 'Gaussian': 3.0}
DIRS = P.DIRS
H0 = 2.0 ** -3
CLASSES = {
    'ComputeAveragePressure': RE.ComputeAveragePressure, 'SummationDensity': RT.SummationDensity,
    'MomentumEquation': RE.MomentumEquation, 'MomentumEquationPressureGradient': RE.MomentumEquationPressureGradient,
    'EDACEquation': RE.EDACEquation, 'MomentumEquationViscosity': RT.MomentumEquationViscosity,
    'MomentumEquationArtificialViscosity': RT.MomentumEquationArtificialViscosity,
    'MomentumEquationArtificialStress': RT.MomentumEquationArtificialStress, 'XSPHCorrection': RBE.XSPHCorrection,
}
# what the methods of an equation write (read off the reference's initialize / loop / post_loop signatures by WRITES below)
LABELS = ('ComputeAveragePressure', 'MomentumEquation', 'MomentumEquationPressureGradient', 'EDACEquation',
          'MomentumEquationViscosity', 'MomentumEquationArtificialViscosity', 'MomentumEquationArtificialStress',
          'XSPHCorrection', 'external_group', 'internal_group', 'internal_solid_group')
COLUMNS = ('x', 'y', 'z', 'u', 'v', 'w', 'h', 'm', 'rho', 'p', 'V', 'uhat', 'vhat', 'what', 'pavg', 'nnbr', 'au', 'av', 'aw',
           'auhat', 'avhat', 'awhat', 'ap', 'ax', 'ay', 'az')
OUTPUT_ORDER = ('au', 'av', 'aw', 'auhat', 'avhat', 'awhat', 'ap', 'ax', 'ay', 'az', 'pavg', 'nnbr', 'rho', 'V')
REQUIRED = ('nnbr_positive', 'nnbr_zero', 'nnbr_self_only', 'tdamp_ramp', 'tdamp_equal', 'tdamp_past', 'tdamp_zero',
            'approaching', 'receding', 'p_equal', 'eps_zero', 'rij_below_1e-12', 'rij_above_1e-12', 'coincident_unequal_h')
UNOBSERVABLE = ('tdamp_equal',)
_TD = ('post_loop', 'if t < self.tdamp:', 'if t >= self.tdamp:')
_AV = ('MomentumEquationArtificialViscosity', 'loop', 'if vijdotrij < 0:', 'if vijdotrij >= 0:')
# branch -> (equation, method, text of the reference's line, replacement) | ('kernel',) | ('no_self',)
MUTANTS = {
    'nnbr_positive': ('ComputeAveragePressure', 'post_loop', 'if d_nnbr[d_idx] > 0:', 'if d_nnbr[d_idx] <= 0:'),
    'nnbr_zero': ('ComputeAveragePressure', 'post_loop', 'if d_nnbr[d_idx] > 0:', 'if d_nnbr[d_idx] <= 0:'),
    'nnbr_self_only': ('no_self',),
    'tdamp_ramp': ('*',) + _TD, 'tdamp_equal': ('*',) + _TD, 'tdamp_past': ('*',) + _TD, 'tdamp_zero': ('*',) + _TD,
    'approaching': _AV, 'receding': _AV,
    'p_equal': ('EDACEquation', 'loop', '(d_p[d_idx] - s_p[s_idx])', '(d_p[d_idx] + s_p[s_idx])'),
    'eps_zero': ('XSPHCorrection', 'loop', 'tmp = -self.eps ', 'tmp = -(self.eps + 1.0) '),
    'rij_below_1e-12': ('kernel',), 'rij_above_1e-12': ('kernel',), 'coincident_unequal_h': ('kernel',),
}
# label -> what a relative 1e-13 is put on: (equation, parameter) or ('column', name)
SENSITIVE = {
    'ComputeAveragePressure': ('column', 'p'), 'MomentumEquation': ('column', 'p'),
    'MomentumEquationPressureGradient': ('MomentumEquationPressureGradient', 'pb'), 'EDACEquation': ('EDACEquation', 'cs'),
    'MomentumEquationViscosity': ('MomentumEquationViscosity', 'nu'),
    'MomentumEquationArtificialViscosity': ('MomentumEquationArtificialViscosity', 'alpha'),
    'MomentumEquationArtificialStress': ('column', 'rho'), 'XSPHCorrection': ('XSPHCorrection', 'eps'),
    'external_group': ('MomentumEquationViscosity', 'nu'), 'internal_group': ('MomentumEquationPressureGradient', 'pb'),
    'internal_solid_group': ('EDACEquation', 'nu'),
}
NU_, ENU_ = 0.375, 0.21875          # nu of the viscosity and of the pressure damping in every table
# wrong arithmetic (--mutants): name -> (equation, method, text, replacement)
ARITH = (
    ('edac_nu swapped with nu', 'params', {'EDACEquation': {'nu': NU_}, 'MomentumEquationViscosity': {'nu': ENU_}}),
    ('Vi2 + Vj2 replaced by 2 Vi2 (pressure rate)', 'EDACEquation', 'loop', '(Vi2 + Vj2)*etaij', '(Vi2 + Vi2)*etaij'),
    ('Vi2 + Vj2 replaced by 2 Vi2 (internal gradient)', 'MomentumEquationPressureGradient', 'loop',
     'tmp = -pij * mi1 * (Vi2 + Vj2)', 'tmp = -pij * mi1 * (Vi2 + Vi2)'),
    ('Vi2 + Vj2 replaced by 2 Vi2 (pb term)', 'MomentumEquationPressureGradient', 'loop',
     'tmp = -self.pb * mi1 * (Vi2 + Vj2)', 'tmp = -self.pb * mi1 * (Vi2 + Vi2)'),
    ('pavg taken off one pressure only', 'MomentumEquationPressureGradient', 'loop', 'rhoi * (pj - pavg)', 'rhoi * (pj)'),
    ('rho_i / rho_j inverted in the pressure rate', 'EDACEquation', 'loop', 'rhoi/rhoj*self.cs', 'rhoj/rhoi*self.cs'),
    ('m_j replaced by m_i in the pressure rate', 'EDACEquation', 'loop', 'self.cs*s_m[s_idx]', 'self.cs*d_m[d_idx]'),
    ('rho_j p_i + rho_i p_j with the densities swapped (external)', 'MomentumEquation', 'loop',
     'pij = rhoj * p_i + rhoi * p_j', 'pij = rhoi * p_i + rhoj * p_j'),
    ('EPS dropped from the viscosity', 'MomentumEquationViscosity', 'loop', 'Fij/(R2IJ + EPS)', 'Fij/(R2IJ)'),
    ('etaij without the factor 2', 'MomentumEquationViscosity', 'loop', 'etaij = 2 * (etai', 'etaij = (etai'),
    ('HIJ dropped from muij', 'MomentumEquationArtificialViscosity', 'loop', 'muij = (HIJ * vijdotrij)', 'muij = (vijdotrij)'),
    ('vijdotrij < 0 changed to <= 0', 'MomentumEquationArtificialViscosity', 'loop', 'if vijdotrij < 0:', 'if vijdotrij <= 0:'),
    ('artificial stress: uhat_j - u_j replaced by uhat_i - u_i', 'MomentumEquationArtificialStress', 'loop',
     'Axxj = rhoj*uj*(uhatj - uj)', 'Axxj = rhoj*uj*(uhati - ui)'),
    ('artificial stress: the factor 0.5 of Ay dropped', 'MomentumEquationArtificialStress', 'loop', 'Ay = 0.5*(', 'Ay = ('),
    ('XSPH: RHOIJ1 squared', 'XSPHCorrection', 'loop', 'WIJ*RHOIJ1', 'WIJ*RHOIJ1*RHOIJ1'),
    ('XSPH: u not added behind the loop', 'XSPHCorrection', 'post_loop', 'd_ax[d_idx] += d_u[d_idx]', 'd_ax[d_idx] += 0.0'),
    ('tdamp ramp with +1/2 for -1/2', 'MomentumEquation', 'post_loop', '(-0.5 + t/self.tdamp)', '(0.5 + t/self.tdamp)'),
    ('t < tdamp changed to t <= tdamp', 'MomentumEquation', 'post_loop', 'if t < self.tdamp:', 'if t <= self.tdamp:'),
    ('nnbr > 0 changed to nnbr > 1', 'ComputeAveragePressure', 'post_loop', 'if d_nnbr[d_idx] > 0:', 'if d_nnbr[d_idx] > 1:'),
    ('the self pair left out (pavg, nnbr, the summed density)', 'no_self'),
)
EQUIVALENT = ('vijdotrij < 0 changed to <= 0', 't < tdamp changed to t <= tdamp', 'nnbr > 0 changed to nnbr > 1')


# -- the two arithmetics: those of the gas-dynamics generator, with the sine of the tdamp ramp ---------------------------
def _vs_sin(x):
    if isinstance(x, P.VS):
        r = mp.sin(x.v)
        return P.VS(r, x.s * abs(mp.cos(x.v)) + abs(r))
    return mp.sin(x)


class Double(P.Double):
    def bind(self):
        RE.sin = RT.sin = math.sin

    def unbind(self):
        unbind()


class Digits50(P.Digits50):
    def __init__(self, kname, dim):
        self.kk, self.dim = KERNEL_IDS[kname], dim
        self.fac0 = mp.mpf(getattr(RK, kname)(dim=dim).fac)       # the double constant is the definition

    def bind(self):
        RE.sin = RT.sin = _vs_sin

    def unbind(self):
        unbind()


class GuardInverted(Double):
    """double, with the kernel's ``rij > 1e-12`` inverted: no gradient above it, dwdq h1 / rij below (raises at 0)"""

    def __init__(self, kname, dim):
        Double.__init__(self, kname, dim)
        self.kk, self.dim = KERNEL_IDS[kname], dim

    def kern(self, xij, rij, h):
        w = self.k.kernel(xij, rij, h)
        if rij > 1e-12:
            return w, [0.0, 0.0, 0.0], 0.0
        h1 = 1.0 / h
        fac = self.k.fac * h1 ** self.dim
        tmp = float(H.mp_kernel(self.kk, rij * h1)[1]) * fac * h1 / rij
        return w, [tmp * c for c in xij], 0.0


class KernelOf(object):
    """SPH_KERNEL of a loop_all: ``gradient`` in the arithmetic N"""

    def __init__(self, N):
        self.N = N

    def gradient(self, xij, rij, h, grad):
        grad[:] = self.N.kern(list(xij), rij, h)[1]


def unbind():
    RE.sin = RT.sin = math.sin


# -- the sweep of a group ------------------------------------------------------------------------------------------------
def neighbours(table):
    """per (destination, source array): the lists of the reference's criterion in double; asserted inside the cluster"""
    rs = RADIUS[table['kernel']]
    out = {}
    A = table['arrays']
    D = A[table['dest']]
    for sn in table['sources']:
        S = A[sn]
        lists = []
        for i in range(len(D['x'])):
            d2 = sum((D[c][i] - S[c]) ** 2 for c in 'xyz')
            hit = (d2 < (rs * D['h'][i]) ** 2) | (d2 < (rs * S['h']) ** 2)
            assert np.all(S['cl'][hit] == D['cl'][i]), (table['key'], sn, i, 'a neighbour outside the cluster')
            assert np.all(hit[S['cl'] == D['cl'][i]]), (table['key'], sn, i, 'a cluster member is no neighbour')
            lists.append([int(j) for j in np.nonzero(hit)[0]])
        out[(table['dest'], sn)] = lists
    return out


def gsweep(table, N, classes=None, params=None, scale_cols=None, no_self=False, guard=None, catch=False):
    """the group of a table in the arithmetic N.  Returns cols, S (50 digits only), recs (per destination: the traces
    of its loop calls as (source, j, equation, trace) and of its post_loop calls).  ``guard``: the arithmetic whose
    gradient replaces DWIJ of every pair but the self pair (the kernel's guard inverted); ``catch``: a ZeroDivisionError
    marks the destination in ``raised`` and the sweep goes on (a mutant that raises where the reference does not)"""
    dest = table['dest']
    eqs = []
    for e in table['group']:
        cls = (classes or {}).get(e['name'], table.get('classes', CLASSES)[e['name']])
        par = dict(e['params'], **((params or {}).get(e['name'], {})))
        eqs.append((e['name'], cls(dest=dest, sources=list(e['sources']), **par)))
    outs = table['outputs']
    hooks = table.get('hooks', {})       # equation name -> called with the trace of each of its loop calls
    N.bind()
    try:
        A = {}
        for name, cols in table['arrays'].items():
            A[name] = dict((c, P.RecList(N.conv(float(x)) * (scale_cols.get((name, c), 1) if scale_cols else 1) for x in v))
                           for c, v in cols.items() if c != 'cl')
        D = A[dest]
        n = len(D['x'])
        nb = table['nbrs']
        mpmode = N.name == 'mp'
        bases = []
        for c in outs:
            if c.split('__')[0] not in bases:
                bases.append(c.split('__')[0])
        S = dict((c, [mp.mpf(0)] * len(D[c])) for c in bases) if mpmode else None
        recs = [dict(loop=[], post=[]) for _ in range(n)]
        raised = np.zeros(n, bool)
        t = N.conv(table['t'])

        def call(eq, meth, i, extra=None, sn=None, j=None, trace=False):
            fn = getattr(eq, meth, None)
            if fn is None:
                return None
            ns = dict(d_idx=i, s_idx=j, t=t, dt=0.0)
            ns.update(extra or {})
            args = []
            for a in P._args(fn):
                if a[:2] == 'd_' and a != 'd_idx':
                    args.append(D[a[2:]])
                elif a[:2] == 's_' and a != 's_idx':
                    args.append(A[sn][a[2:]])
                else:
                    args.append(ns[a])
            try:
                if trace:
                    return P.traced_call(fn, args)
                fn(*args)
            except ZeroDivisionError:
                if not catch:
                    raise
                raised[i] = True
            return None

        for i in range(n):
            for name, eq in eqs:
                call(eq, 'initialize', i)
        if mpmode:
            for c in S:
                D[c].rec = S[c]
        for sn in table['sources']:          # loop_all (acceleration_eval_cython.mako:62-83), behind initialize
            for name, eq in eqs:
                if hasattr(eq, 'loop_all') and sn in eq.sources:
                    for i in range(n):
                        nbrs = [j for j in nb[(dest, sn)][i]]
                        call(eq, 'loop_all', i, dict(SPH_KERNEL=KernelOf(N), NBRS=nbrs, N_NBRS=len(nbrs)), sn)
        need = set()
        for name, eq in eqs:
            if hasattr(eq, 'loop'):
                need |= set(P._args(eq.loop))
        if mpmode:
            for c in S:
                D[c].rec = S[c]
        for sn in table['sources']:
            Sa = A[sn]
            here = [(name, eq) for name, eq in eqs if hasattr(eq, 'loop') and sn in eq.sources]
            for i in range(n):
                for j in nb[(dest, sn)][i]:
                    if no_self and sn == dest and j == i:
                        continue
                    sym = P.symbols(need, N, D, Sa, i, j)
                    if guard is not None and not (sn == dest and j == i):
                        try:
                            sym['DWIJ'] = guard.kern(sym['XIJ'], sym['RIJ'], sym['HIJ'])[1]
                        except ZeroDivisionError:
                            raised[i] = True
                            continue
                    sym.update(table.get('symbols', {}))
                    for name, eq in here:
                        # (the equations of a pair share its symbols, as in the reference's generated loop: what
                        # GradientCorrection writes into DWIJ the equations behind it read)
                        tr = call(eq, 'loop', i, sym, sn, j, trace=True)
                        if name in hooks and tr is not None:
                            hooks[name](tr)
                        recs[i]['loop'].append((sn, j, name, tr))
        for c in D:
            D[c].rec = None
        if mpmode:
            for c in D:
                for i in range(len(D[c])):
                    D[c][i] = P.VS(D[c][i], S[c][i] if c in S else 0)
        for i in range(n):
            for name, eq in eqs:
                tr = call(eq, 'post_loop', i, trace=True)
                if tr is not None:
                    recs[i]['post'].append((name, tr))
        cols = {}
        Sout = {}
        for c in outs:
            b, _, k = c.partition('__')          # a strided property component by component: m_mat__4 = m_mat[4::9]
            stride = len(D[b]) // n
            vals = [P.VS.of(x) if mpmode else float(x) for x in list(D[b])[(int(k) if k else 0)::stride]]
            if mpmode:
                cols[c] = [x.v for x in vals]
                Sout[c] = [mp.mpf(float(np.float32(float(x.s)))) for x in vals]
            else:
                cols[c] = np.array(vals, dtype=np.float64)
        if not scale_cols:
            same = all(all(float(P._val(a)) == float(b) for a, b in zip(A[name][c], table['arrays'][name][c]))
                       for name in A for c in A[name] if not (name == dest and c in bases))
            assert same, (table['key'], 'the reference wrote an input column')
        if mpmode and 'scales' in table:     # a family whose kernel associates a sum differently states the scale of that sum
            net = dict((c, list(v)) for c, v in Sout.items())
            table['scales'](table, Sout, recs)
            # a stated scale is the sum of |product| where the net one is the sum of |increment|: never below it (up to
            # the float32 it is stored in), and a column nothing states stays as it was
            assert set(Sout) == set(net) and all(len(Sout[c]) == len(net[c]) for c in net), table['key']
            assert all(a >= b * (1 - mp.mpf(2) ** -20) for c in net for a, b in zip(Sout[c], net[c])), (table['key'], 'a stated scale below the net-increment scale')
        return dict(cols=cols, S=Sout if mpmode else None, recs=recs, raised=raised)
    finally:
        N.unbind()


def writes(table):
    """the destination columns the group's methods assign (``d_<c>[d_idx] =``, ``+=``, ``/=``), from the reference's text"""
    found = []
    for e in table['group']:
        cls = CLASSES[e['name']]
        for meth in ('initialize', 'loop', 'post_loop'):
            fn = getattr(cls, meth, None)
            if fn is None:
                continue
            for ln in inspect.getsource(fn).split('\n'):
                ln = ln.strip()
                if ln.startswith('d_') and '[d_idx]' in ln.split('=')[0] and '=' in ln:
                    c = ln[2:ln.index('[')]
                    if c not in found:
                        found.append(c)
    return tuple(c for c in OUTPUT_ORDER if c in found)


# -- branches and margins ------------------------------------------------------------------------------------------------
def signature(rec):
    parts = ['%s:%d:%s:%s%s' % (sn, j, name, ','.join(str(k) for k in sorted(tr.lines)), getattr(tr, 'extra', ''))
             for sn, j, name, tr in rec['loop']]
    parts += ['post:%s:%s' % (name, ','.join(str(k) for k in sorted(tr.lines))) for name, tr in rec['post']]
    return ' '.join(parts)


def decisions(table, run, i):
    """(branch names, smallest relative distance of a decision from its threshold) of destination i"""
    names, margin = set(), float('inf')

    def far(x, thr, rel=None):
        nonlocal margin
        margin = min(margin, abs(float(x) - thr) / (abs(thr) if rel is None else rel))

    A = table['arrays']
    D = A[table['dest']]
    group = dict((e['name'], e) for e in table['group'])
    seen = set()
    navg = 0
    for sn, j, name, tr in run['recs'][i]['loop']:
        Sa = A[sn]
        self_pair = sn == table['dest'] and j == i
        if name == 'ComputeAveragePressure':
            navg += 1
        if self_pair:
            continue
        if (sn, j) not in seen:
            seen.add((sn, j))
            rij = math.sqrt(sum((D[c][i] - Sa[c][j]) ** 2 for c in 'xyz'))
            if rij == 0.0:
                if D['h'][i] != Sa['h'][j]:
                    names.add('coincident_unequal_h')
            else:
                far(rij, 1e-12)
                if rij <= 1e-12:
                    names.add('rij_below_1e-12')
                elif rij < 1e-9:
                    names.add('rij_above_1e-12')
        if name == 'MomentumEquationArtificialViscosity':
            L = tr.locals
            dot = float(L['vijdotrij'])
            if dot != 0.0:
                far(dot, 0.0, P._norm(L['VIJ']) * P._norm(L['XIJ']))
                names.add('approaching' if dot < 0 else 'receding')
        if name == 'EDACEquation' and D['p'][i] == Sa['p'][j]:
            names.add('p_equal')
    if 'ComputeAveragePressure' in group:
        own = table['dest'] in group['ComputeAveragePressure']['sources']
        names.add('nnbr_zero' if navg == 0 else 'nnbr_self_only' if (navg == 1 and own) else 'nnbr_positive')
    if 'XSPHCorrection' in group and group['XSPHCorrection']['params']['eps'] == 0.0:
        names.add('eps_zero')
    for name in ('MomentumEquation', 'MomentumEquationPressureGradient'):
        if name in group:
            td, t = group[name]['params']['tdamp'], table['t']
            if td == 0.0:
                far(t, 0.0, 1.0)
                names.add('tdamp_zero')
            elif t == td:
                names.add('tdamp_equal')
            else:
                far(t, td)
                names.add('tdamp_ramp' if t < td else 'tdamp_past')
    return names, margin


def mutant_class(eqname, meth, old, new, classes=CLASSES):
    cls = classes[eqname]
    src = textwrap.dedent(inspect.getsource(getattr(cls, meth)))
    assert src.count(old) == 1, (eqname, meth, old, src.count(old))
    ns = {}
    mod = sys.modules[cls.__module__]
    exec(compile(src.replace(old, new), '<%s.%s changed>' % (eqname, meth), 'exec'), mod.__dict__, ns)
    return type(cls.__name__, (cls,), {meth: ns[meth]})


# -- tables --------------------------------------------------------------------------------------------------------------
def particle(rng, dim, arr, off, h, **kw):
    rho = float(rng.uniform(0.75, 1.5))
    m = float(rng.uniform(0.75, 1.5)) * 2.0 ** -6
    q = dict(arr=arr, off=off, h=h, rho=rho, m=m, V=rho / m * float(rng.uniform(0.9, 1.1)), p=float(rng.uniform(0.5, 2.0)),
             pavg=float(rng.uniform(-0.5, 0.25)))
    vel, hat = rng.uniform(-1, 1, 3), rng.uniform(0.25, 0.75, 3) * rng.choice([-1.0, 1.0], 3)
    for k, c in enumerate('uvw'):
        q[c] = float(vel[k]) if k < dim else 0.0
        q[c + 'hat'] = float(vel[k] + hat[k]) if k < dim else 0.0
    q.update(kw)
    return q


def _off(dim, r):
    return tuple(r * c for c in DIRS[dim])


def clusters(rng, dim, uh, kind, other='fluid'):
    """the clusters of one table; ``other``: the array of a pair's second particle"""
    cl = []

    def hh():
        return H0 if uh else P._h(rng)

    def pair(r, hi=None, hj=None, kwa=None, kwb=None, arr=None):
        hi, hj = hi or hh(), hj or hh()
        cl.append([particle(rng, dim, 'fluid', _off(dim, 0.0), hi, **(kwa or {})),
                   particle(rng, dim, arr or other, _off(dim, r), hj, **(kwb or {}))])

    def sep(hi, hj):
        return min(float(rng.uniform(0.3, 1.5)) * min(hi, hj), 0.23)

    d = DIRS[dim]
    for k in range(8):
        hi, hj = hh(), hh()
        pair(sep(hi, hj), hi, hj, arr=('fluid' if k % 3 == 2 else None))
    for k in range(2):                  # strongly approaching and strongly receding along the line of centres
        s = 2.0 if k == 0 else -2.0
        pair(0.09375, kwa=dict(zip('uvw', [-s * c for c in d])), kwb=dict(zip('uvw', [s * c for c in d])))
    for k in range(2):                  # one destination between two partners, one approaching, one receding
        cl.append([particle(rng, dim, 'fluid', _off(dim, 0.0), hh(), u=0.0, v=0.0, w=0.0),
                   particle(rng, dim, other, _off(dim, 0.0625), hh(), **dict(zip('uvw', [0.5 * c for c in d]))),
                   particle(rng, dim, 'fluid', _off(dim, -0.046875), hh(), **dict(zip('uvw', [0.25 * c for c in d])))])
    pair(2.0 ** -40)
    pair(2.0 ** -40)
    pair(2.0 ** -39)
    pair(2.0 ** -39)
    if uh:
        pair(0.0)
    else:
        pair(0.0, hi=2.0 ** -4 * 1.5, hj=2.0 ** -4 * 2.5)
        pair(0.0, hi=2.0 ** -4 * 3.5, hj=2.0 ** -4 * 2.0)
        pair(0.1875, hi=2.0 ** -4, hj=2.0 ** -2)           # h ratio 4
    if kind in ('edac', 'group'):
        pair(0.078125, kwa=dict(p=1.25), kwb=dict(p=1.25))
        pair(0.0625, kwa=dict(p=0.75), kwb=dict(p=0.75))
    if kind in ('avgp', 'group'):
        cl.append([particle(rng, dim, 'fluid', _off(dim, 0.0), hh())])          # alone
        cl.append([particle(rng, dim, 'fluid', _off(dim, 0.0), hh())])
    if kind == 'stress':                # the base equation's pressure terms small next to the stress
        for c in cl:
            for q in c:
                q['p'] *= 2.0 ** -8
                q['pavg'] *= 2.0 ** -8
    return cl


def columns_of(group):
    """the columns the group's methods name (d_<c>, s_<c>) next to the ones every pair needs, in the order of COLUMNS"""
    used = set(('x', 'y', 'z', 'u', 'v', 'w', 'h', 'm', 'rho', 'p'))
    for e in group:
        for meth in ('initialize', 'loop', 'post_loop'):
            fn = getattr(CLASSES[e['name']], meth, None)
            for a in (P._args(fn) if fn is not None else ()):
                if a[:2] in ('d_', 's_') and a not in ('d_idx', 's_idx'):
                    used.add(a[2:])
    return tuple(c for c in COLUMNS if c in used)


def build_table(key, label, cfg, form, cl, group, dest, t, seed):
    cname, dim, kname = cfg
    rng = np.random.default_rng(seed + 1777)
    sources = []
    for e in group:
        for s in e['sources']:
            if s not in sources:
                sources.append(s)
    names = [dest] + [s for s in sources if s != dest]
    arrays = {}
    for name in names:
        rows = [(c, q) for c, cluster in enumerate(cl) for q in cluster if q['arr'] == name]
        cols = dict((k, np.zeros(len(rows))) for k in columns_of(group))
        cols['cl'] = np.array([c for c, q in rows])
        for r, (c, q) in enumerate(rows):
            for k in columns_of(group):
                if k in 'xyz':
                    cols[k][r] = (c if k == 'x' else 0.0) + q['off']['xyz'.index(k)]
                elif k in q:
                    cols[k][r] = q[k]
                else:
                    cols[k][r] = float(rng.uniform(-1, 1))        # garbage: must be overwritten
        arrays[name] = cols
    table = dict(key=key, label=label, config=cname, dim=dim, kernel=kname, form=form, group=group, dest=dest,
                 sources=tuple(sources), arrays=arrays, t=t)
    table['outputs'] = writes(table)
    table['nbrs'] = neighbours(table)
    return table


G3 = dict(gx=0.5, gy=-0.25, gz=0.125)
C0, NU, ENU, RHO0, PB, ALPHA = 1.5, NU_, ENU_, 1.0, 1.25, 0.75


def _eq(name, sources, **params):
    return dict(name=name, sources=list(sources), params=params)


def all_tables():
    tables = []
    for ci, cfg in enumerate(CONFIGS):
        cname, dim, kname = cfg
        for fi, form in enumerate(('uh', 'vh')):
            uh = form == 'uh'
            rng = np.random.default_rng(5200 + 10 * ci + fi)
            seed = [100 * ci + 50 * fi]

            def add(label, kind, cl, group, t, dest='fluid'):
                seed[0] += 1
                tables.append(build_table('%s/%s/%s/%s' % (label, kind, cname, form), label, cfg, form, cl, group, dest, t, seed[0]))

            f, fs = ['fluid'], ['fluid', 'solid']
            add('ComputeAveragePressure', 'alone', clusters(rng, dim, uh, 'avgp'), [_eq('ComputeAveragePressure', f)], 0.25)
            add('ComputeAveragePressure', 'density', clusters(rng, dim, uh, 'avgp'),
                [_eq('SummationDensity', f), _eq('ComputeAveragePressure', f)], 0.25)
            if not uh:
                add('ComputeAveragePressure', 'other', clusters(rng, dim, uh, 'avgp', other='solid'),
                    [_eq('ComputeAveragePressure', ['solid'])], 0.25)
            add('MomentumEquation', 'alone', clusters(rng, dim, uh, ''),
                [_eq('MomentumEquation', f, c0=C0, tdamp=1.0 if uh else 0.25, **G3)], 0.25)
            add('MomentumEquationPressureGradient', 'alone', clusters(rng, dim, uh, ''),
                [_eq('MomentumEquationPressureGradient', f, pb=PB, tdamp=0.25 if uh else 0.0, **G3)], 0.5)
            add('EDACEquation', 'alone', clusters(rng, dim, uh, 'edac'), [_eq('EDACEquation', f, cs=C0, nu=ENU, rho0=RHO0)], 0.25)
            add('MomentumEquationViscosity', 'edac', clusters(rng, dim, uh, ''),
                [_eq('EDACEquation', f, cs=C0, nu=ENU, rho0=RHO0), _eq('MomentumEquationViscosity', f, nu=NU)], 0.25)
            add('MomentumEquationArtificialViscosity', 'edac', clusters(rng, dim, uh, ''),
                [_eq('EDACEquation', f, cs=C0, nu=ENU, rho0=RHO0), _eq('MomentumEquationArtificialViscosity', f, c0=C0, alpha=ALPHA)], 0.25)
            add('MomentumEquationArtificialStress', 'gradient', clusters(rng, dim, uh, 'stress'),
                [_eq('MomentumEquationPressureGradient', f, pb=2.0 ** -8, tdamp=0.25, gx=0.0, gy=0.0, gz=0.0),
                 _eq('MomentumEquationArtificialStress', f)], 0.5)
            add('XSPHCorrection', 'momentum', clusters(rng, dim, uh, ''),
                [_eq('MomentumEquation', f, c0=C0, tdamp=1.0, **G3), _eq('XSPHCorrection', f, eps=0.5)], 0.25)
            if uh:
                add('XSPHCorrection', 'eps0', clusters(rng, dim, uh, ''),
                    [_eq('MomentumEquation', f, c0=C0, tdamp=0.0, **G3), _eq('XSPHCorrection', f, eps=0.0)], 0.25)
            # the scheme's default force groups (EDACScheme with nu > 0, alpha = 0): the constant-flag kernels
            add('external_group', 'default', clusters(rng, dim, uh, 'group'),
                [_eq('MomentumEquation', f, c0=C0, tdamp=1.0 if uh else 0.0, **G3), _eq('MomentumEquationViscosity', f, nu=NU),
                 _eq('EDACEquation', f, cs=C0, nu=ENU, rho0=RHO0), _eq('XSPHCorrection', f, eps=0.5)], 0.25)
            add('internal_group', 'default', clusters(rng, dim, uh, 'group'),
                [_eq('MomentumEquationPressureGradient', f, pb=PB, tdamp=0.5 if uh else 0.25, **G3),
                 _eq('MomentumEquationViscosity', f, nu=NU), _eq('MomentumEquationArtificialStress', f),
                 _eq('EDACEquation', f, cs=C0, nu=ENU, rho0=RHO0)], 0.5)
            # fluid <- {fluid, solid}, the source lists of EDACScheme (alpha > 0): the run-time-flag kernel
            add('internal_solid_group', 'solid', clusters(rng, dim, uh, 'group', other='solid'),
                [_eq('MomentumEquationPressureGradient', fs, pb=PB, tdamp=1.0, **G3),
                 _eq('MomentumEquationArtificialViscosity', fs, c0=C0, alpha=ALPHA), _eq('MomentumEquationViscosity', f, nu=NU),
                 _eq('MomentumEquationArtificialStress', f), _eq('EDACEquation', fs, cs=C0, nu=ENU, rho0=RHO0)], 0.25)
            # the other form of the two tables above that have one only (drawn from a stream of their own)
            rng = np.random.default_rng(5300 + 10 * ci + fi)
            if uh:
                add('ComputeAveragePressure', 'other', clusters(rng, dim, uh, 'avgp', other='solid'),
                    [_eq('ComputeAveragePressure', ['solid'])], 0.25)
            else:
                add('XSPHCorrection', 'eps0', clusters(rng, dim, uh, ''),
                    [_eq('MomentumEquation', f, c0=C0, tdamp=0.0, **G3), _eq('XSPHCorrection', f, eps=0.0)], 0.25)
    return tables


# -- a table through both arithmetics ------------------------------------------------------------------------------------
def run_table(table, N2, Nmp):
    ref = gsweep(table, N2)
    with mp.workdps(50):
        tru = gsweep(table, Nmp)
        n = len(ref['recs'])
        res = dict(ref=ref, tru=tru, kref={}, names=[], margin=np.zeros(n), sig=np.zeros(n, np.int32), mpok=np.zeros(n, bool))
        for c in table['outputs']:
            res['kref'][c] = P.kmeasure(ref['cols'][c], tru['cols'][c], tru['S'][c])
        for i in range(n):
            names, margin = table.get('decide', decisions)(table, ref, i)
            res['names'].append(names)
            res['margin'][i] = margin
            s = signature(ref['recs'][i])
            res['sig'][i] = P._sig_id(s)
            res['mpok'][i] = s == signature(tru['recs'][i])
    return res


def worst_k(table, res):
    return np.max(np.array([res['kref'][c] for c in table['outputs']]), axis=0)


def bound_of(table, res, k_eq):
    well = res['mpok'] & (worst_k(table, res) <= WELL)
    flat = max(FACTOR, FACTOR * k_eq)
    return dict((c, np.where(res['mpok'] & (res['kref'][c] <= WELL), flat, FACTOR * res['kref'][c])) for c in table['outputs']), well


def leaves_bound(table, res, other, k_eq, rows=None, only_well=False):
    """the destinations in which the columns of the run ``other`` (double) leave the bound around the 50-digit truth"""
    bound, well = bound_of(table, res, k_eq)
    out = np.zeros(len(well), bool)
    with mp.workdps(50):
        for c in table['outputs']:
            k = P.kmeasure(other['cols'][c], res['tru']['cols'][c], res['tru']['S'][c])
            out |= ~(k <= bound[c])
    if only_well:
        out &= well
    return out if rows is None else out & rows


def numerics(tables):
    nums = {}
    for table in tables:
        cfg = (table['kernel'], table['dim'])
        if cfg not in nums:
            nums[cfg] = (Double(*cfg), Digits50(*cfg), GuardInverted(*cfg))
    return nums


def evaluate(tables, quiet=False):
    """every table through both arithmetics and items 1, 2, 4, 5: (results, k_eq, branches)"""
    nums = tables[0].get('numerics', numerics)(tables)
    results = {}
    for table in tables:
        cfg = (table['kernel'], table['dim'])
        results[table['key']] = run_table(table, *nums[cfg][:2])
        if not quiet:
            print(table['key'], sum(len(v['x']) for v in table['arrays'].values()), 'particles', flush=True)
    k_eq, branches = {}, Counter()
    labels = []
    for table in tables:
        if table['label'] not in labels:
            labels.append(table['label'])
    for label in labels:
        good, bad, total = [0.0], 0, 0
        for table in tables:
            if table['label'] != label:
                continue
            res = results[table['key']]
            for names in res['names']:
                branches.update(names)
            assert np.all(res['margin'] >= MARGIN), (table['key'], 'a decision within 1e-3 of its threshold',
                                                     np.nonzero(res['margin'] < MARGIN)[0], res['margin'].min())
            well = res['mpok'] & (worst_k(table, res) <= WELL)
            bad += int(np.sum(~well))
            total += well.size
            for c in table['outputs']:
                k = res['kref'][c][res['mpok']]
                good.extend(k[k <= WELL])
        assert bad * 10 <= total, (label, bad, total)
        k_eq[label] = float(max(good))
        assert k_eq[label] <= WELL
        print('K_eq %-36s %8.3f   (%d of %d destinations not well-conditioned)' % (label, k_eq[label], bad, total), flush=True)
    return results, k_eq, branches, nums


def mutant_run(table, nums, spec):
    """the double run of a table under one entry of MUTANTS / ARITH (``raised``: the destinations in which it raises
    where the reference does not); None where the table has nothing of it"""
    N2, _, NG = nums[(table['kernel'], table['dim'])]
    have = [e['name'] for e in table['group']]
    if spec[0] == 'kernel':
        return gsweep(table, N2, guard=NG, catch=True)
    if spec[0] == 'no_self':
        return gsweep(table, N2, no_self=True, catch=True)
    if spec[0] == 'params':
        par = dict((k, v) for k, v in spec[1].items() if k in have)
        return gsweep(table, N2, params=par, catch=True) if par else None
    eqname, meth, old, new = spec
    hit = [n for n in have if (eqname == '*' and n in ('MomentumEquation', 'MomentumEquationPressureGradient')) or n == eqname]
    if not hit:
        return None
    return gsweep(table, N2, classes=dict((n, mutant_class(n, meth, old, new, table.get('classes', CLASSES))) for n in hit), catch=True)


def caught_rows(table, res, other, k_eq, rows=None):
    out = leaves_bound(table, res, other, k_eq) | other['raised']
    return out if rows is None else out & rows


def build(mod=None):
    """every table of ``mod`` (this module, or make_wcsph_options_pair_golden) through items 1..6 and into the arrays of
    the file"""
    mod = mod or sys.modules[__name__]
    P.SIGS[:] = ['']
    tables = mod.all_tables()
    results, k_eq, branches, nums = evaluate(tables)
    missing = dict((b, branches[b]) for b in mod.REQUIRED if branches[b] < 2)
    assert not missing, ('taken fewer than twice', missing)

    # 3: observability
    observed = Counter()
    for b in mod.REQUIRED:
        for table in tables:
            res = results[table['key']]
            rows = np.array([b in names for names in res['names']])
            if not rows.any():
                continue
            other = mod.mutant_run(table, nums, mod.MUTANTS[b])
            if other is None:
                continue
            observed[b] += int(caught_rows(table, res, other, k_eq[table['label']], rows).sum())
    unobserved = dict((b, observed[b]) for b in mod.REQUIRED if observed[b] < 2 and b not in mod.UNOBSERVABLE)
    assert not unobserved, ('not observable', unobserved)
    assert all(observed[b] == 0 for b in mod.UNOBSERVABLE), observed
    print('observable in', dict(observed), flush=True)

    # 6: sensitivity
    sensitive = Counter()
    for table in tables:
        res = results[table['key']]
        N2 = nums[(table['kernel'], table['dim'])][0]
        what, name = mod.SENSITIVE[table['label']]
        if what == 'column':
            other = gsweep(table, N2, scale_cols=dict(((a, name), 1 + 1e-13) for a in table['arrays']))
        else:
            par = [e for e in table['group'] if e['name'] == what][0]['params']
            other = gsweep(table, N2, params={what: {name: par[name] * (1 + 1e-13)}})
        sensitive[table['label']] += int(leaves_bound(table, res, other, k_eq[table['label']], only_well=True).sum())
    assert all(sensitive[e] >= 1 for e in mod.LABELS), sensitive
    print('sensitive to a part in 1e13:', dict(sensitive), flush=True)

    out = {}
    keys = []
    for table in tables:
        # few members per table (an archive member costs more than a short column holds): the columns of an array as
        # rows of in/<array> (a strided property component by component: gradrho__1 = gradrho[1::3]); S and kref as
        # the two planes of f32; everything that is an integer, a flag or a name in the spec
        key = table['key']
        keys.append(key)
        res = results[key]
        outs = table['outputs']
        bases = set(c.split('__')[0] for c in outs)
        incols = {}
        for name, cols in table['arrays'].items():
            n = len(cols['x'])
            rows, incols[name] = [], []
            for c in cols:
                if c == 'cl' or (name == table['dest'] and c in bases):
                    continue
                stride = len(cols[c]) // n if n else 1
                for k in range(stride):
                    incols[name].append(c if stride == 1 else '%s__%d' % (c, k))
                    rows.append(cols[c][k::stride])
            out['%s/in/%s' % (key, name)] = np.array(rows)
        nbr = dict((sn, table['nbrs'][(table['dest'], sn)]) for sn in table['sources'])
        out[key + '/spec'] = np.array(json.dumps({
            'label': table['label'], 'config': table['config'], 'dim': table['dim'], 'kernel': table['kernel'], 'form': table['form'],
            'group': table['group'], 'dest': table['dest'], 'sources': list(table['sources']), 'arrays': list(table['arrays']),
            'in': incols, 'outputs': list(outs), 't': table['t'],
            'cl': dict((name, [int(c) for c in cols['cl']]) for name, cols in table['arrays'].items()), 'nbr': nbr,
            'names': [sorted(n) for n in res['names']], 'sig': [int(k) for k in res['sig']],
            'mpok': [int(k) for k in res['mpok']]}, separators=(',', ':')))
        with mp.workdps(50):
            pairs = [[P._split(x) for x in res['tru']['cols'][c]] for c in outs]
            out[key + '/ref'] = np.array([res['ref']['cols'][c] for c in outs])
            out[key + '/mp'] = np.array([[p[0] for p in row] for row in pairs])
            # the remainder with a 24-bit mantissa, as a double: a remainder of a value of 1e-24 is below float32's range
            mant, expo = np.frexp(np.array([[p[1] for p in row] for row in pairs]))
            out[key + '/mplo'] = np.ldexp(np.round(mant * 2.0 ** 24) / 2.0 ** 24, expo)
            with np.errstate(over='ignore'):
                out[key + '/f32'] = np.array([[[float(x) for x in res['tru']['S'][c]] for c in outs],    # S
                                              [res['kref'][c] for c in outs]]).astype(np.float32)        # kref
        out[key + '/margin'] = res['margin'].astype(np.float32)
    out['tables'] = np.array(json.dumps(keys))
    out['sigs'] = np.array(json.dumps(P.SIGS))
    out['meta/branches'] = np.array(json.dumps(dict((b, int(branches[b])) for b in sorted(branches))))
    out['meta/required'] = np.array(json.dumps(list(mod.REQUIRED)))
    out['meta/unobservable'] = np.array(json.dumps(list(mod.UNOBSERVABLE)))
    out['meta/observed'] = np.array(json.dumps(dict((b, int(observed[b])) for b in mod.REQUIRED)))
    out['meta/sensitive'] = np.array(json.dumps(dict(sensitive)))
    out['meta/k_eq'] = np.array(json.dumps(k_eq))
    out['meta/constants'] = np.array([WELL, FACTOR, MARGIN])
    return out


def arith_mutants(mod=None):
    """the wrong-arithmetic list: per entry of ARITH the number of destinations that leave the bound, in double"""
    mod = mod or sys.modules[__name__]
    P.SIGS[:] = ['']
    tables = mod.all_tables()
    results, k_eq, branches, nums = evaluate(tables, quiet=True)
    for entry in mod.ARITH:
        caught = 0
        for table in tables:
            other = mod.mutant_run(table, nums, entry[1:])
            if other is None:
                continue
            caught += int(caught_rows(table, results[table['key']], other, k_eq[table['label']]).sum())
        print('%-66s %s' % (entry[0], 'caught (%d)' % caught if caught else 'NOT caught'), flush=True)


def write(mod, path):
    if '--mutants' in sys.argv[1:]:
        return arith_mutants(mod)
    out = build(mod)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 1024 * 1024, size
    print('wrote', path, size // 1024, 'KiB')


def main():
    write(sys.modules[__name__], OUT)


if __name__ == '__main__':
    main()
