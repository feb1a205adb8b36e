#!/usr/bin/env python
"""The solid-mechanics pair families (``FamVGrad_T``, ``FamElastic_T``, pysph_amd/csrc/sph_fam_elastic.h), cluster by
cluster, from the REFERENCE's own classes -- ``VelocityGradient2D``, ``VelocityGradient3D``, ``ContinuityEquation``,
``MonaghanArtificialViscosity``, ``XSPHCorrection`` (basic_equations.py) and ``MomentumEquationWithStress``
(solid_mech/basic.py) -- executed as plain Python by the group sweep of make_edac_pair_golden.py (the layout, the scale
and the bound rule) with the machinery of make_gasd_pair_golden.py and the table builder of make_tvf_pair_golden.py:

    python tests/golden/make_elastic_pair_golden.py             ->  elastic_pair_edges.npz, elastic_tension_pair_edges.npz
                                                                    (the second: the tables of the tension token, below)
    python tests/golden/make_elastic_pair_golden.py --mutants   ->  the wrong-arithmetic list of tests/test_elastic_pair_edges.py

Layout.  As edac_pair_edges.npz: rows of isolated clusters 1 apart (one lone particle, pairs in both orders and
triples), every h in [2^-4, 2^-2], four configurations, a ``uh`` form (every h 2^-3, and ONE mass per array,
2^-6 5/4: what the records without h and m need) and a ``vh`` form (h and m unequal inside the clusters).  The array
constants ``wdeltap`` and ``n`` (``d_wdeltap[0]``, ``d_n[0]`` in the reference) are parameters of the stress equation in
the table's group; wdeltap > 0 is the kernel's value at r = h = 2^-3 rounded to float32.

Tables (one group each, the smallest the product takes into the family.  The product takes a group into the elastic
family only where MomentumEquationWithStress or MonaghanArtificialViscosity is in it: ContinuityEquation and
XSPHCorrection alone are the WCSPH family's, so they stand next to the stress equation):
    VelocityGradient2D/alone      the 2-D configuration, z = 3/8 everywhere and w garbage: neither may be read into v00..v11
    VelocityGradient3D/alone      both 3-D configurations
    ContinuityEquation/stress     [ContinuityEquation, MomentumEquationWithStress(wdeltap = -1)]: arho is the continuity's alone
    MomentumEquationWithStress/n4 n2 n1 n3 n2.5   alone, wdeltap > 0; n = 4 in every configuration, 2 and 3 in the first and
                                  third, 1 and 2.5 in the second and fourth (3 and 2.5 reach ``pow``)
    MomentumEquationWithStress/wzero              alone, wdeltap = 0, n = 4 (wdeltap = -1, the default of
                                  get_particle_array_elastic_dynamics, is in every table next to another equation)
    MonaghanArtificialViscosity/beta, /beta0      next to the stress equation with stresses and pressures of 2^-8
    XSPHCorrection/stress, /eps0  next to the stress equation: F_EXSPH without F_EAV, the run-time-flag kernel
    cf0_group/rates               [Continuity, Stress (wdeltap > 0, n = 4), MonaghanArtificialViscosity, XSPH]: FamElastic_T::CF0

Scale.  That of make_edac_pair_golden.py, with ONE exception: the kernel associates the stress sum differently from the
reference on purpose (sph_fam_elastic.h: S = sum m_j DWIJ and F = sum m_j f^n DWIJ wait for the destination's own tensors
in finish()), so the scale of au av aw under MomentumEquationWithStress is the sum of the absolute values of the
individual PRODUCTS of its statement, not of the statement's net increment: for au the nine pieces
|mb s0ka rhoa21 DWIJ[k]| + |mb s0kb rhob21 DWIJ[k]| + |mb art_stress0k DWIJ[k]|, k = 0, 1, 2 (plus |increment| of the
artificial viscosity where it shares the column).  The clusters ``stress_opposed`` and ``gradient_sum_zero`` show whether
the regrouping holds this scale.

Conditions 1..6 as in make_edac_pair_golden.py.  Decisions: vijdotxij against 0 relative to |VIJ| |XIJ|, RIJ against
1e-12; wdeltap is -1, 0 or of order one.  Branches without a comparison of their own: ``n_*`` and ``r_nonzero`` are seen
through n + 1 for n; ``wij_zero`` (a neighbour by the larger h whose kernel value and gradient under HIJ are 0: f = 0)
through n - 3 for n, which raises 0 ** negative under n = 1, 2, 2.5 (where the compiled reference writes inf * 0);
``beta_zero`` through beta + 1, ``beta_nonzero`` through beta = 0, ``eps_zero`` through eps + 1; ``stress_opposed``
(sigma_a / rho_a^2 = -sigma_b / rho_b^2 to the last bit, rho_a = 1, rho_b = 2) through rhob21 = rhoa21;
``gradient_sum_zero`` (sum m_j DWIJ of the middle particle of a symmetric triple is exactly 0 in double, asserted here)
through the partner's pressure with its sign changed; ``r_zero`` (every r_ij of the cluster 0 under wdeltap > 0) through
r00a + r00b + 1; ``lone_particle`` (the self pair only) through XSPH without u; the kernel's guard is inverted in the
kernel.
"""
import os
import sys

import numpy as np
import mpmath as mp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as MG  # noqa: E402,F401  (sets up the reference imports)
import make_edac_pair_golden as E  # noqa: E402  (the group sweep, the bound rule, the file)
import make_gasd_pair_golden as P  # noqa: E402
import make_tvf_pair_golden as TV  # noqa: E402  (build_table, mutant_run with several replacements)

from pysph.sph import basic_equations as RBE  # noqa: E402
from pysph.sph.solid_mech import basic as RS  # noqa: E402
from pysph.base import kernels as RK  # noqa: E402

OUT = os.path.join(HERE, 'elastic_pair_edges.npz')
WELL, FACTOR, MARGIN = E.WELL, E.FACTOR, E.MARGIN
CONFIGS = E.CONFIGS
DIRS = E.DIRS
H0 = E.H0
M0 = 2.0 ** -6 * 1.25
T = 0.25
_VG2, _VG3, _CONT, _ST, _MAV, _XS = ('VelocityGradient2D', 'VelocityGradient3D', 'ContinuityEquation', 'MomentumEquationWithStress',
                                     'MonaghanArtificialViscosity', 'XSPHCorrection')


class MomentumEquationWithStress(RS.MomentumEquationWithStress):
    """the reference's equation; the two array constants it reads arrive as parameters of the table's group and are
    put into one-element columns by the table builder"""

    def __init__(self, dest, sources, wdeltap=-1.0, n=4.0):
        RS.MomentumEquationWithStress.__init__(self, dest, sources)


MomentumEquationWithStress.__module__ = RS.__name__       # (a changed method is compiled in the reference's module)
CLASSES = {_VG2: RBE.VelocityGradient2D, _VG3: RBE.VelocityGradient3D, _CONT: RBE.ContinuityEquation,
           _ST: MomentumEquationWithStress, _MAV: RBE.MonaghanArtificialViscosity, _XS: RBE.XSPHCorrection}
LABELS = (_VG2, _VG3, _CONT, _ST, _MAV, _XS, 'cf0_group')
_S6 = ('s00', 's01', 's02', 's11', 's12', 's22')
_R6 = ('r00', 'r01', 'r02', 'r11', 'r12', 'r22')
_V9 = ('v00', 'v01', 'v02', 'v10', 'v11', 'v12', 'v20', 'v21', 'v22')
COLUMNS = ('x', 'y', 'z', 'u', 'v', 'w', 'h', 'm', 'rho', 'p', 'cs') + _S6 + _R6 + ('wdeltap', 'n') + _V9 + (
    'arho', 'au', 'av', 'aw', 'ax', 'ay', 'az')
BASE = ('x', 'y', 'z', 'u', 'v', 'w', 'h', 'm', 'rho')
OUTPUT_ORDER = _V9 + ('arho', 'au', 'av', 'aw', 'ax', 'ay', 'az')
REQUIRED = ('wdeltap_positive', 'wdeltap_negative', 'wdeltap_zero', 'n_1', 'n_2', 'n_4', 'n_3', 'n_2.5', 'wij_zero',
            'approaching', 'receding', 'beta_zero', 'beta_nonzero', 'eps_zero', 'stress_opposed', 'gradient_sum_zero',
            'r_zero', 'r_nonzero', 'rij_below_1e-12', 'rij_above_1e-12', 'coincident_unequal_h', 'lone_particle')
UNOBSERVABLE = ()
_WD = (_ST, 'loop', 'if d_wdeltap[0] > 0.:', 'if d_wdeltap[0] <= 0.:')
_NP = (_ST, 'loop', 'fab = pow(fab, d_n[0])', 'fab = pow(fab, d_n[0] + 1.0)')
_MV = (_MAV, 'loop', 'if vijdotxij < 0:', 'if vijdotxij >= 0:')
MUTANTS = {
    'wdeltap_positive': _WD, 'wdeltap_negative': _WD, 'wdeltap_zero': _WD,
    'n_1': _NP, 'n_2': _NP, 'n_4': _NP, 'n_3': _NP, 'n_2.5': _NP, 'r_nonzero': _NP,
    'wij_zero': (_ST, 'loop', 'fab = pow(fab, d_n[0])', 'fab = pow(fab, d_n[0] - 3.0)'),
    'approaching': _MV, 'receding': _MV,
    'beta_zero': (_MAV, 'loop', 'self.beta*muij*muij', '(self.beta + 1.0)*muij*muij'),
    'beta_nonzero': (_MAV, 'loop', 'self.beta*muij*muij', '0.0*muij*muij'),
    'eps_zero': (_XS, 'loop', 'tmp = -self.eps ', 'tmp = -(self.eps + 1.0) '),
    'stress_opposed': (_ST, 'loop', 'rhob21 = 1. / (rhob * rhob)', 'rhob21 = 1. / (rhoa * rhoa)'),
    'gradient_sum_zero': (_ST, 'loop', 's00b = s00b - pb', 's00b = s00b + pb'),
    'r_zero': (_ST, 'loop', 'art_stress00 = fab * (r00a + r00b)', 'art_stress00 = fab * (r00a + r00b + 1.0)'),
    'rij_below_1e-12': ('kernel',), 'rij_above_1e-12': ('kernel',), 'coincident_unequal_h': ('kernel',),
    'lone_particle': (_XS, 'post_loop', 'd_ax[d_idx] += d_u[d_idx]', 'd_ax[d_idx] += 0.0'),
}
SENSITIVE = {_VG2: ('column', 'u'), _VG3: ('column', 'u'), _CONT: ('column', 'u'), _ST: ('column', 'rho'),
             _MAV: (_MAV, 'alpha'), _XS: (_XS, 'eps'), 'cf0_group': ('column', 'rho')}
ARITH = (
    ('pow(fab, n) with n + 1',) + _NP,
    ('pow(fab, n) with n - 1', _ST, 'loop', 'fab = pow(fab, d_n[0])', 'fab = pow(fab, d_n[0] - 1.0)'),
    ('fab applied to r_a only', _ST, 'loop', 'art_stress01 = fab * (r01a + r01b)', 'art_stress01 = fab * r01a + r01b'),
    ('s11a - pa without the pressure', _ST, 'loop', 's11a = s11a - pa', 's11a = s11a - 0.0*pa'),
    ('rhob21 replaced by rhoa21', _ST, 'loop', 'rhob21 = 1. / (rhob * rhob)', 'rhob21 = 1. / (rhoa * rhoa)'),
    ('s12 where s02 belongs (source side of au)', _ST, 'loop', 's02b * rhob21 + art_stress02', 's12b * rhob21 + art_stress02'),
    ('s12 where s02 belongs (destination side of aw)', _ST, 'loop', 'mb * (s20a * rhoa21', 'mb * (s21a * rhoa21'),
    ('wdeltap > 0 changed to >= 0', _ST, 'loop', 'if d_wdeltap[0] > 0.:', 'if d_wdeltap[0] >= 0.:'),
    ('beta dropped', _MAV, 'loop', 'self.beta*muij*muij', '0.0*muij*muij'),
    ('cij without the 0.5', _MAV, 'loop', 'cij = 0.5 * (', 'cij = ('),
    ('rhoij without the 0.5, so RHOIJ1 halved (artificial viscosity)', _MAV, 'loop', 'piij = piij*RHOIJ1', 'piij = piij*RHOIJ1*0.5'),
    ('rhoij without the 0.5, so RHOIJ1 halved (XSPH)', _XS, 'loop', 'WIJ*RHOIJ1', 'WIJ*RHOIJ1*0.5'),
    ('vijdotxij < 0 changed to <= 0', _MAV, 'loop', 'if vijdotxij < 0:', 'if vijdotxij <= 0:'),
    ('XSPH: u not added behind the loop', _XS, 'post_loop', 'd_ax[d_idx] += d_u[d_idx]', 'd_ax[d_idx] += 0.0'),
    ('continuity: m_j replaced by m_j / rho_j', 'multi', _CONT, 'loop',
     (('s_idx, s_m,', 's_idx, s_m, s_rho,'), ('s_m[s_idx]*vijdotdwij', 's_m[s_idx]/s_rho[s_idx]*vijdotdwij'))),
    ('VelocityGradient2D: -VIJ with the sign dropped', _VG2, 'loop', 'd_v00[d_idx] += tmp * -VIJ[0]', 'd_v00[d_idx] += tmp * VIJ[0]'),
    ('VelocityGradient3D: -VIJ with the sign dropped', _VG3, 'loop', 'd_v00[d_idx] += tmp * -VIJ[0]', 'd_v00[d_idx] += tmp * VIJ[0]'),
    ('VelocityGradient2D: DWIJ[j] and DWIJ[i] swapped', _VG2, 'loop', 'd_v01[d_idx] += tmp * -VIJ[0] * DWIJ[1]', 'd_v01[d_idx] += tmp * -VIJ[1] * DWIJ[0]'),
    ('VelocityGradient3D: DWIJ[j] and DWIJ[i] swapped', _VG3, 'loop', 'd_v12[d_idx] += tmp * -VIJ[1] * DWIJ[2]', 'd_v12[d_idx] += tmp * -VIJ[2] * DWIJ[1]'),
)
EQUIVALENT = ('vijdotxij < 0 changed to <= 0',)
mutant_run = TV.mutant_run


# -- the scale of the stress sum -----------------------------------------------------------------------------------------
_ROWS = {'au': ('s00', 's01', 's02'), 'av': ('s10', 's11', 's12'), 'aw': ('s20', 's21', 's22')}


def scales(table, Sout, recs):
    """au av aw under MomentumEquationWithStress: the sum of |product| over the products of its statement (the docstring),
    from the locals of every call at 50 digits; the artificial viscosity's |increment| on top where it runs"""
    if not any(e['name'] == _ST for e in table['group']):
        return
    A = table['arrays']
    for c, row in _ROWS.items():
        for i, rec in enumerate(recs):
            s = mp.mpf(0)
            for sn, j, name, tr in rec['loop']:
                L = tr.locals
                if name == _ST:
                    for k, comp in enumerate(row):
                        w = abs(L['mb'] * L['DWIJ'][k])
                        s += w * (abs(L[comp + 'a'] * L['rhoa21']) + abs(L[comp + 'b'] * L['rhob21']) + abs(L['art_stress' + comp[1:]]))
                elif name == _MAV:
                    s += abs(mp.mpf(float(A[sn]['m'][j])) * L['piij'] * L['DWIJ']['uvw'.index(c[1])])
            assert s >= Sout[c][i] * (1 - mp.mpf(2) ** -20), (table['key'], c, i, 'the sum of |product| is below the sum of |increment|')
            Sout[c][i] = mp.mpf(float(np.float32(float(s))))


# -- branches and margins ------------------------------------------------------------------------------------------------
def decisions(table, run, i):
    names, margin = E.decisions(table, run, i)           # RIJ against 1e-12
    A = table['arrays']
    D = A[table['dest']]
    group = dict((e['name'], e) for e in table['group'])
    tag = table['tags'][i]
    st = group.get(_ST)
    msum = [0.0, 0.0, 0.0]
    allr0 = all(D[c][i] == 0.0 for c in _R6) if st else False
    approaching = False
    for sn, j, name, tr in run['recs'][i]['loop']:
        L = tr.locals
        if sn == table['dest'] and j == i:
            continue
        if name == _ST:
            for k in range(3):
                msum[k] += float(L['mb']) * float(L['DWIJ'][k])
            allr0 = allr0 and all(A[sn][c][j] == 0.0 for c in _R6)
            if st['params']['wdeltap'] > 0 and float(L['WIJ']) == 0.0:
                names.add('wij_zero')
            if tag == 'stress_opposed':
                for c in ('s00', 's01', 's02', 's11', 's12', 's22'):
                    assert float(L[c + 'a']) * float(L['rhoa21']) == -(float(L[c + 'b']) * float(L['rhob21'])), (table['key'], i, c)
        if name == _MAV:
            dot = float(L['vijdotxij'])
            if dot != 0.0:
                margin = min(margin, abs(dot) / (P._norm(L['VIJ']) * P._norm(L['XIJ'])))
                names.add('approaching' if dot < 0 else 'receding')
                approaching = approaching or dot < 0
    if st:
        wd, n = st['params']['wdeltap'], st['params']['n']
        names.add('wdeltap_positive' if wd > 0 else 'wdeltap_zero' if wd == 0 else 'wdeltap_negative')
        if wd > 0:
            names.add('n_%g' % n)
            names.add('r_zero' if allr0 else 'r_nonzero')
        if tag == 'stress_opposed':
            names.add(tag)
        if tag == 'lone':
            assert len(run['recs'][i]['loop']) == len(table['group']), (table['key'], i)
        if tag == 'gradient_sum_zero':
            assert msum == [0.0, 0.0, 0.0] and len(run['recs'][i]['loop']) >= 3, (table['key'], i, msum)
            names.add(tag)
    if _MAV in group and approaching:
        names.add('beta_zero' if group[_MAV]['params']['beta'] == 0.0 else 'beta_nonzero')
    if tag == 'lone':
        names.add('lone_particle')
    if _XS in group and group[_XS]['params']['eps'] == 0.0:
        names.add('eps_zero')
    return names, margin


# -- tables --------------------------------------------------------------------------------------------------------------
def particle(rng, dim, uh, off, h, **kw):
    q = dict(arr='fluid', off=off, h=h, rho=float(rng.uniform(0.75, 1.5)), m=M0 if uh else float(rng.uniform(0.75, 1.5)) * 2.0 ** -6,
             p=float(rng.uniform(0.5, 2.0)), cs=float(rng.uniform(0.8, 1.5)))
    vel = rng.uniform(-1, 1, 3)
    for k, c in enumerate('uvw'):
        q[c] = float(vel[k]) if k < dim else 0.0
    for c, x in zip(_S6, rng.uniform(-1, 1, 6)):
        q[c] = float(x)
    for c, x in zip(_R6, rng.uniform(-0.5, 0.5, 6)):
        q[c] = float(x)
    q.update(kw)
    return q


def _off(dim, r):
    return tuple(r * c for c in DIRS[dim])


def clusters(rng, dim, kname, uh, kind):
    """``stress``: the clusters built for the regrouped stress sum; ``r0``: two pairs without artificial stress;
    ``small``: stresses, pressures and r_ij of 2^-8 (the artificial viscosity next to the stress equation)"""
    cl = []

    def hh():
        return H0 if uh else P._h(rng)

    def pair(off, hi=None, hj=None, kwa=None, kwb=None):
        cl.append([particle(rng, dim, uh, _off(dim, 0.0), hi or hh(), **(kwa or {})), particle(rng, dim, uh, off, hj or hh(), **(kwb or {}))])

    d = DIRS[dim]
    cl.append([particle(rng, dim, uh, _off(dim, 0.0), hh(), tag='lone')])      # the self pair only: every term 0, ax = u
    for k in range(5):
        hi, hj = hh(), hh()
        pair(_off(dim, min(float(rng.uniform(0.3, 1.5)) * min(hi, hj), 0.23)), hi, hj)
    for k in range(2):                  # strongly approaching and strongly receding along the line of centres
        s = 2.0 if k == 0 else -2.0
        pair(_off(dim, 0.09375), kwa=dict(zip('uvw', [-s * c for c in d])), kwb=dict(zip('uvw', [s * c for c in d])))
    for k in range(2):                  # one destination between two partners, one approaching, one receding
        cl.append([particle(rng, dim, uh, _off(dim, 0.0), hh(), u=0.0, v=0.0, w=0.0),
                   particle(rng, dim, uh, _off(dim, 0.0625), hh(), **dict(zip('uvw', [0.5 * c for c in d]))),
                   particle(rng, dim, uh, _off(dim, -0.046875), hh(), **dict(zip('uvw', [0.25 * c for c in d])))])
    for r in (2.0 ** -40, 2.0 ** -40, 2.0 ** -39, 2.0 ** -39):
        pair(_off(dim, r))
    if uh:
        pair(_off(dim, 0.0))
    else:
        pair(_off(dim, 0.0), hi=2.0 ** -4 * 1.5, hj=2.0 ** -4 * 2.5)
        pair(_off(dim, 0.0), hi=2.0 ** -4 * 3.5, hj=2.0 ** -4 * 2.0)
        pair(_off(dim, 0.1875), hi=2.0 ** -4, hj=2.0 ** -2)           # h ratio 4
    if 'stress' in kind:
        for k in range(2):              # sigma_a / rho_a^2 = -sigma_b / rho_b^2 to the last bit: rho 1 and 2, dyadic stresses
            sa = dict(zip(_S6, (0.375, -0.25, 0.625, -0.75, 0.125, 0.5 + 0.25 * k)))
            pa, pb = 0.5, 0.25
            sb = dict((c, (pb - 4.0 * (sa[c] - pa)) if c in ('s00', 's11', 's22') else -4.0 * sa[c]) for c in _S6)
            pair(_off(dim, 0.0625 + 0.03125 * k), kwa=dict(sa, rho=1.0, p=pa, tag='stress_opposed'), kwb=dict(sb, rho=2.0, p=pb, tag='stress_opposed'))
        for k in range(2):              # a symmetric triple with equal masses and equal h of the partners: sum m_j DWIJ = 0
            hp = H0 if uh else 2.0 ** -4 * float(rng.uniform(1.5, 4.0))      # (the partners are 2 r apart: neighbours of each other)
            r = 0.0625 + 0.015625 * k
            cl.append([particle(rng, dim, uh, _off(dim, 0.0), hh(), tag='gradient_sum_zero'),
                       particle(rng, dim, uh, _off(dim, r), hp, m=M0), particle(rng, dim, uh, _off(dim, -r), hp, m=M0)])
        if not uh:                      # a neighbour by the larger h outside the support under HIJ: W = 0, DWIJ = 0
            far = (0.21875, 2.0 ** -3) if E.RADIUS[kname] == 2.0 else (0.25, 2.0 ** -4 * 1.5)
            for k in range(2):
                pair((far[0], 0.0, 0.0), hi=2.0 ** -4, hj=far[1])
    if 'r0' in kind:
        z = dict((c, 0.0) for c in _R6)
        for k in range(2):
            pair(_off(dim, 0.0625 + 0.015625 * k), kwa=dict(z), kwb=dict(z))
    if 'small' in kind:
        for c in cl:
            for q in c:
                for k in _S6 + _R6 + ('p',):
                    q[k] *= 2.0 ** -8
    if 'z' in kind:                     # 2-D: a z that is not 0 (the same everywhere) and a w that no 2-D term may read
        for c in cl:
            for q in c:
                q['off'] = (q['off'][0], q['off'][1], 0.375)
                q['w'] = float(rng.uniform(-1, 1))
    return cl


def wdeltap_of(kname, dim):
    return float(np.float32(getattr(RK, kname)(dim=dim).kernel([H0, 0.0, 0.0], H0, H0)))


def _eq(name, sources, **params):
    return dict(name=name, sources=list(sources), params=params)


def all_tables():
    mod = sys.modules[__name__]
    tables = []
    f = ['fluid']
    for ci, cfg in enumerate(CONFIGS):
        cname, dim, kname = cfg
        wd = wdeltap_of(kname, dim)
        for fi, form in enumerate(('uh', 'vh')):
            uh = form == 'uh'
            rng = np.random.default_rng(8500 + 10 * ci + fi)
            seed = [100 * ci + 50 * fi]

            def add(label, kind, what, group):
                seed[0] += 1
                st = [e for e in group if e['name'] == _ST]
                tables.append(TV.build_table(mod, '%s/%s/%s/%s' % (label, kind, cname, form), label, cfg, form,
                                             clusters(rng, dim, kname, uh, what), group, T, seed[0],
                                             constants=dict(st[0]['params']) if st else None, scales=scales))

            def stress(wdeltap=-1.0, n=4.0):
                return _eq(_ST, f, wdeltap=wdeltap, n=n)

            if dim == 2:
                add(_VG2, 'alone', 'z', [_eq(_VG2, f)])
            if dim == 3:
                add(_VG3, 'alone', '', [_eq(_VG3, f)])
            add(_CONT, 'stress', 'stress', [_eq(_CONT, f), stress()])
            for n in (4.0,) + ((2.0, 3.0) if ci % 2 == 0 else (1.0, 2.5)):
                add(_ST, 'n%g' % n, 'stress r0', [stress(wd, n)])
            add(_ST, 'wzero', 'stress', [stress(0.0, 4.0)])
            add(_MAV, 'beta', 'small', [stress(), _eq(_MAV, f, alpha=0.75, beta=1.5)])
            add(_MAV, 'beta0', 'small', [stress(), _eq(_MAV, f, alpha=0.75, beta=0.0)])
            add(_XS, 'stress', '', [stress(), _eq(_XS, f, eps=0.5)])
            add(_XS, 'eps0', '', [stress(), _eq(_XS, f, eps=0.0)])
            # the rates of ElasticSolidsScheme (solid_mech/basic.py:604-651) on one array, without the no-source equation
            add('cf0_group', 'rates', 'stress r0', [_eq(_CONT, f), stress(wd, 4.0), _eq(_MAV, f, alpha=1.0, beta=1.0), _eq(_XS, f, eps=0.5)])
    return tables


# -- the tension token: a second file --------------------------------------------------------------------------------------
# MonaghanArtificialStress (a no-source equation, judged in tests/test_nosrc_edges.py) runs ahead of the rates on the
# device and tells the records without h and m whether any r_ij is not 0.  These tables hold states on which its result
# is exact on both sides: DIAGONAL stresses, dyadic like p and eps, rho 1 or 2, and sum_k |s_kk - p| a power of two
# (the device scales the tensor by that sum before its Jacobi sweep).  The principal stresses of a diagonal tensor are
# its diagonal and its axes the coordinate axes, so solid_mech/basic.py:218-231 gives r_kk = -eps (s_kk - p) rhoi21
# where s_kk - p > 0 and 0 elsewhere, the off-diagonal r_ij 0: evaluated here as the reference writes it and stored as the
# INPUT r of the rates group, which is the CF0 group of the main file.
OUT_TENSION = os.path.join(HERE, 'elastic_tension_pair_edges.npz')
EPS_STRESS = 0.25
REQUIRED_TENSION = ('wdeltap_positive', 'n_4', 'approaching', 'receding', 'beta_nonzero', 'r_zero', 'r_nonzero', 'lone_particle')
# (s00, s11, s22, p, rho): all three s_kk - p negative / one of them positive; sum |s_kk - p| = 1, 2, 4, 2 and 1, 2
COMPRESSIVE = ((0.25, 0.0, 0.25, 0.5, 1.0), (-0.25, 0.25, 0.25, 0.75, 2.0), (-1.0, 0.5, -0.5, 1.0, 1.0), (0.0, -0.5, 0.0, 0.5, 2.0))
TENSILE = ((0.75, 0.0, 0.0, 0.25, 1.0), (0.0, 1.5, 0.0, 0.5, 2.0))


def artificial_stress(q, eps):
    """solid_mech/basic.py:183-184 and :218-242 for a diagonal tensor (V = its diagonal, R = the identity)"""
    rhoi = q['rho']
    rhoi21 = 1. / (rhoi * rhoi)
    out = dict((c, 0.0) for c in _R6)
    for c, s in (('r00', 's00'), ('r11', 's11'), ('r22', 's22')):
        V = q[s] - q['p']
        out[c] = -eps * V * rhoi21 if V > 0 else 0.0
    return out


def tension_clusters(rng, dim, tensile):
    def state(k, rows=COMPRESSIVE):
        s00, s11, s22, p, rho = rows[k % len(rows)]
        q = dict(s00=s00, s11=s11, s22=s22, s01=0.0, s02=0.0, s12=0.0, p=p, rho=rho)
        assert all((q[c] - p > 0) == (rows is TENSILE and c == ('s00', 's11')[k % 2]) for c in ('s00', 's11', 's22'))
        q.update(artificial_stress(q, EPS_STRESS))
        return q

    d = DIRS[dim]
    cl = [[particle(rng, dim, True, _off(dim, 0.0), H0, tag='lone', **state(0))]]
    for k in range(4):
        cl.append([particle(rng, dim, True, _off(dim, 0.0), H0, **state(k)),
                   particle(rng, dim, True, _off(dim, float(rng.uniform(0.3, 1.5)) * H0), H0, **state(k + 1))])
    for k in range(2):
        s = 2.0 if k == 0 else -2.0
        cl.append([particle(rng, dim, True, _off(dim, 0.0), H0, **dict(state(k + 2), **dict(zip('uvw', [-s * c for c in d])))),
                   particle(rng, dim, True, _off(dim, 0.09375), H0, **dict(state(k + 3), **dict(zip('uvw', [s * c for c in d]))))])
    cl.append([particle(rng, dim, True, _off(dim, 0.0), H0, **state(1)), particle(rng, dim, True, _off(dim, 0.0625), H0, **state(2)),
               particle(rng, dim, True, _off(dim, -0.046875), H0, **state(3))])
    if tensile:                         # ONE cluster in tension
        cl.append([particle(rng, dim, True, _off(dim, 0.0), H0, **state(0, TENSILE)), particle(rng, dim, True, _off(dim, 0.078125), H0, **state(1, TENSILE))])
    return cl


def tension_tables():
    mod = sys.modules[__name__]
    tables = []
    f = ['fluid']
    for ci, cfg in enumerate(CONFIGS):
        cname, dim, kname = cfg
        rng = np.random.default_rng(8700 + ci)
        group = [_eq(_CONT, f), _eq(_ST, f, wdeltap=wdeltap_of(kname, dim), n=4.0), _eq(_MAV, f, alpha=1.0, beta=1.0), _eq(_XS, f, eps=0.5)]
        for k, kind in enumerate(('compressive', 'tensile')):
            tables.append(TV.build_table(mod, 'tension/%s/%s/uh' % (kind, cname), 'tension', cfg, 'uh', tension_clusters(rng, dim, k == 1),
                                         group, T, 900 + 10 * ci + k, constants=dict(group[1]['params']), scales=scales))
    return tables


class Tension(object):
    """the second file through make_edac_pair_golden.build: the tables above, the branches they take"""
    all_tables = staticmethod(tension_tables)
    REQUIRED, UNOBSERVABLE, LABELS = REQUIRED_TENSION, (), ('tension',)
    MUTANTS = dict((b, MUTANTS[b]) for b in REQUIRED_TENSION)
    SENSITIVE = {'tension': ('column', 'rho')}
    mutant_run = staticmethod(TV.mutant_run)


def main():
    E.write(sys.modules[__name__], OUT)
    if '--mutants' not in sys.argv[1:]:
        E.write(Tension, OUT_TENSION)


if __name__ == '__main__':
    main()
