#!/usr/bin/env python
"""Golden vectors for Godunov SPH, from the REFERENCE's own ``GSPHScheme`` (pysph/sph/scheme.py:1144-1458), its equation
classes and Riemann solvers (pysph/sph/gas_dynamics/gsph.py, riemann_solver.py) and ``GSPHStep``
(pysph/sph/integrator_step.py:431-449), executed as plain Python in the manner of make_gasd_golden.py (same driver, same
stored layout):

    python tests/golden/make_gsph_golden.py

    gsph_1d.npz          120 particles of equal mass with an 8:1 spacing jump and a pressure jump (a Sod state); the whole
                         group list with the scheme's defaults (exact, linear, I02)
    gsph_2d.npz          jittered 18 x 14 lattice, masses +-20 %, random u v e, CubicSpline, g1 = 0.3, g2 = 0.5
    gsph_3d.npz          6^3 jittered, QuinticSpline, hllc, IwIn, cubic, interface position; out/ after one evaluation,
                         out2/ + nnps2/ after one GSPHStep and a second evaluation (dt > 0 in both, so the cs dt sij
                         terms act)
    gsph_solvers.npz     the force group alone on the converged 2-D state, once per rsolver 0..10
    gsph_options.npz     on exact and hllc every combination of monotonicity, interpolation and interface_zero, hybrid at
                         t = 0.3 tf, and (prefix coincident/) two fluids with one pair of coincident particles
    gsph_kernels.npz     per smoothing kernel class one tiny case, stored under the class name as prefix
    gsph_steppers.npz    GSPHStep.stage1 on random columns
    gsph_steps.npz       the 3-D case through three Euler steps
    gsph_structures.npz  group lists only, for option combinations (has_ghosts and two fluids included), the choices
                         dictionaries and the constructor defaults of the scheme and of GSPHAcceleration

``declare`` of the two modules is oracle.py_eval.declare; ``declare('matrix(2)', 2)`` (riemann_solver.py:230), for which
that stand-in returns two floats, gives two lists here.  Every output column starts as random garbage.

What the reference did is read off a line tracer (sys.settrace) over the two modules: which lines ran and how often, the
solvers' return values, the loop index and every ``change`` of ``exact``, the relative pressure change of ``van_leer``.
Conditions asserted on the reference alone (re-seeded until met, results under meta/):
  * no solver call returns 1; every iterative solve stops with its loop index below niter - 1;
  * in no iteration is ``change`` (van_leer: the relative pressure change) within a relative 1e-3 of tol.  One solve in
    about ten thousand has such an iteration, so the force-only cases, which share one state, are not re-seeded: a
    case that trips is run again with the next ``tol`` of TOLS, and the ``tol`` it passed with is among its parameters;
  * the same case with every input column perturbed by a relative 1e-13 agrees to 1e-9 of the field maximum: a case in
    which a comparison flips under rounding is re-seeded;
  * rho, p, e > 0; no pair other than the deliberate coincident one closer than 1e-6 h;
  * over all files every branch named in BRANCHES is taken (the count per branch and file is stored).
"""
import json
import os
import sys
from collections import Counter

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_gasd_golden as GG  # noqa: E402  (sets up the reference imports and the stubs gas dynamics needs)
import make_golden as MG  # noqa: E402

from oracle.py_eval import declare as _py_declare  # noqa: E402
from oracle.ref_driver import ListPA, PyLinkedListNNPS, RefEval  # noqa: E402

import pysph.sph.gas_dynamics.gsph as GS  # noqa: E402
import pysph.sph.gas_dynamics.riemann_solver as RS  # noqa: E402


def _declare(spec, *a):
    if spec.replace(' ', '').startswith('matrix(') and a and isinstance(a[0], int):
        return tuple(_py_declare(spec) for _ in range(a[0]))
    return _py_declare(spec, *a)


GS.declare = _declare
RS.declare = _declare

from pysph.sph.acceleration_eval import AccelerationEval  # noqa: E402
from pysph.sph.equation import Group  # noqa: E402
from pysph.sph.scheme import GSPHScheme  # noqa: E402
from pysph.sph.integrator_step import GSPHStep  # noqa: E402
from pysph.base import kernels as RK  # noqa: E402
import inspect  # noqa: E402

GRADS = ('px', 'py', 'pz', 'ux', 'uy', 'uz', 'vx', 'vy', 'vz', 'wx', 'wy', 'wz')
OUTPUTS = ('rho', 'arho', 'grhox', 'grhoy', 'grhoz', 'dwdh', 'div', 'p', 'cs', 'au', 'av', 'aw', 'ae') + GRADS
FORCE_OUT = ('au', 'av', 'aw', 'ae')
TOLS = (1e-6, 1.5e-6, 7e-7, 2e-6, 5e-7, 3e-6, 4e-7, 1.2e-6, 8e-7, 2.5e-6)
SOLVERS = ('non_diffusive', 'van_leer', 'exact', 'hllc', 'ducowicz', 'hlle', 'roe', 'llxf', 'hllc_ball', 'hll_ball', 'hllsy')


def _line(fn, text, nth=0):
    """the line of ``fn``'s source that holds ``text`` (the nth such line)"""
    src, first = inspect.getsourcelines(fn)
    hits = [first + k for k, ln in enumerate(src) if text in ln]
    assert len(hits) > nth, (fn.__name__, text)
    return (fn.__name__, hits[nth])


_LOOP = GS.GSPHAcceleration.loop
_INTERP = GS.GSPHAcceleration.interpolate
# name -> (function, line): a line that runs only when the branch is taken
BRANCHES = {
    'mono0': _line(_LOOP, 'rsi = 0.0', 0),
    'mono1_sign': _line(_LOOP, 'vsi = 0.', 1),               # (vsi * vsj) < 0
    'mono1_shock': _line(_LOOP, 'rsi = 0.', 1),              # min(csi, csj) < 3 (vl - vr)
    'mono2': _line(_LOOP, 'qijr = rhoi - rhoj'),
    'mono2_coincident': _line(_LOOP, 'rsi = 0.0', 1),
    'coincident_eij': _line(_LOOP, 'sij = 1.0/(RIJ + EPS)'),
    'hybrid': _line(_LOOP, 'pstar2 = result[0]'),
    'conduction': _line(_LOOP, 'divj = s_div[s_idx]'),
    'min_zero': _line(GS.monotonicity_min, 'return 0.0'),
    'min_x3_a': _line(GS.monotonicity_min, '_min = x3', 0),
    'min_x2': _line(GS.monotonicity_min, '_min = x2'),
    'min_x3_b': _line(GS.monotonicity_min, '_min = x3', 1),
    'min_x1': _line(GS.monotonicity_min, '_min = x1'),
    'interp_delta': _line(_INTERP, 'vij_i2 = 1./(rhoi * rhoi)'),
    'interp_linear': _line(_INTERP, 'dij = 0.5 * (Vi + Vj)', 0),
    'interp_linear_sstar': _line(_INTERP, 'sstar = 0.5 * hij*hij * cij*dij/vij'),
    'interp_cubic': _line(_INTERP, 'hi2 = hi*hi'),
    'interp_cubic_sstar': _line(_INTERP, 'sstar = ((15.0/32.0)'),
    'prefun_rarefaction': _line(RS.prefun_exact, 'pratio = p/pk'),
    'prefun_shock': _line(RS.prefun_exact, 'ak = g5/dk'),
    'exact_guess_pvrs': _line(RS.exact, 'pm = ppv'),
    'hllc_left_star': _line(RS.hllc, 'mstar = 1./(sl - sm)'),
    'hllc_right_star': _line(RS.hllc, 'mstar = 1./(sr - sm)'),
    'ducowicz_a': _line(RS.ducowicz, 'return 0', 0),
    'ducowicz_b': _line(RS.ducowicz, 'return 0', 1),
    'ducowicz_c': _line(RS.ducowicz, 'return 0', 2),
    'ducowicz_d': _line(RS.ducowicz, 'return 0', 3),
}
# every one of these somewhere in the files; of hllc's and ducowicz's cases at least two each
REQUIRED = ('mono0', 'mono1_sign', 'mono1_shock', 'mono2', 'mono2_coincident', 'coincident_eij', 'hybrid', 'conduction',
            'min_zero', 'min_x2', 'min_x1', 'interp_delta', 'interp_linear', 'interp_linear_sstar', 'interp_cubic',
            'interp_cubic_sstar', 'prefun_rarefaction', 'prefun_shock')
_EXACT_IF = _line(RS.exact, 'if change <= tol')[1]
_VL_IF = _line(RS.van_leer, 'if converged:', 0)[1]
_FILES = (GS.__file__, RS.__file__)


class Tracer(object):
    """lines run in gsph.py / riemann_solver.py, return values of the solvers, margins of the iterative ones"""

    def __init__(self):
        self.lines = Counter()
        self.returns = Counter()
        self.margin = float('inf')     # min over iterations of |change - tol| / tol
        self.max_index = -1            # the largest loop index an iterative solve ended with
        self.max_iter = 0
        self.n_exact = 0

    def __call__(self, frame, event, arg):
        if frame.f_code.co_filename in _FILES:
            return self.local
        return None

    def local(self, frame, event, arg):
        name = frame.f_code.co_name
        if event == 'line':
            no = frame.f_lineno
            self.lines[(name, no)] += 1
            if name == 'exact' and no == _EXACT_IF:
                L = frame.f_locals
                self.margin = min(self.margin, abs(L['change'] - L['tol']) / L['tol'])
            elif name == 'van_leer' and no == _VL_IF:
                L = frame.f_locals
                rel = abs(L['pstar'] - L['pstar_old']) / L['pstar']
                self.margin = min(self.margin, abs(rel - L['tol']) / L['tol'])
                self.max_index = max(self.max_index, L['iteration'])
                assert L['iteration'] < L['niter'] - 1, 'van_leer: loop index at niter - 1'
        elif event == 'return' and name in SOLVERS:
            self.returns[(name, arg)] += 1
            assert arg == 0, 'solver %s returned %r' % (name, arg)
            if name == 'exact':
                L = frame.f_locals
                self.n_exact += 1
                self.max_index = max(self.max_index, L['i'])
                assert L['i'] < L['niter'] - 1, 'exact: loop index at niter - 1'
        return self.local

    def branch_counts(self):
        return dict((k, int(self.lines.get(v, 0))) for k, v in BRANCHES.items())

    def meta(self):
        assert self.margin > 1e-3, ('an iteration within 1e-3 of tol', self.margin)
        return dict(branches=json.dumps(self.branch_counts()), min_tol_margin=min(self.margin, 1e300),
                    max_loop_index=self.max_index, solver_returns=json.dumps(
                        dict(('%s:%d' % k, v) for k, v in self.returns.items())))


TOTAL = Counter()          # branch counts over all files


def traced(fn, tracer):
    sys.settrace(tracer)
    try:
        return fn()
    finally:
        sys.settrace(None)


def needed_props(groups):
    """every d_* / s_* name a method of the equations takes"""
    names = set()
    for g in groups:
        for eq in g.equations:
            for meth in ('initialize', 'loop', 'post_loop'):
                f = getattr(eq, meth, None)
                if f is not None:
                    names.update(a[2:] for a in inspect.getfullargspec(f).args if a[:2] in ('d_', 's_') and a[2:] != 'idx')
    return names


def run_groups(pas, groups, kernel, dim, t, dt, check_nnps=True):
    """the group list over the arrays as AccelerationEval.compute runs it; returns the neighbour search"""
    a_eval = AccelerationEval(pas, groups, kernel)
    nnps = PyLinkedListNNPS(dim, pas, radius_scale=kernel.radius_scale)
    ev = RefEval(a_eval, nnps)
    nnps.update()
    if check_nnps:
        MG.check_nnps(nnps)
    for mg in a_eval.mega_groups:
        assert not mg.iterate and not mg.has_subgroups
        ev._do_group(mg, t, dt)
        if mg.update_nnps:
            nnps.update()
    return nnps


def state_conditions(pas, nnps, allow_coincident=0):
    """rho, p, e > 0 after the evaluation; no pair closer than 1e-6 h except the deliberate ones"""
    close = 0
    for di, pa in enumerate(pas):
        P = dict((k, np.array(pa.properties[k])) for k in ('x', 'y', 'z', 'h', 'rho', 'p', 'e'))
        assert np.all(P['rho'] > 0) and np.all(P['p'] > 0) and np.all(P['e'] > 0), 'rho, p or e <= 0'
        for si, sa in enumerate(pas):
            S = dict((k, np.array(sa.properties[k])) for k in 'xyz')
            for i in range(pa.n_real):
                nb = np.array(nnps.neighbors(si, di, i), dtype=int)
                if si == di:
                    nb = nb[nb != i]
                if nb.size == 0:
                    continue
                r = np.sqrt(sum((P[a][i] - S[a][nb]) ** 2 for a in 'xyz'))
                close += int(np.sum(r < 1e-6 * P['h'][i]))
    assert close == allow_coincident, ('pairs closer than 1e-6 h', close)


def fill(props, rng, n, outputs=OUTPUTS, extra=()):
    props['h0'] = props['h'].copy()
    props['converged'] = np.zeros(n)
    props['omega'] = np.ones(n)
    for k in ('ah',) + tuple(outputs) + tuple(extra):
        props[k] = rng.uniform(-1, 1, n)          # garbage: must be overwritten


def perturbed(props, rng, skip):
    return dict((k, (v if k in skip else v * (1.0 + 1e-13 * rng.uniform(-1, 1, v.size)))) for k, v in props.items())


def compare(a, b, cols, what):
    worst = 0.0
    for k in cols:
        x, y = np.array(a[k]), np.array(b[k])
        scale = max(np.abs(x).max(), 1e-300)
        worst = max(worst, float(np.abs(x - y).max() / scale))
    assert worst < 1e-9, ('%s: a relative 1e-13 of the inputs moves the result by %.3e' % (what, worst))
    return worst


def whole_list(arrays_props, n_reals, kw, kernel, t, dt, tracer, second=False, steps=0, allow_coincident=0):
    """arrays_props: name -> props.  The whole list (and what follows) on ListPAs; returns (out dict, pas)"""
    dim = kw['dim']
    groups = GSPHScheme(**kw).get_equations()
    pas = [ListPA(name, arrays_props[name], n_reals[name]) for name in kw['fluids']]
    for pa in pas:
        assert needed_props(groups) <= set(pa.properties), sorted(needed_props(groups) - set(pa.properties))
    out = {}
    if tracer is not None:
        GG._store(out, pas, 'in')
        for pa in pas:
            out['nreal/' + pa.name] = np.array(pa.n_real)

    def body():
        if steps:
            # pysph/sph/integrator.py:426-437 (EulerIntegrator.one_timestep): compute_accelerations (neighbours rebuilt);
            # stage1; update_domain
            tt = t
            for _ in range(steps):
                nn = run_groups(pas, groups, kernel, dim, tt, dt, check_nnps=False)
                state_conditions(pas, nn)
                for pa in pas:
                    GG.sweep(GSPHStep(), 'stage1', pa, tt, dt)
                tt += dt
            GG._store(out, pas, 'out')
            return
        nn = run_groups(pas, groups, kernel, dim, t, dt)
        state_conditions(pas, nn, allow_coincident)
        GG._store(out, pas, 'out')
        GG._nnps_out(out, nn, 'nnps')
        if second:
            for pa in pas:
                GG.sweep(GSPHStep(), 'stage1', pa, t, dt)
            nn = run_groups(pas, groups, kernel, dim, t + dt, dt)
            state_conditions(pas, nn)
            GG._store(out, pas, 'out2')
            GG._nnps_out(out, nn, 'nnps2')

    if tracer is not None:
        traced(body, tracer)
    else:
        body()
    out['t'] = np.array(t)
    out['dt'] = np.array(dt)
    out['structure'] = np.array(json.dumps(GG.structure(groups)))
    out['scheme'] = np.array(json.dumps(kw))
    out['kernel'] = np.array(type(kernel).__name__)
    return out, pas


def evaluate(make, seeds, what, prefix='', **ev_kw):
    """re-seed until the conditions hold; the run with perturbed inputs has no tracer"""
    for seed in seeds:
        arrays_props, n_reals, kw, kernel = make(seed)
        tr = Tracer()
        try:
            out, pas = whole_list(arrays_props, n_reals, kw, kernel, tracer=tr, **ev_kw)
            meta = tr.meta()
            rng = np.random.default_rng(seed + 7919)
            pert = dict((name, perturbed(p, rng, ('converged', 'omega'))) for name, p in arrays_props.items())
            out_p, pas_p = whole_list(pert, n_reals, kw, kernel, tracer=None, **ev_kw)
            last = 'out2' if ev_kw.get('second') else 'out'
            worst = 0.0
            for pa in pas:
                cols = [k.split('/')[2] for k in out if k.startswith('%s/%s/' % (last, pa.name))]
                worst = max(worst, compare(dict((c, out['%s/%s/%s' % (last, pa.name, c)]) for c in cols),
                                           dict((c, out_p['%s/%s/%s' % (last, pa.name, c)]) for c in cols), cols, what))
            meta['perturbation_1e-13_moves'] = worst
        except AssertionError as e:
            print(what, 'seed', seed, 'rejected:', e, flush=True)
            continue
        for k, v in meta.items():
            out['meta/' + k] = np.array(v)
        out['meta/seed'] = np.array(seed)
        TOTAL.update(tr.branch_counts())
        print(what, 'seed', seed, dict((k, v) for k, v in meta.items() if k != 'branches'), flush=True)
        return dict((prefix + k, v) for k, v in out.items()), seed
    raise RuntimeError('%s: no seed met the conditions' % what)


def _base_props(x, y, z, u, v, w, m, h, e, rng):
    n = x.size
    props = dict(x=x, y=y, z=z, u=u, v=v, w=w, m=m, h=h, e=e)
    fill(props, rng, n)
    return props


def _make_1d(seed):
    rng = np.random.default_rng(seed)
    nl, nr = 96, 24                       # equal masses: spacing ratio 8 <-> density ratio 8
    dxl = 0.5 / nl
    dxr = 8 * dxl
    x = np.concatenate([-0.5 + (np.arange(nl) + 0.5) * dxl, (np.arange(nr) + 0.5) * dxr])
    n = x.size
    spacing = np.concatenate([dxl * np.ones(nl), dxr * np.ones(nr)])
    e = np.concatenate([2.5 * np.ones(nl), 2.0 * np.ones(nr)]) * (1 + 0.02 * rng.uniform(-1, 1, n))   # p = 1 | 0.1
    props = _base_props(x + 0.1 * spacing * rng.uniform(-1, 1, n), np.zeros(n), np.zeros(n), 0.3 * rng.uniform(-1, 1, n),
                        np.zeros(n), np.zeros(n), dxl * np.ones(n), 1.5 * spacing, e, rng)
    kw = dict(fluids=['fluid'], solids=[], dim=1, gamma=1.4, kernel_factor=1.5)
    return dict(fluid=props), dict(fluid=n), kw, RK.Gaussian(dim=1)


def _make_2d(seed, **extra):
    rng = np.random.default_rng(seed)
    lp, n, dx = GG._lattice(2, (18, 14), rng, mvar=0.2, hfac=1.2, hvar=0.1)
    props = _base_props(lp['x'], lp['y'], lp['z'], lp['u'], lp['v'], lp['w'], lp['m'], lp['h'], lp['e'], rng)
    kw = dict(fluids=['fluid'], solids=[], dim=2, gamma=1.4, kernel_factor=1.2, g1=0.3, g2=0.5)
    kw.update(extra)
    return dict(fluid=props), dict(fluid=n), kw, RK.CubicSpline(dim=2)


def _make_3d(seed):
    rng = np.random.default_rng(seed)
    lp, n, dx = GG._lattice(3, (6, 6, 6), rng, hfac=1.2, hvar=0.1)
    props = _base_props(lp['x'], lp['y'], lp['z'], lp['u'], lp['v'], lp['w'], lp['m'], lp['h'], lp['e'], rng)
    # hllc: each evaluation of this case solves 26 000 Riemann problems, and of that many `exact` solves one or two have an
    # iteration within 1e-3 of tol whatever the seed; the iterative solvers are in the smaller cases
    kw = dict(fluids=['fluid'], solids=[], dim=3, gamma=5.0 / 3.0, kernel_factor=1.2, monotonicity=2, interpolation=2,
              interface_zero=False, rsolver=3)
    return dict(fluid=props), dict(fluid=n), kw, RK.QuinticSpline(dim=3)


def save(fname, out):
    GG.save(fname, out)
    assert os.path.getsize(os.path.join(HERE, fname)) < 1024 * 1024, fname


def case_1d():
    out, seed = evaluate(_make_1d, range(100, 140), 'gsph_1d', t=0.0, dt=1e-4)
    save('gsph_1d.npz', out)


def case_2d():
    out, seed = evaluate(_make_2d, range(200, 240), 'gsph_2d', t=0.0, dt=1e-4)
    save('gsph_2d.npz', out)


def case_3d():
    out, seed = evaluate(_make_3d, range(300, 340), 'gsph_3d', t=0.0, dt=2e-3, second=True)
    save('gsph_3d.npz', out)
    for s in range(seed, seed + 40):          # three Euler steps, re-seeded on their own should a later step trip
        try:
            outs, _ = evaluate(_make_3d, [s], 'gsph_steps', t=0.0, dt=2e-3, steps=3)
        except RuntimeError:
            continue
        outs['meta/steps'] = np.array(3)
        save('gsph_steps.npz', outs)
        return
    raise RuntimeError('gsph_steps: no seed met the conditions')


def force_only(props, n, kernel, dim, params, t, dt, tracer):
    """GSPHAcceleration alone over one array; returns the four columns it writes (and checks nothing else moved)"""
    pa = ListPA('fluid', props, n)
    before = dict((k, list(v)) for k, v in pa.properties.items())
    groups = [Group(equations=[GS.GSPHAcceleration(dest='fluid', sources=['fluid'], **params)])]

    def body():
        run_groups([pa], groups, kernel, dim, t, dt, check_nnps=False)
    if tracer is not None:
        traced(body, tracer)
    else:
        body()
    for k, v in pa.properties.items():
        assert k in FORCE_OUT or v == before[k], k
    return dict((k, np.array(pa.properties[k])) for k in FORCE_OUT)


def _converged_2d():
    g = np.load(os.path.join(HERE, 'gsph_2d.npz'))
    props = dict((k.split('/')[2], g[k].copy()) for k in g.files if k.startswith('out/fluid/'))
    rng = np.random.default_rng(4242)
    n = int(g['nreal/fluid'])
    for k in FORCE_OUT:
        props[k] = rng.uniform(-1, 1, n)
    return props, n, json.loads(str(g['scheme'])), RK.CubicSpline(dim=2)


def _force_cases(fname, cases, key):
    """cases: name -> (params of GSPHAcceleration, t).  On the converged 2-D state; a case that trips a condition fails
    the whole file (the state is the 2-D case's: re-seed that)"""
    props, n, kw, kernel = _converged_2d()
    out = dict(('in/fluid/' + k, v.copy()) for k, v in props.items())
    out['nreal/fluid'] = np.array(n)
    dt = 1e-3
    out['dt'] = np.array(dt)
    out['kernel'] = np.array('CubicSpline')
    out['dim'] = np.array(2)
    tr = Tracer()
    rng = np.random.default_rng(977)
    pert = perturbed(props, rng, ())
    worst = 0.0
    for name, (params, t) in cases.items():
        for tol in TOLS:
            params = dict(params, tol=tol)
            one = Tracer()
            try:
                res = force_only(props, n, kernel, 2, params, t, dt, one)
                one.meta()
            except AssertionError as e:
                print(fname, name, 'tol', tol, 'rejected:', e, flush=True)
                continue
            break
        else:
            raise RuntimeError('%s %s: no tol met the conditions' % (fname, name))
        tr.lines.update(one.lines)
        tr.returns.update(one.returns)
        tr.margin = min(tr.margin, one.margin)
        tr.max_index = max(tr.max_index, one.max_index)
        res_p = force_only(pert, n, kernel, 2, params, t, dt, None)
        worst = max(worst, compare(res, res_p, FORCE_OUT, name))
        for k, v in res.items():
            out['%s/%s/fluid/%s' % (key, name, k)] = v
        out['%s/%s/params' % (key, name)] = np.array(json.dumps(params))
        out['%s/%s/t' % (key, name)] = np.array(t)
        print(fname, name, 'ok', flush=True)
    meta = tr.meta()
    meta['perturbation_1e-13_moves'] = worst
    for k, v in meta.items():
        out['meta/' + k] = np.array(v)
    out['names'] = np.array(json.dumps(list(cases)))
    TOTAL.update(tr.branch_counts())
    return out


def case_solvers():
    base = dict(g1=0.3, g2=0.5, monotonicity=1, interpolation=1, gamma=1.4)
    cases = dict((str(k), (dict(base, rsolver=k), 0.0)) for k in range(11))
    save('gsph_solvers.npz', _force_cases('gsph_solvers', cases, 'solver'))


def _make_coincident(seed):
    rng = np.random.default_rng(seed)
    p1, n1, dx = GG._lattice(2, (10, 8), rng, mvar=0.1, hfac=1.2, hvar=0.05)
    p2, n2, _ = GG._lattice(2, (7, 6), rng, mvar=0.1, hfac=1.2, hvar=0.05)
    p2['x'] = 0.25 + 0.5 * p2['x']
    p2['y'] = 0.2 + 0.5 * p2['y']
    p2['m'] = 0.25 * p2['m'] * 0.6
    p2['h'] = 0.5 * p2['h']
    k = 37
    p2['x'][0], p2['y'][0] = p1['x'][k], p1['y'][k]           # the coincident pair: f2[0] on f1[37]
    props = {}
    for name, lp in (('f1', p1), ('f2', p2)):
        props[name] = _base_props(lp['x'], lp['y'], lp['z'], lp['u'], lp['v'], lp['w'], lp['m'], lp['h'], lp['e'], rng)
    kw = dict(fluids=['f1', 'f2'], solids=[], dim=2, gamma=1.4, kernel_factor=1.2, monotonicity=2, interpolation=2)
    return props, dict(f1=n1, f2=n2), kw, RK.CubicSpline(dim=2)


def case_options():
    cases = {}
    for rs in (2, 3):
        for mono in (0, 1, 2):
            for interp in (0, 1, 2):
                for iz in (True, False):
                    name = 'r%d_m%d_i%d_z%d' % (rs, mono, interp, int(iz))
                    cases[name] = (dict(rsolver=rs, monotonicity=mono, interpolation=interp, interface_zero=iz, gamma=1.4), 0.0)
    cases['hybrid'] = (dict(rsolver=2, monotonicity=1, interpolation=1, hybrid=True, blend_alpha=5.0, tf=0.8, gamma=1.4), 0.3 * 0.8)
    out = _force_cases('gsph_options', cases, 'opt')
    # two fluids with one coincident pair (each sees the other's particle at RIJ = 0): the whole list, IwIn, cubic
    co, _ = evaluate(_make_coincident, range(800, 840), 'gsph_options coincident', prefix='coincident/', t=0.0, dt=1e-4,
                     allow_coincident=2)
    out.update(co)
    save('gsph_options.npz', out)


def case_kernels():
    allout = {}
    for k, name in enumerate(GG.KERNELS):
        cls = getattr(RK, name)

        def make(seed, name=name):
            rng = np.random.default_rng(seed)
            if name.endswith('_1D'):
                dim = 1
                lp, n, dx = GG._lattice(1, (40,), rng, hfac=1.3, hvar=0.1, mvar=0.1)
            else:
                dim = 3
                lp, n, dx = GG._lattice(3, (4, 4, 4), rng, hfac=1.2, hvar=0.1, mvar=0.1)
            props = _base_props(lp['x'], lp['y'], lp['z'], lp['u'], lp['v'], lp['w'], lp['m'], lp['h'], lp['e'], rng)
            kw = dict(fluids=['fluid'], solids=[], dim=dim, gamma=1.4, kernel_factor=1.3 if dim == 1 else 1.2, g1=0.2, g2=0.4)
            return dict(fluid=props), dict(fluid=n), kw, cls(dim=dim)
        out, seed = evaluate(make, range(500 + 20 * k, 520 + 20 * k), 'gsph_kernels ' + name, prefix=name + '/', t=0.0, dt=1e-4)
        allout.update(out)
    allout['kernels'] = np.array(json.dumps(list(GG.KERNELS)))
    save('gsph_kernels.npz', allout)


def case_steppers():
    """the reference's stepper method executed as plain Python on 24 random particles"""
    rng = np.random.default_rng(713)
    n = 24
    names = ['x', 'y', 'z', 'u', 'v', 'w', 'e', 'au', 'av', 'aw', 'ae']
    base = dict((k, rng.uniform(-1, 1, n)) for k in names)
    out = dict(('in/' + k, v.copy()) for k, v in base.items())
    dt = 0.0123
    out['dt'] = np.array(dt)
    st = ListPA('fluid', base, n)
    GG.sweep(GSPHStep(), 'stage1', st, 0.0, dt)
    for k, v in st.properties.items():
        out['gsph/stage1/%s' % k] = np.array(v)
    save('gsph_steppers.npz', out)


STRUCTURES = dict(
    default=dict(fluids=['fluid'], solids=[], dim=2, gamma=1.4, kernel_factor=1.2),
    two_fluids_ghosts=dict(fluids=['f1', 'f2'], solids=[], dim=3, gamma=5.0 / 3.0, kernel_factor=1.5, has_ghosts=True,
                           rsolver=3, interpolation=2, monotonicity=2, interface_zero=False),
    conduction_hybrid=dict(fluids=['fluid'], solids=[], dim=1, gamma=1.4, kernel_factor=1.2, g1=0.2, g2=0.4, hybrid=True,
                           blend_alpha=2.0, tf=0.3, niter=40, tol=1e-8, rsolver=1),
    ghosts=dict(fluids=['fluid'], solids=[], dim=2, gamma=1.4, kernel_factor=1.2, has_ghosts=True, monotonicity=0,
                interpolation=0),
)


def _plain(obj, skip=()):
    return dict((k, v) for k, v in vars(obj).items()
                if k not in skip and not k.startswith('_') and isinstance(v, (bool, int, float, str, dict, type(None))))


def case_structures():
    out = {}
    for name, kw in STRUCTURES.items():
        out[name + '/scheme'] = np.array(json.dumps(kw))
        out[name + '/structure'] = np.array(json.dumps(GG.structure(GSPHScheme(**kw).get_equations())))
    out['names'] = np.array(json.dumps(sorted(STRUCTURES)))
    s = GSPHScheme(['fluid'], [], dim=2, gamma=1.4, kernel_factor=1.2)
    out['choices'] = np.array(json.dumps(dict(rsolver=s.rsolver_choices, interpolation=s.interpolation_choices,
                                              monotonicity=s.monotonicity_choices)))
    # constructor defaults, as the objects hold them
    out['defaults/scheme'] = np.array(json.dumps(_plain(s, ('fluids', 'solids', 'solver', 'rsolver_choices',
                                                            'interpolation_choices', 'monotonicity_choices'))))
    out['defaults/acceleration'] = np.array(json.dumps(_plain(GS.GSPHAcceleration('fluid', ['fluid']), GG.SKIP_ATTRS)))
    save('gsph_structures.npz', out)


def check_total():
    missing = [k for k in REQUIRED if TOTAL.get(k, 0) == 0]
    assert not missing, ('branches never taken', missing)
    assert sum(TOTAL.get(k, 0) > 0 for k in ('hllc_left_star', 'hllc_right_star')) >= 2, 'hllc: fewer than two cases'
    assert sum(TOTAL.get(k, 0) > 0 for k in ('ducowicz_a', 'ducowicz_b', 'ducowicz_c', 'ducowicz_d')) >= 2, 'ducowicz'
    assert TOTAL.get('min_x3_a', 0) + TOTAL.get('min_x3_b', 0) > 0, 'monotonicity_min never returns x3'
    print('branches over all files:', dict(TOTAL))


if __name__ == '__main__':
    which = sys.argv[1:] or ['structures', 'steppers', '1d', '2d', '3d', 'solvers', 'options', 'kernels']
    for name in which:
        globals()['case_' + name]()
    if not sys.argv[1:]:
        check_total()
