#!/usr/bin/env python
"""Golden vectors for ADKE gas dynamics, from the REFERENCE's own ``ADKEScheme`` (pysph/sph/scheme.py:1461-1644), its
equation classes (pysph/sph/gas_dynamics/basic.py, boundary_equations.py) and ``ADKEStep``
(pysph/sph/integrator_step.py:452-499), in the manner of make_gasd_golden.py (same driver, same stored layout):

    python tests/golden/make_adke_golden.py

    adke_1d.npz          1-D, 120 particles of equal mass with an 8:1 spacing jump, Gaussian, eps = 0.2 (with 0.5 the
                         free right end takes lambda = 2.7: beyond any cell grid sized by 2 h0)
    adke_2d.npz          18 x 14 jittered fluid with a 2.5:1 mass jump over a three-row wall, CubicSpline, eps = 0.5,
                         k = 1, g1 = 0.5, g2 = 1.0; out/ after one evaluation, out2/ + nnps2/ after moving by dt u, the
                         stepper's initialize and a second evaluation
    adke_3d.npz          6^3 jittered fluid with a one-cell wall layer on one face, QuinticSpline
    adke_two_fluids.npz  two interleaved fluids and a wall, eps = 0.5: the second fluid's sweep sees the first one's new h
    adke_ghost_rows.npz  has_ghosts, one array with n_real < n whose rows behind the real ones carry orig_idx, their own
                         h0 and stale rho, logrho
    adke_kernels.npz     per smoothing kernel class one tiny case, stored under the class name as prefix
    adke_steppers.npz    ADKEStep initialize / stage1 / stage2 on random columns
    adke_steps.npz       the 2-D case through three PEC steps
    adke_structures.npz  group lists only, solids and has_ghosts in all four combinations

``RefEval`` runs no ``reduce``: this script drives it one destination at a time and calls the equation's own ``reduce``
right behind that destination's ``post_loop`` (acceleration_eval_cython.mako:22-131), through a NumPy view of the
``ListPA``; gas_dynamics.basic gets a ``serial_reduce_array`` that is ``numpy.sum`` and an identity
``parallel_reduce_array``.  Every output column starts as random garbage, so that a missing write shows.

Conditions asserted on the reference alone (re-seeded until met, figures under meta/):
  1. at every pair sweep every h of the two arrays of the sweep is <= the hmax the last neighbour update saw, and the
     linked-list neighbours of every destination equal the brute-force ones at that moment (the initial h column is
     2 h0: ``initialize`` overwrites it, but it sizes the cells);
  2. lambda = h / h0 spans at least [0.8, 1.4] in adke_2d, adke_3d and adke_two_fluids (meta/lambda_min, lambda_max;
     the small ghost-row and per-kernel cases store the figures only: 0.83 .. 1.34 and about 0.8 .. 1.4);
  3. both signs of XIJ.VIJ in at least a tenth of the pairs of the force sweep each;
  4. |div| - div non-zero for a tenth of the fluid particles and zero for a tenth;
  5. rho, e > 0;
  6. no pair except the self pairs closer than 1e-6 h;
  7. every wall row has wij > 1e-30 (otherwise IdealGasEOS raises in Python);
  8. a relative 1e-13 on every input moves no result by more than 1e-9 of its field maximum (meta/conditioning).
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402,F401  (sets up the reference imports)
import make_gasd_golden as GG  # noqa: E402  (its module stubs; structure, sweep, save)

from oracle.ref_driver import ListPA, PyLinkedListNNPS, RefEval  # noqa: E402

from pysph.sph.acceleration_eval import AccelerationEval  # noqa: E402
from pysph.sph.gas_dynamics import basic as RB  # noqa: E402
from pysph.sph.scheme import ADKEScheme  # noqa: E402
from pysph.sph.integrator_step import ADKEStep  # noqa: E402
from pysph.base import kernels as RK  # noqa: E402

RB.serial_reduce_array = lambda arr, op='sum': np.sum(arr)
RB.parallel_reduce_array = lambda val, op='sum': val

KERNELS = GG.KERNELS
FLUID_OUT = ('rho', 'arho', 'div', 'logrho', 'p', 'cs', 'au', 'av', 'aw', 'ae', 'am', 'ah', 'wij', 'htmp',
             'x0', 'y0', 'z0', 'u0', 'v0', 'w0', 'e0', 'rho0')
WALL_OUT = FLUID_OUT + ('u', 'v', 'w', 'm', 'e')


class Rejected(AssertionError):
    pass


def need(cond, *what):
    if not cond:
        raise Rejected(what)


class NumpyView(object):
    """what ``SummationDensityADKE.reduce`` touches of its destination: x (for the count), logrho, rho, h0 and h"""

    def __init__(self, pa):
        for k in ('x', 'logrho', 'rho', 'h0', 'h'):
            setattr(self, k, np.array(pa.properties[k]))


class CheckedNNPS(PyLinkedListNNPS):
    """condition 1, asked at the moment of every sweep"""

    def update(self):
        PyLinkedListNNPS.update(self)
        self.hmax_seen = self.cell_size / self.radius_scale
        self.margin = getattr(self, 'margin', float('inf'))
        self.n_lists = getattr(self, 'n_lists', 0)

    def neighbors(self, src, dst, d_idx):
        got = PyLinkedListNNPS.neighbors(self, src, dst, d_idx)
        for a in (src, dst):
            hm = max(self.particles[a].properties['h'])
            need(hm <= self.hmax_seen, 'h beyond the cells', hm, self.hmax_seen)
            self.margin = min(self.margin, 1.0 - hm / self.hmax_seen)
        need(sorted(got) == self.brute_force(src, dst, d_idx), 'linked list != brute force', src, dst, d_idx)
        self.n_lists += 1
        return got


def do_group(ev, mg, t, dt, stats):
    """one leaf group, destination by destination, each with its reduce behind its post_loop"""
    for dest, item in mg.data.items():
        one = types.SimpleNamespace(data={dest: item}, start_idx=mg.start_idx, stop_idx=mg.stop_idx, real=mg.real)
        ev._do_group(one, t, dt)
        dst = ev.arrays[dest]
        for eq in item[2].equations:
            name = type(eq).__name__
            if name == 'WallBoundary':
                need(min(dst.properties['wij'][:dst.n_real]) > 1e-30, 'a wall row no fluid particle reaches')
            if hasattr(eq, 'reduce'):
                view = NumpyView(dst)
                eq.reduce(view, t, dt)
                dst.properties['h'] = [float(v) for v in view.h]
                lam = view.h[:dst.n_real] / view.h0[:dst.n_real]
                stats['lambda_min'] = min(stats.get('lambda_min', np.inf), float(lam.min()))
                stats['lambda_max'] = max(stats.get('lambda_max', -np.inf), float(lam.max()))
    if mg.update_nnps:
        ev.nnps.update()


def compute(ev, a_eval, t, dt, stats):
    for mg in a_eval.mega_groups:
        assert not mg.has_subgroups and not mg.iterate
        do_group(ev, mg, t, dt, stats)


def force_conditions(pas, fluids, nnps, stats):
    """conditions 3..6 at the state the force sweep saw"""
    neg = tot = 0
    idx = dict((pa.name, k) for k, pa in enumerate(pas))
    for pa in pas:
        if pa.name not in fluids:
            continue
        P = dict((k, np.array(pa.properties[k])) for k in ('x', 'y', 'z', 'u', 'v', 'w', 'h', 'e', 'rho', 'div'))
        n = pa.n_real
        need(np.all(P['e'][:n] > 0) and np.all(P['rho'][:n] > 0), 'rho, e > 0')
        pos = int(np.sum(np.abs(P['div'][:n]) - P['div'][:n] != 0.0))
        need(pos * 10 >= n and (n - pos) * 10 >= n, '|div| - div', pos, n)
        stats['n_div_negative'] = stats.get('n_div_negative', 0) + pos
        for src in pas:
            S = dict((k, np.array(src.properties[k])) for k in ('x', 'y', 'z', 'u', 'v', 'w'))
            for i in range(n):
                nb = np.array(PyLinkedListNNPS.neighbors(nnps, idx[src.name], idx[pa.name], i), dtype=int)
                if src is pa:
                    nb = nb[nb != i]
                if nb.size == 0:
                    continue
                r = np.sqrt(sum((P[a][i] - S[a][nb]) ** 2 for a in 'xyz'))
                need(np.all(r >= 1e-6 * P['h'][i]), 'a pair closer than 1e-6 h')
                d = sum((P[a][i] - S[a][nb]) * (P[b][i] - S[b][nb]) for a, b in zip('xyz', 'uvw'))
                neg += int(np.sum(d < 0))
                tot += nb.size
    need(neg * 10 >= tot and (tot - neg) * 10 >= tot, 'signs of XIJ.VIJ', neg, tot)
    stats.update(n_pairs=tot, n_approaching=neg)


def _list_pa(name, props, n_real):
    pa = ListPA(name, props, n_real)
    for k in ('orig_idx', 'tag'):
        if k in pa.properties:
            pa.properties[k] = [int(v) for v in props[k]]
    return pa


def _store(out, pas, which):
    for pa in pas:
        for k, v in pa.properties.items():
            out['%s/%s/%s' % (which, pa.name, k)] = np.array(v)


def run(arrays, kw, kernel, t, dt, second=False, steps=0, lam_range=None, conditions=True, perturb=None):
    """arrays: [(name, props, n_real)]; returns (out, stats)"""
    dim = kw['dim']
    s = ADKEScheme(**kw)
    groups = s.get_equations()
    if perturb is not None:
        arrays = [(name, dict((k, (v * (1.0 + 1e-13 * perturb.choice([-1.0, 1.0], v.shape))
                                   if v.dtype == np.float64 and k != 'tag' else v)) for k, v in props.items()), n)
                  for name, props, n in arrays]
    pas = [_list_pa(name, props, n) for name, props, n in arrays]
    out, stats = {}, {}
    _store(out, pas, 'in')
    for pa in pas:
        out['nreal/' + pa.name] = np.array(pa.n_real)
    a_eval = AccelerationEval(pas, groups, kernel)
    nnps = CheckedNNPS(dim, pas, radius_scale=kernel.radius_scale)
    ev = RefEval(a_eval, nnps)
    fluids = list(kw['fluids'])
    try:
        if steps:
            # pysph/sph/integrator.py:227-246 (PECIntegrator.one_timestep)
            step = ADKEStep()
            tt = t
            for k in range(steps):
                for pa in pas:
                    if pa.name in fluids:
                        GG.sweep(step, 'initialize', pa, tt, dt)
                        GG.sweep(step, 'stage1', pa, tt, dt)
                nnps.update()
                compute(ev, a_eval, tt + 0.5 * dt, dt, stats)
                for pa in pas:
                    if pa.name in fluids:
                        GG.sweep(step, 'stage2', pa, tt, dt)
                tt += dt
            _store(out, pas, 'out')
            stats['steps'] = steps
        else:
            nnps.update()
            compute(ev, a_eval, t, dt, stats)
            _store(out, pas, 'out')
            GG._nnps_out(out, nnps, 'nnps')
            if conditions:
                force_conditions(pas, fluids, nnps, stats)
            if second:
                for pa in pas:
                    if pa.name not in fluids:
                        continue
                    P = pa.properties
                    for a, b in zip('xyz', 'uvw'):
                        P[a] = [x + dt * u for x, u in zip(P[a], P[b])]
                    GG.sweep(ADKEStep(), 'initialize', pa, t, dt)
                nnps.update()
                compute(ev, a_eval, t + dt, dt, stats)
                _store(out, pas, 'out2')
                GG._nnps_out(out, nnps, 'nnps2')
    except ZeroDivisionError as e:
        raise Rejected('ZeroDivisionError', str(e))
    if lam_range is not None:
        need(stats['lambda_min'] <= lam_range[0] and stats['lambda_max'] >= lam_range[1], 'lambda range', stats)
    stats['h_margin'] = nnps.margin
    stats['n_neighbour_lists_checked'] = nnps.n_lists
    need(nnps.nc[0] >= 1)
    stats['ncells'] = [int(v) for v in nnps.nc]
    out['t'] = np.array(t)
    out['dt'] = np.array(dt)
    out['structure'] = np.array(json.dumps(GG.structure(groups)))
    out['scheme'] = np.array(json.dumps(kw))
    out['kernel'] = np.array(type(kernel).__name__)
    return out, stats


def conditioning(out, arrays, kw, kernel, seed, **run_kw):
    """condition 8"""
    out_p, _ = run(arrays, kw, kernel, perturb=np.random.default_rng(seed + 7919), conditions=False, **run_kw)
    worst = 0.0
    for key in out:
        if key.split('/')[0] not in ('out', 'out2') or key.endswith('/tag') or key.endswith('/orig_idx'):
            continue
        a, b = out[key], out_p[key]
        scale = np.abs(a).max()
        if scale > 0:
            worst = max(worst, float(np.abs(a - b).max() / scale))
    need(worst < 1e-9, 'conditioning', worst)
    return worst


def finish(out, stats, prefix=''):
    for k, v in stats.items():
        out['meta/' + k] = np.array(v)
    return dict((prefix + k, v) for k, v in out.items())


def _reseed(fname, seeds, make, cond=True, **run_kw):
    for seed in seeds:
        arrays, kw, kernel = make(seed)
        try:
            out, stats = run(arrays, kw, kernel, **run_kw)
            if cond:
                stats['conditioning'] = conditioning(out, arrays, kw, kernel, seed,
                                                     **dict((k, v) for k, v in run_kw.items() if k not in ('lam_range',)))
        except Rejected as e:
            print(fname, 'seed', seed, 'rejected:', e)
            continue
        stats['seed'] = seed
        GG.save(fname, finish(out, stats), stats)
        return seed
    raise RuntimeError('%s: no seed met the conditions' % fname)


# -- particles ---------------------------------------------------------------------------------------------------------
def _columns(props, rng, n, h0, outs, hinit=2.0):
    props['h0'] = h0
    props['h'] = hinit * h0                          # sizes the cells of the first neighbour update; initialize overwrites it
    for k in outs:
        if k not in props:
            props[k] = rng.uniform(-1, 1, n)       # garbage: must be overwritten (am, ah: must stay)
    return props


def _fluid(dim, shape, rng, dx, origin=(0.0, 0.0, 0.0), jitter=0.2, mjump=1.0, hfac=1.2, hvar=0.1):
    axes = [origin[k] + (np.arange(s) + 0.5) * dx for k, s in enumerate(shape)]
    grid = [a.ravel() for a in np.meshgrid(*axes, indexing='ij')]
    n = grid[0].size
    props = {}
    for k, c in enumerate('xyz'):
        props[c] = grid[k] + jitter * dx * rng.uniform(-1, 1, n) if k < dim else np.zeros(n)
    for k, c in enumerate('uvw'):
        props[c] = rng.uniform(-1, 1, n) if k < dim else np.zeros(n)
    right = grid[0] > origin[0] + 0.5 * shape[0] * dx
    props['m'] = dx ** dim * np.where(right, 1.0, mjump) * (1 + 0.05 * rng.uniform(-1, 1, n))
    props['e'] = rng.uniform(1.0, 3.0, n)
    return _columns(props, rng, n, hfac * dx * (1 + hvar * rng.uniform(-1, 1, n)), FLUID_OUT), n


def _wall(dim, shape, rng, dx, origin, hfac=1.2):
    """a wall lattice; its h column starts as h0 (its h0 may be the larger one: the fluid's 2 h0 sizes the cells)"""
    axes = [origin[k] + (np.arange(s) + 0.5) * dx for k, s in enumerate(shape)]
    grid = [a.ravel() for a in np.meshgrid(*axes, indexing='ij')]
    n = grid[0].size
    props = {}
    for k, c in enumerate('xyz'):
        props[c] = grid[k] if k < dim else np.zeros(n)
    return _columns(props, rng, n, hfac * dx * (1 + 0.03 * rng.uniform(-1, 1, n)), WALL_OUT, hinit=1.0), n


def _make_1d(seed):
    rng = np.random.default_rng(seed)
    nl, nr = 96, 24
    dxl = 0.5 / nl
    dxr = 8 * dxl
    x = np.concatenate([-0.5 + (np.arange(nl) + 0.5) * dxl, (np.arange(nr) + 0.5) * dxr])
    n = x.size
    spacing = np.concatenate([dxl * np.ones(nl), dxr * np.ones(nr)])
    props = dict(x=x + 0.1 * spacing * rng.uniform(-1, 1, n), y=np.zeros(n), z=np.zeros(n),
                 u=0.3 * rng.uniform(-1, 1, n), v=np.zeros(n), w=np.zeros(n), m=dxl * np.ones(n),
                 e=rng.uniform(1.0, 3.0, n))
    _columns(props, rng, n, 1.5 * spacing, FLUID_OUT)
    kw = dict(fluids=['fluid'], solids=[], dim=1, gamma=1.4, alpha=1.0, beta=1.0, k=1.0, eps=0.2, g1=0.2, g2=0.4)
    return [('fluid', props, n)], kw, RK.Gaussian(dim=1)


def case_1d():
    _reseed('adke_1d.npz', range(100, 160), _make_1d, t=0.0, dt=1e-4)


def _make_2d(seed):
    rng = np.random.default_rng(seed)
    dx = 1.0 / 18
    fluid, nf = _fluid(2, (18, 14), rng, dx, mjump=2.5)
    wall, nw = _wall(2, (18, 3), rng, dx, origin=(0.0, -3 * dx, 0.0), hfac=1.7)   # (the third row must reach the fluid)
    kw = dict(fluids=['fluid'], solids=['wall'], dim=2, gamma=1.4, alpha=1.0, beta=2.0, k=1.0, eps=0.5, g1=0.5, g2=1.0)
    return [('fluid', fluid, nf), ('wall', wall, nw)], kw, RK.CubicSpline(dim=2)


def case_2d():
    seed = _reseed('adke_2d.npz', range(200, 260), _make_2d, t=0.0, dt=1e-4, second=True, lam_range=(0.8, 1.4))
    for s2 in range(seed, seed + 40):           # three PEC steps: condition 1 must hold at every sweep of all of them
        arrays, kw, kernel = _make_2d(s2)
        try:
            out, stats = run(arrays, kw, kernel, t=0.0, dt=1e-4, steps=3, conditions=False)
        except Rejected as e:
            print('adke_steps seed', s2, 'rejected:', e)
            continue
        stats['seed'] = s2
        GG.save('adke_steps.npz', finish(out, stats), stats)
        return
    raise RuntimeError('adke_steps: no seed met the conditions')


def _make_3d(seed):
    rng = np.random.default_rng(seed)
    dx = 1.0 / 6
    fluid, nf = _fluid(3, (6, 6, 6), rng, dx, mjump=1.5)
    wall, nw = _wall(3, (6, 6, 1), rng, dx, origin=(0.0, 0.0, -dx))
    kw = dict(fluids=['fluid'], solids=['wall'], dim=3, gamma=5.0 / 3.0, alpha=1.0, beta=2.0, k=1.0, eps=0.5, g1=0.3, g2=0.7)
    return [('fluid', fluid, nf), ('wall', wall, nw)], kw, RK.QuinticSpline(dim=3)


def case_3d():
    _reseed('adke_3d.npz', range(300, 360), _make_3d, t=0.0, dt=1e-4, lam_range=(0.8, 1.4))


def _make_two_fluids(seed):
    rng = np.random.default_rng(seed)
    dx = 1.0 / 14
    both, n = _fluid(2, (14, 10), rng, dx, mjump=2.5)
    pick = rng.uniform(size=n) < 0.5
    arrays = []
    for name, sel in (('f1', pick), ('f2', ~pick)):
        arrays.append((name, dict((k, v[sel].copy()) for k, v in both.items()), int(sel.sum())))
    wall, nw = _wall(2, (14, 3), rng, dx, origin=(0.0, -3 * dx, 0.0), hfac=1.7)
    arrays.append(('wall', wall, nw))
    kw = dict(fluids=['f1', 'f2'], solids=['wall'], dim=2, gamma=1.4, alpha=1.0, beta=2.0, k=1.0, eps=0.5, g1=0.5, g2=1.0)
    return arrays, kw, RK.CubicSpline(dim=2)


def case_two_fluids():
    _reseed('adke_two_fluids.npz', range(400, 460), _make_two_fluids, t=0.0, dt=1e-4, lam_range=(0.8, 1.4))


def _make_ghost_rows(seed):
    rng = np.random.default_rng(seed)
    dx = 1.0 / 12
    fluid, n = _fluid(2, (12, 10), rng, dx, mjump=1.5)
    # the rows behind the real ones: copies of the two leftmost columns, moved to the right of the block
    src = np.where(fluid['x'] < 2 * dx + 0.3 * dx)[0][:24]
    ng = src.size
    props = dict((k, np.concatenate([v, v[src]])) for k, v in fluid.items())
    props['x'][n:] += 1.0
    props['h0'][n:] *= 1 + 0.05 * rng.uniform(-1, 1, ng)              # their own h0
    props['h'][n:] = 2.0 * props['h0'][n:]
    props['rho'][n:] = rng.uniform(0.8, 1.6, ng)                      # stale, but a density
    props['logrho'][n:] = rng.uniform(-0.5, 0.5, ng)                  # stale
    props['div'][n:] = rng.uniform(-1, 1, ng)
    props['orig_idx'] = np.concatenate([np.arange(n), src]).astype(np.int64)
    props['tag'] = np.concatenate([np.zeros(n), 2 * np.ones(ng)]).astype(np.int32)
    kw = dict(fluids=['fluid'], solids=[], dim=2, gamma=1.4, alpha=1.0, beta=2.0, k=1.0, eps=0.5, g1=0.5, g2=1.0,
              has_ghosts=True)
    return [('fluid', props, n)], kw, RK.CubicSpline(dim=2)


def case_ghost_rows():
    _reseed('adke_ghost_rows.npz', range(450, 500), _make_ghost_rows, t=0.0, dt=1e-4)


def case_kernels():
    allout = {}
    for k, name in enumerate(KERNELS):
        cls = getattr(RK, name)
        for seed in range(500 + 20 * k, 520 + 20 * k):
            rng = np.random.default_rng(seed)
            if name.endswith('_1D'):
                dim = 1
                dx = 1.0 / 40
                fluid, nf = _fluid(1, (40,), rng, dx, mjump=1.5, hfac=1.3)
                wall, nw = _wall(1, (3,), rng, dx, origin=(-3 * dx, 0.0, 0.0), hfac=1.8)
            else:
                dim = 3
                dx = 1.0 / 4
                fluid, nf = _fluid(3, (4, 4, 4), rng, dx, mjump=1.5)
                wall, nw = _wall(3, (4, 4, 1), rng, dx, origin=(0.0, 0.0, -dx))
            kw = dict(fluids=['fluid'], solids=['wall'], dim=dim, gamma=1.4, alpha=1.0, beta=2.0, k=1.0, eps=0.5, g1=0.5, g2=1.0)
            try:
                out, stats = run([('fluid', fluid, nf), ('wall', wall, nw)], kw, cls(dim=dim), t=0.0, dt=1e-4, conditions=False)
            except Rejected as e:
                print(name, 'seed', seed, 'rejected', e)
                continue
            break
        else:
            raise RuntimeError('%s: no seed met the conditions' % name)
        stats['seed'] = seed
        print(name, stats)
        allout.update(finish(out, stats, name + '/'))
    allout['kernels'] = np.array(json.dumps(list(KERNELS)))
    GG.save('adke_kernels.npz', allout)


def case_steppers():
    """the reference's stepper methods executed as plain Python on 24 random particles"""
    rng = np.random.default_rng(712)
    n = 24
    names = ['x', 'y', 'z', 'u', 'v', 'w', 'e', 'rho', 'x0', 'y0', 'z0', 'u0', 'v0', 'w0', 'e0', 'rho0',
             'au', 'av', 'aw', 'ae', 'arho']
    base = dict((k, rng.uniform(-1, 1, n)) for k in names)
    out = dict(('in/' + k, v.copy()) for k, v in base.items())
    dt = 0.0123
    out['dt'] = np.array(dt)
    step = ADKEStep()
    st = ListPA('fluid', base, n)
    for meth in ('initialize', 'stage1', 'stage2'):
        GG.sweep(step, meth, st, 0.0, dt)
        for k, v in st.properties.items():
            out['adke/%s/%s' % (meth, k)] = np.array(v)
    GG.save('adke_steppers.npz', out)


STRUCTURES = dict(
    plain=dict(fluids=['fluid'], solids=[], dim=2),
    ghosts=dict(fluids=['fluid'], solids=[], dim=1, gamma=1.4, alpha=1.0, beta=1.0, k=0.3, eps=0.5, g1=0.2, g2=0.4,
                has_ghosts=True),
    solids=dict(fluids=['fluid'], solids=['wall'], dim=2, gamma=5.0 / 3.0, k=1.5, eps=0.3, g1=0.5, g2=1.0),
    solids_ghosts_two_fluids=dict(fluids=['f1', 'f2'], solids=['w1', 'w2'], dim=3, gamma=1.4, alpha=0.5, beta=1.5, k=1.0,
                                  eps=0.5, g1=0.1, g2=0.2, has_ghosts=True),
)


def case_structures():
    out = {}
    for name, kw in STRUCTURES.items():
        out[name + '/scheme'] = np.array(json.dumps(kw))
        out[name + '/structure'] = np.array(json.dumps(GG.structure(ADKEScheme(**kw).get_equations())))
    out['names'] = np.array(json.dumps(sorted(STRUCTURES)))
    GG.save('adke_structures.npz', out)


if __name__ == '__main__':
    which = sys.argv[1:] or ['structures', 'steppers', '1d', '2d', '3d', 'two_fluids', 'ghost_rows', 'kernels']
    for name in which:
        globals()['case_' + name]()
