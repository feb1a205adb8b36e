#!/usr/bin/env python
"""Golden vectors for gas dynamics, from the REFERENCE's own ``GasDScheme`` (pysph/sph/scheme.py:884-1141), its
equation classes (pysph/sph/gas_dynamics/basic.py) and ``GasDFluidStep`` (pysph/sph/integrator_step.py:351-428), in the
manner of make_edac_golden.py (same driver, same stored layout):

    python tests/golden/make_gasd_golden.py

    gasd_1d.npz          1-D, 120 particles of equal mass with an 8:1 spacing jump, Gaussian, htol = 1e-6; the initial h
                         is wrong by a factor between 0.5 and 1.6, so that both clamps act and several iterations run
    gasd_2d.npz          2-D jittered 18 x 14 lattice, masses +-20 %, random velocities and e, CubicSpline,
                         update_alpha1 = update_alpha2 = True, random alpha1 / alpha2
    gasd_3d.npz          6^3 jittered, QuinticSpline, the scheme's default htol; out/ after one evaluation, out2/ + nnps2/
                         after moving by dt u, the stepper's initialize and a second evaluation
    gasd_kernels.npz     per smoothing kernel class one tiny case, stored under the class name as prefix
    gasd_gsph_h.npz      the adaptive_h_scheme='gsph' group list on the 2-D case
    gasd_steppers.npz    GasDFluidStep initialize / stage1 / stage2 on random columns
    gasd_steps.npz       the 3-D case through three PEC steps
    gasd_structures.npz  group lists only, for the option combinations (has_ghosts included)

``RefEval.compute`` refuses iterated groups, so this script drives the iteration itself as the reference's template
does (acceleration_eval_cython.mako:291-363): run the group, update the neighbours, ask ``converged()``, honour
``min_iterations`` / ``max_iterations``.  Every output property starts as random garbage, so that a missing write shows.

Conditions asserted on the reference alone (re-seeded until met, results under meta/):
  * the iterated group stops on convergence after 2 <= n < max_iterations iterations;
  * at least a tenth of the particles converge before the last iteration (they leave with the raw arho) and at least
    one converges in the last (arho * omega);
  * in the 1-D case both clamps, hnew > 1.2 hi and hnew < 0.8 hi, fire at least once;
  * in no iteration has any particle diff within a relative 1e-3 of htol or |omegai| < 1e-6: a rounding difference
    cannot flip a branch;
  * both signs of ``dot`` in at least a tenth of the pairs each, no pair other than the self pair with
    RIJ < 1e-6 h, e > 0 everywhere.
"""
import json
import os
import sys
import types
from inspect import getfullargspec

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402  (sets up the reference imports)

from oracle.ref_driver import ListPA, PyLinkedListNNPS, RefEval  # noqa: E402

# gas_dynamics/basic.py imports the Cython reduce helpers (SummationDensityADKE.reduce only), the ghost tag and,
# through scheme.py, the particle-array factory: none of them is executed here
for _name, _attrs in (('pysph.base.reduce_array', dict(serial_reduce_array=None, parallel_reduce_array=None)),
                      ('pysph.base.particle_array', dict(get_ghost_tag=lambda: 2)),
                      ('pysph.base.utils', dict(get_particle_array=lambda *a, **k: None,
                                                get_particle_array_gasd=lambda *a, **k: None))):
    if _name not in sys.modules:
        _m = types.ModuleType(_name)
        sys.modules[_name] = _m
    for _k, _v in _attrs.items():
        if not hasattr(sys.modules[_name], _k):
            setattr(sys.modules[_name], _k, _v)

from pysph.sph.acceleration_eval import AccelerationEval  # noqa: E402
from pysph.sph.scheme import GasDScheme  # noqa: E402
from pysph.sph.integrator_step import GasDFluidStep  # noqa: E402
from pysph.base import kernels as RK  # noqa: E402

SKIP_ATTRS = ('dest', 'sources', 'name', 'var_name', 'no_source')
KERNELS = ('CubicSpline', 'WendlandQuintic', 'QuinticSpline', 'Gaussian', 'WendlandQuinticC2_1D', 'WendlandQuinticC4',
           'WendlandQuinticC4_1D', 'WendlandQuinticC6', 'WendlandQuinticC6_1D', 'SuperGaussian')

OUTPUTS = ('rho', 'arho', 'grhox', 'grhoy', 'grhoz', 'dwdh', 'div', 'ah', 'p', 'cs', 'au', 'av', 'aw', 'ae', 'am',
           'del2e', 'dt_cfl', 'aalpha1', 'aalpha2')
SAVES = ('x0', 'y0', 'z0', 'u0', 'v0', 'w0', 'e0', 'rho0', 'alpha10', 'alpha20')


def structure(groups):
    out = []
    for g in groups:
        eqs = []
        for eq in g.equations:
            par = dict((k, (bool(v) if isinstance(v, bool) else float(v))) for k, v in vars(eq).items()
                       if k not in SKIP_ATTRS and not k.startswith('_') and isinstance(v, (bool, int, float))
                       and k != 'equation_has_converged')
            eqs.append(dict(cls=type(eq).__name__, dest=eq.dest, sources=list(eq.sources or []), params=par))
        out.append(dict(real=bool(g.real), update_nnps=bool(g.update_nnps), iterate=bool(g.iterate),
                        max_iterations=int(g.max_iterations), min_iterations=int(g.min_iterations), equations=eqs))
    return out


def _nnps_out(out, nnps, prefix):
    out[prefix + '/cell_size'] = np.array(nnps.cell_size)
    out[prefix + '/xmin'] = np.array(nnps.xmin)
    out[prefix + '/xmax'] = np.array(nnps.xmax)
    out[prefix + '/ncells_per_dim'] = np.array(nnps.nc)
    out[prefix + '/n_cells'] = np.array(nnps.n_cells)


def _store(out, pas, which):
    for pa in pas:
        for k, v in pa.properties.items():
            out['%s/%s/%s' % (which, pa.name, k)] = np.array(v)


class Watch(object):
    """what the density iteration decided, per iteration: ``_decisions`` re-evaluates the branch variables of
    SummationDensity.post_loop from h and ``converged`` as they were before the iteration and rho, dwdh after it"""

    def __init__(self):
        self.iters = []


def run_group(ev, nnps, mg, t, dt, fluid, watch):
    """acceleration_eval_cython.mako:291-363 for one leaf group; returns the iterations it ran"""
    if not mg.iterate:
        ev._do_group(mg, t, dt)
        if mg.update_nnps:
            nnps.update()
        return 1
    count = 1
    while True:
        P = fluid.properties
        before = dict(h=list(P['h']), conv=list(P['converged']))
        ev._do_group(mg, t, dt)
        if watch is not None:
            watch.iters.append(_decisions(mg, fluid, before))
        if mg.update_nnps:
            nnps.update()
        done = all(eq.converged() > 0 for eq in mg._orig_group.equations)
        if count >= mg.min_iterations and (done or count == mg.max_iterations):
            break
        count += 1
    return count


def _decisions(mg, fluid, before):
    """the post_loop's branch variables of one iteration (basic.py:150-213) from h before it, and rho, dwdh after it"""
    eq = [e for e in mg._orig_group.equations if e.dest == fluid.name][0]
    P = fluid.properties
    out = dict(up=0, down=0, newly=[], active=0, min_margin=float('inf'), min_omega=float('inf'))
    for i in range(fluid.n_real):
        if before['conv'][i] == 1:
            continue
        out['active'] += 1
        hi, hi0, mi, rho, dwdh = before['h'][i], P['h0'][i], P['m'][i], P['rho'][i], P['dwdh'][i]
        rhoi = mi / (hi / eq.k) ** eq.dim
        dhdrhoi = -hi / (eq.dim * rho)
        omegai = 1.0 - dhdrhoi * dwdh
        out['min_omega'] = min(out['min_omega'], abs(omegai))
        if omegai < 0:
            omegai = 1.0
        hnew = hi - (rhoi - rho) / (omegai / dhdrhoi)
        if hnew > 1.2 * hi:
            out['up'] += 1
            hnew = 1.2 * hi
        elif hnew < 0.8 * hi:
            out['down'] += 1
            hnew = 0.8 * hi
        assert hnew > 1e-6 and 1.0 / omegai >= 1e-6, 'the fallback branch is not part of these cases'
        diff = abs(hnew - hi) / hi0
        out['min_margin'] = min(out['min_margin'], abs(diff - eq.htol) / eq.htol)
        if P['converged'][i] == 1:
            out['newly'].append(i)
            assert diff < eq.htol
        else:
            assert not diff < eq.htol
    return out


def pair_conditions(fluid, nnps):
    P = dict((k, np.array(fluid.properties[k])) for k in 'xyzuvwhe')
    assert np.all(P['e'] > 0.0), 'e <= 0'
    neg = tot = 0
    for i in range(fluid.n_real):
        nb = np.array(nnps.neighbors(0, 0, i))
        nb = nb[nb != i]
        r = np.sqrt(sum((P[a][i] - P[a][nb]) ** 2 for a in 'xyz'))
        assert np.all(r >= 1e-6 * P['h'][i]), 'a pair closer than 1e-6 h'
        d = sum((P[a][i] - P[a][nb]) * (P[b][i] - P[b][nb]) for a, b in zip('uvw', 'xyz'))
        neg += int(np.sum(d <= 0))
        tot += nb.size
    assert neg * 10 >= tot and (tot - neg) * 10 >= tot, (neg, tot)
    return dict(n_pairs=tot, n_approaching=neg)


def iteration_conditions(watch, n_iter, max_iter, n_real, need_clamps):
    meta = dict(iterations=n_iter)
    assert 2 <= n_iter < max_iter, ('iterations', n_iter)
    assert len(watch.iters) == n_iter
    early = sum(len(it['newly']) for it in watch.iters[:-1])
    last = len(watch.iters[-1]['newly'])
    assert early * 10 >= n_real and last >= 1, ('converged early / last', early, last)
    assert early + last == n_real
    meta.update(n_converged_early=early, n_converged_last=last, n_clamped_up=sum(it['up'] for it in watch.iters),
                n_clamped_down=sum(it['down'] for it in watch.iters),
                min_margin=min(it['min_margin'] for it in watch.iters),
                min_abs_omega=min(it['min_omega'] for it in watch.iters))
    if need_clamps:
        assert meta['n_clamped_up'] >= 1 and meta['n_clamped_down'] >= 1, meta
    assert meta['min_margin'] > 1e-3 and meta['min_abs_omega'] > 1e-6, meta
    return meta


def sweep(step, meth, fluid, t, dt):
    f = getattr(step, meth)
    args = [a for a in getfullargspec(f).args if a != 'self']
    ns = dict(('d_' + k, v) for k, v in fluid.properties.items())
    ns.update(dt=dt, t=t)
    for i in range(fluid.n_real):
        ns['d_idx'] = i
        f(*[ns[a] for a in args])


def evaluate(props, n_real, kw, kernel, t, dt, second=False, steps=0, prefix='', need_clamps=False, conditions=True):
    dim = kw['dim']
    s = GasDScheme(**kw)
    groups = s.get_equations()
    fluid = ListPA('fluid', props, n_real)
    pas = [fluid]
    out = {}
    _store(out, pas, 'in')
    out['nreal/fluid'] = np.array(fluid.n_real)
    a_eval = AccelerationEval(pas, groups, kernel)
    nnps = PyLinkedListNNPS(dim, pas, radius_scale=kernel.radius_scale)
    ev = RefEval(a_eval, nnps)
    meta = {}
    max_iter = kw.get('max_density_iterations', 250)

    def compute(tt, watch):
        counts = [run_group(ev, nnps, mg, tt, dt, fluid, watch if mg.iterate else None) for mg in a_eval.mega_groups]
        return [c for c, mg in zip(counts, a_eval.mega_groups) if mg.iterate]

    mpm = kw.get('adaptive_h_scheme', 'mpm') == 'mpm'
    if steps:
        # pysph/sph/integrator.py:227-246 (PECIntegrator.one_timestep): initialize; stage1; update_domain;
        # compute_accelerations (neighbours rebuilt); stage2; update_domain
        step = GasDFluidStep()
        tt = t
        its = []
        for k in range(steps):
            sweep(step, 'initialize', fluid, tt, dt)
            sweep(step, 'stage1', fluid, tt, dt)
            nnps.update()
            w = Watch()
            n_it = compute(tt + 0.5 * dt, w)[0]
            assert n_it < max_iter
            assert min(it['min_margin'] for it in w.iters) > 1e-3 and min(it['min_omega'] for it in w.iters) > 1e-6
            its.append(n_it)
            sweep(step, 'stage2', fluid, tt, dt)
            tt += dt
        _store(out, pas, 'out')
        meta['steps'] = steps
        out['meta/iterations_per_step'] = np.array(its)
    else:
        nnps.update()
        MG.check_nnps(nnps)
        w = Watch()
        its = compute(t, w)
        _store(out, pas, 'out')
        _nnps_out(out, nnps, 'nnps')
        if mpm and conditions:
            meta.update(iteration_conditions(w, its[0], max_iter, fluid.n_real, need_clamps))
        elif mpm:
            meta['iterations'] = its[0]
            assert its[0] < max_iter
            assert min(it['min_margin'] for it in w.iters) > 1e-3 and min(it['min_omega'] for it in w.iters) > 1e-6
        if conditions:
            meta.update(pair_conditions(fluid, nnps))
        if second:
            P = fluid.properties
            for a, b in zip('xyz', 'uvw'):
                P[a] = [x + dt * u for x, u in zip(P[a], P[b])]
            sweep(GasDFluidStep(), 'initialize', fluid, t, dt)
            nnps.update()
            MG.check_nnps(nnps)
            w = Watch()
            its = compute(t + dt, w)
            assert its[0] < max_iter
            assert min(it['min_margin'] for it in w.iters) > 1e-3 and min(it['min_omega'] for it in w.iters) > 1e-6
            meta['second_iterations'] = its[0]
            _store(out, pas, 'out2')
            _nnps_out(out, nnps, 'nnps2')
    out['t'] = np.array(t)
    out['dt'] = np.array(dt)
    out['structure'] = np.array(json.dumps(structure(groups)))
    out['scheme'] = np.array(json.dumps(kw))
    out['kernel'] = np.array(type(kernel).__name__)
    for k, v in meta.items():
        out['meta/' + k] = np.array(v)
    return dict((prefix + k, v) for k, v in out.items()), meta


def save(fname, out, note=''):
    path = os.path.join(HERE, fname)
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path) // 1024, 'KiB', note)


def _fill(props, rng, n, alpha_random=False):
    """the state columns the caller did not set, and garbage in every output and save column"""
    props.setdefault('alpha1', rng.uniform(0.2, 1.5, n) if alpha_random else np.ones(n))
    props.setdefault('alpha2', rng.uniform(0.05, 0.5, n) if alpha_random else 0.1 * np.ones(n))
    props['h0'] = props['h'].copy()
    props['converged'] = np.zeros(n)
    props['omega'] = np.ones(n)
    for k in OUTPUTS + SAVES:
        props[k] = rng.uniform(-1, 1, n)          # garbage: must be overwritten


def _lattice(dim, shape, rng, jitter=0.2, mvar=0.0, hfac=1.3, hvar=0.0, rho0=1.0):
    dx = 1.0 / shape[0]
    axes = [(np.arange(k) + 0.5) * dx for k in shape]
    grid = [a.ravel() for a in np.meshgrid(*axes, indexing='ij')]
    n = grid[0].size
    props = {}
    for k, c in enumerate('xyz'):
        props[c] = grid[k] + jitter * dx * rng.uniform(-1, 1, n) if k < dim else np.zeros(n)
    for k, c in enumerate('uvw'):
        props[c] = rng.uniform(-1, 1, n) if k < dim else np.zeros(n)
    props['m'] = rho0 * dx ** dim * (1 + mvar * rng.uniform(-1, 1, n))
    props['h'] = hfac * dx * (1 + hvar * rng.uniform(-1, 1, n))
    props['e'] = rng.uniform(1.0, 3.0, n)
    return props, n, dx


def _reseed(fname, seeds, make, **ev_kw):
    for seed in seeds:
        props, n, kw, kernel = make(seed)
        try:
            out, meta = evaluate(props, n, kw, kernel, **ev_kw)
        except AssertionError as e:
            print(fname, 'seed', seed, 'rejected:', e)
            continue
        out['meta/seed'] = np.array(seed)
        save(fname, out, meta)
        return seed
    raise RuntimeError('%s: no seed met the conditions' % fname)


def _make_1d(seed):
    rng = np.random.default_rng(seed)
    nl, nr = 96, 24                       # equal masses: spacing ratio 8 <-> density ratio 8
    dxl = 0.5 / nl
    dxr = 8 * dxl
    x = np.concatenate([-0.5 + (np.arange(nl) + 0.5) * dxl, (np.arange(nr) + 0.5) * dxr])
    n = x.size
    spacing = np.concatenate([dxl * np.ones(nl), dxr * np.ones(nr)])
    props = dict(x=x + 0.1 * spacing * rng.uniform(-1, 1, n), y=np.zeros(n), z=np.zeros(n),
                 u=0.3 * rng.uniform(-1, 1, n), v=np.zeros(n), w=np.zeros(n), m=dxl * np.ones(n),
                 h=1.5 * spacing * rng.uniform(0.5, 1.6, n), e=rng.uniform(1.0, 3.0, n))
    _fill(props, rng, n)
    kw = dict(fluids=['fluid'], solids=[], dim=1, gamma=1.4, kernel_factor=1.5, density_iteration_tolerance=1e-6,
              max_density_iterations=60)
    return props, n, kw, RK.Gaussian(dim=1)


def case_1d():
    _reseed('gasd_1d.npz', range(100, 160), _make_1d, t=0.0, dt=1e-4, need_clamps=True)


def _make_2d(seed, **extra):
    rng = np.random.default_rng(seed)
    props, n, dx = _lattice(2, (18, 14), rng, mvar=0.2, hfac=1.2, hvar=0.15)
    _fill(props, rng, n, alpha_random=True)
    kw = dict(fluids=['fluid'], solids=[], dim=2, gamma=1.4, kernel_factor=1.2, update_alpha1=True, update_alpha2=True,
              alpha1=0.3, alpha2=0.2, beta=2.0, max_density_iterations=60)
    kw.update(extra)
    return props, n, kw, RK.CubicSpline(dim=2)


def case_2d():
    seed = _reseed('gasd_2d.npz', range(200, 260), _make_2d, t=0.0, dt=1e-4)
    # the gsph list on the same particles (no iteration: nothing to re-seed for)
    props, n, kw, kernel = _make_2d(seed, adaptive_h_scheme='gsph')
    out, meta = evaluate(props, n, kw, kernel, t=0.0, dt=1e-4, conditions=False)
    out['meta/seed'] = np.array(seed)
    save('gasd_gsph_h.npz', out, meta)


def _make_3d(seed):
    rng = np.random.default_rng(seed)
    props, n, dx = _lattice(3, (6, 6, 6), rng, hfac=1.2, hvar=0.1)
    _fill(props, rng, n)
    kw = dict(fluids=['fluid'], solids=[], dim=3, gamma=5.0 / 3.0, kernel_factor=1.2, max_density_iterations=60)
    return props, n, kw, RK.QuinticSpline(dim=3)


def case_3d():
    seed = _reseed('gasd_3d.npz', range(300, 360), _make_3d, t=0.0, dt=2e-3, second=True)
    props, n, kw, kernel = _make_3d(seed)
    out, meta = evaluate(props, n, kw, kernel, t=0.0, dt=2e-3, steps=3)
    out['meta/seed'] = np.array(seed)
    save('gasd_steps.npz', out, meta)


def case_kernels():
    allout = {}
    for k, name in enumerate(KERNELS):
        cls = getattr(RK, name)
        for seed in range(500 + 20 * k, 520 + 20 * k):      # (no borderline decision: re-seeded like the others)
            rng = np.random.default_rng(seed)
            if name.endswith('_1D'):
                dim = 1
                props, n, dx = _lattice(1, (40,), rng, hfac=1.3, hvar=0.1, mvar=0.1)
            else:
                dim = 3
                props, n, dx = _lattice(3, (4, 4, 4), rng, hfac=1.2, hvar=0.1, mvar=0.1)
            _fill(props, rng, n, alpha_random=True)
            kw = dict(fluids=['fluid'], solids=[], dim=dim, gamma=1.4, kernel_factor=1.3 if dim == 1 else 1.2,
                      update_alpha1=True, update_alpha2=True, max_density_iterations=60)
            try:
                out, meta = evaluate(props, n, kw, cls(dim=dim), t=0.0, dt=1e-4, prefix=name + '/', conditions=False)
            except AssertionError:
                print(name, 'seed', seed, 'rejected')
                continue
            break
        else:
            raise RuntimeError('%s: no seed met the conditions' % name)
        out[name + '/meta/seed'] = np.array(seed)
        print(name, meta)
        allout.update(out)
    allout['kernels'] = np.array(json.dumps(list(KERNELS)))
    save('gasd_kernels.npz', allout)


def case_steppers():
    """the reference's stepper methods executed as plain Python on 24 random particles"""
    rng = np.random.default_rng(711)
    n = 24
    names = ['x', 'y', 'z', 'u', 'v', 'w', 'e', 'h', 'rho', 'x0', 'y0', 'z0', 'u0', 'v0', 'w0', 'e0', 'h0', 'rho0',
             'au', 'av', 'aw', 'ae', 'ah', 'arho', 'converged', 'omega', 'alpha1', 'alpha2', 'alpha10', 'alpha20',
             'aalpha1', 'aalpha2']
    base = dict((k, rng.uniform(-1, 1, n)) for k in names)
    out = dict(('in/' + k, v.copy()) for k, v in base.items())
    dt = 0.0123
    out['dt'] = np.array(dt)
    step = GasDFluidStep()
    st = ListPA('fluid', base, n)
    for meth in ('initialize', 'stage1', 'stage2'):
        sweep(step, meth, st, 0.0, dt)
        for k, v in st.properties.items():
            out['gasd/%s/%s' % (meth, k)] = np.array(v)
    save('gasd_steppers.npz', out)


STRUCTURES = dict(
    mpm_default=dict(fluids=['fluid'], solids=[], dim=2, gamma=1.4, kernel_factor=1.2),
    mpm_two_fluids=dict(fluids=['f1', 'f2'], solids=[], dim=3, gamma=1.4, kernel_factor=1.5, alpha1=0.5, alpha2=0.3,
                        beta=1.5, max_density_iterations=30, density_iteration_tolerance=1e-4),
    mpm_update_alphas=dict(fluids=['fluid'], solids=[], dim=1, gamma=1.4, kernel_factor=1.2, update_alpha1=True,
                           update_alpha2=True),
    mpm_ghosts=dict(fluids=['fluid'], solids=[], dim=2, gamma=1.4, kernel_factor=1.2, has_ghosts=True),
    gsph_default=dict(fluids=['fluid'], solids=[], dim=2, gamma=1.4, kernel_factor=1.2, adaptive_h_scheme='gsph'),
    gsph_ghosts_two_fluids=dict(fluids=['f1', 'f2'], solids=[], dim=3, gamma=5.0 / 3.0, kernel_factor=1.3,
                                adaptive_h_scheme='gsph', has_ghosts=True, update_alpha1=True),
)


def case_structures():
    out = {}
    for name, kw in STRUCTURES.items():
        out[name + '/scheme'] = np.array(json.dumps(kw))
        out[name + '/structure'] = np.array(json.dumps(structure(GasDScheme(**kw).get_equations())))
    out['names'] = np.array(json.dumps(sorted(STRUCTURES)))
    save('gasd_structures.npz', out)


if __name__ == '__main__':
    which = sys.argv[1:] or ['structures', 'steppers', '1d', '2d', '3d', 'kernels']
    for name in which:
        globals()['case_' + name]()
