#!/usr/bin/env python
"""Golden vectors for the WCSPHScheme options delta_sph, nu and update_h, from
the REFERENCE's own equation classes and its own ``WCSPHScheme``, in the
manner of make_more_kernels_golden.py (same driver, same stored layout):

    python tests/golden/make_wcsph_options_golden.py

    opt_dsph3d.npz       3-D 6^3 fluid (last 20 rows ghosts), delta_sph, nu, update_h, WendlandQuintic;
                         out/ after one evaluation, out2/ + nnps2/ after a neighbour update and a second one
    opt_dsph2d_tank.npz  2-D fluid block over three boundary layers, delta_sph, hg_correction, h +-10 %,
                         WendlandQuinticC4
    opt_lamvisc3d.npz    3-D fluid + solid, LaminarViscosity, tensile correction, CubicSpline
    opt_dsph3d_gap.npz   the first case (one evaluation) with GradientCorrection.tol in the middle of the
                         widest gap between the `change` values of its pairs (the fp32 runs)
    opt_singular.npz     an isolated particle, a lone pair and a collinear triple next to a 4^3 block;
                         GradientCorrection.dim = 3, so that the 3 x 3 elimination runs as well

Every file stores the group list as the reference wrote it (``structure``: JSON
of class name, dest, sources, real and the scalar attributes of every
equation), the keyword arguments of the scheme (``scheme``), the attributes
changed after ``get_equations()`` (``overrides``) and the smoothing kernel.

``GradientCorrection`` keeps or drops its corrected gradient by a threshold
(``change < tol``).  A pair whose ``change`` lies next to ``tol`` would take
either branch depending on the last bits of the solve, so the generator
asserts a margin (stored under ``meta/``): 1e-6 in the fp64 cases, 5e-4 in the
gap case, and that both branches are taken by at least a tenth of the pairs.

The driver's ``RefEval`` knows no ``loop_all``; ``OptEval`` below runs it
behind ``initialize`` over the driver's own neighbour lists.  The stub
``declare`` of oracle/_stubs returns None for ``declare('int', 4)``: the three
modules that unpack it get oracle.py_eval.declare.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402  (sets up the reference imports)

from oracle.py_eval import declare as _declare  # noqa: E402
from oracle.ref_driver import ListPA, PyLinkedListNNPS, RefEval  # noqa: E402

import pysph.sph.wc.kernel_correction as _KC  # noqa: E402
import pysph.sph.wc.density_correction as _DC  # noqa: E402
import pysph.sph.wc.linalg as _LA  # noqa: E402

for _m in (_KC, _DC, _LA):
    _m.declare = _declare

from pysph.sph.acceleration_eval import AccelerationEval  # noqa: E402
from pysph.sph.scheme import WCSPHScheme  # noqa: E402
from pysph.base import kernels as RK  # noqa: E402

SKIP_ATTRS = ('dest', 'sources', 'name', 'var_name', 'no_source')


class OptEval(RefEval):
    """RefEval + ``loop_all`` (acceleration_eval_cython.mako:62-83): the groups that have one here hold nothing but
    GradientCorrectionPreStep (initialize + loop_all), so running it behind the base class's pass keeps the order"""

    def _do_group(self, group, t, dt):
        RefEval._do_group(self, group, t, dt)
        for dest, (no_src, sources, all_eqs) in group.data.items():
            dst = self.arrays[dest]
            stop = dst.get_number_of_particles(group.real)
            for source, eq_group in sources.items():
                eqs = [eq for eq in eq_group.equations if hasattr(eq, 'loop_all')]
                if not eqs:
                    continue
                assert all(not hasattr(eq, 'loop') and not hasattr(eq, 'post_loop') for eq in all_eqs.equations)
                ns = self._ns(dst, self.arrays[source], t, dt)
                si, di = self.index[source], self.index[dest]
                for d_idx in range(stop):
                    nb = self.nnps.neighbors(si, di, d_idx)
                    ns.update(d_idx=d_idx, NBRS=nb, N_NBRS=len(nb))
                    for eq in eqs:
                        self._call(eq, 'loop_all', ns)


CHANGES = []        # `change` of every pair GradientCorrection.loop saw (DWIJ != 0), while recording


def _recording_loop(self, d_idx, d_m_mat, DWIJ, HIJ):
    n = self.dim
    dw = list(DWIJ)
    _orig_loop(self, d_idx, d_m_mat, DWIJ, HIJ)
    dmag = sum(abs(dw[i]) for i in range(n))
    if dmag == 0.0:
        return
    # the same statements once more for the number itself (kernel_correction.py:98-120)
    nt = n + 1
    temp = [0.0] * 12
    res = [0.0] * 3
    for i in range(n):
        for j in range(n):
            temp[nt * i + j] = d_m_mat[9 * d_idx + 3 * i + j]
        temp[nt * i + n] = dw[i]
    _LA.gj_solve(temp, n, 1, res)
    rmag = sum(abs(res[i]) for i in range(n))
    CHANGES.append(abs(rmag - dmag) / (dmag + 1.0e-04 * HIJ))


_orig_loop = _KC.GradientCorrection.loop
_KC.GradientCorrection.loop = _recording_loop


def structure(groups):
    out = []
    for g in groups:
        eqs = []
        for eq in g.equations:
            par = dict((k, (bool(v) if isinstance(v, bool) else float(v))) for k, v in vars(eq).items()
                       if k not in SKIP_ATTRS and not k.startswith('_') and isinstance(v, (bool, int, float)))
            eqs.append(dict(cls=type(eq).__name__, dest=eq.dest, sources=list(eq.sources or []), params=par))
        out.append(dict(real=bool(g.real), equations=eqs))
    return out


def apply_overrides(groups, overrides):
    for cls, attr, value in overrides:
        for g in groups:
            for eq in g.equations:
                if type(eq).__name__ == cls:
                    setattr(eq, attr, value)


def margins(tol):
    ch = np.array(CHANGES)
    return dict(margin=float(np.min(np.abs(ch - tol))), n_pairs=ch.size, n_corrected=int(np.sum(ch < tol)))


def run(fname, arrays, kw, kernel, overrides=(), second=False, margin=None, t=0.0, dt=1e-4, extra_meta=None,
        need_both=True):
    """arrays: [(name, props, n_real)]; kw: keyword arguments of the reference's WCSPHScheme.  Returns the recorded
    `change` values of the (last) evaluation."""
    dim = kw['dim']
    s = WCSPHScheme(**kw)
    groups = s.get_equations()
    apply_overrides(groups, overrides)
    pas = [ListPA(name, props, n_real) for name, props, n_real in arrays]
    out = {}
    for pa in pas:
        for k, v in pa.properties.items():
            out['in/%s/%s' % (pa.name, k)] = np.array(v)
        out['nreal/%s' % pa.name] = np.array(pa.n_real)
    a_eval = AccelerationEval(pas, groups, kernel)
    nnps = PyLinkedListNNPS(dim, pas, radius_scale=kernel.radius_scale)

    def nnps_out(prefix):
        out[prefix + '/cell_size'] = np.array(nnps.cell_size)
        out[prefix + '/xmin'] = np.array(nnps.xmin)
        out[prefix + '/xmax'] = np.array(nnps.xmax)
        out[prefix + '/ncells_per_dim'] = np.array(nnps.nc)
        out[prefix + '/n_cells'] = np.array(nnps.n_cells)

    nnps.update()
    MG.check_nnps(nnps)
    ev = OptEval(a_eval, nnps)
    del CHANGES[:]
    ev.compute(t, dt)
    first = np.array(CHANGES)
    for pa in pas:
        for k, v in pa.properties.items():
            out['out/%s/%s' % (pa.name, k)] = np.array(v)
    nnps_out('nnps')
    tol = [eq.tol for g in groups for eq in g.equations if type(eq).__name__ == 'GradientCorrection']
    meta = dict(extra_meta or {})
    if tol and margin is not None:
        m = margins(tol[0])
        assert m['margin'] >= margin, (fname, m)
        if need_both:
            assert min(m['n_corrected'], m['n_pairs'] - m['n_corrected']) * 10 >= m['n_pairs'], (fname, m)
        meta.update(m)
    if second:
        nnps.update()
        MG.check_nnps(nnps)
        del CHANGES[:]
        ev.compute(t + dt, dt)
        for pa in pas:
            for k, v in pa.properties.items():
                out['out2/%s/%s' % (pa.name, k)] = np.array(v)
        nnps_out('nnps2')
        if tol and margin is not None:
            m = margins(tol[0])
            assert m['margin'] >= margin, (fname, 'second', m)
            meta.update(('second_' + k, v) for k, v in m.items())
    out['t'] = np.array(t)
    out['dt'] = np.array(dt)
    out['structure'] = np.array(json.dumps(structure(groups)))
    out['scheme'] = np.array(json.dumps(kw))
    out['overrides'] = np.array(json.dumps([list(o) for o in overrides]))
    out['kernel'] = np.array(type(kernel).__name__)
    for k, v in meta.items():
        out['meta/' + k] = np.array(v)
    path = os.path.join(HERE, fname)
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path) // 1024, 'KiB', meta)
    return first


def _garbage(props, rng, n, strided=True):
    for k in MG.WC_OUT:
        props[k] = rng.uniform(-1, 1, n)          # garbage: must be overwritten
    if strided:
        props['m_mat'] = rng.uniform(-1, 1, 9 * n)
        props['gradrho'] = rng.uniform(-1, 1, 3 * n)


def _cube(n1, seed, rho0=1000.0, varh=0.0, origin=(0.0, 0.0, 0.0), dx=None):
    rng = np.random.default_rng(seed)
    dx = 1.0 / n1 if dx is None else dx
    g = (np.arange(n1) + 0.5) * dx
    x, y, z = [a.ravel() for a in np.meshgrid(g, g, g, indexing='ij')]
    n = x.size
    props = dict(
        x=origin[0] + x + 0.2 * dx * rng.uniform(-1, 1, n), y=origin[1] + y + 0.2 * dx * rng.uniform(-1, 1, n),
        z=origin[2] + z + 0.2 * dx * rng.uniform(-1, 1, n),
        u=rng.uniform(-1, 1, n), v=rng.uniform(-1, 1, n), w=rng.uniform(-1, 1, n),
        h=1.2 * dx * (1 + varh * rng.uniform(-1, 1, n)),
        m=rho0 * dx ** 3 * np.ones(n), rho=rho0 * (1 + 0.05 * rng.uniform(-1, 1, n)))
    return props, n, dx, rng


DSPH3D_KW = dict(fluids=['fluid'], solids=[], dim=3, rho0=1000.0, c0=10.0, hdx=1.2, gx=0.5, gy=-0.25, gz=-9.81,
                 alpha=0.2, beta=0.0, gamma=7.0, delta=0.1, nu=0.01, delta_sph=True, update_h=True)


def case_dsph3d():
    """re-seeded until the reference alone meets the margin conditions, in both evaluations"""
    for seed in range(5, 40):
        props, n, dx, rng = _cube(6, seed)
        _garbage(props, rng, n)
        kw = dict(DSPH3D_KW, h0=1.2 * dx)
        try:
            first = run('opt_dsph3d.npz', [('fluid', props, n - 20)], kw, RK.WendlandQuintic(dim=3), second=True,
                        margin=1e-6, extra_meta=dict(dx=dx, seed=seed))
        except AssertionError as e:
            print('seed', seed, 'rejected:', e)
            continue
        # the gap case: the same particles, tol in the middle of the widest gap that leaves a tenth of the pairs on
        # either side
        ch = np.sort(first)
        lo, hi = ch.size // 10, ch.size - ch.size // 10
        gaps = ch[lo + 1:hi] - ch[lo:hi - 1]
        k = int(np.argmax(gaps))
        tol = float(0.5 * (ch[lo + k] + ch[lo + k + 1]))
        if 0.5 * gaps[k] < 5e-4:
            print('seed', seed, 'rejected: widest gap', gaps[k])
            continue
        props, n, dx, rng = _cube(6, seed)
        _garbage(props, rng, n)
        run('opt_dsph3d_gap.npz', [('fluid', props, n - 20)], kw, RK.WendlandQuintic(dim=3),
            overrides=[('GradientCorrection', 'tol', tol)], margin=5e-4, extra_meta=dict(dx=dx, seed=seed, tol=tol))
        return
    raise RuntimeError('no seed met the margin conditions')


def case_dsph2d_tank():
    for seed in range(60, 90):
        rng = np.random.default_rng(seed)
        dx = 1.0 / 16
        rho0 = 1000.0
        gx, gy = (np.arange(16) + 0.5) * dx, (np.arange(12) + 0.5) * dx
        x, y = [a.ravel() for a in np.meshgrid(gx, gy, indexing='ij')]
        n = x.size
        fluid = dict(x=x + 0.2 * dx * rng.uniform(-1, 1, n), y=y + 0.2 * dx * rng.uniform(-1, 1, n), z=np.zeros(n),
                     u=rng.uniform(-1, 1, n), v=rng.uniform(-1, 1, n), w=np.zeros(n),
                     h=1.3 * dx * (1 + 0.1 * rng.uniform(-1, 1, n)), m=rho0 * dx ** 2 * np.ones(n),
                     rho=rho0 * (1 + 0.05 * rng.uniform(-1, 1, n)))
        _garbage(fluid, rng, n)
        bx, by = (np.arange(-3, 19) + 0.5) * dx, (np.arange(-3, 0) + 0.5) * dx
        x, y = [a.ravel() for a in np.meshgrid(bx, by, indexing='ij')]
        nb = x.size
        wall = dict(x=x + 0.2 * dx * rng.uniform(-1, 1, nb), y=y + 0.2 * dx * rng.uniform(-1, 1, nb), z=np.zeros(nb),
                    u=np.zeros(nb), v=np.zeros(nb), w=np.zeros(nb),
                    h=1.3 * dx * (1 + 0.1 * rng.uniform(-1, 1, nb)), m=rho0 * dx ** 2 * np.ones(nb),
                    rho=rho0 * (1 + 0.05 * rng.uniform(-1, 1, nb)))      # (some below rho0: the HG correction acts)
        _garbage(wall, rng, nb)
        kw = dict(fluids=['fluid'], solids=['boundary'], dim=2, rho0=rho0, c0=10.0, h0=1.3 * dx, hdx=1.3, gy=-9.81,
                  alpha=0.3, beta=0.0, gamma=7.0, delta=0.1, nu=0.0, delta_sph=True, hg_correction=True)
        try:
            run('opt_dsph2d_tank.npz', [('fluid', fluid, n), ('boundary', wall, nb)], kw, RK.WendlandQuinticC4(dim=2),
                margin=1e-6, extra_meta=dict(dx=dx, seed=seed))
            return
        except AssertionError as e:
            print('seed', seed, 'rejected:', e)
    raise RuntimeError('no seed met the margin conditions')


def case_lamvisc3d():
    props, n, dx, rng = _cube(6, 91)
    _garbage(props, rng, n, strided=False)
    g = (np.arange(8) - 0.5) * dx
    x, y, z = [a.ravel() for a in np.meshgrid(g, g, (np.arange(-2, 0) + 0.5) * dx, indexing='ij')]
    ns = x.size
    solid = dict(x=x + 0.1 * dx * rng.uniform(-1, 1, ns), y=y + 0.1 * dx * rng.uniform(-1, 1, ns),
                 z=z + 0.1 * dx * rng.uniform(-1, 1, ns), u=rng.uniform(-1, 1, ns), v=rng.uniform(-1, 1, ns),
                 w=rng.uniform(-1, 1, ns), h=1.2 * dx * np.ones(ns), m=1000.0 * dx ** 3 * np.ones(ns),
                 rho=1000.0 * (1 + 0.05 * rng.uniform(-1, 1, ns)))
    _garbage(solid, rng, ns, strided=False)
    kw = dict(fluids=['fluid'], solids=['solid'], dim=3, rho0=1000.0, c0=10.0, h0=1.2 * dx, hdx=1.2, gz=-9.81,
              alpha=0.5, beta=1.0, gamma=7.0, nu=0.01, tensile_correction=True)
    run('opt_lamvisc3d.npz', [('fluid', props, n), ('solid', solid, ns)], kw, RK.CubicSpline(dim=3),
        extra_meta=dict(dx=dx))


def case_singular():
    """a 4^3 block, and far from it (and from each other): one particle alone, two particles, three on a line"""
    for seed in range(120, 150):
        dx = 0.25
        props, n, dx, rng = _cube(4, seed, dx=dx)
        far = np.array([[3.0, 0.3, 0.2],                                        # alone
                        [0.2, 3.0, 0.4], [0.2 + 0.8 * dx, 3.0 + 0.5 * dx, 0.4 + 0.3 * dx],     # a pair
                        [3.0, 3.0, 0.1], [3.0 + 0.6 * dx, 3.0 + 0.7 * dx, 0.1 + 0.2 * dx],
                        [3.0 + 1.2 * dx, 3.0 + 1.4 * dx, 0.1 + 0.4 * dx]])                  # three on a line
        k = len(far)
        for j, c in enumerate('xyz'):
            props[c] = np.concatenate([props[c], far[:, j]])
        for c in 'uvw':
            props[c] = np.concatenate([props[c], rng.uniform(-1, 1, k)])
        props['h'] = np.concatenate([props['h'], 1.2 * dx * np.ones(k)])
        props['m'] = np.concatenate([props['m'], props['m'][:k]])
        props['rho'] = np.concatenate([props['rho'], 1000.0 * (1 + 0.05 * rng.uniform(-1, 1, k))])
        n += k
        _garbage(props, rng, n)
        kw = dict(fluids=['fluid'], solids=[], dim=3, rho0=1000.0, c0=10.0, h0=1.2 * dx, hdx=1.2, gz=-9.81,
                  alpha=0.2, beta=0.0, gamma=7.0, delta=0.1, nu=0.0, delta_sph=True)
        try:
            run('opt_singular.npz', [('fluid', props, n)], kw, RK.QuinticSpline(dim=3),
                overrides=[('GradientCorrection', 'dim', 3)], margin=1e-6, need_both=False,
                extra_meta=dict(dx=dx, seed=seed, n_degenerate=k))
            return
        except AssertionError as e:
            print('seed', seed, 'rejected:', e)
    raise RuntimeError('no seed met the margin conditions')


if __name__ == '__main__':
    which = sys.argv[1:] or ['dsph3d', 'dsph2d_tank', 'lamvisc3d', 'singular']
    for name in which:
        globals()['case_' + name]()
