#!/usr/bin/env python
"""Golden vectors for the six smoothing kernels beyond the first four
(WendlandQuinticC2_1D, WendlandQuinticC4, WendlandQuinticC4_1D,
WendlandQuinticC6, WendlandQuinticC6_1D, SuperGaussian), from the REFERENCE's
own Python classes, in the manner of make_golden.py (same driver, same stored
layout):

    python tests/golden/make_more_kernels_golden.py

The C oracle knows four kernels, so these files are what the new kernels are
judged against.  Every random draw is seeded; every lattice is jittered by
0.1 - 0.2 dx so that force sums do not cancel and a relative tolerance means
something.

    kernels_more.npz               the layout of kernels.npz (+ gradh) per (class, dim)
    more_wcsph_c4_varh.npz         WCSPH 3-D, 8^3, WendlandQuinticC4, h +-15 %
    more_wcsph_c6.npz              WCSPH 3-D, 8^3, WendlandQuinticC6, one h
    more_tvf2d_sg.npz / _varh      TVF 2-D, 24 x 24, SuperGaussian, one h / h +-15 %
    more_sd1d_<class>.npz          summation density on an irregular line of 130, h +-15 %
    more_elastic2d_c6.npz          make_golden's elastic 2-D block with WendlandQuinticC6
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402  (sets up the reference imports)

from pysph.sph.scheme import WCSPHScheme, TVFScheme  # noqa: E402
from pysph.sph.equation import Group  # noqa: E402
from pysph.sph.basic_equations import SummationDensity  # noqa: E402
from pysph.base import kernels as RK  # noqa: E402

MORE = (('WendlandQuinticC2_1D', (1,)), ('WendlandQuinticC4', (2, 3)),
        ('WendlandQuinticC4_1D', (1,)), ('WendlandQuinticC6', (2, 3)),
        ('WendlandQuinticC6_1D', (1,)), ('SuperGaussian', (1, 2, 3)))


def case_kernels_more():
    out = {}
    rng = np.random.default_rng(31)
    for name, dims in MORE:
        for dim in dims:
            k = getattr(RK, name)(dim=dim)
            h = 0.5 + rng.uniform(0, 1, 64)
            q = np.concatenate([[0.0, 1e-13, 1.0, 2.0, 3.0], rng.uniform(0, 3.5, 59)])
            r = q * h
            r[1] = 1e-13                      # r itself, below the gradient's guard
            xij = rng.uniform(-1, 1, (64, 3))
            gr = []
            for i in range(64):
                g = [0.0, 0.0, 0.0]
                k.gradient(list(xij[i]), r[i], h[i], g)
                gr.append(g)
            key = '%s/%d/' % (name, dim)
            out[key + 'h'] = h
            out[key + 'r'] = r
            out[key + 'xij'] = xij
            out[key + 'w'] = np.array([k.kernel(list(xij[i]), r[i], h[i]) for i in range(64)])
            out[key + 'dwdq'] = np.array([k.dwdq(r[i], h[i]) for i in range(64)])
            out[key + 'grad'] = np.array(gr)
            out[key + 'gradh'] = np.array([k.gradient_h(list(xij[i]), r[i], h[i]) for i in range(64)])
            out[key + 'fac'] = np.array(k.fac)
            out[key + 'deltap'] = np.array(k.get_deltap())
            out[key + 'radius_scale'] = np.array(k.radius_scale)
    path = os.path.join(HERE, 'kernels_more.npz')
    np.savez_compressed(path, **out)
    print('wrote', path)


def _wcsph_cube(fname, kernel, varh, seed):
    """the particles and equation set of make_golden.case_wcsph_cube_varh (tensile correction: WDP / deltap)"""
    rng = np.random.default_rng(seed)
    n1 = 8
    dx = 1.0 / n1
    g = (np.arange(n1) + 0.5) * dx
    x, y, z = [a.ravel() for a in np.meshgrid(g, g, g, indexing='ij')]
    n = x.size
    rho0, c0 = 1000.0, 10.0
    props = dict(
        x=x + 0.2 * dx * rng.uniform(-1, 1, n), y=y + 0.2 * dx * rng.uniform(-1, 1, n),
        z=z + 0.2 * dx * rng.uniform(-1, 1, n),
        u=rng.uniform(-1, 1, n), v=rng.uniform(-1, 1, n), w=rng.uniform(-1, 1, n),
        h=1.2 * dx * (1 + varh * rng.uniform(-1, 1, n)),
        m=rho0 * dx ** 3 * np.ones(n), rho=rho0 * (1 + 0.05 * rng.uniform(-1, 1, n)))
    for k in MG.WC_OUT:
        props[k] = rng.uniform(-1, 1, n)
    s = WCSPHScheme(['fluid'], [], dim=3, rho0=rho0, c0=c0, h0=1.2 * dx, hdx=1.2, gx=0.5, gy=-0.25, gz=-9.81,
                    alpha=1.0, beta=1.0, gamma=7.0, tensile_correction=True, summation_density=True)
    MG.run_case(fname, [('fluid', props, n)], s.get_equations(), kernel, 3, store_nbrs=[('fluid', 'fluid')], meta=dict(dx=dx))


def _tvf_2d(fname, varh, seed):
    rng = np.random.default_rng(seed)
    n1 = 24
    dx = 1.0 / n1
    g = (np.arange(n1) + 0.5) * dx
    x, y = [a.ravel() for a in np.meshgrid(g, g, indexing='ij')]
    n = x.size
    rho0, c0 = 1.0, 10.0
    props = dict(
        x=x + 0.15 * dx * rng.uniform(-1, 1, n), y=y + 0.15 * dx * rng.uniform(-1, 1, n), z=np.zeros(n),
        u=rng.uniform(-1, 1, n), v=rng.uniform(-1, 1, n), w=np.zeros(n),
        uhat=rng.uniform(-1, 1, n), vhat=rng.uniform(-1, 1, n), what=np.zeros(n),
        h=dx * (1 + varh * rng.uniform(-1, 1, n)), m=rho0 * dx ** 2 * np.ones(n),
        rho=rho0 * (1 + 0.05 * rng.uniform(-1, 1, n)))
    for k in ['p', 'V', 'au', 'av', 'aw', 'auhat', 'avhat', 'awhat']:
        props[k] = rng.uniform(0.5, 1, n)
    s = TVFScheme(['fluid'], [], dim=2, rho0=rho0, c0=c0, nu=0.01, p0=c0 * c0 * rho0, pb=c0 * c0 * rho0, h0=dx,
                  gx=0.1, alpha=0.2)
    MG.run_case(fname, [('fluid', props, n)], s.get_equations(), RK.SuperGaussian(dim=2), 2, t=0.01,
                store_nbrs=[('fluid', 'fluid')], meta=dict(dx=dx))


def _sd_1d(name, seed):
    rng = np.random.default_rng(seed)
    n = 130                                   # more than two wavefronts
    dx = 1.0 / n
    x = (np.arange(n) + 0.5) * dx + 0.2 * dx * rng.uniform(-1, 1, n)
    z = np.zeros(n)
    props = dict(x=x, y=z.copy(), z=z.copy(), h=1.3 * dx * (1 + 0.15 * rng.uniform(-1, 1, n)),
                 m=dx * (1 + 0.1 * rng.uniform(-1, 1, n)), rho=z.copy())
    eqs = [Group(equations=[SummationDensity(dest='fluid', sources=['fluid'])])]
    MG.run_case('more_sd1d_%s.npz' % name, [('fluid', props, n)], eqs, getattr(RK, name)(dim=1), 1,
                store_nbrs=[('fluid', 'fluid')])


def case_elastic_2d_c6():
    """make_golden._elastic_case builds its kernel as CubicSpline(dim=dim): hand it the Wendland C6 under that name"""
    saved = MG.CubicSpline
    MG.CubicSpline = RK.WendlandQuinticC6
    try:
        MG._elastic_case('more_elastic2d_c6.npz', 2, 14, 15)
    finally:
        MG.CubicSpline = saved


if __name__ == '__main__':
    case_kernels_more()
    _wcsph_cube('more_wcsph_c4_varh.npz', RK.WendlandQuinticC4(dim=3), 0.15, 41)
    _wcsph_cube('more_wcsph_c6.npz', RK.WendlandQuinticC6(dim=3), 0.0, 42)
    _tvf_2d('more_tvf2d_sg.npz', 0.0, 43)
    _tvf_2d('more_tvf2d_sg_varh.npz', 0.15, 44)
    for i, name in enumerate(('WendlandQuinticC2_1D', 'WendlandQuinticC4_1D', 'WendlandQuinticC6_1D',
                              'SuperGaussian')):
        _sd_1d(name, 50 + i)
    case_elastic_2d_c6()
