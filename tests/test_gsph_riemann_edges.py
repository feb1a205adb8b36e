"""The GSPH Riemann solvers and the state reconstruction of the force sweep (``FamGSPH_T``, pysph_amd/csrc/sph_fam_gas.h), one
pair at a time, against the reference's own solver text evaluated at 50 digits (tests/golden/gsph_riemann_edges.npz, made
by tests/golden/make_gsph_riemann_golden.py; the tests read nothing but that file).

Every table is a 1-D row of isolated pairs, 2^-3 apart, one launch per solver.  pstar and ustar of each ordered pair are
decoded from the au and ae the sweep wrote (helpers.gsph_decode, calibrated by a launch of the same table under the
non-diffusive solver) and measured in units of u S, u = 2^-53, S_p = max(pl, pr, |pstar|), S_u = max(|ul|, |ur|, cl, cr,
|ustar|).  With K_ref the reference's own double result in that measure, a case with K_ref <= 64 is well-conditioned;
K_solver is the largest K_ref over the well-conditioned cases of a solver, and the device is held to max(4, 4 K_solver) on
each of them (the rule of tests/test_nosrc_edges.py) and to 4 K_ref of the case itself on the others (pstar and ustar
each to its own), plus the decoding cost (helpers.GSPH_DECODE_COST).  A case in which the 50-digit run took another path
than the double run is not compared numerically.  Return codes, the failure word, the zeros a failed pair leaves and the
NaN pattern of the two columns are compared exactly.

Measured on an MI355X: DESIGN.md, section 7h."""
import importlib.util
import json
import os

import numpy as np
import pytest

from conftest import load_golden
from helpers import GSPH_DECODE_COST, gsph_decode

U53 = 2.0 ** -53
U24 = 2.0 ** -24
WELL = 64.0
SOLVERS = ('non_diffusive', 'van_leer', 'exact', 'hllc', 'ducowicz', 'hlle', 'roe', 'llxf', 'hllc_ball', 'hll_ball', 'hllsy')
ITERATIVE = ('van_leer', 'exact')
COLS = ('x', 'u', 'rho', 'p', 'cs', 'm', 'h', 'e', 'grhox', 'px', 'ux')
FORCE_OUT = ('au', 'av', 'aw', 'ae')
GUESSES = ('exact_guess_pv', 'exact_guess_tr', 'exact_guess_ts')
REQUIRED = tuple('%s/%s' % (g, s) for g in GUESSES for s in ('left_rarefaction', 'left_shock', 'right_rarefaction', 'right_shock')) + (
    'ducowicz_a', 'ducowicz_b', 'ducowicz_c', 'ducowicz_d', 'hllc_left_star', 'hllc_right_star',
    'hllc_ball_hl_above', 'hllc_ball_hl_below', 'hllc_ball_hr_above', 'hllc_ball_hr_below',
    'van_leer_smallp', 'van_leer_no_smallp', 'hlle_sl_first', 'hlle_sl_second', 'hlle_sr_first', 'hlle_sr_second')
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

_G = []


def fixture():
    if not _G:
        _G.append(load_golden('gsph_riemann_edges.npz'))
    return _G[0]


def params_of(g, key):
    return json.loads(str(g[key + '/params']))


def runs_of(g, key):
    return [tuple(r) for r in json.loads(str(g[key + '/runs']))]


def tables_of(g, prefixes, name):
    """the tables under these prefixes that hold a run of this solver (partial/: the states another solver raises on)"""
    return [key for key in json.loads(str(g['tables'])) if key.split('/')[0] in prefixes and name in [r[0] for r in runs_of(g, key)]]


def k_solver(g):
    return json.loads(str(g['meta/k_solver']))


def scales(args, gamma, pstar, ustar):
    rhol, rhor, pl, pr, ul, ur = args.T
    with np.errstate(invalid='ignore', divide='ignore'):
        cl, cr = np.sqrt(gamma * pl / rhol), np.sqrt(gamma * pr / rhor)
        cl, cr = np.where(np.isnan(cl), 0.0, cl), np.where(np.isnan(cr), 0.0, cr)      # (no sound speed where p / rho < 0)
        sp = np.maximum(np.maximum(pl, pr), np.abs(pstar))
        su = np.max([np.abs(ul), np.abs(ur), cl, cr, np.abs(ustar)], axis=0)
    return sp, su


def measure(got_p, got_u, mpv, args, gamma, unit):
    """the distance of decoded values from the stored 50-digit ones (a double and its remainder) in units of unit * S"""
    sp, su = scales(args, gamma, mpv[:, 0], mpv[:, 2])
    with np.errstate(invalid='ignore', divide='ignore'):
        kp = np.abs((got_p - mpv[:, 0]) - mpv[:, 1]) / (unit * sp)
        ku = np.abs((got_u - mpv[:, 2]) - mpv[:, 3]) / (unit * su)
    return kp, ku


def bounds(g, key, rname, name):
    """per row (pstar, ustar): max(4, 4 K_solver) where the reference itself is within 64 in both values, else four times
    the reference's own figure for that value.  Returns (bound of pstar, bound of ustar, well-conditioned)"""
    kref = np.where(np.isnan(g['%s/%s/kref' % (key, rname)]), 0.0, g['%s/%s/kref' % (key, rname)])
    well = kref.max(axis=1) <= WELL
    flat = max(4.0, 4.0 * k_solver(g)[name])
    return np.where(well, flat, 4.0 * kref[:, 0]), np.where(well, flat, 4.0 * kref[:, 1]), well


# ---------------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------------
def test_golden_generator_imports_cleanly():
    if not os.path.isdir('/root/reference'):
        pytest.skip('the generator needs the reference (build container only)')
    spec = importlib.util.spec_from_file_location('make_gsph_riemann_golden', os.path.join(GOLDEN, 'make_gsph_riemann_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert callable(mod.main) and mod.OUT.endswith('gsph_riemann_edges.npz')
    assert mod.REQUIRED == REQUIRED and (mod.DECODE_P, mod.DECODE_U) == GSPH_DECODE_COST


def test_the_conditions_asserted_on_the_reference_are_in_the_file():
    """every required branch at least twice over the main tables; per solver at most one case in ten not well-conditioned
    (K_ref > 64 or another path at 50 digits); K_solver as stored; gamma (1 + 1e-13) seen by every solver; the file small"""
    g = fixture()
    assert os.path.getsize(os.path.join(GOLDEN, 'gsph_riemann_edges.npz')) < 1024 * 1024
    branches = json.loads(str(g['meta/branches']))
    assert tuple(json.loads(str(g['meta/required']))) == REQUIRED
    short = dict((b, branches.get(b, 0)) for b in REQUIRED if branches.get(b, 0) < 2)
    assert not short, short
    ks = k_solver(g)
    for k, name in enumerate(SOLVERS):
        bad = total = 0
        best = 0.0
        assert tables_of(g, ('main',), name) == ['main/g14', 'main/g53']
        for key in tables_of(g, ('main', 'partial'), name):
            assert (name, k, 20) in runs_of(g, key)
            pair = g[key + '/d'] != g[key + '/s']
            kref, mpok = g['%s/%s/kref' % (key, name)][pair], g['%s/%s/mpok' % (key, name)][pair]
            assert np.all(g['%s/%s/ret' % (key, name)] == g['%s/%s/counted' % (key, name)])
            worst = np.nanmax(np.where(np.isnan(kref), np.inf, kref), axis=1)
            well = mpok & (worst <= WELL)
            bad += int(np.sum(~well))
            total += well.size
            best = max(best, float(np.max(worst[well], initial=0.0)))
        assert bad * 10 <= total, (name, bad, total)
        assert best == ks[name] and best <= WELL, (name, best, ks[name])
    seen = json.loads(str(g['meta/gamma_sensitive_cases']))
    assert all(seen.get(name, 0) >= 1 for name in SOLVERS[1:]), seen
    assert tuple(g['meta/decode_cost']) == GSPH_DECODE_COST
    dropped = json.loads(str(g['meta/dropped']))
    assert all(d['error'] in ('ZeroDivisionError', 'TypeError', 'OverflowError') for d in dropped)
    # the density ratio 1e6 with the pressure ratio 1e8 is there for every solver the reference does not raise on
    for key in tables_of(g, ('partial',), 'hll_ball'):
        assert np.any((g[key + '/args'][:, 0] == 1e6) & (g[key + '/args'][:, 2] == 1e8))
        assert set(SOLVERS) - set(r[0] for r in runs_of(g, key)) == set(d['solver'] for d in dropped if d['table'] == 'main/' + key[-3:])
    # the rows the fp32 comparison leaves out for want of bits are ducowicz's at the density ratio 1e6 and no others
    for key in json.loads(str(g['tables'])):
        if key.split('/')[0] in ('f32', 'f32partial'):
            for name, k, niter in runs_of(g, key):
                out = ~g['%s/%s/f32bits' % (key, name)] & g['%s/%s/mpok' % (key, name)]
                if out.any():
                    dense = np.any(g[key + '/args'][out, :2] == 1e6, axis=1)         # (its self pair included)
                    assert name == 'ducowicz' and key.startswith('f32partial/') and np.all(dense), (key, name)
    # both orientations: the two ordered pairs of a pair are different problems somewhere, and the table holds each state twice
    a = g['main/g14/args']
    assert a.shape[0] % 8 == 0 and not np.array_equal(a[1], a[2])


def test_the_edge_tables_hold_the_edges():
    """the vacuum test from both sides, a converged solve at every last allowed iteration, van_leer's two exits, the NaN
    wave speeds, each fallback and each return of the limiter -- as the reference took them"""
    g = fixture()
    sigs = json.loads(str(g['sigs']))
    for key in ('vacuum/g14', 'vacuum/g53'):
        ret, sig = g[key + '/exact/ret'], [sigs[k] for k in g[key + '/exact/sig']]
        pair = g[key + '/d'] != g[key + '/s']
        assert np.sum(ret[pair] == 1) >= 2 and np.sum(ret[pair] == 0) >= 2
        assert all(('exact_vacuum' in s) == bool(r) for s, r in zip(sig, ret))
        assert np.all(g[key + '/exact/mpok'][ret == 0][pair[ret == 0]])
    stops = [int(k) for k in g['lastiter/stops']]
    assert set((1, 3, 5)) <= set(stops)
    for k in stops:
        at, after = 'lastiter/exact_niter%d/' % (k + 1), 'lastiter/exact_niter%d/' % (k + 2)
        hit = (g[after + 'loop'] == k) & (g[after + 'ret'] == 0)
        assert hit.sum() >= 2, k
        assert np.all(g[at + 'ret'][hit] == 1) and np.all(g[at + 'loop'][hit] == k)       # converged, and refused
        assert np.all(g[at + 'ref'][hit] == 0.0) and np.all(g[at + 'counted'][hit] == 1)
    ret20, ret1 = g['van_leer/van_leer_niter20/ret'], g['van_leer/van_leer_niter1/ret']
    cnt1, ref1 = g['van_leer/van_leer_niter1/counted'], g['van_leer/van_leer_niter1/ref']
    neg = np.any(g['van_leer/args'][:, 2:4] < 0, axis=1)
    assert neg.sum() >= 4 and np.all(ret20[neg] == 1) and np.all(ret20[~neg] == 0)
    assert np.all(cnt1 == neg) and np.sum((ret1 == 1) & ~neg) >= 4 and np.all(ref1[(ret1 == 1) & ~neg, 0] > 0)
    ret = g['hllc_nan/hllc/ret']
    args = g['hllc_nan/args']
    bad = np.isnan(args[:, 2:4]).any(axis=1) | (args[:, 2:4] < 0).any(axis=1)
    assert np.array_equal(ret == 1, bad) and np.isnan(args[:, 2:4]).any() and (args[:, 2:4] < 0).any()
    # python's max on a NaN: ducowicz returns the NaN of max(pstar, 0.0) (fmax would return 0) on a pair it does not fail
    duc = g['minmax_nan/ducowicz/ref']
    pair = g['minmax_nan/d'] != g['minmax_nan/s']
    assert np.all(g['minmax_nan/ducowicz/ret'] == 0) and np.isnan(duc[pair, 0]).all() and np.all(np.isfinite(g['minmax_nan/args']))
    assert np.isnan(g['minmax_nan/ducowicz/au']).all()
    lx = g['minmax_nan/llxf/au']                           # llxf's max(csr, csl): a NaN csl is passed over, a NaN csr stands
    assert np.isnan(lx).sum() == lx.size // 2 and np.isfinite(lx).sum() == lx.size // 2
    # the four fallbacks, each taken, each on a pair of unequal particles: the argument equals the particle's own value and
    # differs from the partner's
    a1, d1, s1 = g['recon/mono1/args'], g['recon/mono1/d'], g['recon/mono1/s']
    assert np.all(a1[:, :4] >= 0) and np.sum(a1[:, 2] == 0) >= 2 and np.sum(a1[:, 3] == 0) >= 2
    lines = json.loads(str(g['recon/mono1/gs_lines']))
    assert lines['mono1_sign'] >= 2 and lines['mono1_shock'] >= 2
    x, e1 = g['recon/mono1/in/x'], None
    e1 = np.sign(x[d1] - x[s1])
    taken = {}
    for what, col, grad, arg, own, other, sgn in (('fallback_rhol', 'rho', 'grhox', 0, s1, d1, 1.0), ('fallback_rhor', 'rho', 'grhox', 1, d1, s1, -1.0),
                                                  ('fallback_pl', 'p', 'px', 2, s1, d1, 1.0), ('fallback_pr', 'p', 'px', 3, d1, s1, -1.0)):
        v, gr = g['recon/mono1/in/' + col], g['recon/mono1/in/' + grad]
        raw = v[own] + sgn * 0.5 * (gr[own] * e1) * 0.125            # dt = 0, sstar = 0, no switch in these rows
        fell = (raw < 0) & (d1 != s1)
        taken[what] = int(fell.sum())
        assert fell.sum() >= 2 and lines[what] == fell.sum(), (what, lines[what], int(fell.sum()))
        assert np.all(a1[fell, arg] == v[own][fell]) and np.all(v[own][fell] != v[other][fell]), what
        assert np.all(a1[(raw == 0) & (d1 != s1), arg] == 0)             # exactly 0 is no fallback
    print('fallbacks taken on unequal particles:', taken)
    lines = json.loads(str(g['recon/mono2/gs_lines']))
    assert min(lines['min_zero'], lines['min_x1'], lines['min_x2'], lines['min_x3_a'] + lines['min_x3_b']) >= 6, lines
    assert params_of(g, 'recon/dt')['dt'] * 3.0 * 8.0 > 1.0


@pytest.mark.parametrize('key', ['main/g14', 'main/g53'])
def test_decoding_recovers_the_reference_from_its_own_columns(key):
    """helpers.gsph_decode on the au and ae the REFERENCE wrote, calibrated by its non-diffusive run, gives back the pstar
    and ustar its solver returned within the stated cost, for every solver and every pair of the table"""
    g = fixture()
    x = g[key + '/in/x']
    d, s, args = g[key + '/d'], g[key + '/s'], g[key + '/args']
    pair = d != s
    assert np.array_equal(d[pair], np.arange(x.size)) and np.array_equal(s[pair], np.arange(x.size) ^ 1)
    p_cal = 0.5 * (args[pair, 2] + args[pair, 3])
    assert np.array_equal(p_cal, g[key + '/non_diffusive/ref'][pair, 0]) and np.all(p_cal != 0)
    worst = [0.0, 0.0]
    for name in SOLVERS[1:]:
        ref = g['%s/%s/ref' % (key, name)][pair]
        ps, us = gsph_decode(x, g['%s/%s/au' % (key, name)], g['%s/%s/ae' % (key, name)], g[key + '/non_diffusive/au'], p_cal)
        ok = ref[:, 0] != 0
        kp = np.abs(ps - ref[:, 0])[ok] / (U53 * np.abs(ref[:, 0][ok]))
        uok = ok & (ref[:, 1] != 0)
        ku = np.abs(us - ref[:, 1])[uok] / (U53 * np.abs(ref[:, 1][uok]))
        assert np.all(ps[~ok] == 0) and np.all(us[ok & (ref[:, 1] == 0)] == 0)
        worst = [max(worst[0], kp.max()), max(worst[1], ku.max())]
        assert kp.max() <= GSPH_DECODE_COST[0] and ku.max() <= GSPH_DECODE_COST[1], (name, kp.max(), ku.max())
    print('%s: decoding the reference costs %.2f u in pstar, %.2f u in ustar' % (key, worst[0], worst[1]))


# ---------------------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------------------
H_VARIABLE = (0.15, 0.1875)
_CAL = {}


def table_array(g, key, variable_h=False):
    from pysph_amd.gas_dynamics import GSPHScheme
    from pysph_amd.particle_array import get_particle_array_gasd
    cols = dict((c, g['%s/in/%s' % (key, c)].copy()) for c in COLS)
    n = cols['x'].size
    if variable_h:
        cols['h'] = np.where(np.arange(n) % 2 == 0, H_VARIABLE[0], H_VARIABLE[1])
    pa = get_particle_array_gasd(name='fluid', **dict((c, cols[c]) for c in ('x', 'u', 'rho', 'p', 'cs', 'm', 'h', 'e')))
    GSPHScheme(['fluid'], [], dim=1, gamma=1.4, kernel_factor=1.2).setup_properties([pa])
    for c in ('grhox', 'px', 'ux'):
        pa.properties[c][:] = cols[c]
    for c in FORCE_OUT:
        pa.properties[c][:] = 7.0              # must be overwritten
    return pa


def launch(g, key, rsolver, niter, variant=6, variable_h=False, f32=False):
    """GSPHAcceleration alone over the table: (au, ae, failure word); every input column must come back unchanged"""
    from pysph_amd import kernels as K
    import test_gsph_gpu as TG
    P = params_of(g, key)
    pa = table_array(g, key, variable_h)
    before = dict((c, pa.properties[c].copy()) for c in TG._floats(pa))
    groups = TG._force_group(dict(rsolver=rsolver, niter=niter, gamma=P['gamma'], tol=P['tol'], monotonicity=P['monotonicity'],
                                  interpolation=0, g1=0.0, g2=0.0))
    a_eval, nnps, ctx = TG.evaluator([pa], groups, K.CubicSpline(dim=1), variant, f32)
    nnps.update()
    a_eval.compute(0.0, P['dt'])
    fails = TG.failures(groups)
    TG.pull_all([pa])
    ctx.close()
    for c, v in before.items():
        if c not in FORCE_OUT:
            assert np.array_equal(pa.properties[c], v, equal_nan=True), (key, c)
    for col in (pa.av, pa.aw):                 # 1-D: nothing but zeros, or pstar 0 = NaN where pstar is a NaN (then au is one too)
        assert np.all((col == 0.0) | np.isnan(pa.au)), key
    return pa.au.copy(), pa.ae.copy(), fails


def calibration(g, key, variant, variable_h, f32):
    ck = (key, variant, variable_h, f32)
    if ck not in _CAL:
        au, ae, fails = launch(g, key, 0, 20, variant, variable_h, f32)
        assert fails == 0
        _CAL[ck] = au
    return _CAL[ck]


def check_run(g, key, rname, rsolver, niter, variant=6, variable_h=False, f32=False):
    """one launch of one solver over one table against the file: the failure word, the zeros of the failed pairs, and
    pstar and ustar of every comparable ordered pair within the bound.  Returns the measured maxima (pstar, ustar)."""
    name = SOLVERS[rsolver]
    pre = '%s/%s/' % (key, rname)
    gamma = params_of(g, key)['gamma']
    x, d, s, args = g[key + '/in/x'], g[key + '/d'], g[key + '/s'], g[key + '/args']
    pair = d != s
    au, ae, fails = launch(g, key, rsolver, niter, variant, variable_h, f32)
    counted, ret = g[pre + 'counted'], g[pre + 'ret']
    assert fails == int(counted.sum()), (key, rname, fails, int(counted.sum()))
    # a destination whose pair failed got nothing; whatever is finite in the reference's columns is finite here
    ref_au, ref_ae = g[pre + 'au'], g[pre + 'ae']
    failed = (counted[pair] == 1) & (ref_au == 0) & (ref_ae == 0)
    assert np.all(au[failed] == 0.0) and np.all(ae[failed] == 0.0), (key, rname)
    assert np.all(np.isfinite(au[np.isfinite(ref_au)])) and np.all(np.isfinite(ae[np.isfinite(ref_ae)])), (key, rname)
    # ... and a NaN the reference carries into a column is one here: min and max take Python's way on a NaN
    assert np.array_equal(np.isnan(au), np.isnan(ref_au)) and np.array_equal(np.isnan(ae), np.isnan(ref_ae)), (key, rname)
    if rsolver == 0:
        return 0.0, 0.0
    with np.errstate(invalid='ignore'):
        if f32:
            p_cal = ((args[pair, 2].astype(np.float32) + args[pair, 3].astype(np.float32)) * np.float32(0.5)).astype(np.float64)
        else:
            p_cal = 0.5 * (args[pair, 2] + args[pair, 3])
    ok = g[pre + ('f32ok' if f32 else 'mpok')][pair] & (counted[pair] == 0)     # (van_leer's unconverged exit has a result)
    assert np.all(p_cal[ok] != 0)
    ps, us = gsph_decode(x, au, ae, calibration(g, key, variant, variable_h, f32), p_cal)
    mpv = g[pre + 'mp'][pair]
    unit = U24 if f32 else U53
    kp, ku = measure(ps, us, mpv, args[pair], gamma, unit)
    if f32 and name in ITERATIVE:
        # the stop test compares a relative change with tol = 1e-6, which fp32 resolves only to 2^-24 = 6e-8: a solve may
        # stop an iteration earlier or later than at 50 digits, and then differs by up to the change tol allows
        bound_p = bound_u = np.full(ok.size, 4.0 * params_of(g, key)['tol'] / unit)
    else:
        bound_p, bound_u = [b[pair] for b in bounds(g, key, rname, name)[:2]]
    u_ok = ok & ~((mpv[:, 0] == 0) & (au == 0))          # pstar = 0 exactly: au = 0 carries no ustar
    flat = max(4.0, 4.0 * k_solver(g)[name])
    well = bounds(g, key, rname, name)[2][pair]
    worst_p, worst_u = float(np.max(kp[ok & well], initial=0.0)), float(np.max(ku[u_ok & well], initial=0.0))
    with np.errstate(invalid='ignore', divide='ignore'):
        ill = float(np.max(np.maximum(kp / (bound_p + GSPH_DECODE_COST[0]), np.where(u_ok, ku / (bound_u + GSPH_DECODE_COST[1]), 0.0))[ok & ~well],
                           initial=0.0))
    print('%s %s variant %d%s%s: K measured pstar %.3f ustar %.3f over %d well-conditioned pairs (bound %.1f); the %d others '
          'at most %.3f of their own bound' % (key, rname, variant, ' variable h' if variable_h else '', ' fp32' if f32 else '',
                                               worst_p, worst_u, int((ok & well).sum()), flat, int((ok & ~well).sum()), ill))
    where = np.nonzero(ok & ~(kp <= bound_p + GSPH_DECODE_COST[0]))[0]
    assert where.size == 0, (key, rname, 'pstar', [(int(i), float(kp[i]), float(bound_p[i]), args[pair][i].tolist()) for i in where[:4]])
    where = np.nonzero(u_ok & ~(ku <= bound_u + GSPH_DECODE_COST[1]))[0]
    assert where.size == 0, (key, rname, 'ustar', [(int(i), float(ku[i]), float(bound_u[i]), args[pair][i].tolist()) for i in where[:4]])
    return worst_p, worst_u


@pytest.mark.gpu
@pytest.mark.parametrize('variant', [6, 0])
@pytest.mark.parametrize('rsolver', range(11))
def test_every_pair_of_the_state_table_fp64(rsolver, variant):
    """uniform h, both schedules, gamma 1.4 and 5/3: decoded pstar and ustar of every ordered pair within the bound, the
    failure word equal to the reference's returns of 1 (self pairs included), zeros where a pair failed, inputs unchanged"""
    g = fixture()
    for key in tables_of(g, ('main', 'partial'), SOLVERS[rsolver]):
        check_run(g, key, SOLVERS[rsolver], rsolver, 20, variant)


@pytest.mark.gpu
@pytest.mark.parametrize('rsolver', range(11))
def test_every_pair_of_the_state_table_variable_h(rsolver):
    """the two particles of a pair at h = 0.15 and 0.1875: the instantiation that reads h from the records; same bounds"""
    g = fixture()
    for key in tables_of(g, ('main', 'partial'), SOLVERS[rsolver]):
        check_run(g, key, SOLVERS[rsolver], rsolver, 20, variable_h=True)


@pytest.mark.gpu
@pytest.mark.parametrize('rsolver', range(11))
def test_every_pair_of_the_state_table_fp32(rsolver):
    """arith_f32 on the states whose inputs and results lie in [2^-40, 2^40], truth at 50 digits on the inputs rounded to
    float32.  A straight-line formula grows by the same number of units of u in either precision, so the non-iterative
    solvers are held to their fp64 bound in units of 2^-24; exact and van_leer stop on a relative change below tol and
    are held to 4 tol S.  First-order growth needs K 2^-24 well below one: the generator leaves a row out of ``f32ok``
    where the reference's own K says fp32 keeps fewer than three bits (ducowicz at the density ratio 1e6, K_ref = 9e7;
    the fp32 sweep returns 1e4 S there, 512 times the bound that row would have had)."""
    g = fixture()
    assert sum(g['%s/%s/f32ok' % (key, SOLVERS[rsolver])].sum() for key in ('f32/g14', 'f32/g53')) >= 80
    for key in tables_of(g, ('f32', 'f32partial'), SOLVERS[rsolver]):
        check_run(g, key, SOLVERS[rsolver], rsolver, 20, f32=True)


@pytest.mark.gpu
@pytest.mark.parametrize('key', ['vacuum/g14', 'vacuum/g53'])
def test_exact_either_side_of_the_vacuum_test(key):
    """gamma4 (cl + cr) against ur - ul a relative 1e-9 apart: counted and zero on one side, solved on the other"""
    check_run(fixture(), key, 'exact', 2, 20)


@pytest.mark.gpu
def test_exact_refuses_a_solve_that_converged_in_the_last_allowed_iteration():
    """a state that stops at loop index k: with niter = k + 1 the reference returns 1 although the solve converged, and
    so must the sweep; with niter = k + 2 it is solved and not counted (k = 1 .. 6, every niter one launch)"""
    g = fixture()
    for rname, rsolver, niter in runs_of(g, 'lastiter'):
        check_run(g, 'lastiter', rname, rsolver, niter)


@pytest.mark.gpu
def test_van_leer_negative_pressure_and_a_single_iteration():
    """a negative pl or pr counts and leaves zeros; niter = 1 on states that need more writes the result of the one
    iteration, equal to the reference's within the bound, and counts nothing (the reference returns 1 there, with its
    result written)"""
    g = fixture()
    for rname, rsolver, niter in runs_of(g, 'van_leer'):
        check_run(g, 'van_leer', rname, rsolver, niter)


@pytest.mark.gpu
@pytest.mark.parametrize('variant', [6, 0])
def test_hllc_counts_the_pairs_with_a_nan_among_the_wave_speeds(variant):
    """one particle with p = NaN, others with p < 0 (sqrt gives NaN): the ordered pairs and self pairs the reference
    counts, zeros on those destinations, and the solvable pairs of the same launch solved"""
    check_run(fixture(), 'hllc_nan', 'hllc', 3, 20, variant)


@pytest.mark.gpu
@pytest.mark.parametrize('variant', [6, 0])
@pytest.mark.parametrize('rsolver', [4, 7])
def test_min_and_max_take_pythons_way_on_a_nan(rsolver, variant):
    """p < 0 on one particle of a pair.  ducowicz ends in max(pstar, 0.0) with pstar a NaN: Python returns its first
    argument unless the second is larger, so the NaN stands (fmax would return 0) and must reach au and ae of both
    particles, with nothing counted; llxf's max(csr, csl) passes a NaN csl over and keeps a NaN csr, and its finite pairs
    are within the bound"""
    check_run(fixture(), 'minmax_nan', SOLVERS[rsolver], rsolver, 20, variant)


@pytest.mark.gpu
@pytest.mark.parametrize('variant', [6, 0])
@pytest.mark.parametrize('key', ['recon/mono1', 'recon/mono2', 'recon/dt'])
def test_reconstruction_and_fallbacks_through_roe(key, variant):
    """gradient columns set by hand to powers of two: the four fallbacks, a state of exactly 0 (no fallback), the sign
    test and the shock switch of monotonicity=1 at equality and one ulp beyond, every return of monotonicity_min in rho,
    p and u, and 1 - cs dt sij < 0.  roe reads all six arguments; its result on the arguments the reference formed is
    the truth."""
    check_run(fixture(), key, 'roe', 6, 20, variant)
