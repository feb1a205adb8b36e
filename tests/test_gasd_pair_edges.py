"""The five gas-dynamics pair families (``FamGasSD_T``, ``FamMPM_T``, ``FamADKESD_T``, ``FamADKE_T``, ``FamGasWall_T``,
pysph_amd/csrc/sph_fam_gas.h), one isolated cluster at a time, against the reference's own classes evaluated at 50 digits
(tests/golden/gasd_pair_edges.npz, made by tests/golden/make_gasd_pair_golden.py; the tests read nothing but that file).

Every table is a row of isolated pairs and triples, 1 apart, and runs ONE equation alone in one Group, one sweep (the
iterating density group with max_iterations = 1), in 1-D under CubicSpline and Gaussian, in 2-D under CubicSpline and in
3-D under QuinticSpline.  Every output element has a scale S -- for a sum, the sum of |increment| over the cluster; for a
column post_loop derives, the first-order propagation of those through the formula plus the formula's own terms (the
generator's docstring has the rules) -- and an error is counted in units of u S, u = 2^-53.  With K_ref the reference's own
double result in that measure, an element with K_ref <= 64 whose 50-digit run took the double run's path is
well-conditioned; K_eq is the largest K_ref over the well-conditioned elements of an equation, and the device is held to
max(4, 4 K_eq) on each of them and to 4 K_ref of the element itself on the others (the rule of tests/test_nosrc_edges.py
and tests/test_gsph_riemann_edges.py).  An element of scale 0 must be exact: ``converged``, h of a row that came in
converged or that no fluid reaches, arho = 0 behind the ADKE density sweep.  Inputs come back bit for bit, the NaN pattern
equals the reference's, the convergence word equals the reference's, the neighbour lists equal the clusters.

Measured on an MI355X: DESIGN.md, sections 7g and 7i.

Mutants.  Each of the following changes was made to the text of the reference's method in memory (the way the generator
builds its inverted comparisons) or to the symbol the sweep is handed, and run in double over the stored inputs on the
CPU; "caught" = the result leaves the bound of this file in at least one stored element (tools: the generator's
``sweep`` and ``leaves_bound``).  No mutant was built for or run on the GPU.
The figure is the number of stored destinations that leave it.
    MPMAccelerations      omega_j dropped from the source's pressure term (``pjw`` without ``s[8]``)      caught (452)
                          DWJ at h_i (``gi`` for ``tj``)                                                  caught (464)
                          RIJ < 1e-8 changed to 1e-6, to 2e-8 (the pairs at 2^-26), to 5e-9 (at 2^-27)   caught (32 each)
                          viscous heating with dot in place of dot dot                                    caught (196)
                          dot <= 0 changed to dot < 0                                                     NOT caught
    SummationDensity      1.2 changed to 1.25                                                             caught (105)
                          0.8 changed to 0.75                                                             caught (70)
                          the reset omegai < 0 -> 1 never taken                                           caught (16)
                          ah also written for a row that does not converge                                caught (189)
                          WI, DWI, GHI at HIJ                                                             caught (352)
    SummationDensityADKE  h not reset to h0 before the sweep                                              caught (136)
                          DWI at HIJ                                                                      caught (136)
    ADKEAccelerations     RHOIJ in place of RHOIJ1                                                        caught (104)
                          g2 as given in place of g1 in Hj                                                caught (106)
                          XIJ.VIJ < 0 changed to <= 0                                                     NOT caught
    WallBoundary          wij > 1e-30 changed to wij > 0, to wij > 1e-28                                  caught (4 each)
                          WI at HIJ                                                                       caught (68)
The two that are not caught are equivalent mutants, out of reach of any test of values: with dot = 0 (XIJ.VIJ = 0) the
viscous terms carry the factor dot (muij) and add zeros on either side of the comparison.
"""
import importlib.util
import json
import os

import numpy as np
import pytest

from conftest import load_golden

U53 = 2.0 ** -53
WELL, FACTOR, MARGIN = 64.0, 4.0, 1e-3
EQUATIONS = ('SummationDensity', 'MPMAccelerations', 'SummationDensityADKE', 'ADKEAccelerations', 'WallBoundary')
OUTPUTS = {
    'SummationDensity': ('rho', 'arho', 'grhox', 'grhoy', 'grhoz', 'dwdh', 'div', 'omega', 'ah', 'h', 'converged'),
    'MPMAccelerations': ('au', 'av', 'aw', 'ae', 'del2e', 'dt_cfl', 'aalpha1', 'aalpha2'),
    'SummationDensityADKE': ('rho', 'arho', 'div', 'logrho', 'h'),
    'ADKEAccelerations': ('au', 'av', 'aw', 'ae'),
    'WallBoundary': ('p', 'u', 'v', 'w', 'm', 'rho', 'e', 'cs', 'div', 'wij', 'h', 'htmp'),
}
REQUIRED = (
    'clamp_up', 'clamp_down', 'no_clamp', 'fallback_small_h', 'omega_reset', 'converged_now', 'not_converged',
    'already_converged', 'once', 'density_iterations_false',
    'approaching', 'receding', 'rij_below_1e-8', 'rij_above_1e-8', 'coincident_pair_unequal_h', 'dt_cfl_from_partner',
    'dt_cfl_from_self', 'dt_cfl_stays_zero', 'update_alpha1_div_negative', 'update_alpha1_div_positive', 'update_alpha2',
    'adke_approaching', 'adke_receding', 'adke_div_pp', 'adke_div_pn', 'adke_div_np', 'adke_div_nn',
    'reached', 'reached_tiny', 'below_threshold', 'not_reached')
CONFIGS = ('1d_cubic', '1d_gauss', '2d_cubic', '3d_quintic')
KINDS = {'SummationDensity': ('main', 'once', 'noiter', 'small'), 'MPMAccelerations': ('main', 'two_a', 'two_b'),
         'SummationDensityADKE': ('main',), 'ADKEAccelerations': ('main',), 'WallBoundary': ('main',)}
TABLES = ['%s/%s/%s' % (e, k, c) for c in CONFIGS for e in EQUATIONS for k in KINDS[e]]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

_G = []


def fixture():
    if not _G:
        _G.append(load_golden('gasd_pair_edges.npz'))
    return _G[0]


def spec_of(g, key):
    return json.loads(str(g[key + '/spec']))


def column(g, key, what, c):
    return g['%s/%s' % (key, what)][OUTPUTS[spec_of(g, key)['equation']].index(c)]


def k_eq(g):
    return json.loads(str(g['meta/k_eq']))


def measure(got, hi, lo, S):
    """|got - (hi + lo)| / (u S) per element, the subtraction in mpmath; 0 where equal, inf where the scale is 0 and they
    differ or where ``got`` is a NaN"""
    import mpmath as mp
    k = np.zeros(len(got))
    with mp.workdps(50):
        for i in range(len(got)):
            if got[i] != got[i]:
                k[i] = np.inf
                continue
            d = abs(mp.mpf(float(got[i])) - (mp.mpf(float(hi[i])) + mp.mpf(float(lo[i]))))
            if d != 0:
                k[i] = float(d / (mp.mpf(U53) * mp.mpf(float(S[i])))) if S[i] != 0 else np.inf
    return k


def bounds(g, key):
    """{column: (bound per element in units of u S, well-conditioned per element)}"""
    eqname = spec_of(g, key)['equation']
    flat = max(FACTOR, FACTOR * k_eq(g)[eqname])
    mpok = g[key + '/mpok']
    out = {}
    for c in OUTPUTS[eqname]:
        kref = column(g, key, 'kref', c).astype(np.float64)
        well = mpok & (kref <= WELL)
        out[c] = (np.where(well, flat, FACTOR * kref), well)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------------
def test_golden_generator_imports_cleanly():
    if not os.path.isdir('/root/reference'):
        pytest.skip('the generator needs the reference (build container only)')
    spec = importlib.util.spec_from_file_location('make_gasd_pair_golden', os.path.join(GOLDEN, 'make_gasd_pair_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert callable(mod.main) and mod.OUT.endswith('gasd_pair_edges.npz')
    assert mod.REQUIRED == REQUIRED and (mod.WELL, mod.FACTOR, mod.MARGIN) == (WELL, FACTOR, MARGIN)
    assert mod.OUTPUTS == OUTPUTS and mod.EQUATIONS == EQUATIONS
    assert set(mod.MUTANTS) == set(REQUIRED)


def test_the_conditions_asserted_on_the_reference_are_in_the_file():
    """items 1..6 of the generator's docstring, from the stored data"""
    g = fixture()
    assert os.path.getsize(os.path.join(GOLDEN, 'gasd_pair_edges.npz')) < 1024 * 1024
    assert json.loads(str(g['tables'])) == TABLES
    assert tuple(json.loads(str(g['meta/required']))) == REQUIRED
    assert tuple(g['meta/constants']) == (WELL, FACTOR, MARGIN)
    taken = dict((b, 0) for b in REQUIRED)
    ks = k_eq(g)
    for eqname in EQUATIONS:
        bad = total = 0
        best = 0.0
        for key in TABLES:
            if not key.startswith(eqname + '/'):
                continue
            sp = spec_of(g, key)
            n = g['%s/in/%s' % (key, sp['dest'])].shape[1]
            assert n <= 512 and sum(g['%s/in/%s' % (key, a)].shape[1] for a in sp['arrays']) <= 512
            for names in json.loads(str(g[key + '/names'])):
                for b in names:
                    if b in taken:
                        taken[b] += 1
            assert np.all(g[key + '/margin'] >= MARGIN), key                       # item 2
            kref, mpok = g[key + '/kref'].astype(np.float64), g[key + '/mpok']
            assert kref.shape == (len(OUTPUTS[eqname]), n)
            well = mpok & (kref.max(axis=0) <= WELL)
            bad += int(np.sum(~well))
            total += n
            el = kref[:, mpok]
            best = max(best, float(np.max(el[el <= WELL], initial=0.0)))
            # every h within [2^-4, 2^-2] (times 2^-24 in the scaled table)
            s = 2.0 ** -24 if '/small/' in key else 1.0
            for a in sp['arrays']:
                h = g['%s/in/%s' % (key, a)][sp['in'][a].index('h')]
                assert np.all((h >= s * 2.0 ** -4) & (h <= s * 2.0 ** -2)), key
        assert bad * 10 <= total, (eqname, bad, total)                           # item 4
        assert best == ks[eqname] and best <= WELL, (eqname, best, ks[eqname])     # item 5
    short = dict((b, n) for b, n in taken.items() if n < 2)
    assert not short, short                                                      # item 1
    observed = json.loads(str(g['meta/observed']))
    assert all(observed[b] >= 2 for b in REQUIRED), observed                     # item 3
    sensitive = json.loads(str(g['meta/sensitive']))
    assert all(sensitive[e] >= 1 for e in EQUATIONS), sensitive                  # item 6
    dropped = json.loads(str(g['meta/dropped']))
    assert len(dropped) == 4 and all('lone' in d['table'] for d in dropped)
    # the two constructed wall rows: a factor 8 either side of 1e-30
    seen = {'reached_tiny': 0, 'below_threshold': 0}
    for key in TABLES:
        if key.startswith('WallBoundary/'):
            wij = column(g, key, 'ref', 'wij')
            for i, names in enumerate(json.loads(str(g[key + '/names']))):
                if 'reached_tiny' in names:
                    assert 8e-30 <= wij[i] < 1e-27
                    seen['reached_tiny'] += 1
                if 'below_threshold' in names:
                    assert 0 < wij[i] <= 1e-30 / 8
                    seen['below_threshold'] += 1
    assert min(seen.values()) >= 2, seen


def test_the_stored_reference_is_within_its_own_k_of_the_50_digit_values():
    """ref, mp + mplo, S and kref of the file agree: K recomputed in mpmath equals the stored float32 figure"""
    g = fixture()
    for key in TABLES:
        eqname = spec_of(g, key)['equation']
        for c in OUTPUTS[eqname]:
            k = measure(column(g, key, 'ref', c), column(g, key, 'mp', c), column(g, key, 'mplo', c), column(g, key, 'S', c))
            kref = column(g, key, 'kref', c).astype(np.float64)
            assert np.array_equal(np.isinf(k), np.isinf(kref)), (key, c)
            fin = np.isfinite(k)
            assert np.allclose(k[fin], kref[fin], rtol=1e-6, atol=0.0), (key, c)          # (kref is a float32)


def test_exact_elements_of_the_file():
    """what the GPU test compares exactly is exact in the file: scale 0 where the value is an input or a constant"""
    g = fixture()
    for key in TABLES:
        sp = spec_of(g, key)
        eqname = sp['equation']
        names = json.loads(str(g[key + '/names']))
        if eqname == 'SummationDensity':
            assert np.all(column(g, key, 'S', 'converged') == 0)
            h_in = g['%s/in/%s' % (key, sp['dest'])][sp['in'][sp['dest']].index('h')]
            for i, nm in enumerate(names):
                if 'already_converged' in nm or 'density_iterations_false' in nm:
                    assert column(g, key, 'S', 'h')[i] == 0 and column(g, key, 'ref', 'h')[i] == h_in[i]
        if eqname == 'SummationDensityADKE':
            assert np.all(column(g, key, 'S', 'arho') == 0) and np.all(column(g, key, 'ref', 'arho') == 0)
        if eqname == 'WallBoundary':
            h0 = g['%s/in/%s' % (key, sp['dest'])][sp['in'][sp['dest']].index('h0')]
            for i, nm in enumerate(names):
                if 'not_reached' in nm or 'below_threshold' in nm:
                    assert column(g, key, 'S', 'h')[i] == 0 and column(g, key, 'ref', 'h')[i] == h0[i]
                if 'not_reached' in nm:
                    assert all(column(g, key, 'ref', c)[i] == 0 for c in OUTPUTS[eqname] if c != 'h')


# ---------------------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------------------
def build_arrays(g, key):
    """the table's arrays with every property its scheme sets up; the stored columns pushed as they are, every pure
    output column garbage"""
    from pysph_amd.gas_dynamics import ADKEScheme, GasDScheme
    from pysph_amd.particle_array import ParticleArray
    sp = spec_of(g, key)
    eqname = sp['equation']
    rng = np.random.default_rng(len(key))
    arrays = []
    for name in sp['arrays']:
        cols = dict(zip(sp['in'][name], g['%s/in/%s' % (key, name)]))
        arrays.append(ParticleArray(name=name, **dict((c, v.copy()) for c, v in cols.items())))
    if eqname in ('SummationDensity', 'MPMAccelerations'):
        GasDScheme(sp['arrays'], [], dim=sp['dim'], gamma=1.4, kernel_factor=1.2).setup_properties(arrays)
    else:
        fluids = [a for a in sp['arrays'] if a != 'wall']
        ADKEScheme(fluids, [a for a in sp['arrays'] if a == 'wall'], dim=sp['dim']).setup_properties(arrays)
    for pa in arrays:
        stored = sp['in'][pa.name]
        for c in stored:
            pa.properties[c][:] = g['%s/in/%s' % (key, pa.name)][stored.index(c)]
        if pa.name == sp['dest']:
            for c in OUTPUTS[eqname]:
                if c not in stored:
                    pa.properties[c][:] = rng.uniform(-7.0, 7.0, pa.properties[c].size)      # must be overwritten
    return arrays


def group_of(sp):
    from pysph_amd import gas_dynamics as GD
    from pysph_amd.equations import Group
    cls = getattr(GD, sp['equation'])
    eq = cls(dest=sp['dest'], sources=list(sp['sources']), **sp['params'])
    if sp['equation'] == 'SummationDensity' and sp['params']['density_iterations']:
        return eq, [Group(equations=[eq], update_nnps=True, iterate=True, max_iterations=1)]
    return eq, [Group(equations=[eq])]


def run_table(g, key, variant):
    """one launch of one equation over one table against the file; returns (worst K over the well-conditioned elements,
    where, the bound, worst fraction of their own bound of the others)"""
    from pysph_amd import kernels as K
    from test_gsph_gpu import evaluator, pull_all, _floats
    sp = spec_of(g, key)
    eqname = sp['equation']
    arrays = build_arrays(g, key)
    by_name = dict((pa.name, pa) for pa in arrays)
    before = dict(((pa.name, c), pa.properties[c].copy()) for pa in arrays for c in _floats(pa))
    eq, groups = group_of(sp)
    a_eval, nnps, ctx = evaluator(arrays, groups, getattr(K, sp['kernel'])(dim=sp['dim']), variant)
    nnps.update()
    names = [pa.name for pa in arrays]
    for sn in sp['sources']:                   # the neighbour lists are the clusters, nothing leaks across
        start, idx = nnps.get_csr(names.index(sn), names.index(sp['dest']))
        assert np.array_equal(start, g['%s/nbr_start/%s' % (key, sn)]), (key, sn)
        assert np.array_equal(idx, g['%s/nbr_idx/%s' % (key, sn)]), (key, sn)
    a_eval.compute(0.0, 0.0)
    flag = eq.converged() if hasattr(eq, 'converged') else 1
    pull_all(arrays)
    ctx.close()
    assert flag == sp['flag'], (key, flag, sp['flag'])
    dest = by_name[sp['dest']]
    for (name, c), v in before.items():
        if not (name == sp['dest'] and c in OUTPUTS[eqname]):
            assert np.array_equal(by_name[name].properties[c], v, equal_nan=True), (key, name, c, 'an input column changed')
    bnd = bounds(g, key)
    mpok = g[key + '/mpok']
    worst, where, ill = 0.0, None, 0.0
    for c in OUTPUTS[eqname]:
        got, ref = dest.properties[c], column(g, key, 'ref', c)
        assert np.array_equal(np.isnan(got), np.isnan(ref)), (key, c, 'NaN pattern')
        S = column(g, key, 'S', c)
        k = measure(got, column(g, key, 'mp', c), column(g, key, 'mplo', c), S)
        exact = (S == 0)
        assert np.all(k[exact] == 0), (key, c, 'an element of scale 0 is not exact', np.nonzero(exact & (k != 0))[0][:4],
                                       got[exact & (k != 0)][:4], ref[exact & (k != 0)][:4])
        bound, well = bnd[c]
        if np.any(well) and k[well].max() > worst:
            worst, where = float(k[well].max()), (c, int(np.argmax(np.where(well, k, -1.0))))
        rest = mpok & ~well
        with np.errstate(invalid='ignore', divide='ignore'):
            ill = max(ill, float(np.max((k / bound)[rest & (k > 0)], initial=0.0)))
        bad = np.nonzero(mpok & ~(k <= bound))[0]       # (a row whose 50-digit run took another path is not compared)
        assert bad.size == 0, (key, c, 'variant %d' % variant,
                               [(int(i), float(k[i]), float(bound[i]), float(got[i]), float(ref[i])) for i in bad[:4]])
    flat = max(FACTOR, FACTOR * k_eq(g)[eqname])
    print('%s variant %d: device K %.3f at %s (bound %.1f); ill-conditioned elements at most %.3f of their own bound'
          % (key, variant, worst, where, flat, ill))
    return worst, where, flat, ill


@pytest.mark.gpu
@pytest.mark.parametrize('variant', [6, 0])
@pytest.mark.parametrize('key', TABLES)
def test_every_cluster_of_the_table(key, variant):
    """one equation alone over one table, both schedules: every output element within its bound of the 50-digit value,
    scale-0 elements exact, the convergence word, the NaN pattern, the neighbour lists, the inputs bit for bit"""
    run_table(fixture(), key, variant)
