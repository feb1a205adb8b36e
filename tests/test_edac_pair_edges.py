"""The EDAC force family and the average pressure (``FamEDAC_T<T, INT>``, ``FamAvgP_T``, pysph_amd/csrc/sph_fam_tvf.h), one
isolated cluster at a time, against the reference's own classes evaluated at 50 digits (tests/golden/edac_pair_edges.npz,
made by tests/golden/make_edac_pair_golden.py with the machinery of make_gasd_pair_golden.py; the tests read nothing
but that file).

Every table is a row of isolated lone particles, pairs and triples, 1 apart, and runs ONE GROUP, the smallest the
product takes into the family: an equation alone where the product accepts it alone (ComputeAveragePressure, both
pressure gradients, EDACEquation), next to a base equation where it does not (the physical and the artificial viscosity
next to EDACEquation, the artificial stress next to the internal pressure gradient with pressures of 2^-8, XSPHCorrection
next to the external one), the two default force groups of EDACScheme (the flag sets compiled as constants) and one
internal group fluid <- {fluid, solid} with EDACScheme's source lists (the run-time-flag kernel; F_EINT reaches the
solid source).  Four configurations (1-D CubicSpline, 2-D WendlandQuintic, 3-D QuinticSpline, 3-D Gaussian), each table
in a ``uh`` form (every h equal: under variant 6 the seven-piece 112-byte records) and a ``vh`` form (h unequal inside
the clusters: the generic 128-byte records, the UH = false geometry), every table under pair_variant 6 and 0, at a stored
t != 0.  The library reports the family that ran (the launch counters ``pair_edac`` / ``pair_avg_pressure``, asserted
here) but neither the record layout nor the flag kernel: those follow from the construction (hmin == hmax; the flag
set equal to the family's CF0 or not).

Bound.  Every output element has a scale S (for a sum, the sum of |increment| over the cluster across all equations of
the group that write the column; behind post_loop the first-order propagation of the generator's rules) and an error is
counted in units of u S, u = 2^-53.  K_ref = the reference's own double result in that measure; an element with
K_ref <= 64 whose 50-digit run took the double run's lines is well-conditioned; K_eq = the largest K_ref over the
well-conditioned elements of a table label, measured by the generator on the reference alone (meta/k_eq).  The device
is held to max(4, 4 K_eq) u S on a well-conditioned element and to 4 K_ref of the element itself on any other; an element
of scale 0 is exact (every gradient term of a partner at 2^-40 or at distance 0, pavg and nnbr of a row no source
reaches); pavg of a row that sees itself only equals its p, ax ay az under eps = 0 equal u v w; the NaN pattern equals
the reference's; every other column of every array comes back bit for bit; the neighbour lists equal the clusters.
(WELL, FACTOR, MARGIN) = (64, 4, 1e-3), the project's constants.

Measured on an MI355X: DESIGN.md, section 7f ("Pair by pair").

Mutants.  Each of the following changes was made to the text of the reference's method in memory (or to the parameters
the group is built with, or to the sweep) and run in double over the stored inputs on the CPU
(``make_edac_pair_golden.py --mutants``); "caught" = the result leaves the bound of this file (or the mutant raises where
the reference does not: EPS dropped divides by zero in the self pair); the figure is the number of stored destinations
that leave it.  No mutant was built for or run on the GPU.
    edac_nu swapped with nu                                            caught (1416)
    Vi2 + Vj2 replaced by 2 Vi2 (pressure rate)                        caught (1344)
    Vi2 + Vj2 replaced by 2 Vi2 (internal gradient)                    caught (940)
    Vi2 + Vj2 replaced by 2 Vi2 (pb term)                              caught (940)
    pavg taken off one pressure only                                   caught (940)
    rho_i / rho_j inverted in the pressure rate                        caught (1500)
    m_j replaced by m_i in the pressure rate                           caught (1500)
    rho_j p_i + rho_i p_j with the densities swapped (external)        caught (990)
    EPS dropped from the viscosity                                     caught (1216)
    etaij without the factor 2                                         caught (808)
    HIJ dropped from muij                                              caught (210)
    vijdotrij < 0 changed to <= 0                                      NOT caught
    artificial stress: uhat_j - u_j replaced by uhat_i - u_i           caught (575)
    artificial stress: the factor 0.5 of Ay dropped                    caught (444)
    XSPH: RHOIJ1 squared                                               caught (640)
    XSPH: u not added behind the loop                                  caught (912)
    tdamp ramp with +1/2 for -1/2                                      caught (616)
    t < tdamp changed to t <= tdamp                                    NOT caught
    nnbr > 0 changed to nnbr > 1                                       NOT caught
    the self pair left out (pavg, nnbr, the summed density)            caught (640)
The three that are not caught are equivalent mutants, out of reach of any test of values: with vijdotrij = 0 muij
carries the factor vijdotrij and the pair adds zeros on either side; at t = tdamp the ramp
0.5 (sin((-1/2 + 1) pi) + 1) is exactly 1.0 in double, what the other side writes (for the same reason the branch
``tdamp_equal`` is taken, stored and compared, but exempt from the observability condition); with nnbr = 1 the
division is by 1.
"""
import importlib.util
import json
import os

import numpy as np
import pytest

from conftest import load_golden
from test_gasd_pair_edges import measure

WELL, FACTOR, MARGIN = 64.0, 4.0, 1e-3
LABELS = ('ComputeAveragePressure', 'MomentumEquation', 'MomentumEquationPressureGradient', 'EDACEquation',
          'MomentumEquationViscosity', 'MomentumEquationArtificialViscosity', 'MomentumEquationArtificialStress',
          'XSPHCorrection', 'external_group', 'internal_group', 'internal_solid_group')
REQUIRED = ('nnbr_positive', 'nnbr_zero', 'nnbr_self_only', 'tdamp_ramp', 'tdamp_equal', 'tdamp_past', 'tdamp_zero',
            'approaching', 'receding', 'p_equal', 'eps_zero', 'rij_below_1e-12', 'rij_above_1e-12', 'coincident_unequal_h')
UNOBSERVABLE = ('tdamp_equal',)
CONFIGS = ('1d_cubic', '2d_wendland', '3d_quintic', '3d_gauss')
# (label, kind, forms), in the generator's order
KINDS = (('ComputeAveragePressure', 'alone', ('uh', 'vh')), ('ComputeAveragePressure', 'density', ('uh', 'vh')),
         ('ComputeAveragePressure', 'other', ('vh',)), ('MomentumEquation', 'alone', ('uh', 'vh')),
         ('MomentumEquationPressureGradient', 'alone', ('uh', 'vh')), ('EDACEquation', 'alone', ('uh', 'vh')),
         ('MomentumEquationViscosity', 'edac', ('uh', 'vh')), ('MomentumEquationArtificialViscosity', 'edac', ('uh', 'vh')),
         ('MomentumEquationArtificialStress', 'gradient', ('uh', 'vh')), ('XSPHCorrection', 'momentum', ('uh', 'vh')),
         ('XSPHCorrection', 'eps0', ('uh',)), ('external_group', 'default', ('uh', 'vh')),
         ('internal_group', 'default', ('uh', 'vh')), ('internal_solid_group', 'solid', ('uh', 'vh')),
         ('ComputeAveragePressure', 'other', ('uh',)), ('XSPHCorrection', 'eps0', ('vh',)))
TABLES = ['%s/%s/%s/%s' % (label, kind, c, f) for c in CONFIGS for f in ('uh', 'vh') for label, kind, forms in KINDS if f in forms]
INTERNAL = ('ComputeAveragePressure', 'SummationDensity', 'MomentumEquationPressureGradient', 'MomentumEquationArtificialStress')
AVGP = ('ComputeAveragePressure', 'SummationDensity')
# the flag sets the two instantiations of the family compile as constants (EDACScheme's default force groups)
CF0 = (('MomentumEquation', 'MomentumEquationViscosity', 'EDACEquation', 'XSPHCorrection'),
       ('MomentumEquationPressureGradient', 'MomentumEquationViscosity', 'MomentumEquationArtificialStress', 'EDACEquation'))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FILE = 'edac_pair_edges.npz'

_G = []


def fixture():
    if not _G:
        _G.append(load_golden(FILE))
    return _G[0]


_SPECS = {}


def spec_of(g, key):
    if (id(g), key) not in _SPECS:
        _SPECS[(id(g), key)] = json.loads(str(g[key + '/spec']))
    return _SPECS[(id(g), key)]


def column(g, key, what, c):
    """ref, mp, mplo (doubles) or S, kref (the two planes of f32) of one output column"""
    k = spec_of(g, key)['outputs'].index(c)
    if what in ('ref', 'mp', 'mplo'):
        return g['%s/%s' % (key, what)][k]
    return g[key + '/f32'][('S', 'kref').index(what)][k].astype(np.float64)


def inputs(g, key, name):
    sp = spec_of(g, key)
    return dict(zip(sp['in'][name], g['%s/in/%s' % (key, name)]))


def k_eq(g):
    return json.loads(str(g['meta/k_eq']))


def bounds(g, key):
    """{column: (bound per element in units of u S, well-conditioned per element)}"""
    sp = spec_of(g, key)
    flat = max(FACTOR, FACTOR * k_eq(g)[sp['label']])
    mpok = np.array(sp['mpok'], bool)
    out = {}
    for c in sp['outputs']:
        kref = column(g, key, 'kref', c)
        well = mpok & (kref <= WELL)
        out[c] = (np.where(well, flat, FACTOR * kref), well)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------------
def test_golden_generator_imports_cleanly():
    if not os.path.isdir('/root/reference'):
        pytest.skip('the generator needs the reference (build container only)')
    spec = importlib.util.spec_from_file_location('make_edac_pair_golden', os.path.join(GOLDEN, 'make_edac_pair_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert callable(mod.main) and mod.OUT.endswith(FILE)
    assert mod.REQUIRED == REQUIRED and (mod.WELL, mod.FACTOR, mod.MARGIN) == (WELL, FACTOR, MARGIN)
    assert mod.LABELS == LABELS and mod.UNOBSERVABLE == UNOBSERVABLE
    assert set(mod.MUTANTS) == set(REQUIRED) and set(mod.SENSITIVE) == set(LABELS)
    assert set(mod.EQUIVALENT) <= set(e[0] for e in mod.ARITH)


def test_the_conditions_asserted_on_the_reference_are_in_the_file():
    """items 1..6 of the generator's docstring, from the stored data"""
    g = fixture()
    assert os.path.getsize(os.path.join(GOLDEN, FILE)) < 1024 * 1024
    assert json.loads(str(g['tables'])) == TABLES
    assert tuple(json.loads(str(g['meta/required']))) == REQUIRED
    assert tuple(json.loads(str(g['meta/unobservable']))) == UNOBSERVABLE
    assert tuple(g['meta/constants']) == (WELL, FACTOR, MARGIN)
    taken = dict((b, 0) for b in REQUIRED)
    ks = k_eq(g)
    assert set(ks) == set(LABELS)
    for label in LABELS:
        bad = total = 0
        best = 0.0
        for key in TABLES:
            sp = spec_of(g, key)
            if sp['label'] != label:
                continue
            n = g['%s/in/%s' % (key, sp['dest'])].shape[1]
            assert sum(g['%s/in/%s' % (key, a)].shape[1] for a in sp['arrays']) <= 512
            assert sp['t'] != 0.0
            for names in sp['names']:
                for b in names:
                    taken[b] += 1
            assert np.all(g[key + '/margin'] >= MARGIN), key                      # item 2
            kref = g[key + '/f32'][1].astype(np.float64)
            mpok = np.array(sp['mpok'], bool)
            assert kref.shape == (len(sp['outputs']), n) and mpok.shape == (n,)
            well = mpok & (kref.max(axis=0) <= WELL)
            bad += int(np.sum(~well))
            total += n
            el = kref[:, mpok]
            best = max(best, float(np.max(el[el <= WELL], initial=0.0)))
            hs = [inputs(g, key, a)['h'] for a in sp['arrays']]
            for h in hs:
                assert np.all((h >= 2.0 ** -4) & (h <= 2.0 ** -2)), key
            if sp['form'] == 'uh':
                assert all(np.all(h == 2.0 ** -3) for h in hs), key
            else:
                assert np.unique(np.concatenate(hs)).size > 8, key
            for a in sp['arrays']:                                              # V is an input near rho / m
                cols = inputs(g, key, a)
                if 'V' in cols:
                    assert np.all(np.abs(cols['V'] * cols['m'] / cols['rho'] - 1.0) <= 0.1 + 1e-12), key
        assert total > 0 and bad * 10 <= total, (label, bad, total)               # item 4
        assert best == ks[label] and best <= WELL, (label, best, ks[label])         # item 5
    short = dict((b, n) for b, n in taken.items() if n < 2)
    assert not short, short                                                       # item 1
    observed = json.loads(str(g['meta/observed']))
    assert all(observed[b] >= 2 for b in REQUIRED if b not in UNOBSERVABLE), observed     # item 3
    sensitive = json.loads(str(g['meta/sensitive']))
    assert all(sensitive[e] >= 1 for e in LABELS), sensitive                      # item 6
    # the two default force groups are the constant flag sets, one of each branch; the group with the solid is not
    for key in TABLES:
        sp = spec_of(g, key)
        eqs = tuple(e['name'] for e in sp['group'])
        if sp['label'] == 'external_group':
            assert eqs == CF0[0] and sp['sources'] == ['fluid']
        if sp['label'] == 'internal_group':
            assert eqs == CF0[1] and sp['sources'] == ['fluid']
        if sp['label'] == 'internal_solid_group':
            by = dict((e['name'], e['sources']) for e in sp['group'])
            assert by['MomentumEquationPressureGradient'] == ['fluid', 'solid'] and by['EDACEquation'] == ['fluid', 'solid']
            assert by['MomentumEquationViscosity'] == ['fluid'] and by['MomentumEquationArtificialStress'] == ['fluid']


def test_the_stored_reference_is_within_its_own_k_of_the_50_digit_values():
    """ref, mp + mplo, S and kref of the file agree: K recomputed in mpmath equals the stored float32 figure"""
    g = fixture()
    for key in TABLES:
        for c in spec_of(g, key)['outputs']:
            k = measure(column(g, key, 'ref', c), column(g, key, 'mp', c), column(g, key, 'mplo', c), column(g, key, 'S', c))
            kref = column(g, key, 'kref', c)
            assert np.array_equal(np.isinf(k), np.isinf(kref)), (key, c)
            fin = np.isfinite(k)
            # (kref and S are float32; mplo has a 24-bit mantissa: 2^-24 of a remainder of at most u |value|)
            assert np.allclose(k[fin], kref[fin], rtol=1e-6, atol=1e-6), (key, c)


def test_exact_elements_of_the_file():
    """what the GPU test compares exactly is exact in the file"""
    g = fixture()
    seen = dict(zero=0, self_only=0, eps_zero=0, no_gradient=0)
    for key in TABLES:
        sp = spec_of(g, key)
        D = inputs(g, key, sp['dest'])
        for c in sp['outputs']:
            S, ref = column(g, key, 'S', c), column(g, key, 'ref', c)
            exact = S == 0
            assert np.array_equal(ref[exact], column(g, key, 'mp', c)[exact]) and np.all(column(g, key, 'mplo', c)[exact] == 0), (key, c)
        cl = np.array(sp['cl'][sp['dest']])
        members = sum(np.bincount(np.array(v), minlength=cl.max() + 1) for v in sp['cl'].values())
        for i, nm in enumerate(sp['names']):
            if 'nnbr_zero' in nm:
                assert all(column(g, key, w, c)[i] == 0 for w in ('ref', 'S') for c in ('pavg', 'nnbr'))
                seen['zero'] += 1
            if 'nnbr_self_only' in nm:
                assert column(g, key, 'ref', 'pavg')[i] == D['p'][i] and column(g, key, 'ref', 'nnbr')[i] == 1.0
                seen['self_only'] += 1
            if 'eps_zero' in nm:
                assert all(column(g, key, 'ref', 'a' + x)[i] == D[u][i] for x, u in zip('xyz', 'uvw'))
                seen['eps_zero'] += 1
            if ('rij_below_1e-12' in nm or 'coincident_unequal_h' in nm) and members[cl[i]] == 2 and sp['label'] == 'EDACEquation':
                assert column(g, key, 'S', 'ap')[i] == 0 and column(g, key, 'ref', 'ap')[i] == 0       # every term carries DWIJ
                seen['no_gradient'] += 1
    assert min(seen.values()) >= 2, seen


# ---------------------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------------------
def build_arrays(g, key):
    """the table's arrays with every property EDACScheme sets up; the stored columns pushed as they are, every other
    column (the outputs, and what the group neither reads nor writes) garbage"""
    from pysph_amd.edac import EDACScheme
    from pysph_amd.particle_array import ParticleArray
    sp = spec_of(g, key)
    rng = np.random.default_rng(len(key))
    arrays = []
    for name in sp['arrays']:
        arrays.append(ParticleArray(name=name, **dict((c, v.copy()) for c, v in inputs(g, key, name).items())))
    internal = any(e['name'] in INTERNAL for e in sp['group'])
    EDACScheme(['fluid'], [a for a in sp['arrays'] if a != 'fluid'], dim=sp['dim'], c0=1.5, nu=0.375, rho0=1.0,
               pb=1.25 if internal else 0.0, h=2.0 ** -3).setup_properties(arrays)
    for pa in arrays:
        stored = inputs(g, key, pa.name)
        for c in pa.properties:
            if pa.properties[c].dtype != np.float64:
                continue
            if c in stored:
                pa.properties[c][:] = stored[c]
            else:
                pa.properties[c][:] = rng.uniform(-7.0, 7.0, pa.properties[c].size)
    return arrays


def group_of(sp):
    from pysph_amd import edac as ED
    from pysph_amd.equations import Group
    eqs = [getattr(ED, e['name'])(dest=sp['dest'], sources=list(e['sources']), **e['params']) for e in sp['group']]
    return [Group(equations=eqs)]


def run_table(g, key, variant):
    """one launch of one group over one table against the file; returns (worst K over the well-conditioned elements,
    where, the bound, worst fraction of their own bound of the others)"""
    from pysph_amd import kernels as K
    from test_gsph_gpu import evaluator, pull_all, _floats
    sp = spec_of(g, key)
    outs = sp['outputs']
    arrays = build_arrays(g, key)
    by_name = dict((pa.name, pa) for pa in arrays)
    before = dict(((pa.name, c), pa.properties[c].copy()) for pa in arrays for c in _floats(pa))
    a_eval, nnps, ctx = evaluator(arrays, group_of(sp), getattr(K, sp['kernel'])(dim=sp['dim']), variant)
    ctx.lib.sph_timer_enable(ctx._h, 1)
    nnps.update()
    names = [pa.name for pa in arrays]
    for sn in sp['sources']:                   # the neighbour lists are the clusters, nothing leaks across
        start, idx = nnps.get_csr(names.index(sn), names.index(sp['dest']))
        want = sp['nbr'][sn]
        assert np.array_equal(start, np.cumsum([0] + [len(v) for v in want])), (key, sn)
        got = [sorted(int(j) for j in idx[start[i]:start[i + 1]]) for i in range(len(want))]
        assert got == want, (key, sn)
    a_eval.compute(sp['t'], 0.0)
    family = 'pair_avg_pressure' if all(e['name'] in AVGP for e in sp['group']) else 'pair_edac'
    launches = dict((k, ctx.timer_get(k)[1]) for k in ('pair_edac', 'pair_avg_pressure', 'pair_tvf', 'pair_density', 'pair_wcsph'))
    pull_all(arrays)
    ctx.close()
    assert launches[family] == 1 and sum(launches.values()) == 1, (key, launches)      # the family under test, nothing else
    dest = by_name[sp['dest']]
    for (name, c), v in before.items():
        if not (name == sp['dest'] and c in outs):
            assert np.array_equal(by_name[name].properties[c], v, equal_nan=True), (key, name, c, 'an input column changed')
    D = inputs(g, key, sp['dest'])
    for i, nm in enumerate(sp['names']):
        if 'nnbr_self_only' in nm:
            assert dest.properties['pavg'][i] == D['p'][i] and dest.properties['nnbr'][i] == 1.0, (key, i)
        if 'eps_zero' in nm:
            assert all(dest.properties['a' + x][i] == D[u][i] for x, u in zip('xyz', 'uvw')), (key, i)
    bnd = bounds(g, key)
    mpok = np.array(sp['mpok'], bool)
    worst, where, ill = 0.0, None, 0.0
    for c in outs:
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
    flat = max(FACTOR, FACTOR * k_eq(g)[sp['label']])
    print('%s variant %d: device K %.3f at %s (bound %.1f); ill-conditioned elements at most %.3f of their own bound'
          % (key, variant, worst, where, flat, ill))
    return worst, where, flat, ill


@pytest.mark.gpu
@pytest.mark.parametrize('variant', [6, 0])
@pytest.mark.parametrize('key', TABLES)
def test_every_cluster_of_the_table(key, variant):
    """one group over one table, both schedules: every output element within its bound of the 50-digit value, scale-0
    elements exact, the family that ran, the NaN pattern, the neighbour lists, every other column bit for bit"""
    run_table(fixture(), key, variant)
