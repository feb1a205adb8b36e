"""The TVF force family (``FamTVF_T``, pysph_amd/csrc/sph_fam_tvf.h), one isolated cluster at a time, against the
reference's own classes evaluated at 50 digits (tests/golden/tvf_pair_edges.npz, made by
tests/golden/make_tvf_pair_golden.py with the machinery of make_edac_pair_golden.py and make_gasd_pair_golden.py; the
tests read nothing but that file).

Every table is a row of isolated lone particles, pairs and triples, 1 apart, and runs ONE GROUP, the smallest the
product takes into the family: each of the four force equations alone (the product accepts each alone), the pressure
gradient a second time with pb = 0, TVFScheme's default force group (its flag set is ``FamTVF_T::CF0``: the
constant-flag kernel), that group with the artificial viscosity (the run-time-flag kernel and, under ``uh``, the
seven-piece compact record, the only one that carries m) and one group fluid <- {fluid, solid} with TVFScheme's source
lists.  Four configurations (1-D CubicSpline, 2-D WendlandQuintic, 3-D QuinticSpline, 3-D Gaussian), each table in a
``uh`` form (every h is 2^-3: under variant 6 the compact records) and a ``vh`` form (h unequal inside the clusters: the
generic records, the UH = false geometry), every table under pair_variant 6 and 0, at the stored t = 1/4 with tdamp
changing from table to table (ramp, t == tdamp, t > tdamp, tdamp = 0).  The library reports the family that ran (the
launch counter ``pair_tvf``, asserted here, every other family 0); the record layout follows from the construction.

Bound.  That of tests/test_edac_pair_edges.py: every output element has a scale S (the sum of |increment| over the
cluster across all equations of the group that write the column, at 50 digits; behind post_loop the first-order
propagation of the generator's rules: a* += g damp) and an error is counted in units of u S, u = 2^-53.  K_ref = the
reference's own double result in that measure; an element with K_ref <= 64 whose 50-digit run took the double run's
lines is well-conditioned; K_eq = the largest K_ref over the well-conditioned elements of a table label, measured by the
generator on the reference alone (meta/k_eq).  The device is held to max(4, 4 K_eq) u S on a well-conditioned element and
to 4 K_ref of the element itself on any other; an element of scale 0 is exact (every gradient term of a partner at 2^-40
or at distance 0; auhat avhat awhat under pb = 0 and of a lone particle); a lone particle's au av aw equal g damp; the
NaN pattern equals the reference's; every other column of every array comes back bit for bit (auhat avhat awhat where
no pressure gradient ran); the neighbour lists equal the clusters.  (WELL, FACTOR, MARGIN) = (64, 4, 1e-3).

The records without p and V (``FamTVFE_T``, ``src_eos = 2``) engage where the force group follows TVF's density
summation and StateEquation, each over all particles, on device-resident state with one mass per array: p and
Vj2 = (m / rho)^2 are then recomputed from the gathered rho, so a stored reference of the force group alone does not
apply.  The ``fused_*`` tables (``uh``, one mass) hold the reference's three groups: ``fused_density`` the density
summation (judged alone like every other table: the family ``pair_density``), ``fused_force`` the default force group on
the double rho and V of the first table and p = StateEquation.loop of that rho.  ``test_records_without_p_and_v`` runs
[SummationDensity | StateEquation | force group] in one context: once to let the neighbour update learn the mass, then
with ``mass_fuse`` on (``n_eos_fused`` grows: the fused records) and with ``mass_fuse`` off (it does not).  rho and V of
either run are held to the density table's bound; p to the stored p with the scale of its formula, S_p = (p0 / rho0) S_rho
bound_rho + 4 (|p0 rho / rho0| + |p0 b|) in units of u.  The fused force outputs F are held to the unfused ones U element
by element: both evaluate the same terms, each of which carries the factor (Vi2 + Vj2) linearly, the pressure term
also (rho_j p_i + rho_i p_j) / (rho_i + rho_j) with p > 0 everywhere; swapping 1 / V_j^2 for (m_j / rho_j)^2 changes a
term by at most eV = max over the cluster of |(m / rho)^2 V^2 - 1| of its size, swapping the stored p for
p0 (rho / rho0 - b) by at most eP = max |p0 (rho / rho0 - b) - p| / |p| (both computed here in numpy in double from the
rho V m p the unfused run left), and the sizes of a destination's terms sum to at most its stored scale S, so
|F - U| <= (FACTOR K_eq u + eV + eP) S to first order; an element of scale 0 is equal.  The unfused family on the same
kind of input is what the plain tables judge.

Measured on an MI355X: DESIGN.md, section 7j ("Pair by pair").

Mutants.  Each of the following changes was made to the text of the reference's method in memory and run in double over
the stored inputs on the CPU (``make_tvf_pair_golden.py --mutants``); "caught" = the result leaves the bound of this
file (or the mutant raises where the reference does not: EPS dropped divides by zero in the self pair); the figure is the
number of stored destinations that leave it.  No mutant was built for or run on the GPU.
    Vi2 + Vj2 replaced by 2 Vi2 (pressure term)                        caught (1212)
    Vi2 + Vj2 replaced by 2 Vi2 (pb term)                              caught (964)
    Vi2 + Vj2 replaced by 2 Vi2 (viscosity)                            caught (768)
    rho_j p_i + rho_i p_j with the densities swapped                   caught (1210)
    EPS dropped from the viscosity                                     caught (1336)
    etaij without the factor 2                                         caught (848)
    HIJ dropped from muij                                              caught (319)
    s_m replaced by d_m in the artificial viscosity                    caught (319)
    vijdotrij < 0 changed to <= 0                                      NOT caught
    artificial stress: uhat_j - u_j replaced by uhat_i - u_i           caught (944)
    artificial stress: the factor 0.5 of Ay dropped                    caught (720)
    artificial stress: rho_j replaced by rho_i                         caught (848)
    tdamp ramp with +1/2 for -1/2                                      caught (336)
    t < tdamp changed to t <= tdamp                                    NOT caught
    the body force not damped                                          caught (488)
The two that are not caught are equivalent mutants, out of reach of any test of values: with vijdotrij = 0 muij carries
the factor vijdotrij and the pair adds zeros on either side (for the same reason the branch ``vijdotrij_zero`` is taken,
stored and compared, but exempt from the observability condition); at t = tdamp the ramp 0.5 (sin((-1/2 + 1) pi) + 1) is
exactly 1.0 in double, what the other side writes (``tdamp_equal``, exempt likewise).
"""
import importlib.util
import json
import os

import numpy as np
import pytest

from conftest import load_golden
from test_gasd_pair_edges import measure
from test_edac_pair_edges import spec_of, column, inputs, k_eq, bounds

WELL, FACTOR, MARGIN = 64.0, 4.0, 1e-3
_PG, _VISC, _AV, _AS = ('MomentumEquationPressureGradient', 'MomentumEquationViscosity', 'MomentumEquationArtificialViscosity',
                        'MomentumEquationArtificialStress')
LABELS = (_PG, _VISC, _AV, _AS, 'default_group', 'av_group', 'solid_group', 'fused_density', 'fused_force')
REQUIRED = ('tdamp_ramp', 'tdamp_equal', 'tdamp_past', 'tdamp_zero', 'approaching', 'receding', 'vijdotrij_zero',
            'rij_below_1e-12', 'rij_above_1e-12', 'coincident_unequal_h', 'rho_unequal', 'lone_particle', 'pb_zero')
UNOBSERVABLE = ('tdamp_equal', 'vijdotrij_zero')
CONFIGS = ('1d_cubic', '2d_wendland', '3d_quintic', '3d_gauss')
KINDS = ((_PG, 'alone'), (_PG, 'pb0'), (_VISC, 'alone'), (_AV, 'alone'), (_AS, 'alone'), ('default_group', 'default'),
         ('av_group', 'alpha'), ('solid_group', 'solid'))
FUSED = (('fused_density', 'alone'), ('fused_force', 'default'))       # uh only: the three groups of TVFScheme, one mass
TABLES = ['%s/%s/%s/%s' % (label, kind, c, f) for c in CONFIGS for f in ('uh', 'vh') for label, kind in KINDS + (FUSED if f == 'uh' else ())]
EOS = dict(p0=1.25, rho0=0.75, b=2.0 ** -10)
CF0 = (_PG, _VISC, _AS)         # the flag set FamTVF_T compiles as a constant: TVFScheme's default force group
FAMILIES = ('pair_wcsph', 'pair_density', 'pair_tvf', 'pair_vgrad', 'pair_elastic', 'pair_nbr', 'pair_wcsph_options',
            'pair_delta_sph_pre', 'pair_edac', 'pair_avg_pressure')
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FILE = 'tvf_pair_edges.npz'

_G = []


def fixture():
    if not _G:
        _G.append(load_golden(FILE))
    return _G[0]


# ---------------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------------
def load_generator(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(GOLDEN, name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_golden_generator_imports_cleanly():
    if not os.path.isdir('/root/reference'):
        pytest.skip('the generator needs the reference (build container only)')
    mod = load_generator('make_tvf_pair_golden')
    assert callable(mod.main) and mod.OUT.endswith(FILE)
    assert mod.REQUIRED == REQUIRED and (mod.WELL, mod.FACTOR, mod.MARGIN) == (WELL, FACTOR, MARGIN)
    assert mod.LABELS == LABELS and mod.UNOBSERVABLE == UNOBSERVABLE
    assert set(mod.MUTANTS) == set(REQUIRED) and set(mod.SENSITIVE) == set(LABELS)
    assert set(mod.EQUIVALENT) <= set(e[0] for e in mod.ARITH) and mod.EOS == EOS


def check_conditions(g, path, tables, labels, required, unobservable, per_table=None):
    """items 1..6 of make_edac_pair_golden.py's docstring, from the stored data of a file of that layout"""
    assert os.path.getsize(path) < 1024 * 1024
    assert json.loads(str(g['tables'])) == tables
    assert tuple(json.loads(str(g['meta/required']))) == required
    assert tuple(json.loads(str(g['meta/unobservable']))) == unobservable
    assert tuple(g['meta/constants']) == (WELL, FACTOR, MARGIN)
    taken = dict((b, 0) for b in required)
    ks = k_eq(g)
    assert set(ks) == set(labels)
    for label in labels:
        bad = total = 0
        best = 0.0
        for key in tables:
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
            if per_table:
                per_table(key, sp)
        assert total > 0 and bad * 10 <= total, (label, bad, total)               # item 4
        assert best == ks[label] and best <= WELL, (label, best, ks[label])         # item 5
    short = dict((b, n) for b, n in taken.items() if n < 2)
    assert not short, short                                                       # item 1
    observed = json.loads(str(g['meta/observed']))
    assert all(observed[b] >= 2 for b in required if b not in unobservable), observed     # item 3
    sensitive = json.loads(str(g['meta/sensitive']))
    assert all(sensitive[e] >= 1 for e in labels), sensitive                      # item 6


def test_the_conditions_asserted_on_the_reference_are_in_the_file():
    g = fixture()

    def per_table(key, sp):
        for a in sp['arrays']:                                              # V is an input near rho / m
            cols = inputs(g, key, a)
            if 'V' in cols:
                assert np.all(np.abs(cols['V'] * cols['m'] / cols['rho'] - 1.0) <= 0.1 + 1e-12), key
        eqs = tuple(e['name'] for e in sp['group'])
        by = dict((e['name'], e['sources']) for e in sp['group'])
        # the default force group is the constant flag set; the other two groups are not
        if sp['label'] == 'fused_density':
            assert eqs == ('SummationDensity',) and sp['outputs'] == ['rho', 'V'] and np.unique(inputs(g, key, 'fluid')['m']).size == 1
        if sp['label'] == 'fused_force':        # the state the first two groups leave: the density table's double rho and V, p of that rho
            cols, dk = inputs(g, key, 'fluid'), key.replace('fused_force/default', 'fused_density/alone')
            assert eqs == CF0 and np.array_equal(cols['rho'], column(g, dk, 'ref', 'rho')) and np.array_equal(cols['V'], column(g, dk, 'ref', 'V'))
            assert np.array_equal(cols['p'], EOS['p0'] * (cols['rho'] / EOS['rho0'] - EOS['b'])) and np.all(cols['p'] > 0)
            assert all(np.array_equal(cols[c], inputs(g, dk, 'fluid')[c]) for c in ('x', 'y', 'z', 'h', 'm'))
        if sp['label'] == 'default_group':
            assert eqs == CF0 and sp['sources'] == ['fluid']
        if sp['label'] == 'av_group':
            assert set(eqs) == set(CF0) | set([_AV]) and sp['sources'] == ['fluid']
        if sp['label'] == 'solid_group':
            assert by[_PG] == ['fluid', 'solid'] and by[_AV] == ['fluid', 'solid'] and by[_VISC] == ['fluid'] and by[_AS] == ['fluid']
        if sp['label'] in (_VISC, _AV, _AS):
            assert eqs == (sp['label'],)
        if sp['label'] == _PG:
            assert eqs == (_PG,)

    check_conditions(g, os.path.join(GOLDEN, FILE), TABLES, LABELS, REQUIRED, UNOBSERVABLE, per_table)


def check_stored_k(g, tables):
    for key in tables:
        for c in spec_of(g, key)['outputs']:
            k = measure(column(g, key, 'ref', c), column(g, key, 'mp', c), column(g, key, 'mplo', c), column(g, key, 'S', c))
            kref = column(g, key, 'kref', c)
            assert np.array_equal(np.isinf(k), np.isinf(kref)), (key, c)
            fin = np.isfinite(k)
            # (kref and S are float32; mplo has a 24-bit mantissa: 2^-24 of a remainder of at most u |value|)
            assert np.allclose(k[fin], kref[fin], rtol=1e-6, atol=1e-6), (key, c)


def test_the_stored_reference_is_within_its_own_k_of_the_50_digit_values():
    """ref, mp + mplo, S and kref of the file agree: K recomputed in mpmath equals the stored float32 figure"""
    check_stored_k(fixture(), TABLES)


def damp_of(sp):
    """the factor on g as the reference's post_loop writes it, in double"""
    import math
    td = [e for e in sp['group'] if e['name'] == _PG][0]['params']['tdamp']
    return 0.5 * (math.sin((-0.5 + sp['t'] / td) * math.pi) + 1.0) if sp['t'] < td else 1.0


def test_exact_elements_of_the_file():
    """what the GPU test compares exactly is exact in the file"""
    g = fixture()
    seen = dict(lone=0, pb_zero=0, no_gradient=0)
    for key in TABLES:
        sp = spec_of(g, key)
        for c in sp['outputs']:
            S, ref = column(g, key, 'S', c), column(g, key, 'ref', c)
            exact = S == 0
            assert np.array_equal(ref[exact], column(g, key, 'mp', c)[exact]) and np.all(column(g, key, 'mplo', c)[exact] == 0), (key, c)
        cl = np.array(sp['cl'][sp['dest']])
        members = sum(np.bincount(np.array(v), minlength=cl.max() + 1) for v in sp['cl'].values())
        for i, nm in enumerate(sp['names']):
            if 'lone_particle' in nm:
                par = [e for e in sp['group'] if e['name'] == _PG][0]['params']
                for c, gk in zip(('au', 'av', 'aw'), ('gx', 'gy', 'gz')):
                    assert column(g, key, 'ref', c)[i] == par[gk] * damp_of(sp), (key, i, c)
                assert all(column(g, key, w, c)[i] == 0 for w in ('ref', 'S') for c in ('auhat', 'avhat', 'awhat'))
                seen['lone'] += 1
            if 'pb_zero' in nm:
                assert all(column(g, key, w, c)[i] == 0 for w in ('ref', 'S') for c in ('auhat', 'avhat', 'awhat'))
                seen['pb_zero'] += 1
            if ('rij_below_1e-12' in nm or 'coincident_unequal_h' in nm) and members[cl[i]] == 2 and sp['label'] in (_VISC, _AV, _AS):
                assert all(column(g, key, w, c)[i] == 0 for w in ('ref', 'S') for c in ('au', 'av', 'aw'))     # every term carries DWIJ
                seen['no_gradient'] += 1
    assert min(seen.values()) >= 2, seen


def check_host_accepts(g, tables, build_arrays, group_of):
    """every table's arrays carry what its group reads and writes: the host layer takes the group as it stands"""
    from pysph_amd import kernels as K
    from pysph_amd.acceleration_eval import AccelerationEval
    for key in tables:
        sp = spec_of(g, key)
        AccelerationEval(build_arrays(g, key), group_of(sp), getattr(K, sp['kernel'])(dim=sp['dim']))


def test_the_host_layer_accepts_every_table():
    check_host_accepts(fixture(), TABLES, build_arrays, group_of)


# ---------------------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------------------
def fill(arrays, g, key):
    """the stored columns pushed as they are, every other float column (the outputs, and what the group neither reads
    nor writes) garbage"""
    rng = np.random.default_rng(len(key))
    for pa in arrays:
        stored = inputs(g, key, pa.name)
        for c in pa.properties:
            if pa.properties[c].dtype != np.float64:
                continue
            if c in stored:
                pa.properties[c][:] = stored[c]
            else:
                pa.properties[c][:] = rng.uniform(-7.0, 7.0, pa.properties[c].size)


def build_arrays(g, key):
    """the table's arrays as the TVF factories make them (utils.py: get_particle_array_tvf_fluid / _solid)"""
    from pysph_amd.particle_array import get_particle_array_tvf_fluid, get_particle_array_tvf_solid
    sp = spec_of(g, key)
    arrays = [(get_particle_array_tvf_fluid if name == 'fluid' else get_particle_array_tvf_solid)(
        name=name, **dict((c, v.copy()) for c, v in inputs(g, key, name).items())) for name in sp['arrays']]
    fill(arrays, g, key)
    return arrays


def group_of(sp):
    from pysph_amd import equations as EQ
    from pysph_amd.equations import Group
    names = {'SummationDensity': 'TVFSummationDensity'}        # (transport_velocity.py's class of that name)
    return [Group(equations=[getattr(EQ, names.get(e['name'], e['name']))(dest=sp['dest'], sources=list(e['sources']), **e['params'])
                             for e in sp['group']])]


def check_neighbours(nnps, arrays, sp, key):
    """the neighbour lists are the clusters, nothing leaks across"""
    names = [pa.name for pa in arrays]
    for sn in sp['sources']:
        start, idx = nnps.get_csr(names.index(sn), names.index(sp['dest']))
        want = sp['nbr'][sn]
        assert np.array_equal(start, np.cumsum([0] + [len(v) for v in want])), (key, sn)
        got = [sorted(int(j) for j in idx[start[i]:start[i + 1]]) for i in range(len(want))]
        assert got == want, (key, sn)


def judge(g, key, dest, what):
    """every output column of the destination against the file: the NaN pattern, scale-0 elements exact, every element
    whose 50-digit run took the double run's path within its bound.  Returns (worst K over the well-conditioned
    elements, where, the flat bound, worst fraction of their own bound of the others)"""
    sp = spec_of(g, key)
    bnd = bounds(g, key)
    mpok = np.array(sp['mpok'], bool)
    worst, where, ill = 0.0, None, 0.0
    for c in sp['outputs']:
        got, ref = dest.properties[c], column(g, key, 'ref', c)
        assert np.array_equal(np.isnan(got), np.isnan(ref)), (key, c, what, 'NaN pattern')
        S = column(g, key, 'S', c)
        k = measure(got, column(g, key, 'mp', c), column(g, key, 'mplo', c), S)
        exact = (S == 0)
        assert np.all(k[exact] == 0), (key, c, what, 'an element of scale 0 is not exact', np.nonzero(exact & (k != 0))[0][:4],
                                       got[exact & (k != 0)][:4], ref[exact & (k != 0)][:4])
        bound, well = bnd[c]
        if np.any(well) and k[well].max() > worst:
            worst, where = float(k[well].max()), (c, int(np.argmax(np.where(well, k, -1.0))))
        rest = mpok & ~well
        with np.errstate(invalid='ignore', divide='ignore'):
            ill = max(ill, float(np.max((k / bound)[rest & (k > 0)], initial=0.0)))
        bad = np.nonzero(mpok & ~(k <= bound))[0]       # (a row whose 50-digit run took another path is not compared)
        assert bad.size == 0, (key, c, what, [(int(i), float(k[i]), float(bound[i]), float(got[i]), float(ref[i])) for i in bad[:4]])
    flat = max(FACTOR, FACTOR * k_eq(g)[sp['label']])
    print('%s %s: device K %.3f at %s (bound %.1f); ill-conditioned elements at most %.3f of their own bound'
          % (key, what, worst, where, flat, ill))
    return worst, where, flat, ill


def run_table(g, key, variant, build_arrays, group_of, family, exact_checks=None):
    """one launch of one group over one table against the file"""
    from pysph_amd import kernels as K
    from test_gsph_gpu import evaluator, pull_all, _floats
    sp = spec_of(g, key)
    arrays = build_arrays(g, key)
    by_name = dict((pa.name, pa) for pa in arrays)
    before = dict(((pa.name, c), pa.properties[c].copy()) for pa in arrays for c in _floats(pa))
    a_eval, nnps, ctx = evaluator(arrays, group_of(sp), getattr(K, sp['kernel'])(dim=sp['dim']), variant)
    ctx.lib.sph_timer_enable(ctx._h, 1)
    nnps.update()
    check_neighbours(nnps, arrays, sp, key)
    a_eval.compute(sp['t'], 0.0)
    launches = dict((k, ctx.timer_get(k)[1]) for k in FAMILIES)
    pull_all(arrays)
    ctx.close()
    assert launches[family] == 1 and sum(launches.values()) == 1, (key, launches)      # the family under test, nothing else
    for (name, c), v in before.items():
        if not (name == sp['dest'] and c in sp['outputs']):
            assert np.array_equal(by_name[name].properties[c], v, equal_nan=True), (key, name, c, 'a column the group does not write changed')
    if exact_checks:
        exact_checks(g, key, by_name[sp['dest']])
    return judge(g, key, by_name[sp['dest']], 'variant %d' % variant)


def exact_checks(g, key, dest):
    sp = spec_of(g, key)
    for i, nm in enumerate(sp['names']):
        if 'lone_particle' in nm and damp_of(sp) == 1.0:        # (on the ramp the sine is the device's: held to the bound)
            par = [e for e in sp['group'] if e['name'] == _PG][0]['params']
            for c, gk in zip(('au', 'av', 'aw'), ('gx', 'gy', 'gz')):
                assert dest.properties[c][i] == par[gk], (key, i, c, 'a lone particle: g')
        if 'lone_particle' in nm or 'pb_zero' in nm:
            assert all(dest.properties[c][i] == 0.0 for c in ('auhat', 'avhat', 'awhat')), (key, i)


@pytest.mark.gpu
@pytest.mark.parametrize('variant', [6, 0])
@pytest.mark.parametrize('key', TABLES)
def test_every_cluster_of_the_table(key, variant):
    """one group over one table, both schedules: every output element within its bound of the 50-digit value, scale-0
    elements exact, the family that ran, the NaN pattern, the neighbour lists, every other column bit for bit"""
    run_table(fixture(), key, variant, build_arrays, group_of, 'pair_density' if key.startswith('fused_density') else 'pair_tvf', exact_checks)


def fused_groups(sp):
    from pysph_amd import equations as EQ
    from pysph_amd.equations import Group
    return [Group(equations=[EQ.TVFSummationDensity(dest='fluid', sources=['fluid'])], real=False),
            Group(equations=[EQ.StateEquation(dest='fluid', sources=None, **EOS)], real=False)] + group_of(sp)


def fused_arrays(g, key):
    """the force table's array with garbage where rho, V and p are: the device computes them"""
    arrays = build_arrays(g, key)
    rng = np.random.default_rng(13)
    for c in ('rho', 'V', 'p'):
        arrays[0].properties[c][:] = rng.uniform(0.5, 7.0, arrays[0].properties[c].size)
    return arrays


FUSED_FORCE = [k for k in TABLES if k.startswith('fused_force')]


def test_the_host_layer_accepts_the_three_groups():
    check_host_accepts(fixture(), FUSED_FORCE, fused_arrays, fused_groups)


@pytest.mark.gpu
@pytest.mark.parametrize('key', FUSED_FORCE)
def test_records_without_p_and_v(key):
    """[SummationDensity | StateEquation | force group] with mass_fuse on and off in one context (the docstring)"""
    from pysph_amd import kernels as K
    from test_gsph_gpu import evaluator, pull_all, _floats
    g = fixture()
    sp = spec_of(g, key)
    dkey = key.replace('fused_force/default', 'fused_density/alone')
    outs = sp['outputs']
    arrays = fused_arrays(g, key)
    dest = arrays[0]
    stored = inputs(g, key, 'fluid')
    before = dict((c, dest.properties[c].copy()) for c in _floats(dest))
    a_eval, nnps, ctx = evaluator(arrays, fused_groups(sp), getattr(K, sp['kernel'])(dim=sp['dim']), 6)
    ctx.lib.sph_timer_enable(ctx._h, 1)
    rng = np.random.default_rng(7)

    def evaluate(what):
        for c in outs + ['rho', 'V', 'p']:            # every evaluation has to write all of them again
            dest.properties[c][:] = rng.uniform(0.5, 7.0, dest.properties[c].size)
        dest.gpu.push(*(outs + ['rho', 'V', 'p']))
        nnps.update()
        a_eval.compute(sp['t'], 0.0)
        pull_all(arrays)
        judge(g, dkey, dest, what)                      # rho and V against the density table, with its bound
        rho, p = dest.properties['rho'], dest.properties['p']
        flat = max(FACTOR, FACTOR * k_eq(g)['fused_density'])
        sp_ = EOS['p0'] / EOS['rho0'] * flat * column(g, dkey, 'S', 'rho') + 4.0 * (np.abs(EOS['p0'] * rho / EOS['rho0']) + abs(EOS['p0'] * EOS['b']))
        assert np.all(np.abs(p - stored['p']) <= 2.0 ** -53 * sp_), (key, what, 'p', np.max(np.abs(p - stored['p']) / (2.0 ** -53 * sp_)))
        return dict((c, dest.properties[c].copy()) for c in outs + ['rho', 'V', 'p', 'm'])

    evaluate('first evaluation')
    n0 = ctx.timer_get('n_eos_fused')[1]
    F = evaluate('mass_fuse on')
    n1 = ctx.timer_get('n_eos_fused')[1]
    ctx.set_option('mass_fuse', 0)
    U = evaluate('mass_fuse off')
    n2 = ctx.timer_get('n_eos_fused')[1]
    families = dict((k, ctx.timer_get(k)[1]) for k in FAMILIES)
    ctx.close()
    assert n1 > n0 and n2 == n1, (key, n0, n1, n2)
    assert families['pair_density'] == 3 and families['pair_tvf'] == 3 and sum(families.values()) == 6, (key, families)
    for c, v in before.items():
        if c not in outs + ['rho', 'V', 'p']:
            assert np.array_equal(dest.properties[c], v, equal_nan=True), (key, c, 'a column the groups do not write changed')
    # the first-order effect of the two swaps, per cluster, from what the unfused run left
    eV = np.abs((U['m'] / U['rho']) ** 2 * U['V'] ** 2 - 1.0)
    eP = np.abs(EOS['p0'] * (U['rho'] / EOS['rho0'] - EOS['b']) - U['p']) / np.abs(U['p'])
    cl = np.array(sp['cl']['fluid'])
    eps = np.array([np.max((eV + eP)[cl == c]) for c in cl])
    flat = max(FACTOR, FACTOR * k_eq(g)['fused_force'])
    worst = 0.0
    for c in outs:
        S = column(g, key, 'S', c)
        tol = (flat * 2.0 ** -53 + eps) * S
        d = np.abs(F[c] - U[c])
        assert np.all(d[S == 0] == 0), (key, c, 'an element of scale 0 differs')
        worst = max(worst, float(np.max(d[S > 0] / (2.0 ** -53 * S[S > 0]), initial=0.0)))
        assert np.all(d <= tol), (key, c, np.nonzero(d > tol)[0][:4], (d / np.where(tol > 0, tol, 1.0)).max())
    print('%s: fused against unfused at most %.3f u S (bound %.1f u S + swap effect, eV + eP at most %.3g u)'
          % (key, worst, flat, float(eps.max()) * 2.0 ** 53))
