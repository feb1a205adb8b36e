"""The solid-mechanics pair families (``FamVGrad_T``, ``FamElastic_T`` and, on device-resident state with one mass per
array, ``FamElasticU_T``; pysph_amd/csrc/sph_fam_elastic.h), one isolated cluster at a time, against the reference's own
classes evaluated at 50 digits (tests/golden/elastic_pair_edges.npz, made by tests/golden/make_elastic_pair_golden.py with
the machinery of make_edac_pair_golden.py and make_gasd_pair_golden.py; the tests read nothing but that file).

Every table is a row of one lone particle (the self pair only: every rate exactly 0, ax ay az = u v w), isolated pairs
and triples, 1 apart, and runs ONE GROUP, the smallest the product takes into
the family.  The product takes a group into the elastic family only where MomentumEquationWithStress or
MonaghanArtificialViscosity is in it (ContinuityEquation or XSPHCorrection alone are the WCSPH family's), so:
VelocityGradient2D alone in the 2-D configuration (z = 3/8 everywhere, w garbage; v02 v12 v20 v21 v22 must come back bit
for bit), VelocityGradient3D alone in both 3-D configurations, ContinuityEquation next to the stress equation,
MomentumEquationWithStress alone with wdeltap > 0 and n = 4, 2, 1 (the three multiplied forms), 3 and 2.5 (``pow``) and
with wdeltap = 0, MonaghanArtificialViscosity (beta != 0 and beta = 0) and XSPHCorrection (eps = 1/2 and 0: F_EXSPH
without F_EAV, the run-time-flag kernel and its ``rhoij1 = fast_rcp(rhoij)``) next to the stress equation with wdeltap = -1
(the default of get_particle_array_elastic_dynamics), and the full ``FamElastic_T::CF0`` group.  ``uh`` tables have every
h 2^-3 and one mass per array, ``vh`` tables h and m unequal inside the clusters; every table under pair_variant 6 and 0.
The launch counters are asserted: ``pair_vgrad`` or ``pair_elastic`` is 1, every other family 0.

Bound.  That of tests/test_edac_pair_edges.py (scale S per element, errors in units of u S, u = 2^-53, K_ref, K_eq per
label, max(4, 4 K_eq) u S on a well-conditioned element and 4 K_ref of the element itself on any other, scale 0 exact,
the NaN pattern, every column the group does not write bit for bit, the neighbour lists; (WELL, FACTOR, MARGIN) =
(64, 4, 1e-3)) with ONE exception, MomentumEquationWithStress: the kernel keeps S = sum m_j DWIJ and
F = sum m_j f^n DWIJ and adds the destination's own t_i . S + r_i . F in finish(), on purpose and documented in the
header, so the scale of au av aw is the sum of the absolute values of the individual PRODUCTS of the reference's
statement (for au the nine pieces |mb s0ka rhoa21 DWIJ[k]|, |mb s0kb rhob21 DWIJ[k]|, |mb art_stress0k DWIJ[k]|), not of
the statement's net increment.  The clusters ``stress_opposed`` (sigma_a / rho_a^2 = -sigma_b / rho_b^2 to the last bit:
the reference's increment is the artificial-stress term alone, exactly 0 without it) and ``gradient_sum_zero`` (a
symmetric triple: sum m_j DWIJ of the middle particle is exactly 0 while its own stress is not) are in every table with
the stress equation and are judged like every other cluster.  ax ay az under eps = 0 equal u v w exactly.

The records without h and m (``FamElasticU_T``) engage only on device-resident state once a neighbour update has seen
one mass per array: ``test_records_without_h_and_m`` evaluates every ``uh`` table of the elastic family a second time
in the same context behind a second neighbour update, asserts that ``n_mass_fused`` grew and judges the second
evaluation against the same stored values with the same bound (nothing is recomputed: the file's reference is the
reference), once as it stands and once under the option ``row_lds`` (``k_pair_rowlds``: ``n_row_lds`` grows).

The tension token.  ``MonaghanArtificialStress`` (a no-source equation, judged in tests/test_nosrc_edges.py) ahead of
the rates tells the records without h and m whether any r_ij of the source is not 0; where none is, the kernel does not
gather them.  tests/golden/elastic_tension_pair_edges.npz (the same generator) holds ``uh`` tables of the CF0 group whose
states make r_ij exact on both sides: diagonal dyadic stresses, dyadic p, eps = 1/4, rho 1 or 2 and sum |s_kk - p| a
power of two (the device scales the tensor by that sum), so r_kk = -eps (s_kk - p) / rho^2 where s_kk - p > 0 and 0
elsewhere.  ``compressive`` tables have every principal stress negative (r = 0 everywhere); ``tensile`` tables add ONE
cluster in tension.  ``test_tension_token`` pushes garbage r, runs [MonaghanArtificialStress | rates] twice in one context
(the second time on the records without h and m) under ``tension_flag`` 1 and 0: the device's r columns equal the stored
ones bit for bit, ``n_tension_flag`` grows under 1 and stays 0 under 0, the rates of the second evaluation are within
the bound of the stored values, and the two settings give the same rates bit for bit.

Measured on an MI355X: DESIGN.md, section 7j ("Pair by pair").

Mutants.  Each of the following changes was made to the text of the reference's method in memory and run in double over
the stored inputs on the CPU (``make_elastic_pair_golden.py --mutants``); "caught" = the result leaves the bound of this
file (or the mutant raises where the reference does not: wdeltap >= 0 divides by wdeltap = 0); the figure is the number of
stored destinations that leave it.  No mutant was built for or run on the GPU.
    pow(fab, n) with n + 1                                             caught (1120)
    pow(fab, n) with n - 1                                             caught (1120)
    fab applied to r_a only                                            caught (1120)
    s11a - pa without the pressure                                     caught (1884)
    rhob21 replaced by rhoa21                                          caught (2608)
    s12 where s02 belongs (source side of au)                          caught (1301)
    s12 where s02 belongs (destination side of aw)                     caught (2510)
    wdeltap > 0 changed to >= 0                                        caught (360)
    beta dropped                                                       caught (265)
    cij without the 0.5                                                caught (399)
    rhoij without the 0.5, so RHOIJ1 halved (artificial viscosity)     caught (399)
    rhoij without the 0.5, so RHOIJ1 halved (XSPH)                     caught (624)
    vijdotxij < 0 changed to <= 0                                      NOT caught
    XSPH: u not added behind the loop                                  caught (872)
    continuity: m_j replaced by m_j / rho_j                            caught (560)
    VelocityGradient2D: -VIJ with the sign dropped                     caught (50)
    VelocityGradient3D: -VIJ with the sign dropped                     caught (100)
    VelocityGradient2D: DWIJ[j] and DWIJ[i] swapped                    caught (30)
    VelocityGradient3D: DWIJ[j] and DWIJ[i] swapped                    caught (60)
The one that is not caught is an equivalent mutant: with vijdotxij = 0 muij is 0 and the pair adds zeros on either side.
"""
import os

import numpy as np
import pytest

from conftest import load_golden
from test_edac_pair_edges import spec_of, column, inputs
import test_tvf_pair_edges as TT

WELL, FACTOR, MARGIN = 64.0, 4.0, 1e-3
_VG2, _VG3, _CONT, _ST, _MAV, _XS = ('VelocityGradient2D', 'VelocityGradient3D', 'ContinuityEquation', 'MomentumEquationWithStress',
                                     'MonaghanArtificialViscosity', 'XSPHCorrection')
LABELS = (_VG2, _VG3, _CONT, _ST, _MAV, _XS, 'cf0_group')
REQUIRED = ('wdeltap_positive', 'wdeltap_negative', 'wdeltap_zero', 'n_1', 'n_2', 'n_4', 'n_3', 'n_2.5', 'wij_zero',
            'approaching', 'receding', 'beta_zero', 'beta_nonzero', 'eps_zero', 'stress_opposed', 'gradient_sum_zero',
            'r_zero', 'r_nonzero', 'rij_below_1e-12', 'rij_above_1e-12', 'coincident_unequal_h', 'lone_particle')
UNOBSERVABLE = ()
CONFIGS = (('1d_cubic', 1), ('2d_wendland', 2), ('3d_quintic', 3), ('3d_gauss', 3))


def kinds(ci, dim):
    """(label, kind) of one configuration, in the generator's order"""
    out = [(_VG2, 'alone')] if dim == 2 else [(_VG3, 'alone')] if dim == 3 else []
    out += [(_CONT, 'stress'), (_ST, 'n4')] + [(_ST, k) for k in (('n2', 'n3') if ci % 2 == 0 else ('n1', 'n2.5'))]
    return out + [(_ST, 'wzero'), (_MAV, 'beta'), (_MAV, 'beta0'), (_XS, 'stress'), (_XS, 'eps0'), ('cf0_group', 'rates')]


TABLES = ['%s/%s/%s/%s' % (label, kind, c, f) for ci, (c, dim) in enumerate(CONFIGS) for f in ('uh', 'vh') for label, kind in kinds(ci, dim)]
UH_ELASTIC = [k for k in TABLES if k.endswith('/uh') and not k.startswith('VelocityGradient')]
CF0 = (_CONT, _ST, _MAV, _XS)
_R6 = ('r00', 'r01', 'r02', 'r11', 'r12', 'r22')
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FILE = 'elastic_pair_edges.npz'
FILE_TENSION = 'elastic_tension_pair_edges.npz'
EPS_STRESS = 0.25
TENSION_TABLES = ['tension/%s/%s/uh' % (k, c) for c, dim in CONFIGS for k in ('compressive', 'tensile')]
REQUIRED_TENSION = ('wdeltap_positive', 'n_4', 'approaching', 'receding', 'beta_nonzero', 'r_zero', 'r_nonzero', 'lone_particle')

_G = []


def fixture():
    if not _G:
        _G.append(load_golden(FILE))
    return _G[0]


_GT = []


def tension_fixture():
    if not _GT:
        _GT.append(load_golden(FILE_TENSION))
    return _GT[0]


# ---------------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------------
def test_golden_generator_imports_cleanly():
    if not os.path.isdir('/root/reference'):
        pytest.skip('the generator needs the reference (build container only)')
    mod = TT.load_generator('make_elastic_pair_golden')
    assert callable(mod.main) and mod.OUT.endswith(FILE)
    assert mod.REQUIRED == REQUIRED and (mod.WELL, mod.FACTOR, mod.MARGIN) == (WELL, FACTOR, MARGIN)
    assert mod.LABELS == LABELS and mod.UNOBSERVABLE == UNOBSERVABLE
    assert set(mod.MUTANTS) == set(REQUIRED) and set(mod.SENSITIVE) == set(LABELS)
    assert set(mod.EQUIVALENT) <= set(e[0] for e in mod.ARITH)
    assert mod.OUT_TENSION.endswith(FILE_TENSION) and mod.EPS_STRESS == EPS_STRESS and mod.Tension.REQUIRED == REQUIRED_TENSION


def test_the_conditions_asserted_on_the_reference_are_in_the_file():
    g = fixture()
    seen = dict(n=set(), wdeltap=set())

    def per_table(key, sp):
        eqs = tuple(e['name'] for e in sp['group'])
        assert sp['sources'] == ['fluid'] and sp['arrays'] == ['fluid']
        if sp['label'] == 'cf0_group':
            assert eqs == CF0
        if sp['label'] in (_VG2, _VG3):
            assert eqs == (sp['label'],)
        if sp['label'] == _VG2:               # z is not 0 and w is garbage: neither may reach v00 .. v11
            cols = inputs(g, key, 'fluid')
            assert sp['dim'] == 2 and np.all(cols['z'] == 0.375) and np.all(cols['w'] != 0.0)
            assert sp['outputs'] == ['v00', 'v01', 'v10', 'v11']
        if sp['label'] == _ST:
            assert eqs == (_ST,)
        if sp['label'] in (_CONT, _MAV, _XS):
            assert eqs in ((_CONT, _ST), (_ST, sp['label']))
        for e in sp['group']:
            if e['name'] == _ST:
                seen['wdeltap'].add(np.sign(e['params']['wdeltap']))
                if e['params']['wdeltap'] > 0:
                    seen['n'].add(e['params']['n'])
        if sp['form'] == 'uh':                # one mass per array: what the records without h and m need
            assert np.unique(inputs(g, key, 'fluid')['m']).size == 1, key

    TT.check_conditions(g, os.path.join(GOLDEN, FILE), TABLES, LABELS, REQUIRED, UNOBSERVABLE, per_table)
    assert seen['n'] == set([1.0, 2.0, 4.0, 3.0, 2.5]) and seen['wdeltap'] == set([-1.0, 0.0, 1.0]), seen


def test_the_stored_reference_is_within_its_own_k_of_the_50_digit_values():
    """ref, mp + mplo, S and kref of the file agree: K recomputed in mpmath equals the stored float32 figure"""
    TT.check_stored_k(fixture(), TABLES)


def test_exact_elements_of_the_file():
    """what the GPU test compares exactly is exact in the file; the built clusters are what their names say"""
    g = fixture()
    seen = dict(eps_zero=0, opposed_zero=0, no_gradient=0, r_zero=0, lone=0)
    for key in TABLES:
        sp = spec_of(g, key)
        D = inputs(g, key, sp['dest'])
        for c in sp['outputs']:
            S, ref = column(g, key, 'S', c), column(g, key, 'ref', c)
            exact = S == 0
            assert np.array_equal(ref[exact], column(g, key, 'mp', c)[exact]) and np.all(column(g, key, 'mplo', c)[exact] == 0), (key, c)
        cl = np.array(sp['cl'][sp['dest']])
        members = np.bincount(cl)
        st = [e for e in sp['group'] if e['name'] == _ST]
        for i, nm in enumerate(sp['names']):
            if 'eps_zero' in nm:
                assert all(column(g, key, 'ref', 'a' + x)[i] == D[u][i] for x, u in zip('xyz', 'uvw'))
                seen['eps_zero'] += 1
            if 'stress_opposed' in nm and st[0]['params']['wdeltap'] <= 0 and sp['label'] in (_ST, _CONT):
                # the reference's increment is exactly 0 there, at a scale that is not
                assert all(column(g, key, 'ref', c)[i] == 0 and column(g, key, 'S', c)[i] > 0 for c in ('au', 'av', 'aw'))
                seen['opposed_zero'] += 1
            if 'lone_particle' in nm:
                assert members[cl[i]] == 1
                for c in sp['outputs']:
                    want = D['uvw'['xyz'.index(c[1])]][i] if c in ('ax', 'ay', 'az') else 0.0
                    assert column(g, key, 'ref', c)[i] == want and (column(g, key, 'S', c)[i] == 0) == (want == 0), (key, c)
                seen['lone'] += 1
            if 'r_zero' in nm:
                assert all(np.all(D[c][cl == cl[i]] == 0) for c in _R6)
                seen['r_zero'] += 1
            if ('rij_below_1e-12' in nm or 'coincident_unequal_h' in nm) and members[cl[i]] == 2 and sp['label'] in (_ST, _VG3, _VG2):
                assert all(column(g, key, w, c)[i] == 0 for w in ('ref', 'S') for c in sp['outputs'])     # every term carries DWIJ
                seen['no_gradient'] += 1
    assert min(seen.values()) >= 2, seen


def build_arrays(g, key):
    """the table's array as get_particle_array_elastic_dynamics makes it, wdeltap and n its constants"""
    from pysph_amd.solid_mech import get_particle_array_elastic_dynamics
    sp = spec_of(g, key)
    st = [e for e in sp['group'] if e['name'] == _ST]
    consts = dict(wdeltap=st[0]['params']['wdeltap'], n=st[0]['params']['n']) if st else None
    arrays = [get_particle_array_elastic_dynamics(constants=consts, name=name, **dict((c, v.copy()) for c, v in inputs(g, key, name).items()))
              for name in sp['arrays']]
    TT.fill(arrays, g, key)
    return arrays


def group_of(sp):
    from pysph_amd import equations as EQ, solid_mech as SM
    from pysph_amd.equations import Group
    eqs = []
    for e in sp['group']:
        cls = getattr(SM, e['name'], None) or getattr(EQ, e['name'])
        par = {} if e['name'] == _ST else e['params']          # (wdeltap and n are constants of the array)
        eqs.append(cls(dest=sp['dest'], sources=list(e['sources']), **par))
    return [Group(equations=eqs)]


def test_the_host_layer_accepts_every_table():
    TT.check_host_accepts(fixture(), TABLES, build_arrays, group_of)


# ---------------------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------------------
def family_of(key):
    return 'pair_vgrad' if key.startswith('VelocityGradient') else 'pair_elastic'


def exact_checks(g, key, dest):
    sp = spec_of(g, key)
    D = inputs(g, key, sp['dest'])
    for i, nm in enumerate(sp['names']):
        if ('eps_zero' in nm or 'lone_particle' in nm) and 'ax' in sp['outputs']:
            assert all(dest.properties['a' + x][i] == D[u][i] for x, u in zip('xyz', 'uvw')), (key, i)


@pytest.mark.gpu
@pytest.mark.parametrize('variant', [6, 0])
@pytest.mark.parametrize('key', TABLES)
def test_every_cluster_of_the_table(key, variant):
    """one group over one table, both schedules: every output element within its bound of the 50-digit value, scale-0
    elements exact, the family that ran, the NaN pattern, the neighbour lists, every other column bit for bit"""
    TT.run_table(fixture(), key, variant, build_arrays, group_of, family_of(key), exact_checks)


@pytest.mark.gpu
@pytest.mark.parametrize('row_lds', [0, 1])
@pytest.mark.parametrize('key', UH_ELASTIC)
def test_records_without_h_and_m(key, row_lds):
    """a second neighbour update and a second evaluation in the same context: the 160-byte records of FamElasticU_T
    (``n_mass_fused`` grows), judged against the same stored values with the same bound; under the option ``row_lds``
    the same records from the LDS copy of a row tile (``k_pair_rowlds``: ``n_row_lds`` grows)"""
    from pysph_amd import kernels as K
    from test_gsph_gpu import evaluator, pull_all, _floats
    g = fixture()
    sp = spec_of(g, key)
    arrays = build_arrays(g, key)
    dest = arrays[0]
    before = dict((c, dest.properties[c].copy()) for c in _floats(dest))
    a_eval, nnps, ctx = evaluator(arrays, group_of(sp), getattr(K, sp['kernel'])(dim=sp['dim']), 6)
    ctx.set_option('row_lds', row_lds)
    ctx.lib.sph_timer_enable(ctx._h, 1)
    nnps.update()
    a_eval.compute(sp['t'], 0.0)
    first = ctx.timer_get('n_mass_fused')[1]
    pull_all(arrays)
    TT.judge(g, key, dest, 'first evaluation')
    rng = np.random.default_rng(7)
    for c in sp['outputs']:                 # the second evaluation has to write every output again
        dest.properties[c][:] = rng.uniform(-7.0, 7.0, dest.properties[c].size)
    dest.gpu.push(*sp['outputs'])
    nnps.update()
    a_eval.compute(sp['t'], 0.0)
    second = ctx.timer_get('n_mass_fused')[1]
    launches, rowlds = ctx.timer_get('pair_elastic')[1], ctx.timer_get('n_row_lds')[1]
    families = dict((k, ctx.timer_get(k)[1]) for k in TT.FAMILIES)
    pull_all(arrays)
    ctx.close()
    assert first == 0 and second > first and launches == 2, (key, first, second, launches)
    assert sum(families.values()) == 2, (key, families)          # both evaluations the elastic family's, nothing else ran
    assert (rowlds > 0) == bool(row_lds), (key, row_lds, rowlds)
    for c, v in before.items():
        if c not in sp['outputs']:
            assert np.array_equal(dest.properties[c], v, equal_nan=True), (key, c, 'a column the group does not write changed')
    exact_checks(g, key, dest)
    TT.judge(g, key, dest, 'records without h and m' + (', row_lds' if row_lds else ''))


# ---------------------------------------------------------------------------------------------------------------------
# the tension token
# ---------------------------------------------------------------------------------------------------------------------
def test_the_tension_file_holds_its_conditions():
    """items 1..6 on the second file; its states are what the docstring says, its stored r the closed form"""
    g = tension_fixture()

    def per_table(key, sp):
        assert tuple(e['name'] for e in sp['group']) == CF0 and sp['form'] == 'uh'
        D = inputs(g, key, 'fluid')
        assert np.unique(D['m']).size == 1
        assert all(np.all(D[c] == 0) for c in ('s01', 's02', 's12', 'r01', 'r02', 'r12'))
        sig = np.array([D[c] - D['p'] for c in ('s00', 's11', 's22')])
        total = np.abs(sig).sum(axis=0)
        assert np.all(np.log2(total) == np.round(np.log2(total))) and np.all(np.isin(D['rho'], (1.0, 2.0)))
        want = np.where(sig > 0, -EPS_STRESS * sig * (1.0 / (D['rho'] * D['rho'])), 0.0)
        assert all(np.array_equal(D[c], w) for c, w in zip(('r00', 'r11', 'r22'), want))
        tense = np.any(sig > 0, axis=0)
        cl = np.array(sp['cl']['fluid'])
        assert (np.unique(cl[tense]).size == 1 and tense.sum() == 2) if '/tensile/' in key else not tense.any()

    TT.check_conditions(g, os.path.join(GOLDEN, FILE_TENSION), TENSION_TABLES, ('tension',), REQUIRED_TENSION, (), per_table)
    TT.check_stored_k(g, TENSION_TABLES)


def tension_groups(sp):
    from pysph_amd.solid_mech import MonaghanArtificialStress
    from pysph_amd.equations import Group
    return [Group(equations=[MonaghanArtificialStress(dest=sp['dest'], sources=None, eps=EPS_STRESS)])] + group_of(sp)


def tension_arrays(g, key):
    """the table's array with garbage where the stored r_ij are: the device computes them"""
    arrays = build_arrays(g, key)
    rng = np.random.default_rng(11)
    for c in _R6:
        arrays[0].properties[c][:] = rng.uniform(-7.0, 7.0, arrays[0].properties[c].size)
    return arrays


def test_the_host_layer_accepts_the_tension_tables():
    TT.check_host_accepts(tension_fixture(), TENSION_TABLES, tension_arrays, tension_groups)


def run_tension(g, key, tension_flag):
    from pysph_amd import kernels as K
    from test_gsph_gpu import evaluator, pull_all, _floats
    sp = spec_of(g, key)
    arrays = tension_arrays(g, key)
    dest = arrays[0]
    stored = inputs(g, key, 'fluid')
    before = dict((c, dest.properties[c].copy()) for c in _floats(dest))
    a_eval, nnps, ctx = evaluator(arrays, tension_groups(sp), getattr(K, sp['kernel'])(dim=sp['dim']), 6)
    ctx.set_option('tension_flag', tension_flag)
    ctx.lib.sph_timer_enable(ctx._h, 1)
    nnps.update()
    a_eval.compute(sp['t'], 0.0)
    rng = np.random.default_rng(7)
    for c in sp['outputs']:                 # the second evaluation has to write every output again
        dest.properties[c][:] = rng.uniform(-7.0, 7.0, dest.properties[c].size)
    dest.gpu.push(*sp['outputs'])
    nnps.update()
    a_eval.compute(sp['t'], 0.0)
    fused, token = ctx.timer_get('n_mass_fused')[1], ctx.timer_get('n_tension_flag')[1]
    families = dict((k, ctx.timer_get(k)[1]) for k in TT.FAMILIES)
    pull_all(arrays)
    ctx.close()
    assert fused > 0 and families['pair_elastic'] == 2 and sum(families.values()) == 2, (key, fused, families)
    assert (token > 0) == bool(tension_flag), (key, tension_flag, token)
    for c in _R6:                           # before the rates are judged: the device's r_ij are the stored ones, bit for bit
        assert np.array_equal(dest.properties[c], stored[c]), (key, c, dest.properties[c], stored[c])
    for c, v in before.items():
        if c not in sp['outputs'] and c not in _R6:
            assert np.array_equal(dest.properties[c], v, equal_nan=True), (key, c, 'a column the groups do not write changed')
    exact_checks(g, key, dest)
    TT.judge(g, key, dest, 'tension_flag %d' % tension_flag)
    return dict((c, dest.properties[c].copy()) for c in sp['outputs'])


@pytest.mark.gpu
@pytest.mark.parametrize('key', TENSION_TABLES)
def test_tension_token(key):
    """[MonaghanArtificialStress | rates] on the records without h and m, with the token and without it"""
    g = tension_fixture()
    on, off = run_tension(g, key, 1), run_tension(g, key, 0)
    for c in on:
        assert np.array_equal(on[c], off[c]), (key, c, 'the token changed a rate')
