"""The delta-SPH / laminar-viscosity rates and the delta-SPH pre-passes (``FamWCSPHX_T<T, DS>``, ``FamDSPre_T``,
pysph_amd/csrc/sph_fam_wcsph.h), one isolated cluster at a time, against the reference's own classes evaluated at 50 digits
(tests/golden/wcsph_options_pair_edges.npz, made by tests/golden/make_wcsph_options_pair_golden.py on the group sweep
of make_edac_pair_golden.py; the tests read nothing but that file).  Layout, scale and bound rule: those of
tests/test_edac_pair_edges.py -- a well-conditioned element (K_ref <= 64, the 50-digit run on the double run's lines,
the lines of gj_solve included) within max(4, 4 K_eq) u S of the 50-digit value, any other within 4 K_ref of itself, an
element of scale 0 exact, the NaN pattern, every other column bit for bit, the neighbour lists equal to the clusters.

Tables, each in four configurations (1-D CubicSpline, 2-D WendlandQuintic, 3-D QuinticSpline, 3-D Gaussian) and in a
``uh`` (every h equal) and a ``vh`` form, under pair_variant 6 and 0:
    GradientCorrectionPreStep/moment_n<k>   the moment pass alone, dim = k = 1, 2, 3 in every configuration: all nine components
                                            compared, those outside the k x k block and every pair at r <= 1e-12 exactly 0
    GradientCorrection/well_n<k>, built_n<k>  [GradientCorrection(dim = k, tol), ContinuityEquationDeltaSPHPreStep], k = 1, 2, 3
                                            in every configuration (also k above the kernel's dimension), with
                                            m_mat PUSHED AS AN INPUT: identity plus dyadic perturbations (tol = 1/4), and
                                            matrices built so that the elimination is exact and the pivot is the number
                                            written (tol = 2^50): M00 = 2^-41 / 2^-39, M11 = 2^-41 / 2^-39, 2^-41 under
                                            k = 1 (it divides), a last pivot of exactly 0 with that row's DWIJ exactly 0
                                            (a partner along an axis) and not (a partner off it).  The entries outside
                                            the k x k block are 1/2.
    ContinuityEquationDeltaSPHPreStep/alone, behind   the gradient pass without a correction, and with one BEHIND it, which
                                            corrects nothing: the same inputs, the same results bit for bit
    the rates                               ContinuityEquation + ContinuityEquationDeltaSPH; MomentumEquation (plain:
                                            alpha = beta = 0, no tensile correction, pressures of 2^-8) +
                                            MomentumEquationDeltaSPH, + LaminarViscosity, + LaminarViscosityDeltaSPH, + both
                                            delta terms; the rates group of WCSPHScheme(delta_sph=True, nu != 0) on the
                                            fluid alone and on fluid <- {fluid, solid} with the delta terms on the fluid
                                            source only.  gradrho of destination and source are independent inputs; one
                                            cluster per continuity table has fac XIJ = gradrho_i + gradrho_j up to 2^-20
                                            (judged at the scale of arho, which ContinuityEquation's own term carries).
The library reports the family that ran (``pair_delta_sph_pre`` / ``pair_wcsph_options``, asserted here).

One derived allowance, on the column ``dt_cfl`` alone.  The reference writes max_j |HIJ VIJ.XIJ / R2IJ| + c0; the base
family forms the quotient as hv * rinv * rinv with rinv from v_rsq_f64 and one Newton step, measured at 4.2e-15 relative
(tools/microbench/rcp_accuracy.hip): two estimated reciprocal square roots in the term.  Measured on
an MI355X without the allowance: LaminarViscosity/momentum/1d_cubic/uh, ``dt_cfl`` of rows 6 and 7 (the strongly
approaching pair, term 3.31 of dt_cfl 4.81), K 19.08 against the bound 18.29 (K_eq 4.57), both schedules; every other
element of the file was inside its bound.  The family is the one the benchmark times, so the accuracy is not restored
there; FACTOR stays 4, and ``dt_cfl`` is allowed 2 x 4.2e-15 x |term| on top of its bound, |term| = dt_cfl - c0 of the
REFERENCE's stored result (0 where no pair set it): 52.1 u S at that element.

Measured on an MI355X: DESIGN.md, section 7e ("Pair by pair").

Mutants.  Each change below was made to the text of the reference's method (or of gj_solve) in memory and run in double
over the stored inputs on the CPU (``make_wcsph_options_pair_golden.py --mutants``); "caught" = the result leaves the
bound of this file or raises where the reference does not; the figure is the number of stored destinations.  No mutant
was built for or run on the GPU.
    gradrho_j dropped from psi                                         caught (372)
    gradrho_i dropped from psi                                         caught (496)
    fac = -2 (rho_j - rho_i) with the sign lost                        caught (416)
    HIJ replaced by h_i (continuity)                                   caught (256)
    HIJ replaced by h_i (momentum)                                     caught (272)
    eta HIJ^2 replaced by EPS with eta = 1/64                          caught (136)
    eta HIJ^2 replaced by eta HIJ                                      caught (136)
    2 (dim + 2) replaced by 2 dim                                      caught (520)
    m_j replaced by V_j in LaminarViscosity                            caught (136)
    V_j replaced by m_j in MomentumEquationDeltaSPH                    caught (520)
    rho_i replaced by rho_j in MomentumEquationDeltaSPH                caught (488)
    moment matrix transposed                                           NOT caught
    moment matrix without V_b                                          caught (504)
    pivot threshold 1e-12 changed to 1e-11 (2^-39 = 1.8e-12)           caught (96)
    pivot threshold 1e-12 changed to 1e-13 (2^-41 = 4.5e-13)           caught (96)
    the zero last pivot eliminated above                               caught (400)
    change relative to |DWIJ| without 1e-4 HIJ                         caught (2320)
    change < tol changed to change <= tol                              NOT caught
    the corrected gradient applied to the first component only         caught (755)
The two that are not caught are equivalent mutants: DWIJ is a multiple of XIJ, so the moment matrix
-sum V DWIJ[i] XIJ[j] is symmetric and its transpose is itself; ``change`` equals ``tol`` in no stored pair (and cannot
but by accident of rounding).
"""
import importlib.util
import json
import os

import numpy as np
import pytest

from conftest import load_golden
from test_gasd_pair_edges import measure
from test_edac_pair_edges import spec_of, column, inputs, k_eq, bounds, WELL, FACTOR, MARGIN

LABELS = ('GradientCorrectionPreStep', 'GradientCorrection', 'ContinuityEquationDeltaSPHPreStep', 'ContinuityEquationDeltaSPH',
          'MomentumEquationDeltaSPH', 'LaminarViscosity', 'LaminarViscosityDeltaSPH', 'delta_terms', 'scheme_rates',
          'scheme_rates_solid')
REQUIRED = ('corrected', 'uncorrected', 'pivot0_below', 'pivot0_above', 'pivot1_below', 'pivot1_above', 'n1_tiny_pivot',
            'last_zero_rhs_small', 'last_zero_rhs_large', 'rho_equal', 'rij_below_1e-12', 'rij_above_1e-12',
            'coincident_unequal_h', 'psi_cancelling')
CONFIGS = (('1d_cubic', 1), ('2d_wendland', 2), ('3d_quintic', 3), ('3d_gauss', 3))
STRIDE = {'m_mat': 9, 'gradrho': 3}
RSQ_ONE_NEWTON = 4.2e-15          # v_rsq_f64 + one Newton step, relative (measured: tools/microbench/rcp_accuracy.hip)
U53 = 2.0 ** -53
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FILE = 'wcsph_options_pair_edges.npz'


def _kinds(dim):
    out = [('GradientCorrectionPreStep', 'moment_n%d' % n) for n in (1, 2, 3)]
    for n in (1, 2, 3):
        out += [('GradientCorrection', 'well_n%d' % n), ('GradientCorrection', 'built_n%d' % n)]
    return out + [('ContinuityEquationDeltaSPHPreStep', 'alone'), ('ContinuityEquationDeltaSPHPreStep', 'behind'),
                  ('ContinuityEquationDeltaSPH', 'continuity'), ('MomentumEquationDeltaSPH', 'momentum'),
                  ('LaminarViscosity', 'momentum'), ('LaminarViscosityDeltaSPH', 'momentum'), ('delta_terms', 'momentum'),
                  ('scheme_rates', 'fluid'), ('scheme_rates_solid', 'solid')]


TABLES = ['%s/%s/%s/%s' % (label, kind, c, f) for c, dim in CONFIGS for f in ('uh', 'vh') for label, kind in _kinds(dim)]
ORDER = [(c, f) for c, dim in CONFIGS for f in ('uh', 'vh')]
PRE = ('GradientCorrectionPreStep', 'GradientCorrection', 'ContinuityEquationDeltaSPHPreStep')

_G = []


def fixture():
    if not _G:
        _G.append(load_golden(FILE))
    return _G[0]


# ---------------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------------
def test_golden_generator_imports_cleanly():
    if not os.path.isdir('/root/reference'):
        pytest.skip('the generator needs the reference (build container only)')
    spec = importlib.util.spec_from_file_location('make_wcsph_options_pair_golden',
                                                  os.path.join(GOLDEN, 'make_wcsph_options_pair_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert callable(mod.main) and mod.OUT.endswith(FILE)
    assert mod.REQUIRED == REQUIRED and (mod.WELL, mod.FACTOR, mod.MARGIN) == (WELL, FACTOR, MARGIN)
    assert mod.LABELS == LABELS and mod.UNOBSERVABLE == () and mod.STRIDE == STRIDE
    assert set(mod.MUTANTS) == set(REQUIRED) and set(mod.SENSITIVE) == set(LABELS)
    assert set(mod.EQUIVALENT) <= set(e[0] for e in mod.ARITH)


def test_the_conditions_asserted_on_the_reference_are_in_the_file():
    """items 1..6 of the generator's docstring, from the stored data"""
    g = fixture()
    assert os.path.getsize(os.path.join(GOLDEN, FILE)) < 1024 * 1024
    assert json.loads(str(g['tables'])) == TABLES
    assert tuple(json.loads(str(g['meta/required']))) == REQUIRED and json.loads(str(g['meta/unobservable'])) == []
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
            eqs = [e['name'] for e in sp['group']]
            if label == 'GradientCorrection':                                   # m_mat is an input of the gradient pass
                assert eqs == ['GradientCorrection', 'ContinuityEquationDeltaSPHPreStep']
                assert all('m_mat__%d' % k in sp['in'][sp['dest']] for k in range(9))
                assert sp['outputs'] == ['gradrho__0', 'gradrho__1', 'gradrho__2']
            if 'ContinuityEquationDeltaSPH' in eqs:                             # gradrho of both ends is an input
                assert all('gradrho__%d' % k in sp['in'][a] for k in range(3) for a in sp['arrays'] if a == 'fluid')
        assert total > 0 and bad * 10 <= total, (label, bad, total)               # item 4
        assert best == ks[label] and best <= WELL, (label, best, ks[label])         # item 5
    short = dict((b, n) for b, n in taken.items() if n < 2)
    assert not short, short                                                       # item 1
    observed = json.loads(str(g['meta/observed']))
    assert all(observed[b] >= 2 for b in REQUIRED), observed                      # item 3
    sensitive = json.loads(str(g['meta/sensitive']))
    assert all(sensitive[e] >= 1 for e in LABELS), sensitive                      # item 6
    # n = 1, 2, 3 in every configuration (n is GradientCorrection.dim, whatever the kernel's dimension: the scheme's
    # default 2 also in a 1-D run, where M11 = 0 is the zero last pivot).  The zero last pivot with that row's DWIJ
    # exactly 0 wherever a partner has it so (not in 1-D under n = 1); with it not 0 wherever one can (n <= dim >= 2: with
    # n > dim the last row's DWIJ is 0 for every partner)
    for c, dim in CONFIGS:
        for f in ('uh', 'vh'):
            for n in (1, 2, 3):
                sp = spec_of(g, 'GradientCorrection/built_n%d/%s/%s' % (n, c, f))
                assert sp['group'][0]['params'] == {'dim': n, 'tol': 2.0 ** 50}
                flat = set(b for nm in sp['names'] for b in nm)
                assert ('last_zero_rhs_small' in flat) == (dim >= 2 or n >= 2), (c, f, n)
                assert ('last_zero_rhs_large' in flat) == (dim >= 2 and n <= dim), (c, f, n)
                well = set(b for nm in spec_of(g, 'GradientCorrection/well_n%d/%s/%s' % (n, c, f))['names'] for b in nm)
                assert ('last_zero_rhs_small' in well) == (dim >= 2 or n >= 2), (c, f, n)
                assert ('n1_tiny_pivot' in flat) == (n == 1) and ('pivot0_below' in flat) == (n >= 2)
                assert ('pivot1_above' in flat) == (n == 3)


def test_the_stored_reference_is_within_its_own_k_of_the_50_digit_values():
    """ref, mp + mplo, S and kref of the file agree: K recomputed in mpmath equals the stored float32 figure"""
    g = fixture()
    for key in TABLES:
        for c in spec_of(g, key)['outputs']:
            k = measure(column(g, key, 'ref', c), column(g, key, 'mp', c), column(g, key, 'mplo', c), column(g, key, 'S', c))
            kref = column(g, key, 'kref', c)
            assert np.array_equal(np.isinf(k), np.isinf(kref)), (key, c)
            fin = np.isfinite(k)
            assert np.allclose(k[fin], kref[fin], rtol=1e-6, atol=1e-6), (key, c)


def test_exact_elements_of_the_file():
    """what the GPU test compares exactly is exact in the file: the moment matrix outside its block, a pair at
    r <= 1e-12, a pair of equal densities, a result of zero applied under tol = 2^50, and the order rule"""
    g = fixture()
    seen = dict(outside=0, no_gradient=0, rho_equal=0, zero_result=0, order=0)
    for key in TABLES:
        sp = spec_of(g, key)
        for c in sp['outputs']:
            S, ref = column(g, key, 'S', c), column(g, key, 'ref', c)
            exact = S == 0
            assert np.array_equal(ref[exact], column(g, key, 'mp', c)[exact]) and np.all(column(g, key, 'mplo', c)[exact] == 0), (key, c)
        cl = np.array(sp['cl'][sp['dest']])
        members = sum(np.bincount(np.array(v), minlength=cl.max() + 1) for v in sp['cl'].values())
        if sp['label'] == 'GradientCorrectionPreStep':
            n = sp['group'][0]['params']['dim']
            for i in range(3):
                for j in range(3):
                    if i >= n or j >= n:
                        assert np.all(column(g, key, 'ref', 'm_mat__%d' % (3 * i + j)) == 0) and np.all(column(g, key, 'S', 'm_mat__%d' % (3 * i + j)) == 0)
                        seen['outside'] += 1
        for i, nm in enumerate(sp['names']):
            pair = members[cl[i]] == 2
            if pair and ('rij_below_1e-12' in nm or 'coincident_unequal_h' in nm) and sp['label'] in PRE:
                assert all(column(g, key, w, c)[i] == 0 for w in ('ref', 'S') for c in sp['outputs']), (key, i)
                seen['no_gradient'] += 1
            if pair and 'rho_equal' in nm and sp['label'] in ('GradientCorrection', 'ContinuityEquationDeltaSPHPreStep'):
                assert all(column(g, key, w, c)[i] == 0 for w in ('ref', 'S') for c in sp['outputs']), (key, i)
                seen['rho_equal'] += 1
            if pair and sp['label'] == 'GradientCorrection' and ('pivot0_below' in nm or 'pivot1_below' in nm or 'last_zero_rhs_large' in nm) \
                    and 'corrected' in nm:
                n = sp['group'][0]['params']['dim']
                assert all(column(g, key, 'ref', 'gradrho__%d' % k)[i] == 0 for k in range(n)), (key, i)      # DWIJ := res = 0
                seen['zero_result'] += 1
    for c, f in ORDER:
        a, b = ['ContinuityEquationDeltaSPHPreStep/%s/%s/%s' % (k, c, f) for k in ('alone', 'behind')]
        ia, ib = inputs(g, a, 'fluid'), inputs(g, b, 'fluid')           # (the second also holds the m_mat its correction reads)
        assert set(ia) <= set(ib) and all(np.array_equal(ia[k], ib[k]) for k in ia) and np.array_equal(g[a + '/ref'], g[b + '/ref'])
        assert spec_of(g, b)['group'][1]['name'] == 'GradientCorrection'
        seen['order'] += 1
    assert min(seen.values()) >= 2, seen


# ---------------------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------------------
def build_arrays(g, key):
    """the table's arrays with every property WCSPHScheme(delta_sph=True) sets up, m_mat and gradrho with their strides;
    the stored columns as they are, every other column garbage"""
    from pysph_amd.particle_array import get_particle_array_wcsph
    from pysph_amd.scheme import WCSPHScheme
    sp = spec_of(g, key)
    rng = np.random.default_rng(len(key))
    arrays = []
    for name in sp['arrays']:
        arrays.append(get_particle_array_wcsph(name=name, **dict((c, v.copy()) for c, v in inputs(g, key, name).items() if '__' not in c)))
    WCSPHScheme(['fluid'], [a for a in sp['arrays'] if a != 'fluid'], dim=sp['dim'], rho0=1.0, c0=1.5, h0=2.0 ** -3, hdx=1.0,
                delta_sph=True, nu=0.375).setup_properties(arrays)
    for pa in arrays:
        stored = inputs(g, key, pa.name)
        for c in pa.properties:
            v = pa.properties[c]
            if v.dtype != np.float64:
                continue
            s = STRIDE.get(c, 1)
            for k in range(s):
                comp = c if s == 1 else '%s__%d' % (c, k)
                v[k::s] = stored[comp] if comp in stored else rng.uniform(-7.0, 7.0, v.size // s)
    return arrays


def device_names(pa):
    out = []
    for c in sorted(pa.properties):
        if pa.properties[c].dtype == np.float64:
            s = STRIDE.get(c, 1)
            out += [c] if s == 1 else ['%s__%d' % (c, k) for k in range(s)]
    return out


def group_of(sp):
    from pysph_amd import equations as EQ
    eqs = [getattr(EQ, e['name'])(dest=sp['dest'], sources=list(e['sources']), **e['params']) for e in sp['group']]
    return [EQ.Group(equations=eqs)]


def evaluate(g, key, variant):
    """one launch of one group over one table; returns the arrays after it (everything pulled) and what they held before"""
    from pysph_amd import device as dev
    from pysph_amd import kernels as K
    from pysph_amd.acceleration_eval import AccelerationEval, SPHCompiler
    from pysph_amd.nnps import HipNNPS
    sp = spec_of(g, key)
    arrays = build_arrays(g, key)
    before = dict(((pa.name, c), pa.properties[c].copy()) for pa in arrays for c in pa.properties if pa.properties[c].dtype == np.float64)
    kernel = getattr(K, sp['kernel'])(dim=sp['dim'])
    ctx = dev.HipContext(0)
    ctx.set_option('pair_variant', variant)
    a_eval = AccelerationEval(arrays, group_of(sp), kernel)
    SPHCompiler(a_eval, ctx=ctx, sync='manual').compile()
    for pa in arrays:
        pa.gpu.push(*device_names(pa))
    nnps = HipNNPS(kernel.dim, arrays, radius_scale=kernel.radius_scale, ctx=ctx, sync=False)
    a_eval.set_nnps(nnps)
    ctx.lib.sph_timer_enable(ctx._h, 1)
    nnps.update()
    names = [pa.name for pa in arrays]
    for sn in sp['sources']:                   # the neighbour lists are the clusters, nothing leaks across
        start, idx = nnps.get_csr(names.index(sn), names.index(sp['dest']))
        want = sp['nbr'][sn]
        assert np.array_equal(start, np.cumsum([0] + [len(v) for v in want])), (key, sn)
        assert [sorted(int(j) for j in idx[start[i]:start[i + 1]]) for i in range(len(want))] == want, (key, sn)
    a_eval.compute(sp['t'], 0.0)
    launches = dict((k, ctx.timer_get(k)[1]) for k in ('pair_delta_sph_pre', 'pair_wcsph_options', 'pair_wcsph', 'pair_density'))
    for pa in arrays:
        pa.gpu.pull(*device_names(pa))
    ctx.close()
    family = 'pair_delta_sph_pre' if sp['label'] in PRE else 'pair_wcsph_options'
    assert launches[family] == 1 and sum(launches.values()) == 1, (key, launches)      # the family under test, nothing else
    return arrays, before


def run_table(g, key, variant):
    sp = spec_of(g, key)
    outs = sp['outputs']
    bases = set(c.split('__')[0] for c in outs)
    arrays, before = evaluate(g, key, variant)
    by_name = dict((pa.name, pa) for pa in arrays)
    dest = by_name[sp['dest']]
    for (name, c), v in before.items():
        if not (name == sp['dest'] and c in bases):
            assert np.array_equal(by_name[name].properties[c], v, equal_nan=True), (key, name, c, 'an input column changed')
    bnd = bounds(g, key)
    mpok = np.array(sp['mpok'], bool)
    worst, where, ill = 0.0, None, 0.0
    for c in outs:
        b, _, comp = c.partition('__')
        got = dest.properties[b][(int(comp) if comp else 0)::STRIDE.get(b, 1)]
        ref = column(g, key, 'ref', c)
        assert np.array_equal(np.isnan(got), np.isnan(ref)), (key, c, 'NaN pattern')
        S = column(g, key, 'S', c)
        k = measure(got, column(g, key, 'mp', c), column(g, key, 'mplo', c), S)
        exact = (S == 0)
        assert np.all(k[exact] == 0), (key, c, 'an element of scale 0 is not exact', np.nonzero(exact & (k != 0))[0][:4],
                                       got[exact & (k != 0)][:4], ref[exact & (k != 0)][:4])
        bound, well = bnd[c]
        if c == 'dt_cfl':       # the derived allowance of the docstring: two estimated rsq in |HIJ VIJ.XIJ / R2IJ|
            c0 = [e for e in sp['group'] if e['name'] == 'MomentumEquation'][0]['params']['c0']
            term = np.where(ref > 0, ref - c0, 0.0)
            assert np.all(term >= 0)
            with np.errstate(invalid='ignore', divide='ignore'):
                bound = bound + np.where(S > 0, 2 * RSQ_ONE_NEWTON * term / (U53 * S), 0.0)
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


@pytest.mark.gpu
@pytest.mark.parametrize('variant', [6, 0])
@pytest.mark.parametrize('config,form', ORDER)
def test_a_correction_behind_the_pre_step_corrects_nothing(config, form, variant):
    """[ContinuityEquationDeltaSPHPreStep, GradientCorrection] against the pre-step alone on the same inputs: gradrho
    bit for bit (each of the two is held to the uncorrected 50-digit sums by the test above)"""
    g = fixture()
    res = []
    for kind in ('alone', 'behind'):
        arrays, _ = evaluate(g, 'ContinuityEquationDeltaSPHPreStep/%s/%s/%s' % (kind, config, form), variant)
        res.append(arrays[0].properties['gradrho'].copy())
    assert np.abs(res[0]).max() > 0 and np.array_equal(res[0], res[1])
