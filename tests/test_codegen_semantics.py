"""The translator's own semantics, construct by construct: the corpus of
tests/codegen_semantics_equations.py as generated HIP against the same class
bodies executed by CPython (oracle/py_eval.py on lists of Python floats).

Acceptance
  * "ops", "sel", "flow" (+ - * /, %, comparisons, and / or / not, selections,
    max / min, floor / ceil / sqrt / fabs / fmod, constants, parameters, integer
    arithmetic, statements, control flow, helpers): bit-identical, the sign of
    a zero included.
  * "libm" (one library call per case): within 4 ulp of mpmath at 50 digits,
    the budget tests/test_device_functions.py allows the device exp.
  * the float build of "flow" on inputs that are multiples of 1/8 below 64
    (every intermediate exact in fp32): equal to the Python result.
  * "pair" (the constructs inside a pair loop, 65 particles on a line): 1e-10
    of each field's maximum, the bar of the other generated-family tests (the
    pair symbols come from the fast reciprocal / square root paths).

Inputs stay where CPython does not raise (no division by zero, no sqrt / log of
a non-positive number, no pow overflow) and hold no NaN.

Worst error of the device libm on an MI355X over the rows of this table, in ulp
of the result (each function over all the cases that call it):

    pow / ** general 0.99   ** 3 (pow) 1.11   ** -1 1.05   ** 0.5 0.99
    (-x) ** k  0.90         ** 2 (a product) 0.50
    exp  0.73   log  0.50   log10 0.45   sin  0.57   cos  0.57   tan   0.61
    tanh 0.55   asin 0.61   acos  0.68   atan 0.73   sinh 0.51   cosh  0.51
    erf  0.74   atan2 1.16

Every function is inside the 4 ulp bound; none needed a bound of its own.
"""
import functools
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

N = 257                 # one full 256-thread block of the no-source launch and a ragged one
T, DT = 0.25, 1e-3
T32, DT32 = 0.25, 0.125
LIBM_ULP = 4.0


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
def input_table(f32=False):
    """rows of a, b, c: signed zeros, small and large magnitudes, exact ties, both sides of every threshold a
    case compares with (0, +-0.25, +-0.5, 1, 2, 1e100), multiples and half-multiples for % / floor / ceil, then
    seeded random rows; p > 0, u in [-1, 1] \\ {0}, e in [-700, 700] \\ {0}, k an integer in [-5, 5]"""
    rng = np.random.default_rng(20240611)
    if f32:
        special = [0.0, -0.0, 0.5, -0.5, 0.25, -0.25, 0.125, -0.125, 0.375, 0.625, -0.375, -0.625, 0.75, -0.75, 1.0,
                   -1.0, 2.0, 1.5, 2.5, -2.5, 3.0, 63.875, -63.875, 32.0]
        fill = lambda n: rng.integers(-511, 512, n) / 8.0
    else:
        up, dn = lambda x: np.nextafter(x, np.inf), lambda x: np.nextafter(x, -np.inf)
        special = [0.0, -0.0, 1e-100, -1e-100, 1e100, -1e100, 0.5, -0.5, up(0.5), dn(0.5), up(-0.5), dn(-0.5), 0.25,
                   -0.25, up(-0.25), dn(-0.25), 1.0, up(1.0), dn(1.0), -1.0, 2.0, up(2.0), dn(2.0), 0.3, -0.3, 0.6,
                   -0.6, 0.15, 0.9, 0.75, -0.75, 1.5, -1.5, 2.5, -2.5, 3.0, -3.0, 2.0 ** 51 + 0.5, -(2.0 ** 51 + 0.5),
                   5e-324, -5e-324, 1e-3, 123.456]
        fill = lambda n: rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)
    rows = [(x, x, x) for x in special]                                 # exact ties
    pick = special[:8] + [0.75, -0.75]
    for i, x in enumerate(pick):                                        # every ordering of a few values
        for j, y in enumerate(pick):
            rows.append((x, y, pick[(i + 2 * j + 1) % len(pick)]))
    rows += [(0.75, -0.75, 1.0), (0.75, 0.625, -0.75), (-0.75, 0.5, 0.0), (0.625, 0.75, -0.5)]
    assert len(rows) < N - 40
    abc = np.array(rows + list(zip(fill(N - len(rows)), fill(N - len(rows)), fill(N - len(rows)))))
    a, b, c = abc[:, 0].copy(), abc[:, 1].copy(), abc[:, 2].copy()
    pv = [0.25, 0.3, 1.0, 2.0, 1e-3, 1e3, 0.1, 7.0, 0.5, 1.5]
    p = np.array([pv[i % len(pv)] for i in range(N)])
    p[N // 2:] = 10.0 ** rng.uniform(-3, 3, N - N // 2)
    if not f32:
        # exact multiples and half-multiples of the divisor for %, floor(a / p), ceil(a / p)
        mult = [1.0, 2.0, -1.0, -3.0, 2.5, -0.5, 4.5, 2.0 ** 40]
        for i in range(N - 32, N):
            a[i] = mult[i % len(mult)] * p[i]
    uv = [1.0, -1.0, 0.5, -0.5, 1e-8, -1e-8, 0.999999, 2.0 ** -30, 0.25, -0.75]
    u = np.array([uv[i % len(uv)] for i in range(N)])
    u[40:] = rng.uniform(-1, 1, N - 40)
    u[u == 0] = 0.5
    ev = [700.0, -700.0, 1e-5, -1e-5, 1.0, -1.0, 0.5, 100.0, -100.0, 3.141592653589793, 1.5707963267948966, 20.0,
          -20.0, 355.0, 0.1]
    e = np.array([ev[i % len(ev)] for i in range(N)])
    e[45:200] = rng.uniform(-30, 30, 155)
    e[200:] = rng.uniform(-700, 700, N - 200)
    e[e == 0] = 0.5
    k = np.array([float(i % 11 - 5) for i in range(N)])
    return {'a': a, 'b': b, 'c': c, 'p': p, 'u': u, 'e': e, 'k': k}


# ---------------------------------------------------------------------------
# the two sides
# ---------------------------------------------------------------------------
def family_equations(name, f32=False):
    import codegen_semantics_equations as CE
    if f32:
        return [cls('fluid', None) for cls in CE.F32_FAMILIES[name] + [CE.Inexact32]] + \
            [CE.PairCount('fluid', ['fluid'])]
    return [cls('fluid', None) for cls in CE.FAMILIES[name]]


def output_names(eqs):
    import codegen_semantics_equations as CE
    from pysph_amd.codegen import method_properties
    outs = []
    for eq in eqs:
        outs += [p for p in method_properties(eq)[0] if p not in CE.INPUTS and p not in outs]
    return outs


def device_case(name, f32=False):
    """(particle array, [Group]) of one corpus family"""
    import codegen_semantics_equations as CE
    from pysph_amd.equations import Group
    from pysph_amd.particle_array import get_particle_array
    eqs = family_equations(name, f32)
    pa = get_particle_array(name='fluid', x=0.125 * np.arange(N), h=0.15 * np.ones(N))
    for k, v in input_table(f32).items():
        if k not in pa.properties:
            pa.add_property(k)
        pa.properties[k][:] = v
    for p in output_names(eqs):
        if p not in pa.properties:
            pa.add_property(p, stride=CE.STRIDED.get(p, 1))
    return pa, [Group(equations=eqs)]


class ListArray(object):
    """what oracle.py_eval.PyEval needs of a particle array, the properties as lists of Python floats: the
    reference arithmetic is CPython's own, no numpy scalar in it"""

    def __init__(self, name, n, table, outs, strides):
        self.name, self.n, self.constants = name, n, {}
        self.properties = dict((k, [float(x) for x in v]) for k, v in table.items())
        for p in outs:
            self.properties[p] = [0.0] * (n * strides.get(p, 1))

    def get_number_of_particles(self, real=False):
        return self.n


@functools.lru_cache(maxsize=None)
def python_results(name, f32=False):
    """the family executed by CPython: ({output: float64 array}, equations) -- computed once, shared"""
    import codegen_semantics_equations as CE
    from oracle.py_eval import PyEval
    from pysph_amd.equations import Group
    eqs = [e for e in family_equations(name, f32) if not e.sources]
    outs = output_names(eqs)
    ref = ListArray('fluid', N, input_table(f32), outs, CE.STRIDED)
    PyEval([ref], [Group(equations=eqs)], None, None).compute(*((T32, DT32) if f32 else (T, DT)))
    res = dict((p, np.array([float(x) for x in ref.properties[p]])) for p in outs)
    for v in res.values():
        v.setflags(write=False)
    return res, eqs


def run_on_device(name, f32=False):
    from test_hip_parity import make_eval
    from pysph_amd import kernels as K
    pa, groups = device_case(name, f32)
    a_eval, nnps, ctx = make_eval([pa], groups, K.CubicSpline(dim=1), 1)
    if f32:
        ctx.set_option('arith_f32', 1)
    a_eval.compute(*((T32, DT32) if f32 else (T, DT)))
    return pa, groups[0].equations


def differing(got, want):
    """indices where two float64 arrays are not the same values, zeros told apart by their sign"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    same = ((got == want) | (np.isnan(got) & np.isnan(want))) & (np.signbit(got) == np.signbit(want))
    return np.nonzero(~same)[0]


def case_labels(eqs):
    """{property: case} of the equations of one family, each class under the corpus family it belongs to"""
    import codegen_semantics_equations as CE
    from pysph_amd.codegen import method_properties
    label = {}
    for eq in eqs:
        fam = [f for f, classes in CE.FAMILIES.items() if type(eq) in classes]
        for p in method_properties(eq)[0]:
            label[p] = CE.CASES[fam[0]].get(p, p) if fam else p
    return label


def report_exact(pa, want, eqs):
    import codegen_semantics_equations as CE
    tab, bad, label = pa.properties, [], case_labels(eqs)
    for p, w in sorted(want.items()):
        idx = differing(tab[p], w)
        if idx.size:
            s = CE.STRIDED.get(p, 1)
            i = idx[0]
            bad.append('%s (%s): %d rows differ, first row %d (a=%r b=%r c=%r p=%r): device %r, CPython %r' % (
                label[p], p, idx.size, i // s, tab['a'][i // s], tab['b'][i // s], tab['c'][i // s], tab['p'][i // s],
                tab[p][i], w[i]))
    return bad


# ---------------------------------------------------------------------------
# GPU: differential tests
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('name', ['ops', 'sel', 'flow'])
def test_exact_constructs_are_bit_identical_to_cpython(name):
    want, _ = python_results(name)
    assert not any(np.isnan(v).any() for v in want.values())
    pa, eqs = run_on_device(name)
    bad = report_exact(pa, want, eqs)
    print('%s: %d cases, %d divergent' % (name, len(want), len(bad)))
    assert not bad, '\n'.join(bad)
    if name == 'flow':
        flag = [e for e in eqs if type(e).__name__ == 'StateFlag'][0]
        assert flag.flag == -1 and isinstance(flag.flag, int)       # the state slot came back


def exact_f32_results(name):
    """the CPython results of a float family without the deliberately inexact probe; they must fit fp32"""
    want = dict(python_results(name, True)[0])
    third = want.pop('r00')
    for v in want.values():
        assert np.array_equal(v, v.astype(np.float32).astype(np.float64))
    return want, third


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['flow', 'sel'])
def test_float_build_is_exact_on_dyadic_inputs(name):
    want, third = exact_f32_results(name)
    pa, eqs = run_on_device(name, True)
    bad = report_exact(pa, want, eqs)
    assert not bad, '\n'.join(bad)
    # it was the float build that ran: a / 3 is rounded to fp32 (half an ulp: 2^-24 relative), not to fp64
    got = pa.r00
    assert np.all(np.abs(got - third) <= 2.0 ** -24 * np.abs(third)) and np.count_nonzero(got != third) > N // 2
    assert np.array_equal(got, got.astype(np.float32).astype(np.float64))
    x = pa.x
    nn = (np.abs(x[:, None] - x[None, :]) < 2.0 * 0.15).sum(axis=1)           # CubicSpline radius 2 h
    assert np.array_equal(pa.r01, nn.astype(np.float64)) and nn.min() == 3 and nn.max() == 5
    if name == 'flow':
        assert [e for e in eqs if type(e).__name__ == 'StateFlag'][0].flag == -1


@functools.lru_cache(maxsize=None)
def libm_reference():
    """{case: [mpf per row]} at 50 digits"""
    import mpmath as mp
    import codegen_semantics_equations as CE
    mp.mp.dps = 50
    fn = {'sq': lambda x: x * x, 'cube': lambda x: x ** 3, 'inv': lambda x: 1 / x, 'sqrt': mp.sqrt,
          'pow': mp.power, 'negcube': lambda x: (-x) ** 3, 'negpow': lambda x, k: mp.power(-x, int(k)),
          'negsq': lambda x: -(x * x), 'powneg': lambda x, y: mp.power(x, -y),
          'exp': mp.exp, 'log': mp.log, 'log10': mp.log10, 'sin': mp.sin, 'cos': mp.cos, 'tan': mp.tan,
          'tanh': mp.tanh, 'asin': mp.asin, 'acos': mp.acos, 'atan': mp.atan, 'sinh': mp.sinh, 'cosh': mp.cosh,
          'erf': mp.erf, 'atan2': mp.atan2}
    tab = input_table()
    out = {}
    for case, spec in CE.LIBM_CASES.items():
        cols = [tab[c] for c in spec[1:]]
        out[case] = [fn[spec[0]](*[mp.mpf(float(col[i])) for col in cols]) for i in range(N)]
    return out


def ulp_errors(got, ref):
    """|got - ref| in units of the spacing of doubles at ref, the subtraction in mpmath"""
    import mpmath as mp
    mp.mp.dps = 50
    out = np.empty(len(ref))
    for i, (g, r) in enumerate(zip(got, ref)):
        out[i] = float(abs(mp.mpf(float(g)) - r) / mp.mpf(float(np.spacing(abs(float(r))))))
    return out


def check_libm(results, who):
    import codegen_semantics_equations as CE
    ref, bad, tab = libm_reference(), [], input_table()
    results = dict((CE.CASES['libm'][p], v) for p, v in results.items())      # by case
    assert sorted(results) == sorted(CE.LIBM_CASES)
    for case in sorted(ref):
        assert np.isfinite(results[case]).all(), case
        err = ulp_errors(results[case], ref[case])
        i = int(err.argmax())
        print('%s %-7s worst %.3f ulp at %s' % (who, case, err[i], ', '.join(
            '%s=%r' % (c, float(tab[c][i])) for c in CE.LIBM_CASES[case][1:])))
        if err[i] > LIBM_ULP:
            bad.append('%s: %.3f ulp' % (case, err[i]))
    assert not bad, '; '.join(bad)


@pytest.mark.gpu
def test_libm_cases_within_4_ulp_of_mpmath():
    import codegen_semantics_equations as CE
    pa, _ = run_on_device('libm')
    check_libm(dict((p, pa.properties[p]) for p in CE.CASES['libm']), 'device')


@pytest.mark.gpu
def test_pair_family_vs_python(oracle):
    """early return, a run-time loop with break, writes to WI / WJ and DWIJ, % and a value ``or`` inside a pair loop:
    65 particles on a line (more than one wavefront), CubicSpline"""
    from helpers import rel_err
    from oracle.py_eval import PyEval
    from test_hip_parity import make_eval
    pa, groups, kernel = pair_case()
    ref, rgroups, _ = pair_case()
    a_eval, nnps, ctx = make_eval([pa], groups, kernel, 1)
    a_eval.compute(T, DT)
    onn = oracle.OracleNNPS(1, [ref], radius_scale=kernel.radius_scale)
    onn.update()
    PyEval([ref], rgroups, kernel, onn).compute(T, DT)
    assert np.array_equal(pa.arho, ref.arho) and ref.arho.max() == 4 and ref.arho.min() == 2
    for prop in ('q', 'gx', 'gy'):
        assert np.abs(ref.properties[prop]).max() > 0
        assert rel_err(pa.properties[prop], ref.properties[prop]) < 1e-10, prop


def pair_case():
    import codegen_semantics_equations as CE
    from pysph_amd import kernels as K
    from pysph_amd.equations import Group
    from pysph_amd.particle_array import get_particle_array
    n = 65
    rng = np.random.default_rng(65)
    pa = get_particle_array(name='fluid', x=0.1 * np.arange(n), h=0.13 * np.ones(n), m=rng.uniform(0.5, 1.5, n))
    for p in ('q', 'gx', 'gy', 'arho'):         # names the suite registers anyway
        pa.add_property(p)
    eqs = [CE.PairFlow('fluid', ['fluid']), CE.PairAfter('fluid', ['fluid'])]
    return pa, [Group(equations=eqs)], K.CubicSpline(dim=1)


def prebuild(plan):
    """every family of this module, for tests/prebuild_generated.py"""
    from pysph_amd import kernels as K
    n = 0
    for name in ('ops', 'sel', 'flow', 'libm'):
        pa, groups = device_case(name)
        n += plan([pa], groups, K.CubicSpline(dim=1))
    for name in ('flow', 'sel'):
        pa, groups = device_case(name, True)
        n += plan([pa], groups, K.CubicSpline(dim=1), f32=True)
    pa, groups, kernel = pair_case()
    n += plan([pa], groups, kernel)
    return n


# ---------------------------------------------------------------------------
# host side
# ---------------------------------------------------------------------------
def _family(eqs, arrays=None, name='cg_sem'):
    from pysph_amd.codegen import GeneratedFamily
    if arrays is None:
        pa, _ = device_case('ops')
        arrays = {'fluid': pa}
    return GeneratedFamily('fluid', eqs, arrays, 1, name)


def test_corpus_runs_as_cpython_and_the_libm_reference_describes_it():
    """the reference side alone: every family runs under CPython without raising and without a NaN, the fp32 table
    is what the float build needs, and CPython's own libm results are within the bound of the mpmath reference
    (so LIBM_CASES says what the bodies compute)"""
    for name in ('ops', 'sel', 'flow'):
        res, _ = python_results(name)
        assert res and not any(np.isnan(v).any() or np.isinf(v).any() for v in res.values()), name
    tab = input_table(True)
    for k in 'abc':
        assert np.all(np.abs(tab[k]) < 64) and np.array_equal(tab[k] * 8, np.round(tab[k] * 8))
    for name in ('flow', 'sel'):
        want, third = exact_f32_results(name)
        assert want and np.count_nonzero(third != third.astype(np.float32)) > N // 2
    tab = input_table()
    assert np.signbit(tab['a']).any() and (tab['a'] == tab['b']).any() and tab['p'].min() > 0
    assert np.all(tab['u'] != 0) and np.all(np.abs(tab['u']) <= 1) and np.all(tab['e'] != 0)
    check_libm(python_results('libm')[0], 'CPython')


@pytest.mark.parametrize('name,f32', [('ops', False), ('sel', False), ('flow', False), ('libm', False),
                                      ('flow', True), ('sel', True), ('pair', False)])
def test_corpus_families_translate_and_cross_compile(name, f32):
    import ctypes as C
    if name == 'pair':
        pa, groups, _ = pair_case()
    else:
        pa, groups = device_case(name, f32)
    fam = _family(groups[0].equations, {'fluid': pa}, 'sem_' + name)
    assert '#pragma clang fp contract(off)' in fam.source
    for f in ([fam, fam.flavour_f32()] if f32 else [fam]):
        lib = C.CDLL(f.build())
        assert lib.sphgen_kernel_kind() == 1 and hasattr(lib, 'sphgen_launch')


def _probe(d, body, args='d_idx, d_cs, d_a, d_b', extra=''):
    """translate one probe equation given as text (inspect.getsource needs a file: a module in the directory d)"""
    import importlib
    d = str(d)
    name = 'sem_probe_%d' % abs(hash(body + args))
    with open(os.path.join(d, name + '.py'), 'w') as f:
        f.write('from oracle.py_eval import declare\nfrom pysph_amd.equations import Equation\n%s\n'
                'class Probe(Equation):\n    def loop(self, %s):\n%s\n' % (
                    extra, args, '\n'.join('        ' + ln for ln in body.split('\n'))))
    sys.path.insert(0, d)
    try:
        mod = importlib.import_module(name)
    finally:
        sys.path.remove(d)
    return _family([mod.Probe('fluid', None)])


def _lines(fam, needle):
    return [ln.strip() for ln in fam.source.splitlines() if needle in ln and 'a.p.d' not in ln]


def test_true_division_of_integers_goes_through_the_arithmetic_type(tmp_path):
    fam = _probe(tmp_path, "i, j = declare('int', 2)\nfor i in range(1, 3):\n    for j in range(1, 3):\n"
                 "        d_cs[d_idx] += i / j + (i < j) / j + i / 2 + d_a[d_idx] / j")
    ln, = _lines(fam, 'D.d_cs +=')
    assert '((double)i / (double)j)' in ln and '((double)((i < j)) / (double)j)' in ln
    assert '((double)i / 2.0)' in ln and '(D.d_a / (double)j)' in ln
    assert '(float)i / (float)j' in fam.flavour_f32().source


def test_modulo_has_the_sign_of_the_divisor_and_fmod_by_name_stays_c(tmp_path):
    fam = _probe(tmp_path, "d_cs[d_idx] = (-d_a[d_idx]) % 0.3 + fmod(d_a[d_idx], d_b[d_idx])", extra='from math import fmod')
    ln, = _lines(fam, 'D.d_cs =')
    assert 'gen_pymod((-D.d_a), 0.3)' in ln and ' fmod(D.d_a, D.d_b)' in ln
    assert 'if ((y < 0.0) != (r < 0.0)) r += y;' in fam.source and 'else r = y < 0.0 ? -0.0 : 0.0;' in fam.source


def test_and_or_as_values_pick_an_operand_and_stay_operators_in_conditions(tmp_path):
    fam = _probe(tmp_path, "d_cs[d_idx] = d_a[d_idx] or 5.0\nd_cs[d_idx] += d_a[d_idx] and d_b[d_idx]\n"
                 "d_cs[d_idx] -= (d_a[d_idx] + 1.0) or d_b[d_idx]\n"
                 "if d_a[d_idx] and d_b[d_idx] or not d_a[d_idx]:\n    d_cs[d_idx] *= 2.0 if d_a[d_idx] or d_b[d_idx] else 3.0")
    assert _lines(fam, 'D.d_cs =') == ['D.d_cs = (D.d_a ? D.d_a : (5.0));']
    assert _lines(fam, 'D.d_cs +=') == ['D.d_cs += (D.d_a ? (D.d_b) : D.d_a);']
    assert _lines(fam, 'D.d_cs -=') == ['D.d_cs -= ((D.d_a + 1.0) ? (D.d_a + 1.0) : (D.d_b));']
    assert _lines(fam, 'if (((') == ['if (((((D.d_a) && (D.d_b))) || ((!(D.d_a))))) {']
    assert _lines(fam, 'D.d_cs *=') == ['D.d_cs *= ((((D.d_a) || (D.d_b))) ? (2.0) : (3.0));']


def test_max_min_keep_the_first_of_equal_arguments_and_floor_ceil_drop_the_sign_of_zero(tmp_path):
    fam = _probe(tmp_path, "d_cs[d_idx] = max(d_a[d_idx], d_b[d_idx], 0.0) + floor(d_a[d_idx]) + np.ceil(d_b[d_idx]) + min(d_a[d_idx], 1.0)",
                 extra='from math import floor\nimport numpy as np')
    ln, = _lines(fam, 'D.d_cs =')
    assert 'gen_pymax(gen_pymax(D.d_a, D.d_b), 0.0)' in ln and '(floor(D.d_a) + 0.0)' in ln and ' ceil(D.d_b))' in ln
    assert 'gen_pymax(double x, double y) { return y > x ? y : x; }' in fam.source
    assert 'gen_pymin(double x, double y) { return y < x ? y : x; }' in fam.source
    assert 'gen_pymin(D.d_a, 1.0)' in ln and 'gen_pymod' not in fam.source          # only what the bodies call


@pytest.mark.parametrize('body,msg', [
    ("k = declare('int')\nk = 4\nk /= 2\nd_cs[d_idx] = k", 'line 4: non-integer augmented assignment to the declared int k'),
    ("k = declare('int')\nk = 4\nk += 0.5\nd_cs[d_idx] = k", 'line 4: non-integer augmented assignment to the declared int k'),
    ("k = declare('int')\nk = 4\nk *= 1.5\nd_cs[d_idx] = k", 'line 4: non-integer augmented assignment to the declared int k'),
    ("k = declare('int')\nk = d_a[d_idx] * 2.0\nd_cs[d_idx] = k", 'line 3: non-integer expression assigned to the declared int k'),
    ("k = declare('int')\nk = 3 / 2\nd_cs[d_idx] = k", 'line 3: non-integer expression assigned to the declared int k'),
    ("k, m = declare('int', 2)\nk, m = 1, d_a[d_idx]\nd_cs[d_idx] = k", 'line 3: non-integer expression assigned to the declared int m'),
    ("k = declare('int')\nk = d_a[d_idx]\nd_cs[d_idx] = k * 0.5", 'line 4: int local k holds a property value truncated to an index'),
    # a negative subscript counts from the end in Python: not translated to an out-of-bounds access
    ("v = declare('matrix(3)')\nv[2] = d_a[d_idx]\nd_cs[d_idx] = v[-1]", 'line 4: array index must be an integer literal or a loop variable'),
    ("v = declare('matrix(3)')\ni = declare('int')\ni = 1\nv[-i] = d_a[d_idx]\nd_cs[d_idx] = v[0]", 'line 5: array index must be'),
    # Python restores the counter on the next pass
    ("i = declare('int')\nfor i in range(3):\n    i = 5\nd_cs[d_idx] = 1.0", 'line 4: assignment to i, the counter of a running loop'),
    ("i = declare('int')\nfor i in range(3):\n    i += 1\nd_cs[d_idx] = 1.0", 'line 4: assignment to i, the counter of a running loop'),
])
def test_what_python_would_keep_as_a_float_does_not_go_into_an_int(body, msg, tmp_path):
    from pysph_amd.codegen import CodegenError
    with pytest.raises(CodegenError) as ei:
        _probe(tmp_path, body)
    assert msg in str(ei.value)


def test_integer_statements_that_stay_integers_still_translate(tmp_path):
    fam = _probe(tmp_path, "k, m, i, j = declare('int', 4)\nk = 4\nk += 3\nk *= i\nk -= (k < m)\nm = -k if k > 2 else k % 3\n"
                 "for i in range(k):\n    k -= 1\nd_cs[d_idx] = k + m + i + i ** 3\nfor j in range(k):\n    d_cs[d_idx] += j")
    src = fam.source
    assert 'k += (int)(3.0);' in src and 'k *= (int)(i);' in src and 'm = (int)(' in src
    assert 'for (int i_it8 = 0, i_it8_end = k; i_it8 < i_it8_end; i_it8++) {' in src and 'i = i_it8;' in src
    assert '(i * i * i)' in src
    assert 'for (int j = 0; j < k; j++) {' in src       # bound untouched by the body, counter not read afterwards
    # an index held in a (double) property still becomes an int that indexes the destination
    from custom_equations import CopyFromOriginal
    from test_hip_parity import _image_case
    fam = _family([CopyFromOriginal('fluid', None)], {'fluid': _image_case()})
    assert 'idx = (int)(D.d_orig_idx);' in fam.source and 'D.d_rho = a.p.dout[' in fam.source


def test_helper_called_from_a_strict_equation_is_strict_too():
    import codegen_semantics_equations as CE
    pa, _ = device_case('flow')
    fam = _family([CE.HelperCalls('fluid', None)], {'fluid': pa})
    body = fam.source[fam.source.index('double gen_helper_h_scale('):]
    assert body.split('\n')[2].strip() == '#pragma clang fp contract(off)'


def test_negative_range_bounds_translate_and_dead_counter_stores_are_not_emitted(tmp_path):
    fam = _probe(tmp_path, "i, n = declare('int', 2)\nn = 2\nn += 1\nfor i in range(-3, n):\n    d_cs[d_idx] += i\n"
                           "for i in range(-n, -1):\n    d_cs[d_idx] += i")
    assert 'for (int i = (-3); i < n; i++) {' in fam.source and 'for (int i = (-n); i < (-1); i++) {' in fam.source
    # an unrolled loop over the components of a strided property: the counter is set afterwards only if it is read
    body = "i = declare('int')\nfor i in range(3):\n    d_g3[3 * d_idx + i] = d_a[d_idx]"
    pa, _ = device_case('flow')
    from pysph_amd.codegen import GeneratedFamily
    import importlib
    for tail, want in (('', False), ('\nd_g3[3 * d_idx] += i', True)):
        name = 'sem_unrolled_%d' % want
        (tmp_path / (name + '.py')).write_text(
            'from oracle.py_eval import declare\nfrom pysph_amd.equations import Equation\n'
            'class Probe(Equation):\n    def loop(self, d_idx, d_a, d_g3):\n%s\n' % '\n'.join(
                '        ' + ln for ln in (body + tail).split('\n')))
        sys.path.insert(0, str(tmp_path))
        try:
            mod = importlib.import_module(name)
        finally:
            sys.path.remove(str(tmp_path))
        src = GeneratedFamily('fluid', [mod.Probe('fluid', None)], {'fluid': pa}, 1, name).source
        assert ('i = 2;' in src) == want


def test_every_math_name_translates_the_same_under_every_prefix(tmp_path):
    """the corpus runs each libm name bare and under one prefix; the prefix handling does not depend on the name
    (floor / ceil apart, whose np and non-np forms the corpus runs): here every name under every prefix"""
    from pysph_amd.codegen import MATH_1, MATH_2
    lines, want = [], []
    for fn in sorted(MATH_1):
        for pre in ('', 'math.', 'np.', 'numpy.', 'M.'):
            lines.append('d_cs[d_idx] += %s%s(d_a[d_idx])' % (pre, fn))
            c = '%s(D.d_a)' % MATH_1[fn]
            want.append('D.d_cs += (%s + 0.0);' % c if fn in ('floor', 'ceil') and pre[:2] != 'np' and pre != 'numpy.'
                        else 'D.d_cs += %s;' % c)
    for fn in sorted(MATH_2):
        for pre in ('', 'math.', 'np.', 'numpy.', 'M.'):
            lines.append('d_cs[d_idx] += %s%s(d_a[d_idx], d_b[d_idx])' % (pre, fn))
            want.append('D.d_cs += %s(D.d_a, D.d_b);' % MATH_2[fn])
    fam = _probe(tmp_path, '\n'.join(lines), extra='from math import *\nimport math, numpy, numpy as np, math as M')
    assert _lines(fam, 'D.d_cs +=') == want

