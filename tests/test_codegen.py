"""Host-side tests of the generated-family path (pysph_amd/codegen.py): the
Python -> HIP translation, its loud failure modes, and the hipcc build for
gfx950 (cross-compiles without a GPU).  Running the generated kernels is
covered under -m gpu (tests/test_hip_parity.py::test_generated_*)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def _arrays():
    from pysph_amd.particle_array import (get_particle_array_tvf_fluid,
                                          get_particle_array_tvf_solid)
    f = get_particle_array_tvf_fluid(name='fluid', x=np.zeros(3))
    w = get_particle_array_tvf_solid(name='wall', x=np.zeros(3))
    return {'fluid': f, 'wall': w}


def _body_lines(src):
    """generated source without comment-only differences"""
    out = []
    for ln in src.splitlines():
        ln = ln.split('//')[0].rstrip()
        if ln:
            out.append(ln)
    return out


def test_wall_equations_translate_build_and_export():
    from pysph_amd.codegen import GeneratedFamily
    from wall_equations_fixture import (SetWallVelocity, SolidWallNoSlipBC,
                                          SolidWallPressureBC)
    arrays = _arrays()
    fam = GeneratedFamily('wall', [SetWallVelocity('wall', ['fluid'])], arrays, 3, 'cg_swv')
    assert fam.din == ['u', 'v', 'w']
    assert fam.dout == ['uf', 'vf', 'wf', 'wij', 'ug', 'vg', 'wg']
    assert fam.sprops == ['u', 'v', 'w'] and fam.sources == ['fluid']
    assert 'WIJ' in fam.symbols and 'DWIJ' not in fam.symbols
    lib = C.CDLL(fam.build())
    assert lib.sphgen_kernel_kind() == 3
    assert hasattr(lib, 'sphgen_launch')
    # parameters are frozen by value at build time (equation.py:885-892)
    eq = SolidWallPressureBC('wall', ['fluid'], rho0=1.0, p0=100.0, gy=-1.0)
    fam = GeneratedFamily('wall', [eq], arrays, 3, 'cg_pbc')
    eq.gy = 5.0
    vals = dict((k[2], v) for k, v in zip([p[0] for p in fam.params], fam.param_values()))
    assert vals['gy'] == -1.0 and vals['p0'] == 100.0
    # two equations, different source lists -> per-source flag bits
    fam = GeneratedFamily('fluid', [SolidWallNoSlipBC('fluid', ['wall'], nu=0.01),
                                    SetWallVelocity('fluid', ['fluid', 'wall'])],
                          arrays, 3, 'cg_two')
    assert fam.sources == ['wall', 'fluid']
    assert fam.src_flags == {'wall': 3, 'fluid': 2}
    fam.build()


def test_float_build_of_a_family():
    """`codegen.source_f32` (option arith_f32 for generated families): the arithmetic of the emitted source in
    float, the interface parts untouched, a binary of its own that cross-compiles and exports the launch entry."""
    import re
    from pysph_amd.codegen import GeneratedFamily, source_f32
    from custom_equations import KitchenSink, PyMomentum
    from pysph_amd.particle_array import get_particle_array
    pa = get_particle_array(name='fluid', x=np.zeros(3), constants=dict(coef=np.array([1.25, -0.5])),
                            additional_props=['q', 'gx', 'gy', 'gz', 'e', 'au', 'av', 'aw', 'p', 'cs', 'dt_cfl', 'dt_force'])
    arrays = {'fluid': pa}
    for eqs in ([KitchenSink('fluid', ['fluid'], a=0.3, b=0.05, flag=True)],
                [PyMomentum(dest='fluid', sources=['fluid'], c0=10.0, alpha=0.25, beta=0.1, gz=-9.81,
                            tensile_correction=True)]):
        fam = GeneratedFamily('fluid', eqs, arrays, 2, 'cg_f32')
        f32 = fam.flavour_f32()
        assert f32 is fam.flavour_f32() and f32.hash != fam.hash and f32.source == source_f32(fam.source)
        src = f32.source

        def block(text, first, last):
            i = text.index(first)
            return text[i:text.index(last, i) + len(last)]
        # kept as they are: Params (fp64 pointers), the fp64 record reader, the launch wrapper
        for first, last in (('    struct Params {', '\n    };'),
                            ('template <> __device__ __forceinline__ void load_record<FamGen, true>', '\n}\n'),
                            ('extern "C" int sphgen_kernel_kind', 'return (int)hipGetLastError();\n}')):
            assert block(src, first, last) == block(fam.source, first, last)
        # everything else computes in float: no double left outside those blocks (index casts aside), literals suffixed
        rest = src
        for first, last in (('    struct Params {', '\n    };'),
                            ('template <> __device__ __forceinline__ void load_record<FamGen, true>', '\n}\n'),
                            ('extern "C" int sphgen_kernel_kind', 'return (int)hipGetLastError();\n}'),
                            ('struct GenF32View {', '};')):
            rest = rest.replace(block(rest, first, last), '')
        rest = rest.replace('((double)d_idx)', '').replace('((double)o)', '')
        code = '\n'.join(ln.split('//')[0] for ln in rest.splitlines())
        assert not re.search(r'\bdouble\b', code), re.findall(r'.*\bdouble\b.*', code)[:3]
        assert 'typedef float Real;' in src and 'PairGeomT<float> g;' in src and 'const GenF32View PAR{a.p.par};' in src
        assert not re.search(r'(?<![\w.])\d+\.\d*(?:[eE][+-]?\d+)?(?![\w.f])', code)       # no double literal left
        lib = C.CDLL(f32.build())
        assert lib.sphgen_kernel_kind() == 2 and hasattr(lib, 'sphgen_launch')
    # a pair body that reads a neighbour's ABSOLUTE position keeps fp64 records (fp32 records are origin-relative)
    from pysph_amd.equations import Equation

    class AbsPos(Equation):
        def loop(self, d_idx, s_idx, d_q, s_x, s_m):
            d_q[d_idx] += s_m[s_idx] * s_x[s_idx]
    assert GeneratedFamily('fluid', [AbsPos('fluid', ['fluid'])], arrays, 2, 'cg_abs').abs_src_pos
    assert not fam.abs_src_pos


def test_float_literal_rewrite_touches_only_floating_literals():
    """the literal pass of `source_f32`: floating literals get the float suffix, nothing else is touched (integers,
    flag masks, identifiers with digits, array sizes, member names, already-suffixed literals)"""
    from pysph_amd.codegen import _F32_LITERAL
    cases = [('x = 0.5 * y;', 'x = 0.5f * y;'), ('a = 1e-12;', 'a = 1e-12f;'), ('b = 2.;', 'b = 2.f;'),
             ('c = .25 + 1.0e+3;', 'c = .25f + 1.0e+3f;'), ('d = 3.5E-2 - 7;', 'd = 3.5E-2f - 7;'),
             ('if (fl & 4u) {', 'if (fl & 4u) {'), ('double s00 = D.d_s00;', 'double s00 = D.d_s00;'),
             ('m[((w * 1) + 2)] = x1e5;', 'm[((w * 1) + 2)] = x1e5;'), ('v = a.k.dim * 3;', 'v = a.k.dim * 3;'),
             ('t = pj.x - 0.0;', 't = pj.x - 0.0f;'), ('u = d_amat__10 + 10.0;', 'u = d_amat__10 + 10.0f;'),
             ('w = q[2] * 1.5f;', 'w = q[2] * 1.5f;'), ('k = 0x1f + 1;', 'k = 0x1f + 1;')]
    for src, want in cases:
        assert _F32_LITERAL.sub(r'\1f', src) == want, src


def test_translation_details():
    from pysph_amd.codegen import GeneratedFamily
    from pysph_amd.equations import Equation

    class E(Equation):
        def __init__(self, dest, sources):
            self.k = 2.5
            self.on = True
            super(E, self).__init__(dest, sources)

        def loop(self, d_idx, s_idx, d_au, s_m, XIJ, RIJ, WIJ):
            a = min(RIJ, 1.0, self.k) ** 2
            b = a if (RIJ > 0.5 and self.on) or not (WIJ < 0) else -a
            d_au[d_idx] += b * s_m[s_idx] * XIJ[0] / (RIJ + 1e-3)

    fam = GeneratedFamily('fluid', [E('fluid', ['fluid'])], _arrays(), 2, 'cg_det')
    src = fam.source
    # min() keeps the first of equal arguments, as Python does: gen_pymin, not fmin
    assert 'gen_pymin(gen_pymin(RIJ, 1.0), PAR[0])' in src and 'fmin(' not in src
    assert '(gen_pymin(gen_pymin(RIJ, 1.0), PAR[0]) * gen_pymin(gen_pymin(RIJ, 1.0), PAR[0]))' in src   # **2 -> product
    assert '&&' in src and '||' in src and '!(' in src and '?' in src
    assert 'D.d_au +=' in src and 's_m = s[0]' in src
    assert [p[0][2] for p in fam.params] == ['k', 'on'] and fam.param_values() == [2.5, 1.0]


@pytest.mark.parametrize('body,msg', [
    ('while RIJ > 0:\n                pass', 'statement While'),
    ('d_au[d_idx] += foo(RIJ)', 'call to foo()'),
    ('s_m[s_idx] = 1.0', 'read-only'),
    ('d_au[d_idx] += undefined_name', 'unknown name'),
    ('d_au[s_idx] += 1.0', 'must be indexed with d_idx'),
    ('d_au[d_idx] += XIJ', 'must be subscripted'),
])
def test_unsupported_constructs_fail_loudly(body, msg, tmp_path):
    from pysph_amd.codegen import CodegenError, GeneratedFamily
    mod = tmp_path / 'bad_eq.py'
    mod.write_text(
        'from pysph_amd.equations import Equation\n'
        'class Bad(Equation):\n'
        '    def loop(self, d_idx, s_idx, d_au, s_m, XIJ, RIJ):\n'
        '        %s\n' % body.replace('\n                ', '\n            '))
    sys.path.insert(0, str(tmp_path))
    try:
        import importlib
        if 'bad_eq' in sys.modules:
            del sys.modules['bad_eq']
        bad = importlib.import_module('bad_eq')
        with pytest.raises(CodegenError) as ei:
            GeneratedFamily('fluid', [bad.Bad('fluid', ['fluid'])], _arrays(), 2, 'bad')
        assert msg in str(ei.value)
    finally:
        sys.path.remove(str(tmp_path))


def test_loop_all_families_and_missing_kernel():
    from pysph_amd.acceleration_eval import _CGroup
    from pysph_amd.codegen import CodegenError, GeneratedFamily
    from pysph_amd.equations import Equation, Group

    class NeedsLists(Equation):
        def loop_all(self, d_idx, d_au, s_m, NBRS, N_NBRS):
            i = declare('int')
            for i in range(N_NBRS):
                d_au[d_idx] += s_m[NBRS[i]]

    class PairToo(Equation):
        def loop(self, d_idx, d_au, WIJ):
            d_au[d_idx] += WIJ

    class NoBody(Equation):
        pass

    arrays = _arrays()
    fam = GeneratedFamily('fluid', [NeedsLists('fluid', ['fluid'])], arrays, 2, 'la')
    assert fam.loop_all and not fam.split_init and fam.sprops == ['m']
    assert 'S_m[((int)NBRS[i])]' in fam.source
    # loop and loop_all on one destination: loop_all launch, then the pair launch,
    # initialize split off (mako :62-110 runs loop_all, then loop, per source)
    mix = GeneratedFamily('fluid', [NeedsLists('fluid', ['fluid']), PairToo('fluid', ['fluid'])],
                          arrays, 2, 'mix')
    assert mix.loop_all and mix.also_pair and mix.split_init
    ids = {'fluid': 0, 'wall': 1}
    with pytest.raises(NotImplementedError):      # neither hand-written nor translatable
        _CGroup(Group([NoBody('fluid', ['fluid'])]), ids, arrays, 2)


def test_mixed_destination_rules():
    """hand-written + generated equations on one destination: a generated
    initialize that only repeats the hand-written resets is dropped, any other
    initialize is refused."""
    from pysph_amd.acceleration_eval import _CGroup
    from pysph_amd.equations import (Equation, Group,
                                     MomentumEquationPressureGradient)
    from wall_equations_fixture import SolidWallNoSlipBC

    class Scales(Equation):
        def initialize(self, d_idx, d_au):
            d_au[d_idx] = d_au[d_idx] * 0.5

        def loop(self, d_idx, s_idx, d_au, WIJ):
            d_au[d_idx] += WIJ

    arrays = _arrays()
    ids = {'fluid': 0, 'wall': 1}
    mom = MomentumEquationPressureGradient('fluid', ['fluid', 'wall'], pb=1.0)
    cg = _CGroup(Group([mom, SolidWallNoSlipBC('fluid', ['wall'], nu=0.1)]), ids, arrays, 3)
    assert [type(u).__name__ for u in cg.units] == ['_BuiltinUnit', '_GeneratedUnit']
    assert cg.units[1].fam.bodies['initialize'] == []          # dropped
    with pytest.raises(NotImplementedError):
        _CGroup(Group([mom, Scales('fluid', ['wall'])]), ids, arrays, 3)


def _sha256_lines(lines):
    import hashlib
    return hashlib.sha256('\n'.join(lines).encode()).hexdigest()


def test_reference_classes_translate_like_the_restatements():
    """The reference's own wall-equation classes, put through the same translator,
    gave the SAME generated code as tests/wall_equations_fixture.py (comments
    aside): the in-repo bodies are the reference's semantics, statement by
    statement.  The reference's side is stored in tests/golden/reference_pins.json
    (tests/golden/make_golden.py reference_pins: SHA-256 of the generated code and
    the property lists); the restatements must translate to it.  The same holds for
    a loop_all equation (ShepardFilter, density_correction.py:24-46: initialize()
    split off).  The reference's ContinuityEquation + MomentumEquation +
    XSPHCorrection, as one family, used the symbols (WDP, RHOIJ1, VIJ ...) and
    source flags of their restatements in tests/custom_equations.py, whose family
    is compiled."""
    import json
    import wall_equations_fixture as mine
    from pysph_amd.codegen import GeneratedFamily
    with open(os.path.join(REPO, 'tests', 'golden', 'reference_pins.json')) as f:
        ref = json.load(f)['translations']
    arrays = _arrays()
    cases = [
        ('SetWallVelocity', dict(dest='wall', sources=['fluid'])),
        ('SolidWallPressureBC', dict(dest='wall', sources=['fluid'], rho0=1.0, p0=100.0, gy=-1.0)),
        ('SolidWallNoSlipBC', dict(dest='fluid', sources=['wall'], nu=0.01)),
        ('ContinuitySolid', dict(dest='fluid', sources=['wall'])),
        ('VolumeSummation', dict(dest='fluid', sources=['fluid', 'wall'])),
        ('VolumeFromMassDensity', dict(dest='fluid', sources=None)),
    ]
    sys.path.insert(0, os.path.join(REPO, 'tests'))
    import custom_equations as ce
    from pysph_amd.particle_array import get_particle_array_wcsph
    pf = get_particle_array_wcsph(name='fluid', x=np.zeros(2))
    pf.add_property('rhotmp')
    b = GeneratedFamily('fluid', [ce.ShepardFilter('fluid', ['fluid'])], {'fluid': pf}, 2, 'm')
    assert ref['ShepardFilter'] == {'body_sha256': _sha256_lines(_body_lines(b.source)),
                                    'loop_all': b.loop_all, 'split_init': b.split_init}
    assert b.loop_all and b.split_init
    for name, kw in cases:
        b = GeneratedFamily(kw['dest'], [getattr(mine, name)(**kw)], arrays, 3, 'm')
        assert ref[name]['body_sha256'] == _sha256_lines(_body_lines(b.source)), name
        assert (ref[name]['din'], ref[name]['dout'], ref[name]['sprops']) == (b.din, b.dout, b.sprops)
    fam = GeneratedFamily('fluid', [
        ce.PyContinuity('fluid', ['fluid', 'wall']),
        ce.PyMomentum('fluid', ['fluid', 'wall'], c0=10.0, alpha=0.2, beta=0.1,
                      gz=-9.81, tensile_correction=True),
        ce.PyXSPH('fluid', ['fluid'], eps=0.5)], arrays, 2, 'ref_wcsph')
    r = ref['wcsph_family']
    assert r['symbols'] == sorted(fam.symbols) and r['src_flags'] == fam.src_flags
    assert {'WDP', 'WIJ', 'DWIJ', 'VIJ', 'RHOIJ1'} <= fam.symbols
    assert fam.src_flags == {'fluid': 7, 'wall': 3}
    fam.build()


def test_locals_named_like_cpp_keywords_or_skeleton_variables():
    """`const`, `a`, `D` ... are fine Python locals (swe/basic.py uses `const`);
    in the generated C++ they get a trailing underscore."""
    from pysph_amd.codegen import GeneratedFamily
    from pysph_amd.equations import Equation

    class Keywordy(Equation):
        def loop(self, d_idx, s_idx, d_au, s_m, WIJ):
            const = 2.0
            a = const * WIJ
            D = declare('matrix(3)')
            D[0] = a
            for o in range(2):
                D[0] += o
            d_au[d_idx] += D[0] * s_m[s_idx]

    fam = GeneratedFamily('fluid', [Keywordy('fluid', ['fluid'])], _arrays(), 1, 'kw')
    src = fam.source
    assert 'double const_ = 0.0;' in src and 'double a_ = 0.0;' in src
    assert 'double D_[3] = {};' in src and 'for (int o_ = 0; o_ < 2; o_++)' in src
    assert 'D.d_au += (D_[0] * s_m);' in src
    fam.build()


def test_tvf_scheme_wall_equations_are_the_products_own_or_the_callers():
    """TVFScheme(fluids, solids) builds the reference's group list with the
    product's own wall equations (pysph_amd/wall_bc.py, written from the papers'
    formulae -- not the restatement of the reference's bodies the tests keep for
    cross-checking), or with whatever module the caller hands over."""
    import wall_equations_fixture
    from pysph_amd import wall_bc
    from pysph_amd.scheme import TVFScheme
    kw = dict(dim=3, rho0=1.0, c0=10.0, nu=0.01, p0=100.0, pb=100.0, h0=0.1)
    for mod, expect in ((None, wall_bc), (wall_equations_fixture, wall_equations_fixture)):
        groups = TVFScheme(['fluid'], ['wall'], wall_equations=mod, **kw).get_equations()
        eqs = [e for g in groups for e in g.equations]
        names = [type(e).__name__ for e in eqs]
        assert {'SetWallVelocity', 'SolidWallPressureBC', 'SolidWallNoSlipBC'} <= set(names)
        assert all(type(e).__module__ == expect.__name__ for e in eqs
                   if type(e).__name__.startswith(('SetWall', 'SolidWall')))
    # the two modules are different texts of the same mathematics
    import inspect
    a = inspect.getsource(wall_bc.SolidWallNoSlipBC.loop)
    b = inspect.getsource(wall_equations_fixture.SolidWallNoSlipBC.loop)
    assert a != b
    # no solids: nothing is needed
    assert len(TVFScheme(['fluid'], [], **kw).get_equations()) == 3


def test_cache_miss_without_hipcc_says_so(monkeypatch, tmp_path):
    """A box without ROCm's compiler runs prebuilt families only: a family that is
    not in the cache must name the missing .so and the compiler path, not die in
    subprocess with FileNotFoundError."""
    import pysph_amd.codegen as cg
    from wall_equations_fixture import SetWallVelocity
    monkeypatch.setattr(cg, 'GEN_DIR', str(tmp_path))        # empty cache
    monkeypatch.setattr(cg, 'DEFERRED', None)
    monkeypatch.setenv('HIPCC', str(tmp_path / 'no-such-hipcc'))
    fam = cg.GeneratedFamily('wall', [SetWallVelocity('wall', ['fluid'])], _arrays(), 3, 'cg_nohipcc')
    with pytest.raises(cg.CodegenError) as e:
        fam.build()
    msg = str(e.value)
    assert 'not in the prebuilt cache' in msg and 'no-such-hipcc' in msg and 'fam_' in msg
