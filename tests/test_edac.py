"""EDAC without a GPU: the group lists equal the reference's (stored by tests/golden/make_edac_golden.py next to
its vectors), name resolution, property sets, the inlet/outlet hooks, and the rewritten wall-equation bodies executed
as Python on the golden inputs against the reference's wall outputs."""
import json
import os
import re

import numpy as np
import pytest

from conftest import load_golden, arrays_from_golden, REPO
from helpers import rel_err

EVAL_CASES = ('edac_ext3d', 'edac_int2d', 'edac_int3d_nosolid')
SKIP_ATTRS = ('dest', 'sources', 'name', 'var_name', 'no_source')
KINDS = {'SPH_EQ_EDAC_AVG_PRESSURE': 30, 'SPH_EQ_EDAC_MOMENTUM': 31, 'SPH_EQ_EDAC_MOM_PRESSURE': 32, 'SPH_EQ_EDAC': 33}
TOL = 1e-10


def scheme_of(g, prefix=''):
    from pysph_amd.edac import EDACScheme
    return EDACScheme(**json.loads(str(g[prefix + 'scheme'])))


def equations_of(g, prefix=''):
    return scheme_of(g, prefix).get_equations()


def structure(groups):
    """as the generator's; a class is known by the name it carries (TVFSummationDensity: 'SummationDensity')"""
    out = []
    for g in groups:
        eqs = []
        for eq in g.equations:
            par = dict((k, (bool(v) if isinstance(v, bool) else float(v))) for k, v in vars(eq).items()
                       if k not in SKIP_ATTRS and not k.startswith('_') and isinstance(v, (bool, int, float)))
            eqs.append(dict(cls=eq.name, dest=eq.dest, sources=list(eq.sources or []), params=par))
        out.append(dict(real=bool(g.real), equations=eqs))
    return out


def assert_same_structure(got, want, what):
    assert len(got) == len(want), what
    for k, (a, b) in enumerate(zip(got, want)):
        assert a['real'] == b['real'], (what, k, a['real'])
        assert [e['cls'] for e in a['equations']] == [e['cls'] for e in b['equations']], (what, k)
        for ea, eb in zip(a['equations'], b['equations']):
            assert ea['dest'] == eb['dest'] and ea['sources'] == eb['sources'], (what, k, ea, eb)
            assert ea['params'] == eb['params'], (what, k, ea['cls'], ea['params'], eb['params'])


@pytest.mark.parametrize('case', EVAL_CASES + ('edac_steps',))
def test_group_list_equals_the_reference(case):
    g = load_golden(case + '.npz')
    assert_same_structure(structure(equations_of(g)), json.loads(str(g['structure'])), case)


def test_group_list_of_every_kernel_case_and_option_combination():
    g = load_golden('edac_kernels.npz')
    for name in json.loads(str(g['kernels'])):
        assert_same_structure(structure(equations_of(g, name + '/')), json.loads(str(g[name + '/structure'])), name)
    g = load_golden('edac_structures.npz')
    names = json.loads(str(g['names']))
    assert set(('bql_false', 'alpha0_nu0', 'no_solids_ext', 'no_solids_int', 'clamp_p_with_pb')) <= set(names)
    for name in names:
        assert_same_structure(structure(equations_of(g, name + '/')), json.loads(str(g[name + '/structure'])), name)


def test_average_pressure_sits_where_the_reference_puts_it():
    from pysph_amd.edac import EDACScheme
    kw = dict(dim=2, c0=10.0, nu=0.01, rho0=1.0, pb=10.0, h=0.1)
    groups = EDACScheme(['fluid'], [], **kw).get_equations()
    assert [e.name for e in groups[0].equations] == ['SummationDensity', 'ComputeAveragePressure'] and not groups[0].real
    groups = EDACScheme(['fluid'], ['wall'], **kw).get_equations()
    assert 'ComputeAveragePressure' not in [e.name for e in groups[0].equations]
    assert [e.name for e in groups[1].equations] == ['ComputeAveragePressure'] and groups[1].real
    assert len(EDACScheme(['fluid'], ['wall'], bql=False, **kw).get_equations()) == 2


def test_edac_nu_rule_is_silent(capsys):
    from pysph_amd.edac import EDACScheme
    s = EDACScheme(['fluid'], [], dim=2, c0=10.0, nu=0.03, rho0=1.0, h=0.2, edac_alpha=0.5)
    assert s.art_nu == 0.5 * 0.2 * 10.0 / 8 and s._get_edac_nu() == s.art_nu and not s.use_tvf
    s = EDACScheme(['fluid'], [], dim=2, c0=10.0, nu=0.03, rho0=1.0, h=0.2, edac_alpha=0.0, pb=1e-13)
    assert s._get_edac_nu() == 0.03 and s.use_tvf
    s.get_equations()
    assert capsys.readouterr().out == ''


def _named(name, module, base, **attrs):
    cls = type(name, (base,), {})
    cls.__module__ = module
    eq = cls('fluid', ['fluid'])
    for k, v in attrs.items():
        setattr(eq, k, v)
    return eq


def test_resolve_equation_tells_the_namesakes_apart_by_module():
    from pysph_amd import equations as E
    from pysph_amd import edac as ED
    par = dict(c0=10.0, gx=0.0, gy=0.0, gz=-1.0, tdamp=0.5, pb=7.0, alpha=0.1, beta=0.0, tensile_correction=False)
    for module, mom, press in (('pysph.sph.wc.edac', 31, 32), ('pysph_amd.edac', 31, 32), ('pysph.sph.wc.basic', 4, 9),
                               ('pysph.sph.wc.transport_velocity', 4, 9), ('user_script', 4, 9)):
        assert E.resolve_equation(_named('MomentumEquation', module, E.Equation, **par))[0] == mom, module
        assert E.resolve_equation(_named('MomentumEquationPressureGradient', module, E.Equation, **par))[0] == press, module
    kind, vals, dprops, sprops = E.resolve_equation(ED.MomentumEquation('fluid', ['fluid'], c0=10.0, gz=-1.0, tdamp=0.5))
    assert (kind, vals) == (31, [10.0, 0.0, 0.0, -1.0, 0.5])
    kind, vals, dprops, sprops = E.resolve_equation(ED.MomentumEquationPressureGradient('fluid', ['fluid'], pb=3.0, gx=1.0))
    assert (kind, vals) == (32, [3.0, 1.0, 0.0, 0.0, 0.0]) and 'pavg' in dprops
    assert E.resolve_equation(ED.EDACEquation('fluid', ['fluid'], cs=10.0, nu=0.2, rho0=1.0))[:2] == (33, [10.0, 0.2, 1.0])
    assert E.resolve_equation(ED.ComputeAveragePressure('fluid', ['fluid']))[0] == 30
    # the old classes keep their kernels
    assert E.resolve_equation(E.MomentumEquation('fluid', ['fluid'], c0=10.0))[0] == 4
    assert E.resolve_equation(E.MomentumEquationPressureGradient('fluid', ['fluid'], pb=1.0))[0] == 9


def test_kind_and_stepper_constants_equal_the_header():
    from pysph_amd import equations as E
    from pysph_amd import integrator as I
    hdr = open(os.path.join(REPO, 'include', 'sphhip.h')).read()
    ids = dict((c, int(v)) for c, v in re.findall(r'(SPH_EQ_[A-Z0-9_]+)\s*=\s*(\d+)', hdr))
    for cname, val in KINDS.items():
        assert ids[cname] == val and getattr(E, cname[4:]) == val, cname
    assert len(set(ids.values())) == len(ids)
    steps = dict((c, int(v)) for c, v in re.findall(r'(SPH_STEP_[A-Z0-9_]+)\s*=\s*(\d+)', hdr))
    assert steps['SPH_STEP_EDAC'] == I.STEP_EDAC == 6 and steps['SPH_STEP_EDAC_TVF'] == I.STEP_EDAC_TVF == 7
    assert len(set(steps.values())) == len(steps)
    assert I.stepper_kind(I.EDACStep()) == 6 and I.stepper_kind(I.EDACTVFStep()) == 7
    ref_named = type('EDACTVFStep', (object,), {})        # the reference's own stepper object: matched by class name
    assert I.stepper_kind(ref_named()) == 7


def test_particle_arrays_carry_the_reference_property_sets():
    from pysph_amd import particle_array as P
    assert P.EDAC_PROPS == ('ap', 'au', 'av', 'aw', 'ax', 'ay', 'az', 'x0', 'y0', 'z0', 'u0', 'v0', 'w0', 'p0', 'V')
    assert P.EDAC_SOLID_PROPS == ('ap', 'p0', 'wij', 'uf', 'vf', 'wf', 'ug', 'vg', 'wg', 'ax', 'ay', 'az', 'V')
    f = P.get_particle_array_edac(name='fluid', x=np.zeros(3))
    s = P.get_particle_array_edac_solid(name='wall', x=np.zeros(2))
    assert set(P.EDAC_PROPS) | set(P.DEFAULT_PROPS) == set(f.properties)
    assert set(P.EDAC_SOLID_PROPS) | set(P.DEFAULT_PROPS) == set(s.properties)
    assert f.output_property_arrays == ['x', 'y', 'z', 'u', 'v', 'w', 'rho', 'p', 'au', 'av', 'aw', 'ap', 'm', 'h']
    assert s.output_property_arrays == ['x', 'y', 'z', 'u', 'v', 'w', 'rho', 'p', 'h']


def test_setup_properties_and_stepper_choice():
    from pysph_amd import particle_array as P
    from pysph_amd.edac import EDACScheme
    from pysph_amd.integrator import EDACStep, EDACTVFStep, EPECIntegrator, PECIntegrator
    from pysph_amd.acceleration_eval import AccelerationEval
    from pysph_amd import kernels as K
    for pb, step_cls in ((0.0, EDACStep), (5.0, EDACTVFStep)):
        pas = [P.get_particle_array(name=n, x=np.zeros(4)) for n in ('fluid', 'wall', 'slip')]
        s = EDACScheme(['fluid'], ['wall'], dim=2, c0=10.0, nu=0.01, rho0=1.0, pb=pb, h=0.1, alpha=0.1,
                       inviscid_solids=['slip'])
        s.setup_properties(pas)
        fluid, wall, slip = pas
        if pb:
            assert set(('pavg', 'nnbr', 'uhat', 'auhat', 'ap', 'p0', 'V', 'x0')) <= set(fluid.properties)
            assert set(('xn', 'yn', 'zn', 'uhat', 'wij', 'ug', 'V')) <= set(slip.properties)
            assert 'pavg' in fluid.output_property_arrays
        else:
            assert set(P.EDAC_PROPS) <= set(fluid.properties) and 'pavg' not in fluid.properties
            assert set(P.EDAC_SOLID_PROPS) <= set(wall.properties)
        # every equation finds its properties
        AccelerationEval(pas, s.get_equations(), K.QuinticSpline(dim=2))
        integ = s.configure_solver()
        assert isinstance(integ, PECIntegrator) and type(integ.steppers['fluid']) is step_cls
        assert s.kernel.radius_scale == 3.0 and s.kernel.dim == 2
        assert isinstance(s.configure_solver(integrator_cls=EPECIntegrator), EPECIntegrator)
        assert s.get_timestep() > 0.0


class _StubIOM(object):
    def __init__(self):
        self.calls = []

    def get_io_names(self, ghost=False):
        self.calls.append('get_io_names(ghost=%s)' % ghost)
        return ['inlet']

    def get_equations(self, scheme, use_tvf):
        self.calls.append('get_equations(%s)' % use_tvf)
        from pysph_amd.equations import Group
        return [Group(equations=[], name='io_pre')]

    def get_equations_post_compute_acceleration(self):
        self.calls.append('get_equations_post_compute_acceleration')
        from pysph_amd.equations import Group
        return [Group(equations=[], name='io_post')]

    def get_stepper(self, scheme, cls, use_tvf):
        self.calls.append('get_stepper(%s, %s)' % (cls.__name__, use_tvf))
        from pysph_amd.integrator import WCSPHStep
        return {'inlet': WCSPHStep()}

    def add_io_properties(self, pa, scheme):
        self.calls.append('add_io_properties(%s)' % pa.name)

    def setup_iom(self, dim, kernel):
        self.calls.append('setup_iom(%d)' % dim)


@pytest.mark.parametrize('pb', [0.0, 5.0])
def test_inlet_outlet_manager_hooks_in_the_reference_order(pb):
    """wc/edac.py:783-795 / :891-904 (names, then the manager's groups first), :874-878 / :972-976 (its groups last),
    :689-703 (steppers, then setup_iom), :737-750 (ghost names, then add_io_properties per array)"""
    from pysph_amd import particle_array as P
    from pysph_amd.edac import EDACScheme
    iom = _StubIOM()
    s = EDACScheme(['fluid'], [], dim=2, c0=10.0, nu=0.01, rho0=1.0, pb=pb, h=0.1, inlet_outlet_manager=iom)
    groups = s.get_equations()
    tvf = str(bool(pb))
    assert iom.calls == ['get_io_names(ghost=False)', 'get_equations(%s)' % tvf, 'get_equations_post_compute_acceleration']
    assert groups[0].name == 'io_pre' and groups[-1].name == 'io_post'
    dens = groups[1].equations
    assert [e.dest for e in dens if e.name == 'SummationDensity'] == ['fluid', 'inlet']
    assert dens[0].sources == ['fluid', 'inlet']
    force = groups[-2].equations
    assert set(e.dest for e in force) == set(['fluid'])            # the io arrays are sources of the force group only
    del iom.calls[:]
    integ = s.configure_solver()
    assert iom.calls == ['get_stepper(PECIntegrator, %s)' % tvf, 'setup_iom(2)']
    assert sorted(integ.steppers) == ['fluid', 'inlet']
    del iom.calls[:]
    s.setup_properties([P.get_particle_array(name=n, x=np.zeros(2)) for n in ('fluid', 'inlet')])
    assert iom.calls == ['get_io_names(ghost=True)', 'add_io_properties(fluid)', 'add_io_properties(inlet)']


def _wall_groups(g):
    """the equations of the scheme's first group that run through the generated path, with the fluid's density and
    number density (hand-written SummationDensity, same group, an earlier destination) as the golden has them"""
    from pysph_amd.acceleration_eval import is_builtin
    from pysph_amd.equations import Group
    first = equations_of(g)[0]
    eqs = [eq for eq in first.equations if not is_builtin(eq)]
    return [Group(equations=eqs, real=False)]


@pytest.mark.parametrize('case', ['edac_ext3d', 'edac_int2d'])
def test_wall_equation_bodies_reproduce_the_reference(oracle, case):
    """SourceNumberDensity, VolumeSummation, SolidWallPressureBC, SetWallVelocity, ClampWallPressure and the two
    free-slip extrapolations, executed by oracle/py_eval.py: every wall output of the golden, every element.  Both
    sides are Python floats; only the order of the neighbour sums differs."""
    from oracle.py_eval import PyEval
    from pysph_amd import kernels as K
    g = load_golden(case + '.npz')
    arrays = arrays_from_golden(g)
    kw = json.loads(str(g['scheme']))
    fluid = [pa for pa in arrays if pa.name == 'fluid'][0]
    for p in ('rho', 'V'):
        fluid.properties[p][:] = g['out/fluid/' + p]
    groups = _wall_groups(g)
    names = set(eq.name for eq in groups[0].equations)
    want = set(['SourceNumberDensity', 'VolumeSummation', 'SolidWallPressureBC', 'SetWallVelocity'])
    if case == 'edac_ext3d':
        want |= set(['ClampWallPressure', 'NoSlipVelocityExtrapolation'])
    assert names == want
    kernel = getattr(K, str(g['kernel']))(dim=kw['dim'])
    onn = oracle.OracleNNPS(kw['dim'], arrays, radius_scale=kernel.radius_scale)
    onn.update()
    PyEval(arrays, groups, kernel, onn).compute(float(g['t']), float(g['dt']))
    n = 0
    for pa in arrays:
        if pa.name == 'fluid':
            continue
        for key in g.files:
            if key.startswith('out/%s/' % pa.name):
                prop = key.split('/')[2]
                e = rel_err(pa.properties[prop], g[key])
                assert e < TOL, (case, pa.name, prop, e)
                n += 1
    assert n >= 20
    if case == 'edac_ext3d':
        wall = [pa for pa in arrays if pa.name == 'wall'][0]
        assert np.any(wall.wij == 0.0) and np.any((wall.p == 0.0) & (wall.wij > 0)) and np.any(wall.p > 0.0)


def test_free_slip_advection_velocity_body():
    """NoSlipAdvVelocityExtrapolation is NoSlipVelocityExtrapolation on uhat, vhat, what (internal branch with
    inviscid solids): the Shepard mean reflected about the normal, by hand for one wall particle"""
    from pysph_amd.edac import NoSlipAdvVelocityExtrapolation
    eq = NoSlipAdvVelocityExtrapolation('slip', ['fluid'])
    uh, vh, wh = [0.0], [0.0], [0.0]
    eq.initialize(0, uh, vh, wh)
    su, sv, sw, wts = [1.0, 3.0], [2.0, -1.0], [0.5, 0.25], [0.2, 0.6]
    for j in range(2):
        eq.loop(0, j, uh, vh, wh, su, sv, sw, wts[j])
    n = np.array([0.6, 0.0, 0.8])
    eq.post_loop(0, [0.8], uh, vh, wh, [n[0]], [n[1]], [n[2]])
    mean = np.array([np.dot(su, wts), np.dot(sv, wts), np.dot(sw, wts)]) / 0.8
    want = mean - 2 * np.dot(mean, n) * n
    assert np.allclose([uh[0], vh[0], wh[0]], want, rtol=1e-15)
    eq.initialize(0, uh, vh, wh)
    eq.post_loop(0, [0.0], uh, vh, wh, [n[0]], [n[1]], [n[2]])      # no fluid in reach: stays zero
    assert (uh[0], vh[0], wh[0]) == (0.0, 0.0, 0.0)


def test_golden_conditions_hold():
    """what the generator asserted on the reference alone, stored with the vectors"""
    g = load_golden('edac_ext3d.npz')
    for pre in ('', 'second_'):
        assert int(g['meta/%sn_wij_zero' % pre]) >= 1 and float(g['meta/%smin_wij_nonzero' % pre]) >= 1e-8
        n, k = int(g['meta/%sn_pairs' % pre]), int(g['meta/%sn_approaching' % pre])
        assert min(k, n - k) * 10 >= n
        assert int(g['meta/%sn_clamped' % pre]) >= 1 and int(g['meta/%sn_unclamped' % pre]) >= 1
    g = load_golden('edac_int2d.npz')
    assert int(g['meta/n_wij_zero']) >= 1 and float(g['meta/min_wij_nonzero']) >= 1e-8 and float(g['meta/min_nnbr']) >= 1
    assert float(load_golden('edac_int3d_nosolid.npz')['meta/min_nnbr']) >= 1
    for name in EVAL_CASES:      # every output started as garbage in [-1, 1] and was written
        g = load_golden(name + '.npz')
        for p in ('rho', 'V', 'au', 'ap'):
            assert not np.array_equal(g['in/fluid/' + p][:int(g['nreal/fluid'])], g['out/fluid/' + p][:int(g['nreal/fluid'])])
