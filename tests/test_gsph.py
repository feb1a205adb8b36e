"""Godunov SPH without a GPU: the group lists, parameters, choices and constructor defaults of ``GSPHScheme`` and
``GSPHAcceleration`` equal the reference's (stored by tests/golden/make_gsph_golden.py next to its vectors), the constants
equal the header, solids and slab-decomposed arrays are refused, and the conditions the generator asserted on the
reference are in the files."""
import json
import os
import re

import numpy as np
import pytest

from conftest import load_golden, REPO
import test_gasd as TG

EVAL_CASES = ('gsph_1d', 'gsph_2d', 'gsph_3d')
KINDS = {'SPH_EQ_GSPH_GRADIENTS': 40, 'SPH_EQ_GSPH_UPDATE_GHOST_PROPS': 41, 'SPH_EQ_GSPH_ACCELERATION': 42}
GRADS = ('px', 'py', 'pz', 'ux', 'uy', 'uz', 'vx', 'vy', 'vz', 'wx', 'wy', 'wz')
# of these every one is taken somewhere in the files; of hllc's two star cases both, of ducowicz's four at least two
REQUIRED = ('mono0', 'mono1_sign', 'mono1_shock', 'mono2', 'mono2_coincident', 'coincident_eij', 'hybrid', 'conduction',
            'min_zero', 'min_x2', 'min_x1', 'interp_delta', 'interp_linear', 'interp_linear_sstar', 'interp_cubic',
            'interp_cubic_sstar', 'prefun_rarefaction', 'prefun_shock', 'hllc_left_star', 'hllc_right_star')


def scheme_of(g, prefix=''):
    from pysph_amd.gas_dynamics import GSPHScheme
    return GSPHScheme(**json.loads(str(g[prefix + 'scheme'])))


def equations_of(g, prefix=''):
    return scheme_of(g, prefix).get_equations()


@pytest.mark.parametrize('case', EVAL_CASES + ('gsph_steps',))
def test_group_list_equals_the_reference(case):
    g = load_golden(case + '.npz')
    TG.assert_same_structure(TG.structure(equations_of(g)), json.loads(str(g['structure'])), case)


def test_group_list_of_every_kernel_case_and_option_combination():
    g = load_golden('gsph_kernels.npz')
    for name in json.loads(str(g['kernels'])):
        TG.assert_same_structure(TG.structure(equations_of(g, name + '/')), json.loads(str(g[name + '/structure'])), name)
    g = load_golden('gsph_options.npz')
    TG.assert_same_structure(TG.structure(equations_of(g, 'coincident/')), json.loads(str(g['coincident/structure'])),
                             'coincident')
    g = load_golden('gsph_structures.npz')
    names = json.loads(str(g['names']))
    assert set(('default', 'two_fluids_ghosts', 'conduction_hybrid', 'ghosts')) <= set(names)
    for name in names:
        want = json.loads(str(g[name + '/structure']))
        TG.assert_same_structure(TG.structure(equations_of(g, name + '/')), want, name)
        kw = json.loads(str(g[name + '/scheme']))
        ghosts = [grp for grp in want if [e['cls'] for e in grp['equations']] == ['GSPHUpdateGhostProps'] * len(kw['fluids'])]
        assert len(ghosts) == (1 if kw.get('has_ghosts') else 0) and all(not grp['real'] for grp in ghosts), name
        assert len(want) == 7 + len(ghosts), name
        # the reference's list does not hand tf to GSPHAcceleration: the equation keeps its own default
        acc = want[-1]['equations'][0]
        assert acc['cls'] == 'GSPHAcceleration' and acc['params']['tf'] == 1.0


def test_choices_and_constructor_defaults_equal_the_reference():
    from pysph_amd import gas_dynamics as G
    g = load_golden('gsph_structures.npz')
    s = G.GSPHScheme(['fluid'], [], dim=2, gamma=1.4, kernel_factor=1.2)
    choices = json.loads(str(g['choices']))
    assert choices == dict(rsolver=s.rsolver_choices, interpolation=s.interpolation_choices,
                           monotonicity=s.monotonicity_choices)
    assert len(choices['rsolver']) == 11 and sorted(choices['rsolver'].values()) == list(range(11))
    for key, val in json.loads(str(g['defaults/scheme'])).items():
        assert getattr(s, key) == val, key
    eq = G.GSPHAcceleration('fluid', ['fluid'])
    want = json.loads(str(g['defaults/acceleration']))
    assert set(('g1', 'g2', 'monotonicity', 'rsolver', 'interpolation', 'interface_zero', 'hybrid', 'blend_alpha', 'tf',
                'gamma', 'niter', 'tol', 'sstar', 'thermal_conduction')) <= set(want)
    for key, val in want.items():
        assert getattr(eq, key) == val, key
    assert G.GSPHAcceleration('fluid', ['fluid'], g2=0.1).thermal_conduction == 1
    assert (G.Exact, G.HLLC, G.HLLSY, G.Linear, G.Cubic) == (2, 3, 10, 1, 2)


def test_kind_selection_and_parameters():
    from pysph_amd import equations as E
    from pysph_amd import gas_dynamics as G
    kind, vals, dprops, sprops = E.resolve_equation(G.GSPHGradients('fluid', ['fluid']))
    assert (kind, vals) == (40, []) and set(GRADS) <= set(dprops) and set(('p', 'u', 'v', 'w', 'm', 'rho')) <= set(sprops)
    kind, vals, dprops, sprops = E.resolve_equation(G.GSPHUpdateGhostProps('fluid'))
    assert (kind, vals, sprops) == (41, [], ())
    assert set(dprops) == set(GRADS + ('grhox', 'grhoy', 'grhoz', 'dwdh', 'rho', 'div', 'p', 'cs', 'orig_idx'))
    assert 41 in E.NO_SOURCE_KINDS and G.GSPHUpdateGhostProps('fluid').no_source
    eq = G.GSPHAcceleration('fluid', ['fluid'], g1=0.2, g2=0.4, monotonicity=2, rsolver=G.HLLC, interpolation=G.Cubic,
                            interface_zero=False, hybrid=True, blend_alpha=3.0, tf=0.7, gamma=1.6, niter=30, tol=1e-7)
    kind, vals, dprops, sprops = E.resolve_equation(eq)
    assert (kind, vals) == (42, [0.2, 0.4, 2.0, 3.0, 2.0, 0.0, 1.0, 3.0, 0.7, 1.6, 30.0, 1e-7])
    state = set(('u', 'v', 'w', 'm', 'rho', 'p', 'cs', 'e', 'div', 'grhox', 'grhoy', 'grhoz') + GRADS)
    assert state <= set(sprops) and state | set(('au', 'av', 'aw', 'ae')) <= set(dprops)
    # the reference's own objects: classes of these names in a module of the reference's name
    for cls, want in ((G.GSPHGradients, 40), (G.GSPHAcceleration, 42)):
        clone = type(cls.__name__, (cls,), {})
        clone.__module__ = 'pysph.sph.gas_dynamics.gsph'
        assert E.resolve_equation(clone('fluid', ['fluid']))[0] == want


def test_kind_and_stepper_constants_equal_the_header():
    from pysph_amd import equations as E
    from pysph_amd import integrator as I
    hdr = open(os.path.join(REPO, 'include', 'sphhip.h')).read()
    ids = dict((c, int(v)) for c, v in re.findall(r'(SPH_EQ_[A-Z0-9_]+)\s*=\s*(\d+)', hdr))
    for cname, val in KINDS.items():
        assert ids[cname] == val and getattr(E, cname[4:]) == val, cname
    assert len(set(ids.values())) == len(ids) and max(ids.values()) < 64
    steps = dict((c, int(v)) for c, v in re.findall(r'(SPH_STEP_[A-Z0-9_]+)\s*=\s*(\d+)', hdr))
    assert steps['SPH_STEP_GSPH'] == I.STEP_GSPH == 9 and len(set(steps.values())) == len(steps)
    assert I.stepper_kind(I.GSPHStep()) == 9
    ref_named = type('GSPHStep', (object,), {})      # the reference's own stepper object: matched by class name
    assert I.stepper_kind(ref_named()) == 9
    ctx_src = open(os.path.join(REPO, 'pysph_amd', 'csrc', 'sph_ctx.hip')).read()
    for key in ('pair_gsph_gradients', 'pair_gsph', 'gsph_keep'):
        assert '"%s"' % key in ctx_src
    from pysph_amd import device as dev
    assert 'sph_gsph_failures' in dev.SIGNATURES and 'int sph_gsph_failures(' in hdr


def test_setup_properties_and_the_solver_configuration():
    from pysph_amd import particle_array as P
    from pysph_amd.gas_dynamics import GSPHScheme
    bare = P.ParticleArray(name='fluid', x=np.zeros(4), h=np.ones(4))
    s = GSPHScheme(['fluid'], [], dim=1, gamma=1.4, kernel_factor=1.2)
    s.setup_properties([bare])
    assert set(P.GASD_PROPS) | set(GRADS) <= set(bare.properties)
    assert np.array_equal(bare.properties['orig_idx'], np.arange(4)) and bare.properties['orig_idx'].dtype.kind == 'i'
    integ = s.configure_solver(tf=0.25, dt=1e-4)
    assert type(integ).__name__ == 'EulerIntegrator' and type(integ.steppers['fluid']).__name__ == 'GSPHStep'
    assert type(s.kernel).__name__ == 'Gaussian' and s.kernel.dim == 1
    assert s.tf == 0.25                                   # taken from the solver's keywords, as the reference does
    assert s.get_equations()[-1].equations[0].tf == 1.0   # ... and not handed on
    s.configure(rsolver=s.rsolver_choices['roe'], hybrid=True)
    acc = s.get_equations()[-1].equations[0]
    assert (acc.rsolver, acc.hybrid) == (6, True)
    with pytest.raises(RuntimeError):
        s.configure(no_such_parameter=1)


def test_solids_are_refused_at_construction():
    from pysph_amd.gas_dynamics import GSPHScheme
    with pytest.raises(NotImplementedError, match='WallBoundary'):
        GSPHScheme(['fluid'], ['wall'], dim=2, gamma=1.4, kernel_factor=1.2)


def _gsph_array(n=8):
    from pysph_amd import particle_array as P
    from pysph_amd.gas_dynamics import GSPHScheme
    pa = P.get_particle_array_gasd(name='fluid', x=np.linspace(0, 1, n), h=0.2 * np.ones(n), m=np.ones(n), e=np.ones(n))
    s = GSPHScheme(['fluid'], [], dim=1, gamma=1.4, kernel_factor=1.2, has_ghosts=True)
    return pa, s


def test_slab_decomposed_arrays_are_refused_before_any_launch():
    class NoDevice(object):
        helpers = {}

        class lib(object):
            @staticmethod
            def sph_eval_group(*a):
                raise AssertionError('launched')

    pa, s = _gsph_array()
    s.setup_properties([pa])
    plan = TG._evaluator_without_a_device([pa], s.get_equations())
    units = [u for cg in plan for u in cg.units]
    assert len(units) == 8 and all(u.gasd_arrays == set(['fluid']) for u in units)
    assert [bool(getattr(u, 'gsph_force', False)) for u in units] == [False] * 7 + [True]
    pa.slab_decomposed = True
    for u in units:
        with pytest.raises(NotImplementedError, match='slab-decomposed'):
            u.run(NoDevice(), 0.0, 1e-3)


def test_ghost_group_needs_orig_idx_and_the_failure_count_is_on_the_equation():
    pa, s = _gsph_array()
    with pytest.raises(RuntimeError, match="missing properties .*'px'"):     # the property check of AccelerationEval
        TG._evaluator_without_a_device([pa], s.get_equations())
    for col in GRADS:
        pa.add_property(col)
    with pytest.raises(RuntimeError, match='orig_idx'):
        TG._evaluator_without_a_device([pa], s.get_equations())
    s.setup_properties([pa])
    groups = s.get_equations()
    plan = TG._evaluator_without_a_device([pa], groups)
    ghost = [cg for cg in plan if cg.orig_idx_arrays]
    assert len(ghost) == 1 and ghost[0].orig_idx_arrays == set(['fluid']) and not ghost[0].group.real
    acc = groups[-1].equations[0]
    assert acc.solver_failures == plan[-1].solver_failures and acc.solver_failures() == 0    # (nothing has run)


def _meta_files():
    out = [(case, load_golden(case + '.npz'), '') for case in EVAL_CASES + ('gsph_steps', 'gsph_solvers', 'gsph_options')]
    g = load_golden('gsph_options.npz')
    out.append(('gsph_options coincident', g, 'coincident/'))
    g = load_golden('gsph_kernels.npz')
    out.extend(('gsph_kernels ' + name, g, name + '/') for name in json.loads(str(g['kernels'])))
    return out


def test_the_conditions_asserted_on_the_reference_are_in_the_files():
    """no solver returned 1, no iterative solve ended at niter - 1, no iteration within 1e-3 of tol, a relative 1e-13 of
    the inputs moves no result by 1e-9 -- per file; every branch taken somewhere -- over all files"""
    total = {}
    for what, g, prefix in _meta_files():
        returns = json.loads(str(g[prefix + 'meta/solver_returns']))
        assert returns and all(key.endswith(':0') for key in returns), (what, returns)
        assert float(g[prefix + 'meta/min_tol_margin']) > 1e-3, what
        assert int(g[prefix + 'meta/max_loop_index']) < 20 - 1, what
        assert float(g[prefix + 'meta/perturbation_1e-13_moves']) < 1e-9, what
        for key, n in json.loads(str(g[prefix + 'meta/branches'])).items():
            total[key] = total.get(key, 0) + n
    missing = [k for k in REQUIRED if total.get(k, 0) == 0]
    assert not missing, missing
    assert sum(total.get(k, 0) > 0 for k in ('ducowicz_a', 'ducowicz_b', 'ducowicz_c', 'ducowicz_d')) >= 2
    assert total.get('min_x3_a', 0) + total.get('min_x3_b', 0) > 0
    g = load_golden('gsph_solvers.npz')
    returns = json.loads(str(g['meta/solver_returns']))
    assert set(k.split(':')[0] for k in returns) == set((
        'non_diffusive', 'van_leer', 'exact', 'hllc', 'ducowicz', 'hlle', 'roe', 'llxf', 'hllc_ball', 'hll_ball', 'hllsy'))


def test_every_output_column_of_the_vectors_started_as_garbage_and_no_case_is_large():
    for case in EVAL_CASES:
        g = load_golden(case + '.npz')
        n = int(g['nreal/fluid'])
        assert n <= 252
        for col in ('rho', 'p', 'cs', 'div', 'au', 'ae') + GRADS[:3]:
            assert not np.array_equal(g['in/fluid/' + col], g['out/fluid/' + col]), (case, col)
        for col in ('x', 'y', 'z', 'u', 'v', 'w', 'm', 'e'):
            assert np.array_equal(g['in/fluid/' + col], g['out/fluid/' + col]), (case, col)
        assert np.all(g['out/fluid/rho'] > 0) and np.all(g['out/fluid/p'] > 0) and np.all(g['out/fluid/e'] > 0)
    g = load_golden('gsph_options.npz')
    assert int(g['coincident/nreal/f1']) + int(g['coincident/nreal/f2']) <= 252
    x1, y1 = g['coincident/in/f1/x'], g['coincident/in/f1/y']
    assert np.sum((x1 == g['coincident/in/f2/x'][0]) & (y1 == g['coincident/in/f2/y'][0])) == 1
    assert len(json.loads(str(g['names']))) == 2 * 3 * 3 * 2 + 1
