"""ADKE gas dynamics without a GPU: the group lists of ``ADKEScheme`` equal the reference's (stored by
tests/golden/make_adke_golden.py next to its vectors), the four equation classes select kinds 43..46 with their
parameter vectors (``g2 = g1`` included), the constants equal the header, ``setup_properties`` and ``configure_solver``,
the refusal of slab-decomposed arrays, and the conditions the generator stored under ``meta/``."""
import json
import os
import re

import numpy as np
import pytest

from conftest import load_golden, REPO
import test_gasd as TG

EVAL_CASES = ('adke_1d', 'adke_2d', 'adke_3d', 'adke_two_fluids', 'adke_ghost_rows')
KINDS = {'SPH_EQ_SUMMATION_DENSITY_ADKE': 43, 'SPH_EQ_ADKE_ACCELERATIONS': 44, 'SPH_EQ_ADKE_UPDATE_GHOST_PROPS': 45,
         'SPH_EQ_GASD_WALL_BOUNDARY': 46}
REQUIRED = ['x', 'y', 'z', 'u', 'v', 'w', 'rho', 'h', 'm', 'cs', 'p', 'e', 'au', 'av', 'aw', 'arho', 'ae', 'am', 'ah', 'x0',
            'y0', 'z0', 'u0', 'v0', 'w0', 'rho0', 'e0', 'h0', 'div', 'wij', 'htmp', 'logrho']


def scheme_of(g, prefix=''):
    from pysph_amd.gas_dynamics import ADKEScheme
    return ADKEScheme(**json.loads(str(g[prefix + 'scheme'])))


def equations_of(g, prefix=''):
    return scheme_of(g, prefix).get_equations()


@pytest.mark.parametrize('case', EVAL_CASES + ('adke_steps',))
def test_group_list_equals_the_reference(case):
    g = load_golden(case + '.npz')
    TG.assert_same_structure(TG.structure(equations_of(g)), json.loads(str(g['structure'])), case)


def test_group_list_of_every_kernel_case_and_option_combination():
    g = load_golden('adke_kernels.npz')
    for name in json.loads(str(g['kernels'])):
        TG.assert_same_structure(TG.structure(equations_of(g, name + '/')), json.loads(str(g[name + '/structure'])), name)
    g = load_golden('adke_structures.npz')
    names = json.loads(str(g['names']))
    combos = set()
    for name in names:
        want = json.loads(str(g[name + '/structure']))
        TG.assert_same_structure(TG.structure(equations_of(g, name + '/')), want, name)
        kw = json.loads(str(g[name + '/scheme']))
        combos.add((bool(kw['solids']), bool(kw.get('has_ghosts'))))
        classes = [[e['cls'] for e in grp['equations']] for grp in want]
        nf, ns = len(kw['fluids']), len(kw['solids'])
        walls = [c for c in classes if c == ['WallBoundary'] * ns]
        assert len(walls) == (3 if ns else 0), name
        ghosts = [grp for grp, c in zip(want, classes) if c == ['ADKEUpdateGhostProps'] * nf]
        assert len(ghosts) == (1 if kw.get('has_ghosts') else 0) and all(not grp['real'] for grp in ghosts), name
        assert classes[-1] == ['ADKEAccelerations'] * nf
        assert ['IdealGasEOS'] * (nf + ns) in classes            # the EOS runs on the walls too
        # the neighbour update comes only behind the second density sweep
        assert [grp['update_nnps'] for grp in want].count(True) == 1
        k = [grp['update_nnps'] for grp in want].index(True)
        assert classes[k] == ['SummationDensity'] * nf
    assert combos == set([(False, False), (False, True), (True, False), (True, True)])


def test_kinds_and_parameter_vectors():
    from pysph_amd import equations as E
    from pysph_amd import gas_dynamics as G
    kind, vals, dprops, sprops = E.resolve_equation(G.SummationDensityADKE('fluid', ['fluid', 'wall'], k=0.3, eps=0.5))
    assert (kind, vals) == (43, [0.3, 0.5])
    assert set(('h0', 'rho', 'arho', 'div', 'logrho')) <= set(dprops) and set(sprops) == set('xyzhuvwm')
    eq = G.ADKEAccelerations('fluid', ['fluid', 'wall'], alpha=1.0, beta=2.0, g1=0.5, g2=1.0, k=0.3, eps=0.5)
    kind, vals, dprops, sprops = E.resolve_equation(eq)
    # the reference's constructor drops the g2 it is given (gas_dynamics/basic.py:287-288): g2 = g1
    assert (kind, vals) == (44, [1.0, 2.0, 0.5, 0.5, 0.3, 0.5]) and eq.g2 == eq.g1 == 0.5
    assert set(('p', 'rho', 'cs', 'e', 'div', 'm', 'u', 'v', 'w')) <= set(sprops)
    assert set(('au', 'av', 'aw', 'ae')) <= set(dprops)
    kind, vals, dprops, sprops = E.resolve_equation(G.ADKEUpdateGhostProps('fluid', None))
    assert (kind, vals, sprops) == (45, [], ()) and set(dprops) == set(('p', 'cs', 'rho', 'orig_idx'))
    assert G.ADKEUpdateGhostProps('fluid').dim == 2 and G.ADKEUpdateGhostProps('fluid').no_source
    kind, vals, dprops, sprops = E.resolve_equation(G.WallBoundary('wall', ['fluid']))
    assert (kind, vals) == (46, [])
    assert set(('wij', 'htmp', 'h0', 'p', 'rho', 'e', 'm', 'cs', 'div', 'u', 'v', 'w')) <= set(dprops)
    assert 45 in E.NO_SOURCE_KINDS and not set((43, 44, 46)) & set(E.NO_SOURCE_KINDS)
    d = G.SummationDensityADKE('fluid', ['fluid'])
    assert (d.k, d.eps) == (1.0, 0.0) and not hasattr(d, 'reduce')


def test_reference_named_and_moduled_clones_resolve_alike():
    from pysph_amd import equations as E
    from pysph_amd import gas_dynamics as G

    def clone(cls, module, *args, **kw):
        c = type(cls.__name__, (cls,), {})
        c.__module__ = module
        return c(*args, **kw)
    basic = 'pysph.sph.gas_dynamics.basic'
    assert E.resolve_equation(clone(G.SummationDensityADKE, basic, 'fluid', ['fluid'], k=0.3, eps=0.5))[:2] == (43, [0.3, 0.5])
    assert E.resolve_equation(clone(G.ADKEAccelerations, basic, 'fluid', ['fluid'], 1.0, 2.0, 0.2, 0.4, 0.3, 0.5))[0] == 44
    assert E.resolve_equation(clone(G.ADKEUpdateGhostProps, basic, 'fluid', None))[0] == 45
    assert E.resolve_equation(clone(G.WallBoundary, 'pysph.sph.gas_dynamics.boundary_equations', 'wall', ['fluid']))[0] == 46
    # WallBoundary is not a unique name in the reference: its namesakes of psph / tsph / magma2 are other equations
    for module in ('pysph.sph.gas_dynamics.psph', 'pysph.sph.gas_dynamics.tsph', 'pysph.sph.gas_dynamics.magma2'):
        with pytest.raises(NotImplementedError):
            E.resolve_equation(clone(G.WallBoundary, module, 'wall', ['fluid']))
    # the density equation of kind 6 in the ADKE list is basic_equations', not one of its gas-dynamics namesakes
    s = G.ADKEScheme(['fluid'], [], dim=1)
    assert [E.resolve_equation(grp.equations[0])[0] for grp in s.get_equations()] == [43, 6, 35, 44]


def test_constants_equal_the_header():
    from pysph_amd import equations as E
    from pysph_amd import integrator as I
    hdr = open(os.path.join(REPO, 'include', 'sphhip.h')).read()
    ids = dict((c, int(v)) for c, v in re.findall(r'(SPH_EQ_[A-Z0-9_]+)\s*=\s*(\d+)', hdr))
    for cname, val in KINDS.items():
        assert ids[cname] == val and getattr(E, cname[4:]) == val, cname
    assert len(set(ids.values())) == len(ids)
    steps = dict((c, int(v)) for c, v in re.findall(r'(SPH_STEP_[A-Z0-9_]+)\s*=\s*(\d+)', hdr))
    assert steps['SPH_STEP_ADKE'] == I.STEP_ADKE == 10
    assert len(set(steps.values())) == len(steps)
    assert I.stepper_kind(I.ADKEStep()) == 10
    assert I.stepper_kind(type('ADKEStep', (object,), {})()) == 10     # the reference's own stepper: matched by name
    ctx_src = open(os.path.join(REPO, 'pysph_amd', 'csrc', 'sph_ctx.hip')).read()
    for key in ('pair_adke_density', 'pair_adke', 'pair_gasd_wall'):
        assert '"%s"' % key in ctx_src


def test_setup_properties_and_configure_solver():
    from pysph_amd import particle_array as P
    from pysph_amd.gas_dynamics import ADKEScheme, ADKE_PROPS
    assert list(ADKE_PROPS) == REQUIRED
    fluid = P.ParticleArray(name='fluid', x=np.zeros(4), h=np.ones(4))
    wall = P.ParticleArray(name='wall', x=np.zeros(3), h=np.ones(3))
    s = ADKEScheme(['fluid'], ['wall'], dim=2)
    assert (s.gamma, s.alpha, s.beta, s.k, s.eps, s.g1, s.g2, s.has_ghosts) == (1.4, 1.0, 2.0, 1.0, 0.0, 0, 0, False)
    s.setup_properties([fluid, wall])
    assert set(REQUIRED) <= set(fluid.properties) and set(REQUIRED) <= set(wall.properties)
    assert np.array_equal(fluid.properties['orig_idx'], np.arange(4)) and fluid.properties['orig_idx'].dtype.kind == 'i'
    assert 'orig_idx' not in wall.properties
    out = ['x', 'y', 'u', 'v', 'rho', 'm', 'h', 'cs', 'p', 'e', 'au', 'av', 'ae', 'pid', 'gid', 'tag']
    assert fluid.output_property_arrays == out and wall.output_property_arrays == out
    integ = s.get_integrator()
    assert type(integ).__name__ == 'PECIntegrator' and sorted(integ.steppers) == ['fluid']
    assert type(integ.steppers['fluid']).__name__ == 'ADKEStep'
    assert type(s.kernel).__name__ == 'Gaussian' and s.kernel.dim == 2
    s.configure(k=0.3, eps=0.5)
    assert (s.k, s.eps) == (0.3, 0.5)
    with pytest.raises(RuntimeError):
        s.configure(kernel_factor=1.2)


def test_these_groups_are_not_fusable_and_the_reduce_hook_is_replaced():
    from pysph_amd import particle_array as P
    from pysph_amd.acceleration_eval import _plain_leaf, annotate_plan
    from pysph_amd.gas_dynamics import ADKEScheme
    fluid = P.ParticleArray(name='fluid', x=np.linspace(0, 1, 8), h=0.2 * np.ones(8))
    wall = P.ParticleArray(name='wall', x=np.linspace(-0.3, -0.1, 3), h=0.2 * np.ones(3))
    s = ADKEScheme(['fluid'], ['wall'], dim=1, has_ghosts=True)
    s.setup_properties([fluid, wall])
    groups = s.get_equations()
    plan = TG._evaluator_without_a_device([fluid, wall], groups)
    names = [[e.name for e in grp.equations] for grp in groups]
    for grp, cg, cls in zip(groups, plan, names):
        writes_h = cls[0] in ('WallBoundary', 'SummationDensityADKE')
        assert _plain_leaf(grp, cg) == (not writes_h and not grp.update_nnps), cls
        assert all(u.gasd_arrays for u in cg.units if cls[0] != 'SummationDensity')
        assert (len(cg.device_reduce) == 1) == (cls[0] == 'SummationDensityADKE')
        if writes_h:
            assert 'h' in cg.outputs_exact[grp.equations[0].dest]
        if cls[0] == 'WallBoundary':
            assert set(('h', 'm', 'u', 'v', 'w')) <= cg.outputs_exact['wall']
    annotate_plan(list(zip(groups, plan)))
    assert all(u.cg.nl_mode == 0 and u.cg.src_eos == 0 for cg in plan for u in cg.units)
    ghost = [cg for cg in plan if cg.orig_idx_arrays]
    assert len(ghost) == 1 and ghost[0].units[0].ceqs[0].kind == 45 and ghost[0].units[0].cg.real == 0
    assert 'h0' in plan[1].inputs['fluid']          # what a domain manager restricted to the evaluator's inputs carries


def test_slab_decomposed_arrays_are_refused_before_any_launch():
    from pysph_amd import particle_array as P
    from pysph_amd.gas_dynamics import ADKEScheme

    class NoDevice(object):
        helpers = {}

        class lib(object):
            @staticmethod
            def sph_eval_group(*a):
                raise AssertionError('launched')

    fluid = P.ParticleArray(name='fluid', x=np.linspace(0, 1, 8), h=0.2 * np.ones(8))
    wall = P.ParticleArray(name='wall', x=np.linspace(-0.3, -0.1, 3), h=0.2 * np.ones(3))
    s = ADKEScheme(['fluid'], ['wall'], dim=1, has_ghosts=True)
    s.setup_properties([fluid, wall])
    plan = TG._evaluator_without_a_device([fluid, wall], s.get_equations())
    fluid.slab_decomposed = True
    adke = [u for cg in plan for u in cg.units if any(u.ceqs[k].kind in (43, 44, 45, 46) for k in range(len(u.eqs)))]
    assert len(adke) == 6
    for u in adke:
        with pytest.raises(NotImplementedError, match='slab-decomposed'):
            u.run(NoDevice(), 0.0, 1e-3)


@pytest.mark.parametrize('case', EVAL_CASES)
def test_meta_conditions_of_the_golden_files(case):
    g = load_golden(case + '.npz')
    kw = json.loads(str(g['scheme']))
    assert float(g['meta/h_margin']) >= 0.0 and int(g['meta/n_neighbour_lists_checked']) > 0
    assert int(g['meta/n_approaching']) * 10 >= int(g['meta/n_pairs'])
    assert (int(g['meta/n_pairs']) - int(g['meta/n_approaching'])) * 10 >= int(g['meta/n_pairs'])
    n = sum(int(g['nreal/' + f]) for f in kw['fluids'])
    neg = int(g['meta/n_div_negative'])
    assert neg * 10 >= n and (n - neg) * 10 >= n
    assert float(g['meta/conditioning']) < 1e-9
    if case in ('adke_2d', 'adke_3d', 'adke_two_fluids'):
        assert kw['eps'] == 0.5
        assert float(g['meta/lambda_min']) <= 0.8 and float(g['meta/lambda_max']) >= 1.4
    for f in kw['fluids']:
        for col in ('rho', 'e'):
            assert np.all(g['out/%s/%s' % (f, col)][:int(g['nreal/' + f])] > 0.0)
    for w in kw['solids']:
        assert np.all(g['out/%s/wij' % w] > 1e-30)
    if case == 'adke_2d':
        assert kw['g1'] != kw['g2']                                  # a "repaired" g2 would show
        assert int(g['nreal/fluid']) == 252 and int(g['nreal/wall']) == 54
    assert any(sum(int(v) >= 4 for v in load_golden(c + '.npz')['meta/ncells']) >= 2 for c in EVAL_CASES)


def test_ghost_rows_case_holds_what_it_is_for():
    g = load_golden('adke_ghost_rows.npz')
    n_real, n = int(g['nreal/fluid']), g['in/fluid/x'].size
    assert n_real < n and np.all(g['in/fluid/tag'][n_real:] == 2) and np.all(g['in/fluid/orig_idx'][n_real:] < n_real)
    # three columns and no more: div of the rows behind the real ones is what went in
    assert np.array_equal(g['out/fluid/div'][n_real:], g['in/fluid/div'][n_real:])
    src = g['in/fluid/orig_idx'][n_real:]
    for col in ('p', 'cs', 'rho'):
        assert np.array_equal(g['out/fluid/' + col][n_real:], g['out/fluid/' + col][src])
    # the reduction counted them: h of every row from the sum over all n rows
    kw = json.loads(str(g['scheme']))
    logrho = np.concatenate([g['out/fluid/logrho'][:n_real], g['in/fluid/logrho'][n_real:]])
    assert np.array_equal(logrho, g['out/fluid/logrho'])
