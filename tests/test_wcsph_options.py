"""WCSPHScheme options delta_sph / nu / update_h without a GPU: the group lists equal the reference's (stored by
tests/golden/make_wcsph_options_golden.py next to its vectors), the properties, the name table and the kind ids."""
import json
import os
import re

import numpy as np
import pytest

from conftest import load_golden, REPO

CASES = ('opt_dsph3d', 'opt_dsph2d_tank', 'opt_lamvisc3d', 'opt_dsph3d_gap', 'opt_singular')
NAMES = {'GradientCorrectionPreStep': 22, 'GradientCorrection': 23, 'ContinuityEquationDeltaSPHPreStep': 24,
         'ContinuityEquationDeltaSPH': 25, 'MomentumEquationDeltaSPH': 26, 'LaminarViscosity': 27,
         'LaminarViscosityDeltaSPH': 28, 'UpdateSmoothingLengthFerrari': 29}
SKIP_ATTRS = ('dest', 'sources', 'name', 'var_name', 'no_source')


def scheme_of(g):
    from pysph_amd.scheme import WCSPHScheme
    return WCSPHScheme(**json.loads(str(g['scheme'])))


def equations_of(g):
    """the scheme's group list with the attributes the generator changed after get_equations()"""
    groups = scheme_of(g).get_equations()
    for cls, attr, value in json.loads(str(g['overrides'])):
        for grp in groups:
            for eq in grp.equations:
                if type(eq).__name__ == cls:
                    setattr(eq, attr, value)
    return groups


def structure(groups):
    out = []
    for g in groups:
        eqs = []
        for eq in g.equations:
            par = dict((k, (bool(v) if isinstance(v, bool) else float(v))) for k, v in vars(eq).items()
                       if k not in SKIP_ATTRS and not k.startswith('_') and isinstance(v, (bool, int, float)))
            eqs.append(dict(cls=type(eq).__name__, dest=eq.dest, sources=list(eq.sources or []), params=par))
        out.append(dict(real=bool(g.real), equations=eqs))
    return out


@pytest.mark.parametrize('case', CASES)
def test_group_list_equals_the_reference(case):
    """same groups, same order inside a group, same `real` flags, same parameters -- field by field"""
    g = load_golden(case + '.npz')
    want = json.loads(str(g['structure']))
    got = structure(equations_of(g))
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a['real'] == b['real'], (k, a['real'])
        assert [e['cls'] for e in a['equations']] == [e['cls'] for e in b['equations']], k
        for ea, eb in zip(a['equations'], b['equations']):
            assert ea['dest'] == eb['dest'] and ea['sources'] == eb['sources'], (k, ea, eb)
            assert ea['params'] == eb['params'], (k, ea['cls'], ea['params'], eb['params'])


def test_every_option_combination_builds():
    """the guard is gone: all eight combinations (and summation density, under which the delta-SPH density terms are
    dropped as in the reference) give the expected equations in the expected places"""
    from pysph_amd.scheme import WCSPHScheme
    for delta_sph in (False, True):
        for nu in (0.0, 0.01):
            for update_h in (False, True):
                for sd in (False, True):
                    s = WCSPHScheme(['fluid'], ['wall'], dim=2, rho0=1.0, c0=10.0, h0=0.1, hdx=1.3, alpha=0.2,
                                    delta_sph=delta_sph, nu=nu, update_h=update_h, summation_density=sd)
                    groups = s.get_equations()
                    names = [[type(e).__name__ for e in g.equations] for g in groups]
                    flat = sum(names, [])
                    assert ('GradientCorrectionPreStep' in flat) == (delta_sph and not sd)
                    assert ('ContinuityEquationDeltaSPH' in flat) == (delta_sph and not sd)
                    assert ('MomentumEquationDeltaSPH' in flat) == delta_sph
                    assert ('LaminarViscosityDeltaSPH' in flat) == (delta_sph and nu > 0)
                    assert ('LaminarViscosity' in flat) == (not delta_sph and nu > 0)
                    assert ('UpdateSmoothingLengthFerrari' in names[-1]) == update_h
                    rates = groups[-2 if update_h else -1]
                    assert type(rates.equations[-1]).__name__ == 'XSPHCorrection'
                    if nu > 0:
                        assert type(rates.equations[-2]).__name__.startswith('LaminarViscosity')
                    mom = [e for e in rates.equations if type(e).__name__ == 'MomentumEquation'][0]
                    assert mom.alpha == (0.0 if delta_sph else 0.2)


def test_setup_properties_adds_the_strided_properties():
    from pysph_amd.particle_array import get_particle_array_wcsph
    from pysph_amd.scheme import WCSPHScheme
    pas = [get_particle_array_wcsph(name=n, x=np.zeros(5)) for n in ('fluid', 'wall')]
    WCSPHScheme(['fluid'], ['wall'], dim=3, rho0=1.0, c0=10.0, h0=0.1, hdx=1.3).setup_properties(pas)
    assert all('m_mat' not in pa.properties for pa in pas)
    WCSPHScheme(['fluid'], ['wall'], dim=3, rho0=1.0, c0=10.0, h0=0.1, hdx=1.3, delta_sph=True).setup_properties(pas)
    for pa in pas:
        assert pa.properties['m_mat'].size == 45 and pa.stride['m_mat'] == 9
        assert pa.properties['gradrho'].size == 15 and pa.stride['gradrho'] == 3


def test_resolve_equation_knows_the_eight_names():
    from pysph_amd import equations as E
    for name, kind in NAMES.items():
        assert name in E.EQUATION_TABLE and E.EQUATION_TABLE[name][0] == kind
    g = load_golden('opt_dsph3d.npz')
    seen = set()
    for grp in equations_of(g):
        for eq in grp.equations:
            kind, vals, dprops, sprops = E.resolve_equation(eq)
            seen.add(kind)
            assert len(vals) == len(E.EQUATION_TABLE[type(eq).__name__][1])
    assert set((22, 23, 24, 25, 26, 28, 29)) <= seen
    eq = E.LaminarViscosity(dest='fluid', sources=['fluid'], nu=0.5)
    assert E.resolve_equation(eq)[:2] == (27, [0.5, 0.01])
    assert E.resolve_equation(E.UpdateSmoothingLengthFerrari('fluid', None, dim=2, hdx=1.3))[1] == [0.5, 1.3]
    assert E.EQ_UPDATE_H_FERRARI in E.NO_SOURCE_KINDS


def test_kind_constants_equal_the_header():
    """parsed as tests/test_cabi.py parses it"""
    from pysph_amd import equations as E
    hdr = open(os.path.join(REPO, 'include', 'sphhip.h')).read()
    ids = dict((c, int(v)) for c, v in re.findall(r'(SPH_EQ_[A-Z0-9_]+)\s*=\s*(\d+)', hdr))
    want = {'SPH_EQ_GRADIENT_CORRECTION_PRESTEP': 22, 'SPH_EQ_GRADIENT_CORRECTION': 23,
            'SPH_EQ_CONTINUITY_DELTA_SPH_PRESTEP': 24, 'SPH_EQ_CONTINUITY_DELTA_SPH': 25,
            'SPH_EQ_MOMENTUM_DELTA_SPH': 26, 'SPH_EQ_LAMINAR_VISCOSITY': 27,
            'SPH_EQ_LAMINAR_VISCOSITY_DELTA_SPH': 28, 'SPH_EQ_UPDATE_H_FERRARI': 29}
    for cname, val in want.items():
        assert ids[cname] == val, cname
        assert getattr(E, cname[4:]) == val, cname
    assert len(set(ids.values())) == len(ids)           # no id twice


def test_component_columns_are_built_in_properties():
    """m_mat and gradrho live on the device as columns with ids of their own: they need none of the user slots"""
    from pysph_amd import device as dev
    hdr = open(os.path.join(REPO, 'include', 'sphhip.h')).read()
    body = re.sub(r'/\*.*?\*/', '', hdr[hdr.index('enum sph_prop {'):hdr.index('SPH_USER0,')], flags=re.S)
    names = [n.strip() for n in body.split('{')[1].split(',') if n.strip()]
    cols = ['m_mat__%d' % k for k in range(9)] + ['gradrho__%d' % k for k in range(3)]
    assert [n for n in names[-12:]] == ['SPH_MMAT%d' % k for k in range(9)] + ['SPH_GRADRHO%d' % k for k in range(3)]
    assert [dev.prop_id(c) for c in cols] == list(range(len(names) - 12, len(names)))


def test_example_takes_the_options():
    from pysph_amd.examples import dam_break_3d as db
    plain = [[type(e).__name__ for e in g.equations] for g in db.create_scheme(0.1).get_equations()]
    assert len(plain) == 2 and 'LaminarViscosity' not in plain[1]
    s = db.create_scheme(0.1, delta_sph=True, nu=0.01, update_h=True)
    names = [[type(e).__name__ for e in g.equations] for g in s.get_equations()]
    assert len(names) == 5 and names[1] == ['GradientCorrectionPreStep']
    assert 'LaminarViscosityDeltaSPH' in names[3] and names[4] == ['UpdateSmoothingLengthFerrari']


def test_golden_margins_hold():
    """what the generator asserted, stored with the vectors: no pair of the fp64 cases within 1e-6 of the threshold,
    5e-4 in the gap case, both branches taken by a tenth of the pairs"""
    for case, margin in (('opt_dsph3d', 1e-6), ('opt_dsph2d_tank', 1e-6), ('opt_dsph3d_gap', 5e-4), ('opt_singular', 1e-6)):
        g = load_golden(case + '.npz')
        assert float(g['meta/margin']) >= margin
        if case != 'opt_singular':
            n, k = int(g['meta/n_pairs']), int(g['meta/n_corrected'])
            assert min(k, n - k) * 10 >= n
    assert float(load_golden('opt_dsph3d.npz')['meta/second_margin']) >= 1e-6
