"""Drop-in check on the CPU: the backend consumes the REFERENCE's own objects.

The reference's ``WCSPHScheme`` / ``TVFScheme`` / kernel classes / ``AccelerationEval``
were marshalled by the same code path ``HipAccelerationEval`` uses (``_CGroup``)
and the result stored in tests/golden/reference_pins.json
(tests/golden/make_golden.py reference_pins): the C-ABI structs marshalled from
this package's specification classes must equal them.
"""
import json
import os

import numpy as np

from conftest import GOLDEN


def _pins():
    with open(os.path.join(GOLDEN, 'reference_pins.json')) as f:
        return json.load(f)


def _plain(x):
    """tuples -> lists, as the stored JSON holds them"""
    return json.loads(json.dumps(x))


def _marshal(groups, arrays):
    from pysph_amd.acceleration_eval import _CGroup
    ids = dict((pa.name, i) for i, pa in enumerate(arrays))
    amap = dict((pa.name, pa) for pa in arrays)
    out = []
    for g in groups:
        cg = _CGroup(g, ids, amap)
        cg.refresh_range()
        eqs = []
        for u in cg.units:          # one unit per destination, in order
            for i in range(u.cg.neq):
                e = u.ceqs[i]
                eqs.append((e.kind, e.dest, e.nsrc, list(e.src)[:e.nsrc],
                            [e.par[k] for k in range(16)]))
        u0 = cg.units[0]
        out.append((u0.cg.real, u0.cg.start_idx, u0.cg.stop_idx, eqs))
    return out


def test_reference_wcsph_scheme_marshals_identically():
    from pysph_amd.scheme import WCSPHScheme
    from pysph_amd.kernels import WendlandQuintic, kernel_id
    from pysph_amd.examples import dam_break_3d as db
    ref = _pins()['wcsph_scheme']
    arrays = db.create_particles(0.2)
    kw = dict(dim=3, rho0=db.ro, c0=db.c0, h0=0.26, hdx=1.3, gz=-9.81,
              alpha=db.alpha, beta=db.beta, gamma=db.gamma, hg_correction=True,
              tensile_correction=False)
    mine = WCSPHScheme(['fluid'], ['boundary', 'obstacle'], **kw).get_equations()
    assert ref['marshal'] == _plain(_marshal(mine, arrays))
    mk, rk = WendlandQuintic(dim=3), ref['kernel']
    assert rk['id'] == kernel_id(mk)
    assert (rk['fac'], rk['radius_scale'], rk['deltap'], rk['dim']) == \
        (mk.fac, mk.radius_scale, mk.get_deltap(), mk.dim)


def test_reference_tvf_scheme_marshals_identically():
    from pysph_amd.scheme import TVFScheme
    from pysph_amd.particle_array import get_particle_array_tvf_fluid
    pa = get_particle_array_tvf_fluid(name='fluid', x=np.zeros(4))
    kw = dict(dim=3, rho0=1.0, c0=10.0, nu=0.01, p0=100.0, pb=100.0, h0=0.1,
              gx=0.1, alpha=0.2)
    mine = TVFScheme(['fluid'], [], **kw).get_equations()
    assert _pins()['tvf_scheme']['marshal'] == _plain(_marshal(mine, [pa]))


def test_reference_accelerationeval_is_accepted():
    """A real pysph AccelerationEval (equation_groups, kernel, particle_arrays)
    is what HipAccelerationEval reads; its MegaGroup order equals ours."""
    from pysph_amd.acceleration_eval import AccelerationEval
    from pysph_amd.scheme import WCSPHScheme
    from pysph_amd.kernels import WendlandQuintic
    from pysph_amd.examples import dam_break_3d as db
    ref = _pins()['acceleration_eval']
    arrays = db.create_particles(0.2)
    kw = dict(dim=3, rho0=db.ro, c0=db.c0, h0=0.26, hdx=1.3, gz=-9.81,
              alpha=db.alpha, beta=db.beta, gamma=db.gamma, hg_correction=True)
    mine = AccelerationEval(arrays, WCSPHScheme(['fluid'], ['boundary', 'obstacle'],
                                                **kw).get_equations(),
                            WendlandQuintic(dim=3))
    assert len(ref['mega_groups']) == len(mine.mega_groups)
    for rg, mg in zip(ref['mega_groups'], mine.mega_groups):
        assert list(rg.keys()) == list(mg.data.keys())
        for dest in rg:
            r_no, r_src, r_all = rg[dest]
            m_no, m_src, m_all = mg.data[dest]
            assert r_no == [e.name for e in m_no.equations]
            assert list(r_src.keys()) == list(m_src.keys())
            for src in r_src:
                assert r_src[src] == [e.name for e in m_src[src].equations]
            assert r_all == [e.name for e in m_all.equations]
    assert ref['marshal'] == _plain(_marshal(mine.equation_groups, arrays))
