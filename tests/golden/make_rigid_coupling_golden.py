#!/usr/bin/env python
"""Generate tests/golden/rigid_coupling.npz from the REFERENCE's own classes.

Run in the build container only (needs the reference's sources):

    python tests/golden/make_rigid_coupling_golden.py

pysph/sph/rigid_body.py's ``BodyForce``, ``NumberDensity``,
``PressureRigidBody``, ``ViscosityRigidBody``, ``AkinciRigidFluidCoupling`` and
``LiuFluidForce`` are imported under the stubs of oracle/_stubs (as
make_golden.py does) and their Python bodies run by oracle/py_eval.py on a
small fluid-over-solid lattice: inputs and outputs are recorded, numbers only.
tests/test_scatter.py runs the bodies of pysph_amd/rigid_body.py the same way
on the recorded inputs (``arrays_from``, ``equations`` and ``OUTPUTS`` below
are shared with it).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))

# the properties recorded: inputs of the six classes, and what they write
INPUTS = ('x', 'y', 'z', 'h', 'u', 'v', 'w', 'm', 'rho', 'p', 'V', 'fx', 'fy', 'fz', 'au', 'av', 'aw')
OUTPUTS = {'fluid': ('au', 'av', 'aw'), 'solid': ('V', 'fx', 'fy', 'fz')}


def equations(mod):
    """the two groups, with the classes of `mod` (the reference's module or pysph_amd.rigid_body)"""
    from pysph_amd.equations import Group
    return [Group(equations=[mod.BodyForce(dest='solid', sources=None, gx=0.3, gy=-9.81, gz=0.1),
                             mod.NumberDensity(dest='solid', sources=['solid'])]),
            Group(equations=[mod.AkinciRigidFluidCoupling(dest='fluid', sources=['solid'], fluid_rho=1.2),
                             mod.PressureRigidBody(dest='fluid', sources=['solid'], rho0=1.1),
                             mod.ViscosityRigidBody(dest='fluid', sources=['solid'], rho0=1.1, nu=0.05),
                             mod.LiuFluidForce(dest='fluid', sources=['solid'])])]


def arrays_from(g, which):
    from pysph_amd.particle_array import ParticleArray
    out = []
    for name in ('fluid', 'solid'):
        props = dict((key.split('/')[2], g[key].copy()) for key in g.files
                     if key.startswith('%s/%s/' % (which, name)))
        out.append(ParticleArray(name=name, **props))
    return out


def main():
    sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]
    from oracle.ref_driver import setup_reference_imports
    setup_reference_imports()
    import types
    if 'pysph.base.reduce_array' not in sys.modules:
        # only RigidBodyMoments.reduce (not run here) calls it; the real module needs the cyarray extension
        m = types.ModuleType('pysph.base.reduce_array')
        m.parallel_reduce_array = m.serial_reduce_array = lambda *a, **k: None
        sys.modules['pysph.base.reduce_array'] = m
    import pysph.sph.rigid_body as ref
    from oracle import oracle as orc
    from oracle.py_eval import PyEval
    from pysph_amd import kernels as K
    from test_scatter import base_case
    arrays = base_case(0.15, seed=21)
    out = {}
    for pa in arrays:
        for k in INPUTS:
            out['in/%s/%s' % (pa.name, k)] = pa.properties[k].copy()
    kernel = K.CubicSpline(dim=3)
    nnps = orc.OracleNNPS(3, arrays, radius_scale=kernel.radius_scale)
    nnps.update()
    PyEval(arrays, equations(ref), kernel, nnps).compute(0.0, 1e-3)
    for pa in arrays:
        for k in OUTPUTS[pa.name]:
            out['out/%s/%s' % (pa.name, k)] = pa.properties[k].copy()
    path = os.path.join(HERE, 'rigid_coupling.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
