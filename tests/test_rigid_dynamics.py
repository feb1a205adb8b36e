"""Rigid-body dynamics: RigidBodyMoments, RigidBodyMotion, RK2StepRigidBody / EulerStepRigidBody.

The reference is tests/golden/rigid_dynamics.npz -- the reference's own classes driven by hand
(tests/golden/make_rigid_dynamics_golden.py) -- and, at the shapes where the moment kernels can go wrong, the formulae
evaluated with mpmath at 50 digits.  Tolerance: 1e-10 of the largest magnitude within the vector or tensor compared
(per body), the project's own; the pure sums total_mass and force are held to n 2^-52 sum |term| per body against
math.fsum, which bounds any summation order of n doubles.
"""
import math
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

if GOLDEN not in sys.path:
    sys.path.append(GOLDEN)
import make_rigid_dynamics_golden as mk  # noqa: E402

from pysph_amd.particle_array import RIGID_BODY_CONSTANTS  # noqa: E402

TOL = 1e-10
STATE = mk.STATE
WIDTH = dict(RIGID_BODY_CONSTANTS)
assert tuple(WIDTH) == STATE
MOMENT_FIELDS = ('total_mass', 'cm', 'mi', 'force', 'ac', 'torque', 'omega_dot')


def golden():
    return np.load(os.path.join(GOLDEN, 'rigid_dynamics.npz'))


def body_err(got, ref, width, scale=None):
    """largest error of a per-body field, per body relative to the largest magnitude within that body's vector / tensor"""
    got, ref = np.asarray(got, dtype=float).reshape(-1, width), np.asarray(ref, dtype=float).reshape(-1, width)
    assert got.shape == ref.shape
    mag = np.abs(ref).max(axis=1) if scale is None else np.asarray(scale, dtype=float)
    zero = mag == 0                          # a vector that is exactly zero (vc0 before the first step) must be so
    assert np.all(got[zero] == 0.0)
    if np.all(zero):
        return 0.0
    return float((np.abs(got - ref).max(axis=1)[~zero] / mag[~zero]).max())


def check_state(pa, ref, fields, label, tol=TOL):
    for k in fields:
        want = ref[k] if isinstance(ref, dict) else getattr(ref, k)
        w = 9 if k == 'mi' else WIDTH[k]        # the inertia tensor proper; slots 9..15 are temporaries of the reference
        got = pa.constants[k].reshape(-1, WIDTH[k])[:, :w]
        e = body_err(got, np.asarray(want).reshape(-1, WIDTH[k])[:, :w], w)
        print('%s %s err %.3e' % (label, k, e))
        assert e < tol, (label, k, e)


def field_err(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def sum_bound_check(pa, label):
    """total_mass and force of every body against math.fsum, within n 2^-52 sum |term|"""
    ids = pa.body_id
    for b in range(int(pa.num_body[0])):
        rows = np.nonzero(ids == b)[0]
        for name, terms, got in (('total_mass', pa.m[rows], pa.total_mass[b]), ('fx', pa.fx[rows], pa.force[3 * b]),
                                 ('fy', pa.fy[rows], pa.force[3 * b + 1]), ('fz', pa.fz[rows], pa.force[3 * b + 2])):
            bound = rows.size * 2.0 ** -52 * math.fsum(abs(float(v)) for v in terms)
            err = abs(float(got) - math.fsum(float(v) for v in terms))
            assert err <= bound, (label, b, name, err, bound)


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------
def lattice_bodies(sizes, seed=3, spacing=0.05, pitch=1.0):
    """one array of len(sizes) bodies: body b is the first sizes[b] points of a jittered cubic lattice; the bodies
    sit on a coarse cubic grid of `pitch` centred on the origin (so that the parallel-axis subtraction costs few
    digits); masses, forces, omega and vc from a seeded generator"""
    from pysph_amd.particle_array import get_particle_array_rigid_body
    rng = np.random.default_rng(seed)
    G = max(2, int(math.ceil(len(sizes) ** (1.0 / 3.0) - 1e-9)))
    xs, ys, zs, ids = [], [], [], []
    for b, k in enumerate(sizes):
        side = max(2, int(math.ceil(k ** (1.0 / 3.0) - 1e-9)))
        c = np.arange(side) * spacing
        lx, ly, lz = [a.ravel()[:k] for a in np.meshgrid(c, c, c, indexing='ij')]
        origin = (np.array([b % G, (b // G) % G, b // (G * G)]) - 0.5 * (G - 1)) * pitch
        jit = rng.uniform(-0.2, 0.2, (3, k)) * spacing
        xs.append(lx + origin[0] + jit[0]); ys.append(ly + origin[1] + jit[1]); zs.append(lz + origin[2] + jit[2])
        ids.append(np.full(k, b))
    x, y, z = np.concatenate(xs), np.concatenate(ys), np.concatenate(zs)
    n, nb = x.size, len(sizes)
    pa = get_particle_array_rigid_body(name='body', x=x, y=y, z=z, m=rng.uniform(0.5, 2.0, n), h=1.3 * spacing * np.ones(n),
                                       body_id=np.concatenate(ids), fx=rng.normal(0.0, 5.0, n),
                                       fy=rng.normal(-3.0, 5.0, n), fz=rng.normal(1.0, 5.0, n))
    pa.omega[:] = rng.normal(0.0, 2.0, 3 * nb)
    pa.vc[:] = rng.normal(0.0, 1.0, 3 * nb)
    return pa


def take_rows(pa, rows, nreal=None):
    """a new array holding the given rows of `pa` (its body state copied); rows >= nreal are tagged as ghosts"""
    from pysph_amd.particle_array import get_particle_array_rigid_body
    props = dict((k, v[rows].copy()) for k, v in pa.properties.items())
    out = get_particle_array_rigid_body(name=pa.name, **props)
    for k in STATE:
        out.constants[k][:] = pa.constants[k]
    if nreal is not None:
        out.tag[nreal:] = 2
        out.set_num_real_particles(nreal)
    return out


_MP = {}


def mp_moments(pa):
    """every field RigidBodyMoments writes, from the reference formulae at 50 digits (dict of float64 arrays)"""
    key = id(pa)
    if key in _MP:
        return _MP[key]
    import mpmath as mp
    mp.mp.dps = 50
    f = mp.mpf
    nb = int(pa.num_body[0])
    out = dict((k, np.zeros(WIDTH[k] * nb)) for k in MOMENT_FIELDS)
    for b in range(nb):
        rows = np.nonzero(pa.body_id == b)[0]
        P = [(f(float(pa.x[i])), f(float(pa.y[i])), f(float(pa.z[i])), f(float(pa.m[i])), f(float(pa.fx[i])),
              f(float(pa.fy[i])), f(float(pa.fz[i]))) for i in rows]
        M = mp.fsum(p[3] for p in P)
        cx, cy, cz = [mp.fsum(p[3] * p[a] for p in P) / M for a in range(3)]
        ixx = mp.fsum(p[3] * (p[1] ** 2 + p[2] ** 2) for p in P) - (cy * cy + cz * cz) * M
        iyy = mp.fsum(p[3] * (p[0] ** 2 + p[2] ** 2) for p in P) - (cx * cx + cz * cz) * M
        izz = mp.fsum(p[3] * (p[0] ** 2 + p[1] ** 2) for p in P) - (cx * cx + cy * cy) * M
        ixy = -mp.fsum(p[3] * p[0] * p[1] for p in P) + cx * cy * M
        ixz = -mp.fsum(p[3] * p[0] * p[2] for p in P) + cx * cz * M
        iyz = -mp.fsum(p[3] * p[1] * p[2] for p in P) + cy * cz * M
        F = [mp.fsum(p[4 + a] for p in P) for a in range(3)]
        T = [mp.fsum(p[1] * p[6] - p[2] * p[5] for p in P) - (cy * F[2] - cz * F[1]),
             mp.fsum(p[2] * p[4] - p[0] * p[6] for p in P) - (cz * F[0] - cx * F[2]),
             mp.fsum(p[0] * p[5] - p[1] * p[4] for p in P) - (cx * F[1] - cy * F[0])]
        I = mp.matrix([[ixx, ixy, ixz], [ixy, iyy, iyz], [ixz, iyz, izz]])
        w = mp.matrix([f(float(v)) for v in pa.omega[3 * b:3 * b + 3]])
        L = I * w
        rhs = mp.matrix([T[0] - (w[1] * L[2] - w[2] * L[1]), T[1] - (w[2] * L[0] - w[0] * L[2]),
                         T[2] - (w[0] * L[1] - w[1] * L[0])])
        od = mp.lu_solve(I, rhs)
        out['total_mass'][b] = float(M)
        out['cm'][3 * b:3 * b + 3] = [float(cx), float(cy), float(cz)]
        out['mi'][16 * b:16 * b + 9] = [float(v) for v in (ixx, ixy, ixz, ixy, iyy, iyz, ixz, iyz, izz)]
        out['force'][3 * b:3 * b + 3] = [float(v) for v in F]
        out['ac'][3 * b:3 * b + 3] = [float(v / M) for v in F]
        out['torque'][3 * b:3 * b + 3] = [float(v) for v in T]
        out['omega_dot'][3 * b:3 * b + 3] = [float(od[a]) for a in range(3)]
    _MP[key] = out
    return out


def chunk_sizes():
    from pysph_amd import device as dev
    C = int(dev.load_library().sph_rigid_chunk())
    assert C % 64 == 0 and C >= 64
    return [4, 63, 64, 65, C - 1, C, C + 1, 2 * C + 1]


_CASE = {}


def edge_case():
    """the array of GPU test 1 and its mpmath reference, made once"""
    if not _CASE:
        pa = lattice_bodies(chunk_sizes())
        _CASE['pa'] = pa
        _CASE['ref'] = mp_moments(pa)
    return _CASE['pa'], _CASE['ref']


def device_moments(pa, ctx=None):
    """push, sph_rigid_moments, pull of the body state; returns the helper"""
    from pysph_amd import device as dev
    h = dev.attach(pa, ctx or dev.HipContext(0))
    h.push()
    h.rigid_setup()
    h.rigid_moments()
    h.pull(*STATE)
    return h


def host_moments(pa):
    from pysph_amd import rigid_body as rb
    rb.RigidBodyMoments(dest=pa.name, sources=None).reduce(pa, 0.0, 0.0)


def clone(pa):
    return take_rows(pa, np.arange(pa.get_number_of_particles()), pa.get_number_of_particles(True))


def dynamics_equations(mod=None, gravity=None, **motion_kw):
    from pysph_amd.equations import Group
    from pysph_amd import rigid_body as rb
    mod = mod or rb
    eqs = []
    if gravity is not None:
        eqs.append(Group(equations=[rb.BodyForce(dest='body', sources=None, gy=gravity)]))
    eqs.append(Group(equations=[mod.RigidBodyMoments(dest='body', sources=None)]))
    eqs.append(Group(equations=[mod.RigidBodyMotion(dest='body', sources=None)], **motion_kw))
    return eqs


def make_eval(pa, eqs, sync='manual', integrator=None):
    from pysph_amd import device as dev
    from pysph_amd import kernels as K
    from pysph_amd.acceleration_eval import AccelerationEval, SPHCompiler
    from pysph_amd.integrator import setup_integrator
    from pysph_amd.nnps import HipNNPS
    ctx = dev.HipContext(0)
    kernel = K.CubicSpline(dim=3)
    a_eval = AccelerationEval([pa], eqs, kernel)
    SPHCompiler(a_eval, ctx=ctx, sync=sync).compile()
    if sync == 'manual':
        dev.attach(pa, ctx).push()
    nnps = HipNNPS(3, [pa], radius_scale=kernel.radius_scale, ctx=ctx, sync=(sync == 'auto'))
    a_eval.set_nnps(nnps)
    if integrator is not None:
        setup_integrator(integrator, a_eval, nnps)
    return a_eval, nnps, ctx


def prebuild():
    """the generated families of the GPU tests below, built without a GPU (__graft_entry__.build())"""
    from pysph_amd import codegen
    from pysph_amd import kernels as K
    from pysph_amd.acceleration_eval import AccelerationEval, _CGroup
    from pysph_amd.examples import body_in_tank as B

    def plan(arrays, eqs):
        kernel = K.CubicSpline(dim=3)
        a = AccelerationEval(arrays, eqs, kernel)
        ids = dict((pa.name, i) for i, pa in enumerate(arrays))
        amap = dict((pa.name, pa) for pa in arrays)
        return sum(hasattr(u, 'fam') for g in a.equation_groups for u in _CGroup(g, ids, amap, K.kernel_id(kernel)).units)

    def every():
        return plan([lattice_bodies([8, 8])], dynamics_equations(gravity=-9.81)) + \
            plan(B.create_particles(0.1, free=True), B.create_equations(0.1, free=True))
    codegen.DEFERRED = []
    every()
    codegen.build_deferred()
    return every()


# ---------------------------------------------------------------------------
# CPU tests
# ---------------------------------------------------------------------------
def test_host_twins_reproduce_the_golden_outputs():
    from pysph_amd import rigid_body as rb
    g = golden()
    pa = mk.array_from(g)
    out = {}
    mk.drive(rb, pa, out)
    checked = 0
    for which, props in (('reduce', ()), ('motion', ('u', 'v', 'w')), ('steps', ('x', 'y', 'z', 'u', 'v', 'w', 'x0', 'y0', 'z0'))):
        for k in props:
            e = field_err(out['%s/%s' % (which, k)], g['%s/%s' % (which, k)])
            assert e < TOL, (which, k, e)
            checked += 1
        for k in STATE:
            w = WIDTH[k]
            e = body_err(out['%s/%s' % (which, k)], g['%s/%s' % (which, k)], w)
            print('%s %s err %.3e' % (which, k, e))
            assert e < TOL, (which, k, e)
            checked += 1
    assert checked == 12 + 33
    # the recorded run did something: bodies moved and turned
    assert not np.array_equal(g['steps/x'], g['in/x']) and not np.array_equal(g['steps/omega'], g['in/omega'])


def test_euler_stepper_twin():
    """EulerStepRigidBody.stage1: vc, omega by their rates, positions by the velocities, once per body"""
    from pysph_amd import rigid_body as rb
    pa = mk.array_from(golden(), 'in')
    host_moments(pa)
    mk.call(rb.RigidBodyMotion(dest='body', sources=None), 'initialize', pa)
    before = dict((k, pa.constants[k].copy()) for k in ('vc', 'omega'))
    x0 = pa.x.copy()
    mk.call(rb.EulerStepRigidBody(), 'stage1', pa, 0.25)
    assert np.allclose(pa.vc, before['vc'] + 0.25 * pa.ac, rtol=0, atol=1e-15 * np.abs(pa.vc).max())
    assert np.allclose(pa.omega, before['omega'] + 0.25 * pa.omega_dot, rtol=0, atol=1e-15 * np.abs(pa.omega).max())
    assert np.array_equal(pa.x, x0 + 0.25 * pa.u)


def test_rigid_body_array_factory():
    from pysph_amd.particle_array import get_particle_array_rigid_body
    x = np.linspace(0.0, 1.0, 7)
    pa = get_particle_array_rigid_body(name='b', x=x, body_id=np.array([0, 0, 1, 1, 2, 2, 2]))
    for p in ('au', 'av', 'aw', 'V', 'fx', 'fy', 'fz', 'x0', 'y0', 'z0', 'tang_disp_x', 'tang_velocity_z', 'rad_s',
              'nx', 'ny', 'nz', 'body_id', 'x', 'm', 'h', 'rho', 'tag'):
        assert pa.properties[p].size == 7, p
    assert pa.body_id.dtype.kind == 'i'
    assert pa.num_body.dtype.kind == 'i' and pa.num_body.size == 1 and pa.num_body[0] == 3
    for k in STATE:
        assert pa.constants[k].dtype == np.float64 and pa.constants[k].size == WIDTH[k] * 3, k
    assert 'body_id' in pa.output_property_arrays and 'fx' in pa.output_property_arrays
    for _ in range(int(pa.num_body[0])):       # what the reference's reduce does with it
        pass
    one = get_particle_array_rigid_body(name='b', x=x)
    assert one.num_body[0] == 1 and np.all(one.body_id == 0) and one.cm.size == 3 and one.mi.size == 16
    # add_constant: float unless told otherwise
    one.add_constant('k', [1, 2])
    one.add_constant('j', [1, 2], type='int')
    assert one.k.dtype == np.float64 and one.j.dtype.kind == 'i'


def test_body_index_and_its_refusals():
    from pysph_amd.rigid_body import body_index
    ids = np.array([2, 0, 1, 0, 2, 2, 1])
    order, start = body_index(ids, 3)
    assert list(order) == [1, 3, 2, 6, 0, 4, 5] and list(start) == [0, 2, 4, 7]
    with pytest.raises(ValueError, match='no particles'):
        body_index(np.array([0, 0, 2, 2]), 3)           # a gap in the ids
    with pytest.raises(ValueError, match='outside'):
        body_index(np.array([0, -1, 1]), 2)
    with pytest.raises(ValueError, match='outside'):
        body_index(np.array([0, 1, 2]), 2)


def test_dynamics_equations_plan_off_the_merged_path():
    """the two equations become units of their own, their group is no plain leaf, reduce is not a host hook"""
    from pysph_amd import kernels as K
    from pysph_amd.acceleration_eval import AccelerationEval, _CGroup, _RigidUnit, _plain_leaf
    pa = lattice_bodies([8, 8])
    a = AccelerationEval([pa], dynamics_equations(), K.CubicSpline(dim=3))
    groups = [_CGroup(g, {'body': 0}, {'body': pa}, 1) for g in a.equation_groups]
    assert [len(c.units) for c in groups] == [0, 1] and len(groups[0].moments) == 1
    assert isinstance(groups[1].units[0], _RigidUnit) and groups[1].units[0].kind == 'RigidBodyMotion'
    assert not any(_plain_leaf(g, c) for g, c in zip(a.equation_groups, groups))
    assert 'body_id' in groups[0].inputs['body'] and groups[1].outputs_exact['body'] == {'u', 'v', 'w'}
    # a missing constant is reported like a missing property
    del pa.constants['omega']
    with pytest.raises(RuntimeError, match='omega'):
        AccelerationEval([pa], dynamics_equations(), K.CubicSpline(dim=3))


# ---------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('layout', ['contiguous', 'interleaved', 'ghost_rows'])
def test_moments_at_the_chunk_edges(layout):
    """bodies of 4, 63, 64, 65, C-1, C, C+1, 2C+1 particles against mpmath; the same particles with their rows
    shuffled (bodies interleaved), and with trailing rows that are not real"""
    base, ref = edge_case()
    n = base.get_number_of_particles()
    if layout == 'contiguous':
        pa = clone(base)
    elif layout == 'interleaved':
        pa = take_rows(base, np.random.default_rng(17).permutation(n))
    else:
        pa = take_rows(base, np.arange(n), nreal=n - 300)
        assert pa.get_number_of_particles(True) == n - 300
    device_moments(pa)
    check_state(pa, ref, MOMENT_FIELDS, layout)
    sum_bound_check(pa, layout)
    assert np.array_equal(pa.omega, base.omega) and np.array_equal(pa.vc, base.vc)   # inputs are left alone


@pytest.mark.gpu
def test_moments_of_a_thousand_small_bodies():
    pa = lattice_bodies([8] * 1000, seed=9, pitch=0.4)
    ref = clone(pa)
    host_moments(ref)
    device_moments(pa)
    check_state(pa, ref, MOMENT_FIELDS, '1000x8')
    sum_bound_check(pa, '1000x8')


@pytest.mark.gpu
def test_moments_are_bit_identical():
    """from call to call, and for a body alone in an array or next to others"""
    base, _ = edge_case()
    pa = clone(base)
    h = device_moments(pa)
    first = dict((k, pa.constants[k].copy()) for k in STATE)
    h.rigid_moments()
    h.pull(*STATE)
    for k in STATE:
        assert np.array_equal(first[k], pa.constants[k]), k
    b = 3
    rows = np.nonzero(base.body_id == b)[0]
    assert rows.size == 65
    from pysph_amd.particle_array import get_particle_array_rigid_body
    props = dict((k, v[rows].copy()) for k, v in base.properties.items())
    props['body_id'][:] = 0
    alone = get_particle_array_rigid_body(name='body', **props)
    alone.omega[:] = base.omega[3 * b:3 * b + 3]
    alone.vc[:] = base.vc[3 * b:3 * b + 3]
    device_moments(alone)
    for k in MOMENT_FIELDS:
        w = WIDTH[k]
        assert np.array_equal(alone.constants[k], first[k][w * b:w * (b + 1)]), k


@pytest.mark.gpu
@pytest.mark.parametrize('how', ['spatial_order', 'align'])
def test_moments_follow_a_reordered_array(how):
    """the body index is rebuilt when the rows move on the device"""
    from pysph_amd import device as dev
    from pysph_amd.nnps import HipNNPS
    base, _ = edge_case()
    pa = take_rows(base, np.random.default_rng(23).permutation(base.get_number_of_particles()))
    ctx = dev.HipContext(0)
    h = device_moments(pa, ctx)
    first = dict((k, pa.constants[k].copy()) for k in STATE)
    ids_before = pa.body_id.copy()
    if how == 'spatial_order':
        nnps = HipNNPS(3, [pa], radius_scale=2.0, ctx=ctx, sync=False)
        nnps.update()
        nnps.spatially_order_particles(0)
    else:
        h.align(np.random.default_rng(29).permutation(pa.get_number_of_particles()))
    h.rigid_moments()
    h.pull()
    assert not np.array_equal(pa.body_id, ids_before)         # the rows did move
    check_state(pa, first, MOMENT_FIELDS, how)
    twin = clone(pa)
    host_moments(twin)
    check_state(pa, twin, MOMENT_FIELDS, how + ' twin')


@pytest.mark.gpu
def test_first_evaluation_reads_the_forces_on_the_device():
    """device-resident, no stepper: BodyForce writes fx fy fz on the device, and the FIRST moments of the evaluation
    -- the call that creates the body state -- sum those, not the host's (zero) columns"""
    grav = -9.81
    pa = lattice_bodies([27, 64, 300], seed=37)
    pa.fx[:], pa.fy[:], pa.fz[:] = 0.0, 0.0, 0.0
    a_eval, nnps, ctx = make_eval(pa, dynamics_equations(gravity=grav))
    a_eval.compute(0.0, 1e-3)
    assert np.all(pa.fy == 0.0)                  # the host was not touched
    pa.gpu.pull('force', 'ac', 'total_mass')
    for b in range(3):
        rows = np.nonzero(pa.body_id == b)[0]
        terms = [float(v) * grav for v in pa.m[rows]]
        bound = rows.size * 2.0 ** -52 * math.fsum(abs(v) for v in terms)
        assert abs(pa.force[3 * b + 1] - math.fsum(terms)) <= bound, (b, pa.force[3 * b + 1], math.fsum(terms))
        assert pa.force[3 * b] == 0.0 and pa.force[3 * b + 2] == 0.0
        assert abs(pa.ac[3 * b + 1] - grav) < TOL * abs(grav)


@pytest.mark.gpu
def test_body_state_created_after_a_device_reorder():
    """the rows are put in cell order on the device BEFORE the body state exists (the host keeps the old order): the
    bodies are those of the device's body_id column, which moved with its rows"""
    from pysph_amd import device as dev
    from pysph_amd.nnps import HipNNPS
    base, ref = edge_case()
    pa = take_rows(base, np.random.default_rng(41).permutation(base.get_number_of_particles()))
    ids_host = pa.body_id.copy()
    ctx = dev.HipContext(0)
    h = dev.attach(pa, ctx)
    h.push()
    nnps = HipNNPS(3, [pa], radius_scale=2.0, ctx=ctx, sync=False)
    nnps.update()
    nnps.spatially_order_particles(0)
    assert np.array_equal(pa.body_id, ids_host)              # device-resident: the host rows stayed
    h.rigid_setup()
    h.rigid_moments()
    h.pull(*STATE)
    check_state(pa, ref, MOMENT_FIELDS, 'setup after reorder')
    h.pull()
    assert not np.array_equal(pa.body_id, ids_host)           # the device rows had moved
    sum_bound_check(pa, 'setup after reorder')


@pytest.mark.gpu
@pytest.mark.parametrize('rows', ['all', 'range', 'real'])
def test_motion_matches_the_host_twin(rows):
    from pysph_amd import rigid_body as rb
    g = golden()
    pa = mk.array_from(g)
    for k in STATE:                       # the state RigidBodyMotion reads: what the recorded reduce left
        pa.constants[k][:] = g['reduce/%s' % k]
    n = pa.get_number_of_particles()
    lo, hi, kw = 0, n, dict(real=False)
    if rows == 'range':
        lo, hi, kw = 10, 300, dict(real=False, start_idx=10, stop_idx=300)
    elif rows == 'real':
        hi, kw = n - 50, dict(real=True)
        pa.tag[hi:] = 2
        pa.set_num_real_particles(hi)
    pa.u[:], pa.v[:], pa.w[:] = 7.0, 8.0, 9.0
    from pysph_amd.equations import Group
    a_eval, nnps, ctx = make_eval(pa, [Group(equations=[rb.RigidBodyMotion(dest='body', sources=None)], **kw)])
    a_eval.compute(0.0, mk.DT)
    pa.gpu.pull('u', 'v', 'w')
    for k in 'uvw':
        got, want = pa.properties[k], g['motion/%s' % k]
        assert field_err(got[lo:hi], want[lo:hi]) < TOL, k
        assert np.all(got[:lo] == {'u': 7.0, 'v': 8.0, 'w': 9.0}[k]) and np.all(got[hi:] == {'u': 7.0, 'v': 8.0, 'w': 9.0}[k])


@pytest.mark.gpu
@pytest.mark.parametrize('sync', ['manual', 'auto'])
def test_golden_sequence_on_the_device(sync):
    """reduce, motion and two EPEC steps through AccelerationEval + EPECIntegrator(body=RK2StepRigidBody())"""
    from pysph_amd import rigid_body as rb
    from pysph_amd.integrator import EPECIntegrator
    g = golden()
    pa = mk.array_from(g)
    integ = EPECIntegrator(body=rb.RK2StepRigidBody())
    a_eval, nnps, ctx = make_eval(pa, dynamics_equations(real=False), sync=sync, integrator=integ)
    a_eval.compute(0.0, mk.DT)
    if sync == 'manual':
        pa.gpu.pull()
    check_state(pa, dict((k, g['reduce/%s' % k]) for k in STATE), MOMENT_FIELDS, 'reduce ' + sync)
    for k in 'uvw':
        assert field_err(pa.properties[k], g['motion/%s' % k]) < TOL, k
    t = 0.0
    for _ in range(mk.NSTEPS):
        integ.step(t, mk.DT)
        t += mk.DT
    if sync == 'manual':
        assert np.array_equal(pa.x, g['in/x'])         # the host was not touched
        pa.gpu.pull()
    for k in ('x', 'y', 'z', 'u', 'v', 'w', 'x0', 'y0', 'z0'):
        e = field_err(pa.properties[k], g['steps/%s' % k])
        print('steps %s err %.3e' % (k, e))
        assert e < TOL, (k, e)
    check_state(pa, dict((k, g['steps/%s' % k]) for k in STATE), STATE, 'steps ' + sync)


@pytest.mark.gpu
def test_free_fall_is_exact():
    """BodyForce(gy = g), moments, motion, 20 EPEC steps: vc = g t, the centre of mass falls by g t^2 / 2 (the
    midpoint rule is exact for a constant acceleration), nothing turns"""
    from pysph_amd import rigid_body as rb
    from pysph_amd.integrator import EPECIntegrator
    grav, dt, steps = -9.81, 1e-2, 20
    pa = lattice_bodies([27, 64], seed=31)
    pa.omega[:] = 0.0
    pa.vc[:] = 0.0
    start = clone(pa)
    host_moments(start)
    integ = EPECIntegrator(body=rb.RK2StepRigidBody())
    a_eval, nnps, ctx = make_eval(pa, dynamics_equations(gravity=grav), integrator=integ)
    t = 0.0
    for _ in range(steps):
        integ.step(t, dt)
        t += dt
    a_eval.compute(t, dt)                 # cm of the final positions
    pa.gpu.pull()
    for b in range(2):
        vc, cm, cm0 = pa.vc[3 * b:3 * b + 3], pa.cm[3 * b:3 * b + 3], start.cm[3 * b:3 * b + 3]
        assert abs(vc[1] - grav * t) < TOL * abs(grav * t) and abs(vc[0]) < TOL * abs(grav * t) and abs(vc[2]) < TOL * abs(grav * t)
        fall = 0.5 * grav * t * t
        assert abs((cm[1] - cm0[1]) - fall) < TOL * abs(fall), (cm[1] - cm0[1], fall)
        assert abs(cm[0] - cm0[0]) < TOL * abs(fall) and abs(cm[2] - cm0[2]) < TOL * abs(fall)
    # nothing turns: gravity has no torque about the centre of mass.  Scale: the angular acceleration |g| / L the
    # weight would give at a lever arm of the body's size L
    scale = abs(grav) / 0.1
    assert np.abs(pa.omega_dot).max() < TOL * scale and np.abs(pa.omega).max() < TOL * scale * t


@pytest.mark.gpu
def test_torque_free_spin_of_an_isotropic_body():
    """a 5^3 cube of equal masses: I is a multiple of the unit matrix, omega x (I omega) = 0, omega stays"""
    from pysph_amd import rigid_body as rb
    from pysph_amd.integrator import EPECIntegrator
    from pysph_amd.particle_array import get_particle_array_rigid_body
    c = (np.arange(5) - 2.0) * 0.1
    x, y, z = [a.ravel() for a in np.meshgrid(c, c, c, indexing='ij')]
    pa = get_particle_array_rigid_body(name='body', x=x + 0.05, y=y - 0.02, z=z + 0.01, m=0.7 * np.ones(125),
                                       h=0.13 * np.ones(125))
    omega = np.array([0.9, -1.2, 0.5])
    pa.omega[:] = omega
    integ = EPECIntegrator(body=rb.RK2StepRigidBody())
    a_eval, nnps, ctx = make_eval(pa, dynamics_equations(), integrator=integ)
    w2 = float(omega @ omega)
    t, dt = 0.0, 1e-3
    for _ in range(20):
        integ.step(t, dt)
        t += dt
        pa.gpu.pull('omega', 'omega_dot')
        assert np.abs(pa.omega_dot).max() < TOL * w2, pa.omega_dot
    assert np.abs(pa.omega - omega).max() < TOL * np.abs(omega).max()
    pa.gpu.pull('x')
    assert np.abs(pa.x - (x + 0.05)).max() > 1e-4          # it did turn


@pytest.mark.gpu
def test_refusals_on_the_device():
    from pysph_amd import device as dev
    from pysph_amd.particle_array import get_particle_array_rigid_body
    # a body without particles: body 1 of 3
    pa = get_particle_array_rigid_body(name='body', x=np.arange(4.0), m=np.ones(4), body_id=np.array([0, 0, 2, 2]))
    with pytest.raises(ValueError, match='no particles'):
        make_eval(pa, dynamics_equations())[0].compute(0.0, 1e-3)
    # ... also when it loses its particles on the device, after the state was set up
    pa = lattice_bodies([8, 8, 8])
    h = device_moments(pa)
    h.align(np.arange(16))
    with pytest.raises(ValueError, match='no particles|outside'):
        h.rigid_moments()
    # a slab-decomposed array, periodic images
    for mark in ('slab', 'periodic'):
        pa = lattice_bodies([8, 8])
        a_eval, nnps, ctx = make_eval(pa, dynamics_equations())
        if mark == 'slab':
            pa.slab_decomposed = True
        else:
            pa.gpu.ghost_owner = 'domain'
        with pytest.raises(NotImplementedError, match='rigid bodies are not supported'):
            a_eval.compute(0.0, 1e-3)
    # the stages need the body state
    ctx = dev.HipContext(0)
    plain = lattice_bodies([8])
    hp = dev.attach(plain, ctx)
    hp.push('x')
    with pytest.raises(dev.SphError, match='sph_rigid_setup'):
        dev._check(ctx.lib.sph_integrate_stage(ctx._h, hp.array_id, 4, 1, 1e-3))


@pytest.mark.gpu
def test_body_in_tank_free():
    """the example with --free at dx = 0.1 for 10 steps: finite, the block has moved, and the force of the body
    state is the sum of the particles' forces"""
    from pysph_amd import device as dev
    from pysph_amd.examples import body_in_tank as B
    start = B.create_particles(0.1, free=True)[2]
    arrays, forces = B.run(dx=0.1, n_steps=10, ctx=dev.HipContext(0), log=False, free=True)
    block = arrays[2]
    block.gpu.pull()
    for pa in arrays[:2]:
        pa.gpu.pull('x', 'y', 'z', 'u', 'v', 'w', 'rho')
    for pa in arrays:
        for k in ('x', 'y', 'z', 'u', 'v', 'w', 'rho'):
            assert np.all(np.isfinite(pa.properties[k])), (pa.name, k)
    for k in STATE:
        assert np.all(np.isfinite(block.constants[k])), k
    assert len(forces) == 10 and np.all(np.isfinite(forces))
    assert np.abs(block.y - start.y).max() > 0.0 and block.vc[1] != 0.0
    assert np.array_equal(np.asarray(forces[-1]), block.force)
    sum_bound_check(block, 'body_in_tank')
