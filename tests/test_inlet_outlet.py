"""Device-resident open boundaries: pysph_amd/inlet_outlet.py and the
``sph_io_*`` entry points behind ``pa.gpu.classify_plane / transfer_selected /
shift_selected / remove_selected``.

A  the reference's own scenarios (pysph/sph/bc/tests/test_simple_inlet_outlet.py:
   TestSimpleInlet1D :19-122, TestSimpleOutlet1D :125-252), restated minimally,
   with the values the reference asserts (line numbers per test);
B  a differential against a numpy statement written here, bit for bit;
C  the fused classification against ``IOEvaluate`` as a generated family;
D  the host arrays are not in the loop (NaN-poisoned before the update);
E  the channel example stepped through the device path and through the
   package's host-side structural helpers, step by step;
F  what the library knows of an array (one h / one m, the previous bounds) is
   re-examined after rows arrive and after ``sph_array_fill`` on positions.

Ordering: appended rows in ascending source index, removal stable -- the
reference's remove_particles fills holes from the end, so A compares with the
reference's VALUES at the reference's (1-D, monotone) positions and B / E
compare row for row with this package's own contract."""
import ctypes as C

import numpy as np
import pytest

from pysph_amd.equations import Group
from pysph_amd.inlet_outlet import (InletBase, InletInfo, InletOutletManager, IOEvaluate,
                                    OutletBase, OutletInfo)
from pysph_amd.particle_array import ParticleArray, get_particle_array, get_particle_array_wcsph

DX = 0.1


# ---------------------------------------------------------------------------
# plain Python (no GPU)
# ---------------------------------------------------------------------------
def test_manager_names_ghost_pairs_lengths_and_mirror_images():
    x = -DX * np.arange(5, 0, -1)
    inlet = get_particle_array(name='inlet', x=x, m=np.ones(5), h=1.5 * DX * np.ones(5), u=2.0 * np.ones(5))
    outlet = get_particle_array(name='outlet', x=1.0 - x)
    fluid = get_particle_array(name='fluid', x=np.linspace(0.05, 0.95, 10))
    iom = InletOutletManager(
        ['fluid'], [InletInfo('inlet', normal=[-1.0, 0.0, 0.0], refpoint=[-DX / 2, 0.0, 0.0])],
        [OutletInfo('outlet', normal=[1.0, 0.0, 0.0], refpoint=[1.0 + DX / 2, 0.0, 0.0])])
    assert iom.inlets == ['inlet'] and iom.outlets == ['outlet']
    assert iom.inlet_pairs == {'inlet': 'ghost_inlet'} and iom.outlet_pairs == {}
    assert iom.get_io_names() == ['inlet', 'outlet']
    assert iom.get_io_names(ghost=True) == ['inlet', 'outlet', 'ghost_inlet']
    assert iom.inletinfo[0].update_cls is InletBase and iom.outletinfo[0].update_cls is OutletBase
    assert iom.get_equations(None) == [] and iom.get_equations_post_compute_acceleration() == []
    with pytest.raises(NotImplementedError):
        iom.get_stepper(None, None)
    iom.update_dx(DX)
    assert [i.dx for i in iom.inletinfo + iom.outletinfo] == [DX, DX]
    ghost = iom.create_ghost(inlet, inlet=True)
    assert ghost.name == 'ghost_inlet' and iom.create_ghost(outlet, inlet=False) is None
    # mirror image about x = -dx/2; m, h, u carried over, p zero
    assert np.allclose(ghost.x, 2 * (-DX / 2) - x, atol=1e-15) and np.all(ghost.u == 2.0) and np.all(ghost.p == 0.0)
    assert np.all(ghost.h == inlet.h) and np.all(ghost.m == 1.0)
    iom.setup_iom(1, 'kernel')
    iom.active_stages = [2]
    arrays = {'inlet': inlet, 'outlet': outlet, 'fluid': fluid, 'ghost_inlet': ghost}
    ios = iom.get_inlet_outlet(arrays)
    assert [type(o) for o in ios] == [InletBase, OutletBase]
    assert abs(iom.inletinfo[0].length - 0.5) < 1e-14 and abs(iom.outletinfo[0].length - 0.5) < 1e-14
    assert ios[0].ghost_pa is ghost and ios[0].dest_pa is fluid and ios[1].source_pa is fluid
    assert ios[0].active_stages == [2] and ios[0].kernel == 'kernel' and ios[0].dim == 1
    # inactive stage: nothing is touched (not even the device requirement); active: a clear error
    ios[0].update(0.0, 0.1, 1)
    with pytest.raises(RuntimeError, match='device'):
        ios[0].update(0.0, 0.1, 2)
    with pytest.raises(RuntimeError, match='device'):
        ios[1].update(0.0, 0.1, 2)


def np_classify(x, y, z, ref, nrm, maxdist=1000.0):
    """the statement the device classification is held against"""
    d = (x - ref[0]) * nrm[0] + (y - ref[1]) * nrm[1] + (z - ref[2]) * nrm[2]
    ioid = np.where((d > 1e-6) & (d - maxdist < 1e-6), 1.0, np.where(d - maxdist > 1e-6, 2.0, 0.0))
    return d, ioid


def test_ioevaluate_body_as_python_matches_the_three_comparisons():
    eq = IOEvaluate('fluid', None, x=0.5, y=0.0, z=0.0, xn=1.0, yn=0.0, zn=0.0, maxdist=0.25)
    assert IOEvaluate('a', None, 0, 0, 0, 1, 0, 0).maxdist == 1000.0
    x = 0.5 + np.array([-0.1, 0.0, 1e-6, 2e-6, 0.1, 0.25, 0.25 + 1e-6, 0.25 + 3e-6, 0.4])
    y = z = np.zeros_like(x)
    ioid, disp = np.full(x.size, -1.0), np.zeros(x.size)
    for i in range(x.size):
        eq.loop(i, x, y, z, ioid, disp)
    d, want = np_classify(x, y, z, (0.5, 0.0, 0.0), (1.0, 0.0, 0.0), 0.25)
    assert np.array_equal(disp, d) and np.array_equal(ioid, want)
    assert list(want[[0, 1, 4, 8]]) == [0.0, 0.0, 1.0, 2.0]


# ---------------------------------------------------------------------------
# helpers of the GPU tests
# ---------------------------------------------------------------------------
def float_props(pa):
    return [k for k, v in pa.properties.items() if v.dtype == np.float64]


def push_all(pa, ctx):
    """every float property (strided ones by component) and gid to the device"""
    from pysph_amd import device as dev
    g = dev.attach(pa, ctx)
    dev.prop_register('gid')
    names = ['gid']
    for k in float_props(pa):
        st = pa.stride.get(k, 1)
        names += [k] if st == 1 else ['%s__%d' % (k, c) for c in range(st)]
    g.push(*names)
    return g


def device_values(pa):
    """{property: values on the DEVICE} for every float property and gid"""
    from pysph_amd import device as dev
    g = pa.gpu
    n = g.get_number_of_particles()
    out = {}
    for k in float_props(pa):
        out[k] = dev.DeviceProperty(g, k).get()
    gid = np.empty(n)
    if n:
        dev._check(g.lib.sph_array_pull(g.ctx._h, g.array_id, dev.prop_id('gid'), gid.ctypes.data_as(dev._PD), 0, n))
    out['gid'] = gid
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---------------------------------------------------------------------------
# A. the reference's scenarios
# ---------------------------------------------------------------------------
LB_PROPS = ['x', 'y', 'z', 'u', 'v', 'w', 'm', 'h', 'rho', 'p', 'au', 'av', 'aw', 'ioid', 'disp']


class _Scene(object):
    """setUp of TestSimpleInlet1D (:20-38) / TestSimpleOutlet1D (:126-145): five
    particles at x = -0.5 ... -0.1, an EMPTY second array, interface at -dx/2,
    length 0.5"""

    def __init__(self, kind):
        from pysph_amd import device as dev
        x = -DX * np.arange(5, 0, -1)
        full = get_particle_array(name='inlet' if kind == 'inlet' else 'fluid', x=x, m=np.ones(5),
                                  h=1.5 * DX * np.ones(5), p=5.0 * np.ones(5))
        empty = get_particle_array(name='fluid' if kind == 'inlet' else 'outlet')
        for pa in (full, empty):
            pa.add_property('ioid')
            pa.add_property('disp')
        self.ctx = dev.HipContext(0)
        for pa in (full, empty):
            push_all(pa, self.ctx)
        self.full, self.empty = full, empty
        if kind == 'inlet':
            self.info = InletInfo('inlet', normal=[-1.0, 0.0, 0.0], refpoint=[-DX / 2, 0.0, 0.0])
        else:
            self.info = OutletInfo('outlet', normal=[1.0, 0.0, 0.0], refpoint=[-DX / 2, 0.0, 0.0],
                                   props_to_copy=LB_PROPS)
        self.info.length = 0.5

    def move(self, pa, by):
        pa.gpu.sync_host()
        pa.x += by
        pa.gpu.push('x')

    def host(self):
        for pa in (self.full, self.empty):
            pa.gpu.sync_host()

    def close(self):
        self.ctx.close()


def _check_five(pa, x_expect):
    assert pa.get_number_of_particles() == len(x_expect) == len(pa.x)
    assert np.allclose(pa.x, x_expect)
    assert np.allclose(pa.p, 5.0, atol=1e-14) and np.allclose(pa.h, 1.5 * DX, atol=1e-14)
    assert np.all(pa.tag == 0)


@pytest.mark.gpu
def test_inlet_update_creates_particles_in_destination():       # :40-74
    s = _Scene('inlet')
    inlet = InletBase(s.full, s.empty, s.info, dim=1, kernel=None)
    s.move(s.full, 0.12)
    inlet.update(time=0.0, dt=0.0, stage=1)
    assert inlet.last_counts == (1, 4, 0)
    s.host()
    x_expect = -np.arange(5, 0, -1) * DX + 0.12
    x_expect[x_expect > 0.0] -= 0.5
    _check_five(s.full, x_expect)
    # the destination was empty and now holds the one particle that crossed
    _check_five(s.empty, -np.arange(1, 0, -1) * DX + 0.12)
    s.close()


@pytest.mark.gpu
def test_inlet_updates_only_in_its_active_stages():             # :76-101
    s = _Scene('inlet')
    inlet = InletBase(s.full, s.empty, s.info, dim=1, kernel=None)
    s.move(s.full, 0.15)
    inlet.active_stages = [1]
    inlet.update(time=0.0, dt=0.0, stage=2)
    s.host()
    _check_five(s.full, -np.arange(5, 0, -1) * DX + 0.15)
    assert s.empty.get_number_of_particles() == 0
    s.close()


@pytest.mark.gpu
def test_inlet_calls_callback():                                # :103-122
    s = _Scene('inlet')
    calls = []
    inlet = InletBase(s.full, s.empty, s.info, dim=1.0, kernel=None, callback=lambda d, i: calls.append((d, i)))
    s.move(s.full, 0.5)
    inlet.update(time=0.0, dt=0.0, stage=1)
    assert len(calls) == 1 and calls[0][0] is s.empty and calls[0][1] is s.full
    s.close()


@pytest.mark.gpu
def test_outlet_absorbs_particles_from_source():                # :147-182
    s = _Scene('outlet')
    outlet = OutletBase(s.empty, s.full, s.info, dim=1, kernel=None)
    s.move(s.full, 0.12)
    outlet.update(time=0.0, dt=0.0, stage=1)
    s.host()
    _check_five(s.full, -np.arange(5, 1, -1) * DX + 0.12)
    _check_five(s.empty, -np.arange(1, 0, -1) * DX + 0.12)
    s.close()


@pytest.mark.gpu
def test_outlet_updates_only_in_its_active_stages():            # :184-209
    s = _Scene('outlet')
    outlet = OutletBase(s.empty, s.full, s.info, dim=1, kernel=None)
    s.move(s.full, 0.15)
    outlet.active_stages = [1]
    outlet.update(time=0.0, dt=0.0, stage=2)
    s.host()
    _check_five(s.full, -np.arange(5, 0, -1) * DX + 0.15)
    assert s.empty.get_number_of_particles() == 0
    s.close()


@pytest.mark.gpu
def test_outlet_deletes_particles():                            # :211-231
    s = _Scene('outlet')
    outlet = OutletBase(s.empty, s.full, s.info, dim=1, kernel=None)
    s.move(s.full, 0.5)
    outlet.update(time=0.0, dt=0.0, stage=1)
    assert s.full.get_number_of_particles() == 0 and s.full.gpu.get_number_of_particles() == 0
    assert s.empty.get_number_of_particles() == 5 and s.empty.gpu.get_number_of_particles() == 5
    s.move(s.empty, 0.12)
    outlet.update(time=0.0, dt=0.0, stage=1)
    assert s.empty.get_number_of_particles() == 4 and s.empty.gpu.get_number_of_particles() == 4
    s.host()
    # the one beyond the far end went; the others kept their order
    _check_five(s.empty, -np.arange(5, 1, -1) * DX + 0.5 + 0.12)
    s.close()


@pytest.mark.gpu
def test_outlet_calls_callback():                               # :233-252
    s = _Scene('outlet')
    calls = []
    outlet = OutletBase(s.empty, s.full, s.info, dim=1.0, kernel=None, callback=lambda a, b: calls.append((a, b)))
    s.move(s.full, 0.5)
    outlet.update(time=0.0, dt=0.0, stage=1)
    assert len(calls) == 1 and calls[0][0] is s.full and calls[0][1] is s.empty
    s.close()


# ---------------------------------------------------------------------------
# B / D. differential against a numpy statement
# ---------------------------------------------------------------------------
# Every coordinate is a multiple of 2^-30 below 2 in magnitude and every component of the plane's normal a multiple of
# 2^-18 (an oblique vector of length 1 +- 2^-19): the differences have at most 32 significant bits, the three products
# at most 50, their sum is a multiple of 2^-48 below 4 -- disp is EXACT in binary64 whether or not a compiler fuses
# multiply and add, so the numpy statement and the device must agree in every bit.  (_points checks the exactness.)
GRID = 2.0 ** -30
NRM = tuple(np.round(np.array([0.48, 0.6, 0.64]) * 2 ** 18) / 2 ** 18)
REF = (0.125, -0.0625, 0.03125)
LENGTH = 0.25


def _place(rng, d, ref, nrm):
    """points at signed distance d from the plane (measured with `nrm` as it is, not normalised), scattered along it"""
    d, nrm = np.asarray(d, dtype=float), np.asarray(nrm, dtype=float)
    t1 = np.cross(nrm, [0.0, 0.0, 1.0])
    t2 = np.cross(nrm, t1)
    a, b = rng.uniform(-0.4, 0.4, d.size), rng.uniform(-0.4, 0.4, d.size)
    return (np.asarray(ref)[None, :] + (d / (nrm @ nrm))[:, None] * nrm[None, :] + a[:, None] * t1[None, :] +
            b[:, None] * t2[None, :])


def _points(rng, d):
    """... on the grid (which moves a point by up to 1e-9 along the normal), with the exactness of disp checked"""
    p = np.round(_place(rng, d, REF, NRM) / GRID) * GRID
    exact = sum((p[:, k].astype(np.longdouble) - REF[k]) * np.longdouble(NRM[k]) for k in range(3))
    disp = np_classify(p[:, 0], p[:, 1], p[:, 2], REF, NRM)[0]
    assert np.all(exact == disp.astype(np.longdouble)) and np.all(np.abs(p) < 2.0)
    assert np.max(np.abs(disp - d)) < 2e-9
    return p


def _edge_distances(thresholds):
    """on (to the grid's 1e-9) and within 1e-6 of each threshold"""
    offs = [0.0, 4e-10, -4e-10, 1e-9, -1e-9, 1e-8, -1e-8, 1e-7, -1e-7, 5e-7, -5e-7, 9.99e-7, -9.99e-7, 1e-6, -1e-6]
    return [t + o for t in thresholds for o in offs]


def _random_array(name, rng, pts, extra=()):
    n = pts.shape[0]
    pa = get_particle_array(name=name, x=pts[:, 0].copy(), y=pts[:, 1].copy(), z=pts[:, 2].copy())
    for k in ('u', 'v', 'w', 'm', 'h', 'rho', 'p', 'au', 'av', 'aw'):
        pa.properties[k][:] = rng.uniform(-1, 1, n)
    pa.add_property('ioid', data=rng.uniform(5, 6, n) if n else None)
    pa.add_property('disp', data=rng.uniform(5, 6, n) if n else None)
    pa.add_property('g3', stride=3, data=rng.uniform(-1, 1, 3 * n) if n else None)
    for k in extra:
        pa.add_property(k, data=rng.uniform(1, 2, n) if n else None)
    return pa


def _snapshot(pa):
    out = dict((k, pa.properties[k].copy()) for k in float_props(pa))
    out['gid'] = pa.gid.astype(np.float64)
    return out


def _stride(pa, k):
    return pa.stride.get(k, 1)


def _take(v, idx, st):
    return v[idx] if st == 1 else v.reshape(-1, st)[idx].ravel()


def _delete(v, idx, st):
    return np.delete(v, idx) if st == 1 else np.delete(v.reshape(-1, st), idx, axis=0).ravel()


def _np_append(dst, dst_pa, src, idx, copied):
    """dst <- dst + rows idx of src: copied properties travel, the others read 0"""
    for k in dst:
        st = _stride(dst_pa, k)
        new = _take(src[k], idx, st) if (k in copied and k in src) else np.zeros(idx.size * st)
        dst[k] = np.concatenate([dst[k], new])


def _np_remove(arr, pa, idx):
    for k in arr:
        arr[k] = _delete(arr[k], idx, _stride(pa, k))


def _build(kind, seed):
    """the arrays of one scenario and what the numpy statement expects of them after ONE update"""
    rng = np.random.default_rng(seed)
    if kind.startswith('inlet'):
        d_in = np.concatenate([rng.uniform(-0.1 * LENGTH, LENGTH, 3000), _edge_distances([0.0, 1e-6]), [0.0, LENGTH]])
        inlet = _random_array('inlet', rng, _points(rng, rng.permutation(d_in)), extra=('only_inlet',))
        fluid = _random_array('fluid', rng, _points(rng, rng.uniform(-0.5, 0.0, 2000)), extra=('only_fluid',))
        arrays = [inlet, fluid]
        if kind == 'inlet+ghost':
            ghost = _random_array('ghost_inlet', rng, _points(rng, -rng.permutation(d_in)))
            arrays.append(ghost)
        gid0 = 0
        for pa in arrays:
            pa.gid[:] = np.arange(gid0, gid0 + pa.get_number_of_particles())
            gid0 += pa.get_number_of_particles()
        want = [_snapshot(pa) for pa in arrays]
        wi, wf = want[0], want[1]
        wi['disp'], wi['ioid'] = np_classify(wi['x'], wi['y'], wi['z'], REF, NRM, LENGTH)
        wf['disp'], wf['ioid'] = np_classify(wf['x'], wf['y'], wf['z'], REF, NRM)
        idx = np.where(wi['ioid'] == 0)[0]
        _np_append(wf, fluid, wi, idx, copied=set(wi))
        for k, c in zip('xyz', NRM):
            wi[k][idx] += LENGTH * c
            if kind == 'inlet+ghost':
                want[2][k][idx] -= LENGTH * c
        counts = tuple(int(np.count_nonzero(wi['ioid'] == c)) for c in (0, 1, 2))
        assert 100 < counts[0] < 1000 and counts[2] == 0
        return arrays, want, counts
    d_src = np.concatenate([rng.uniform(-0.5, 0.1, 3000), _edge_distances([1e-6])])
    d_out = np.concatenate([rng.uniform(0.0, 1.3 * LENGTH, 1500), _edge_distances([LENGTH, LENGTH + 1e-6]), [LENGTH]])
    fluid = _random_array('fluid', rng, _points(rng, rng.permutation(d_src)), extra=('only_fluid',))
    outlet = _random_array('outlet', rng, _points(rng, rng.permutation(d_out)), extra=('only_outlet',))
    fluid.gid[:] = np.arange(fluid.get_number_of_particles())
    outlet.gid[:] = 10 ** 6 + np.arange(outlet.get_number_of_particles())
    want = [_snapshot(outlet), _snapshot(fluid)]
    wo, ws = want
    wo['disp'], wo['ioid'] = np_classify(wo['x'], wo['y'], wo['z'], REF, NRM, LENGTH)
    ws['disp'], ws['ioid'] = np_classify(ws['x'], ws['y'], ws['z'], REF, NRM)
    gone = np.where(wo['ioid'] == 2)[0]
    idx = np.where(ws['ioid'] == 1)[0]
    _np_append(wo, outlet, ws, idx, copied=set(OUTLET_COPIES))
    _np_remove(ws, fluid, idx)
    _np_remove(wo, outlet, gone)
    counts = (tuple(int(np.count_nonzero(np_classify(outlet.x, outlet.y, outlet.z, REF, NRM, LENGTH)[1] == c)) for c in (0, 1, 2)),
              tuple(int(np.count_nonzero(np_classify(fluid.x, fluid.y, fluid.z, REF, NRM)[1] == c)) for c in (0, 1, 2)))
    assert counts[0][2] > 100 and 100 < counts[1][1] < 1000
    return [outlet, fluid], want, counts


# a strict subset of the shared properties, a strided one among them; v, w, p, au ..., disp and gid read 0 on new rows
OUTLET_COPIES = ['x', 'y', 'z', 'u', 'm', 'h', 'rho', 'g3', 'ioid']


class _Traffic(object):
    """counts the property copies between host and device (sph_array_push / sph_array_pull) while installed"""

    def __init__(self, lib):
        self.lib, self.bytes, self.calls = lib, 0, 0

    def __enter__(self):
        self.saved = (self.lib.sph_array_push, self.lib.sph_array_pull)

        def wrap(fn):
            def counted(ctx, aid, prop, host, offset, n):
                self.bytes += 8 * int(n)
                self.calls += 1
                return fn(ctx, aid, prop, host, offset, n)
            return counted
        self.lib.sph_array_push, self.lib.sph_array_pull = wrap(self.saved[0]), wrap(self.saved[1])
        return self

    def __exit__(self, *exc):
        self.lib.sph_array_push, self.lib.sph_array_pull = self.saved


def _run_scenario(kind, poison):
    from pysph_amd import device as dev
    arrays, want, counts = _build(kind, seed=11)
    ctx = dev.HipContext(0)
    for pa in arrays:
        push_all(pa, ctx)
    if poison:          # D: the host copies are not an input of the update
        for pa in arrays:
            for k in float_props(pa):
                pa.properties[k][:] = np.nan
    if kind.startswith('inlet'):
        info = InletInfo('inlet', normal=list(NRM), refpoint=list(REF), has_ghost=kind == 'inlet+ghost')
        info.length = LENGTH
        io = InletBase(arrays[0], arrays[1], info, None, 3, ghost_pa=arrays[2] if kind == 'inlet+ghost' else None)
    else:
        info = OutletInfo('outlet', normal=list(NRM), refpoint=list(REF), props_to_copy=OUTLET_COPIES)
        info.length = LENGTH
        io = OutletBase(arrays[0], arrays[1], info, None, 3)
    with _Traffic(ctx.lib) as traffic:
        io.update(0.0, 0.1, 1)
    # no property data crosses in either direction: the update makes no sph_array_push / sph_array_pull at all
    assert traffic.calls == 0 and traffic.bytes == 0
    assert io.last_counts == counts, (io.last_counts, counts)
    for pa, w in zip(arrays, want):
        got = device_values(pa)
        assert sorted(got) == sorted(w)
        n = w['x'].size
        assert pa.gpu.get_number_of_particles() == pa.gpu.get_number_of_particles(True) == n
        for k in sorted(w):
            assert same_bits(got[k], w[k]), (kind, pa.name, k, int(np.count_nonzero(got[k] != w[k])))
        # the host array follows in shape; new rows are Local
        assert pa.get_number_of_particles() == pa.get_number_of_particles(True) == n
        assert all(v.size == n * _stride(pa, k) for k, v in pa.properties.items())
        assert np.all(pa.tag == 0)
    if poison:
        for pa, w in zip(arrays, want):
            pa.gpu.sync_host()
            assert np.all(pa.tag == 0) and pa.get_number_of_particles() == w['x'].size
            for k in float_props(pa):
                assert same_bits(pa.properties[k], w[k]), (kind, pa.name, k)
            assert np.array_equal(pa.gid, w['gid'].astype(np.uint32))
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['inlet+ghost', 'inlet', 'outlet'])
def test_update_equals_numpy_statement_bit_for_bit(kind):
    _run_scenario(kind, poison=False)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['inlet+ghost', 'inlet', 'outlet'])
def test_host_arrays_are_not_in_the_loop(kind):
    _run_scenario(kind, poison=True)


# ---------------------------------------------------------------------------
# C. fused classification vs the generated IOEvaluate
# ---------------------------------------------------------------------------
def _classify_case():
    """the inlet points of B plus points with full mantissas (where fusing
    multiply and add would change disp) and a plane whose numbers are not exact"""
    rng = np.random.default_rng(3)
    d = np.concatenate([rng.uniform(-0.1 * LENGTH, 1.2 * LENGTH, 3000), _edge_distances([0.0, 1e-6, LENGTH, LENGTH + 1e-6])])
    exact = _points(rng, d)
    nrm = np.array([0.3, -0.5, 0.7])
    nrm /= np.sqrt(nrm @ nrm)
    ref = np.array([0.1, 0.2, -0.3])
    dd = np.concatenate([rng.uniform(-0.1, 0.3, 3000), _edge_distances([1e-6, 0.2 + 1e-6])])
    loose = _place(rng, dd, ref, nrm)
    return [(exact, REF, NRM, LENGTH), (loose, tuple(ref), tuple(nrm), 0.2)]


def _classify_array(pts):
    pa = get_particle_array(name='fluid', x=pts[:, 0].copy(), y=pts[:, 1].copy(), z=pts[:, 2].copy(),
                            h=0.05 * np.ones(pts.shape[0]), m=np.ones(pts.shape[0]))
    pa.add_property('ioid', data=7.0)
    pa.add_property('disp', data=7.0)
    return pa


def _classify_equations(ref, nrm, maxdist):
    return [Group(equations=[IOEvaluate('fluid', None, x=ref[0], y=ref[1], z=ref[2], xn=nrm[0], yn=nrm[1],
                                        zn=nrm[2], maxdist=maxdist)], real=False)]


@pytest.mark.gpu
def test_fused_classification_equals_generated_ioevaluate():
    from pysph_amd import device as dev
    from pysph_amd import kernels as K
    from pysph_amd.acceleration_eval import AccelerationEval, SPHCompiler
    from pysph_amd.nnps import HipNNPS
    kernel = K.CubicSpline(dim=3)
    for pts, ref, nrm, maxdist in _classify_case():
        pa = _classify_array(pts)
        ctx = dev.HipContext(0)
        g = push_all(pa, ctx)
        counts = g.classify_plane(ref, nrm, maxdist=maxdist)
        fused = device_values(pa)
        ctx.close()
        pb = _classify_array(pts)
        ctx = dev.HipContext(0)
        a_eval = AccelerationEval([pb], _classify_equations(ref, nrm, maxdist), kernel)
        SPHCompiler(a_eval, ctx=ctx).compile()
        a_eval.set_nnps(HipNNPS(3, [pb], radius_scale=kernel.radius_scale, ctx=ctx))
        a_eval.compute(0.0, 0.1)
        ctx.close()
        assert np.array_equal(fused['ioid'], pb.ioid)
        assert same_bits(fused['disp'], pb.disp)
        assert counts == tuple(int(np.count_nonzero(pb.ioid == c)) for c in (0, 1, 2)) and min(counts) > 0
        # ... and both against the numpy statement: with contraction off on the device, disp is the same sequence of
        # binary64 operations numpy performs
        d, ioid = np_classify(pts[:, 0], pts[:, 1], pts[:, 2], ref, nrm, maxdist)
        assert same_bits(d, pb.disp) and np.array_equal(ioid, pb.ioid)


# ---------------------------------------------------------------------------
# error behaviour
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_arrays_with_ghosts_and_stale_selections_are_refused():
    from pysph_amd import device as dev
    rng = np.random.default_rng(0)
    a = _random_array('inlet', rng, _points(rng, rng.uniform(-0.1, 0.2, 200)))
    b = _random_array('fluid', rng, _points(rng, rng.uniform(-0.5, 0.0, 100)))
    ctx = dev.HipContext(0)
    ga, gb = push_all(a, ctx), push_all(b, ctx)
    lib, ids = ctx.lib, (C.c_int * 1)(dev.prop_id('x'))
    # no selection yet
    with pytest.raises(dev.SphError, match='selection'):
        ga.transfer_selected(gb, 0)
    n0 = ga.classify_plane(REF, NRM, maxdist=LENGTH, read=False)
    assert n0 is None
    # counts not read yet
    with pytest.raises(dev.SphError, match='counts'):
        dev._check(lib.sph_io_transfer(ctx._h, ga.array_id, gb.array_id, 0, 1, ids, 1))
    (c0, c1, c2), = dev.HipDeviceHelper.read_io_counts(ga)
    assert c0 + c1 + c2 == 200 and c0 > 0
    # a receiver with ghosts behind its real rows: the library refuses ...
    dev._check(lib.sph_array_resize(ctx._h, gb.array_id, 100, 90))
    with pytest.raises(dev.SphError, match='ghosts'):
        dev._check(lib.sph_io_transfer(ctx._h, ga.array_id, gb.array_id, 0, 1, ids, 1))
    with pytest.raises(dev.SphError, match='ghosts'):
        ga.transfer_selected(gb, 0)
    dev._check(lib.sph_array_resize(ctx._h, gb.array_id, 100, 100))
    # ... and so does the helper for an array owned by a slab halo / device domain manager
    gb.ghost_owner = 'slab'
    with pytest.raises(dev.SphError, match='slab'):
        ga.transfer_selected(gb, 0)
    gb.ghost_owner = None
    with pytest.raises(dev.SphError):
        dev._check(lib.sph_io_transfer(ctx._h, ga.array_id, ga.array_id, 0, 1, ids, 1))
    with pytest.raises(dev.SphError):
        dev._check(lib.sph_io_transfer(ctx._h, ga.array_id, gb.array_id, 3, 1, ids, 1))
    # a shift through another array's selection needs as many rows
    with pytest.raises(dev.SphError, match='rows'):
        gb.shift_selected(0, 1.0, 0.0, 0.0, flags=ga)
    assert ga.transfer_selected(gb, 0) == c0 and gb.get_number_of_particles() == 100 + c0
    # rows changed: the selection of the source is still current (keep=True), a removal ends it
    assert ga.remove_selected(0) == c0
    with pytest.raises(dev.SphError, match='selection'):
        ga.remove_selected(1)
    ctx.close()


# ---------------------------------------------------------------------------
# F. invalidation
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_rows_with_other_h_and_m_end_the_uniform_promises(oracle):
    """a fluid with ONE h and ONE m is evaluated twice device-resident (the
    second neighbour update has looked at the masses: uniform-mass records);
    then rows with another h and another m arrive from a feeder array -- the next
    evaluation must match the oracle on the combined particles"""
    from helpers import WC_OUT, rel_err
    from test_hip_parity import TOL, _copy_arrays, cube_equations, make_cube, make_eval
    from pysph_amd import device as dev
    from pysph_amd import kernels as K
    pa, dx = make_cube(14, jitter=0.1)
    rng = np.random.default_rng(5)
    m = 300
    feed = get_particle_array_wcsph(
        name='feed', x=rng.uniform(0.2, 0.8, m), y=rng.uniform(0.2, 0.8, m), z=rng.uniform(0.95, 1.1, m),
        h=1.1 * pa.h[0] * np.ones(m), m=1.5 * pa.m[0] * np.ones(m), rho=1000.0 * (1 + 0.01 * rng.uniform(-1, 1, m)),
        u=rng.uniform(-1, 1, m), v=rng.uniform(-1, 1, m), w=rng.uniform(-1, 1, m))
    both = ParticleArray(name='fluid', **dict((k, np.concatenate([v, feed.properties[k]])) for k, v in pa.properties.items()))
    eqs, kernel = cube_equations(dx), K.WendlandQuintic(dim=3)
    a_eval, nnps, ctx = make_eval([pa], eqs, kernel, 3, 6, sync='manual')
    pa.gpu.push()
    nnps.sync = False
    for _ in range(2):
        nnps.update()
        a_eval.compute(0.0, 1e-5)
    known = (C.c_double(), C.c_double())
    is_known = ctx.lib.sph_array_h_known(ctx._h, pa.gpu.array_id, C.byref(known[0]), C.byref(known[1]))
    print('before: h known without looking: %d [%g, %g], uniform-mass launches %d'
          % (is_known, known[0].value, known[1].value, ctx.timer_get('n_mass_fused')[1]))
    gf = dev.attach(feed, ctx)
    gf.push()
    counts = gf.classify_plane((10.0, 0.0, 0.0), (1.0, 0.0, 0.0))          # everything on the near side: class 0
    assert counts == (m, 0, 0)
    assert gf.transfer_selected(pa.gpu, 0) == m
    nnps.update()
    a_eval.compute(0.0, 1e-5)
    a_eval.c_acceleration_eval.pull_outputs()
    pa.gpu.pull('rho', 'p', 'cs')
    ref = _copy_arrays([both])
    onn = oracle.OracleNNPS(3, ref, radius_scale=kernel.radius_scale)
    onn.update()
    oev = oracle.OracleEval(ref, eqs, kernel, nthreads=8)
    oev.set_nnps(onn)
    oev.compute(0.0, 1e-5)
    assert pa.get_number_of_particles() == both.get_number_of_particles()
    for prop in WC_OUT:
        e = rel_err(pa.properties[prop], ref[0].properties[prop])
        assert e < TOL, (prop, e)
    s1, _ = nnps.get_csr(0, 0)
    s2, _ = onn.get_csr(0, 0, nthreads=8)
    assert np.array_equal(s1, s2)
    ctx.close()


@pytest.mark.gpu
def test_fill_on_positions_is_seen_by_the_next_neighbour_update():
    from test_hip_parity import make_cube
    from pysph_amd import device as dev
    from pysph_amd.nnps import HipNNPS
    pa, dx = make_cube(12)
    pb, _ = make_cube(12)
    ctx = dev.HipContext(0)
    dev.attach(pa, ctx).push()
    nnps = HipNNPS(3, [pa], radius_scale=2.0, ctx=ctx, sync=False)
    for _ in range(3):                      # steady state: updates bin on the previous update's bounds
        nnps.update()
    assert float(nnps.xmax[0]) < 1.2
    dev._check(ctx.lib.sph_array_fill(ctx._h, pa.gpu.array_id, dev.prop_id('x'), 2.5, 100, 50))
    nnps.update()
    pb.x[100:150] = 2.5
    cb = dev.HipContext(0)
    nb = HipNNPS(3, [pb], radius_scale=2.0, ctx=cb)
    assert float(nnps.xmax[0]) == float(nb.xmax[0]) >= 2.5
    assert nnps.cell_size == nb.cell_size and list(nnps.ncells_per_dim) == list(nb.ncells_per_dim)
    sa, ia = nnps.get_csr(0, 0)
    sb, ib = nb.get_csr(0, 0)
    assert np.array_equal(sa, sb) and np.array_equal(ia, ib)
    ctx.close()
    cb.close()


# ---------------------------------------------------------------------------
# E. stepping: the channel example, device path vs the host-side helpers
# ---------------------------------------------------------------------------
CHANNEL = dict(dx=0.02, nx=10, ny=32, nz=32, n_io=4, phases=4)      # 10240 fluid particles
N_STEPS = 40


class _HostInlet(object):
    """InletBase.update through extract_particles / append_parray / DeviceProperty
    get + set: the structural helpers the package had before the device path"""

    def __init__(self, io, log):
        self.io, self.log = io, log

    def update(self, t, dt, stage):
        from pysph_amd.device import DeviceProperty as DP
        io = self.io
        if not io._active(stage):
            return
        inlet, fluid = io.inlet_pa, io.dest_pa
        ref, nrm = (io.x, io.y, io.z), (io.xn, io.yn, io.zn)
        xyz = [DP(inlet.gpu, k).get() for k in 'xyz']
        d, ioid = np_classify(xyz[0], xyz[1], xyz[2], ref, nrm, io.length)
        DP(inlet.gpu, 'disp').set(d)
        DP(inlet.gpu, 'ioid').set(ioid)
        fd, fioid = np_classify(*[DP(fluid.gpu, k).get() for k in 'xyz'], ref, nrm)
        DP(fluid.gpu, 'disp').set(fd)
        DP(fluid.gpu, 'ioid').set(fioid)
        idx = np.where(ioid == 0)[0]
        self.log.append(('in', inlet.gid[idx].copy()))
        if idx.size:
            fluid.gpu.append_parray(inlet.gpu.extract_particles(idx))
            for k, c, v in zip('xyz', nrm, xyz):
                v[idx] += io.length * c
                DP(inlet.gpu, k).set(v)


class _HostOutlet(object):
    def __init__(self, io, log):
        self.io, self.log = io, log

    def update(self, t, dt, stage):
        from pysph_amd.device import DeviceProperty as DP
        io = self.io
        if not io._active(stage):
            return
        outlet, fluid = io.outlet_pa, io.source_pa
        ref, nrm = (io.x, io.y, io.z), (io.xn, io.yn, io.zn)
        od, oioid = np_classify(*[DP(outlet.gpu, k).get() for k in 'xyz'], ref, nrm, io.length)
        DP(outlet.gpu, 'disp').set(od)
        DP(outlet.gpu, 'ioid').set(oioid)
        fd, fioid = np_classify(*[DP(fluid.gpu, k).get() for k in 'xyz'], ref, nrm)
        DP(fluid.gpu, 'disp').set(fd)
        DP(fluid.gpu, 'ioid').set(fioid)
        idx = np.where(fioid == 1)[0]
        self.log.append(('out', fluid.gid[idx].copy()))
        if idx.size:
            outlet.gpu.append_parray(fluid.gpu.extract_particles(idx, props=io.props_to_copy))
            fluid.gpu.remove_particles(idx)
        gone = np.where(oioid == 2)[0]
        if gone.size:
            outlet.gpu.remove_particles(gone)


def _host_updates(log):
    def make(sim):
        return [_HostInlet(sim.ios[0], log), _HostOutlet(sim.ios[1], log)]
    return make


def prebuild():
    """the generated families of this file, built without a GPU (the stage
    bodies of the channel example's steppers, IOEvaluate)"""
    from pysph_amd import kernels as K
    from pysph_amd.acceleration_eval import AccelerationEval, _CGroup
    from pysph_amd.examples import channel_flow as cf
    from pysph_amd.integrator import generated_stages
    n = 0
    arrays = cf.create_particles(dx=0.1, nx=2, ny=2, nz=2)
    kind = K.kernel_id(K.WendlandQuintic(dim=3))
    for pa in arrays[1:3]:
        n += len(generated_stages(cf.CarriedStep(), pa, 0, kind))
    pts = np.zeros((2, 3))
    a = AccelerationEval([_classify_array(pts)], _classify_equations(REF, NRM, LENGTH), K.CubicSpline(dim=3))
    for g in a.equation_groups:
        n += len(_CGroup(g, {'fluid': 0}, {'fluid': a.particle_arrays[0]}, K.kernel_id(K.CubicSpline(dim=3))).units)
    return n


@pytest.mark.gpu
def test_channel_flow_device_path_equals_host_path_step_by_step():
    """Counts per array agree at every step, fields to 1e-10 norm-wise (the
    package's parity bar; bit equality is reported), the fluid's gid set is
    {initial} + {entered} - {left} without duplicates at every step; the run
    has updates where nothing crosses and the outlet outgrows its capacity."""
    from helpers import rel_err
    from pysph_amd import device as dev
    from pysph_amd.examples.channel_flow import ChannelFlow
    log = []
    a = ChannelFlow(**CHANNEL)                                   # device path
    b = ChannelFlow(make_updates=_host_updates(log), **CHANNEL)  # host-side helpers
    init = set(int(g) for g in a.by_name['fluid'].gid)
    inlet_gids = set(int(g) for g in a.by_name['inlet'].gid)
    assert len(init) == 10240 and a.sizes()['outlet'] == 0
    entered, left = [], []
    quiet = busy = 0
    caps_outgrown = 0
    cap = 64                        # what the first property of an empty array is allocated with
    bits = True
    for step in range(N_STEPS):
        mark = len(log)
        a.step()
        b.step()
        sa, sb = a.sizes(), b.sizes()
        assert sa == sb, (step, sa, sb)
        for what, gids in log[mark:]:
            (entered if what == 'in' else left).extend(int(g) for g in gids)
        for io in a.ios:
            cnt = io.last_counts
            moved = cnt[0] if isinstance(io, InletBase) else cnt[1][1] + cnt[0][2]
            quiet += moved == 0
            busy += moved != 0
        # capacity of the receiving outlet array as sph_array_resize grows it (n + n/8 + 64)
        if sa['outlet'] > cap:
            caps_outgrown += 1
            cap = sa['outlet'] + sa['outlet'] // 8 + 64
        assert len(set(entered)) == len(entered) and set(entered) <= inlet_gids
        want = (init | set(entered)) - set(left)
        for sim in (a, b):
            if sim is a:
                gid = device_values(sim.by_name['fluid'])['gid'].astype(np.int64)
            else:
                gid = sim.by_name['fluid'].gid.astype(np.int64)
            assert gid.size == len(set(gid.tolist())) == sa['fluid'], step
            assert set(gid.tolist()) == want, step
        if step % 10 == 9 or step == N_STEPS - 1:
            worst = 0.0
            for name in ('fluid', 'inlet', 'outlet', 'wall'):
                va, vb = device_values(a.by_name[name]), device_values(b.by_name[name])
                for k in sorted(va):
                    if k == 'gid':
                        continue
                    e = rel_err(va[k], vb[k])
                    worst = max(worst, e)
                    bits = bits and same_bits(va[k], vb[k])
                    assert e < 1e-10, (step, name, k, e)
            print('step %d: sizes %s, worst norm-wise difference %.3e, bit-identical so far: %s' % (step + 1, sa, worst, bits))
    print('entered %d, left %d, quiet updates %d, busy updates %d, outlet allocations %d'
          % (len(entered), len(left), quiet, busy, caps_outgrown))
    assert len(entered) >= 512 and len(left) >= 512 and quiet > 0 and busy > 0
    assert caps_outgrown >= 2
    # the host follows after sync_host: right lengths, Local tags, the device's values
    a.sync_host()
    for pa in a.arrays:
        assert pa.get_number_of_particles() == a.sizes()[pa.name] and np.all(pa.tag == 0)
        assert same_bits(pa.x, device_values(pa)['x'])
    a.ctx.close()
    b.ctx.close()
