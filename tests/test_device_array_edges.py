"""The device array layer beyond one wavefront: the storage operations behind ``pa.gpu`` (sph_array_resize / push /
pull / fill / permute, the gather of sph_nnps_reorder_array, HipDeviceHelper's structural operations), the two
reductions of the adaptive time step (sph_reduce_max / min) and the stage sweep (sph_integrate_stage), at sizes where
a wavefront, a block, the capacity or the grid-stride loop decides the result.

References are plain numpy on host copies: ``a[idx]``, slicing, ``np.max``; for the stage sweep the numpy steppers of
oracle/steppers.py (pinned bit-exactly to the reference's methods by tests/test_integrator.py).  Copies and gathers
have no tolerance: after every operation the expected numpy state, the host ParticleArray and the device (through
``gpu.<prop>.get()`` and through ``sph_array_pull``) are compared bit for bit.  Every row of every property holds a
value of its own (property index * 1e6 + row id), so that a row in the wrong place or the wrong property shows.

Every out-of-range case here is rejected on the host before any launch (read from csrc/sph_ctx.hip, sph_nnps.hip)."""
import ctypes as C
import sys
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

UINT_MAX = np.iinfo(np.uint32).max
SIZES = [1, 63, 64, 65, 255, 256, 257, 1023, 1025]
USER = 'test'                 # a user-registered property (the name tests/test_device_helper.py registers: user
                              # slots are a process-wide pool of 128, and the whole suite nearly fills it)
STRIDED = 'force'             # a stride-3 property: lives on the device as force__0 .. __2 (as test_device_helper.py's)
DEVONLY = 'cs'                # device storage only (sph_array_ensure_prop): the host arrays here do not have it


def bits_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float64:
        return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))
    return np.array_equal(a, b)


def tag_pattern(ids):
    """Local and non-Local rows interleaved, so that every block boundary has both on either side"""
    return np.array([0, 1, 0, 2], dtype=np.int32)[np.asarray(ids, dtype=np.int64) % 4]


class Mirror(object):
    """a particle array of n rows with distinct values, its device mirror in a context of its own, and the
    expected state `exp` (numpy arrays the tests transform with numpy alone)"""

    def __init__(self, n, name='edges', mixed_tags=False, positions=False, attach=True):
        from pysph_amd import device as dev
        from pysph_amd.particle_array import get_particle_array
        self.dev = dev
        pa = get_particle_array(name=name, x=np.zeros(n))
        pa.add_property(USER)
        pa.add_property(STRIDED, stride=3)
        self.pa = pa
        self.float_names = [k for k, a in pa.properties.items() if a.dtype == np.float64]
        self.fill_rows(pa, np.arange(n), mixed_tags)
        if positions:       # a cloud the neighbour search can bin into many cells
            rng = np.random.default_rng(n)
            for k in 'xyz':
                pa.properties[k][:] = rng.uniform(0.0, 1.0, n)
            pa.properties['h'][:] = 0.05
        self.exp = dict((k, a.copy()) for k, a in pa.properties.items())
        self.devonly = None
        self.ctx = self.gpu = None
        if attach:
            self.ctx = dev.HipContext(0)
            self.lib, self.h = self.ctx.lib, self.ctx._h
            self.gpu = dev.attach(pa, self.ctx)
            self.gpu.push()
            self.gpu.push(USER, *['%s__%d' % (STRIDED, k) for k in range(3)])
            self.aid = self.gpu.array_id

    def close(self):
        if self.ctx is not None:
            self.ctx.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- values --------------------------------------------------------------------------------------------------
    def code(self, key):
        return (self.float_names.index(key) + 1) * 1e6

    def fill_rows(self, pa, ids, mixed_tags):
        """the rows of `pa` take the values of the particles `ids`"""
        ids = np.asarray(ids, dtype=np.int64)
        for key in self.float_names:
            st = pa.stride.get(key, 1)
            vals = self.code(key) + ids.astype(np.float64)
            pa.properties[key][:] = vals if st == 1 else (vals[:, None] + 0.25 * np.arange(st)[None, :]).ravel()
        pa.properties['gid'][:] = ids
        pa.properties['pid'][:] = ids % 5
        pa.properties['tag'][:] = tag_pattern(ids) if mixed_tags else 0

    def stride(self, key):
        return self.pa.stride.get(key, 1)

    def add_devonly(self):
        dev = self.dev
        pid = dev.prop_register(DEVONLY)
        dev._check(self.lib.sph_array_ensure_prop(self.h, self.aid, pid))
        n = self.n
        assert bits_equal(self.pull(DEVONLY, 0, n), np.zeros(n))      # zero-filled when created
        self.devonly = 99e6 + np.arange(n, dtype=np.float64)
        self.push_rows(DEVONLY, 0, self.devonly)

    # -- raw C-ABI access ------------------------------------------------------------------------------------------
    @property
    def n(self):
        return len(self.exp['tag'])

    def pull(self, name, offset, count):
        dev = self.dev
        out = np.full(max(count, 1), -12345.0)
        dev._check(self.lib.sph_array_pull(self.h, self.aid, dev.prop_id(name), out.ctypes.data_as(dev._PD),
                                           offset, count))
        return out[:count]

    def push_rows(self, name, offset, values):
        dev = self.dev
        values = np.ascontiguousarray(values, dtype=np.float64)
        buf = values if values.size else np.zeros(1)
        dev._check(self.lib.sph_array_push(self.h, self.aid, dev.prop_id(name), buf.ctypes.data_as(dev._PD),
                                           offset, values.size))

    # -- numpy transformations of the expected state ----------------------------------------------------------------
    def take(self, idx):
        idx = np.asarray(idx, dtype=np.int64)
        for key, a in self.exp.items():
            st = self.stride(key)
            self.exp[key] = a[idx] if st == 1 else a.reshape(-1, st)[idx].ravel()
        if self.devonly is not None:
            self.devonly = self.devonly[idx]

    def shrink(self, n):
        self.take(np.arange(n))

    def grow_to(self, n):
        """new rows read 0 (gid: the "no gid" value, as ParticleArray.resize gives it)"""
        k = n - self.n
        assert k >= 0
        for key, a in self.exp.items():
            new = np.zeros(k * self.stride(key), dtype=a.dtype)
            if key == 'gid':
                new[:] = UINT_MAX
            self.exp[key] = np.concatenate([a, new])
        if self.devonly is not None:
            self.devonly = np.concatenate([self.devonly, np.zeros(k)])

    def append_rows(self, rows):
        """rows: {property: values} of the new particles; every other property reads 0 there"""
        n0 = self.n
        count = len(rows['tag'])
        self.grow_to(n0 + count)
        for key, vals in rows.items():
            self.exp[key][n0 * self.stride(key):] = vals

    def align_expected(self):
        order = np.argsort(self.exp['tag'] != 0, kind='stable')
        self.take(order)
        return int(np.count_nonzero(self.exp['tag'] == 0))

    # -- the three-way comparison -----------------------------------------------------------------------------------
    def check_device(self, what=''):
        """the device against the expected state (both read paths)"""
        n = self.n
        assert self.gpu.get_number_of_particles() == n, what
        for key, want in self.exp.items():
            st = self.stride(key)
            if want.dtype != np.float64:
                continue
            for k in range(st):
                name = key if st == 1 else '%s__%d' % (key, k)
                assert bits_equal(self.pull(name, 0, n), want[k::st]), (what, 'sph_array_pull', name)
        if self.devonly is not None:
            assert bits_equal(self.pull(DEVONLY, 0, n), self.devonly), (what, 'sph_array_pull', DEVONLY)

    def check(self, what='', n_real=None):
        pa, gpu = self.pa, self.gpu
        assert pa.get_number_of_particles() == self.n, what
        for key, want in self.exp.items():
            assert bits_equal(pa.properties[key], want), (what, 'host', key)
            assert bits_equal(getattr(gpu, key).get(), want), (what, 'gpu.get', key)
        self.check_device(what)
        assert gpu.get_number_of_particles(True) == pa.get_number_of_particles(True), what
        if n_real is not None:
            assert pa.get_number_of_particles(True) == n_real, what

    def check_rows(self, what=''):
        """the integer metadata against the float properties, row by row: every row still carries the tag, pid and
        gid of the particle whose id its x (host and device) encodes"""
        pa = self.pa
        for x in (pa.properties['x'], self.pull('x', 0, self.n)):
            ids = x - self.code('x')
            assert np.array_equal(pa.properties['gid'], ids), what
            assert np.array_equal(pa.properties['pid'], ids % 5), what
            assert np.array_equal(pa.properties['tag'], tag_pattern(ids)), what
            assert np.array_equal(pa.properties[USER] - self.code(USER), ids), what
            assert np.array_equal(pa.properties[STRIDED][2::3] - self.code(STRIDED) - 0.5, ids), what


# ---------------------------------------------------------------------------------------------------------------------
# push / pull with an offset
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', SIZES)
def test_push_pull_at_offsets(n):
    from pysph_amd.device import SphError
    with Mirror(n) as m:
        m.check('initial')
        serial = 0
        for offset in sorted(set([0, 1, 255, 256, n - 1])):
            if offset >= n:
                continue
            for count in sorted(set([n - offset, (n - offset + 1) // 2])):
                for name in ('x', 'h', 'm', USER, STRIDED + '__1'):
                    serial += 1
                    vals = -(serial * 1e7 + np.arange(offset, offset + count, dtype=np.float64))
                    if name.startswith(STRIDED):
                        for a in (m.exp[STRIDED], m.pa.properties[STRIDED]):
                            a[1 + 3 * offset:3 * (offset + count):3] = vals
                    else:
                        m.exp[name][offset:offset + count] = vals
                        m.pa.properties[name][offset:offset + count] = vals
                    m.push_rows(name, offset, vals)
                    assert bits_equal(m.pull(name, offset, count), vals), (name, offset, count)
                m.check('push offset %d count %d' % (offset, count))
            # one row too many: refused on the host (sph_ctx.hip: the range check comes before the copy)
            buf = np.zeros(n - offset + 1)
            for fn in (m.lib.sph_array_push, m.lib.sph_array_pull):
                with pytest.raises(SphError, match=r'> n=%d' % n):
                    m.dev._check(fn(m.h, m.aid, m.dev.prop_id('x'), buf.ctypes.data_as(m.dev._PD), offset, n - offset + 1))
            assert np.all(buf == 0.0)
        for offset in (0, n):                     # count == 0: accepted up to offset == n, and nothing moves
            m.push_rows('x', offset, np.zeros(0))
            assert m.pull('x', offset, 0).size == 0
        with pytest.raises(SphError):
            m.push_rows('x', n + 1, np.zeros(0))
        m.check('after the refused calls')


# ---------------------------------------------------------------------------------------------------------------------
# resize
# ---------------------------------------------------------------------------------------------------------------------
def test_resize_inside_and_past_the_capacity():
    """from 257 rows the capacity is 257 + 257/8 + 64 = 353: 353 rows fit, 354 reallocate; the old rows survive both
    and the new ones read 0 in every property, the device-only one included"""
    with Mirror(257) as m:
        m.add_devonly()
        ptr = m.gpu.x.data
        m.gpu.resize(353)
        m.grow_to(353)
        m.check('353 rows', n_real=353)
        assert m.gpu.x.data == ptr                      # no reallocation
        for name in ('x', USER):                        # the new rows get values that must survive the reallocation
            vals = -7e7 - np.arange(257, 353, dtype=np.float64)
            m.exp[name][257:] = vals
            m.pa.properties[name][257:] = vals
            m.push_rows(name, 257, vals)
        m.devonly[257:] = -8e7 - np.arange(257, 353)
        m.push_rows(DEVONLY, 257, m.devonly[257:])
        m.gpu.resize(354)
        m.grow_to(354)
        m.check('354 rows', n_real=354)
        m.gpu.resize(2000)
        m.grow_to(2000)
        m.check('2000 rows', n_real=2000)


@pytest.mark.parametrize('how', ['resize', 'extend'])
@pytest.mark.parametrize('n', SIZES)
def test_shrink_then_grow_exposes_zeros(n, how):
    """finding A: ParticleArray.resize zero-fills and extend promises zero-valued particles, so the rows a shrink
    dropped must not come back when the array grows again inside its capacity (sph_array_resize clears nothing:
    HipDeviceHelper.resize / extend zero the rows they add).  Before that fix the device kept them: n = 257, shrink to 128, grow to 257 read x[128:257] = 1000128.0 .. 1000256.0 (the old
    values) where the host has 0.0 -- from row n // 2 on, for every n here and both ways of growing."""
    with Mirror(n) as m:
        m.add_devonly()
        keep = n // 2                                   # (n = 1: shrink to 0, then grow)
        m.gpu.resize(keep)
        m.shrink(keep)
        m.check('shrunk to %d' % keep, n_real=keep)
        if how == 'resize':
            m.gpu.resize(n)
        else:
            m.gpu.extend(n - keep)
        m.grow_to(n)
        m.check('grown back to %d by %s' % (n, how))


def test_shrink_to_zero_then_grow_and_refusals():
    from pysph_amd.device import SphError
    with Mirror(257) as m:
        m.add_devonly()
        with pytest.raises(SphError, match='n_real 258 > n 257'):        # refused, sizes as they were
            m.dev._check(m.lib.sph_array_resize(m.h, m.aid, 257, 258))
        m.check('after the refused resize', n_real=257)
        m.gpu.resize(0)
        m.shrink(0)
        m.check('empty', n_real=0)
        m.gpu.resize(300)
        m.grow_to(300)
        m.check('300 rows from none')
        m.gpu.resize(0)
        m.shrink(0)
        m.gpu.extend(65)
        m.grow_to(65)
        m.check('65 rows from none by extend')


# ---------------------------------------------------------------------------------------------------------------------
# permute / align
# ---------------------------------------------------------------------------------------------------------------------
def gather_indices(kind, n):
    rng = np.random.default_rng(1000 + n)
    if kind == 'identity':
        return np.arange(n)
    if kind == 'reversal':
        return np.arange(n)[::-1].copy()
    if kind == 'random':
        return rng.permutation(n)
    if kind == 'repeated':
        return rng.integers(0, n, n)
    if kind == 'keep':          # drops the first row, the last row and every row at a position = 255, 256 (mod 256)
        keep = np.ones(n, dtype=bool)
        keep[0] = keep[-1] = False
        keep[255::256] = False
        keep[256::256] = False
        return np.nonzero(keep)[0]
    assert kind == 'none'
    return np.zeros(0, dtype=np.int64)


@pytest.mark.parametrize('kind', ['identity', 'reversal', 'random', 'repeated', 'keep', 'none'])
@pytest.mark.parametrize('n', SIZES)
def test_align_gathers_rows(n, kind):
    """new row i = old row idx[i] in every property (strided ones move as rows); what a shorter gather drops does not
    come back: extend exposes zeros.  (kind 'none', n_new == 0, launches no gather at all: before extend zeroed the
    rows it adds, it exposed every old row, x[0] = 1000000.0 for 0.0.)"""
    idx = gather_indices(kind, n)
    with Mirror(n) as m:
        m.add_devonly()
        m.gpu.align(idx)
        m.take(idx)
        m.check('align %s' % kind, n_real=idx.size)
        if idx.size < n:
            m.gpu.extend(n - idx.size)
            m.grow_to(n)
            m.check('extend after align %s' % kind)


def test_permute_refusals_leave_the_state_untouched():
    """both checks of sph_array_permute run on the host before anything is copied or launched"""
    from pysph_amd.device import SphError
    n = 257
    with Mirror(n) as m:
        m.add_devonly()
        idx = np.arange(n, dtype=np.uint32)
        idx[256] = n                                           # one index == n
        with pytest.raises(SphError, match='index 257 out of range'):
            m.dev._check(m.lib.sph_array_permute(m.h, m.aid, idx.ctypes.data_as(m.dev._PU), n, n))
        m.check('index == n', n_real=n)
        idx = np.zeros(n + 1, dtype=np.uint32)                 # more indices than rows
        with pytest.raises(SphError, match='258 indices for 257 particles'):
            m.dev._check(m.lib.sph_array_permute(m.h, m.aid, idx.ctypes.data_as(m.dev._PU), n + 1, n + 1))
        m.check('n + 1 indices', n_real=n)
        with pytest.raises(SphError):                          # n_real_new > n_new
            m.dev._check(m.lib.sph_array_permute(m.h, m.aid, idx.ctypes.data_as(m.dev._PU), 5, 6))
        m.check('n_real_new > n_new', n_real=n)


# ---------------------------------------------------------------------------------------------------------------------
# the structural operations of HipDeviceHelper, tags interleaved across the block boundaries
# ---------------------------------------------------------------------------------------------------------------------
STRUCT_SIZES = [257, 1025]


@pytest.mark.parametrize('n', STRUCT_SIZES)
def test_align_particles_is_stable(n):
    with Mirror(n, mixed_tags=True) as m:
        m.add_devonly()
        m.gpu.align_particles()
        n_real = m.align_expected()
        assert n_real == (n + 1) // 2
        m.check('align_particles', n_real=n_real)
        m.check_rows('align_particles')
        assert np.all(np.diff(m.pa.gid[:n_real].astype(np.int64)) > 0)      # stable: ids ascend among the Local rows
        assert np.all(np.diff(m.pa.gid[n_real:].astype(np.int64)) > 0)      # ... and among the others
        m.gpu.align_particles()                                             # again: nothing moves
        m.check('align_particles twice', n_real=n_real)


@pytest.mark.parametrize('which', ['some', 'all', 'none'])
@pytest.mark.parametrize('n', STRUCT_SIZES)
def test_remove_particles(n, which):
    rng = np.random.default_rng(n)
    gone = {'some': np.unique(np.concatenate([[0, 255, 256, n - 1], rng.integers(0, n, n // 3)])),
            'all': np.arange(n), 'none': np.zeros(0, dtype=np.int64)}[which]
    with Mirror(n, mixed_tags=True) as m:
        m.add_devonly()
        m.gpu.remove_particles(gone)
        keep = np.ones(n, dtype=bool)
        keep[gone] = False
        m.take(np.nonzero(keep)[0])
        n_real = m.align_expected()
        m.check('remove_particles %s' % which, n_real=n_real)
        m.check_rows('remove_particles %s' % which)
        assert m.n == n - gone.size
        if which == 'all':                      # ... and the array can be used again: new rows read 0
            m.gpu.extend(70)
            m.grow_to(70)
            m.check('extend after removing everything')


@pytest.mark.parametrize('tag', [0, 1, 2, 3])
@pytest.mark.parametrize('n', STRUCT_SIZES)
def test_remove_tagged_particles(n, tag):
    with Mirror(n, mixed_tags=True) as m:
        m.add_devonly()
        m.gpu.remove_tagged_particles(tag)
        m.take(np.nonzero(m.exp['tag'] != tag)[0])
        n_real = m.align_expected()
        assert n_real == (0 if tag == 0 else (n + 1) // 2)
        m.check('remove_tagged_particles(%d)' % tag, n_real=n_real)
        m.check_rows('remove_tagged_particles(%d)' % tag)


def new_rows(m, ids):
    """property values of new particles `ids` in the array's own coding: x, the user property, the strided one and
    the integer metadata are given, every other property is left to its default"""
    ids = np.asarray(ids, dtype=np.int64)
    f = ids.astype(np.float64)
    return {'x': m.code('x') + f, USER: m.code(USER) + f,
            STRIDED: (m.code(STRIDED) + f[:, None] + 0.25 * np.arange(3)[None, :]).ravel(),
            'gid': ids.astype(np.uint32), 'pid': (ids % 5).astype(np.int32), 'tag': tag_pattern(ids)}


@pytest.mark.parametrize('n', STRUCT_SIZES)
def test_add_particles(n):
    with Mirror(n, mixed_tags=True) as m:
        m.add_devonly()
        rows = new_rows(m, np.arange(n, n + 70))
        m.gpu.add_particles(**rows)
        m.append_rows(rows)
        n_real = m.align_expected()
        m.check('add_particles', n_real=n_real)
        m.check_rows('add_particles')
        assert np.count_nonzero(m.exp['h'] == 0.0) == 70 and np.count_nonzero(m.devonly == 0.0) == 70


@pytest.mark.parametrize('n', STRUCT_SIZES)
def test_add_particles_after_a_shrink(n):
    """finding A through add_particles: the properties that are not given (and the device-only one) read 0 on the
    new rows although the rows a shrink dropped lie in the same storage"""
    with Mirror(n) as m:
        m.add_devonly()
        m.gpu.resize(n - 70)
        m.shrink(n - 70)
        rows = new_rows(m, np.arange(n, n + 70))
        rows['tag'] = np.zeros(70, dtype=np.int32)
        m.gpu.add_particles(**rows)
        m.append_rows(rows)
        m.check('add_particles after a shrink', n_real=n)


@pytest.mark.parametrize('n', STRUCT_SIZES)
def test_append_parray(n):
    with Mirror(n, mixed_tags=True) as m:
        m.add_devonly()
        other = Mirror(70, name='other', attach=False)
        other.fill_rows(other.pa, np.arange(n, n + 70), True)
        m.gpu.append_parray(other.pa)
        m.append_rows(dict((k, a.copy()) for k, a in other.pa.properties.items()))
        n_real = m.align_expected()
        m.check('append_parray', n_real=n_real)
        m.check_rows('append_parray')
        m.gpu.append_parray(other.pa.extract_particles(np.zeros(0, dtype=np.int64)))      # no rows: a no-op
        m.check('append_parray of an empty array', n_real=n_real)


@pytest.mark.parametrize('n', STRUCT_SIZES)
def test_extract_particles_into_an_array_that_holds_rows(n):
    """the DEVICE values of the chosen rows land behind the rows the destination has, then real rows first"""
    rng = np.random.default_rng(n)
    with Mirror(n, mixed_tags=True) as m:
        dest = Mirror(6, name='dest', attach=False)
        dest.fill_rows(dest.pa, np.arange(5000, 5006), True)
        before = dict((k, a.copy()) for k, a in dest.pa.properties.items())
        m.push_rows('x', 0, m.exp['x'] + 0.5)            # the device differs from the host copy
        idx = np.concatenate([[n - 1, 0, 256, 255], rng.integers(0, n, 40)])
        out = m.gpu.extract_particles(idx, dest.pa)
        assert out is dest.pa
        want = {}
        for key, a in before.items():
            st = m.stride(key)
            src = m.exp[key] + (0.5 if key == 'x' else 0)
            rows = src[idx] if st == 1 else src.reshape(-1, st)[idx].ravel()
            want[key] = np.concatenate([a, rows.astype(a.dtype)])
        order = np.argsort(want['tag'] != 0, kind='stable')
        for key, a in want.items():
            st = m.stride(key)
            a = a[order] if st == 1 else a.reshape(-1, st)[order].ravel()
            assert bits_equal(out.properties[key], a), key
        assert out.get_number_of_particles() == 6 + idx.size
        assert out.get_number_of_particles(True) == int(np.count_nonzero(want['tag'] == 0))
        m.push_rows('x', 0, m.exp['x'])
        m.check('the source is untouched', n_real=n)
        clone = m.gpu.extract_particles(np.zeros(0, dtype=np.int64))         # no rows into a fresh clone
        assert clone.get_number_of_particles() == 0


# ---------------------------------------------------------------------------------------------------------------------
# sph_array_fill
# ---------------------------------------------------------------------------------------------------------------------
def test_fill_ranges_around_a_block_boundary():
    from pysph_amd.device import SphError
    n = 600
    with Mirror(n) as m:
        for s in (0, 255, 256, 257):
            for e in (255, 256, 257, n):
                if s > e:
                    continue
                for name in ('x', USER):
                    value = -(1000.0 * s + e) - 0.5
                    m.dev._check(m.lib.sph_array_fill(m.h, m.aid, m.dev.prop_id(name), value, s, e - s))
                    m.exp[name][s:e] = value
                    m.pa.properties[name][s:e] = value
                m.check('fill [%d, %d)' % (s, e))          # the rows outside the range are untouched
        with pytest.raises(SphError, match='> n=600'):     # refused on the host before the launch
            m.dev._check(m.lib.sph_array_fill(m.h, m.aid, m.dev.prop_id('x'), 1.0, 257, n - 257 + 1))
        m.check('after the refused fill')


def test_fill_of_x_is_seen_by_the_next_neighbour_update(oracle):
    """positions written by sph_array_fill may lie anywhere: the next update must look at the particles instead of
    binning on the bounds of the update before (the bounds are the CPU oracle's for the same positions)"""
    from pysph_amd import device as dev
    from pysph_amd.nnps import HipNNPS
    from pysph_amd.particle_array import get_particle_array
    rng = np.random.default_rng(5)
    n = 300
    pa = get_particle_array(name='cloud', x=rng.uniform(0, 1, n), y=rng.uniform(0, 1, n), z=rng.uniform(0, 1, n),
                            h=np.full(n, 0.1))
    ctx = dev.HipContext(0)
    try:
        gpu = dev.attach(pa, ctx)
        gpu.push()
        nn = HipNNPS(3, [pa], radius_scale=2.0, ctx=ctx, sync=False)
        nn.update()
        nn.update()                                     # steady state: an update that may reuse what it knows
        on = oracle.OracleNNPS(3, [pa], radius_scale=2.0)
        on.update()
        assert np.array_equal(nn.xmin, on.xmin) and np.array_equal(nn.xmax, on.xmax)
        xmax0 = nn.xmax.copy()
        dev._check(ctx.lib.sph_array_fill(ctx._h, gpu.array_id, dev.prop_id('x'), 5.0, 255, n - 255))
        pa.x[255:] = 5.0
        nn.update()
        on.update()
        assert np.array_equal(nn.xmin, on.xmin) and np.array_equal(nn.xmax, on.xmax)
        assert nn.xmax[0] >= 5.0 > xmax0[0]
        assert list(nn.ncells_per_dim) == list(on.ncells_per_dim)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# the gather of sph_nnps_reorder_array
# ---------------------------------------------------------------------------------------------------------------------
def test_reorder_array_gathers_every_property():
    from pysph_amd.device import SphError
    from pysph_amd.nnps import HipNNPS
    n = 1025
    with Mirror(n, positions=True) as m:
        m.add_devonly()
        nn = HipNNPS(3, [m.pa], radius_scale=2.0, ctx=m.ctx, sync=False)
        order = nn.get_spatially_ordered_indices(0).astype(np.int64)
        assert np.array_equal(np.sort(order), np.arange(n)) and not np.array_equal(order, np.arange(n))
        m.dev._check(m.lib.sph_nnps_reorder_array(m.h, m.aid))
        host = dict((k, a.copy()) for k, a in m.exp.items())
        m.take(order)                                   # every property equals host[order] ...
        m.check_device('reordered')
        for key, a in host.items():                     # ... while the host array is left alone
            assert bits_equal(m.pa.properties[key], a), key
        with pytest.raises(SphError, match='one reorder per update'):      # refused on the host: the order is used up
            m.dev._check(m.lib.sph_nnps_reorder_array(m.h, m.aid))
        m.check_device('after the refused reorder')


# ---------------------------------------------------------------------------------------------------------------------
# reductions
# ---------------------------------------------------------------------------------------------------------------------
RED_SIZES = [1, 63, 64, 65, 255, 256, 257, 131071, 131072, 131073, 131072 + 257]
RED_SMALL = [1, 65, 257, 131073]
GHOSTS = 70
DBL_MAX = sys.float_info.max


class Reducer(object):
    """n_real real rows and GHOSTS ghost rows behind them; `rho` is reduced with max and carries +5 on its ghost rows,
    `p` with min and carries -5 there: would-be extrema that "the first n_real particles" (sphhip.h) excludes"""

    def __init__(self, n_real, ghosts=GHOSTS):
        from pysph_amd import device as dev
        from pysph_amd.particle_array import ParticleArray
        self.dev, self.n_real, self.n = dev, n_real, n_real + ghosts
        pa = ParticleArray(name='red', rho=np.zeros(self.n), p=np.zeros(self.n))
        pa.tag[n_real:] = 1
        pa.set_num_real_particles(n_real)
        self.pa = pa
        self.ctx = dev.HipContext(0)
        self.gpu = dev.attach(pa, self.ctx)
        assert self.gpu.get_number_of_particles(True) == n_real and self.gpu.get_number_of_particles() == self.n

    def set(self, for_max, for_min=None):
        pa = self.pa
        pa.rho[:self.n_real] = for_max
        pa.rho[self.n_real:] = 5.0
        pa.p[:self.n_real] = for_max if for_min is None else for_min
        pa.p[self.n_real:] = -5.0
        self.gpu.push('rho', 'p')

    def poke(self, name, row, value):
        buf = np.array([value])
        self.dev._check(self.ctx.lib.sph_array_push(self.ctx._h, self.gpu.array_id, self.dev.prop_id(name),
                                                    buf.ctypes.data_as(self.dev._PD), row, 1))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.close()


@pytest.mark.parametrize('n_real', RED_SIZES)
def test_reduce_planted_extremum(n_real):
    """random values in [-1, 1] and one planted extremum at each wavefront / block / grid-stride boundary the size
    has; 131072 = 512 blocks of 256 is where the grid-stride loop and the 512-partial second pass begin"""
    rng = np.random.default_rng(n_real)
    base = rng.uniform(-1.0, 1.0, n_real)
    with Reducer(n_real) as r:
        r.set(base)
        assert r.gpu.max('rho') == np.max(base) and r.gpu.min('p') == np.min(base)
        rows = [0, 63, 64, 255, 256, n_real - 1, 131071, 131072, (n_real - 1) // 64 * 64]
        for row in sorted(set(k for k in rows if k < n_real)):
            host = base.copy()
            host[row] = 2.0
            r.poke('rho', row, 2.0)
            got = r.gpu.max('rho')
            assert got == np.max(host) == 2.0, ('max', row, got)
            r.poke('rho', row, base[row])
            host[row] = -2.0
            r.poke('p', row, -2.0)
            got = r.gpu.min('p')
            assert got == np.min(host) == -2.0, ('min', row, got)
            r.poke('p', row, base[row])
        assert r.gpu.max('rho') == np.max(base) and r.gpu.min('p') == np.min(base)


@pytest.mark.parametrize('n_real', RED_SMALL)
def test_reduce_one_sign_and_signed_zeros(n_real):
    rng = np.random.default_rng(n_real)
    with Reducer(n_real) as r:
        neg, pos = rng.uniform(-2.0, -1.0, n_real), rng.uniform(1.0, 2.0, n_real)
        r.set(neg, pos)                 # the sign trick of min must not leak the initial value
        assert r.gpu.max('rho') == np.max(neg) and r.gpu.min('p') == np.min(pos)
        tiny = rng.uniform(1.0, 2.0, n_real) * 1e-300
        r.set(-tiny, tiny)
        assert r.gpu.max('rho') == np.max(-tiny) and r.gpu.min('p') == np.min(tiny)
        zeros = np.where(rng.integers(0, 2, n_real) == 1, 0.0, -0.0)
        r.set(zeros)
        # -0.0 and +0.0 compare equal and fmax may return either: the sign bit of the result is not asserted
        assert r.gpu.max('rho') == 0.0 and r.gpu.min('p') == 0.0
        r.set(np.full(n_real, -0.0))
        assert r.gpu.max('rho') == 0.0 and r.gpu.min('p') == 0.0


@pytest.mark.parametrize('n_real', RED_SMALL)
def test_reduce_infinities(n_real):
    """finding B: k_max started from -DBL_MAX, so max over a range of nothing but -inf gave -1.7976931348623157e308
    (and min over +inf the same with the other sign) at every size here; numpy gives the infinity"""
    rng = np.random.default_rng(n_real)
    inf = float('inf')
    with Reducer(n_real) as r:
        r.set(np.full(n_real, -inf), np.full(n_real, inf))
        assert r.gpu.max('rho') == np.max(np.full(n_real, -inf)) == -inf
        assert r.gpu.min('p') == np.min(np.full(n_real, inf)) == inf
        vals = rng.uniform(-1.0, 1.0, n_real)
        hi, lo = vals.copy(), vals.copy()
        hi[n_real - 1] = inf
        lo[n_real // 2] = -inf
        r.set(hi, lo)
        assert r.gpu.max('rho') == np.max(hi) == inf and r.gpu.min('p') == np.min(lo) == -inf
        r.set(lo, hi)                     # an infinity of the other sign does not win
        assert r.gpu.max('rho') == np.max(lo) and r.gpu.min('p') == np.min(hi)


@pytest.mark.parametrize('n_real', RED_SMALL)
def test_reduce_ignores_nan_rows(n_real):
    """the stated contract of sph_reduce_max / min (sphhip.h): a NaN row is ignored (numpy and the host path of
    Integrator._reduce propagate it), and an all-NaN range yields the identity"""
    rng = np.random.default_rng(n_real)
    nan, inf = float('nan'), float('inf')
    with Reducer(n_real) as r:
        vals = rng.uniform(-1.0, 1.0, n_real)
        vals[0] = nan
        vals[(n_real - 1) // 64 * 64] = nan
        vals[n_real - 1] = nan if n_real > 65 else vals[n_real - 1]
        if np.all(np.isnan(vals)):
            want_max, want_min = -inf, inf
        else:
            want_max, want_min = np.nanmax(vals), np.nanmin(vals)
        r.set(vals)
        assert r.gpu.max('rho') == want_max and r.gpu.min('p') == want_min
        r.set(np.full(n_real, nan))
        assert r.gpu.max('rho') == -inf and r.gpu.min('p') == inf


def test_reduce_empty_ranges_and_missing_property():
    from pysph_amd.device import SphError
    with Reducer(0) as r:                            # n_real == 0 with 70 ghost rows
        r.set(np.zeros(0))
        assert r.gpu.max('rho') == -DBL_MAX and r.gpu.min('p') == DBL_MAX
        with pytest.raises(SphError, match='error -5'):                  # SPH_ERR_MISSING_PROP: no device storage
            r.gpu.max('cs')
        with pytest.raises(SphError, match='error -5'):
            r.gpu.min('cs')
    with Reducer(0, ghosts=0) as r:                  # n == 0
        r.dev._check(r.ctx.lib.sph_array_ensure_prop(r.ctx._h, r.gpu.array_id, r.dev.prop_id('rho')))
        r.dev._check(r.ctx.lib.sph_array_ensure_prop(r.ctx._h, r.gpu.array_id, r.dev.prop_id('p')))
        assert r.gpu.max('rho') == -DBL_MAX and r.gpu.min('p') == DBL_MAX


def test_dt_adapt_of_an_array_of_ghosts_is_no_constraint():
    """finding C: the device reduces over the real rows, so a device-resident array whose rows are all ghosts has
    nothing to say; the reference's answer for "no constraint" is inf (integrator.py:83-117).  Before the fix the
    empty range's DBL_MAX passed ``dt_min > 0`` and compute_time_step returned 1.7976931348623157e308.  The
    acceleration evaluator is a stand-in with exactly what Integrator._reduce reads of one."""
    from pysph_amd import device as dev
    from pysph_amd.integrator import Integrator, WCSPHStep
    from pysph_amd.particle_array import ParticleArray
    n = 70
    pa = ParticleArray(name='fluid', x=np.zeros(n), h=np.ones(n), dt_adapt=np.full(n, 0.01))
    pa.dt_adapt[:35] = 0.25
    pa.tag[35:] = 1
    pa.set_num_real_particles(35)
    ctx = dev.HipContext(0)
    try:
        gpu = dev.attach(pa, ctx)
        gpu.push('dt_adapt', 'h')
        ev = types.SimpleNamespace(sync='manual', outputs={'fluid': ('dt_adapt',)}, outputs_exact={})
        integ = Integrator(fluid=WCSPHStep())
        integ.set_acceleration_evals([types.SimpleNamespace(particle_arrays=[pa], c_acceleration_eval=ev)])
        # the device path is the one taken: the ghost rows' smaller value does not count
        assert integ.compute_time_step(1e-3, 0.3) == 0.25
        pa.tag[:] = 1
        pa.set_num_real_particles(0)
        gpu.push('dt_adapt')                       # (takes the new real count to the device)
        assert gpu.get_number_of_particles(True) == 0 and gpu.get_number_of_particles() == n
        got = integ.compute_time_step(1e-3, 0.3)
        assert got == float('inf'), got
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# the stage sweep at block edges
# ---------------------------------------------------------------------------------------------------------------------
EPS = 2.0 ** -52
_XYZ0 = ['x0', 'y0', 'z0', 'u0', 'v0', 'w0']
_HAT = ['uhat', 'vhat', 'what', 'auhat', 'avhat', 'awhat']
STEPPERS = {
    'wcsph': (1, ['x', 'y', 'z', 'u', 'v', 'w', 'rho'] + _XYZ0 + ['rho0', 'au', 'av', 'aw', 'ax', 'ay', 'az', 'arho']),
    'tvf': (2, ['x', 'y', 'z', 'u', 'v', 'w', 'au', 'av', 'aw', 'vmag2'] + _HAT),
    'solid': (3, None),          # filled below from the oracle's table
    'edac': (6, ['x', 'y', 'z', 'u', 'v', 'w', 'p'] + _XYZ0 + ['p0', 'au', 'av', 'aw', 'ax', 'ay', 'az', 'ap']),
    'edac_tvf': (7, ['x', 'y', 'z', 'u', 'v', 'w', 'p'] + _XYZ0 + ['p0', 'au', 'av', 'aw', 'ap'] + _HAT),
    'gasd': (8, ['x', 'y', 'z', 'u', 'v', 'w', 'e', 'h', 'rho'] + _XYZ0 + ['e0', 'h0', 'rho0', 'au', 'av', 'aw', 'ae',
                 'ah', 'arho', 'converged', 'omega', 'alpha1', 'alpha2', 'alpha10', 'alpha20', 'aalpha1', 'aalpha2']),
    'gsph': (9, ['x', 'y', 'z', 'u', 'v', 'w', 'e', 'au', 'av', 'aw', 'ae']),
}
STAGE_DT = 3.7e-3


def stepper_props(tag):
    from oracle import steppers as S
    kind, names = STEPPERS[tag]
    if names is None:
        names = [q for t in S._SM for q in t]
    return kind, names


def twin_stage(tag, pa, dt, stage):
    """the numpy stepper of oracle/steppers.py on the real rows of `pa` (the stages defined as no-ops do nothing)"""
    from oracle import steppers as S
    if tag == 'wcsph':
        S.wcsph_initialize(pa) if stage == 0 else S.wcsph_stage(pa, dt, stage)
    elif tag == 'solid':
        S.solid_initialize(pa) if stage == 0 else S.solid_stage(pa, dt, stage)
    elif tag == 'tvf':
        if stage == 1:
            S.tvf_stage1(pa, dt)
        elif stage == 2:
            S.tvf_stage2(pa, dt)
    elif tag in ('edac', 'edac_tvf'):
        S.edac_initialize(pa) if stage == 0 else S.edac_stage(pa, dt, stage, tag == 'edac_tvf')
    elif tag == 'gasd':
        S.gasd_initialize(pa) if stage == 0 else S.gasd_stage(pa, dt, stage)
    elif tag == 'gsph':
        if stage == 1:
            S.gsph_stage1(pa, dt)


def stage_bounds(tag, stage, pre, post, dt):
    """{property: per-row bound on |device - numpy|}; a property that is not named is bit-exact.

    The device may contract q0 + f*a into one fma where numpy rounds the product and the sum: the two differ by at
    most one rounding of the product plus one of the sum, |got - want| <= 2^-52 (|q0| + |f a|).  Where an update
    reads the result of another (uhat from u, x from uhat or u), the bound of the input is carried through the
    coefficient it is multiplied with and the operation adds its own 2^-52 (sum of the absolute terms).  Copies
    (stage 0), everything GSPH does (compiled with contraction off) and every property a stage does not write are
    bit-exact."""
    from oracle import steppers as S
    if stage == 0 or tag == 'gsph':
        return {}
    ab = np.abs
    f = 0.5 * dt if stage == 1 else dt
    b = {}

    def axpy(q, q0, aq, f=f):
        b[q] = EPS * (ab(pre[q0]) + ab(f * pre[aq]))

    if tag in ('wcsph', 'solid'):
        table = S._SM if tag == 'solid' else [(q, q + '0', 'a' + q) for q in ('u', 'v', 'w', 'x', 'y', 'z', 'rho')]
        for q, q0, aq in table:
            axpy(q, q0, aq)
    elif tag == 'tvf':
        dtb2 = 0.5 * dt
        for q in 'uvw':
            axpy(q, q, 'a' + q, dtb2)
        if stage == 1:
            for q, x in zip('uvw', 'xyz'):
                qh = q + 'hat'
                b[qh] = b[q] + EPS * (ab(post[q]) + ab(dtb2 * pre['a' + qh]))
                b[x] = dt * b[qh] + EPS * (ab(pre[x]) + ab(dt * post[qh]))
        else:
            # u u + v v + w w: three products and two sums on either side, each within three half-ulp roundings of
            # the sum of the absolute terms, plus the bound of u, v, w carried through d(q^2) = 2 |q| dq + dq^2
            sq = post['u'] ** 2 + post['v'] ** 2 + post['w'] ** 2
            b['vmag2'] = 3 * EPS * sq + sum(2 * ab(post[q]) * b[q] + b[q] ** 2 for q in 'uvw')
    elif tag in ('edac', 'edac_tvf'):
        for q in 'uvw':
            axpy(q, q + '0', 'a' + q)
        axpy('p', 'p0', 'ap')
        for q, x in zip('uvw', 'xyz'):
            if tag == 'edac':
                axpy(x, x + '0', 'a' + x)
            else:
                qh = q + 'hat'
                b[qh] = b[q] + EPS * (ab(post[q]) + ab(f * pre['a' + qh]))
                b[x] = f * b[qh] + EPS * (ab(pre[x + '0']) + ab(f * post[qh]))
    elif tag == 'gasd':
        for q, x in zip('uvw', 'xyz'):
            axpy(q, q + '0', 'a' + q)
            b[x] = f * b[q] + EPS * (ab(pre[x + '0']) + ab(f * post[q]))
        axpy('e', 'e0', 'ae')
        if stage == 1:
            axpy('h', 'h0', 'ah')
            axpy('rho', 'rho0', 'arho')
        axpy('alpha1', 'alpha10', 'aalpha1')
        axpy('alpha2', 'alpha20', 'aalpha2')
    return b


def stage_inputs(names, n, seed):
    """random, distinct per property, magnitudes spread over 1e-3 .. 1e3, mixed signs"""
    rng = np.random.default_rng(seed)
    return dict((k, 10.0 ** rng.uniform(-3.0, 3.0, n) * rng.choice([-1.0, 1.0], n)) for k in names)


@pytest.mark.parametrize('ghosts', [0, 70])
@pytest.mark.parametrize('n_real', [1, 255, 256, 257, 1025])
@pytest.mark.parametrize('tag', sorted(STEPPERS))
def test_stage_sweep_at_block_edges(tag, n_real, ghosts):
    """every stage 0 / 1 / 2 of every stepper the sweep knows (the no-op stages included) against its numpy twin on
    the rows [0, n_real); the ghost rows behind, and every property a stage does not write, stay bit-identical"""
    from pysph_amd import device as dev
    from pysph_amd.particle_array import ParticleArray
    kind, names = stepper_props(tag)
    n = n_real + ghosts
    props = stage_inputs(names, n, 7 * n_real + ghosts)
    pa = ParticleArray(name='fluid', **dict((k, v.copy()) for k, v in props.items()))
    ref = ParticleArray(name='fluid', **dict((k, v.copy()) for k, v in props.items()))
    for a in (pa, ref):
        a.tag[n_real:] = 1
        a.set_num_real_particles(n_real)
    ctx = dev.HipContext(0)
    try:
        gpu = dev.attach(pa, ctx)
        gpu.push(*names)
        assert gpu.get_number_of_particles(True) == n_real and gpu.get_number_of_particles() == n
        for stage in (0, 1, 2):
            pre = dict((k, ref.properties[k].copy()) for k in names)
            twin_stage(tag, ref, STAGE_DT, stage)
            post = dict((k, ref.properties[k]) for k in names)
            bounds = stage_bounds(tag, stage, pre, post, STAGE_DT)
            dev._check(ctx.lib.sph_integrate_stage(ctx._h, gpu.array_id, kind, stage, STAGE_DT))
            gpu.pull(*names)
            changed = 0
            for k in names:
                got, want = pa.properties[k], post[k]
                assert bits_equal(got[n_real:], pre[k][n_real:]), (tag, stage, k, 'ghost rows')
                if k in bounds:
                    err = np.abs(got[:n_real] - want[:n_real])
                    worst = int(np.argmax(err - bounds[k][:n_real]))
                    assert np.all(err <= bounds[k][:n_real]), (tag, stage, k, worst, err[worst], bounds[k][worst])
                else:
                    assert bits_equal(got[:n_real], want[:n_real]), (tag, stage, k)
                changed += not bits_equal(want, pre[k])
            noop = (tag == 'tvf' and stage == 0) or (tag == 'gsph' and stage != 1)
            assert (changed == 0) == noop, (tag, stage, changed)       # the twin itself moved something
            for k in names:                  # the next stage starts from the device's state on both sides
                ref.properties[k][:] = pa.properties[k]
    finally:
        ctx.close()


@pytest.mark.parametrize('tag', sorted(STEPPERS))
def test_stage_sweep_without_real_rows(tag):
    """n_real == 0 with n == 70: every stage succeeds, nothing changes, and the properties the stages need have
    device storage afterwards (zero-filled: only x was ever pushed)"""
    from pysph_amd import device as dev
    from pysph_amd.particle_array import ParticleArray
    kind, names = stepper_props(tag)
    n = 70
    x = 1e6 + np.arange(n, dtype=np.float64)
    pa = ParticleArray(name='fluid', x=x.copy())
    pa.tag[:] = 1
    pa.set_num_real_particles(0)
    ctx = dev.HipContext(0)
    try:
        gpu = dev.attach(pa, ctx)
        gpu.push('x')
        for stage in (0, 1, 2):
            dev._check(ctx.lib.sph_integrate_stage(ctx._h, gpu.array_id, kind, stage, STAGE_DT))
        assert gpu.get_number_of_particles(True) == 0 and gpu.get_number_of_particles() == n
        have = set(gpu.device_props())
        out = np.empty(n)
        for k in names:
            pid = dev.prop_id(k)
            assert pid >= 0 and pid in have, k
            dev._check(ctx.lib.sph_array_pull(ctx._h, gpu.array_id, pid, out.ctypes.data_as(dev._PD), 0, n))
            assert bits_equal(out, x if k == 'x' else np.zeros(n)), k
    finally:
        ctx.close()


def _cloud(names, n, seed):
    rng = np.random.default_rng(seed)
    props = dict((k, np.zeros(n)) for k in names)
    for k in 'xyz':
        props[k] = rng.uniform(0.0, 1.0, n)
    props['h'] = rng.uniform(0.08, 0.12, n)
    props['m'] = np.ones(n)
    return props, rng


def test_position_moving_stage_invalidates_the_neighbour_state():
    from pysph_amd import device as dev
    from pysph_amd.device import SphError
    from pysph_amd.nnps import HipNNPS
    from pysph_amd.particle_array import ParticleArray
    kind, names = stepper_props('wcsph')
    props, rng = _cloud(names + ['h'], 257, 11)
    props['ax'] = rng.uniform(-1.0, 1.0, 257)
    pa = ParticleArray(name='fluid', **props)
    ctx = dev.HipContext(0)
    try:
        dev.attach(pa, ctx).push(*props)
        nn = HipNNPS(3, [pa], radius_scale=2.0, ctx=ctx, sync=False)
        pairs = nn.count_neighbors(0, 0)
        assert pairs > 257
        dev._check(ctx.lib.sph_integrate_stage(ctx._h, pa.gpu.array_id, kind, 0, STAGE_DT))
        assert nn.count_neighbors(0, 0) == pairs               # the copies of stage 0 move nothing
        dev._check(ctx.lib.sph_integrate_stage(ctx._h, pa.gpu.array_id, kind, 1, STAGE_DT))
        with pytest.raises(SphError, match='call sph_nnps_update first'):      # refused on the host
            nn.count_neighbors(0, 0)
        nn.update()
        assert nn.count_neighbors(0, 0) > 257
    finally:
        ctx.close()


def test_gasd_stage1_h_is_seen_by_the_next_neighbour_update():
    """GasDFluidStep.stage1 predicts h: the next update bins on cells of radius_scale * max(h) of the NEW h
    (nnps_base.pyx:955-975), here a non-uniform one whose maximum differs from the old one's"""
    from pysph_amd import device as dev
    from pysph_amd.nnps import HipNNPS
    from pysph_amd.particle_array import ParticleArray
    kind, names = stepper_props('gasd')
    n = 300
    props, rng = _cloud(names, n, 12)
    props['ah'] = rng.uniform(-5.0, 5.0, n)
    props['rho'] = np.ones(n)
    pa = ParticleArray(name='fluid', **props)
    ctx = dev.HipContext(0)
    try:
        gpu = dev.attach(pa, ctx)
        gpu.push(*props)
        nn = HipNNPS(3, [pa], radius_scale=2.0, ctx=ctx, sync=False)
        assert nn.cell_size == 2.0 * props['h'].max()
        for stage in (0, 1):
            dev._check(ctx.lib.sph_integrate_stage(ctx._h, gpu.array_id, kind, stage, 0.01))
        nn.update()
        h_new = gpu.h.get()
        assert np.abs(h_new - (props['h'] + 0.005 * props['ah'])).max() < 1e-15
        assert h_new.max() != props['h'].max() and h_new.min() != props['h'].min()
        assert nn.cell_size == 2.0 * h_new.max()
        assert nn.hmin == 2.0 * h_new.min()
    finally:
        ctx.close()
