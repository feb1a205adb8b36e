"""The placed neighbour update (option sort_place, csrc/sph_nnps.hip: k_bin_place -> k_bucket_sort on the bucket table
of the previous update) and the mailbox by which a lagged update's bounds reach the host (plain stores + a sequence number
instead of a copy and an event).

Every case runs with sort_place 1 and 0 on the same inputs and compares the tables the ONE sort of an update leaves
(sorted position -> index, sorted fine keys, fine_start, cell_start, the slot bytes of a merged order) bit for bit, and
the order with numpy's stable argsort of the fine keys restated on the host.  Which updates must have placed, and how
many pairs must have gone through the overflow list, is PREDICTED here from the rule of DESIGN.md section 3 (class
Model below) -- bucket counts of the host keys, never from what the library did -- and compared with the counters
n_placed / n_place_overflow.

sort_lbits is 9 and the boxes have 10..11 cells a side: some twenty buckets of 64 cells.  Arrays are generated in cell
order and via_unordered is 0 except where that traversal is the subject: the few wavefronts of these sizes hit more than
n / 8 buckets even in cell order, which the library takes for "no spatial order" (and the `via` traversal never places).
Moving particles keep two resting ANCHOR particles in opposite corners of the box, so that the bounds -- the binning grid --
stay what they were; where the grid is meant to change, an anchor moves."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from pysph_amd.particle_array import get_particle_array
from test_particle_sort import cloud, host_fine_keys

pytestmark = pytest.mark.gpu

LBITS = 9
OVF_DIV = 256            # SORT_PLACE_OVF_DIV: beyond n / 256 pairs in the list the host last saw, the next update does not place
T_PERM, T_FKEYS, T_FINE_START, T_CELL_START, T_SLOT = range(5)
H = 0.05                 # cells of 0.1


def ordered_cloud(n, seed, name='a', lo=0.1, hi=0.9, anchors=True):
    """n random points of [lo, hi]^3 in cell order (z, y cell, then x); with anchors the first two rows are the corners
    (0, 0, 0) and (1, 1, 1) of the box and never move"""
    pa = cloud(n, seed, name=name, box=1.0, h=H)
    x, y, z = [lo + (hi - lo) * np.asarray(a) for a in (pa.x, pa.y, pa.z)]
    if anchors and n >= 2:
        order = 2 + np.lexsort((x[2:], np.floor(y[2:] / 0.1), np.floor(z[2:] / 0.1)))
        x = np.concatenate(([0.0, 1.0], x[order])); y = np.concatenate(([0.0, 1.0], y[order])); z = np.concatenate(([0.0, 1.0], z[order]))
    else:
        order = np.lexsort((x, np.floor(y / 0.1), np.floor(z / 0.1)))
        x, y, z = x[order], y[order], z[order]
    return get_particle_array(name=name, x=x, y=y, z=z, h=H * np.ones(n), m=np.ones(n))


def shift(pa, delta):
    """positions += delta (n x 3) in device memory, as a stage kernel moves particles; the host copy follows"""
    from helpers import device_add
    for k, f in enumerate('xyz'):
        device_add(pa, f, np.ascontiguousarray(delta[:, k]))


def jiggle(pa, seed, amp, rest=2):
    """uniform motion of +- amp / 2 per axis for every particle but the first `rest` (the anchors)"""
    rng = np.random.default_rng(seed)
    d = amp * (rng.random((pa.x.size, 3)) - 0.5)
    d[:rest] = 0.0
    shift(pa, d)


class Model:
    """which updates place, and their overflow, by the stated rule: a lagged update places when the previous update left a
    bucket table for the same binning grid, key split and array sizes, and the overflow the host last saw is at most
    n / OVF_DIV; pair number p of a bucket (arrival order) overflows when p >= the bucket's count in the previous update"""

    def __init__(self, place):
        self.place, self.prev, self.sig, self.seen = place, None, None, 0
        self.n_placed, self.n_overflow, self.log = 0, 0, []

    def forget(self):            # something else used the sort's tables
        self.prev = None

    def update(self, keys, lbits, grid, sizes, lagged, blocked=False):
        n = keys.size
        cnt = np.bincount(keys >> lbits).astype(np.int64)
        sig = (lbits, tuple(sizes)) + tuple(np.asarray(g).tobytes() for g in grid)
        if not lagged:
            self.seen = 0
        ok = (self.place and lagged and not blocked and self.prev is not None and self.sig == sig
              and self.seen * OVF_DIV <= n)
        ovf = 0
        if ok:
            m = max(cnt.size, self.prev.size)
            a, b = np.zeros(m, np.int64), np.zeros(m, np.int64)
            a[:cnt.size] = cnt; b[:self.prev.size] = self.prev
            ovf = int(np.maximum(a - b, 0).sum())
            self.n_placed += 1
        self.prev, self.sig = cnt, sig
        if lagged:               # the count travels with the bounds; the tests read the grid after every update
            self.seen = ovf
            self.n_overflow += ovf
        self.log.append((bool(ok), ovf))


def read_table(ctx, which, dtype):
    from pysph_amd import device as dev
    nb = C.c_size_t(0)
    dev._check(ctx.lib.sph_nnps_read_table(ctx._h, which, None, 0, C.byref(nb)))
    out = np.empty(nb.value // np.dtype(dtype).itemsize, dtype)
    if nb.value:
        dev._check(ctx.lib.sph_nnps_read_table(ctx._h, which, out.ctypes.data_as(C.c_void_p), nb.value, C.byref(nb)))
    return out


class Run:
    """one context, one neighbour search; update() records the tables, checks the stable order and the counters"""

    def __init__(self, arrays, place, opts=()):
        from pysph_amd import device as dev
        from pysph_amd.nnps import HipNNPS
        self.arrays, self.ctx = arrays, dev.HipContext(0)
        self.lbits = LBITS
        for k, v in (('sort_lbits', LBITS), ('sort_place', place), ('via_unordered', 0)) + tuple(opts):
            self.ctx.set_option(k, v)
        self.ctx.timer_enable(True)
        for a in arrays:
            dev.attach(a, self.ctx).push()
        self.model = Model(place)
        self.ndev = [a.get_number_of_particles() for a in arrays]    # rows on the device (sph_array_resize changes them)
        self.snaps, self.grid, self.n_async = [], None, 0
        self.nn = HipNNPS(3, arrays, radius_scale=2.0, ctx=self.ctx, sync=False)
        self._after_update(False)

    def count(self, key):
        return self.ctx.timer_get(key)[1]

    def update(self, blocked=False):
        self.nn.update()
        self._after_update(blocked)

    def _after_update(self, blocked):
        nn = self.nn
        reported = (np.array(nn.xmin), np.float64(nn.cell_size), np.array(nn.ncells_per_dim))    # (the host now holds the mailbox)
        n_async = self.count('n_async')
        lagged = n_async == self.n_async + 1
        assert lagged or n_async == self.n_async
        self.n_async = n_async
        grid = self.grid if lagged else reported       # a lagged update bins on the grid of the bounds before it
        self.grid = reported
        g = SimpleNamespace(xmin=grid[0], cell_size=float(grid[1]), ncells_per_dim=grid[2])
        keys = np.concatenate([host_fine_keys(SimpleNamespace(x=a.x[:n], y=a.y[:n], z=a.z[:n]), g)
                               for a, n in zip(self.arrays, self.ndev)]).astype(np.int64)
        self.model.update(keys, self.lbits, grid, self.ndev, lagged, blocked)
        snap = {'perm': read_table(self.ctx, T_PERM, np.uint32), 'fkeys': read_table(self.ctx, T_FKEYS, np.uint32),
                'fine_start': read_table(self.ctx, T_FINE_START, np.uint32), 'cell_start': read_table(self.ctx, T_CELL_START, np.uint32),
                'slot': read_table(self.ctx, T_SLOT, np.uint8)}
        # the order a stable sort of the host keys gives, the sorted keys and the table that falls out of them
        want = np.argsort(keys, kind='stable')
        off = np.concatenate(([0], np.cumsum(self.ndev)))[:-1]
        got = snap['perm'].astype(np.int64) + (off[snap['slot']] if snap['slot'].size else 0)
        assert np.array_equal(got, want), len(self.snaps)
        assert np.array_equal(snap['fkeys'], keys[want].astype(np.uint32)), len(self.snaps)
        fs = snap['fine_start']
        assert np.array_equal(fs, np.searchsorted(keys[want], np.arange(fs.size), side='left').astype(np.uint32)), len(self.snaps)
        assert np.array_equal(snap['cell_start'], fs[::8]), len(self.snaps)
        print('update %d: lagged %d placed/overflow predicted %s, counters %d %d' % (
            len(self.snaps), lagged, self.model.log[-1], self.count('n_placed'), self.count('n_place_overflow')))
        assert self.count('n_placed') == self.model.n_placed, (len(self.snaps), self.model.log)
        assert self.count('n_place_overflow') == self.model.n_overflow, (len(self.snaps), self.model.log)
        self.snaps.append(snap)

    def close(self):
        self.ctx.close()
        return self.snaps, self.model.log


def both(make, script, opts=()):
    """the script with sort_place 1 and 0 on the same inputs: the same tables after every update; returns the log
    [(placed, overflow) per update] of the placing run"""
    res = {}
    for place in (1, 0):
        run = Run(make(), place, opts)
        try:
            script(run)
        finally:
            res[place] = run.close()
    (s1, log1), (s0, log0) = res[1], res[0]
    assert len(s1) == len(s0) and not any(p for p, _ in log0)
    for k, (a, b) in enumerate(zip(s1, s0)):
        for name in a:
            assert np.array_equal(a[name], b[name]), (k, name)
    return log1


@pytest.mark.parametrize('n', [1, 63, 64, 65, 257, 1025, 4097])
def test_static_particles_place_from_the_second_update_on_without_overflow(n):
    def script(run):
        for _ in range(3):
            run.update()
    log = both(lambda: [ordered_cloud(n, n, anchors=False)], script)
    assert log == [(False, 0)] + [(True, 0)] * 3


@pytest.mark.parametrize('amp', [0.02, 0.002], ids=['tenth-of-a-cell', 'hundredth-of-a-cell'])
def test_a_few_bucket_crossings_go_through_the_overflow_list(amp):
    """five updates with motion in between.  A tenth of a cell sends some hundred of the 4097 pairs through the list: more
    than n / 256, so every other update takes the four launches; a hundredth keeps the list under that and every update
    places, on a table that is itself the product of a placed update with overflow."""
    counts = []

    def script(run):
        for step in range(5):
            jiggle(run.arrays[0], 40 + step, amp)
            run.update()
            counts.append(np.bincount(read_table(run.ctx, T_FKEYS, np.uint32) >> LBITS, minlength=32))
    log = both(lambda: [ordered_cloud(4097, 7)], script)
    placed = [k for k, (p, o) in enumerate(log) if p]
    assert all(0 < log[k][1] < 4097 // 8 for k in placed), log                      # overflow: there, and small
    d = counts[1] - counts[0]
    assert (d > 0).any() and (d < 0).any()                                          # some buckets grew, some shrank
    if amp == 0.002:
        assert [p for p, _ in log] == [False] + [True] * 5, log
    else:
        assert [p for p, _ in log] == [False, True, False, True, False, True], log


def test_collapse_into_one_cell_overflows_massively_and_the_next_update_takes_four_launches():
    """all particles but the anchors move into one cell: its bucket receives 4095 pairs, more than the 3840-pair stage
    (the global-memory unit sorts it), nearly all of them through the list.  The host sees the count with the bounds, so
    the update after that one does not place; the one after it does again."""
    def script(run):
        pa = run.arrays[0]
        run.update()
        rng = np.random.default_rng(3)
        target = 0.5 + 0.09 * rng.random((pa.x.size, 3))
        d = target - np.stack([pa.x, pa.y, pa.z], axis=1)
        d[:2] = 0.0
        shift(pa, d)
        for _ in range(4):
            run.update()
    log = both(lambda: [ordered_cloud(4097, 8)], script)
    assert [p for p, _ in log] == [False, True, True, False, True, True], log
    assert log[2][1] > 3500 and log[4][1] == 0 and log[5][1] == 0, log


def test_expansion_from_one_bucket_to_the_whole_box():
    """the reverse: nearly every pair of the update after the expansion goes through the list"""
    spread = ordered_cloud(4097, 9)

    def make():
        rng = np.random.default_rng(4)
        pa = ordered_cloud(4097, 9)
        for f in 'xyz':
            getattr(pa, f)[2:] = 0.5 + 0.09 * rng.random(4095)
        return [pa]

    def script(run):
        pa = run.arrays[0]
        run.update()
        d = np.stack([spread.x, spread.y, spread.z], axis=1) - np.stack([pa.x, pa.y, pa.z], axis=1)
        d[:2] = 0.0
        shift(pa, d)
        for _ in range(3):
            run.update()
    log = both(make, script)
    assert [p for p, _ in log] == [False, True, True, False, True], log
    assert log[2][1] > 3500, log


def test_ineligible_updates_take_the_four_launches_and_the_next_eligible_one_places_again():
    from pysph_amd import device as dev

    def script(run):
        pa, ctx = run.arrays[0], run.ctx
        placed = lambda: [p for p, _ in run.model.log]
        run.update()
        # one particle leaves the box: the update after the move still bins on the old grid; the next one has a new grid
        d = np.zeros((pa.x.size, 3)); d[1, 0] = 0.5
        shift(pa, d)
        run.update(); run.update(); run.update()
        if run.model.place:
            assert placed()[-4:] == [True, True, False, True], run.model.log
        # n changes
        n = run.ndev[0] - 5
        pa.gpu.resize(n)                 # (sph_array_resize; the host array follows)
        run.ndev[0] = n
        run.update(); run.update()
        if run.model.place:
            assert placed()[-2:] == [False, True], run.model.log
        # another split of the key
        ctx.set_option('sort_lbits', 10); run.lbits = 10
        run.update(); run.update()
        ctx.set_option('sort_lbits', LBITS); run.lbits = LBITS
        run.update(); run.update()
        if run.model.place:
            assert placed()[-4:] == [False, True, False, True], run.model.log
        # sph_nnps_minmax between two updates uses the sort's work areas
        mm = (C.c_double * 8)()
        ids = (C.c_int * 1)(pa.gpu.array_id)
        dev._check(ctx.lib.sph_nnps_minmax(ctx._h, 1, ids, mm))
        run.model.forget()
        run.update(); run.update()
        if run.model.place:
            assert placed()[-2:] == [False, True], run.model.log
        # an update that looks at the particles first
        ctx.set_option('async_update', 0)
        run.update()
        ctx.set_option('async_update', 1)
        run.update(); run.update()
        if run.model.place:
            assert placed()[-3:] == [False, False, True] or placed()[-3:] == [False, True, True], run.model.log
    both(lambda: [ordered_cloud(4097, 10)], script)


def test_the_traversal_through_the_previous_order_never_places():
    """a shuffled array with via_unordered 1: from the third update on (the count of atomic groups travels with the bounds
    of the second, which still places) the key pass visits it through the previous cell order, which the placed pass does
    not do; with the option off again the next update places on the table the last four-launch update left"""
    def make():
        pa = ordered_cloud(4097, 11)
        order = np.random.default_rng(5).permutation(4097)
        return [get_particle_array(name='a', x=pa.x[order], y=pa.y[order], z=pa.z[order], h=H * np.ones(4097), m=np.ones(4097))]

    def script(run):
        run.update()
        run.update(blocked=True); run.update(blocked=True)
        run.ctx.set_option('via_unordered', 0)
        run.update(); run.update()
    log = both(make, script, opts=(('via_unordered', 1),))
    assert [p for p, _ in log] == [False, True, False, False, True, True], log


@pytest.mark.parametrize('n,amp', [(63, 0.0), (1025, 0.0), (4097, 0.0), (4097, 0.02), (4097, 0.002)])
def test_merged_order_of_three_arrays_one_empty(n, amp):
    def make():
        return [ordered_cloud(n, 12, 'fluid'), get_particle_array(name='none', x=np.zeros(0)),
                ordered_cloud(max(n // 4, 1), 13, 'solid', anchors=False)]

    def script(run):
        for step in range(5 if amp else 3):
            if amp:
                jiggle(run.arrays[0], 60 + step, amp)
                jiggle(run.arrays[2], 70 + step, amp, rest=0)
            run.update()
    log = both(make, script, opts=(('merge_arrays', 1),))
    if amp == 0.0:
        assert log == [(False, 0)] + [(True, 0)] * 3
    else:
        assert any(p and o > 0 for p, o in log), log


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def test_whole_step_is_bit_identical_with_and_without_placing():
    """TaitEOS + WCSPH on a 513-point jittered lattice with trailing ghosts, three lagged updates with motion of the interior
    points in between (the points that hold the bounds rest, so the grid stays and the updates place)"""
    from pysph_amd import kernels as K
    from pysph_amd.particle_array import get_particle_array_wcsph
    from test_hip_parity import cube_equations, make_eval
    OUT = ('arho', 'au', 'av', 'aw', 'ax', 'ay', 'az', 'p', 'cs')
    n, dx = 513, 1.0 / 16
    res = {}
    for place in (1, 0):
        rng = np.random.default_rng(17)
        g = np.arange(9) * dx
        c = np.array([a.ravel() for a in np.meshgrid(g, g, g, indexing='ij')]).T[:n].copy()
        inner = np.all((c > 0.5 * dx) & (c < c.max(axis=0) - 0.5 * dx), axis=1)
        c += 0.1 * dx * rng.uniform(-1, 1, c.shape)
        pa = get_particle_array_wcsph(name='fluid', x=c[:, 0].copy(), y=c[:, 1].copy(), z=c[:, 2].copy(), h=1.3 * dx * np.ones(n),
                                      m=1000.0 * dx ** 3 * np.ones(n), rho=1000.0 * (1 + 0.02 * rng.uniform(-1, 1, n)),
                                      u=rng.uniform(-1, 1, n), v=rng.uniform(-1, 1, n), w=rng.uniform(-1, 1, n))
        pa.set_num_real_particles(n - n // 8)
        a_eval, nnps, ctx = make_eval([pa], cube_equations(dx), K.WendlandQuintic(dim=3), 3, 6, sync='manual')
        try:
            ctx.set_option('sort_lbits', LBITS); ctx.set_option('sort_place', place); ctx.set_option('via_unordered', 0)
            ctx.timer_enable(True)
            pa.gpu.push()
            nnps.sync = False
            got = []
            for rep in range(5):                 # (the first two look at the pushed particles: positions, then masses)
                if rep:
                    d = 0.1 * dx * (np.random.default_rng(80 + rep).random((n, 3)) - 0.5)
                    d[~inner] = 0.0
                    shift(pa, d)
                nnps.update()
                a_eval.compute(0.0, 1e-5)
                a_eval.c_acceleration_eval.pull_outputs()
                pa.gpu.pull('p', 'cs')
                got.append({k: np.array(pa.properties[k]) for k in OUT})
            res[place] = (got, ctx.timer_get('n_placed')[1], ctx.timer_get('n_async')[1])
        finally:
            ctx.close()
    (on, placed_on, async_on), (off, placed_off, async_off) = res[1], res[0]
    print('whole step: n_async %d, n_placed %d' % (async_on, placed_on))
    assert async_on == async_off == 3 and placed_off == 0
    assert placed_on == async_on                                     # every lagged update found the table of the one before
    for rep, (a, b) in enumerate(zip(on, off)):
        for k in OUT:
            same = _bits(a[k]) == _bits(b[k])
            assert same.all(), (rep, k, int((~same).sum()))


def test_lagged_bounds_cross_the_mailbox_exactly():
    """after each of ten lagged updates with moving bounds the reported grid is the one a context that looks at the
    particles reports: the bounds are the payload the sequence number vouches for"""
    from pysph_amd import device as dev
    from pysph_amd.nnps import HipNNPS
    from test_particle_sort import _moved
    pa = cloud(30000, 5, 'fluid', h=0.03)
    ctx = dev.HipContext(0)
    ctx.timer_enable(True)
    dev.attach(pa, ctx).push()
    nn = HipNNPS(3, [pa], radius_scale=2.0, ctx=ctx, sync=False)
    for step in range(10):
        _moved(pa, 200 + step, 0.02, on_device=True)
        nn.update()
        fresh_ctx = dev.HipContext(0)
        copy = get_particle_array(name='fluid', x=pa.x.copy(), y=pa.y.copy(), z=pa.z.copy(), h=pa.h.copy(), m=pa.m.copy())
        fresh = HipNNPS(3, [copy], radius_scale=2.0, ctx=fresh_ctx)
        assert nn.cell_size == fresh.cell_size and nn.n_cells == fresh.n_cells, step
        assert np.array_equal(nn.xmin, fresh.xmin) and np.array_equal(nn.xmax, fresh.xmax), step
        assert np.array_equal(nn.ncells_per_dim, fresh.ncells_per_dim), step
        fresh_ctx.close()
    assert ctx.timer_get('n_async')[1] == 10
    ctx.close()
