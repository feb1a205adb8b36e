"""The halo / migration primitives at their edges, device and test double against ONE statement of the rule.

Every multi-rank test of this project (tests/test_parallel_gloo.py, tests/test_eight_ranks_gloo.py) runs ``SlabHalo`` /
``SlabDecomposition`` on the numpy doubles ``NumpyHaloOps`` / ``NumpyDirectHaloOps`` / ``NumpyPaddedHaloOps``; the product
runs ``pysph_amd.parallel.DeviceHaloOps`` on the kernels of ``pysph_amd/csrc/sph_halo.hip``.  Here each scenario has one
plain-numpy expectation (the ``rule_*`` functions below, written from the protocol, not from either implementation) and
two legs that are driven through the same method calls:

* ``numpy``  -- the doubles imported from tests/test_parallel_gloo.py (runs anywhere);
* ``device`` -- ``DeviceHaloOps`` on a ``HipContext`` (``@pytest.mark.gpu``); where the wrapper hides an argument
  (``upto``, ``sph_halo_pack_mirror``, ``sph_halo_image``) the C entry points are called directly.

The protocol:

* selection: ``x < lo`` for the low face, ``x >= hi`` for the high face, over the real rows (or the first ``upto`` rows);
* message rows in ascending particle index, laid out ``[nprops][cap]`` with ONE header double behind them: the row
  count, + 0.5 when a selected row breaks the sender's promise, negated when the count exceeds ``cap``;
* a padding row has x = y = z = 1e18 and 0 elsewhere; a promised h / m that did not travel is written into ALL appended rows;
* flag bit 0: an incomplete message (negative header), bit 1: a ghost row differs from the promise at the receiver.

Every operation is a copy, one fp64 add or ``v + 2.0 * (plane - v)`` (exact under contraction: 2 * d is exact), so
every comparison is ``np.array_equal``.  The sizes are the smallest at which a path changes: 64 / 256 (wavefront, block),
524 288 / 524 289 (chunk length ``q256`` 1 -> 2 of ``sph_halo_select_pack_promised``), 4 194 304 + 257 (``q256`` = 9: the
trips q >= 8 of ``k_halo_pack_direct`` read the coordinate directly), 16 384 / 16 385 and 65 536 / 65 537 (items per
trip, one launch -> three, of the prefix sums behind ``sph_halo_remove_selected``), ``gone * 4 == n`` / ``n - 1`` (its two
algorithms).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_parallel_gloo import NumpyDirectHaloOps, NumpyHaloOps, NumpyPaddedHaloOps  # noqa: E402

from pysph_amd.particle_array import ParticleArray, get_particle_array_wcsph  # noqa: E402

COLS = ('x', 'y', 'z', 'u', 'rho', 'h', 'm')        # what lives on the device / travels in a ghost message
NO_HM = ('x', 'y', 'z', 'u', 'rho')                 # ... when h and m are promised and do not travel
H0, M0 = 0.01, 1.5
LO, HI = 0.25, 0.75
PERIOD = 3.0
PARKED = 1e18
NAN = float('nan')


# ---------------------------------------------------------------------------------------------------------------------
# the rule, in plain numpy
# ---------------------------------------------------------------------------------------------------------------------
def rule_select(x, n_real, lo, hi, upto=0):
    """index lists of the two faces, ascending (a NaN compares false both times)"""
    m = min(upto, x.size) if upto else n_real
    v = x[:m]
    with np.errstate(invalid='ignore'):
        return np.nonzero(v < lo)[0], np.nonzero(v >= hi)[0]


def rule_rows(cols, idx, names, shift):
    """the packed rows of the listed particles: a copy, the axis coordinate (x) + shift"""
    return dict((p, cols[p][idx] + shift if p == 'x' else cols[p][idx].copy()) for p in names)


def rule_message(cols, idx, names, cap, shift, broken=False, prefill=-7.0):
    """the fixed-capacity message of one face, in a buffer that held `prefill` everywhere"""
    msg = np.full(len(names) * cap + 1, prefill)
    fit = min(idx.size, cap)
    rows = rule_rows(cols, idx[:fit], names, shift)
    for k, p in enumerate(names):
        msg[k * cap:k * cap + fit] = rows[p]
    hdr = idx.size + (0.5 if broken else 0.0)
    msg[-1] = hdr if idx.size <= cap else -hdr
    return msg


def rule_padded(msg, names, cap, h_promise=NAN, m_promise=NAN):
    """(appended columns, flag bits) of one fixed-capacity message: |header| rows (at most cap) are ghosts, the rest
    padding; bit 0: negative header, bit 1: a GHOST row whose travelling h / m differs from the promise"""
    hdr = msg[len(names) * cap]
    count = int(min(np.floor(abs(hdr)), cap))
    flag = 1 if hdr < 0 else 0
    out = {}
    for k, p in enumerate(names):
        col = np.full(cap, PARKED if p in 'xyz' else 0.0)
        col[:count] = msg[k * cap:k * cap + count]
        out[p] = col
        for q, v in (('h', h_promise), ('m', m_promise)):
            if p == q and v == v and np.any(col[:count] != v):
                flag |= 2
    for q, v in (('h', h_promise), ('m', m_promise)):
        if q not in names and v == v:           # promised and did not travel: written into ALL rows
            out[q] = np.full(cap, v)
    return out, flag


def lattice(n):
    """multiples of 1/16 in [0, 1): exact, every value in every 16 consecutive rows"""
    return ((np.arange(n) * 7) % 16) / 16.0


def spread(n, count):
    """`count` distinct ascending indices below n, the first of them 0"""
    assert 0 <= count <= n
    return (np.arange(count, dtype=np.int64) * n) // max(count, 1)


def particles(x, n_real=None, h=H0, m=M0, lean=False):
    """rho carries the row's original index, u = 2 id, y = 1000 + id, z = -id: a moved row is identifiable"""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    ids = np.arange(n, dtype=np.float64)
    if lean:        # the one 4 M-row case: the coordinate and one payload column
        pa = ParticleArray(name='fluid', x=x.copy(), rho=ids)
    else:
        pa = get_particle_array_wcsph(name='fluid', x=x.copy(), y=1000.0 + ids, z=-ids, u=2.0 * ids, rho=ids,
                                      h=h * np.ones(n), m=m * np.ones(n))
    if n_real is not None:
        pa.set_num_real_particles(n_real)
        pa.tag[n_real:] = 1
    return pa


# ---------------------------------------------------------------------------------------------------------------------
# the two legs
# ---------------------------------------------------------------------------------------------------------------------
class NumpyLeg(object):
    device = False

    def __init__(self, pa, props=COLS, fill_holes=1):
        self.pa = pa
        self.ops = NumpyPaddedHaloOps(pa, 0, props)
        assert isinstance(self.ops, NumpyDirectHaloOps) and isinstance(self.ops, NumpyHaloOps)

    def tensor(self, values):
        return torch.from_numpy(np.array(values, dtype=np.float64))

    def host(self, t):
        return t.numpy().copy()

    def sizes(self):
        return self.pa.get_number_of_particles(), self.pa.get_number_of_particles(True)

    def col(self, name):
        return self.pa.properties[name][:self.pa.get_number_of_particles()].copy()

    def write(self, name, values):
        self.pa.properties[name][:] = values

    def all_names(self):
        return list(self.ops.all_props())

    def flags(self, n):
        return [int(v) for v in self.ops.flag_words(n)[:n]]

    def append_faces(self, bufs, caps, hp, mp, slot):
        flags = self.ops.flag_words(slot + 1)
        for b, c in zip(bufs, caps):            # the order two calls give: lo face first
            if b is not None:
                self.ops.append_padded(b, c, hp, mp, flags, slot)

    def close(self):
        pass


class DeviceLeg(object):
    device = True

    def __init__(self, pa, props=COLS, fill_holes=1):
        from pysph_amd import device as dev
        from pysph_amd.parallel import DeviceHaloOps
        self.dev = dev
        self.pa = pa
        pa.properties.pop('gid', None)          # (host metadata: the device holds the columns of `props` only)
        # torch fills the message buffers, the library reads and writes them: both on ONE stream
        self.stream = torch.cuda.Stream()
        torch.cuda.set_stream(self.stream)
        self.ctx = dev.HipContext(0, self.stream.cuda_stream)
        try:
            self.ctx.set_option('fill_holes', fill_holes)
            self.ops = DeviceHaloOps(pa, self.ctx, props, 0)
            self.ops.gpu.push(*[p for p in COLS if p in pa.properties])
        except Exception:
            self.close()
            raise
        self.lib, self.h, self.id = self.ctx.lib, self.ctx._h, self.ops.id

    def tensor(self, values):
        return torch.tensor(np.array(values, dtype=np.float64), dtype=torch.float64, device='cuda')

    def host(self, t):
        return t.cpu().numpy()

    def sizes(self):
        return self.ops.gpu.get_number_of_particles(), self.ops.gpu.get_number_of_particles(True)

    def col(self, name):
        out = np.empty(self.sizes()[0])
        if out.size:
            self.ops.gpu.pull_into(name, out)
        return out

    def write(self, name, values):
        self.pa.properties[name][:] = values
        self.ops.gpu.push(name)

    def all_names(self):
        by_id = dict((self.dev.prop_id(p), p) for p in self.pa.properties if self.dev.prop_id(p) >= 0)
        return [by_id[i] for i in self.ops.all_props()]

    def flags(self, n):
        return [int(v) for v in self.ops.flag_words(n)[:n].cpu().tolist()]

    def append_faces(self, bufs, caps, hp, mp, slot):
        self.ops.append_padded_faces(bufs, caps, hp, mp, self.ops.flag_words(slot + 1), slot)

    def props_c(self, names):
        return (C.c_int * len(names))(*[self.dev.prop_id(p) for p in names])

    def h_known(self):
        lo, hi = C.c_double(), C.c_double()
        known = self.lib.sph_array_h_known(self.h, self.id, C.byref(lo), C.byref(hi))
        return (known, lo.value, hi.value) if known else (0, None, None)

    def look_at_h(self):
        """a reduction over the array looks at h: the library knows its range from here on"""
        out = (C.c_double * 8)()
        self.dev._check(self.lib.sph_nnps_minmax(self.h, 1, (C.c_int * 1)(self.id), out))

    def close(self):
        if getattr(self, 'ctx', None) is not None:
            self.ctx.close()
            self.ctx = None
        torch.cuda.set_stream(torch.cuda.default_stream())


LEGS = {'numpy': NumpyLeg, 'device': DeviceLeg}


@pytest.fixture
def make_leg():
    """factory of legs; every context a test opened is closed, whatever the test's outcome"""
    made = []

    def make(kind, pa, **kw):
        made.append(LEGS[kind](pa, **kw))
        return made[-1]
    yield make
    for L in made:
        L.close()


@pytest.fixture(params=['numpy', pytest.param('device', marks=pytest.mark.gpu)])
def leg(request, make_leg):
    return lambda pa, **kw: make_leg(request.param, pa, **kw)


@pytest.fixture
def device_leg(make_leg):
    return lambda pa, **kw: make_leg('device', pa, **kw)


def snapshot(pa):
    return dict((p, pa.properties[p].copy()) for p in pa.properties if pa.properties[p].dtype == np.float64)


def rows_of(L, buf, names, count, stride=None):
    stride = count if stride is None else stride
    a = L.host(buf)
    return dict((p, a[k * stride:k * stride + count]) for k, p in enumerate(names))


def assert_rows(got, want, what):
    assert sorted(got) == sorted(want), what
    for p in want:
        assert np.array_equal(got[p], want[p]), (what, p)


# ---------------------------------------------------------------------------------------------------------------------
# 1. list-based select / pack / pack_all / append
# ---------------------------------------------------------------------------------------------------------------------
def cuts(n):
    """(name, x, lo, hi) of the selection scenarios of one size"""
    x = lattice(n)
    out = [('none', x, -1.0, 2.0), ('all-low', x, 2.0, 3.0), ('all-high', x, -1.0, -0.5), ('both', x, LO, HI),
           ('overlap', x, HI, LO)]
    if n:
        xl, xh, xn = x.copy(), x.copy(), x.copy()
        xl[0] = LO          # equal to lo: NOT selected
        xh[-1] = HI         # equal to hi: selected
        xn[n // 2] = NAN    # nobody's
        out += [('edge-lo', xl, LO, HI), ('edge-hi', xh, LO, HI), ('nan', xn, LO, HI)]
    return out


@pytest.mark.parametrize('n', [0, 1, 63, 64, 65, 255, 256, 257, 513])
def test_select_pack_and_pack_all_follow_the_rule(leg, n):
    """`select` counts, `pack` and `pack_all` rows of both faces for every cut: nothing / everything selected, a value
    equal to lo (not selected) and one equal to hi (selected), lo > hi (rows in both lists), a NaN (in neither)"""
    L = leg(particles(lattice(n)))
    for name, x, lo, hi in cuts(n):
        L.write('x', x)
        cols = snapshot(L.pa)
        want = rule_select(x, n, lo, hi)
        if name == 'edge-lo':
            assert 0 not in want[0] and 0 not in want[1]
        if name == 'edge-hi':
            assert n - 1 in want[1]
        if name == 'nan':
            assert n // 2 not in want[0] and n // 2 not in want[1]
        if name == 'overlap' and n >= 16:
            assert np.intersect1d(want[0], want[1]).size > 0
        got = L.ops.select(lo, hi)
        assert tuple(got) == (want[0].size, want[1].size), (name, got)
        for s in (0, 1):
            cnt, shift = want[s].size, (PERIOD, -PERIOD)[s]
            buf = L.ops.pack(s, cnt, shift)
            assert_rows(rows_of(L, buf, COLS, cnt), rule_rows(cols, want[s], COLS, shift), (name, s, 'pack'))
            buf, npr = L.ops.pack_all(s, cnt, shift)
            names = L.all_names()
            assert npr == len(names) and names[L.ops.axis_row()] == 'x' and set(COLS) <= set(names)
            assert_rows(rows_of(L, buf, names, cnt), rule_rows(cols, want[s], names, shift), (name, s, 'pack_all'))
        assert L.sizes() == (n, n)


def test_ghost_rows_are_not_selected(leg):
    """rows behind n_real lie where both cuts would take them: `select` looks at the real rows only"""
    n, n_real = 300, 257
    x = lattice(n)
    x[n_real:] = np.where(np.arange(n - n_real) % 2 == 0, -5.0, 5.0)
    L = leg(particles(x, n_real=n_real))
    want = rule_select(x, n_real, LO, HI)
    assert max(want[0].max(), want[1].max()) < n_real
    assert tuple(L.ops.select(LO, HI)) == (want[0].size, want[1].size)
    cols = snapshot(L.pa)
    for s in (0, 1):
        buf = L.ops.pack(s, want[s].size, 0.5)
        assert_rows(rows_of(L, buf, COLS, want[s].size), rule_rows(cols, want[s], COLS, 0.5), s)
    L.ops.drop_ghosts()
    assert L.sizes() == (n_real, n_real)


@pytest.mark.gpu
@pytest.mark.parametrize('upto', [259, 280, 300, 1000])
def test_select_upto_takes_ghost_rows_up_to_that_row(device_leg, upto):
    """sph_halo_select(upto): the first `upto` rows (at most all of them), ghosts included"""
    n, n_real = 300, 257
    x = lattice(n)
    x[n_real:] = np.where(np.arange(n - n_real) % 2 == 0, -5.0, 5.0)
    L = device_leg(particles(x, n_real=n_real))
    cols = snapshot(L.pa)
    want = rule_select(x, n_real, LO, HI, upto=upto)
    assert want[0].max() >= n_real and want[1].max() >= n_real
    counts = (C.c_size_t * 2)()
    L.dev._check(L.lib.sph_halo_select(L.h, L.id, 0, 0, LO, HI, 0.0, upto, counts))
    assert (counts[0], counts[1]) == (want[0].size, want[1].size)
    for s in (0, 1):
        buf = L.ops.pack(s, want[s].size, -0.5)
        assert_rows(rows_of(L, buf, COLS, want[s].size), rule_rows(cols, want[s], COLS, -0.5), s)


@pytest.mark.gpu
@pytest.mark.parametrize('n', [1, 64, 257, 513])
def test_pack_mirror_reflects_the_coordinate_and_negates_the_normal_velocity(device_leg, n):
    """sph_halo_pack_mirror: the axis coordinate is v + 2 (plane - v), u changes sign, the rest is copied"""
    rng = np.random.default_rng(n)
    x = rng.uniform(0.0, 1.0, n)
    x[0] = 0.1
    pa = particles(x)
    pa.u[:] = rng.uniform(-1.0, 1.0, n)
    L = device_leg(pa)
    cols = snapshot(pa)
    want = rule_select(x, n, LO, HI)
    assert tuple(L.ops.select(LO, HI)) == (want[0].size, want[1].size) and want[0].size
    for s, plane in ((0, LO), (1, HI)):
        cnt = want[s].size
        buf = L.ops.new_buffer(cnt)
        L.dev._check(L.lib.sph_halo_pack_mirror(L.h, L.id, s, len(COLS), L.props_c(COLS), 0, plane,
                                                C.c_void_p(buf.data_ptr())))
        expect = rule_rows(cols, want[s], COLS, 0.0)
        v = cols['x'][want[s]]
        expect['x'] = v + 2.0 * (plane - v)
        expect['u'] = -cols['u'][want[s]]
        assert_rows(rows_of(L, buf, COLS, cnt), expect, s)


def message_rows(names, count, stride, base):
    """a [len(names)][stride] buffer whose element (k, i) is base + 1000 k + i; -3 behind row `count`"""
    a = np.full(len(names) * stride, -3.0)
    for k in range(len(names)):
        a[k * stride:k * stride + count] = base + 1000.0 * k + np.arange(count)
    return a


@pytest.mark.parametrize('n0', [0, 65])
def test_append_reads_strided_rows_and_a_count_of_zero_is_a_no_op(leg, n0):
    """`append`: `count` rows of a message with `stride` >= count become ghosts behind the rows present"""
    L = leg(particles(lattice(n0)))
    before = snapshot(L.pa)
    count, stride = 70, 100
    msg = message_rows(COLS, count, stride, 5.0)
    L.ops.append(L.tensor(msg), count, stride)
    assert L.sizes() == (n0 + count, n0)
    for k, p in enumerate(COLS):
        assert np.array_equal(L.col(p), np.concatenate([before[p], msg[k * stride:k * stride + count]])), p
    L.ops.append(L.tensor(msg), 0, stride)
    L.ops.append(L.tensor(msg), 0)
    assert L.sizes() == (n0 + count, n0)
    msg2 = message_rows(COLS, 5, 5, 70000.0)
    L.ops.append(L.tensor(msg2), 5)             # stride defaults to the count
    assert L.sizes() == (n0 + count + 5, n0)
    for k, p in enumerate(COLS):
        assert np.array_equal(L.col(p)[n0 + count:], msg2[k * 5:k * 5 + 5]), p
        assert np.array_equal(L.col(p)[:n0], before[p]), p


def test_append_under_a_promise_fills_the_new_rows_only(leg):
    """h and m promised and not sent: the appended rows get the promised values, the rows present keep theirs"""
    n0, count, stride = 65, 33, 64
    L = leg(particles(lattice(n0), h=2.0 * H0, m=3.0 * M0))
    L.ops.set_promise(H0, M0, send=False)
    assert L.ops.nprops == len(NO_HM)
    msg = message_rows(NO_HM, count, stride, 9.0)
    L.ops.append(L.tensor(msg), count, stride)
    assert L.sizes() == (n0 + count, n0)
    for k, p in enumerate(NO_HM):
        assert np.array_equal(L.col(p)[n0:], msg[k * stride:k * stride + count]), p
    assert np.array_equal(L.col('h'), np.concatenate([np.full(n0, 2.0 * H0), np.full(count, H0)]))
    assert np.array_equal(L.col('m'), np.concatenate([np.full(n0, 3.0 * M0), np.full(count, M0)]))


@pytest.mark.gpu
def test_argument_errors_are_errors_not_overruns(device_leg):
    """stride < count, a property without device storage, a removal with ghosts present, an image of a selection
    made on more rows than the array has now: all refused before any launch"""
    n = 257
    L = device_leg(particles(lattice(n)))
    dev, lib = L.dev, L.lib
    buf = L.tensor(np.zeros(len(COLS) * 16))
    with pytest.raises(dev.SphError):
        L.ops.append(buf, 10, 5)
    assert L.sizes() == (n, n)
    assert min(L.ops.select(LO, HI)) > 0
    no_store = ('x', 'w')                       # w was never pushed
    out = L.ops.new_buffer(n, 2)
    with pytest.raises(dev.SphError):
        dev._check(lib.sph_halo_pack(L.h, L.id, 0, 2, L.props_c(no_store), 0, 0.0, C.c_void_p(out.data_ptr())))
    with pytest.raises(dev.SphError):
        dev._check(lib.sph_halo_pack_mirror(L.h, L.id, 0, 2, L.props_c(no_store), 0, 0.0, C.c_void_p(out.data_ptr())))
    cnt = C.c_size_t()
    with pytest.raises(dev.SphError):
        dev._check(lib.sph_halo_image(L.h, L.id, 0, 2, L.props_c(no_store), 0, 0, PERIOD, C.byref(cnt)))
    assert L.sizes() == (n, n)
    # ghosts present: no removal
    L.ops.append(L.tensor(message_rows(COLS, 3, 3, 1.0)), 3)
    assert L.sizes() == (n + 3, n)
    with pytest.raises(dev.SphError):
        L.ops.remove_selected()
    assert L.sizes() == (n + 3, n)
    # the array shrank below the rows the selection was made on: its lists are stale
    dev._check(lib.sph_array_resize(L.h, L.id, n - 100, n - 100))
    with pytest.raises(dev.SphError):
        dev._check(lib.sph_halo_image(L.h, L.id, 0, len(COLS), L.props_c(COLS), 0, 0, PERIOD, C.byref(cnt)))
    with pytest.raises(dev.SphError):
        L.ops.remove_selected()
    assert L.sizes() == (n - 100, n - 100)


# ---------------------------------------------------------------------------------------------------------------------
# 2. select_pack (sph_halo_select_pack_promised)
# ---------------------------------------------------------------------------------------------------------------------
def faces(n, c_lo, c_hi):
    """x with exactly c_lo rows below LO (even rows, row 0 among them) and c_hi rows at or above HI (odd rows, the last
    odd row among them), every other row strictly between the cuts; the values differ from row to row"""
    x = 0.375 + 0.25 * lattice(n)                           # [0.375, 0.625)
    even, odd = (n + 1) // 2, n // 2
    lo_idx = 2 * spread(even, c_lo)
    if c_lo >= 2:
        lo_idx[-1] = 2 * (even - 1)                         # ... and the last even row
    hi_idx = 2 * (odd - 1 - spread(odd, c_hi)[::-1]) + 1
    x[lo_idx] = 0.125 * lattice(n)[lo_idx]                  # [0, 0.125)
    x[hi_idx] = HI + 0.125 * lattice(n)[hi_idx]             # [0.75, 0.875)
    if c_hi:
        x[hi_idx[0]] = HI                                   # equal to the cut: selected
    free = np.setdiff1d(np.arange(min(n, 8)), np.concatenate([lo_idx, hi_idx]))
    if free.size:
        x[free[0]] = LO                                     # equal to the cut: not selected
    return x, lo_idx, hi_idx


def face_counts(n):
    """counts one above a multiple of 64 where the size allows"""
    evens, odds = (n + 1) // 2, n // 2
    c_lo = max(c for c in (0, 1, 65, 129, 6401) if c <= evens)
    c_hi = max(c for c in (0, 1, 65, 193) if c <= odds)
    return c_lo, c_hi


def run_select_pack(L, names, caps, open_faces=(), shifts=(PERIOD, -PERIOD)):
    bufs = [None if s in open_faces else L.tensor(np.full(len(names) * caps[s] + 1, -7.0)) for s in (0, 1)]
    L.ops.select_pack(LO, HI, shifts, caps, bufs)
    return [None if b is None else L.host(b) for b in bufs]


def check_select_pack(L, cols, names, want, scenarios, broken=(False, False)):
    for what, caps, open_faces in scenarios:
        got = run_select_pack(L, names, caps, open_faces)
        for s in (0, 1):
            if s in open_faces:
                assert got[s] is None
                continue
            expect = rule_message(cols, want[s], names, caps[s], (PERIOD, -PERIOD)[s], broken[s])
            assert got[s][-1] == expect[-1], (what, s, got[s][-1], expect[-1])
            assert np.array_equal(got[s], expect), (what, s)


def capacity_scenarios(cnt):
    tight = [max(c - 1, 0) for c in cnt]
    return [('exact', list(cnt), ()), ('one-short', tight, ()), ('zero', [0, 0], ()),
            ('lo-overfull-hi-roomy', [tight[0], cnt[1] + 5], ()), ('lo-roomy-hi-overfull', [cnt[0] + 64, tight[1]], ()),
            ('one-wavefront', [64, 1], ()), ('roomy', [cnt[0] + 37, cnt[1] + 500], ()),
            ('lo-open', list(cnt), (0,)), ('hi-open', tight, (1,)), ('both-open', list(cnt), (0, 1))]


@pytest.mark.parametrize('n', [0, 1, 255, 256, 257, 524288, 524289])
def test_select_pack_messages_at_their_capacities(leg, n):
    """both faces selected and packed into fixed-capacity messages: capacity exactly full, one short, zero, a multiple
    of 64 with the count one above it, open faces; nothing is written behind the rows that fit (-7 prefill)"""
    c_lo, c_hi = face_counts(n)
    x, lo_idx, hi_idx = faces(n, c_lo, c_hi)
    want = rule_select(x, n, LO, HI)
    assert np.array_equal(want[0], lo_idx) and np.array_equal(want[1], hi_idx)
    if n >= 255:
        assert (c_lo - 1) % 64 == 0 and (c_hi - 1) % 64 == 0 and c_lo > 64   # 'one-short' is a multiple of 64
        assert lo_idx[0] == 0 and max(lo_idx[-1], hi_idx[-1]) == n - 1 and HI in x and LO in x
    L = leg(particles(x))
    cols = snapshot(L.pa)
    scenarios = capacity_scenarios((c_lo, c_hi)) if n else [('empty', [3, 2], ()), ('empty-zero', [0, 0], ()),
                                                            ('empty-open', [3, 2], (0,))]
    check_select_pack(L, cols, COLS, want, scenarios)
    if n == 0:
        got = run_select_pack(L, COLS, [3, 2])
        assert [g[-1] for g in got] == [0.0, 0.0] and all(np.all(g[:-1] == -7.0) for g in got)
    if L.device:
        # ... and the list-based path gives the same rows at these sizes (select_pack leaves no lists: select after it)
        direct = run_select_pack(L, COLS, [c_lo, c_hi])
        assert tuple(L.ops.select(LO, HI)) == (c_lo, c_hi)
        for s in (0, 1):
            listed = L.host(L.ops.pack(s, want[s].size, (PERIOD, -PERIOD)[s]))[:len(COLS) * want[s].size]
            assert np.array_equal(direct[s][:-1], listed), s
    assert L.sizes() == (n, n)


def test_select_pack_with_nine_trips_per_chunk(leg):
    """n = 4 194 304 + 257: q256 = 9, the trips q >= 8 of the packing kernel read the coordinate directly; selected
    rows lie in those trips and before them"""
    n = 4194304 + 257
    q256 = -(-n // (256 * 2048))
    assert q256 == 9
    c_lo, c_hi = 6401, 193
    x, lo_idx, hi_idx = faces(n, c_lo, c_hi)
    for idx in (lo_idx, hi_idx):
        trip = (idx % (256 * q256)) // 256
        assert (trip >= 8).any() and (trip < 8).any()
    want = rule_select(x, n, LO, HI)
    assert np.array_equal(want[0], lo_idx) and np.array_equal(want[1], hi_idx)
    names = ('x', 'rho')
    L = leg(particles(x, lean=True), props=names)
    cols = snapshot(L.pa)
    check_select_pack(L, cols, names, want, [('exact', [c_lo, c_hi], ()), ('one-short', [c_lo - 1, c_hi - 1], ()),
                                             ('lo-open-roomy', [c_lo, c_hi + 70], (0,))])
    if L.device:
        direct = run_select_pack(L, names, [c_lo, c_hi])
        assert tuple(L.ops.select(LO, HI)) == (c_lo, c_hi)
        for s in (0, 1):
            listed = L.host(L.ops.pack(s, want[s].size, (PERIOD, -PERIOD)[s]))[:2 * want[s].size]
            assert np.array_equal(direct[s][:-1], listed), s


@pytest.mark.parametrize('n', [1, 257, 524288, 524289])
def test_select_pack_checks_the_promise_on_the_senders_side(leg, n):
    """h and m promised and taken out of the messages (`set_promise(.., send=False)`): a SELECTED row with another
    h / m adds 0.5 to the header of its face and of no other -- wherever the row lies: first chunk, last chunk, a chunk
    that is neither the first nor the one that writes the headers; together with an overfull face -(count + 0.5)"""
    c_lo, c_hi = face_counts(n)
    x, lo_idx, hi_idx = faces(n, c_lo, c_hi)
    want = (lo_idx, hi_idx)
    L = leg(particles(x))
    L.ops.set_promise(H0, M0, send=False)
    assert L.ops.nprops == len(NO_HM)
    cols = snapshot(L.pa)
    cnt = (c_lo, c_hi)
    tight = [max(c - 1, 0) for c in cnt]
    basic = [('exact', list(cnt), ()), ('one-short', tight, ()), ('roomy', [c_lo + 3, c_hi + 64], ())]
    check_select_pack(L, cols, NO_HM, want, basic)                                  # the promise holds
    h, m = np.full(n, H0), np.full(n, M0)

    def with_rows(prop, rows):
        v = (h if prop == 'h' else m).copy()
        v[np.asarray(rows, dtype=np.int64)] *= 1.0 + 2.0 ** -52     # one ulp away from the promise
        L.write(prop, v)

    chunk = 256 * -(-n // (256 * 2048))
    last = (n - 1) // chunk                         # the chunk whose workgroup writes the headers
    places = sorted(set([int(lo_idx[0]), int(lo_idx[c_lo // 2]), int(lo_idx[-1])]))
    assert places[0] // chunk == 0 and places[-1] // chunk == last
    if n >= 524288:
        assert 0 < places[1] // chunk < last
    for r in places:                                # a low-face row breaks h: the high header stays integral
        with_rows('h', [r])
        check_select_pack(L, cols, NO_HM, want, basic, broken=(True, False))
    with_rows('h', [])
    if n > 1:
        with_rows('m', [int(hi_idx[-1])])           # a high-face row (in the last chunk) breaks m
        check_select_pack(L, cols, NO_HM, want, basic, broken=(False, True))
        with_rows('m', [])
        between = np.setdiff1d(np.arange(n), np.concatenate([lo_idx, hi_idx]))
        with_rows('h', between[[0, between.size // 2, -1]])                         # unselected rows: nothing changes
        check_select_pack(L, cols, NO_HM, want, basic)
        with_rows('h', [int(lo_idx[-1]), int(hi_idx[0])])                           # both faces
        check_select_pack(L, cols, NO_HM, want, basic, broken=(True, True))
        with_rows('h', [])
    check_select_pack(L, cols, NO_HM, want, basic)
    # with h and m IN the messages the sender checks nothing: the receiver does
    L.ops.set_promise(H0, M0, send=True)
    assert L.ops.nprops == len(COLS)
    with_rows('h', [int(lo_idx[0])])
    cols = snapshot(L.pa)
    check_select_pack(L, cols, COLS, want, basic)


# ---------------------------------------------------------------------------------------------------------------------
# 3. append_padded / append_padded_faces
# ---------------------------------------------------------------------------------------------------------------------
def padded_message(names, cap, hdr, base=0.0, h_bad_rows=(), h_pad=None):
    """[len(names)][cap] rows (every row filled: what lies behind the count must not be looked at) + header"""
    msg = np.empty(len(names) * cap + 1)
    for k, p in enumerate(names):
        msg[k * cap:(k + 1) * cap] = base + 100000.0 * (k + 1) + np.arange(cap)
        if p == 'h':
            msg[k * cap:(k + 1) * cap] = H0
            for r in h_bad_rows:
                msg[k * cap + r] = 2.0 * H0
            count = int(min(np.floor(abs(hdr)), cap))
            if h_pad is not None:
                msg[k * cap + count:(k + 1) * cap] = h_pad
        if p == 'm':
            msg[k * cap:(k + 1) * cap] = M0
    msg[-1] = hdr
    return msg


def headers_of(cap):
    return [0.0, float(cap), float(cap - 1), -float(cap + 3), cap // 2 + 0.5, -(cap + 0.5)]


def check_appended(L, before, n_real, parts, names_written):
    """the array is `before` followed by the parts (dicts of appended columns), n_real unchanged"""
    total = sum(next(iter(p.values())).size for p in parts)
    n0 = next(iter(before.values())).size
    assert L.sizes() == (n0 + total, n_real)
    for p in names_written:
        want = np.concatenate([before[p]] + [part[p] for part in parts])
        assert np.array_equal(L.col(p), want), p


@pytest.mark.parametrize('cap', [1, 64, 255, 256, 257])
def test_append_padded_rows_and_flag_words(leg, cap):
    """one message: |header| ghost rows (at most cap), parked padding behind them; bit 0 only for a negative header,
    bit 1 only for a GHOST row with another h than promised (a padding row's h is not looked at, nor is the + 0.5 of
    the sender); the word at the slot given, its neighbours untouched, sticky until `clear_flags`"""
    n0 = 5
    L = leg(particles(lattice(n0)))
    before = dict((p, snapshot(L.pa)[p]) for p in COLS)
    nflags, slot = 3, 1
    L.ops.flag_words(nflags)
    for hdr in headers_of(cap):
        msg = padded_message(COLS, cap, hdr, h_pad=7.0 * H0)
        want, flag = rule_padded(msg, COLS, cap, H0, M0)
        assert flag == (1 if hdr < 0 else 0)
        L.ops.append_padded(L.tensor(msg), cap, H0, M0, L.ops.flag_words(nflags), slot)
        check_appended(L, before, n0, [want], COLS)
        assert L.flags(nflags) == [0, flag, 0], hdr
        L.ops.clear_flags()
        assert L.flags(nflags) == [0, 0, 0]
        L.ops.drop_ghosts()
        assert L.sizes() == (n0, n0)
    # a ghost row with another h: bit 1 -- in the first and in the last ghost row
    count = max(cap - 1, 1)
    for r in sorted(set([0, count - 1])):
        msg = padded_message(COLS, cap, float(count), h_bad_rows=[r])
        want, flag = rule_padded(msg, COLS, cap, H0, M0)
        assert flag == 2
        L.ops.append_padded(L.tensor(msg), cap, H0, M0, L.ops.flag_words(nflags), slot)
        check_appended(L, before, n0, [want], COLS)
        assert L.flags(nflags) == [0, 2, 0]
        # no promise: nothing to break
        L.ops.drop_ghosts()
        L.ops.clear_flags()
        L.ops.append_padded(L.tensor(msg), cap, NAN, NAN, L.ops.flag_words(nflags), slot)
        check_appended(L, before, n0, [want], COLS)
        assert L.flags(nflags) == [0, 0, 0]
        L.ops.drop_ghosts()
    # sticky across two calls, other slots stay
    L.ops.append_padded(L.tensor(padded_message(COLS, cap, -float(cap + 3))), cap, H0, M0, L.ops.flag_words(nflags), 2)
    L.ops.append_padded(L.tensor(padded_message(COLS, cap, float(cap))), cap, H0, M0, L.ops.flag_words(nflags), 2)
    assert L.flags(nflags) == [0, 0, 1]
    L.ops.append_padded(L.tensor(padded_message(COLS, cap, float(cap), h_bad_rows=[cap - 1])), cap, H0, M0,
                        L.ops.flag_words(nflags), 2)
    assert L.flags(nflags) == [0, 0, 3] and L.sizes() == (n0 + 3 * cap, n0)
    L.ops.clear_flags()
    assert L.flags(nflags) == [0, 0, 0]


@pytest.mark.parametrize('cap', [1, 64, 255, 256, 257])
def test_append_padded_fills_a_promise_that_did_not_travel(leg, cap):
    """`set_promise(.., send=False)`: every appended row, padding rows included, carries the promised h and m; the rows
    present keep theirs, n_real stays, bit 1 is never set"""
    n0 = 5
    L = leg(particles(lattice(n0), h=2.0 * H0, m=3.0 * M0))
    L.ops.set_promise(H0, M0, send=False)
    before = dict((p, snapshot(L.pa)[p]) for p in COLS)
    for hdr in headers_of(cap):
        msg = padded_message(NO_HM, cap, hdr)
        want, flag = rule_padded(msg, NO_HM, cap, H0, M0)
        assert np.all(want['h'] == H0) and np.all(want['m'] == M0) and want['h'].size == cap and not flag & 2
        L.ops.append_padded(L.tensor(msg), cap, H0, M0, L.ops.flag_words(2), 0)
        check_appended(L, before, n0, [want], COLS)
        assert L.flags(2) == [flag, 0], hdr
        L.ops.clear_flags()
        L.ops.drop_ghosts()


def two_face_cases():
    out = []
    for caps in ((64, 0), (0, 64), (257, 0), (0, 257), (64, 257), (257, 1), (255, 256), (1, 64)):
        for hdrs in (('full', 'full'), ('neg', 'ok'), ('ok', 'neg'), ('zero', 'ok'), ('ok', 'zero'), ('half', 'neg')):
            out.append((caps, hdrs))
    return out


def header_named(kind, cap):
    if cap == 0:
        return 0.0
    return {'full': float(cap), 'neg': -float(cap + 3), 'ok': float(cap - 1), 'zero': 0.0,
            'half': cap // 2 + 0.5}[kind]


@pytest.mark.parametrize('send', [True, False], ids=['hm-travel', 'hm-filled'])
def test_append_padded_faces_two_messages_in_one_call(leg, send):
    """both faces' messages in one call: face 0's `cap` rows, then face 1's; (cap, 0), (0, cap) and unequal capacities;
    one face negative and the other not; a header of 0 (all padding); a missing second message"""
    n0 = 3
    names = COLS if send else NO_HM
    L = leg(particles(lattice(n0)))
    L.ops.set_promise(H0, M0, send=send)
    before = dict((p, snapshot(L.pa)[p]) for p in COLS)
    for caps, kinds in two_face_cases():
        hdrs = [header_named(k, c) for k, c in zip(kinds, caps)]
        msgs = [padded_message(names, c, h, base=1e7 * s, h_pad=5.0 * H0) for s, (c, h) in enumerate(zip(caps, hdrs))]
        parts, flag = [], 0
        for msg, c in zip(msgs, caps):
            want, f = rule_padded(msg, names, c, H0, M0)
            if c:
                parts.append(want)
                flag |= f
        assert flag == (1 if min(hdrs) < 0 else 0)
        L.append_faces([L.tensor(m) for m in msgs], list(caps), H0, M0, 1)
        check_appended(L, before, n0, parts, COLS)
        assert L.flags(3) == [0, flag, 0], (caps, kinds)
        L.ops.clear_flags()
        L.ops.drop_ghosts()
    # a ghost of the SECOND face breaks the promise (when h travels); one message only
    cap = 65
    if send:
        msgs = [padded_message(names, cap, float(cap)), padded_message(names, cap, float(cap - 1), base=1e7, h_bad_rows=[cap - 2])]
        parts = [rule_padded(m, names, cap, H0, M0)[0] for m in msgs]
        L.append_faces([L.tensor(m) for m in msgs], [cap, cap], H0, M0, 0)
        check_appended(L, before, n0, parts, COLS)
        assert L.flags(3) == [2, 0, 0]
        L.ops.clear_flags()
        L.ops.drop_ghosts()
    msg = padded_message(names, cap, -float(cap + 1))
    L.append_faces([L.tensor(msg)], [cap], H0, M0, 2)
    check_appended(L, before, n0, [rule_padded(msg, names, cap, H0, M0)[0]], COLS)
    assert L.flags(3) == [0, 0, 1]
    if L.device:
        # the low face missing: sph_halo_append_padded2 takes the second message as the only one
        L.ops.drop_ghosts()
        L.ops.clear_flags()
        L.ops.append_padded_faces([None, L.tensor(msg)], [0, cap], H0, M0, L.ops.flag_words(3), 0)
        check_appended(L, before, n0, [rule_padded(msg, names, cap, H0, M0)[0]], COLS)
        assert L.flags(3) == [1, 0, 0]


@pytest.mark.gpu
@pytest.mark.parametrize('send', [True, False], ids=['hm-travel', 'hm-filled'])
@pytest.mark.parametrize('state', ['empty', 'same-h-known', 'other-h-known', 'h-not-looked-at'])
def test_what_the_library_knows_of_h_after_a_promised_message(device_leg, state, send):
    """sph_halo_append_padded2 (`keep_h` / `empty0`): an EMPTY array that receives a promised message has the promised
    range from there on; an array known to hold the promised h keeps that knowledge; one that holds another h, or
    whose h nobody has looked at, does not"""
    names = COLS if send else NO_HM
    n0 = 0 if state == 'empty' else 65
    L = device_leg(particles(lattice(n0), h=2.0 * H0 if state == 'other-h-known' else H0))
    L.ops.set_promise(H0, M0, send=send)
    if state in ('same-h-known', 'other-h-known'):
        L.look_at_h()
        assert L.h_known() == (1,) + ((H0, H0) if state == 'same-h-known' else (2.0 * H0, 2.0 * H0))
    else:
        assert L.h_known()[0] == 0
    caps = (64, 257)
    msgs = [padded_message(names, c, float(c - 1), base=1e7 * s) for s, c in enumerate(caps)]
    L.append_faces([L.tensor(m) for m in msgs], list(caps), H0, M0, 0)
    assert L.sizes() == (n0 + sum(caps), n0)
    if state in ('empty', 'same-h-known'):
        assert L.h_known() == (1, H0, H0)
    else:
        assert L.h_known()[0] == 0
    assert L.flags(1) == [0]
    hcol = L.col('h')[n0:]
    if send:
        want = np.concatenate([rule_padded(m, names, c, H0, M0)[0]['h'] for m, c in zip(msgs, caps)])
        assert np.array_equal(hcol, want)
    else:
        assert np.all(hcol == H0)


# ---------------------------------------------------------------------------------------------------------------------
# 4. remove_selected and append_real
# ---------------------------------------------------------------------------------------------------------------------
def leaver_cases(n):
    """{name: (low-list leavers, high-list leavers)} by construction"""
    none = np.zeros(0, dtype=np.int64)
    out = {'none': (none, none), 'first': (np.array([0]), none), 'last': (none, np.array([n - 1]))}
    allrows = np.arange(n)
    out['all'] = (allrows[:n // 2], allrows[n // 2:])
    if n >= 16:
        g = n // 8
        tail, head = np.arange(n - g, n), np.arange(g)
        out['tail-only'] = (tail[::2], tail[1::2])          # no kept row in the tail: nothing to move
        out['below-keepn-only'] = (head[::2], head[1::2])   # every tail row kept: the whole tail moves
        out['low-below-high-in-tail'] = (np.arange(0, g // 2), np.arange(n - (g - g // 2), n))
        out['low-in-tail-high-below'] = (np.arange(n - g // 2, n), np.arange(0, g - g // 2))    # holes from the high list only
        out['low-list-only'] = (spread(n, g), none)
        out['high-list-only'] = (none, n - 1 - spread(n, g)[::-1])
        out['mixed'] = (spread(n, g)[::2], spread(n, g)[1::2])
        # the two sides of `gone * 4 < n`
        if n % 4 == 0:
            out['gone*4==n'] = (spread(n, n // 4)[::2], spread(n, n // 4)[1::2])
            out['gone*4==n-4'] = (spread(n, n // 4 - 1)[::2], spread(n, n // 4 - 1)[1::2])
        if n % 4 == 1:
            out['gone*4==n-1'] = (spread(n, n // 4)[::2], spread(n, n // 4)[1::2])
            out['gone*4==n+3'] = (spread(n, n // 4 + 1)[::2], spread(n, n // 4 + 1)[1::2])
    return out


def removal_x(n, low, high):
    x = 0.3 + 0.4 * lattice(n)          # [0.3, 0.7): stays
    x[low] = -1.0 - lattice(n)[low]
    x[high] = 2.0 + lattice(n)[high]
    return x


@pytest.mark.parametrize('n', [1, 2, 257, 4096, 16385, 65537])
@pytest.mark.parametrize('kind', ['numpy', pytest.param('device-fill-holes', marks=pytest.mark.gpu),
                                  pytest.param('device-compact', marks=pytest.mark.gpu)])
def test_remove_selected_keeps_exactly_the_kept_rows(make_leg, kind, n):
    """exactly the kept particles remain and every column still belongs to its id.  In the kept order with
    fill_holes = 0 and on the compaction branch (gone * 4 >= n); on the fill-holes branch every kept row below keepn stays
    where it was.  (The double is stable: always in the kept order.)  A `select` on the shrunk array is right again."""
    fill_holes = 0 if kind == 'device-compact' else 1
    for name, (low, high) in leaver_cases(n).items():
        x = removal_x(n, low, high)
        L = make_leg(kind.split('-')[0], particles(x), fill_holes=fill_holes)
        want = rule_select(x, n, LO, HI)
        assert np.array_equal(want[0], low) and np.array_equal(want[1], high)
        assert tuple(L.ops.select(LO, HI)) == (low.size, high.size), name
        gone = low.size + high.size
        keepn = n - gone
        kept = np.setdiff1d(np.arange(n), np.concatenate([low, high]))
        assert L.ops.remove_selected() == keepn, name
        assert L.sizes() == (keepn, keepn), name
        ids = L.col('rho').astype(np.int64)
        assert np.array_equal(np.sort(ids), kept), name
        assert np.array_equal(L.col('x'), x[ids]) and np.array_equal(L.col('u'), 2.0 * ids), name
        assert np.array_equal(L.col('y'), 1000.0 + ids) and np.array_equal(L.col('z'), -1.0 * ids), name
        assert np.all(L.col('h') == H0) and np.all(L.col('m') == M0), name
        fills = L.device and fill_holes and gone * 4 < n
        if not fills:
            assert np.array_equal(ids, kept), name
        else:
            stay = kept[kept < keepn]
            assert np.array_equal(ids[stay], stay), name
            assert (ids != np.arange(keepn)).sum() == (kept >= keepn).sum(), name   # the holes took the tail's kept rows
        if name == 'tail-only':
            assert np.array_equal(ids, np.arange(keepn))
        # no stale lists or counts: the next selection sees the shrunk array
        xs = x[ids]
        again = rule_select(xs, keepn, 0.45, 0.55)
        assert tuple(L.ops.select(0.45, 0.55)) == (again[0].size, again[1].size), name
        cols = dict(x=xs, y=1000.0 + ids, z=-1.0 * ids, u=2.0 * ids, rho=1.0 * ids, h=np.full(keepn, H0), m=np.full(keepn, M0))
        for s in (0, 1):
            buf = L.ops.pack(s, again[s].size, 0.25)
            assert_rows(rows_of(L, buf, COLS, again[s].size), rule_rows(cols, again[s], COLS, 0.25), (name, s))
        L.close()


def migrants(names, count, h=H0, m=M0, base=0.0):
    """[len(names)][count] rows of arrivals: element (k, i) = base + 1000 (k + 1) + i, h and m as given"""
    a = np.empty(len(names) * count)
    for k, p in enumerate(names):
        a[k * count:(k + 1) * count] = base + 1000.0 * (k + 1) + np.arange(count)
        if p == 'h':
            a[k * count:(k + 1) * count] = h
        if p == 'm':
            a[k * count:(k + 1) * count] = m
    return a


@pytest.mark.parametrize('n', [2, 257, 4096])
def test_append_real_after_a_removal(leg, n):
    """the migrants land behind the survivors and are real; a count of 0 changes nothing"""
    low, high = leaver_cases(n)['mixed' if n >= 16 else 'first']
    x = removal_x(n, low, high)
    L = leg(particles(x))
    L.ops.select(LO, HI)
    left = L.ops.remove_selected()
    names = L.all_names()
    before = dict((p, L.col(p)) for p in names)
    count = 70
    buf = migrants(names, count)
    L.ops.append_real(L.tensor(buf), count)
    assert L.sizes() == (left + count, left + count)
    for k, p in enumerate(names):
        assert np.array_equal(L.col(p), np.concatenate([before[p], buf[k * count:(k + 1) * count]])), p
    L.ops.append_real(L.tensor(buf), 0)
    assert L.sizes() == (left + count, left + count)
    for k, p in enumerate(names):
        assert np.array_equal(L.col(p)[left:], buf[k * count:(k + 1) * count]), p
    # ... and the grown array is selected from as a whole
    xs = L.col('x')
    want = rule_select(xs, left + count, 0.45, 0.55)
    assert tuple(L.ops.select(0.45, 0.55)) == (want[0].size, want[1].size)


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['same-h', 'other-h', 'other-h-last-row', 'empty', 'empty-other-h', 'count-0'])
def test_append_real_under_a_promise(device_leg, case):
    """sph_halo_append_promised: arrivals with the promised h keep what the library knows, an arrival with another h
    sets bit 1 of the word at the slot given; arrivals into an EMPTY array establish the promised range"""
    empty = case.startswith('empty')
    n = 0 if empty else 257
    low, high = (np.zeros(0, dtype=np.int64),) * 2 if empty else leaver_cases(n)['mixed']
    x = removal_x(n, low, high)
    L = device_leg(particles(x))
    L.ops.set_promise(H0, M0)
    if not empty:
        L.look_at_h()
        L.ops.select(LO, HI)
        L.ops.remove_selected()
        assert L.h_known() == (1, H0, H0)
    else:
        assert L.h_known()[0] == 0
    left = L.sizes()[0]
    names = L.all_names()
    assert sorted(names) == sorted(COLS)
    count = 0 if case == 'count-0' else 130
    buf = migrants(names, max(count, 1))
    if 'other-h' in case:
        kh = names.index('h')
        buf[kh * count + (count - 1 if case.endswith('last-row') else 64)] = 3.0 * H0
    flags = L.ops.flag_words(3)
    L.ops.append_real(L.tensor(buf), count, flags, 1)
    assert L.sizes() == (left + count, left + count)
    assert L.flags(3) == [0, 2 if 'other-h' in case else 0, 0]
    assert L.h_known() == (1, H0, H0)       # (a broken promise is the flag word's business: the caller raises)
    for k, p in enumerate(names):
        assert np.array_equal(L.col(p)[left:], buf[k * count:(k + 1) * count]), p


# ---------------------------------------------------------------------------------------------------------------------
# 5. sph_domain_images_padded at its capacities
# ---------------------------------------------------------------------------------------------------------------------
def rule_images(cols, n, p0, p1, p2, shift, caps):
    """periodic images of one axis (x): lo: v - p0 <= p2, hi: p1 - v <= p2, a parked row is nobody's; the low face's
    images move up by `shift`, the high face's down; rows behind the counts are parked"""
    v = cols['x'][:n]
    live = np.abs(v) < 1e17
    lists = (np.nonzero(live & ((v - p0) <= p2))[0], np.nonzero(live & ((p1 - v) <= p2))[0])
    parts, counts = [], []
    for s in (0, 1):
        cap, idx = caps[s], lists[s]
        fit = min(idx.size, cap)
        part = {}
        for p in cols:
            col = np.full(cap, PARKED if p in 'xyz' else 0.0)
            col[:fit] = cols[p][idx[:fit]]
            if p == 'x':
                col[:fit] = cols[p][idx[:fit]] + (shift if s == 0 else -shift)
            part[p] = col
        parts.append(part)
        counts.append(float(idx.size) if idx.size <= cap else -float(idx.size))
    return lists, parts, counts


def image_cases(n):
    """(name, x, width, caps as offsets from the counts, or absolute)"""
    x = lattice(n) + np.arange(n) * 2.0 ** -30          # distinct values in [0, 1)
    out = [('exact', x, 0.125, (0, 0), None), ('one-short', x, 0.125, (-1, -1), None), ('lo-zero', x, 0.125, None, (0, None)),
           ('hi-zero-roomy', x, 0.125, None, (None, 0)), ('roomy', x, 0.125, (70, 3), None),
           ('narrow-box', x, 0.625, (0, 5), None)]       # width > half the box: rows imaged on both faces
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('n', [1, 256, 257, 524289])
def test_domain_images_padded_at_its_capacities(device_leg, n):
    """sph_domain_images_padded against a numpy model of face_rule<true>: count == cap, count == cap + 1 (a negative
    count through sph_domain_counts_queue / _collect), cap = 0 on one face, a box narrower than twice the width (a
    row imaged on both faces), parked rows of an earlier axis (not imaged)"""
    p0, p1 = 0.0, 1.0
    L = device_leg(particles(image_cases(n)[0][1]))
    dev, lib = L.dev, L.lib
    for name, x, width, offs, fixed in image_cases(n):
        n_all = n
        assert L.sizes() == (n, n)
        if name == 'roomy' and n > 1:
            # an earlier axis left images and parked rows behind the real ones: a padded message does the same here
            cap0 = 9
            msg = padded_message(COLS, cap0, 4.0)
            msg[:cap0] = [0.01, 0.99, 0.5, 0.02, 9, 9, 9, 9, 9]          # x of the rows; 4 ghosts, 5 parked
            L.ops.append_padded(L.tensor(msg), cap0, NAN, NAN, L.ops.flag_words(1), 0)
            n_all = n + cap0
        cols = dict((p, L.col(p)) for p in COLS)
        assert cols['x'].size == n_all
        lists, _, _ = rule_images(cols, n_all, p0, p1, width, 1.0, (0, 0))
        cnt = [lists[0].size, lists[1].size]
        if name == 'narrow-box' and n > 16:
            assert np.intersect1d(lists[0], lists[1]).size > 0
        if name == 'roomy' and n > 1:
            assert n in lists[0] and n + 1 in lists[1] and n + 3 in lists[0] and max(lists[0].max(), lists[1].max()) < n + 4
        if fixed is None:
            caps = [max(cnt[s] + offs[s], 0) for s in (0, 1)]
        else:
            caps = [cnt[s] + 2 if fixed[s] is None else fixed[s] for s in (0, 1)]
        _, parts, counts = rule_images(cols, n_all, p0, p1, width, 1.0, caps)
        if name == 'one-short':
            assert [c < 0 for c in counts] == [cnt[0] > 0, cnt[1] > 0]
        dev._check(lib.sph_domain_images_padded(L.h, L.id, 0, p0, p1, width, 1.0, (C.c_size_t * 2)(*caps), len(COLS),
                                                L.props_c(COLS)))
        dev._check(lib.sph_domain_counts_queue(L.h))
        out = (C.c_double * (dev.MAX_ARRAYS * 6))()
        dev._check(lib.sph_domain_counts_collect(L.h, out))
        assert [out[L.id * 6], out[L.id * 6 + 1]] == counts, (name, caps)
        check_appended(L, cols, n, [p for p, c in zip(parts, caps) if c], COLS)
        L.ops.drop_ghosts()


# ---------------------------------------------------------------------------------------------------------------------
# 6. histogram, coord_range, hm_range
# ---------------------------------------------------------------------------------------------------------------------
def rule_histogram(x, n_real, vmin, span, nbins):
    v = x[:n_real]
    v = v[np.abs(v) < 1e17]             # (a NaN and a parked row compare false)
    b = np.floor((v - vmin) * (nbins / span)).astype(np.int64)
    return np.bincount(np.clip(b, 0, nbins - 1), minlength=nbins).astype(np.float64)


@pytest.mark.gpu
@pytest.mark.parametrize('nbins', [1, 8])
@pytest.mark.parametrize('n', [1, 257])
def test_histogram_at_its_edges(device_leg, n, nbins):
    """a value equal to vmin + span lies in the last bin, one below vmin in the first, a parked row and a NaN in none,
    ghosts in none"""
    vmin, span = 0.25, 0.5
    n_ghost = 40
    L = device_leg(particles(0.25 + 0.5 * lattice(n + n_ghost), n_real=n))
    for special in ([vmin + span], [vmin - 0.125], [PARKED], [NAN], [vmin], [vmin + span, vmin - 1.0, PARKED, NAN]):
        x = 0.25 + 0.5 * lattice(n + n_ghost)
        k = min(len(special), n)
        x[n - k:n] = special[:k]
        with np.errstate(invalid='ignore'):
            want = rule_histogram(x, n, vmin, span, nbins)
        if special == [vmin + span]:
            assert want[-1] >= 1
        if special[0] in (PARKED,) or special[0] != special[0]:
            assert want.sum() == n - 1
        L.write('x', x)
        got = L.ops.histogram(vmin, span, nbins)
        assert np.array_equal(got, want), (special, got, want)


@pytest.mark.parametrize('n', [0, 1, 257])
def test_ranges_ignore_ghosts_and_are_empty_for_an_empty_array(leg, n):
    """hm_range / coord_range (device) and hm_range / coords (double): over the real rows only; (inf, -inf) when
    there are none"""
    n_ghost = 33
    x = 0.25 + 0.5 * lattice(n + n_ghost) + np.arange(n + n_ghost) * 2.0 ** -20
    x[n:] = np.where(np.arange(n_ghost) % 2 == 0, -9.0, 9.0)
    pa = particles(x, n_real=n)
    pa.h[:n] = H0 * (1.0 + np.arange(n) / 1024.0)
    pa.m[:n] = M0 * (2.0 - np.arange(n) / 1024.0)
    pa.h[n:] = [100.0 * H0, 0.01 * H0] * 16 + [H0]
    pa.m[n:] = [100.0 * M0, 0.01 * M0] * 16 + [M0]
    h, m = pa.h[:n].copy(), pa.m[:n].copy()
    L = leg(pa)
    inf = float('inf')
    want = [h.min(), h.max(), m.min(), m.max()] if n else [inf, -inf, inf, -inf]
    assert [float(v) for v in L.ops.hm_range()] == want
    assert np.array_equal(L.ops.coords(), x[:n])
    if L.device:
        assert L.ops.coord_range() == ((x[:n].min(), x[:n].max()) if n else (inf, -inf))
    assert L.sizes() == (n + n_ghost, n)
