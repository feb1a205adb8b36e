"""Shared builders for the parity tests (equation sets named like the
reference's schemes)."""
import os

import numpy as np

from pysph_amd import kernels as K
from pysph_amd.equations import Group, SummationDensity
from pysph_amd.scheme import WCSPHScheme, TVFScheme
from pysph_amd.examples import dam_break_3d as db

WC_OUT = ['rho', 'p', 'cs', 'arho', 'au', 'av', 'aw', 'ax', 'ay', 'az',
          'dt_cfl', 'dt_force']
EL_OUT = ['p', 'v00', 'v01', 'v02', 'v10', 'v11', 'v12', 'v20', 'v21', 'v22',
          'r00', 'r01', 'r02', 'r11', 'r12', 'r22', 'arho', 'au', 'av', 'aw',
          'ax', 'ay', 'az', 'as00', 'as01', 'as02', 'as11', 'as12', 'as22']
TVF_OUT = ['rho', 'V', 'p', 'au', 'av', 'aw', 'auhat', 'avhat', 'awhat']


def golden_case(name, g, wall_equations=None):
    """(equations, kernel, dim, output props) matching make_golden.py."""
    if name in ('wcsph_dam_dx0.1', 'wcsph_dam_varh'):
        dx = float(g['meta/dx'])
        s = db.create_scheme(dx)
        return s.get_equations(), K.WendlandQuintic(dim=3), 3, WC_OUT
    if name == 'wcsph_cube_varh':
        dx = float(g['meta/dx'])
        s = WCSPHScheme(['fluid'], [], dim=3, rho0=1000.0, c0=10.0,
                        h0=1.2 * dx, hdx=1.2, gx=0.5, gy=-0.25, gz=-9.81,
                        alpha=1.0, beta=1.0, gamma=7.0,
                        tensile_correction=True, summation_density=True)
        return s.get_equations(), K.CubicSpline(dim=3), 3, WC_OUT
    if name == 'sd_1d_line':
        eqs = [Group(equations=[SummationDensity(dest='fluid',
                                                 sources=['fluid'])])]
        return eqs, K.CubicSpline(dim=1), 1, ['rho']
    if name == 'tvf_cube':
        dx = float(g['meta/dx'])
        s = TVFScheme(['fluid'], [], dim=3, rho0=1.0, c0=10.0, nu=0.01,
                      p0=100.0, pb=100.0, h0=dx, gx=0.1, alpha=0.2)
        return s.get_equations(), K.QuinticSpline(dim=3), 3, TVF_OUT
    if name == 'tvf_wall':
        dx = float(g['meta/dx'])
        # wall equations: the product's own (pysph_amd/wall_bc.py), or -- for the
        # cross-check against the statement-by-statement restatement of the
        # reference's bodies -- tests/wall_equations_fixture.py
        s = TVFScheme(['fluid'], ['wall'], dim=3, rho0=1.0, c0=10.0, nu=0.01,
                      p0=100.0, pb=100.0, h0=dx, gy=-0.5, alpha=0.2,
                      wall_equations=wall_equations)
        return s.get_equations(), K.QuinticSpline(dim=3), 3, TVF_OUT + [
            'wij', 'uf', 'vf', 'wf', 'ug', 'vg', 'wg']
    if name in ('elastic_2d', 'elastic_3d'):
        from pysph_amd.solid_mech import ElasticSolidsScheme
        dim = int(g['meta/dim'])
        s = ElasticSolidsScheme(['solid'], [], dim=dim)
        return s.get_equations(), K.CubicSpline(dim=dim), dim, EL_OUT
    raise KeyError(name)


def rel_err(a, b, scale=None):
    """max |a-b| / scale, scale = max|b| of the field unless given (mixed
    abs/rel measure: accelerations near cancellation are judged against the
    field's magnitude, SURVEY.md section 7 'Hard parts')."""
    a = np.asarray(a, dtype=float)
    b = np.asarray(b, dtype=float)
    if scale is None:
        scale = max(np.max(np.abs(b)), 1e-300) if b.size else 1.0
    return float(np.max(np.abs(a - b)) / scale) if b.size else 0.0


class ThreadDist(object):
    """In-process stand-in for ``torch.distributed`` used by the -m gpu tests:
    `world` threads play the ranks of one node on ONE GPU (RCCL cannot put two
    ranks on one device).  Tensors are handed over by reference and copied on
    the receiver's stream after a device synchronize -- the ordering RCCL's
    stream semantics give.  ``view(rank)`` returns the per-rank object to pass
    as ``dist=``."""

    def __init__(self, world):
        import queue
        import threading
        try:                      # initialise torch's HIP state once, in the
            import torch          # creating thread (lazy init from several
            if torch.cuda.is_available():      # threads at once races)
                torch.cuda.init()
                torch.zeros(1, device='cuda')      # forces context creation
                torch.cuda.synchronize()
        except ImportError:
            pass
        self.world = world
        self.barrier = threading.Barrier(world)
        self.slots = [None] * world
        self.q = {(a, b): queue.Queue() for a in range(world) for b in range(world)}

    def view(self, rank):
        return _ThreadDistRank(self, rank)


class _Done(object):
    def wait(self):
        return True


class _ThreadDistRank(object):
    class ReduceOp(object):
        MIN, MAX, SUM = 'min', 'max', 'sum'

    class P2POp(object):
        def __init__(self, op, tensor, peer):
            self.op, self.tensor, self.peer = op, tensor, peer

    isend, irecv = 'isend', 'irecv'

    def __init__(self, hub, rank):
        self.hub, self.rank = hub, rank

    def _sync(self):
        import torch
        if torch.cuda.is_available():
            torch.cuda.synchronize()

    def all_gather_into_tensor(self, out, inp):
        import torch
        hub = self.hub
        self._sync()
        hub.slots[self.rank] = inp.clone()
        self._sync()
        hub.barrier.wait()
        out.copy_(torch.cat([s.reshape(-1) for s in hub.slots]))
        self._sync()
        hub.barrier.wait()

    def all_reduce(self, t, op=None):
        import torch
        hub = self.hub
        self._sync()
        hub.slots[self.rank] = t.clone()
        self._sync()
        hub.barrier.wait()
        st = torch.stack(hub.slots)
        r = {'min': st.min(0).values, 'max': st.max(0).values, 'sum': st.sum(0)}[op]
        self._sync()
        hub.barrier.wait()
        t.copy_(r)
        self._sync()
        hub.barrier.wait()

    def batch_isend_irecv(self, reqs):
        hub = self.hub
        self._sync()
        for r in reqs:
            if r.op == 'isend':
                hub.q[(self.rank, r.peer)].put(r.tensor)
        for r in reqs:
            if r.op == 'irecv':
                src = hub.q[(r.peer, self.rank)].get(timeout=120)
                r.tensor.copy_(src[:r.tensor.numel()])
        self._sync()
        return [_Done()]

    def barrier(self):
        self.hub.barrier.wait()


def live_rows(pa, prop='x'):
    """property `prop` of every row the DEVICE array holds that is a particle: the padding rows of the round-trip-free
    ghost protocols (sph_halo_append_padded, sph_domain_images_padded) are parked at 1e18 and skipped"""
    import numpy as np
    from pysph_amd import device as dev
    g = pa.gpu
    n = g.get_number_of_particles()
    out = {}
    for q in ('x', prop):
        b = np.empty(n)
        dev._check(g.lib.sph_array_pull(g.ctx._h, g.array_id, dev.prop_id(q), b.ctypes.data_as(dev._PD), 0, n))
        out[q] = b
    return out[prop][np.abs(out['x']) < 1e17]


class _DeviceView(object):
    """n doubles at a raw device address, for torch.as_tensor (__cuda_array_interface__)"""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {'shape': (int(n),), 'typestr': '<f8', 'data': (int(ptr), False), 'version': 2}


def device_add(pa, prop, delta, n=None):
    """property `prop` of the DEVICE copy of `pa` += delta (host array, first n rows), written in place on the device
    through the property's raw pointer -- what a device-resident mover (a stage kernel) does; a host push of positions
    would make the next neighbour update look at the particles first (positions from the host may lie anywhere).  The
    host copy is updated alike."""
    import torch
    g = pa.gpu
    n = len(delta) if n is None else n
    g.ctx.synchronize()
    t = torch.as_tensor(_DeviceView(g.device_ptr(prop), n), device=torch.device('cuda', g.ctx.device))
    t += torch.from_numpy(np.ascontiguousarray(delta[:n], dtype=np.float64)).to(t.device)
    torch.cuda.synchronize()
    pa.properties[prop][:n] += delta[:n]


# ---------------------------------------------------------------------------
# Device-function probes (tests/probes/device_functions.hip) and their
# high-precision reference
# ---------------------------------------------------------------------------
_TESTS = os.path.dirname(os.path.abspath(__file__))
_REPO = os.path.dirname(_TESTS)
PROBE_SRC = os.path.join(_TESTS, 'probes', 'device_functions.hip')
KERNEL_NAMES = {1: 'CubicSpline', 2: 'WendlandQuintic', 3: 'QuinticSpline', 4: 'Gaussian'}
KERNEL_SUPPORT = {1: 2.0, 2: 2.0, 3: 3.0, 4: 3.0}
KERNEL_KNOTS = {1: (1.0,), 2: (), 3: (1.0, 2.0), 4: ()}
PAIR_OUT = ('rij', 'rinv', 'hij', 'h1', 'q', 'fac', 'eps', 'w', 'gradfac', 'gradh')


def _probe_command(out):
    """hipcc with exactly the CXXFLAGS of pysph_amd/csrc/Makefile (read from it, so that the probe is optimised and
    contracted like the product) + -shared."""
    import re
    csrc = os.path.join(_REPO, 'pysph_amd', 'csrc')
    flags = None
    with open(os.path.join(csrc, 'Makefile')) as f:
        for line in f:
            m = re.match(r'CXXFLAGS\s*=\s*(.*)', line)
            if m:
                flags = m.group(1).split()
                break
    assert flags, 'no CXXFLAGS in pysph_amd/csrc/Makefile'
    flags = [x.replace('$(ARCH)', 'gfx950') for x in flags]
    flags = ['-I' + os.path.normpath(os.path.join(csrc, x[2:])) if x.startswith('-I') else x for x in flags]
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    return [hipcc] + flags + ['-I' + csrc, '-shared', PROBE_SRC, '-o', out]


def probe_library_path():
    """content-addressed: the probe's own source, everything srchash covers (csrc/, include/) and the command line"""
    import hashlib
    import sys
    sys.path.insert(0, os.path.join(_REPO, 'pysph_amd', 'csrc'))
    import srchash
    from pysph_amd import codegen
    h = hashlib.sha256()
    with open(PROBE_SRC, 'rb') as f:
        h.update(f.read())
    h.update(srchash.source_hash().encode())
    h.update(' '.join(_probe_command('')[1:]).encode())
    return os.path.join(codegen.GEN_DIR, 'probe_device_functions_%s.so' % h.hexdigest()[:16])


def build_probe_library():
    """The probe library next to the generated families' shared objects (built by tests/prebuild_generated.py, so it
    travels with the tree); compiled here when it is missing.  No hipcc and no library is an error, not a skip."""
    import shutil
    import subprocess
    so = os.environ.get('SPH_PROBE_LIBRARY') or probe_library_path()      # like SPH_LIBRARY: one built elsewhere
    if os.path.exists(so):
        return so
    cmd = _probe_command(so + '.tmp%d' % os.getpid())
    if not (os.path.isfile(cmd[0]) or shutil.which(cmd[0])):
        raise RuntimeError('%s is missing and there is no hipcc (%s) to build it' % (so, cmd[0]))
    os.makedirs(os.path.dirname(so), exist_ok=True)
    subprocess.check_call(cmd)
    os.replace(cmd[-1], so)
    return so


_PROBE = []


def probe_library():
    import ctypes as C
    if not _PROBE:
        lib = C.CDLL(build_probe_library())
        vp, i, d = C.c_void_p, C.c_int, C.c_double
        lib.probe_kernel.argtypes = [i, i, i, i, vp, vp, vp, vp]
        lib.probe_rcp.argtypes = [i, i, vp, vp]
        lib.probe_sqrt_rsqrt.argtypes = [i, i, vp, vp, vp]
        lib.probe_pair.argtypes = [i, i, i, i, vp, vp, vp, d, i, d, d, d, d, vp]
        _PROBE.append(lib)
    return _PROBE[0]


def _vp(a):
    return a.ctypes.data


def probe_kernel(kk, insup, q):
    """device SphKernel<kk>::w/dw/dwq<insup>(q); the dtype of q (float64 / float32) selects the arithmetic"""
    q = np.ascontiguousarray(q)
    out = [np.empty_like(q) for _ in range(3)]
    rc = probe_library().probe_kernel(kk, int(insup), int(q.dtype == np.float32), q.size, _vp(q), *map(_vp, out))
    assert rc == 0, 'probe_kernel: HIP error %d' % rc
    return out


def probe_rcp(x):
    x = np.ascontiguousarray(x)
    r = np.empty_like(x)
    rc = probe_library().probe_rcp(int(x.dtype == np.float32), x.size, _vp(x), _vp(r))
    assert rc == 0, 'probe_rcp: HIP error %d' % rc
    return r


def probe_sqrt_rsqrt(x):
    x = np.ascontiguousarray(x)
    s, rs = np.empty_like(x), np.empty_like(x)
    rc = probe_library().probe_sqrt_rsqrt(int(x.dtype == np.float32), x.size, _vp(x), _vp(s), _vp(rs))
    assert rc == 0, 'probe_sqrt_rsqrt: HIP error %d' % rc
    return s, rs


def probe_pair(kk, uh, r2, hi, hj, sigma, dim, uniform=(0.0, 0.0, 0.0, 0.0)):
    """device pair_geom<kk, uh> + pair_w / pair_gradfac / pair_gradh; dict of the PAIR_OUT arrays"""
    r2 = np.ascontiguousarray(r2)
    hi = np.ascontiguousarray(hi, dtype=r2.dtype)
    hj = np.ascontiguousarray(hj, dtype=r2.dtype)
    assert hi.size == r2.size and hj.size == r2.size
    out = np.empty((len(PAIR_OUT), r2.size), dtype=r2.dtype)
    rc = probe_library().probe_pair(kk, int(uh), int(r2.dtype == np.float32), r2.size, _vp(r2), _vp(hi), _vp(hj),
                                    float(sigma), int(dim), *[float(u) for u in uniform], _vp(out))
    assert rc == 0, 'probe_pair: HIP error %d' % rc
    return dict(zip(PAIR_OUT, out))


def mp_kernel(kk, q):
    """(W(q), dW/dq(q)) without the normalisation, at mpmath's working precision, from the formulas and branch
    conditions of the reference's pysph/base/kernels.py (CubicSpline.kernel/dwdq, WendlandQuintic, QuinticSpline,
    Gaussian) -- NOT from pysph_amd/kernels.py -- with ITS operations in ITS order (Python evaluates a * b * c as
    (a * b) * c).  At 50 digits the order is immaterial; at a working precision of 53 bits mpmath rounds every
    operation to nearest like IEEE double, and the same lines then retrace the reference's own fp64 evaluation
    rounding by rounding -- which is how the formulas are pinned against tests/golden/kernels.npz before anything is
    judged by them.  q: an mpf (a double or float converts exactly).  The reference's rij > 1e-12 guard of dwdq
    belongs to the caller (it tests rij, not q)."""
    import mpmath as mp
    q = mp.mpf(q)
    f = mp.mpf
    if kk == 1:
        tmp2 = 2 - q
        if q > 2:
            return f(0), f(0)
        if q > 1:
            return f(0.25) * tmp2 * tmp2 * tmp2, f(-0.75) * tmp2 * tmp2
        return 1 - f(1.5) * q * q * (1 - f(0.5) * q), f(-3) * q * (1 - f(0.75) * q)
    if kk == 2:
        tmp = 1 - f(0.5) * q
        if q < 2:
            return tmp * tmp * tmp * tmp * (2 * q + 1), f(-5) * q * tmp * tmp * tmp
        return f(0), f(0)
    if kk == 3:
        tmp3, tmp2, tmp1 = 3 - q, 2 - q, 1 - q
        if q > 3:
            return f(0), f(0)
        w = tmp3 * tmp3 * tmp3 * tmp3 * tmp3
        dw = f(-5) * tmp3 * tmp3 * tmp3 * tmp3
        if q <= 2:
            w -= f(6) * tmp2 * tmp2 * tmp2 * tmp2 * tmp2
            dw += f(30) * tmp2 * tmp2 * tmp2 * tmp2
        if q <= 1:
            w += f(15) * tmp1 * tmp1 * tmp1 * tmp1 * tmp1
            dw -= f(75) * tmp1 * tmp1 * tmp1 * tmp1
        return w, dw
    if kk == 4:
        if q < 3:
            return mp.exp(-q * q), f(-2) * q * mp.exp(-q * q)
        return f(0), f(0)
    raise KeyError(kk)


def mp_kernel_wdw(kk, r, h, sigma, dim, xij=None):
    """the reference's kernel(rij, h) and dwdq(rij, h) -- and, with xij, gradient(xij, rij, h) -- at mpmath's working
    precision, operation by operation as the reference writes them (fac = self.fac * h1 * h1 * h1, val * fac,
    wdash * h1 / rij * xij).  Its h1 = 1 / h and q = rij * h1 are formed in the arithmetic of the inputs' type: that
    rounding is the reference's definition of q, not an error of W."""
    import mpmath as mp
    one = type(r)(1)
    h1 = one / h
    q = r * h1
    w, dw = mp_kernel(kk, q)
    fac = mp.mpf(float(sigma))
    for _ in range(dim):
        fac = fac * mp.mpf(h1)
    if not r > 1e-12:
        dw = mp.mpf(0)
    w, dw = w * fac, dw * fac
    if xij is None:
        return w, dw
    tmp = dw * mp.mpf(h1) / mp.mpf(r) if r > 1e-12 else mp.mpf(0)
    return w, dw, [tmp * mp.mpf(float(c)) for c in xij]


# ---------------------------------------------------------------------------
# Equations without sources (k_nosrc): high-precision restatements of the reference's bodies, each with the
# condition scale of every output element, and numpy restatements of the DEVICE arithmetic (for mutation runs)
# ---------------------------------------------------------------------------
U53 = 2.0 ** -53      # unit roundoff of fp64
S6 = ('s00', 's01', 's02', 's11', 's12', 's22')
R6 = ('r00', 'r01', 'r02', 'r11', 'r12', 'r22')
AS6 = ('as00', 'as01', 'as02', 'as11', 'as12', 'as22')
V9 = ('v00', 'v01', 'v02', 'v10', 'v11', 'v12', 'v20', 'v21', 'v22')
_IJ6 = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def _dps50(fn):
    """run fn at 50 significant digits (mpf values keep the precision they were made with; operations round to the
    working precision in force)"""
    import functools

    @functools.wraps(fn)
    def wrapped(*a, **k):
        import mpmath as mp
        with mp.workdps(50):
            return fn(*a, **k)
    return wrapped


@_dps50
def mp_tait(rho, rho0, c0, gamma, p0=0.0, hg=False):
    """TaitEOS (wc/basic.py:60-65) or, with hg, TaitEOSHGCorrection (:118-126) at mpmath's working precision from the
    fp64 inputs: {'rho': written-back density, 'p': (value, scale), 'cs': (value, scale)} with lists over rho.
    Scale of p: B(|tmp| + 1) + |p0|; of cs (a single product): |c0 ratio^gamma1|."""
    import mpmath as mp
    f = mp.mpf
    rho0, c0, gamma, p0 = f(float(rho0)), f(float(c0)), f(float(gamma)), f(float(p0))
    rho01, gamma1, B = 1 / rho0, (gamma - 1) / 2, rho0 * c0 * c0 / gamma
    out = {'rho': [], 'p': ([], []), 'cs': ([], [])}
    for r in rho:
        r = f(float(r))
        if hg and r < rho0:
            r = rho0
        ratio = r * rho01
        tmp = mp.power(ratio, gamma)
        out['rho'].append(r)
        out['p'][0].append(p0 + B * (tmp - 1))
        out['p'][1].append(B * (abs(tmp) + 1) + abs(p0))
        cs = c0 * mp.power(ratio, gamma1)
        out['cs'][0].append(cs)
        out['cs'][1].append(abs(cs))
    return out


@_dps50
def mp_state_equation(rho, p0, rho0, b):
    """transport_velocity.py:215-216: p0 (rho / rho0 - b); scale |p0| (|rho / rho0| + |b|)"""
    import mpmath as mp
    f = mp.mpf
    p0, rho0, b = f(float(p0)), f(float(rho0)), f(float(b))
    val = [p0 * (f(float(r)) / rho0 - b) for r in rho]
    return {'p': (val, [abs(p0) * (abs(f(float(r)) / rho0) + abs(b)) for r in rho])}


@_dps50
def mp_isothermal(rho, rho0, c0, p0):
    """basic_equations.py:175-176: p0 + c0^2 (rho - rho0); with p0 = 0 also solid_mech/basic.py:100-101
    (c0_ref c0_ref (rho - rho_ref)).  Scale |p0| + c0^2 |rho - rho0|: the terms as the formula writes them."""
    import mpmath as mp
    f = mp.mpf
    rho0, c0, p0 = f(float(rho0)), f(float(c0)), f(float(p0))
    val = [p0 + c0 * c0 * (f(float(r)) - rho0) for r in rho]
    return {'p': (val, [abs(p0) + c0 * c0 * abs(f(float(r)) - rho0) for r in rho])}


@_dps50
def mp_artificial_stress(rho, p, s6, eps):
    """solid_mech/basic.py:170-242 with the eigen-decomposition of mpmath.eigsy: R = sum over lambda_k > 0 of
    (-eps lambda_k / rho^2) v_k v_k^T of S = s - p I (formed exactly from the fp64 inputs).  Returns ({r00..r22:
    (values, scales)}, eigenvalues per particle); the scale of all six components of a particle is eps |S|_F / rho^2."""
    import mpmath as mp
    f = mp.mpf
    eps = f(float(eps))
    out = dict((k, ([], [])) for k in R6)
    lams = []
    for i in range(len(rho)):
        S = mp.zeros(3, 3)
        for k, (a, b) in zip(S6, _IJ6):
            S[a, b] = S[b, a] = f(float(s6[k][i]))
        for a in range(3):
            S[a, a] -= f(float(p[i]))
        rho21 = 1 / (f(float(rho[i])) ** 2)
        fro = mp.sqrt(sum(S[a, b] ** 2 for a in range(3) for b in range(3)))
        if fro == 0:
            E, Q = [f(0)] * 3, mp.eye(3)
        else:
            E, Q = mp.eigsy(S / fro)            # scaled like the reference: mpmath's iteration then sees O(1) entries
            # an exact zero eigenvalue comes back as +-1e-50: below 1e-40 (ten digits above eigsy's own error at this
            # precision, 24 below fp64's) it IS zero
            E = [(e if abs(e) > mp.mpf(10) ** -40 else f(0)) * fro for e in E]
        R = mp.zeros(3, 3)
        for k in range(3):
            if E[k] > 0:
                rd = -eps * E[k] * rho21
                for a in range(3):
                    for b in range(a, 3):
                        R[a, b] += Q[a, k] * rd * Q[b, k]
        lams.append(list(E))
        for k, (a, b) in zip(R6, _IJ6):
            out[k][0].append(R[a, b])
            out[k][1].append(eps * fro * rho21)
    return out, lams


@_dps50
def mp_hooke(v9, s6, G, termwise=False):
    """solid_mech/basic.py:418-505: as_ij = 2G (eps_ij - delta_ij trace) + sum_k s_ik omega_jk + sum_k s_kj omega_ik,
    eps = (v + v^T)/2, omega = (v - v^T)/2, trace = (eps00 + eps11 + eps22)/3.  Scale of a component: |2G eps_ij|,
    |2G trace| on the diagonal, and every |s omega| product of its two sums; with termwise the trace enters by ITS
    terms, 2G (|eps00| + |eps11| + |eps22|) / 3 (a trace that cancels carries the roundings of its sum)."""
    import mpmath as mp
    f = mp.mpf
    G2 = 2 * f(float(G))
    out = dict((k, ([], [])) for k in AS6)
    for n in range(len(v9['v00'])):
        v = [[f(float(v9['v%d%d' % (a, b)][n])) for b in range(3)] for a in range(3)]
        s = [[f(0)] * 3 for _ in range(3)]
        for k, (a, b) in zip(S6, _IJ6):
            s[a][b] = s[b][a] = f(float(s6[k][n]))
        e = [[(v[a][b] + v[b][a]) / 2 for b in range(3)] for a in range(3)]
        w = [[(v[a][b] - v[b][a]) / 2 for b in range(3)] for a in range(3)]
        trace = (e[0][0] + e[1][1] + e[2][2]) / 3
        for k, (i, j) in zip(AS6, _IJ6):
            val = G2 * (e[i][j] - (trace if i == j else 0))
            tr = (abs(e[0][0]) + abs(e[1][1]) + abs(e[2][2])) / 3 if termwise else abs(trace)
            scale = abs(G2 * e[i][j]) + (abs(G2) * tr if i == j else 0)
            for m in range(3):
                val += s[i][m] * w[j][m] + s[m][j] * w[i][m]
                scale += abs(s[i][m] * w[j][m]) + abs(s[m][j] * w[i][m])
            out[k][0].append(val)
            out[k][1].append(scale)
    return out


@_dps50
def k_measure(got, ref):
    """max over the elements of |got - ref| / (u scale), evaluated in mpmath so that the reference is never rounded;
    an element of scale 0 (every term of its formula is zero) must be exact.  got: {name: fp64 array}, ref: {name:
    (values, scales)}.  Returns (K, (name, index) of the worst element)."""
    import mpmath as mp
    worst, where = 0.0, None
    u = mp.mpf(U53)
    for name, (vals, scales) in ref.items():
        g = got[name]
        assert len(g) == len(vals), (name, len(g), len(vals))
        for i in range(len(vals)):
            d = abs(mp.mpf(float(g[i])) - vals[i])
            if d == 0:
                continue
            k = float(d / (u * scales[i])) if scales[i] != 0 else float('inf')
            if not k <= worst:
                worst, where = k, (name, i)
    return worst, where


def np_jacobi_eigen3(S, max_sweeps=12, tol=1e-18):
    """numpy restatement of the device's jacobi_eigen3 (pysph_amd/csrc/sph_eval.hip), statement by statement, without
    fma contraction; max_sweeps / tol are the knobs the mutation runs turn"""
    A = np.array(S, dtype=float)
    V = np.eye(3)
    for sweep in range(max_sweeps):
        off = abs(A[0, 1]) + abs(A[0, 2]) + abs(A[1, 2])
        diag = abs(A[0, 0]) + abs(A[1, 1]) + abs(A[2, 2])
        if off <= 1e-300 or off <= tol * diag:
            break
        for p, q in ((0, 1), (0, 2), (1, 2)):
            apq = A[p, q]
            if apq == 0.0:
                continue
            with np.errstate(all='ignore'):
                theta = (A[q, q] - A[p, p]) / (2.0 * apq)
                t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
            c = 1.0 / np.sqrt(t * t + 1.0)
            s = t * c
            A[p, p] -= t * apq
            A[q, q] += t * apq
            A[p, q] = A[q, p] = 0.0
            r = 3 - p - q
            arp, arq = A[r, p], A[r, q]
            A[r, p] = A[p, r] = c * arp - s * arq
            A[r, q] = A[q, r] = s * arp + c * arq
            for k in range(3):
                vkp, vkq = V[k, p], V[k, q]
                V[k, p] = c * vkp - s * vkq
                V[k, q] = s * vkp + c * vkq
    return np.diag(A).copy(), V


def np_artificial_stress(rho, p, s6, eps, mutation=None):
    """numpy restatement of k_nosrc's SPH_EQ_MONAGHAN_ART_STRESS case (Gershgorin shortcut, scaling, Jacobi, the
    lam > 0 selection, R diag(rd) R^T); returns {r00..r22: array}.  mutation: None, 'sweeps' (the Jacobi iteration
    stops after two sweeps), ('gershgorin', r, c) (the term |S_rc| of row r's bound enters with the wrong sign) or 'ge'
    (lam >= 0 in place of lam > 0)."""
    n = len(rho)
    out = dict((k, np.zeros(n)) for k in R6)
    for i in range(n):
        S = np.zeros((3, 3))
        for k, (a, b) in zip(S6, _IJ6):
            S[a, b] = S[b, a] = s6[k][i]
        for a in range(3):
            S[a, a] -= p[i]
        rhoi21 = 1.0 / (rho[i] * rho[i])
        sgn = np.ones((3, 3))
        if isinstance(mutation, tuple) and mutation[0] == 'gershgorin':
            sgn[mutation[1], mutation[2]] = -1.0
        g0 = S[0, 0] + sgn[0, 1] * abs(S[0, 1]) + sgn[0, 2] * abs(S[0, 2])
        g1 = S[1, 1] + sgn[1, 0] * abs(S[0, 1]) + sgn[1, 2] * abs(S[1, 2])
        g2 = S[2, 2] + sgn[2, 0] * abs(S[0, 2]) + sgn[2, 1] * abs(S[1, 2])
        if max(g0, g1, g2) <= 0.0:
            continue
        sc = 0.0
        for a in range(3):
            for b in range(3):
                sc += abs(S[a, b])
        if sc == 0.0:
            lam, R = np.zeros(3), np.eye(3)
        else:
            lam, R = np_jacobi_eigen3(S / sc, max_sweeps=2 if mutation == 'sweeps' else 12)
            lam = lam * sc
        rd = np.zeros(3)
        for k in range(3):
            if (lam[k] >= 0 if mutation == 'ge' else lam[k] > 0):
                rd[k] = -eps * lam[k] * rhoi21
        for key, (a, b) in zip(R6, _IJ6):
            t = 0.0
            for k in range(3):
                t += R[a, k] * rd[k] * R[b, k]
            out[key][i] = t
    return out


def np_tait(rho, rho0, c0, gamma, p0=0.0, hg=False, mutation=None):
    """numpy restatement of k_nosrc's two Tait cases (rho (1 / rho0); powers by multiplication for gamma in 1, 3, 5, 7
    as tait_powers forms them, pow otherwise); mutation 'short': the power of gamma = 2 gk + 1 one multiplication
    short"""
    rho = np.array(rho, dtype=float)
    if hg:
        rho = np.where(rho < rho0, rho0, rho)
    ratio = rho * (1.0 / rho0)
    gk = {7.0: 3, 5.0: 2, 3.0: 1, 1.0: 0}.get(float(gamma), -1)
    r2 = ratio * ratio
    if gk == 3:
        rk = r2 * ratio
        rg = (r2 * r2) * (r2 if mutation == 'short' else rk)
    elif gk == 2:
        rk = r2
        rg = (r2 * r2) if mutation == 'short' else (r2 * r2) * ratio
    elif gk == 1:
        rk = ratio
        rg = r2 if mutation == 'short' else r2 * ratio
    elif gk == 0:
        rk, rg = np.ones_like(ratio), ratio
    else:
        rg, rk = np.power(ratio, gamma), np.power(ratio, 0.5 * (gamma - 1.0))
    return {'rho': rho, 'p': p0 + (rho0 * c0 * c0 / gamma) * (rg - 1.0), 'cs': c0 * rk}


# rounding cost, in units of u of the decoded value, of gsph_decode below (pstar, ustar), counted from the operations:
#   pstar: the destination's column is au = fl(fl(-m_j pstar) C) x_ij with C = c_i + c_j the pair factor.  m_j is a power
#          of two and x_ij = +-2^-3, so au carries one rounding, the calibration column (pstar_0 = fl((pl + pr) / 2), formed
#          here from the same two doubles in the same way) another, and the quotient and the product of the decoding one
#          each: 4 u.  C is the same bits in both launches and cancels.
#   ustar: the device forms ae = fl(f fl(ustar (e . x_ij))) with e . x_ij = 2^-3 and au = f x_ij exactly: two roundings and
#          the quotient, 3 u.  The reference forms vstar . DWI and vstar . DWJ (one rounding each), weighs them with
#          vij_i and vij_j (one each), adds (one) and multiplies by fl(-m_j pstar) (one); au goes the same way without
#          the first pair.  Both sums have terms of one sign, so each factor (1 + d) passes to the sum: 4 + 3 roundings
#          and the quotient, 8 u.  The larger figure is the stated one.
GSPH_DECODE_COST = (4.0, 8.0)


def gsph_decode(x, au, ae, au_cal, p_cal):
    """(pstar, ustar) of every destination of a table of isolated 1-D pairs (particles 2 k and 2 k + 1 are partners, 2^-3
    apart; tests/golden/make_gsph_riemann_golden.py) from the two columns GSPHAcceleration wrote with delta interpolation
    and no conduction: au_i = -m_j pstar (c_i + c_j) x_ij and ae_i = f ustar e x_ij.  ``au_cal`` is au of the SAME table
    under the non-diffusive solver, whose pstar is ``p_cal`` = (pl + pr) / 2, one rounding; where that is zero the pair
    cannot be calibrated (give it a twin).  ustar is not defined where au is zero (pstar = 0): NaN there.  The cost in
    roundings is GSPH_DECODE_COST."""
    x, au, ae, au_cal, p_cal = [np.asarray(a, dtype=np.float64) for a in (x, au, ae, au_cal, p_cal)]
    partner = np.arange(x.size) ^ 1
    e = np.sign(x - x[partner])
    assert np.all(np.abs(x - x[partner]) == 0.125)
    with np.errstate(divide='ignore', invalid='ignore'):
        pstar = au / au_cal * p_cal
        ustar = np.where(au != 0.0, e * ae / au, np.nan)
    return pstar, ustar
