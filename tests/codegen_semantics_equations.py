"""Construct corpus for the translator (pysph_amd/codegen.py): every Python
construct it accepts, a few statements per case, each case writing ONE
destination property from the input properties

    a b c   any sign and magnitude (signed zeros, ties, thresholds)
    p       > 0         u   in [-1, 1], never 0
    e       in [-700, 700], never 0         k   integer-valued, in [-5, 5]

and ``self.*`` parameters.  The classes are no physics.  They run as CPython
(oracle/py_eval.py) and as generated HIP; tests/test_codegen_semantics.py
compares the two value by value.  Every class sets ``_fp_contract_ = False``:
each product and sum is rounded on its own, so plain arithmetic is comparable
bit for bit.  The classes named in F32_FAMILIES keep every intermediate exact in
fp32 when the inputs are multiples of 1/8 below 64 (dyadic literals, at most
two inputs multiplied, divisions by powers of two).
"""
import math
import math as M
from math import (acos, asin, atan, atan2, ceil, cos, cosh, erf, exp, fabs, floor, fmod,  # noqa: F401
                  log, log10, pi, sin, sinh, sqrt, tan, tanh)

import numpy as np

from oracle.py_eval import declare  # noqa: F401
from pysph_amd.equations import Equation

# the C spellings the translator accepts, with the values of <math.h>
M_PI = 3.14159265358979323846
M_PI_2 = 1.57079632679489661923
M_1_PI = 0.31830988618379067154
M_2_SQRTPI = 1.12837916709551257390
INFINITY = float('inf')


class Strict(Equation):
    _fp_contract_ = False


# ---------------------------------------------------------------------------
# family "ops": operators on doubles
# ---------------------------------------------------------------------------
class Arith(Strict):
    def loop(self, d_idx, d_a, d_b, d_c, d_p, d_cs, d_arho, d_au, d_av, d_aw, d_ax, d_ay, d_az):
        """a docstring is skipped"""
        d_cs[d_idx] = d_a[d_idx] + d_b[d_idx]  # add
        d_arho[d_idx] = d_a[d_idx] - d_b[d_idx]  # sub
        d_au[d_idx] = d_a[d_idx] * d_b[d_idx]  # mul
        d_av[d_idx] = d_a[d_idx] / d_p[d_idx] + 1 / d_p[d_idx]  # div
        d_aw[d_idx] = d_a[d_idx] * d_b[d_idx] + d_c[d_idx]  # mac
        d_ax[d_idx] = -d_a[d_idx] - -d_b[d_idx]  # neg
        d_ay[d_idx] = +d_a[d_idx]  # pos
        d_az[d_idx] = 3 + 0.25 * d_a[d_idx] + True - False * 2 + 1e-3 + 7 / 2  # lit


class Modulo(Strict):
    def loop(self, d_idx, d_a, d_p, d_V, d_uhat, d_vhat, d_what, d_auhat, d_avhat, d_awhat, d_x0,
             d_y0, d_z0, d_u0, d_v0):
        d_V[d_idx] = d_a[d_idx] % d_p[d_idx]  # mpp
        d_uhat[d_idx] = d_a[d_idx] % -d_p[d_idx]  # mpn
        d_vhat[d_idx] = (-d_a[d_idx]) % d_p[d_idx]  # mnp
        d_what[d_idx] = (-d_a[d_idx]) % (-d_p[d_idx])  # mnn
        d_auhat[d_idx] = d_a[d_idx] % 0.3  # mlit
        d_avhat[d_idx] = (-d_a[d_idx]) % 0.3  # mlitn
        d_awhat[d_idx] = (d_p[d_idx] * 4.0) % d_p[d_idx]           # mmul: an exact multiple: the zero has the divisor's sign
        d_x0[d_idx] = (d_p[d_idx] * -4.0) % d_p[d_idx] + (d_p[d_idx] * 2.0) % -d_p[d_idx]  # mmuln
        d_y0[d_idx] = (d_p[d_idx] * 2.5) % d_p[d_idx]  # mhalf
        d_z0[d_idx] = fmod(d_a[d_idx], d_p[d_idx])              # mfm: by name: C semantics, as math.fmod
        d_u0[d_idx] = math.fmod(-d_a[d_idx], d_p[d_idx]) + np.fmod(d_a[d_idx], -d_p[d_idx])  # mfn
        d_v0[d_idx] = d_idx % 3 + (d_idx % 4) / 2  # midx


class Compare(Strict):
    def loop(self, d_idx, d_a, d_b, d_c, d_w0, d_rho0, d_vmag2, d_ae, d_e0, d_v00, d_v01, d_v02, d_v10, d_v11):
        d_w0[d_idx] = d_a[d_idx] < d_b[d_idx]  # lt
        d_rho0[d_idx] = d_a[d_idx] > d_b[d_idx]  # gt
        d_vmag2[d_idx] = d_a[d_idx] <= d_b[d_idx]  # le
        d_ae[d_idx] = d_a[d_idx] >= d_b[d_idx]  # ge
        d_e0[d_idx] = d_a[d_idx] == d_b[d_idx]  # eq
        d_v00[d_idx] = d_a[d_idx] != d_b[d_idx]  # ne
        d_v01[d_idx] = d_a[d_idx] < d_b[d_idx] < d_c[d_idx]  # ch1
        d_v02[d_idx] = d_a[d_idx] < d_b[d_idx] >= d_c[d_idx]  # ch2
        d_v10[d_idx] = (d_a[d_idx] < d_b[d_idx]) * 2.5 + (d_b[d_idx] <= d_c[d_idx]) - (d_a[d_idx] == d_c[d_idx]) / 4  # cnum
        # clit
        d_v11[d_idx] = (d_a[d_idx] > 0.5) + 2 * (d_a[d_idx] >= 0.5) + 4 * (d_a[d_idx] < -0.25) + \
            8 * (d_a[d_idx] <= -0.25) + 16 * (d_a[d_idx] == 0) + 32 * (d_a[d_idx] != 1e100)


class BoolValues(Strict):
    def loop(self, d_idx, d_a, d_b, d_c, d_v12, d_v20, d_v21, d_v22, d_s00, d_s01, d_s02, d_s11):
        d_v12[d_idx] = d_a[d_idx] or 5.0  # orv
        d_v20[d_idx] = d_a[d_idx] and d_b[d_idx]  # andv
        d_v21[d_idx] = d_a[d_idx] or d_b[d_idx] or d_c[d_idx]  # or3
        d_v22[d_idx] = d_a[d_idx] and d_b[d_idx] or d_c[d_idx]  # mix
        d_s00[d_idx] = (d_a[d_idx] - d_b[d_idx]) or (d_b[d_idx] * 2.0 and d_c[d_idx])  # ornest
        d_s01[d_idx] = (not d_a[d_idx]) * 3.0 + (not d_b[d_idx])  # notv
        d_s02[d_idx] = not (d_a[d_idx] < d_b[d_idx])  # notc
        r = 0.0
        if d_a[d_idx] > 0 and d_b[d_idx] > 0 or not d_c[d_idx] > 0:
            r = 1.0
        if d_a[d_idx] and not d_b[d_idx]:
            r += 2.0
        if (d_a[d_idx] or d_b[d_idx]) and d_c[d_idx]:
            r += 4.0
        d_s11[d_idx] = r  # bif


# ---------------------------------------------------------------------------
# family "sel": selections, rounding, constants and parameters
# ---------------------------------------------------------------------------
class Select(Strict):
    def __init__(self, dest, sources, lim=0.5):
        self.lim = lim
        super(Select, self).__init__(dest, sources)

    def loop(self, d_idx, d_a, d_b, d_c, d_cs, d_arho, d_au, d_av, d_aw, d_ax, d_ay, d_az, d_V,
             d_uhat, d_vhat):
        d_cs[d_idx] = d_a[d_idx] if d_a[d_idx] > d_b[d_idx] else d_b[d_idx]  # sel
        # sel2
        d_arho[d_idx] = d_a[d_idx] if d_a[d_idx] > self.lim else (
            d_b[d_idx] if d_b[d_idx] > self.lim else (d_c[d_idx] if d_c[d_idx] <= -self.lim else 0.25))
        d_au[d_idx] = max(d_a[d_idx], d_b[d_idx])  # mx2
        d_av[d_idx] = max(d_a[d_idx], d_b[d_idx], d_c[d_idx])  # mx3
        d_aw[d_idx] = max(d_a[d_idx], d_b[d_idx], d_c[d_idx], 0.0)  # mx4
        d_ax[d_idx] = min(d_a[d_idx], d_b[d_idx])  # mn2
        d_ay[d_idx] = min(d_a[d_idx], d_b[d_idx], d_c[d_idx])  # mn3
        d_az[d_idx] = min(d_a[d_idx], d_b[d_idx], d_c[d_idx], -0.0)  # mn4
        d_V[d_idx] = max(d_a[d_idx], 1) + min(2, d_b[d_idx])  # mxl
        d_uhat[d_idx] = abs(d_a[d_idx] - d_b[d_idx])  # abs
        # fab
        d_vhat[d_idx] = fabs(d_a[d_idx]) + math.fabs(d_b[d_idx]) + np.fabs(d_c[d_idx]) + M.fabs(d_a[d_idx]) + \
            np.abs(d_b[d_idx])


class Rounding(Strict):
    def loop(self, d_idx, d_a, d_p, d_what, d_auhat, d_avhat, d_awhat, d_x0, d_y0, d_z0, d_u0):
        d_what[d_idx] = floor(d_a[d_idx])  # flo
        d_auhat[d_idx] = ceil(d_a[d_idx])  # cei
        d_avhat[d_idx] = math.floor(d_a[d_idx] * 0.5)  # flm
        d_awhat[d_idx] = M.ceil(d_a[d_idx] * 0.5)  # cem
        d_x0[d_idx] = np.floor(d_a[d_idx])          # fln: numpy keeps the sign of a zero
        d_y0[d_idx] = np.ceil(d_a[d_idx])  # cen
        d_z0[d_idx] = sqrt(d_p[d_idx]) + math.sqrt(d_p[d_idx] * 2.0) + np.sqrt(d_p[d_idx] * 3.0) + M.sqrt(d_p[d_idx] * 5.0)  # sq
        d_u0[d_idx] = floor(d_a[d_idx] / d_p[d_idx]) + ceil(d_a[d_idx] / d_p[d_idx])  # flq


class Constants(Strict):
    def __init__(self, dest, sources, f=0.3, n=3, flag=True, off=False):
        self.f = f
        self.n = n
        self.flag = flag
        self.off = off
        super(Constants, self).__init__(dest, sources)

    def loop(self, d_idx, d_a, d_v0, d_w0, d_rho0, d_vmag2, d_ae, d_e0, d_v00, d_v01, d_v02,
             d_v10, d_v11, d_v12, d_v20, d_v21, t, dt):
        d_v0[d_idx] = d_a[d_idx] * M_PI  # kpi
        d_w0[d_idx] = d_a[d_idx] * pi  # kpi2
        d_rho0[d_idx] = d_a[d_idx] * M_1_PI  # k1pi
        d_vmag2[d_idx] = d_a[d_idx] * M_2_SQRTPI  # k2sp
        d_ae[d_idx] = d_a[d_idx] * M_PI_2  # kpih
        d_e0[d_idx] = min(d_a[d_idx], INFINITY) + (d_a[d_idx] < INFINITY)  # kinf
        d_v00[d_idx] = d_a[d_idx] + math.pi  # kmath
        d_v01[d_idx] = d_a[d_idx] - np.pi  # knp
        d_v02[d_idx] = d_a[d_idx] / M.pi  # km
        d_v10[d_idx] = d_a[d_idx] * self.f  # parf
        d_v11[d_idx] = self.n / 2 + d_a[d_idx] * self.n  # pari
        d_v12[d_idx] = self.flag * 2.5 + (1.0 if self.flag else 0.0) + (4.0 if self.off else 0.5) + self.off  # parb
        d_v20[d_idx] = d_idx * 0.5 + d_idx / 4  # idxv
        d_v21[d_idx] = t + 2 * dt  # tv


# ---------------------------------------------------------------------------
# family "flow": integers, statements, control flow, helpers (fp32-safe but for IntDivide64)
# ---------------------------------------------------------------------------
class IntArith(Strict):
    def __init__(self, dest, sources, n=5):
        self.n = n
        super(IntArith, self).__init__(dest, sources)

    def loop(self, d_idx, d_a, d_cs, d_arho, d_au, d_av, d_aw, d_ax, d_ay, d_az, d_V):
        i, j = declare('int', 2)
        ihalf = 0.0
        idiv = 0.0
        idivj = 0.0
        imod = 0.0
        imodj = 0.0
        isq = 0.0
        ineg = 0.0
        iflt = 0.0
        icmp = 0.0
        for i in range(-3, 6):
            ihalf += i * 0.5
            idiv += i / 2
            imod += (i % 2) * d_a[d_idx] + i % 4 / 4
            isq += i ** 2 + i ** 3 / 8
            ineg += -i * d_a[d_idx] + +i
            iflt += float(i) / 4 + float(i < 2)
            for j in range(1, 3):
                idivj += i / j + (i < j) / j + i / -j / 2
                imodj += i % j + i % -j
                icmp += (i == j) + 2 * (i < self.n) + 4 * (i != j)
        d_cs[d_idx] = ihalf  # ihalf
        d_arho[d_idx] = idiv  # idiv
        d_au[d_idx] = idivj  # idivj
        d_av[d_idx] = imod  # imod
        d_aw[d_idx] = imodj  # imodj
        d_ax[d_idx] = isq  # isq
        d_ay[d_idx] = ineg  # ineg
        d_az[d_idx] = iflt  # iflt
        d_V[d_idx] = icmp  # icmp


class IntLocals(Strict):
    def __init__(self, dest, sources, n=3):
        self.n = n
        super(IntLocals, self).__init__(dest, sources)

    def loop(self, d_idx, d_a, d_uhat, d_vhat):
        k, m, i = declare('int', 3)
        k = self.n
        m = k * 2 + 2
        k += m
        k -= 2
        k *= 3
        d_vhat[d_idx] = k / m  # il2
        m = -k if k > 20 else k
        m = m % 5
        i = (m < 3) + 1
        d_uhat[d_idx] = k * d_a[d_idx] + m / 4 + i  # il


class IntDivide64(Strict):
    """quotients that are no dyadic rationals: fp64 only"""

    def loop(self, d_idx, d_a, d_what):
        i, j = declare('int', 2)
        s = 0.0
        for i in range(-4, 5):
            for j in range(1, 8):
                s += i / j + (i % j) / j + (i < j) / j + i / -j * d_a[d_idx]
        d_what[d_idx] = s  # idv


class Statements(Strict):
    def loop(self, d_idx, d_a, d_b, d_c, d_auhat, d_avhat, d_awhat, d_x0, d_g3):
        """a docstring, then pass"""
        pass
        x, y = d_a[d_idx], d_b[d_idx] * 2.0
        d_auhat[d_idx] = x - y  # tup
        x, y = y, x
        x, y, z = y + 1.0, x, x + y
        d_avhat[d_idx] = x * 4.0 - y * 2.0 + z  # swap
        s = declare('double')
        n = declare('int')
        v = declare('matrix(3)')
        m = declare('matrix((3, 3))')
        i, j = declare('int', 2)
        f, g = declare('double'), declare('int')
        for i in range(3):
            v[i] = d_a[d_idx] * (i + 1)
            for j in range(3):
                m[3 * i + j] = (i - j) * d_b[d_idx]
        s = 0
        f = 0.5
        g = 2
        for i in range(3):
            for j in range(3):
                s += m[3 * i + j] * (j + g) + v[j] * f
        d_awhat[d_idx] = s  # decl
        w = d_c[d_idx]
        w += d_a[d_idx]
        w -= 0.5
        w *= d_b[d_idx]
        w /= 4
        n = 2
        n += 3
        n *= 2
        n -= i
        d_x0[d_idx] = w + n  # aug
        for i in range(3):
            d_g3[3 * d_idx + i] = v[i] + i  # v3


class Control(Strict):
    def __init__(self, dest, sources, n=4, lo=0.5):
        self.n = n
        self.lo = lo
        super(Control, self).__init__(dest, sources)

    def loop(self, d_idx, d_a, d_b, d_c, d_y0, d_z0, d_u0, d_v0, d_w0):
        r = 0.0
        if d_a[d_idx] > self.lo:
            if d_b[d_idx] > self.lo:
                if d_c[d_idx] > self.lo:
                    r = 1.0
                elif d_c[d_idx] < -self.lo:
                    r = 2.0
                else:
                    r = 3.0
            elif d_b[d_idx] == -d_a[d_idx]:
                r = 4.0
            else:
                r = 5.0
        elif d_a[d_idx] < -self.lo:
            r = 6.0 if d_b[d_idx] > 0 else 7.0
        else:
            r = 8.0
        d_y0[d_idx] = r  # ifs
        i, j, lo_, hi_, cnt = declare('int', 5)
        s = 0.0
        for i in range(4):
            s += i * d_a[d_idx]
        for i in range(self.n):
            s += 1
        for i in range(2, self.n):
            s += i
        lo_ = 1
        hi_ = 4
        for i in range(lo_, hi_):
            s += i * 0.25
            hi_ = 2                     # range() has taken its bounds already
        for i in range(hi_ + 2, lo_):
            s += 100.0                  # empty
        for i in range(3, 3):
            s += 100
        for i in range(0):
            s += 100
        d_z0[d_idx] = s + i            # rng: the counter of the last loop that ran
        s = 0.0
        cnt = 0
        for i in range(self.n):
            if i == 1:
                continue
            for j in range(6):
                if j == i:
                    continue
                if j > 3:
                    break
                s += d_b[d_idx] * j + i
                cnt += 1
            if i >= 2 and d_c[d_idx] > 0:
                break
        d_u0[d_idx] = s  # brk
        d_v0[d_idx] = cnt  # cnt
        d_w0[d_idx] = i + j * 0.5  # after


class EarlyReturnIf(Strict):
    def loop(self, d_idx, d_a, d_rho0):
        d_rho0[d_idx] = -1.0  # ret1
        if d_a[d_idx] > 0.5:
            return
        d_rho0[d_idx] = d_a[d_idx] * 2.0


class EarlyReturnFor(Strict):
    def post_loop(self, d_idx, d_b, d_vmag2):
        i = declare('int')
        d_vmag2[d_idx] = 0.0  # ret2
        for i in range(5):
            if i * 0.5 > d_b[d_idx]:
                return
            d_vmag2[d_idx] += 1.0
        d_vmag2[d_idx] += 100.0


def h_scale(x, y=2.0):
    return x * y + 0.25


def h_int(x, n=2, m=1):
    i = declare('int')
    s = 0.0
    for i in range(n):
        s += x * (i + m)
    return s


def h_fill(v=[0.0, 0.0], n=3, x=1.0):
    i = declare('int')
    for i in range(n):
        v[i] = x * (i + 1)


def h_dot(u=[0.0, 0.0], v=[0.0, 0.0], n=3):
    i = declare('int')
    s = 0.0
    for i in range(n):
        s += u[i] * v[i]
    return s


class HelperCalls(Strict):
    def _get_helpers_(self):
        return [h_scale, h_int, h_fill, h_dot]

    def loop(self, d_idx, d_a, d_b, d_ae, d_e0, d_v00):
        d_ae[d_idx] = h_scale(d_a[d_idx]) + h_scale(d_a[d_idx], 0.5) + h_scale(y=d_a[d_idx], x=d_b[d_idx])  # h1
        d_e0[d_idx] = h_int(d_a[d_idx]) + h_int(d_b[d_idx], 3) + h_int(d_a[d_idx], m=2) + h_int(d_b[d_idx], 3, 2)  # h2
        v = declare('matrix(3)')
        w = declare('matrix(3)')
        h_fill(v, 3, d_a[d_idx])
        h_fill(w, x=d_b[d_idx])
        d_v00[d_idx] = h_dot(v, w) + h_dot(v, w, 2)  # h3


class HelperAgain(Strict):
    """the helpers of HelperCalls from a second equation"""

    def _get_helpers_(self):
        return [h_scale, h_int]

    def loop(self, d_idx, d_b, d_c, d_v01):
        d_v01[d_idx] = h_scale(d_c[d_idx], d_b[d_idx]) - h_int(d_c[d_idx], 2)  # h4


class StateFlag(Strict):
    def __init__(self, dest, sources):
        self.flag = 0
        super(StateFlag, self).__init__(dest, sources)

    def loop(self, d_idx, d_a, d_v02):
        self.flag = -1
        d_v02[d_idx] = d_a[d_idx]  # st


class Inexact32(Strict):
    """no fp32-exact result: tells a float build from the fp64 build of the same family"""

    def loop(self, d_idx, d_a, d_r00):
        d_r00[d_idx] = d_a[d_idx] / 3.0


class PairCount(Equation):
    """gives the float build of a no-source family a pair launch to run in"""

    def initialize(self, d_idx, d_r01):
        d_r01[d_idx] = 0.0

    def loop(self, d_idx, d_r01):
        d_r01[d_idx] += 1.0


# ---------------------------------------------------------------------------
# family "libm": ONE library call per case (judged against mpmath)
# ---------------------------------------------------------------------------
class Powers(Strict):
    def loop(self, d_idx, d_p, d_u, d_k, d_cs, d_arho, d_au, d_av, d_aw, d_ax, d_ay, d_az, d_V,
             d_uhat, d_vhat):
        n = declare('int')
        d_cs[d_idx] = d_p[d_idx] ** 2  # pw2
        d_arho[d_idx] = d_p[d_idx] ** 2.0  # pw2f
        d_au[d_idx] = d_p[d_idx] ** 3  # pw3
        d_av[d_idx] = d_p[d_idx] ** -1  # pwm1
        d_aw[d_idx] = d_p[d_idx] ** 0.5  # pwh
        d_ax[d_idx] = d_p[d_idx] ** d_u[d_idx]  # pwr
        d_ay[d_idx] = (-d_p[d_idx]) ** 3  # pwn3
        d_az[d_idx] = (-d_p[d_idx]) ** d_k[d_idx]  # pwnk
        d_V[d_idx] = -d_p[d_idx] ** 2  # pwprec
        d_uhat[d_idx] = pow(d_p[d_idx], d_u[d_idx])  # pwcall
        n = 3
        d_vhat[d_idx] = d_p[d_idx] ** n  # pwint


class Libm(Strict):
    def loop(self, d_idx, d_p, d_u, d_e, d_what, d_auhat, d_avhat, d_awhat, d_x0, d_y0, d_z0, d_u0, d_v0,
             d_w0, d_rho0, d_vmag2, d_ae, d_e0):
        d_what[d_idx] = exp(d_e[d_idx])  # exp
        d_auhat[d_idx] = log(d_p[d_idx])  # log
        d_avhat[d_idx] = log10(d_p[d_idx])  # log10
        d_awhat[d_idx] = sin(d_e[d_idx])  # sin
        d_x0[d_idx] = cos(d_e[d_idx])  # cos
        d_y0[d_idx] = tan(d_e[d_idx])  # tan
        d_z0[d_idx] = tanh(d_e[d_idx])  # tanh
        d_u0[d_idx] = asin(d_u[d_idx])  # asin
        d_v0[d_idx] = acos(d_u[d_idx])  # acos
        d_w0[d_idx] = atan(d_e[d_idx])  # atan
        d_rho0[d_idx] = sinh(d_e[d_idx])  # sinh
        d_vmag2[d_idx] = cosh(d_e[d_idx])  # cosh
        d_ae[d_idx] = erf(d_u[d_idx])  # erf
        d_e0[d_idx] = atan2(d_u[d_idx], d_e[d_idx])  # atan2


class LibmPrefixed(Strict):
    """the same names through math. / np. / M. (numpy has no erf)"""

    def loop(self, d_idx, d_p, d_u, d_e, d_v00, d_v01, d_v02, d_v10, d_v11, d_v12, d_v20, d_v21,
             d_v22, d_s00, d_s01, d_s02, d_s11, d_s12, d_s22, d_as00):
        d_v00[d_idx] = math.exp(d_e[d_idx])  # mexp
        d_v01[d_idx] = np.log(d_p[d_idx])  # nlog
        d_v02[d_idx] = M.log10(d_p[d_idx])  # mlog10
        d_v10[d_idx] = np.sin(d_e[d_idx])  # nsin
        d_v11[d_idx] = math.cos(d_e[d_idx])  # mcos
        d_v12[d_idx] = np.tan(d_e[d_idx])  # ntan
        d_v20[d_idx] = M.tanh(d_e[d_idx])  # mtanh
        d_v21[d_idx] = np.asin(d_u[d_idx])  # nasin
        d_v22[d_idx] = math.acos(d_u[d_idx])  # macos
        d_s00[d_idx] = np.atan(d_e[d_idx])  # natan
        d_s01[d_idx] = M.sinh(d_e[d_idx])  # msinh
        d_s02[d_idx] = np.cosh(d_e[d_idx])  # ncosh
        d_s11[d_idx] = math.erf(d_u[d_idx])  # merf
        d_s12[d_idx] = np.atan2(d_e[d_idx], d_u[d_idx])  # natan2
        d_s22[d_idx] = np.pow(d_p[d_idx], d_u[d_idx])  # npow
        d_as00[d_idx] = M.pow(d_p[d_idx], -d_u[d_idx])  # mpow


# what each libm case computes, for the mpmath reference: case -> (function, argument properties)
LIBM_CASES = {
    'pw2': ('sq', 'p'), 'pw2f': ('sq', 'p'), 'pw3': ('cube', 'p'), 'pwm1': ('inv', 'p'), 'pwh': ('sqrt', 'p'),
    'pwr': ('pow', 'p', 'u'), 'pwn3': ('negcube', 'p'), 'pwnk': ('negpow', 'p', 'k'), 'pwprec': ('negsq', 'p'),
    'pwcall': ('pow', 'p', 'u'), 'pwint': ('cube', 'p'),
    'exp': ('exp', 'e'), 'log': ('log', 'p'), 'log10': ('log10', 'p'), 'sin': ('sin', 'e'), 'cos': ('cos', 'e'),
    'tan': ('tan', 'e'), 'tanh': ('tanh', 'e'), 'asin': ('asin', 'u'), 'acos': ('acos', 'u'), 'atan': ('atan', 'e'),
    'sinh': ('sinh', 'e'), 'cosh': ('cosh', 'e'), 'erf': ('erf', 'u'), 'atan2': ('atan2', 'u', 'e'),
    'mexp': ('exp', 'e'), 'nlog': ('log', 'p'), 'mlog10': ('log10', 'p'), 'nsin': ('sin', 'e'), 'mcos': ('cos', 'e'),
    'ntan': ('tan', 'e'), 'mtanh': ('tanh', 'e'), 'nasin': ('asin', 'u'), 'macos': ('acos', 'u'),
    'natan': ('atan', 'e'), 'msinh': ('sinh', 'e'), 'ncosh': ('cosh', 'e'), 'merf': ('erf', 'u'),
    'natan2': ('atan2', 'e', 'u'), 'npow': ('pow', 'p', 'u'), 'mpow': ('powneg', 'p', 'u'),
}


# ---------------------------------------------------------------------------
# family "pair": the same constructs inside a pair loop
# ---------------------------------------------------------------------------
class PairFlow(Strict):
    def __init__(self, dest, sources, n=4):
        self.n = n
        super(PairFlow, self).__init__(dest, sources)

    def initialize(self, d_idx, d_q, d_gx, d_arho):
        d_q[d_idx] = 0.0
        d_gx[d_idx] = 0.0
        d_arho[d_idx] = 0.0

    def loop(self, d_idx, s_idx, d_q, d_gx, d_arho, s_m, XIJ, RIJ, WIJ, WI, WJ, DWIJ):
        i = declare('int')
        if RIJ < 1e-12:
            return
        d_arho[d_idx] += 1.0
        WI = 0.5 * (WI + WJ)
        WJ = WI * 2.0
        DWIJ[0] = DWIJ[0] * 0.5
        s = 0.0
        for i in range(self.n):
            if i * 0.1 + 0.05 > RIJ:
                break
            s += s_m[s_idx] * (i + 1)
        d_q[d_idx] += s * WIJ + WJ + i / 2
        d_gx[d_idx] += DWIJ[0] * s_m[s_idx] + XIJ[0] % 0.3


class PairAfter(Strict):
    """reads the DWIJ the equation before it rewrote"""

    def initialize(self, d_idx, d_gy):
        d_gy[d_idx] = 0.0

    def loop(self, d_idx, s_idx, d_gy, s_m, DWIJ, RIJ):
        d_gy[d_idx] += DWIJ[0] * s_m[s_idx] * (RIJ or 5.0)


INPUTS = ('a', 'b', 'c', 'p', 'u', 'e', 'k')
FAMILIES = {
    'ops': [Arith, Modulo, Compare, BoolValues],
    'sel': [Select, Rounding, Constants],
    'flow': [IntArith, IntLocals, IntDivide64, Statements, Control, EarlyReturnIf, EarlyReturnFor, HelperCalls,
             HelperAgain, StateFlag],
    'libm': [Powers, Libm, LibmPrefixed],
}
# the classes of "flow" whose every intermediate is exact in fp32 on inputs that are multiples of 1/8 below 64
F32_SAFE = [IntArith, IntLocals, Statements, Control, EarlyReturnIf, EarlyReturnFor, HelperCalls, HelperAgain,
            StateFlag]
# the float builds: these classes, Inexact32 and PairCount (selections and value and / or are exact on the same inputs)
F32_FAMILIES = {'flow': F32_SAFE, 'sel': [Select, BoolValues]}
STRIDED = {'g3': 3}
# Outputs travel under the names of built-in properties (and g3, a strided property the suite has already): a
# name without a built-in id takes one of the process-wide user property slots the whole test session shares.
# family -> {property: case}
CASES = {
    'ops': {
        'cs': 'add', 'arho': 'sub', 'au': 'mul', 'av': 'div', 'aw': 'mac', 'ax': 'neg', 'ay': 'pos', 'az': 'lit',
        'V': 'mpp', 'uhat': 'mpn', 'vhat': 'mnp', 'what': 'mnn', 'auhat': 'mlit', 'avhat': 'mlitn', 'awhat': 'mmul',
        'x0': 'mmuln', 'y0': 'mhalf', 'z0': 'mfm', 'u0': 'mfn', 'v0': 'midx', 'w0': 'lt', 'rho0': 'gt',
        'vmag2': 'le', 'ae': 'ge', 'e0': 'eq', 'v00': 'ne', 'v01': 'ch1', 'v02': 'ch2', 'v10': 'cnum',
        'v11': 'clit', 'v12': 'orv', 'v20': 'andv', 'v21': 'or3', 'v22': 'mix', 's00': 'ornest', 's01': 'notv',
        's02': 'notc', 's11': 'bif',
    },
    'sel': {
        'cs': 'sel', 'arho': 'sel2', 'au': 'mx2', 'av': 'mx3', 'aw': 'mx4', 'ax': 'mn2', 'ay': 'mn3', 'az': 'mn4',
        'V': 'mxl', 'uhat': 'abs', 'vhat': 'fab', 'what': 'flo', 'auhat': 'cei', 'avhat': 'flm', 'awhat': 'cem',
        'x0': 'fln', 'y0': 'cen', 'z0': 'sq', 'u0': 'flq', 'v0': 'kpi', 'w0': 'kpi2', 'rho0': 'k1pi',
        'vmag2': 'k2sp', 'ae': 'kpih', 'e0': 'kinf', 'v00': 'kmath', 'v01': 'knp', 'v02': 'km', 'v10': 'parf',
        'v11': 'pari', 'v12': 'parb', 'v20': 'idxv', 'v21': 'tv',
    },
    'flow': {
        'cs': 'ihalf', 'arho': 'idiv', 'au': 'idivj', 'av': 'imod', 'aw': 'imodj', 'ax': 'isq', 'ay': 'ineg',
        'az': 'iflt', 'V': 'icmp', 'uhat': 'il', 'vhat': 'il2', 'what': 'idv', 'auhat': 'tup', 'avhat': 'swap',
        'awhat': 'decl', 'x0': 'aug', 'g3': 'v3', 'y0': 'ifs', 'z0': 'rng', 'u0': 'brk', 'v0': 'cnt', 'w0': 'after',
        'rho0': 'ret1', 'vmag2': 'ret2', 'ae': 'h1', 'e0': 'h2', 'v00': 'h3', 'v01': 'h4', 'v02': 'st',
    },
    'libm': {
        'cs': 'pw2', 'arho': 'pw2f', 'au': 'pw3', 'av': 'pwm1', 'aw': 'pwh', 'ax': 'pwr', 'ay': 'pwn3',
        'az': 'pwnk', 'V': 'pwprec', 'uhat': 'pwcall', 'vhat': 'pwint', 'what': 'exp', 'auhat': 'log',
        'avhat': 'log10', 'awhat': 'sin', 'x0': 'cos', 'y0': 'tan', 'z0': 'tanh', 'u0': 'asin', 'v0': 'acos',
        'w0': 'atan', 'rho0': 'sinh', 'vmag2': 'cosh', 'ae': 'erf', 'e0': 'atan2', 'v00': 'mexp', 'v01': 'nlog',
        'v02': 'mlog10', 'v10': 'nsin', 'v11': 'mcos', 'v12': 'ntan', 'v20': 'mtanh', 'v21': 'nasin',
        'v22': 'macos', 's00': 'natan', 's01': 'msinh', 's02': 'ncosh', 's11': 'merf', 's12': 'natan2',
        's22': 'npow', 'as00': 'mpow',
    },
}
