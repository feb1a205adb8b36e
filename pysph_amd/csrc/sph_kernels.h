// sph_kernels.h -- SPH smoothing kernels as device functions.
//
// Hand-written equivalents of the kernel classes in pysph/base/kernels.py
// (CubicSpline :29-163, WendlandQuintic :274-380, QuinticSpline :1050-1210,
// Gaussian :830-930).  The polynomial forms and branch conditions are the
// reference's; what changes is that h1 = 1/h, q and the normalisation
// fac = sigma * h1^dim are computed ONCE per pair and shared by W, dW/dq and
// the gradient (the reference recomputes them in every method).
// INSUP = true: the caller guarantees q < radius_scale (uniform-h pairs that
// passed the neighbour criterion), so the support test is dropped.
// Every function takes the dimension as a trailing argument; only the
// SuperGaussian, whose shape depends on it, reads it.  CUTOFF: the kernel is
// cut off where it is not zero (Gaussian, SuperGaussian).  GRADH_FLIPPED: the
// reference's gradient_h of this class has the opposite sign of
// -fac h1 (dw q + w dim), see SphKernel<10>.
#pragma once

#include <hip/hip_runtime.h>

template <int KIND> struct SphKernel;

// max / min as ONE instruction: fmax()/fmin() compile to a canonicalising v_max x, x in front of the v_max proper
// (IEEE mode, signalling-NaN quieting); the operands here are results of arithmetic, canonical already
__device__ __forceinline__ double raw_max(double a, double b)
{
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ double raw_min(double a, double b)
{
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float raw_max(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ float raw_min(float a, float b) { return fminf(a, b); }


// kernels.py:73-79: fac = self.fac*h1 | *h1*h1 | *h1*h1*h1
template <class R> __device__ __forceinline__ R kernel_norm(R sigma, R h1, int dim)
{
    R f = sigma * h1;
    if (dim > 1) f *= h1;
    if (dim > 2) f *= h1;
    return f;
}

template <> struct SphKernel<1> { // CubicSpline
    static constexpr bool HAS_DWQ = false, CUTOFF = false, GRADH_FLIPPED = false;
    template <bool INSUP = false, class R> static __device__ __forceinline__ R dwq(R, int = 0) { return R(0); }
    template <bool INSUP = false, class R> static __device__ __forceinline__ R w(R q, int = 0)
    {
        R t2 = R(2) - q;
        R a = R(0.25) * t2 * t2 * t2;
        R b = R(1) - R(1.5) * q * q * (R(1) - R(0.5) * q);
        return (!INSUP && q > R(2)) ? R(0) : (q > R(1) ? a : b);
    }
    template <bool INSUP = false, class R> static __device__ __forceinline__ R dw(R q, int = 0)
    {
        R t2 = R(2) - q;
        R a = R(-0.75) * t2 * t2;
        R b = R(-3) * q * (R(1) - R(0.75) * q);
        return (!INSUP && q > R(2)) ? R(0) : (q > R(1) ? a : b);
    }
};

// The reference tests q < 2 (kernels.py:318); at q == 2 the polynomial is an exact zero (t = 0), so q <= 2 returns the
// same value -- and the same bits, sign of the zero included, as INSUP = true, which has no test at all.
template <> struct SphKernel<2> { // WendlandQuintic
    static constexpr bool HAS_DWQ = true; // dw/q = -5 (1 - q/2)^3: no division by r needed
    static constexpr bool CUTOFF = false, GRADH_FLIPPED = false;
    template <bool INSUP = false, class R> static __device__ __forceinline__ R dwq(R q, int = 0)
    {
        R t = R(1) - R(0.5) * q;
        return (INSUP || q <= R(2)) ? R(-5) * t * t * t : R(0);
    }
    template <bool INSUP = false, class R> static __device__ __forceinline__ R w(R q, int = 0)
    {
        R t = R(1) - R(0.5) * q;
        R v = t * t * t * t * (R(2) * q + R(1));
        return (INSUP || q <= R(2)) ? v : R(0);
    }
    template <bool INSUP = false, class R> static __device__ __forceinline__ R dw(R q, int = 0)
    {
        R t = R(1) - R(0.5) * q;
        R v = R(-5) * q * t * t * t;
        return (INSUP || q <= R(2)) ? v : R(0);
    }
};

template <> struct SphKernel<3> { // QuinticSpline
    static constexpr bool HAS_DWQ = false, CUTOFF = false, GRADH_FLIPPED = false;
    template <bool INSUP = false, class R> static __device__ __forceinline__ R dwq(R, int = 0) { return R(0); }
    template <bool INSUP = false, class R> static __device__ __forceinline__ R w(R q, int = 0)
    {
        // the branches q <= 2, q <= 1 of kernels.py:1120-1140 as max(., 0): a term beyond its knot is exactly zero,
        // so the value is the reference's bit for bit, without two compare-and-select pairs
        R t3 = R(3) - q, t2 = raw_max(R(2) - q, R(0)), t1 = raw_max(R(1) - q, R(0));
        R v = t3 * t3 * t3 * t3 * t3;
        v -= R(6) * t2 * t2 * t2 * t2 * t2;
        v += R(15) * t1 * t1 * t1 * t1 * t1;
        return (!INSUP && q > R(3)) ? R(0) : v;
    }
    template <bool INSUP = false, class R> static __device__ __forceinline__ R dw(R q, int = 0)
    {
        // No fma contraction here: towards q = 0 the three terms cancel (-405 + 480 - 75) and the result is the
        // rounding of the products; with the reference's own roundings (kernels.py:1137-1151) it is the reference's
        // value bit for bit, like w above (tests/test_edac_pair_edges.py, a partner at 2^-39)
#pragma clang fp contract(off)
        R t3 = R(3) - q, t2 = raw_max(R(2) - q, R(0)), t1 = raw_max(R(1) - q, R(0));
        R v = R(-5) * t3 * t3 * t3 * t3;
        v += R(30) * t2 * t2 * t2 * t2;
        v -= R(75) * t1 * t1 * t1 * t1;
        return (!INSUP && q > R(3)) ? R(0) : v;
    }
};

// The Gaussian is CUT OFF at q = 3 where it is still 1.2e-4 of its peak, so the
// support test is kept even when the caller guarantees the neighbour criterion:
// a pair at r = 3h to within rounding must give exactly 0 like the reference
// (the polynomial kernels vanish at their support radius, there INSUP is safe).
template <> struct SphKernel<4> { // Gaussian
    static constexpr bool HAS_DWQ = true; // dw/q = -2 exp(-q^2)
    static constexpr bool GRADH_FLIPPED = false;
    static constexpr bool CUTOFF = true;  // not zero at q = 3: exact q, support test kept (sph_pair.h pair_geom)
    template <bool INSUP = false, class R> static __device__ __forceinline__ R dwq(R q, int = 0) { return (q < R(3)) ? R(-2) * exp(-q * q) : R(0); }
    template <bool INSUP = false, class R> static __device__ __forceinline__ R w(R q, int = 0) { return (q < R(3)) ? exp(-q * q) : R(0); }
    template <bool INSUP = false, class R> static __device__ __forceinline__ R dw(R q, int = 0)
    {
        return (q < R(3)) ? R(-2) * q * exp(-q * q) : R(0);
    }
};

// ---------------------------------------------------------------------------
// The Wendland family beyond C2 (kernels.py: C2_1D :166-272, C4_1D :383-491, C4 :493-604, C6_1D :606-717,
// C6 :719-828).  All are t^n poly(q) with t = 1 - q/2, and dW/dq = -c q t^(n-1) poly'(q): t is an exact zero at q == 2,
// so q <= 2 gives the reference's q < 2 bit for bit and INSUP drops the test (as for SphKernel<2>); dw / q has no
// division.  Powers of t by squaring.
// ---------------------------------------------------------------------------
template <> struct SphKernel<5> { // WendlandQuinticC2_1D: t^3 (1.5 q + 1)
    static constexpr bool HAS_DWQ = true, CUTOFF = false, GRADH_FLIPPED = false; // dw/q = -3 t^2
    template <bool INSUP = false, class R> static __device__ __forceinline__ R dwq(R q, int = 0)
    {
        R t = R(1) - R(0.5) * q;
        return (INSUP || q <= R(2)) ? R(-3) * t * t : R(0);
    }
    template <bool INSUP = false, class R> static __device__ __forceinline__ R w(R q, int = 0)
    {
        R t = R(1) - R(0.5) * q;
        R v = t * t * t * (R(1.5) * q + R(1));
        return (INSUP || q <= R(2)) ? v : R(0);
    }
    template <bool INSUP = false, class R> static __device__ __forceinline__ R dw(R q, int = 0)
    {
        R t = R(1) - R(0.5) * q;
        R v = R(-3) * q * t * t;
        return (INSUP || q <= R(2)) ? v : R(0);
    }
};

template <> struct SphKernel<6> { // WendlandQuinticC4 (2-D, 3-D): t^6 (35/12 q^2 + 3 q + 1)
    static constexpr bool HAS_DWQ = true, CUTOFF = false, GRADH_FLIPPED = false; // dw/q = -14/3 (1 + 2.5 q) t^5
    template <bool INSUP = false, class R> static __device__ __forceinline__ R dwq(R q, int = 0)
    {
        R t = R(1) - R(0.5) * q, t2 = t * t;
        R v = R(-14.0 / 3.0) * (R(1) + R(2.5) * q) * (t2 * t2 * t);
        return (INSUP || q <= R(2)) ? v : R(0);
    }
    template <bool INSUP = false, class R> static __device__ __forceinline__ R w(R q, int = 0)
    {
        R t = R(1) - R(0.5) * q, t2 = t * t;
        R v = (t2 * t2 * t2) * ((R(35.0 / 12.0) * q + R(3)) * q + R(1));
        return (INSUP || q <= R(2)) ? v : R(0);
    }
    template <bool INSUP = false, class R> static __device__ __forceinline__ R dw(R q, int = 0)
    {
        R t = R(1) - R(0.5) * q, t2 = t * t;
        R v = R(-14.0 / 3.0) * q * (R(1) + R(2.5) * q) * (t2 * t2 * t);
        return (INSUP || q <= R(2)) ? v : R(0);
    }
};

template <> struct SphKernel<7> { // WendlandQuinticC4_1D: t^5 (2 q^2 + 2.5 q + 1)
    static constexpr bool HAS_DWQ = true, CUTOFF = false, GRADH_FLIPPED = false; // dw/q = -3.5 (2 q + 1) t^4
    template <bool INSUP = false, class R> static __device__ __forceinline__ R dwq(R q, int = 0)
    {
        R t = R(1) - R(0.5) * q, t2 = t * t;
        R v = R(-3.5) * (R(2) * q + R(1)) * (t2 * t2);
        return (INSUP || q <= R(2)) ? v : R(0);
    }
    template <bool INSUP = false, class R> static __device__ __forceinline__ R w(R q, int = 0)
    {
        R t = R(1) - R(0.5) * q, t2 = t * t;
        R v = (t2 * t2 * t) * ((R(2) * q + R(2.5)) * q + R(1));
        return (INSUP || q <= R(2)) ? v : R(0);
    }
    template <bool INSUP = false, class R> static __device__ __forceinline__ R dw(R q, int = 0)
    {
        R t = R(1) - R(0.5) * q, t2 = t * t;
        R v = R(-3.5) * q * (R(2) * q + R(1)) * (t2 * t2);
        return (INSUP || q <= R(2)) ? v : R(0);
    }
};

template <> struct SphKernel<8> { // WendlandQuinticC6 (2-D, 3-D): t^8 (4 q^3 + 6.25 q^2 + 4 q + 1)
    static constexpr bool HAS_DWQ = true, CUTOFF = false, GRADH_FLIPPED = false; // dw/q = -5.5 t^7 (1 + 3.5 q + 4 q^2)
    template <bool INSUP = false, class R> static __device__ __forceinline__ R dwq(R q, int = 0)
    {
        R t = R(1) - R(0.5) * q, t2 = t * t, t4 = t2 * t2;
        R v = R(-5.5) * (t4 * t2 * t) * ((R(4) * q + R(3.5)) * q + R(1));
        return (INSUP || q <= R(2)) ? v : R(0);
    }
    template <bool INSUP = false, class R> static __device__ __forceinline__ R w(R q, int = 0)
    {
        R t = R(1) - R(0.5) * q, t2 = t * t, t4 = t2 * t2;
        R v = (t4 * t4) * (((R(4) * q + R(6.25)) * q + R(4)) * q + R(1));
        return (INSUP || q <= R(2)) ? v : R(0);
    }
    template <bool INSUP = false, class R> static __device__ __forceinline__ R dw(R q, int = 0)
    {
        R t = R(1) - R(0.5) * q, t2 = t * t, t4 = t2 * t2;
        R v = R(-5.5) * q * (t4 * t2 * t) * ((R(4) * q + R(3.5)) * q + R(1));
        return (INSUP || q <= R(2)) ? v : R(0);
    }
};

template <> struct SphKernel<9> { // WendlandQuinticC6_1D: t^7 (2.625 q^3 + 4.75 q^2 + 3.5 q + 1)
    static constexpr bool HAS_DWQ = true, CUTOFF = false, GRADH_FLIPPED = false; // dw/q = -0.5 (26.25 q^2 + 27 q + 9) t^6
    template <bool INSUP = false, class R> static __device__ __forceinline__ R dwq(R q, int = 0)
    {
        R t = R(1) - R(0.5) * q, t2 = t * t;
        R v = R(-0.5) * ((R(26.25) * q + R(27)) * q + R(9)) * (t2 * t2 * t2);
        return (INSUP || q <= R(2)) ? v : R(0);
    }
    template <bool INSUP = false, class R> static __device__ __forceinline__ R w(R q, int = 0)
    {
        R t = R(1) - R(0.5) * q, t2 = t * t, t4 = t2 * t2;
        R v = (t4 * t2 * t) * (((R(2.625) * q + R(4.75)) * q + R(3.5)) * q + R(1));
        return (INSUP || q <= R(2)) ? v : R(0);
    }
    template <bool INSUP = false, class R> static __device__ __forceinline__ R dw(R q, int = 0)
    {
        R t = R(1) - R(0.5) * q, t2 = t * t;
        R v = R(-0.5) * q * ((R(26.25) * q + R(27)) * q + R(9)) * (t2 * t2 * t2);
        return (INSUP || q <= R(2)) ? v : R(0);
    }
};

// SuperGaussian (kernels.py:944-1048): exp(-q^2) (1 + dim/2 - q^2), negative beyond q^2 = 1 + dim/2 and cut off at
// q = 3 where it is -9e-4 of its peak: like the Gaussian it keeps its support test under INSUP and takes the exact q.
// Its gradient_h (:1027-1047) is a closed form of its own, (-d^2/2 + 2 d q^2 - d - 2 q^4 + 4 q^2) exp(-q^2) times
// -fac h1 -- which is +fac h1 (dw q + w d), the NEGATIVE of dW/dh and of what every other class returns.  GHIJ / GHI /
// GHJ of a reference script carry that sign, so pair_gradh reproduces it.
template <> struct SphKernel<10> {
    static constexpr bool GRADH_FLIPPED = true;
    static constexpr bool HAS_DWQ = true, CUTOFF = true; // dw/q = (2 q^2 - dim - 4) exp(-q^2)
    template <bool INSUP = false, class R> static __device__ __forceinline__ R dwq(R q, int dim)
    {
        R q2 = q * q;
        return (q < R(3)) ? (R(2) * q2 - R(dim + 4)) * exp(-q2) : R(0);
    }
    template <bool INSUP = false, class R> static __device__ __forceinline__ R w(R q, int dim)
    {
        R q2 = q * q;
        return (q < R(3)) ? exp(-q2) * (R(1) + R(0.5) * R(dim) - q2) : R(0);
    }
    template <bool INSUP = false, class R> static __device__ __forceinline__ R dw(R q, int dim)
    {
        R q2 = q * q;
        return (q < R(3)) ? q * (R(2) * q2 - R(dim + 4)) * exp(-q2) : R(0);
    }
};
