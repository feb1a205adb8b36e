// sph_records.h -- the contract between the record packer (k_pack, sph_pack.h), the host planner (sph_pack_plan.h) and the
// families' record loaders: the layouts of a packed record and the slots k_pack derives, each named once, with one
// constexpr trait per layout fact that both sides read.  Plain C++, usable on host and device.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SPH_HD __host__ __device__
#else
#define SPH_HD
#endif

#define MAX_AUX 24
#define PACK_MAXP ((4 + MAX_AUX) / 2) // 16-B pieces of the widest record

// PackArgs::layout: how k_pack lays one particle out.  x y z are the position, h the smoothing length, the other names
// the aux slots of the family's PackPlan; `|` separates 16-B pieces; x-x0: relative to PackArgs::gmin (fp32 records).
// (PL_WCSPH, PL_DENSITY, PL_TVF: aggregated kernel only)
enum PackLayoutId : int {
    PL_PLAIN = 0,          // [x y z h | aux...], nr doubles
    PL_WCSPH = 1,          // WCSPH [x y | z cs | u v | w m | rho tmpj] (+ [h p]: variable h / tensile correction)
    PL_DENSITY = 2,        // density, uniform h [x y | z m]
    PL_TVF = 3,            // TVF, uniform h [x y | z rho | u v | w p | Vj2 what | uhat vhat] (+ [m -]: artificial viscosity)
    PL_GEN_UH = 4,         // generated families, uniform h [x y z | aux...] (h is a launch constant)
    PL_F32 = 5,            // fp32 records of any family [x-x0 y-y0 z-z0 h | aux...], nr floats (option record_f32)
    PL_WCSPH_EOS = 6,      // WCSPH, p and cs recomputed by the pair kernel [x y | z u | v w | rho m] (64 B); with
                           // PackArgs::umass the last slot carries p / rho^2 instead of m
    PL_WCSPH_EOS_F32 = 7,  // the same in fp32 [x-x0 y-y0 z-z0 u | v w rho m] (32 B)
    PL_TVF_STATE = 8,      // TVF, p and V recomputed from rho [x y | z rho | u v | w uhat | vhat what] (80 B; 64 B without
                           // the artificial stress)
    PL_TVF_STATE_F32 = 9,  // the same in fp32 [x-x0 y-y0 z-z0 rho | u v w uhat | vhat what - -] (48 B / 32 B)
    PL_ELASTIC_U = 10,     // elastic rates without h and m [x y | z u | v w | rho cs | t x6 | r x6] (160 B)
    PL_ELASTIC_U_F32 = 11, // the same in fp32 [x-x0 y-y0 z-z0 u | v w rho cs | t t t t | t t r r | r r r r] (80 B)
    PL_WCSPH_EOSV = 12,    // WCSPH with variable h, one mass per array, EOS recomputed [x y | z h | u v | w rho] (64 B)
    PL_WCSPH_EOSV_F32 = 13, // the same in fp32 [x-x0 y-y0 z-z0 h | u v w rho] (32 B)
    PL_COUNT
};

// PackArgs::derived: what k_pack computes from the slots it has read (aux[k] = slot k of the PackPlan)
enum PackDerived : int {
    PD_NONE = 0,
    PD_P_RHO2 = 1,      // aux[5] = p / rho^2 (p = aux[7], rho = aux[4])
    PD_VJ2 = 2,         // aux[10] = 1 / V^2 (V = aux[8])
    PD_SIGMA_RHO2 = 3,  // aux[6..11] = (s_ij - p delta_ij) / rho^2 (p = aux[18], rho = aux[4])
    PD_M_RHO_VGRAD = 4, // aux[3] = m / rho (m = aux[3], rho = aux[4]; aux[4] itself is not stored): VelocityGradient
    PD_ORIG_INDEX = 5,  // aux[0] = the particle's original index (neighbour lists)
    PD_GSPH_SYM = 6,    // aux[15..20] = ux, uy+vx, uz+wx, vy, vz+wy, wz from the nine velocity gradients aux[15..23]
                        // (GSPHAcceleration reads them through eij . G . eij only)
    PD_M_RHO_GGRAD = 7, // aux[4] = m / rho (m = aux[4], rho = aux[5]; aux[5] itself is not stored): GSPHGradients
    PD_COUNT
};

// One row per layout:
//   PER      values in a 16-B piece: two doubles or four floats
//   PIECES   16-B pieces of a record, or 0: from PackArgs::nr
//   NV       aux slots k_pack reads at most (slots 0 .. NV-1; beyond PackArgs::na only what pack_reads_slot names)
//   COMPILED the library holds k_pack<layout>; the others run k_pack<-1> with PackArgs::layout read at run time
//   F32      the layout of the same records under fp32 arithmetic (itself: the layout is an fp32 one)
#define PACK_LAYOUT_TABLE(X)                                              \
    /* layout            PER PIECES NV       COMPILED F32 */              \
    X(PL_PLAIN,          2,  0,     MAX_AUX, false,   PL_F32)             \
    X(PL_WCSPH,          2,  0,     MAX_AUX, false,   PL_F32)             \
    X(PL_DENSITY,        2,  2,     1,       true,    PL_F32)             \
    X(PL_TVF,            2,  0,     11,      true,    PL_F32)             \
    X(PL_GEN_UH,         2,  0,     MAX_AUX, false,   PL_F32)             \
    X(PL_F32,            4,  0,     MAX_AUX, false,   PL_F32)             \
    X(PL_WCSPH_EOS,      2,  4,     8,       true,    PL_WCSPH_EOS_F32)   \
    X(PL_WCSPH_EOS_F32,  4,  2,     8,       true,    PL_WCSPH_EOS_F32)   \
    X(PL_TVF_STATE,      2,  0,     11,      true,    PL_TVF_STATE_F32)   \
    X(PL_TVF_STATE_F32,  4,  0,     11,      true,    PL_TVF_STATE_F32)   \
    X(PL_ELASTIC_U,      2,  10,    MAX_AUX, true,    PL_ELASTIC_U_F32)   \
    X(PL_ELASTIC_U_F32,  4,  5,     MAX_AUX, true,    PL_ELASTIC_U_F32)   \
    X(PL_WCSPH_EOSV,     2,  4,     8,       true,    PL_WCSPH_EOSV_F32)  \
    X(PL_WCSPH_EOSV_F32, 4,  2,     8,       true,    PL_WCSPH_EOSV_F32)

struct PackLayoutTraits {
    int per, pieces, nv;
    bool compiled;
    int f32;
};
// (layout -1, k_pack's "read PackArgs::layout at run time", has the traits of the widest record)
SPH_HD constexpr PackLayoutTraits pack_traits(int layout)
{
    switch (layout) {
#define X(ID, PER, PIECES, NV, COMPILED, F32) case ID: return PackLayoutTraits{PER, PIECES, NV, COMPILED, F32};
        PACK_LAYOUT_TABLE(X)
#undef X
    default: return PackLayoutTraits{2, 0, MAX_AUX, false, PL_F32};
    }
}

// does k_pack read aux slot k of a plan with `na` slots?  Beyond na: the inputs of the derived slots
SPH_HD constexpr bool pack_reads_slot(int derived, int na, int k)
{
    return k < na || (derived == PD_SIGMA_RHO2 && k == 18) || (derived == PD_M_RHO_VGRAD && k == 4) || (derived == PD_GSPH_SYM && k < 24) ||
           (derived == PD_M_RHO_GGRAD && k == 5);
}

#define X(ID, PER, PIECES, NV, COMPILED, F32)                                                                  \
    static_assert((PER) == 2 || (PER) == 4, "a 16-B piece holds two doubles or four floats");                  \
    static_assert((PIECES) <= PACK_MAXP, "PACK_MAXP is the piece count of the widest record");                 \
    static_assert((NV) >= 1 && (NV) <= MAX_AUX, "NV counts aux slots");                                         \
    static_assert(pack_traits(F32).per == 4 && pack_traits(F32).f32 == (F32), "the fp32 form is an fp32 layout"); \
    static_assert(((PER) == 4) == ((F32) == (ID)), "an fp32 layout is its own fp32 form");
PACK_LAYOUT_TABLE(X)
#undef X
#define X(...) +1
static_assert(0 PACK_LAYOUT_TABLE(X) == PL_COUNT, "one row per layout");
#undef X
static_assert(PL_COUNT == 14 && PD_COUNT == 8, "PackArgs::layout / derived keep their numeric values");
