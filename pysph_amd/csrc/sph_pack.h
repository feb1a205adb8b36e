// sph_pack.h -- the record packer of the pair loop: particle properties gathered into cell order as packed records.
// Part of the sph_eval.hip translation units (included there, not compiled on its own).  The host side that fills
// PackArgs (pack_plan, pack_layout, launch_pack, pack_array) is sph_pack_plan.h.
// Included after the family headers: the record sizes k_pack names are those the families' loaders export.
#include "sph_records.h"

struct PackArgs {
    const uint32_t *perm;
    size_t n;
    size_t off;
    const double *x, *y, *z, *h;
    int na;                       // doubles in the aux record
    const double *src[MAX_AUX];   // nullptr -> 0.0
    int derived;                  // a PackDerived (sph_records.h)
    double4 *posh;
    double *aux;
    double *rec;                  // non-null: interleaved records [x y z h aux... pad], nr doubles each
    int nr;
    int layout;                   // a PackLayoutId (sph_records.h)
    int umass;                    // PL_WCSPH_EOS(_F32): the last slot carries p / rho^2 (PD_P_RHO2) instead of m
    float4 *fpos;                 // non-null: fp32 {x-xmin, y-ymin, z-zmin, radius_scale*h} for the prefilter tiles
    int lds_np;                   // 16-B pieces per record when the launch carries 256 * lds_np * 16 B of LDS, else 0
    double gmin[3];
    double radius_scale;
    double hu;                    // h == nullptr: the one h of every particle (uniform h, PL_WCSPH_EOS(_F32): the record holds none)
    int eos_abs;                  // PL_WCSPH_EOS* / PL_WCSPH_EOSV*: the Tait EOS of the group before has NOT run (sph_group.src_eos = 3):
                                  // p and cs are computed here from the rho just loaded, stored, and p / rho^2 formed from that p
    double eos_par[4];            // rho0 c0 gamma p0
    double *p_out, *cs_out;
};

// Store one record of `np` 16-B pieces per lane.  The 64 records of a wavefront are contiguous in
// the packed buffer: a whole block transposes them through (dynamic) LDS so that each store
// instruction writes 1 KiB of whole lines instead of 64 pieces a record apart (k_pack 0.29 -> 0.22 ms
// on the 4 M cube); the ragged last block, and launches without LDS, store per lane.
template <class PA>
__device__ __forceinline__ void emit_pieces(const PA &a, size_t i, const double2 (&pc)[PACK_MAXP], int np)
{
    extern __shared__ __attribute__((aligned(16))) double2 pack_lds[];
    double2 *const base = reinterpret_cast<double2 *>(a.rec);
    if (a.lds_np == np && ((size_t)blockIdx.x + 1) * 256 <= a.n) {
        const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
        double2 *const sw = pack_lds + (size_t)w * 64 * np;
#pragma unroll
        for (int q = 0; q < PACK_MAXP; q++)
            if (q < np) sw[l * np + q] = pc[q];
        // private to the wavefront: program order is execution order, the fence is for the compiler
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        double2 *const ow = base + (a.off + (size_t)blockIdx.x * 256 + (size_t)w * 64) * np;
#pragma unroll
        for (int q = 0; q < PACK_MAXP; q++)
            if (q < np) ow[q * 64 + l] = sw[q * 64 + l];
    } else {
        double2 *const r2 = base + (a.off + i) * np;
#pragma unroll
        for (int q = 0; q < PACK_MAXP; q++)
            if (q < np) r2[q] = pc[q];
    }
}

// LAYOUT >= 0: the record layout as a compile-time constant (the hot layouts of the hand-written families: the layout
// switch folds away, the piece count is a constant, and the record never passes through a dynamically indexed local array
// -- the one-kernel-for-all form kept 32 B per lane in scratch); -1: PackArgs::layout at run time (every other layout).
template <int LAYOUT>
__global__ __launch_bounds__(256) void k_pack(PackArgs a)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    uint32_t o = a.perm[i];
    const int layout = LAYOUT >= 0 ? LAYOUT : a.layout;
    double4 ph;
    ph.x = a.x[o]; ph.y = a.y[o]; ph.z = a.z[o]; ph.w = a.h ? a.h[o] : a.hu;
    double v[MAX_AUX];
    // (compile-time layouts read the slots their record holds: WCSPH u v w m rho tmpj cs p = 0..7, elastic 0..17 + p)
    constexpr int NV = pack_traits(LAYOUT).nv;
#pragma unroll
    for (int k = 0; k < MAX_AUX; k++) v[k] = (k < NV && pack_reads_slot(a.derived, a.na, k) && a.src[k]) ? a.src[k][o] : 0.0;
    if constexpr (LAYOUT == PL_WCSPH_EOS || LAYOUT == PL_WCSPH_EOS_F32 || LAYOUT == PL_WCSPH_EOSV || LAYOUT == PL_WCSPH_EOSV_F32) {
        if (a.eos_abs) { // the Tait EOS of this particle, as k_nosrc would have left it (p is not read: a.src[7] is null)
            double p, cs;
            tait_eos(v[4], a.eos_par[0], a.eos_par[1], a.eos_par[2], a.eos_par[3], p, cs);
            a.p_out[o] = p;
            a.cs_out[o] = cs;
            v[7] = p;
        }
    }
    if (a.derived == PD_P_RHO2) v[5] = v[4] != 0.0 ? v[7] * (1.0 / (v[4] * v[4])) : 0.0; // tmpj = p*rhoj21, wc/basic.py:211,234
    if (a.derived == PD_VJ2) { double Vj = 1. / v[8]; v[10] = Vj * Vj; } // Vj2, transport_velocity.py:303-306
    if (a.derived == PD_M_RHO_VGRAD) v[3] = v[3] / v[4]; // m/rho, basic_equations.py:103,139 (VelocityGradient tmp)
    if (a.derived == PD_ORIG_INDEX) v[0] = (double)o;
    if (a.derived == PD_M_RHO_GGRAD) { v[4] = v[4] / v[5]; v[5] = 0.0; } // m/rho, gsph.py:81,86 (GSPHGradients)
    if (a.derived == PD_GSPH_SYM) { // gsph.py:269-284: the symmetric sums of the velocity gradient
        const double uy = v[16], uz = v[17], vx = v[18], vy = v[19], vz = v[20], wx = v[21], wy = v[22], wz = v[23];
        v[16] = uy + vx; v[17] = uz + wx; v[18] = vy; v[19] = vz + wy; v[20] = wz;
        v[21] = v[22] = v[23] = 0.0;
    }
    if (a.derived == PD_SIGMA_RHO2) { // (sigma_ij)/rho^2 with sigma = s - p I: solid_mech/basic.py:281-283,333-339,367-378
        const double r21 = 1. / (v[4] * v[4]), pr = v[18];
        v[6] = (v[6] - pr) * r21; v[7] *= r21; v[8] *= r21;
        v[9] = (v[9] - pr) * r21; v[10] *= r21; v[11] = (v[11] - pr) * r21;
        v[18] = 0.0;
    }
    if (a.fpos)
        a.fpos[a.off + i] = make_float4((float)(ph.x - a.gmin[0]), (float)(ph.y - a.gmin[1]), (float)(ph.z - a.gmin[2]),
                                        (float)(a.radius_scale * ph.w));
    if (a.rec) {
        // the record as 16-B pieces, then ONE way out (emit_pieces): the records of a wavefront
        // are contiguous, so they leave transposed through LDS as whole lines
        double2 pc[PACK_MAXP];
#pragma unroll
        for (int q = 0; q < PACK_MAXP; q++) pc[q] = make_double2(0.0, 0.0);
        int np;
        // the highest aux slot each branch below stores or derives from lies below its layout's NV
#define PACK_USES_SLOT(ID, K) static_assert(pack_traits(ID).nv > (K), #ID ": k_pack uses an aux slot it does not read")
        PACK_USES_SLOT(PL_WCSPH_EOS, 7); PACK_USES_SLOT(PL_WCSPH_EOS_F32, 7); PACK_USES_SLOT(PL_TVF_STATE, 6); PACK_USES_SLOT(PL_TVF_STATE_F32, 6);
        PACK_USES_SLOT(PL_WCSPH_EOSV, 4); PACK_USES_SLOT(PL_WCSPH_EOSV_F32, 4); PACK_USES_SLOT(PL_ELASTIC_U, 18); PACK_USES_SLOT(PL_ELASTIC_U_F32, 18);
        PACK_USES_SLOT(PL_WCSPH, 7); PACK_USES_SLOT(PL_F32, MAX_AUX - 1); PACK_USES_SLOT(PL_GEN_UH, MAX_AUX - 1); PACK_USES_SLOT(PL_TVF, 10);
        PACK_USES_SLOT(PL_DENSITY, 0); PACK_USES_SLOT(PL_PLAIN, MAX_AUX - 1);
#undef PACK_USES_SLOT
        if (layout == PL_WCSPH_EOS) { // WCSPH with the EOS fused into the pair kernel: one 64-B half line per record
            pc[0] = make_double2(ph.x, ph.y); pc[1] = make_double2(ph.z, v[0]);
            pc[2] = make_double2(v[1], v[2]); pc[3] = make_double2(v[4], a.umass ? v[5] : v[3]); // [rho m], uniform mass: [rho p/rho^2]
            np = pack_traits(PL_WCSPH_EOS).pieces;
        } else if (layout == PL_WCSPH_EOS_F32) {
            pc[0] = __builtin_bit_cast(double2, make_float4((float)(ph.x - a.gmin[0]), (float)(ph.y - a.gmin[1]),
                                                            (float)(ph.z - a.gmin[2]), (float)v[0]));
            pc[1] = __builtin_bit_cast(double2, make_float4((float)v[1], (float)v[2], (float)v[4], (float)(a.umass ? v[5] : v[3])));
            np = pack_traits(PL_WCSPH_EOS_F32).pieces;
        } else if (layout == PL_TVF_STATE) { // TVF with the state equation fused: [x y | z rho | u v | w uhat | vhat what] (no artificial stress: 4 pieces)
            pc[0] = make_double2(ph.x, ph.y); pc[1] = make_double2(ph.z, v[6]);
            pc[2] = make_double2(v[0], v[1]); pc[3] = make_double2(v[2], v[3]);
            pc[4] = make_double2(v[4], v[5]);
            np = a.nr / pack_traits(PL_TVF_STATE).per;
        } else if (layout == PL_TVF_STATE_F32) { // the same in fp32: [x-x0 y-y0 z-z0 rho | u v w uhat | vhat what - -]
            pc[0] = __builtin_bit_cast(double2, make_float4((float)(ph.x - a.gmin[0]), (float)(ph.y - a.gmin[1]),
                                                            (float)(ph.z - a.gmin[2]), (float)v[6]));
            pc[1] = __builtin_bit_cast(double2, make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]));
            pc[2] = __builtin_bit_cast(double2, make_float4((float)v[4], (float)v[5], 0.f, 0.f));
            np = a.nr / pack_traits(PL_TVF_STATE_F32).per;
        } else if (layout == PL_WCSPH_EOSV) { // WCSPH, variable h, one mass, EOS recomputed: [x y | z h | u v | w rho]
            pc[0] = make_double2(ph.x, ph.y); pc[1] = make_double2(ph.z, ph.w);
            pc[2] = make_double2(v[0], v[1]); pc[3] = make_double2(v[2], v[4]);
            np = pack_traits(PL_WCSPH_EOSV).pieces;
        } else if (layout == PL_WCSPH_EOSV_F32) { // the same in fp32: [x y z h | u v w rho]
            pc[0] = __builtin_bit_cast(double2, make_float4((float)(ph.x - a.gmin[0]), (float)(ph.y - a.gmin[1]),
                                                            (float)(ph.z - a.gmin[2]), (float)ph.w));
            pc[1] = __builtin_bit_cast(double2, make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[4]));
            np = pack_traits(PL_WCSPH_EOSV_F32).pieces;
        } else if (layout == PL_ELASTIC_U) { // elastic, uniform h and mass: [x y | z u | v w | rho cs | t x6 | r x6]
            pc[0] = make_double2(ph.x, ph.y); pc[1] = make_double2(ph.z, v[0]);
            pc[2] = make_double2(v[1], v[2]); pc[3] = make_double2(v[4], v[5]);
#pragma unroll
            for (int q = 0; q < 6; q++) pc[4 + q] = make_double2(v[6 + 2 * q], v[7 + 2 * q]);
            np = pack_traits(PL_ELASTIC_U).pieces;
        } else if (layout == PL_ELASTIC_U_F32) { // the same in fp32: [x y z u | v w rho cs | t t t t | t t r r | r r r r]
            pc[0] = __builtin_bit_cast(double2, make_float4((float)(ph.x - a.gmin[0]), (float)(ph.y - a.gmin[1]),
                                                            (float)(ph.z - a.gmin[2]), (float)v[0]));
            pc[1] = __builtin_bit_cast(double2, make_float4((float)v[1], (float)v[2], (float)v[4], (float)v[5]));
#pragma unroll
            for (int q = 0; q < 3; q++)
                pc[2 + q] = __builtin_bit_cast(double2, make_float4((float)v[6 + 4 * q], (float)v[7 + 4 * q], (float)v[8 + 4 * q], (float)v[9 + 4 * q]));
            np = pack_traits(PL_ELASTIC_U_F32).pieces;
        } else if (layout == PL_WCSPH) { // WCSPH [x y | z cs | u v | w m | rho tmpj] (+ [h p]: variable h / tensile correction)
            pc[0] = make_double2(ph.x, ph.y); pc[1] = make_double2(ph.z, v[6]);
            pc[2] = make_double2(v[0], v[1]); pc[3] = make_double2(v[2], v[3]);
            pc[4] = make_double2(v[4], v[5]); pc[5] = make_double2(ph.w, v[7]);
            np = a.nr / pack_traits(PL_WCSPH).per;
        } else if (layout == PL_F32) { // fp32 records [x-x0 y-y0 z-z0 h | aux...] (option record_f32), a.nr floats
            float w[4 + MAX_AUX];
            w[0] = (float)(ph.x - a.gmin[0]); w[1] = (float)(ph.y - a.gmin[1]); w[2] = (float)(ph.z - a.gmin[2]);
            w[3] = (float)ph.w;
#pragma unroll
            for (int k = 0; k < MAX_AUX; k++) w[4 + k] = k < a.na ? (float)v[k] : 0.f;
#pragma unroll
            for (int q = 0; q < (4 + MAX_AUX) / 4; q++)
                pc[q] = __builtin_bit_cast(double2, make_float4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]));
            np = a.nr / pack_traits(PL_F32).per;
        } else if (layout == PL_GEN_UH) { // generated families under uniform h: [x y z | aux...] (h is a launch constant)
            double w[3 + MAX_AUX + 1];
            w[0] = ph.x; w[1] = ph.y; w[2] = ph.z;
#pragma unroll
            for (int k = 0; k < MAX_AUX + 1; k++) w[3 + k] = k < a.na ? v[k < MAX_AUX ? k : 0] : 0.0;
#pragma unroll
            for (int q = 0; q < (3 + MAX_AUX + 1) / 2; q++) pc[q] = make_double2(w[2 * q], w[2 * q + 1]);
            np = (a.nr + 1) / pack_traits(PL_GEN_UH).per;
        } else if (layout == PL_TVF) { // TVF under uniform h: [x y | z rho | u v | w p | Vj2 what | uhat vhat] (+ [m -] with artificial viscosity)
            pc[0] = make_double2(ph.x, ph.y); pc[1] = make_double2(ph.z, v[6]);
            pc[2] = make_double2(v[0], v[1]); pc[3] = make_double2(v[2], v[7]);
            pc[4] = make_double2(v[10], v[5]); pc[5] = make_double2(v[3], v[4]);
            pc[6] = make_double2(v[9], 0.0);
            np = (a.nr > FamTVF::NR_COMPACT ? FamTVF::NR_COMPACT_M : FamTVF::NR_COMPACT) / pack_traits(PL_TVF).per;
        } else if (layout == PL_DENSITY) { // compact density records [x y z m] (uniform h)
            pc[0] = make_double2(ph.x, ph.y); pc[1] = make_double2(ph.z, v[0]);
            np = pack_traits(PL_DENSITY).pieces;
        } else { // [x y z h | aux...]
            pc[0] = make_double2(ph.x, ph.y); pc[1] = make_double2(ph.z, ph.w);
#pragma unroll
            for (int q = 0; q < MAX_AUX / 2; q++) pc[2 + q] = make_double2(v[2 * q], v[2 * q + 1]);
            np = a.nr / pack_traits(PL_PLAIN).per;
        }
        emit_pieces(a, i, pc, np);
    } else {
        a.posh[a.off + i] = ph;
        double *dst = a.aux + (a.off + i) * (size_t)a.na;
#pragma unroll
        for (int k = 0; k < MAX_AUX; k++) if (k < a.na) dst[k] = v[k];
    }
}

// Records of the MERGED order (FamWCSPHM_T): thread p packs the particle at merged position p -- array slot[p], original
// index perm[p] -- from ITS array's properties (pointer tables read per lane from the kernarg segment) into
// [x y | z u | v w | +-rho p/rho^2] (fp32: [x-x0 y-y0 z-z0 u | v w +-rho p/rho^2]); the sign of rho is the array's class.
// One launch for all arrays; consecutive merged positions are consecutive records, so whole blocks leave through LDS
// as full lines like k_pack's.
struct PackMArgs {
    const uint32_t *perm;
    const uint8_t *slot;
    size_t n, off;                 // off = 0 (emit_pieces)
    const double *prop[9][SPH_MAX_ARRAYS]; // x y z u v w rho p h, per slot (h: variable-h records only)
    int vh;                        // 1: variable h -- records [x y | z h | u v | w +-rho], p / rho^2 recomputed by the pair kernel
    uint32_t cls;                  // bit s: slot s is a class-1 array
    double *rec;
    float4 *fpos;
    int f32, lds_np;
    double gmin[3];
    double hr;                     // radius_scale * h (uniform h)
    uint32_t *rho_flag;            // device word: set to 1 when a density is not positive (the class bit is the SIGN of rho)
};

// (F32, VH: PackMArgs::f32 / vh as compile-time constants -- the piece count of the record is then one too)
template <bool F32, bool VH>
__global__ __launch_bounds__(256) void k_pack_merged(PackMArgs a)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t o = a.perm[i], sl = a.slot[i];
    double v[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const double *p = kernarg_read<const double *>(__builtin_offsetof(PackMArgs, prop) + ((size_t)k * SPH_MAX_ARRAYS + sl) * sizeof(double *));
        v[k] = p[o];
    }
    const double rho = v[6];
    const double q = rho != 0.0 ? v[7] * (1.0 / (rho * rho)) : 0.0; // tmpj = p*rhoj21, wc/basic.py:211,234 (as k_pack, PD_P_RHO2)
    const double srho = ((a.cls >> sl) & 1u) ? -rho : rho;
    // rho <= 0 (or NaN): this record's class bit is not to be trusted (padding rows of sph_halo_append_padded, parked far
    // outside the domain with rho = 0, are nobody's neighbour)
    if (!(rho > 0.0) && fabs(v[0]) < SPH_PARKED_MIN) atomicOr(a.rho_flag, 1u);
    double hp = 0.0;
    if (VH) hp = kernarg_read<const double *>(__builtin_offsetof(PackMArgs, prop) + ((size_t)8 * SPH_MAX_ARRAYS + sl) * sizeof(double *))[o];
    a.fpos[i] = make_float4((float)(v[0] - a.gmin[0]), (float)(v[1] - a.gmin[1]), (float)(v[2] - a.gmin[2]),
                            VH ? (float)(a.hr * hp) : (float)a.hr); // hr: radius_scale * h, or radius_scale alone with variable h
    double2 pc[PACK_MAXP];
#pragma unroll
    for (int k = 0; k < PACK_MAXP; k++) pc[k] = make_double2(0.0, 0.0);
    int np;
    if (VH && F32) {
        pc[0] = __builtin_bit_cast(double2, make_float4((float)(v[0] - a.gmin[0]), (float)(v[1] - a.gmin[1]), (float)(v[2] - a.gmin[2]), (float)hp));
        pc[1] = __builtin_bit_cast(double2, make_float4((float)v[3], (float)v[4], (float)v[5], (float)srho));
        np = 2;
    } else if (VH) {
        pc[0] = make_double2(v[0], v[1]); pc[1] = make_double2(v[2], hp);
        pc[2] = make_double2(v[3], v[4]); pc[3] = make_double2(v[5], srho);
        np = 4;
    } else if (F32) {
        pc[0] = __builtin_bit_cast(double2, make_float4((float)(v[0] - a.gmin[0]), (float)(v[1] - a.gmin[1]), (float)(v[2] - a.gmin[2]), (float)v[3]));
        pc[1] = __builtin_bit_cast(double2, make_float4((float)v[4], (float)v[5], (float)srho, (float)q));
        np = 2;
    } else {
        pc[0] = make_double2(v[0], v[1]); pc[1] = make_double2(v[2], v[3]);
        pc[2] = make_double2(v[4], v[5]); pc[3] = make_double2(srho, q);
        np = 4;
    }
    emit_pieces(a, i, pc, np);
}
