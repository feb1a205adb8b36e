// sph_eval.hip -- AccelerationEval.compute on the device.
//
// Replaces one leaf-group block of the code the reference generates from
// pysph/sph/acceleration_eval_cython.mako:10-154 (initialize -> no-source
// loops -> per-source [neighbours -> precomputed symbols -> Equation.loop] ->
// post_loop), with the destination/source regrouping of MegaGroup
// (pysph/sph/acceleration_eval.py:94-162) done here on the host.
//
// Design (gfx950, no MFMA -- an irregular gather, not a contraction):
//   * every array taking part in a (dest, sources) block is gathered into
//     cell order as packed records {x,y,z,h | equation-family aux} (+ a compact
//     fp32 position array for the prefilter) -> all pair-loop reads are
//     contiguous runs (a row of cells along x is one run, sorted along x to 1/8
//     of a cell);
//   * one fused kernel per destination does initialize + ALL sources + post_loop
//     with the sums held in registers and ONE write per output, no atomics;
//   * two schedules of the same arithmetic:
//       variant 6 (default) k_pair_wave   : one wavefront per 64 destinations,
//                                           fp32 prefilter tiles in LDS, per-lane
//                                           hit-mask slot lists (sph_pair.h),
//       variant 0           k_pair_direct : plain per-lane 27-cell walk, the
//                                           independent cross-check;
//     (schedules measured and dropped: DESIGN.md section 4);
//   * every family is a template on the arithmetic type: double (default) or
//     float (option arith_f32);
//   * the exact criterion of the reference (r2 < (k h_i)^2 or r2 < (k h_j)^2,
//     linked_list_nnps.pyx:176-184) decides neighbourhood in every schedule;
//     the fp32 test in front of it is a conservative superset filter.
#include "sph_internal.h"
#include "sph_kernels.h"
#include "sph_pair.h"

#include <cfloat>
#include <cmath>
#include <type_traits>

// 0: the primary compile (everything; pair kernels of SphKernel<1..4>).  5..10: a kernel unit -- the pair kernels of
// that one smoothing kernel behind externally linked launch functions, nothing else (see launch_pair_k below)
#ifndef SPH_KERNEL_UNIT
#define SPH_KERNEL_UNIT 0
#endif
#define SPH_PRIMARY_UNIT (SPH_KERNEL_UNIT == 0)

// TaitEOS (wc/basic.py:60-65): ONE body for k_nosrc and for the pack kernel that absorbs the equation (PackArgs::eos_abs),
// so that p and cs have the same bits whichever of the two wrote them
__device__ __forceinline__ void tait_eos(double rho, double rho0, double c0, double gamma, double p0, double &p, double &cs)
{
    double ratio = rho * (1.0 / rho0);
    double tmp, csr;
    if (tait_gk(gamma) >= 0) { // odd integer exponents (7: water): the powers by multiplication (two pow() calls made this kernel compute-bound)
        tait_powers(ratio, tait_gk(gamma), tmp, csr);
    } else {
        tmp = pow(ratio, gamma);
        csr = pow(ratio, 0.5 * (gamma - 1.0));
    }
    p = p0 + (rho0 * c0 * c0 / gamma) * (tmp - 1.0);
    cs = c0 * csr;
}

#if SPH_PRIMARY_UNIT

// ---------------------------------------------------------------------------
// equations without sources (elementwise)
// ---------------------------------------------------------------------------
struct EosArgs {
    int kind;
    double par[SPH_MAX_PAR];
    double *rho, *p, *cs;
    size_t start, stop;
    double *q[SPH_PROP_COUNT]; // every device property of the destination (elastic equations)
    uint32_t *tflag;           // MonaghanArtificialStress: set to 1 when any r_ij is non-zero (DevArray::tflag), or null
    int gcol[20];              // GSPHUpdateGhostProps: the twenty columns an image row takes from its row
};

// Symmetric 3x3 eigen-decomposition by cyclic Jacobi rotations.  The reference
// uses EISPACK tred2/tql2 (pysph/base/linalg3.pyx:259-536); what the caller
// needs is the matrix function V f(lambda) V^T, which does not depend on the
// eigen-solver, its ordering or sign conventions -- only on its accuracy.
__device__ inline void jacobi_eigen3(double A[3][3], double V[3][3], double d[3])
{
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) V[i][j] = (i == j) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 12; sweep++) {
        double off = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[1][2]);
        double diag = fabs(A[0][0]) + fabs(A[1][1]) + fabs(A[2][2]);
        if (off <= 1e-300 || off <= 1e-18 * diag) break;
#pragma unroll
        for (int pq = 0; pq < 3; pq++) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            double apq = A[p][q];
            if (apq == 0.0) continue;
            double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
            double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
            A[p][p] -= t * apq;
            A[q][q] += t * apq;
            A[p][q] = A[q][p] = 0.0;
            const int r = 3 - p - q;
            double arp = A[r][p], arq = A[r][q];
            A[r][p] = A[p][r] = c * arp - s * arq;
            A[r][q] = A[q][r] = s * arp + c * arq;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                double vkp = V[k][p], vkq = V[k][q];
                V[k][p] = c * vkp - s * vkq;
                V[k][q] = s * vkp + c * vkq;
            }
        }
    }
    d[0] = A[0][0]; d[1] = A[1][1]; d[2] = A[2][2];
}

__global__ __launch_bounds__(256) void k_nosrc(EosArgs a)
{
    size_t i = a.start + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.stop) return;
    switch (a.kind) {
    case SPH_EQ_TAIT_EOS: {
        double p, cs;
        tait_eos(a.rho[i], a.par[0], a.par[1], a.par[2], a.par[3], p, cs);
        a.p[i] = p;
        a.cs[i] = cs;
        break;
    }
    case SPH_EQ_TAIT_EOS_HG: { // wc/basic.py:118-126
        double rho0 = a.par[0], c0 = a.par[1], gamma = a.par[2];
        double r = a.rho[i];
        if (r < rho0) { r = rho0; a.rho[i] = r; }
        double ratio = r * (1.0 / rho0);
        double tmp, csr;
        if (tait_gk(gamma) >= 0) { // as TaitEOS above: the EOS-fused pair kernel recomputes p, cs by the same multiplications
            tait_powers(ratio, tait_gk(gamma), tmp, csr);
        } else {
            tmp = pow(ratio, gamma);
            csr = pow(ratio, 0.5 * (gamma - 1.0));
        }
        a.p[i] = (rho0 * c0 * c0 / gamma) * (tmp - 1.0);
        a.cs[i] = c0 * csr;
        break;
    }
    case SPH_EQ_TVF_STATE_EQUATION: // transport_velocity.py:215-216; rho / rho0 as rho * (1 / rho0), like TaitEOS above: the
                                    // state-fused TVF pair kernel (FamTVFE_T) recomputes exactly this
        a.p[i] = a.par[0] * (a.rho[i] * (1.0 / a.par[1]) - a.par[2]);
        break;
    case SPH_EQ_ISOTHERMAL_EOS: // basic_equations.py:175-176
        a.p[i] = a.par[2] + (a.par[1] * a.par[1]) * (a.rho[i] - a.par[0]);
        break;
    case SPH_EQ_SOLID_ISOTHERMAL_EOS: // solid_mech/basic.py:100-101; par c0_ref rho_ref
        a.p[i] = a.par[0] * a.par[0] * (a.rho[i] - a.par[1]);
        break;
    case SPH_EQ_MONAGHAN_ART_STRESS: { // solid_mech/basic.py:170-242; par eps
        double **q = a.q;
        const double rhoi = a.rho[i], rhoi21 = 1. / (rhoi * rhoi), pr = a.p[i];
        double S[3][3], R[3][3], lam[3], rd[3];
        S[0][0] = q[SPH_S00][i] - pr; S[1][1] = q[SPH_S11][i] - pr; S[2][2] = q[SPH_S22][i] - pr;
        S[0][1] = S[1][0] = q[SPH_S01][i];
        S[0][2] = S[2][0] = q[SPH_S02][i];
        S[1][2] = S[2][1] = q[SPH_S12][i];
        // Gershgorin: every eigenvalue <= max_i (S_ii + sum_{j != i} |S_ij|).  When that bound is not positive no principal
        // stress is tensile, every rd below would be zero and R = 0: no eigen-decomposition (most particles of a body under
        // compression; an eigenvalue the reference's solver would round to +1e-17 of the stress scale is all this can miss)
        {
            const double g0 = S[0][0] + fabs(S[0][1]) + fabs(S[0][2]), g1 = S[1][1] + fabs(S[0][1]) + fabs(S[1][2]),
                         g2 = S[2][2] + fabs(S[0][2]) + fabs(S[1][2]);
            if (fmax(g0, fmax(g1, g2)) <= 0.0) {
                q[SPH_R00][i] = 0.0; q[SPH_R11][i] = 0.0; q[SPH_R22][i] = 0.0;
                q[SPH_R12][i] = 0.0; q[SPH_R02][i] = 0.0; q[SPH_R01][i] = 0.0;
                break;
            }
        }
        // same scaling as linalg3.eigen_decomposition (:520-536): tiny matrices stay accurate
        double sc = 0.0;
        for (int r = 0; r < 3; r++) for (int cc = 0; cc < 3; cc++) sc += fabs(S[r][cc]);
        if (sc == 0.0) {
            lam[0] = lam[1] = lam[2] = 0.0;
            for (int r = 0; r < 3; r++) for (int cc = 0; cc < 3; cc++) R[r][cc] = (r == cc);
        } else {
            for (int r = 0; r < 3; r++) for (int cc = 0; cc < 3; cc++) S[r][cc] /= sc;
            jacobi_eigen3(S, R, lam);
            for (int k = 0; k < 3; k++) lam[k] *= sc;
        }
        for (int k = 0; k < 3; k++) rd[k] = lam[k] > 0 ? -a.par[0] * lam[k] * rhoi21 : 0.0;
        if (a.tflag && (rd[0] != 0.0 || rd[1] != 0.0 || rd[2] != 0.0)) *a.tflag = 1u; // a particle in tension: r_ij != 0
        // transform_diag_inv: R diag(rd) R^T  (linalg3.pyx:220-234)
        double Rab[3][3];
        for (int r = 0; r < 3; r++)
            for (int cc = r; cc < 3; cc++) {
                double t = 0.0;
                for (int k = 0; k < 3; k++) t += R[r][k] * rd[k] * R[cc][k];
                Rab[r][cc] = t;
            }
        q[SPH_R00][i] = Rab[0][0]; q[SPH_R11][i] = Rab[1][1]; q[SPH_R22][i] = Rab[2][2];
        q[SPH_R12][i] = Rab[1][2]; q[SPH_R02][i] = Rab[0][2]; q[SPH_R01][i] = Rab[0][1];
        break;
    }
    case SPH_EQ_HOOKES_DEVIATORIC_STRESS_RATE: { // solid_mech/basic.py:418-505; par G
        double **q = a.q;
        const double v00 = q[SPH_V00][i], v01 = q[SPH_V01][i], v02 = q[SPH_V02][i];
        const double v10 = q[SPH_V10][i], v11 = q[SPH_V11][i], v12 = q[SPH_V12][i];
        const double v20 = q[SPH_V20][i], v21 = q[SPH_V21][i], v22 = q[SPH_V22][i];
        const double s00 = q[SPH_S00][i], s01 = q[SPH_S01][i], s02 = q[SPH_S02][i];
        const double s11 = q[SPH_S11][i], s12 = q[SPH_S12][i], s22 = q[SPH_S22][i];
        const double s10 = s01, s20 = s02, s21 = s12;
        const double eps00 = v00, eps01 = 0.5 * (v01 + v10), eps02 = 0.5 * (v02 + v20);
        const double eps11 = v11, eps12 = 0.5 * (v12 + v21), eps22 = v22;
        const double omega01 = 0.5 * (v01 - v10), omega02 = 0.5 * (v02 - v20), omega12 = 0.5 * (v12 - v21);
        const double omega10 = -omega01, omega20 = -omega02, omega21 = -omega12;
        const double tmp = 2.0 * a.par[0];
        const double trace = 1.0 / 3.0 * (eps00 + eps11 + eps22);
        q[SPH_AS00][i] = tmp * (eps00 - trace) + (s01 * omega01 + s02 * omega02) + (s10 * omega01 + s20 * omega02);
        q[SPH_AS01][i] = tmp * eps01 + (s00 * omega10 + s02 * omega12) + (s11 * omega01 + s21 * omega02);
        q[SPH_AS02][i] = tmp * eps02 + (s00 * omega20 + s01 * omega21) + (s12 * omega01 + s22 * omega02);
        q[SPH_AS11][i] = tmp * (eps11 - trace) + (s10 * omega10 + s12 * omega12) + (s01 * omega10 + s21 * omega12);
        q[SPH_AS12][i] = tmp * eps12 + (s10 * omega20 + s11 * omega21) + (s02 * omega10 + s22 * omega12);
        q[SPH_AS22][i] = tmp * (eps22 - trace) + (s20 * omega20 + s21 * omega21) + (s02 * omega20 + s12 * omega21);
        break;
    }
    case SPH_EQ_UPDATE_H_FERRARI: // wc/basic.py:459-463; par dim1 (= 1 / dim) hdx
        a.q[SPH_H][i] = a.par[1] * pow(a.q[SPH_M][i] / a.rho[i], a.par[0]);
        break;
    case SPH_EQ_IDEAL_GAS_EOS: { // gas_dynamics/basic.py:228-230; par gamma
        const double r = a.rho[i], p = (a.par[0] - 1.0) * r * a.q[SPH_E][i];
        a.p[i] = p;
        a.cs[i] = sqrt(a.par[0] * p / r);
        break;
    }
    case SPH_EQ_SCALE_SMOOTHING_LENGTH: // gas_dynamics/basic.py:18-19; par factor
        a.q[SPH_H][i] = a.q[SPH_H][i] * a.par[0];
        break;
    case SPH_EQ_UPDATE_H_FROM_VOLUME: // gas_dynamics/basic.py:28-29; par k dim1 (= 1 / dim)
        a.q[SPH_H][i] = a.par[0] * pow(a.q[SPH_M][i] / a.rho[i], a.par[1]);
        break;
    case SPH_EQ_MPM_UPDATE_GHOST_PROPS: { // gas_dynamics/basic.py:492-497; par[0] = the array's real rows, par[1] = the column of orig_idx
        const size_t n_real = (size_t)a.par[0];
        if (i < n_real) break;            // (tag == Ghost: the rows behind the real ones)
        const double oi = a.q[(int)a.par[1]][i];
        if (!(oi >= 0.0 && oi < (double)n_real)) break; // a row whose orig_idx names no real row is left alone
        const size_t idx = (size_t)oi;
        a.p[i] = a.p[idx];
        a.cs[i] = a.cs[idx];
        break;
    }
    case SPH_EQ_ADKE_UPDATE_GHOST_PROPS: { // gas_dynamics/basic.py:506-512; par as above: p, cs and rho, no more
        const size_t n_real = (size_t)a.par[0];
        if (i < n_real) break;
        const double oi = a.q[(int)a.par[1]][i];
        if (!(oi >= 0.0 && oi < (double)n_real)) break;
        const size_t idx = (size_t)oi;
        a.p[i] = a.p[idx];
        a.cs[i] = a.cs[idx];
        a.rho[i] = a.rho[idx];
        break;
    }
    case SPH_EQ_GSPH_UPDATE_GHOST_PROPS: { // gas_dynamics/gsph.py:113-145; par as above, gcol: px..wz grhox..z dwdh rho div p cs
        const size_t n_real = (size_t)a.par[0];
        if (i < n_real) break;
        const double oi = a.q[(int)a.par[1]][i];
        if (!(oi >= 0.0 && oi < (double)n_real)) break;
        const size_t idx = (size_t)oi;
#pragma unroll
        for (int k = 0; k < 20; k++) a.q[a.gcol[k]][i] = a.q[a.gcol[k]][idx];
        break;
    }
    }
}

#endif // SPH_PRIMARY_UNIT

// ---------------------------------------------------------------------------
// equation families
// ---------------------------------------------------------------------------
enum { F_VG2 = 1, F_VG3 = 2,                                            // velocity gradient
       F_ECONT = 1, F_ESTRESS = 2, F_EAV = 4, F_EXSPH = 8 };            // elastic rates
enum { F_DCONT = 16, F_DMOM = 32, F_LAM = 64, F_LAMD = 128,             // WCSPH options (next to the WCSPH flags below)
       F_MOMENT = 1, F_GRADRHO = 2, F_GCORR = 4 };                      // delta-SPH pre-passes
enum { F_CONT = 1, F_MOM = 2, F_XSPH = 4, F_TENSILE = 8,               // WCSPH
       F_SD = 1, F_TVFSD = 2,                                           // density
       F_TP = 1, F_TVISC = 2, F_TAV = 4, F_TAS = 8 };                   // TVF force

#define MAX_AUX 24
struct PackArgs {
    const uint32_t *perm;
    size_t n;
    size_t off;
    const double *x, *y, *z, *h;
    int na;                       // doubles in the aux record
    const double *src[MAX_AUX];   // nullptr -> 0.0
    int derived;                  // 1: aux[5] = p/(rho*rho) (p = aux[7], rho = aux[4]); 2: aux[10] = 1/V^2 (V = aux[8]);
                                  // 3: aux[6..11] = (s_ij - p delta_ij)/rho^2 (p = aux[18], rho = aux[4])
                                  // 4: aux[3] = m/rho (m = aux[3], rho = aux[4]; aux[4] itself is not stored)
                                  // 5: aux[0] = the particle's original index (neighbour lists)
                                  // 6: aux[15..20] = ux, uy+vx, uz+wx, vy, vz+wy, wz from the nine velocity gradients
                                  //    aux[15..23] (GSPHAcceleration reads them through eij . G . eij only)
                                  // 7: aux[4] = m/rho (m = aux[4], rho = aux[5]; aux[5] itself is not stored)
    double4 *posh;
    double *aux;
    double *rec;                  // non-null: interleaved records [x y z h aux... pad], nr doubles each
    int nr;
    int layout;                   // 0: [x y z h | aux...]; 1: WCSPH [x y z cs | u v w m | rho tmpj | h p]; 2: density [x y z m];
                                  // 3: TVF [x y z rho | u v w p | Vj2 m uhat vhat | what -];
                                  // 4: generated, uniform h [x y z | aux...]; 5: fp32 records (floats, any family)
                                  // 6: WCSPH, p and cs recomputed by the pair kernel [x y | z u | v w | rho m] (64 B);
                                  // 7: the same in fp32 [x-x0 y-y0 z-z0 u | v w rho m] (32 B)
                                  // 8 / 9: TVF, p and V recomputed from rho (fp64 80 B / fp32 48 B)
                                  // 10 / 11: elastic rates without h and m (fp64 160 B / fp32 80 B)
                                  // 12 / 13: WCSPH with variable h, one mass per array, EOS recomputed (64 B / 32 B)
                                  // (1, 2: aggregated kernel only)
    int umass;                    // layouts 6 / 7: the last slot carries p / rho^2 (derived 1) instead of m
    float4 *fpos;                 // non-null: fp32 {x-xmin, y-ymin, z-zmin, radius_scale*h} for the prefilter tiles
    int lds_np;                   // 16-B pieces per record when the launch carries 256 * lds_np * 16 B of LDS, else 0
    double gmin[3];
    double radius_scale;
    double hu;                    // h == nullptr: the one h of every particle (uniform h, layouts 6 / 7: the record holds none)
    int eos_abs;                  // layouts 6 / 7 / 12 / 13: the Tait EOS of the group before has NOT run (sph_group.src_eos = 3):
                                  // p and cs are computed here from the rho just loaded, stored, and p / rho^2 formed from that p
    double eos_par[4];            // rho0 c0 gamma p0
    double *p_out, *cs_out;
};

#define PACK_MAXP ((4 + MAX_AUX) / 2) // 16-B pieces of the widest record

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
    constexpr int NV = (LAYOUT == 6 || LAYOUT == 7 || LAYOUT == 12 || LAYOUT == 13) ? 8 : (LAYOUT == 2 ? 1 : (LAYOUT == 3 || LAYOUT == 8 || LAYOUT == 9) ? 11 : MAX_AUX);
#pragma unroll
    for (int k = 0; k < MAX_AUX; k++) v[k] = (k < NV && (k < a.na || (a.derived == 3 && k == 18) || (a.derived == 4 && k == 4) || (a.derived == 6 && k < 24) || (a.derived == 7 && k == 5)) && a.src[k]) ? a.src[k][o] : 0.0;
    if constexpr (LAYOUT == 6 || LAYOUT == 7 || LAYOUT == 12 || LAYOUT == 13) {
        if (a.eos_abs) { // the Tait EOS of this particle, as k_nosrc would have left it (p is not read: a.src[7] is null)
            double p, cs;
            tait_eos(v[4], a.eos_par[0], a.eos_par[1], a.eos_par[2], a.eos_par[3], p, cs);
            a.p_out[o] = p;
            a.cs_out[o] = cs;
            v[7] = p;
        }
    }
    if (a.derived == 1) v[5] = v[4] != 0.0 ? v[7] * (1.0 / (v[4] * v[4])) : 0.0; // tmpj = p*rhoj21, wc/basic.py:211,234
    if (a.derived == 2) { double Vj = 1. / v[8]; v[10] = Vj * Vj; } // Vj2, transport_velocity.py:303-306
    if (a.derived == 4) v[3] = v[3] / v[4]; // m/rho, basic_equations.py:103,139 (VelocityGradient tmp)
    if (a.derived == 5) v[0] = (double)o;
    if (a.derived == 7) { v[4] = v[4] / v[5]; v[5] = 0.0; } // m/rho, gsph.py:81,86 (GSPHGradients)
    if (a.derived == 6) { // gsph.py:269-284: the symmetric sums of the velocity gradient
        const double uy = v[16], uz = v[17], vx = v[18], vy = v[19], vz = v[20], wx = v[21], wy = v[22], wz = v[23];
        v[16] = uy + vx; v[17] = uz + wx; v[18] = vy; v[19] = vz + wy; v[20] = wz;
        v[21] = v[22] = v[23] = 0.0;
    }
    if (a.derived == 3) { // (sigma_ij)/rho^2 with sigma = s - p I: solid_mech/basic.py:281-283,333-339,367-378
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
        if (layout == 6) { // WCSPH with the EOS fused into the pair kernel: one 64-B half line per record
            pc[0] = make_double2(ph.x, ph.y); pc[1] = make_double2(ph.z, v[0]);
            pc[2] = make_double2(v[1], v[2]); pc[3] = make_double2(v[4], a.umass ? v[5] : v[3]); // [rho m], uniform mass: [rho p/rho^2]
            np = 4;
        } else if (layout == 7) {
            pc[0] = __builtin_bit_cast(double2, make_float4((float)(ph.x - a.gmin[0]), (float)(ph.y - a.gmin[1]),
                                                            (float)(ph.z - a.gmin[2]), (float)v[0]));
            pc[1] = __builtin_bit_cast(double2, make_float4((float)v[1], (float)v[2], (float)v[4], (float)(a.umass ? v[5] : v[3])));
            np = 2;
        } else if (layout == 8) { // TVF with the state equation fused: [x y | z rho | u v | w uhat | vhat what] (no artificial stress: 4 pieces)
            pc[0] = make_double2(ph.x, ph.y); pc[1] = make_double2(ph.z, v[6]);
            pc[2] = make_double2(v[0], v[1]); pc[3] = make_double2(v[2], v[3]);
            pc[4] = make_double2(v[4], v[5]);
            np = a.nr / 2;
        } else if (layout == 9) { // the same in fp32: [x-x0 y-y0 z-z0 rho | u v w uhat | vhat what - -]
            pc[0] = __builtin_bit_cast(double2, make_float4((float)(ph.x - a.gmin[0]), (float)(ph.y - a.gmin[1]),
                                                            (float)(ph.z - a.gmin[2]), (float)v[6]));
            pc[1] = __builtin_bit_cast(double2, make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]));
            pc[2] = __builtin_bit_cast(double2, make_float4((float)v[4], (float)v[5], 0.f, 0.f));
            np = a.nr / 4;
        } else if (layout == 12) { // WCSPH, variable h, one mass, EOS recomputed: [x y | z h | u v | w rho]
            pc[0] = make_double2(ph.x, ph.y); pc[1] = make_double2(ph.z, ph.w);
            pc[2] = make_double2(v[0], v[1]); pc[3] = make_double2(v[2], v[4]);
            np = 4;
        } else if (layout == 13) { // the same in fp32: [x y z h | u v w rho]
            pc[0] = __builtin_bit_cast(double2, make_float4((float)(ph.x - a.gmin[0]), (float)(ph.y - a.gmin[1]),
                                                            (float)(ph.z - a.gmin[2]), (float)ph.w));
            pc[1] = __builtin_bit_cast(double2, make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[4]));
            np = 2;
        } else if (layout == 10) { // elastic, uniform h and mass: [x y | z u | v w | rho cs | t x6 | r x6]
            pc[0] = make_double2(ph.x, ph.y); pc[1] = make_double2(ph.z, v[0]);
            pc[2] = make_double2(v[1], v[2]); pc[3] = make_double2(v[4], v[5]);
#pragma unroll
            for (int q = 0; q < 6; q++) pc[4 + q] = make_double2(v[6 + 2 * q], v[7 + 2 * q]);
            np = 10;
        } else if (layout == 11) { // the same in fp32: [x y z u | v w rho cs | t t t t | t t r r | r r r r]
            pc[0] = __builtin_bit_cast(double2, make_float4((float)(ph.x - a.gmin[0]), (float)(ph.y - a.gmin[1]),
                                                            (float)(ph.z - a.gmin[2]), (float)v[0]));
            pc[1] = __builtin_bit_cast(double2, make_float4((float)v[1], (float)v[2], (float)v[4], (float)v[5]));
#pragma unroll
            for (int q = 0; q < 3; q++)
                pc[2 + q] = __builtin_bit_cast(double2, make_float4((float)v[6 + 4 * q], (float)v[7 + 4 * q], (float)v[8 + 4 * q], (float)v[9 + 4 * q]));
            np = 5;
        } else if (layout == 1) { // WCSPH [x y | z cs | u v | w m | rho tmpj] (+ [h p]: variable h / tensile correction)
            pc[0] = make_double2(ph.x, ph.y); pc[1] = make_double2(ph.z, v[6]);
            pc[2] = make_double2(v[0], v[1]); pc[3] = make_double2(v[2], v[3]);
            pc[4] = make_double2(v[4], v[5]); pc[5] = make_double2(ph.w, v[7]);
            np = a.nr / 2;
        } else if (layout == 5) { // fp32 records [x-x0 y-y0 z-z0 h | aux...] (option record_f32), a.nr floats
            float w[4 + MAX_AUX];
            w[0] = (float)(ph.x - a.gmin[0]); w[1] = (float)(ph.y - a.gmin[1]); w[2] = (float)(ph.z - a.gmin[2]);
            w[3] = (float)ph.w;
#pragma unroll
            for (int k = 0; k < MAX_AUX; k++) w[4 + k] = k < a.na ? (float)v[k] : 0.f;
#pragma unroll
            for (int q = 0; q < (4 + MAX_AUX) / 4; q++)
                pc[q] = __builtin_bit_cast(double2, make_float4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]));
            np = a.nr / 4;
        } else if (layout == 4) { // generated families under uniform h: [x y z | aux...] (h is a launch constant)
            double w[3 + MAX_AUX + 1];
            w[0] = ph.x; w[1] = ph.y; w[2] = ph.z;
#pragma unroll
            for (int k = 0; k < MAX_AUX + 1; k++) w[3 + k] = k < a.na ? v[k < MAX_AUX ? k : 0] : 0.0;
#pragma unroll
            for (int q = 0; q < (3 + MAX_AUX + 1) / 2; q++) pc[q] = make_double2(w[2 * q], w[2 * q + 1]);
            np = (a.nr + 1) / 2;
        } else if (layout == 3) { // TVF under uniform h: [x y | z rho | u v | w p | Vj2 what | uhat vhat] (+ [m -] with artificial viscosity)
            pc[0] = make_double2(ph.x, ph.y); pc[1] = make_double2(ph.z, v[6]);
            pc[2] = make_double2(v[0], v[1]); pc[3] = make_double2(v[2], v[7]);
            pc[4] = make_double2(v[10], v[5]); pc[5] = make_double2(v[3], v[4]);
            pc[6] = make_double2(v[9], 0.0);
            np = a.nr > 12 ? 7 : 6;
        } else if (layout == 2) { // compact density records [x y z m] (uniform h)
            pc[0] = make_double2(ph.x, ph.y); pc[1] = make_double2(ph.z, v[0]);
            np = 2;
        } else { // [x y z h | aux...]
            pc[0] = make_double2(ph.x, ph.y); pc[1] = make_double2(ph.z, ph.w);
#pragma unroll
            for (int q = 0; q < MAX_AUX / 2; q++) pc[2 + q] = make_double2(v[2 * q], v[2 * q + 1]);
            np = a.nr / 2;
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
    const double q = rho != 0.0 ? v[7] * (1.0 / (rho * rho)) : 0.0; // tmpj = p*rhoj21, wc/basic.py:211,234 (as k_pack, derived 1)
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

template <class T> struct FamWCSPH_T {
    typedef T Real; // arithmetic type of the pair loop
    static constexpr uint32_t CF0 = F_CONT | F_MOM | F_XSPH; // flag set compiled as a constant (variant 6)
#ifndef SPH_WCSPH_MINB
#define SPH_WCSPH_MINB 4
#endif
    static constexpr int MINB = SPH_WCSPH_MINB; // wavefronts per SIMD the pair kernel is compiled for (VGPR budget)
    static constexpr int NA = 8; // u v w m rho tmpj(=p/rho^2) cs p
    static constexpr int NR = 12; // x y z h + NA (128-B padded records measured slower: larger L2 footprint)
    struct Params {
        T c0, alpha, beta, gx, gy, gz, eps;
        double *arho, *au, *av, *aw, *ax, *ay, *az, *dt_cfl, *dt_force;
    };
    struct Dest {
        T u, v, w, rho, p, cs, tmpi;
        T arho, au, av, aw, ax, ay, az, dt_cfl;
    };
    template <class A> static __device__ __forceinline__ void load(Dest &D, const T *a, const A &, uint32_t)
    {
        D.u = a[0]; D.v = a[1]; D.w = a[2]; D.rho = a[4]; D.tmpi = a[5]; D.cs = a[6]; D.p = a[7];
        D.arho = D.au = D.av = D.aw = D.ax = D.ay = D.az = T(0.0);
        D.dt_cfl = T(-1.0); // running max of |h v.x / r2| over the pairs; -1: none yet (finish)
    }
    // The algebra below is the reference's (cited per term) regrouped so that a
    // pair costs one rsqrt and one reciprocal:  DWIJ = tg*XIJ  =>
    //   DWIJ.VIJ = tg*(XIJ.VIJ),   f*DWIJ = (f*tg)*XIJ,
    //   1/(R2IJ+EPS) and 1/RHOIJ from one reciprocal of their product,
    //   1/R2IJ = rinv^2.
    // PRED: the lean kernel calls pair() for every lane of every iteration and
    // passes the neighbour criterion as `pass`; a pair that fails contributes
    // exactly zero because every term carries the factor m_j (set to 0) -- no
    // branch around the accumulators, which then stay in their registers.
    static constexpr bool PRED = true;
    template <int KK, bool UH, class A>
    static __device__ __forceinline__ void pair(Dest &D, const real4<T> &pi, const real4<T> &pj, T r2,
                                                const T (&s)[NA], uint32_t fl, const A &a, bool pass = true)
    {
        PairGeomT<T> g;
        // (one transcendental per pair where the momentum equation acts: pair_geom_mom)
        constexpr bool MRG = SPH_MERGED_RSQ && sizeof(T) == 8 && !SphKernel<KK>::CUTOFF;
        T tt_m = T(0.0);
        if constexpr (MRG) {
            if (fl & F_MOM) tt_m = pair_geom_mom<KK, UH>(g, pi, pj, r2, T(0.5) * (D.rho + s[4]), a);
            else pair_geom<KK, UH>(g, pi, pj, r2, a);
        } else {
            pair_geom<KK, UH>(g, pi, pj, r2, a);
        }
        const T tg = pair_gradfac<KK, UH>(g);
        const T vij0 = D.u - s[0], vij1 = D.v - s[1], vij2 = D.w - s[2]; // VIJ equation.py:214-223
        const T vdotx = vij0 * g.xij[0] + vij1 * g.xij[1] + vij2 * g.xij[2];
        const T mj = pass ? s[3] : T(0.0);
        if (fl & F_CONT) D.arho = fma(mj * tg, vdotx, D.arho); // basic_equations.py:187-192
        if (fl & (F_MOM | F_XSPH)) {
            const T rhoij = T(0.5) * (D.rho + s[4]); // RHOIJ equation.py:196
            T rhoij1;                              // RHOIJ1 :199
            T wij = T(0.0);
            if (fl & (F_XSPH | F_TENSILE)) wij = pair_w<KK, UH>(g);
            if (fl & F_MOM) { // wc/basic.py:204-259
                const T re = r2 + g.eps;
                const T tt = MRG ? tt_m : fast_rcp(re * rhoij);
                const T inv_re = rhoij * tt;
                rhoij1 = re * tt;
                const T hv = g.hij * vdotx;
                // the viscosity acts for approaching pairs only (vdotx < 0; h > 0): muij from min(hv, 0) is exactly
                // zero otherwise and takes piij with it
                const T muij = raw_min(hv, T(0.0)) * inv_re;
                const T cij = T(0.5) * (D.cs + s[6]);
                const T piij = (a.p.beta * muij - a.p.alpha * cij) * muij * rhoij1;
                // dt_cfl = max_j (|h v.x / r2| + c0) = max_j |h v.x / r2| + c0 (rounding is monotonic): the running
                // maximum starts at -1 (no pair yet), finish() adds c0 once
                const T dtv = fabs(hv * (g.rinv * g.rinv));
                D.dt_cfl = raw_max(D.dt_cfl, (r2 > T(1e-12) && pass) ? dtv : T(-1.0));
                const T tmpj = s[5];
                T tmp = D.tmpi + tmpj;
                if (fl & F_TENSILE) {
                    // WDP = KERNEL(XIJ, DELTAP*HIJ, HIJ)  equation.py:243-246
                    const T qd = (a.k.deltap * g.hij) * g.h1;
                    const T wdp = SphKernel<KK>::w(qd, g.dim) * g.fac;
                    T fij = wij * fast_rcp(wdp);
                    fij = fij * fij;
                    fij = fij * fij;
                    const T Ri = D.p > 0 ? T(0.01) * D.tmpi : T(0.2) * fabs(D.tmpi);
                    const T Rj = s[7] > 0 ? T(0.01) * tmpj : T(0.2) * fabs(tmpj);
                    tmp = (D.tmpi + tmpj) + (Ri + Rj) * fij;
                }
                const T ft = -mj * (tmp + piij) * tg;
                D.au = fma(ft, g.xij[0], D.au);
                D.av = fma(ft, g.xij[1], D.av);
                D.aw = fma(ft, g.xij[2], D.aw);
            } else {
                rhoij1 = fast_rcp(rhoij);
            }
            if (fl & F_XSPH) { // basic_equations.py:290-295
                const T tmp = -a.p.eps * mj * wij * rhoij1;
                D.ax = fma(tmp, vij0, D.ax);
                D.ay = fma(tmp, vij1, D.ay);
                D.az = fma(tmp, vij2, D.az);
            }
        }
    }
    template <class A> static __device__ __forceinline__ void finish(Dest &D, const A &a, uint32_t o)
    {
        if (a.dflags & F_CONT) a.p.arho[o] = D.arho;
        if (a.dflags & F_MOM) { // post_loop wc/basic.py:261-271
            T au = D.au + a.p.gx, av = D.av + a.p.gy, aw = D.aw + a.p.gz;
            a.p.au[o] = au; a.p.av[o] = av; a.p.aw[o] = aw;
            a.p.dt_cfl[o] = D.dt_cfl < T(0.0) ? T(0.0) : D.dt_cfl + a.p.c0;
            a.p.dt_force[o] = au * au + av * av + aw * aw;
        }
        if (a.dflags & F_XSPH) { // post_loop basic_equations.py:297-300
            a.p.ax[o] = D.ax + D.u; a.p.ay[o] = D.ay + D.v; a.p.az[o] = D.az + D.w;
        }
    }
};
typedef FamWCSPH_T<double> FamWCSPH;

// The same equations on 64-byte records [x y | z u | v w | rho m] (fp32: 32 bytes): when the group before
// this one was the Tait EOS over every array read here (sph_group.src_eos), p and cs are functions of rho
// and are recomputed per gathered record -- four 16-B pieces in ONE 64-B half line instead of five pieces
// that straddle a 128-B line half of the time.  ~14 more VALU operations per pair, hidden under the gathers.
// Arithmetic as k_nosrc's (TaitEOS, gamma = 7) and k_pack's p / rho^2.
// UM (uniform-mass records): every particle of a source array has the same mass (seen by the last sph_nnps_update),
// so the record's eighth slot carries p / rho^2 as k_pack computes it for the 80-byte records and m is a constant of
// the source: of the EOS only cs = c0 (rho/rho0)^3 is left in the loop (13 of its 17 instructions go).
template <class T, bool UM = false> struct FamWCSPHE_T : FamWCSPH_T<T> {
    static constexpr bool EOSF = true;
    static constexpr bool UMASS = UM;
    static constexpr int NR = 8;
    // one gathered record as it arrives (four / two 16-B pieces), and its decoding
    struct Raw {
        typename std::conditional<sizeof(T) == 8, double2, float4>::type q[sizeof(T) == 8 ? 4 : 2];
    };
    template <class A> static __device__ __forceinline__ void load_raw(const A &a, uint32_t jg, Raw &r)
    {
        if constexpr (sizeof(T) == 8) {
            const double2 *p = reinterpret_cast<const double2 *>(a.rec) + (unsigned long long)jg * 4;
            r.q[0] = p[0]; r.q[1] = p[1]; r.q[2] = p[2]; r.q[3] = p[3];
        } else {
            const float4 *p = reinterpret_cast<const float4 *>(a.rec) + (unsigned long long)jg * 2;
            r.q[0] = p[0]; r.q[1] = p[1];
        }
    }
    // gk: the exponent gamma = 2 gk + 1 -- the constant 3 here (water: the compiler folds the powers), the launch
    // argument in FamWCSPHEG_T below
    template <class A> static __device__ __forceinline__ void decode(const A &a, const Raw &r, uint32_t fl, T mu, real4<T> &pj, T (&s)[8],
                                                                     int gk = 3)
    {
        T rho;
        if constexpr (sizeof(T) == 8) {
            pj.x = r.q[0].x; pj.y = r.q[0].y; pj.z = r.q[1].x; pj.w = 0.0;
            s[0] = r.q[1].y; s[1] = r.q[2].x; s[2] = r.q[2].y; s[3] = r.q[3].y; rho = r.q[3].x;
        } else {
            pj.x = r.q[0].x; pj.y = r.q[0].y; pj.z = r.q[0].z; pj.w = 0.f;
            s[0] = r.q[0].w; s[1] = r.q[1].x; s[2] = r.q[1].y; s[3] = r.q[1].w; rho = r.q[1].z;
        }
        s[4] = rho;
        s[5] = s[6] = s[7] = T(0.0);
        if constexpr (UM) {
            const T q = s[3]; // p / rho^2
            s[3] = mu;
            if (fl & F_MOM) {
                const T ratio = rho * (T)a.e_rho01;
                s[5] = q;
                s[6] = (T)a.e_c0 * tait_cs_power(ratio, gk);
            }
        } else
        if (fl & F_MOM) { // the flags of this (destination, source): a compile-time constant in the common case; a
                          // continuity-only destination -- a dam break's walls -- reads neither
            const T ratio = rho * (T)a.e_rho01;
            T r7, r3; // (ratio^gamma, ratio^((gamma - 1) / 2): named for the usual exponent)
            tait_powers(ratio, gk, r7, r3);
            const T p = (T)a.e_p0 + (T)a.e_B * (r7 - T(1.0));
            s[5] = rho != T(0.0) ? p * fast_rcp(rho * rho) : T(0.0);
            s[6] = (T)a.e_c0 * r3;
            s[7] = p;
        }
    }
    template <class A> static __device__ __forceinline__ void load_fused(const A &a, uint32_t jg, uint32_t fl, T mu, real4<T> &pj, T (&s)[8])
    {
        Raw r;
        load_raw(a, jg, r);
        decode(a, r, fl, mu, pj, s);
    }
};

// ... with the exponent as a launch argument (gamma = 1, 3, 5: PairArgs::e_gk).  A family of its own because the select
// costs the water kernels 1.3-2 % of their time when they carry it (profiles/r06_ab_tables.txt).
template <class T, bool UM = false> struct FamWCSPHEG_T : FamWCSPHE_T<T, UM> {
    typedef FamWCSPHE_T<T, UM> Base;
    template <class A> static __device__ __forceinline__ void load_fused(const A &a, uint32_t jg, uint32_t fl, T mu, real4<T> &pj, T (&s)[8])
    {
        typename Base::Raw r;
        Base::load_raw(a, jg, r);
        Base::decode(a, r, fl, mu, pj, s, a.e_gk);
    }
};

// Variable h with ONE mass per source array: [x y | z h | u v | w rho] (fp32: [x y z h | u v w rho]) -- 64 bytes instead of
// the 96-byte records with cs, m, p / rho^2 and p: the mass is a constant of the source, p, cs and p / rho^2 are the
// Tait EOS of the gathered rho (as FamWCSPHE_T without the uniform-mass slot).  Run with UH = false.
template <class T> struct FamWCSPHV_T : FamWCSPH_T<T> {
    static constexpr bool EOSF = true;
    static constexpr int NR = 8;
    template <class A> static __device__ __forceinline__ void load_fused(const A &a, uint32_t jg, uint32_t fl, T mu, real4<T> &pj, T (&s)[8])
    {
        T rho;
        if constexpr (sizeof(T) == 8) {
            const double2 *p = reinterpret_cast<const double2 *>(a.rec) + (unsigned long long)jg * 4;
            const double2 q0 = p[0], q1 = p[1], q2 = p[2], q3 = p[3];
            pj.x = q0.x; pj.y = q0.y; pj.z = q1.x; pj.w = q1.y;
            s[0] = q2.x; s[1] = q2.y; s[2] = q3.x; rho = q3.y;
        } else {
            const float4 *p = reinterpret_cast<const float4 *>(a.rec) + (unsigned long long)jg * 2;
            const float4 q0 = p[0], q1 = p[1];
            pj.x = q0.x; pj.y = q0.y; pj.z = q0.z; pj.w = q0.w;
            s[0] = q1.x; s[1] = q1.y; s[2] = q1.z; rho = q1.w;
        }
        s[3] = mu;
        s[4] = rho;
        s[5] = s[6] = s[7] = T(0.0);
        if (fl & F_MOM) {
            const T ratio = rho * (T)a.e_rho01;
            T r7, r3; // (ratio^gamma, ratio^((gamma - 1) / 2): named for the usual exponent)
            tait_powers(ratio, 3, r7, r3); // (gamma = 7 only: sph_eval_group checks)
            const T p = (T)a.e_p0 + (T)a.e_B * (r7 - T(1.0));
            s[5] = rho != T(0.0) ? p * fast_rcp(rho * rho) : T(0.0);
            s[6] = (T)a.e_c0 * r3;
            s[7] = p;
        }
    }
};

// ---- the same equations over the MERGED order of all arrays of the grid (sph_ctx::merged): ONE record stream, one
// phase 1 and one phase 2 per wavefront whatever the number of arrays, destinations of every array in one launch.
// A dam break -- fluid <- {fluid, boundary, obstacle}, walls <- fluid -- is two CLASSES of arrays: which equations act for
// a (destination, source) pair depends on the classes of the two particles only.  Records are the uniform-mass ones,
// [x y | z u | v w | +-rho p/rho^2]: the SIGN of rho is the particle's class (rho > 0 always), the mass a constant of
// the class.  The class table is the kernel's compile-time flag constant CF = f00 | f01 << 4 | f10 << 8 | f11 << 12
// (f<destination class><source class>: F_CONT | F_MOM | F_XSPH bits), so every "does equation e act for this pair" is
// a boolean expression of two sign bits, and the criterion stays a factor: a pair without equations adds exactly zero.
// Reference semantics: per-source equation lists of pysph/sph/acceleration_eval.py:126-151 (here per class pair),
// equations wc/basic.py:198-269, basic_equations.py:187-192,285-300.  Sums run over all arrays in cell order instead of
// source by source (another association of the same terms).
#define WCSPHM_CT(f00, f01, f10, f11) ((uint32_t)(f00) | ((uint32_t)(f01) << 4) | ((uint32_t)(f10) << 8) | ((uint32_t)(f11) << 12))
template <class T> struct FamWCSPHM_T : FamWCSPHE_T<T, true> {
    typedef FamWCSPHE_T<T, true> Base;
    typedef typename Base::Raw Raw;
    static constexpr bool MERGED = true;
    // WCSPHScheme(fluids, solids): fluid <- fluid all three, fluid <- solid no XSPH, solid <- fluid continuity only
    static constexpr uint32_t CF0 = WCSPHM_CT(F_CONT | F_MOM | F_XSPH, F_CONT | F_MOM, F_CONT, 0);
    struct Params {
        T c0, alpha, beta, gx, gy, gz, eps;
        double mu1;                                // mass of the class-1 arrays (class 0: SrcDesc::mu)
        uint32_t rng[SPH_MAX_ARRAYS][2];           // per slot: destination index range [start, stop) (empty: no destination)
        double *out[SPH_MAX_ARRAYS][9];            // per slot: arho au av aw ax ay az dt_cfl dt_force
    };
    static __device__ __forceinline__ size_t rng_offset(uint32_t slot) { return __builtin_offsetof(Params, rng) + (size_t)slot * 8; }
    struct Dest : Base::Dest { bool dc; };
    template <class A> static __device__ __forceinline__ void load(Dest &D, const T *a, const A &A_, uint32_t o, uint32_t)
    {
        Base::load(D, a, A_, o);
        D.dc = a[3] < T(0.0); // decode() left the class in the sign of the mass
    }
    template <class A> static __device__ __forceinline__ void decode(const A &a, const Raw &r, uint32_t, T mu, real4<T> &pj, T (&s)[8])
    {
        T rho, q;
        if constexpr (sizeof(T) == 8) {
            pj.x = r.q[0].x; pj.y = r.q[0].y; pj.z = r.q[1].x; pj.w = 0.0;
            s[0] = r.q[1].y; s[1] = r.q[2].x; s[2] = r.q[2].y; q = r.q[3].y; rho = r.q[3].x;
        } else {
            pj.x = r.q[0].x; pj.y = r.q[0].y; pj.z = r.q[0].z; pj.w = 0.f;
            s[0] = r.q[0].w; s[1] = r.q[1].x; s[2] = r.q[1].y; q = r.q[1].w; rho = r.q[1].z;
        }
        const bool c1 = rho < T(0.0);
        s[3] = c1 ? -(T)a.p.mu1 : mu;          // +-m: the sign is the class
        rho = fabs(rho);
        s[4] = rho;
        const T ratio = rho * (T)a.e_rho01;
        s[5] = q;                               // p / rho^2 as k_pack_merged computed it from the stored p
        s[6] = (T)a.e_c0 * tait_cs_power(ratio, 3); // (gamma = 7 only: sph_eval_group checks)
        s[7] = T(0.0);
    }
    template <class A> static __device__ __forceinline__ void load_fused(const A &a, uint32_t jg, uint32_t fl, T mu, real4<T> &pj, T (&s)[8])
    {
        Raw r;
        Base::load_raw(a, jg, r);
        decode(a, r, fl, mu, pj, s);
    }
    // does equation `bit` act for (destination class dc, source class sc)?  ct is a compile-time constant
    static __device__ __forceinline__ bool acts(uint32_t ct, uint32_t bit, bool dc, bool sc)
    {
        const bool c00 = ct & bit, c01 = (ct >> 4) & bit, c10 = (ct >> 8) & bit, c11 = (ct >> 12) & bit;
        return dc ? (sc ? c11 : c10) : (sc ? c01 : c00);
    }
    template <int KK, bool UH, class A>
    static __device__ __forceinline__ void pair(Dest &D, const real4<T> &pi, const real4<T> &pj, T r2,
                                                const T (&s)[8], uint32_t ct, const A &a, bool pass = true)
    {
        PairGeomT<T> g;
        constexpr bool MRG = SPH_MERGED_RSQ && sizeof(T) == 8 && !SphKernel<KK>::CUTOFF;
        T tt_m = T(0.0);
        if constexpr (MRG) tt_m = pair_geom_mom<KK, UH>(g, pi, pj, r2, T(0.5) * (D.rho + s[4]), a);
        else pair_geom<KK, UH>(g, pi, pj, r2, a);
        const T tg = pair_gradfac<KK, UH>(g);
        const T vij0 = D.u - s[0], vij1 = D.v - s[1], vij2 = D.w - s[2];
        const T vdotx = vij0 * g.xij[0] + vij1 * g.xij[1] + vij2 * g.xij[2];
        const bool sc = s[3] < T(0.0);
        const T m = fabs(s[3]);
        const bool on_c = pass && acts(ct, F_CONT, D.dc, sc), on_m = pass && acts(ct, F_MOM, D.dc, sc),
                   on_x = pass && acts(ct, F_XSPH, D.dc, sc);
        D.arho = fma((on_c ? m : T(0.0)) * tg, vdotx, D.arho); // basic_equations.py:187-192
        const T rhoij = T(0.5) * (D.rho + s[4]);
        const T wij = pair_w<KK, UH>(g);
        // wc/basic.py:204-259
        const T re = r2 + g.eps;
        const T tt = MRG ? tt_m : fast_rcp(re * rhoij);
        const T inv_re = rhoij * tt;
        const T rhoij1 = re * tt;
        const T hv = g.hij * vdotx;
        const T muij = raw_min(hv, T(0.0)) * inv_re; // approaching pairs only, as FamWCSPH_T::pair
        const T cij = T(0.5) * (D.cs + s[6]);
        const T piij = (a.p.beta * muij - a.p.alpha * cij) * muij * rhoij1;
        const T dtv = fabs(hv * (g.rinv * g.rinv));
        D.dt_cfl = raw_max(D.dt_cfl, (r2 > T(1e-12) && on_m) ? dtv : T(-1.0));
        const T ft = -(on_m ? m : T(0.0)) * ((D.tmpi + s[5]) + piij) * tg;
        D.au = fma(ft, g.xij[0], D.au);
        D.av = fma(ft, g.xij[1], D.av);
        D.aw = fma(ft, g.xij[2], D.aw);
        // basic_equations.py:290-295
        const T tmp = -a.p.eps * (on_x ? m : T(0.0)) * wij * rhoij1;
        D.ax = fma(tmp, vij0, D.ax);
        D.ay = fma(tmp, vij1, D.ay);
        D.az = fma(tmp, vij2, D.az);
    }
    template <class A> static __device__ __forceinline__ void finish(Dest &D, const A &a, uint32_t o, uint32_t slot)
    {
        // the equations with this lane's class as destination (class table row); its array's output pointers
        const uint32_t ct = a.dflags;
        const uint32_t row = D.dc ? ((ct >> 8) | (ct >> 12)) & 15u : (ct | (ct >> 4)) & 15u;
        const size_t base = __builtin_offsetof(A, p) + __builtin_offsetof(Params, out) + (size_t)slot * (9 * sizeof(double *));
        auto out = [&](int k) { return kernarg_read<double *>(base + (size_t)k * sizeof(double *)); };
        if (row & F_CONT) out(0)[o] = D.arho;
        if (row & F_MOM) { // post_loop wc/basic.py:261-271
            const T au = D.au + a.p.gx, av = D.av + a.p.gy, aw = D.aw + a.p.gz;
            out(1)[o] = au; out(2)[o] = av; out(3)[o] = aw;
            out(7)[o] = D.dt_cfl < T(0.0) ? T(0.0) : D.dt_cfl + a.p.c0;
            out(8)[o] = au * au + av * av + aw * aw;
        }
        if (row & F_XSPH) { // post_loop basic_equations.py:297-300
            out(4)[o] = D.ax + D.u; out(5)[o] = D.ay + D.v; out(6)[o] = D.az + D.w;
        }
    }
};

// ... and with VARIABLE h (round 5): records [x y | z h | u v | w +-rho] (fp32 [x y z h | u v w +-rho]) as FamWCSPHV_T's
// with the class in the sign of rho; p / rho^2 and cs are the Tait EOS of the gathered rho.  Run with UH = false.
template <class T> struct FamWCSPHMV_T : FamWCSPHM_T<T> {
    typedef FamWCSPHM_T<T> Base;
    template <class A> static __device__ __forceinline__ void load_fused(const A &a, uint32_t jg, uint32_t, T mu, real4<T> &pj, T (&s)[8])
    {
        T rho;
        if constexpr (sizeof(T) == 8) {
            const double2 *p = reinterpret_cast<const double2 *>(a.rec) + (unsigned long long)jg * 4;
            const double2 q0 = p[0], q1 = p[1], q2 = p[2], q3 = p[3];
            pj.x = q0.x; pj.y = q0.y; pj.z = q1.x; pj.w = q1.y;
            s[0] = q2.x; s[1] = q2.y; s[2] = q3.x; rho = q3.y;
        } else {
            const float4 *p = reinterpret_cast<const float4 *>(a.rec) + (unsigned long long)jg * 2;
            const float4 q0 = p[0], q1 = p[1];
            pj.x = q0.x; pj.y = q0.y; pj.z = q0.z; pj.w = q0.w;
            s[0] = q1.x; s[1] = q1.y; s[2] = q1.z; rho = q1.w;
        }
        const bool c1 = rho < T(0.0);
        s[3] = c1 ? -(T)a.p.mu1 : mu; // +-m: the sign is the class
        rho = fabs(rho);
        s[4] = rho;
        const T ratio = rho * (T)a.e_rho01;
        T r7, r3;
        tait_powers(ratio, 3, r7, r3); // (gamma = 7 only: sph_eval_group checks)
        const T p = (T)a.e_p0 + (T)a.e_B * (r7 - T(1.0));
        s[5] = rho != T(0.0) ? p * fast_rcp(rho * rho) : T(0.0);
        s[6] = (T)a.e_c0 * r3;
        s[7] = T(0.0);
    }
};

// WCSPH records of the aggregated kernel use the layout
//   [x y z cs | u v w m | rho tmpj | h p]
// so that the common case (uniform h, no tensile correction) gathers 80 B =
// five 16-B pieces per pair and never touches the last piece.
template <bool UH>
__device__ __forceinline__ void load_record_wcsph(const double *__restrict__ rj, uint32_t fl, double4 &pj, double (&s)[8])
{
    const double2 *r2 = reinterpret_cast<const double2 *>(rj);
    const double2 a0 = r2[0], a1 = r2[1], b0 = r2[2], b1 = r2[3], c = r2[4];
    pj.x = a0.x; pj.y = a0.y; pj.z = a1.x; pj.w = 0.0;
    s[0] = b0.x; s[1] = b0.y; s[2] = b1.x; s[3] = b1.y; s[4] = c.x; s[5] = c.y; s[6] = a1.y; s[7] = 0.0;
    if (!UH || (fl & F_TENSILE)) {
        const double2 d = *reinterpret_cast<const double2 *>(rj + 10);
        pj.w = d.x; s[7] = d.y;
    }
}
template <> __device__ __forceinline__ void load_record<FamWCSPH, true>(const double *__restrict__ rj, uint32_t fl, double4 &pj, double (&s)[8]) { load_record_wcsph<true>(rj, fl, pj, s); }
template <> __device__ __forceinline__ void load_record<FamWCSPH, false>(const double *__restrict__ rj, uint32_t fl, double4 &pj, double (&s)[8]) { load_record_wcsph<false>(rj, fl, pj, s); }

// ---- WCSPHScheme options: delta-SPH, laminar viscosity ---------------------------------
// The rates group of WCSPHScheme(delta_sph=True and / or nu != 0) in ONE sweep: Continuity / Momentum / XSPH exactly as
// FamWCSPH_T evaluates them, plus
//   F_DCONT  ContinuityEquationDeltaSPH   wc/basic.py:400-414   (reads gradrho of destination and source)
//   F_DMOM   MomentumEquationDeltaSPH     wc/basic.py:326-343
//   F_LAM    LaminarViscosity             wc/viscosity.py:12-27
//   F_LAMD   LaminarViscosityDeltaSPH     wc/viscosity.py:134-144
// per (destination, source) like every other flag.  All terms add into arho / au av aw before finish(), so dt_force sees
// the summed acceleration as the reference's post_loop does.  Records [x y z h | u v w m rho p/rho^2 cs p] and, with
// DS (a delta-SPH continuity term acts on this destination), three more values: the source's gradrho.
// The new terms are the reference's, regrouped as FamWCSPH_T::pair regroups (DWIJ = tg XIJ, reciprocals shared); the
// one place where terms cancel -- psi = fac XIJ - gradrho_i - gradrho_j -- keeps the reference's order.
template <class T, bool DS> struct FamWCSPHX_T : FamWCSPH_T<T> {
    typedef FamWCSPH_T<T> Base;
    static constexpr uint32_t CF0 = DS ? (F_CONT | F_MOM | F_XSPH | F_DCONT | F_DMOM | F_LAMD) : (F_CONT | F_MOM | F_XSPH | F_LAM);
    static constexpr int MINB = DS ? 2 : 3; // (the base family's sums and inputs + the extra terms' registers)
    static constexpr int NA = DS ? 11 : 8;  // Base's eight + gradrho x y z
    static constexpr int NR = DS ? 16 : 12;
    struct Params : Base::Params {
        T nu4, eta;   // LaminarViscosity: 4 nu, eta
        T lfac;       // LaminarViscosityDeltaSPH: 2 (dim + 2) nu rho0
        T mfac;       // MomentumEquationDeltaSPH: alpha c0 rho0
        T dfac;       // ContinuityEquationDeltaSPH: delta c0
    };
    struct Dest : Base::Dest { T g0, g1, g2, rho1; };
    template <class A> static __device__ __forceinline__ void load(Dest &D, const T *s, const A &a, uint32_t o)
    {
        Base::load(D, s, a, o);
        D.g0 = D.g1 = D.g2 = T(0.0);
        if constexpr (DS) { D.g0 = s[8]; D.g1 = s[9]; D.g2 = s[10]; }
        D.rho1 = fast_rcp(D.rho);
    }
    template <int KK, bool UH, class A>
    static __device__ __forceinline__ void pair(Dest &D, const real4<T> &pi, const real4<T> &pj, T r2,
                                                const T (&s)[NA], uint32_t fl, const A &a, bool pass = true)
    {
        Base::template pair<KK, UH>(D, pi, pj, r2, reinterpret_cast<const T (&)[8]>(s), fl, a, pass);
        if (!(fl & (F_DCONT | F_DMOM | F_LAM | F_LAMD))) return;
        PairGeomT<T> g;
        pair_geom<KK, UH>(g, pi, pj, r2, a);
        const T tg = pair_gradfac<KK, UH>(g); // DWIJ = tg XIJ (0 for r <= 1e-12)
        const T vij0 = D.u - s[0], vij1 = D.v - s[1], vij2 = D.w - s[2];
        const T vdotx = vij0 * g.xij[0] + vij1 * g.xij[1] + vij2 * g.xij[2];
        const T rhoj = s[4];
        if (fl & F_LAM) { // tmp = mb 4 nu Fij / ((rhoa + rhob) (R2IJ + eta HIJ^2)),  Fij = DWIJ.XIJ
            const T fij = tg * (g.xij[0] * g.xij[0] + g.xij[1] * g.xij[1] + g.xij[2] * g.xij[2]);
            const T den = (D.rho + rhoj) * (r2 + a.p.eta * g.hij * g.hij);
            const T tmp = pass ? s[3] * a.p.nu4 * fij * fast_rcp(den) : T(0.0);
            D.au = fma(tmp, vij0, D.au);
            D.av = fma(tmp, vij1, D.av);
            D.aw = fma(tmp, vij2, D.aw);
        }
        if (fl & (F_DCONT | F_DMOM | F_LAMD)) {
            const T re1 = fast_rcp(r2 + g.eps);
            // Vj = mj / rhoj; a candidate outside the criterion adds exactly zero (a select, not a product: a parked
            // padding row has rho = 0)
            const T Vj = pass ? s[3] * fast_rcp(rhoj) : T(0.0);
            if (fl & (F_DMOM | F_LAMD)) { // both are  f piij Vj / rhoi DWIJ  with piij = VIJ.XIJ / (R2IJ + EPS)
                T f = T(0.0);
                if (fl & F_DMOM) f = a.p.mfac * g.hij; // alpha HIJ c0 rho0
                if (fl & F_LAMD) f += a.p.lfac;        // 2 (dim + 2) nu rho0
                const T ft = f * (vdotx * re1) * Vj * D.rho1 * tg;
                D.au = fma(ft, g.xij[0], D.au);
                D.av = fma(ft, g.xij[1], D.av);
                D.aw = fma(ft, g.xij[2], D.aw);
            }
            if constexpr (DS) {
                if (fl & F_DCONT) {
                    const T fac = T(-2.0) * (rhoj - D.rho) * re1;
                    const T px = (fac * g.xij[0] - D.g0) - s[8];
                    const T py = (fac * g.xij[1] - D.g1) - s[9];
                    const T pz = (fac * g.xij[2] - D.g2) - s[10];
                    const T psidot = tg * (px * g.xij[0] + py * g.xij[1] + pz * g.xij[2]);
                    D.arho = fma(a.p.dfac * g.hij * psidot, Vj, D.arho);
                }
            }
        }
    }
};

// ---- delta-SPH pre-passes on [x y z h | m rho] records --------------------------------------------------------
//   F_MOMENT   GradientCorrectionPreStep          wc/kernel_correction.py:46-74: m_mat[3i+j] = -sum V_b DWIJ[i] XIJ[j]
//   F_GRADRHO  ContinuityEquationDeltaSPHPreStep  wc/basic.py:355-369: gradrho = sum (rho_b - rho_a) DWIJ V_b
//   F_GCORR    GradientCorrection                 wc/kernel_correction.py:98-123, in front of it in the group: DWIJ
//              becomes res = M^-1 DWIJ on the leading n x n block when |sum|res| - sum|DWIJ|| / (sum|DWIJ| + 1e-4 HIJ) < tol
// The reference solves M res = DWIJ per pair with gj_solve (wc/linalg.py:94-166).  Its row search exchanges nothing
// (after `bigrow = row` the exchange is of an element with itself), so it is elimination in the given row order, and
// that does not depend on the right-hand side: load() factorises M once per destination (multipliers, the upper
// triangle, reciprocal pivots), pair() applies the factors to DWIJ in gj_solve's own order.  gj_solve's ways out:
//   * a pivot but the last below 1e-12 in magnitude: it returns with the result untouched (zero).  All factors are set
//     to zero, which gives res = 0;
//   * the last pivot exactly zero: with |rhs| > 1e-12 in that row the result stays zero; otherwise the row is left as
//     it is (res_last = rhs_last, nothing eliminated above it): reciprocal 1, its column of the triangle 0, and the
//     per-pair test of that rhs (`chk`).
// res = 0 makes the change ~1 and DWIJ stays uncorrected (for tol <= 1), as in the reference.
template <class T> struct FamDSPre_T {
    typedef T Real;
    static constexpr bool PRED = true;
    static constexpr uint32_t CF0 = F_GRADRHO | F_GCORR;
    static constexpr int MINB = 3;
    static constexpr int NA = 2; // m rho
    static constexpr int NR = 6;
    struct Params {
        int mdim;       // GradientCorrectionPreStep.dim
        int n;          // GradientCorrection.dim
        T tol;
        double *mm[9];  // m_mat__0..8 of the destination: written by F_MOMENT, read by F_GCORR
        double *gr[3];  // gradrho__0..2
    };
    struct Dest {
        T rho;
        T acc[9];                       // F_MOMENT: the nine sums; F_GRADRHO: acc[0..2]
        T c10, c20, c21, u01, u02, u12; // elimination multipliers, upper triangle
        T i0, i1, i2;                   // reciprocal pivots
        bool chk;                       // last pivot exactly zero: the pair tests its right-hand side
    };
    template <class A> static __device__ __forceinline__ void load(Dest &D, const T *s, const A &a, uint32_t o)
    {
        D.rho = s[1];
#pragma unroll
        for (int k = 0; k < 9; k++) D.acc[k] = T(0.0);
        D.c10 = D.c20 = D.c21 = D.u01 = D.u02 = D.u12 = D.i0 = D.i1 = D.i2 = T(0.0);
        D.chk = false;
        if (!(a.dflags & F_GCORR)) return;
        const int n = a.p.n;
        T M[3][3];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) M[i][j] = (i < n && j < n) ? (T)a.p.mm[3 * i + j][o] : T(i == j ? 1.0 : 0.0);
        bool ok = true;
        if (n > 1) { // column 0
            const T d = M[0][0];
            if (fabs(d) < T(1e-12)) ok = false;
            else {
                D.c10 = -M[1][0] / d;
                M[1][1] += D.c10 * M[0][1]; M[1][2] += D.c10 * M[0][2];
                if (n > 2) { D.c20 = -M[2][0] / d; M[2][1] += D.c20 * M[0][1]; M[2][2] += D.c20 * M[0][2]; }
            }
        }
        if (ok && n > 2) { // column 1
            const T d = M[1][1];
            if (fabs(d) < T(1e-12)) ok = false;
            else { D.c21 = -M[2][1] / d; M[2][2] += D.c21 * M[1][2]; }
        }
        if (!ok) { D.c10 = D.c20 = D.c21 = T(0.0); return; } // every factor zero: res = 0
        D.u01 = M[0][1]; D.u02 = M[0][2]; D.u12 = M[1][2];
        D.i0 = T(1.0) / M[0][0]; D.i1 = T(1.0) / M[1][1]; D.i2 = T(1.0) / M[2][2]; // (rows >= n: identity)
        const T last = n == 3 ? M[2][2] : (n == 2 ? M[1][1] : M[0][0]);
        if (last == T(0.0)) {
            D.chk = true;
            if (n == 3) { D.i2 = T(1.0); D.u02 = D.u12 = T(0.0); }
            else if (n == 2) { D.i1 = T(1.0); D.u01 = T(0.0); }
            else D.i0 = T(1.0);
        }
    }
    template <int KK, bool UH, class A>
    static __device__ __forceinline__ void pair(Dest &D, const real4<T> &pi, const real4<T> &pj, T r2,
                                                const T (&s)[NA], uint32_t fl, const A &a, bool pass = true)
    {
        PairGeomT<T> g;
        pair_geom<KK, UH>(g, pi, pj, r2, a);
        const T tg = pair_gradfac<KK, UH>(g);
        T dw[3] = {tg * g.xij[0], tg * g.xij[1], tg * g.xij[2]};
        const T Vj = pass ? s[0] * fast_rcp(s[1]) : T(0.0); // (a select: a parked padding row has rho = 0)
        if (fl & F_MOMENT) {
            const int md = a.p.mdim;
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int j = 0; j < 3; j++)
                    if (i < md && j < md) D.acc[3 * i + j] = fma(-Vj * dw[i], g.xij[j], D.acc[3 * i + j]);
        }
        if (fl & F_GRADRHO) {
            if (fl & F_GCORR) {
                const int n = a.p.n;
                // forward: rows 1, 2 += multiplier * row above, in gj_solve's order
                T y0 = dw[0], y1 = dw[1], y2 = dw[2];
                if (n > 1) y1 = fma(D.c10, y0, y1);
                if (n > 2) { y2 = fma(D.c20, y0, y2); y2 = fma(D.c21, y1, y2); }
                const T ylast = n == 3 ? y2 : (n == 2 ? y1 : y0);
                // back substitution from the last row up
                T x0, x1 = T(0.0), x2 = T(0.0);
                if (n > 2) { x2 = y2 * D.i2; y1 = fma(-D.u12, x2, y1); y0 = fma(-D.u02, x2, y0); }
                if (n > 1) { x1 = y1 * D.i1; y0 = fma(-D.u01, x1, y0); }
                x0 = y0 * D.i0;
                if (D.chk && fabs(ylast) > T(1e-12)) { x0 = x1 = x2 = T(0.0); }
                T rmag = fabs(x0), dmag = fabs(dw[0]);
                if (n > 1) { rmag += fabs(x1); dmag += fabs(dw[1]); }
                if (n > 2) { rmag += fabs(x2); dmag += fabs(dw[2]); }
                const T change = fabs(rmag - dmag) / (dmag + T(1.0e-4) * g.hij);
                if (change < a.p.tol) {
                    dw[0] = x0;
                    if (n > 1) dw[1] = x1;
                    if (n > 2) dw[2] = x2;
                }
            }
            const T cf = (s[1] - D.rho) * Vj;
            D.acc[0] = fma(cf, dw[0], D.acc[0]);
            D.acc[1] = fma(cf, dw[1], D.acc[1]);
            D.acc[2] = fma(cf, dw[2], D.acc[2]);
        }
    }
    template <class A> static __device__ __forceinline__ void finish(Dest &D, const A &a, uint32_t o)
    {
        if (a.dflags & F_MOMENT) {
#pragma unroll
            for (int k = 0; k < 9; k++) a.p.mm[k][o] = D.acc[k];
        }
        if (a.dflags & F_GRADRHO) {
#pragma unroll
            for (int k = 0; k < 3; k++) a.p.gr[k][o] = D.acc[k];
        }
    }
};

// ---- density summations (basic_equations.py:19-29, transport_velocity.py:24-58)
template <class T> struct FamDensity_T {
    typedef T Real; // arithmetic type of the pair loop
    static constexpr bool PRED = true; // see FamWCSPH
    static constexpr uint32_t CF0 = F_TVFSD; // flag set compiled as a constant (variant 6)
    static constexpr int MINB = 4; // wavefronts per SIMD the pair kernel is compiled for (VGPR budget)
    static constexpr int NA = 1; // m
    static constexpr int NR = 6;  // x y z h m pad
    struct Params { double *rho, *V; };
    struct Dest { T m, rho, V; };
    template <class A> static __device__ __forceinline__ void load(Dest &D, const T *a, const A &, uint32_t) { D.m = a[0]; D.rho = T(0.0); D.V = T(0.0); }
    template <int KK, bool UH, class A>
    static __device__ __forceinline__ void pair(Dest &D, const real4<T> &pi, const real4<T> &pj, T r2,
                                                const T (&s)[NA], uint32_t fl, const A &a, bool pass = true)
    {
        PairGeomT<T> g;
        pair_geom<KK, UH>(g, pi, pj, r2, a);
        T wij = pair_w<KK, UH>(g);
        wij = pass ? wij : T(0.0); // PRED: a pair outside the criterion adds exactly zero
        if (fl & F_SD) D.rho += s[0] * wij;
        if (fl & F_TVFSD) { D.V += wij; D.rho += D.m * wij; }
    }
    template <class A> static __device__ __forceinline__ void finish(Dest &D, const A &a, uint32_t o)
    {
        a.p.rho[o] = D.rho;
        if (a.dflags & F_TVFSD) a.p.V[o] = D.V;
    }
};
typedef FamDensity_T<double> FamDensity;

// Density records of the aggregated kernel under uniform h: [x y z m] (32 B, two
// 16-B pieces per pair); otherwise the generic [x y z h | m pad].
template <> __device__ __forceinline__ void load_record<FamDensity, true>(const double *__restrict__ rj, uint32_t fl, double4 &pj, double (&s)[1])
{
    const double2 *r2 = reinterpret_cast<const double2 *>(rj);
    const double2 a0 = r2[0], a1 = r2[1];
    pj.x = a0.x; pj.y = a0.y; pj.z = a1.x; pj.w = 0.0;
    s[0] = a1.y;
}

// ---- neighbour lists (LinkedListNNPS.find_nearest_neighbors, linked_list_nnps.pyx:92-196; the reference's
//      NeighborCache, nnps_base.pyx:1144-1257) on the pair-kernel skeleton: the "equation" counts the pairs
//      that pass the exact criterion and, in the fill pass, writes the neighbour's ORIGINAL index (it travels
//      in the record as a double) behind the destination's list start.  Same candidate tiles, fp32 prefilter
//      and exact test as every other family, so the lists are the pair loops' own neighbour sets.
struct FamNbr {
    typedef double Real;
    static constexpr bool PRED = true;
    static constexpr uint32_t CF0 = 1;
    static constexpr int MINB = 4;
    static constexpr int NA = 1; // original index of the particle
    static constexpr int NR = 6; // x y z h idx pad  (uniform h: [x y z idx])
    struct Params { uint32_t *count; const uint32_t *start; uint32_t *nbrs; };
    struct Dest { uint32_t n, base; };
    template <class A> static __device__ __forceinline__ void load(Dest &D, const double *, const A &a, uint32_t o)
    {
        D.n = 0;
        D.base = a.p.start ? a.p.start[o] : 0u;
    }
    template <int KK, bool UH, class A>
    static __device__ __forceinline__ void pair(Dest &D, const double4 &, const double4 &, double, const double (&s)[NA], uint32_t,
                                                const A &a, bool pass = true)
    {
        if (pass) {
            if (a.p.nbrs) a.p.nbrs[D.base + D.n] = (uint32_t)s[0];
            D.n++;
        }
    }
    template <class A> static __device__ __forceinline__ void finish(Dest &D, const A &a, uint32_t o)
    {
        if (a.p.count) a.p.count[o] = D.n;
    }
};
template <> __device__ __forceinline__ void load_record<FamNbr, true>(const double *__restrict__ rj, uint32_t, double4 &pj, double (&s)[1])
{
    const double2 *r2 = reinterpret_cast<const double2 *>(rj);
    const double2 a0 = r2[0], a1 = r2[1];
    pj.x = a0.x; pj.y = a0.y; pj.z = a1.x; pj.w = 0.0;
    s[0] = a1.y;
}

// ---- TVF momentum terms (transport_velocity.py:219-545) -------------------
template <class T> struct FamTVF_T {
    typedef T Real; // arithmetic type of the pair loop
    static constexpr bool PRED = true; // see FamWCSPH
    static constexpr uint32_t CF0 = F_TP | F_TVISC | F_TAS; // flag set compiled as a constant (variant 6)
    static constexpr int MINB = 4; // wavefronts per SIMD the pair kernel is compiled for (VGPR budget; fp64: 125-129 registers)
    static constexpr int NA = 12; // u v w uhat vhat what rho p V m Vj2 pad
    static constexpr int NR = 16; // x y z h + NA
    struct Params {
        T pb, gx, gy, gz, tdamp, nu, c0, alpha;
        const double *m; // the destination's own mass (a neighbour's travels in the records only with F_TAV)
        double *au, *av, *aw, *auhat, *avhat, *awhat;
    };
    struct Dest {
        T u, v, w, uh, vh, wh, rho, p, Vi2, mi1;
        T au, av, aw, auh, avh, awh;
    };
    template <class A> static __device__ __forceinline__ void load(Dest &D, const T *a, const A &A_, uint32_t o)
    {
        D.u = a[0]; D.v = a[1]; D.w = a[2]; D.uh = a[3]; D.vh = a[4]; D.wh = a[5];
        D.rho = a[6]; D.p = a[7]; D.Vi2 = a[10]; D.mi1 = T(1.0) / T(A_.p.m[o]);
        D.au = D.av = D.aw = D.auh = D.avh = D.awh = T(0.0);
    }
    template <int KK, bool UH, class A>
    static __device__ __forceinline__ void pair(Dest &D, const real4<T> &pi, const real4<T> &pj, T r2,
                                                const T (&s)[NA], uint32_t fl, const A &a, bool pass = true)
    {
        PairGeomT<T> g;
        pair_geom<KK, UH>(g, pi, pj, r2, a);
        T tg = pair_gradfac<KK, UH>(g);
        tg = pass ? tg : T(0.0); // PRED: every term carries DWIJ
        T dw0 = tg * g.xij[0], dw1 = tg * g.xij[1], dw2 = tg * g.xij[2];
        T rhoj = s[6], Vj2 = s[10];
        T vsum = D.Vi2 + Vj2;
        T vij0 = D.u - s[0], vij1 = D.v - s[1], vij2 = D.w - s[2];
        if (fl & F_TP) { // :290-320
            T pij = rhoj * D.p + D.rho * s[7];
            pij *= fast_rcp(rhoj + D.rho);
            T tmp = -pij * D.mi1 * vsum;
            D.au += tmp * dw0; D.av += tmp * dw1; D.aw += tmp * dw2;
            tmp = -a.p.pb * D.mi1 * vsum;
            D.auh += tmp * dw0; D.avh += tmp * dw1; D.awh += tmp * dw2;
        }
        if (fl & F_TAV) { // :420-436
            T vijdotrij = vij0 * g.xij[0] + vij1 * g.xij[1] + vij2 * g.xij[2];
            T piij = T(0.0);
            if (vijdotrij < 0) {
                T muij = (g.hij * vijdotrij) * fast_rcp(r2 + g.eps);
                piij = -a.p.alpha * a.p.c0 * muij;
                piij = s[9] * piij * fast_rcp(T(0.5) * (D.rho + rhoj));
            }
            D.au += -piij * dw0; D.av += -piij * dw1; D.aw += -piij * dw2;
        }
        if (fl & F_TVISC) { // :363-384
            T etai = a.p.nu * D.rho, etaj = a.p.nu * rhoj;
            T etaij = 2 * (etai * etaj) * fast_rcp(etai + etaj);
            T Fij = dw0 * g.xij[0] + dw1 * g.xij[1] + dw2 * g.xij[2];
            T tmp = D.mi1 * vsum * etaij * Fij * fast_rcp(r2 + g.eps);
            D.au += tmp * vij0; D.av += tmp * vij1; D.aw += tmp * vij2;
        }
        if (fl & F_TAS) { // :473-545
            // A = rho v (x) (vhat - v);  0.5 (A_i + A_j) . DWIJ, with the dot
            // products (vhat - v) . DWIJ taken first (same terms as the
            // reference's 18 products, associated per particle)
            const T ddi = (D.uh - D.u) * dw0 + (D.vh - D.v) * dw1 + (D.wh - D.w) * dw2;
            const T ddj = (s[3] - s[0]) * dw0 + (s[4] - s[1]) * dw1 + (s[5] - s[2]) * dw2;
            const T ci = D.rho * ddi, cj = rhoj * ddj;
            const T tmp = T(0.5) * D.mi1 * vsum;
            D.au += tmp * (ci * D.u + cj * s[0]);
            D.av += tmp * (ci * D.v + cj * s[1]);
            D.aw += tmp * (ci * D.w + cj * s[2]);
        }
    }
    template <class A> static __device__ __forceinline__ void finish(Dest &D, const A &a, uint32_t o)
    {
        T damp = T(1.0); // post_loop :322-325
        if (a.t < a.p.tdamp) damp = T(0.5) * (sin((-T(0.5) + a.t / a.p.tdamp) * M_PI) + T(1.0));
        T gx = (a.dflags & F_TP) ? a.p.gx * damp : T(0.0);
        T gy = (a.dflags & F_TP) ? a.p.gy * damp : T(0.0);
        T gz = (a.dflags & F_TP) ? a.p.gz * damp : T(0.0);
        a.p.au[o] = D.au + gx; a.p.av[o] = D.av + gy; a.p.aw[o] = D.aw + gz;
        if (a.dflags & F_TP) { a.p.auhat[o] = D.auh; a.p.avhat[o] = D.avh; a.p.awhat[o] = D.awh; }
    }
};
typedef FamTVF_T<double> FamTVF;

// TVF records of the aggregated kernel under uniform h (see k_pack layout 3):
// five 16-B pieces per pair, a sixth when the artificial-stress term acts, a
// seventh (the neighbour's mass) only for the artificial viscosity.
template <> __device__ __forceinline__ void load_record<FamTVF, true>(const double *__restrict__ rj, uint32_t fl, double4 &pj, double (&s)[12])
{
    const double2 *r2 = reinterpret_cast<const double2 *>(rj);
    const double2 a0 = r2[0], a1 = r2[1], b0 = r2[2], b1 = r2[3], c0 = r2[4];
    pj.x = a0.x; pj.y = a0.y; pj.z = a1.x; pj.w = 0.0;
    s[0] = b0.x; s[1] = b0.y; s[2] = b1.x; s[6] = a1.y; s[7] = b1.y; s[8] = 0.0; s[9] = 0.0; s[10] = c0.x; s[11] = 0.0;
    s[3] = s[4] = 0.0; s[5] = c0.y;
    if (fl & F_TAS) {
        const double2 d0 = r2[5];
        s[3] = d0.x; s[4] = d0.y;
    }
    if (fl & F_TAV) s[9] = r2[6].x;
}

// The same terms on records WITHOUT p and V (sph_group.src_eos = 2): the group before this one was TVF's StateEquation
// over every particle of every array read here and its density summation ran earlier in the evaluation, so
// p = p0 (rho / rho0 - b) and V = rho / m are functions of the gathered rho and the source array's ONE mass:
// [x y | z rho | u v | w uhat | vhat what] -- 80 bytes, five 16-B pieces instead of six (four without the artificial
// stress); fp32: [x y z rho | u v w uhat | vhat what - -], three pieces instead of four.  One reciprocal more per pair.
template <class T> struct FamTVFE_T : FamTVF_T<T> {
    static constexpr bool EOSF = true;
    static constexpr int NA = 12;
    template <class A> static __device__ __forceinline__ void load_fused(const A &a, uint32_t jg, uint32_t fl, T mu, real4<T> &pj, T (&s)[12])
    {
        T rho;
        if constexpr (sizeof(T) == 8) {
            const double2 *p = reinterpret_cast<const double2 *>(a.rec) + (unsigned long long)jg * (unsigned)(a.nrec >> 1);
            const double2 q0 = p[0], q1 = p[1], q2 = p[2], q3 = p[3];
            pj.x = q0.x; pj.y = q0.y; pj.z = q1.x; pj.w = 0.0; rho = q1.y;
            s[0] = q2.x; s[1] = q2.y; s[2] = q3.x; s[3] = q3.y; s[4] = s[5] = 0.0;
            if (fl & F_TAS) { const double2 q4 = p[4]; s[4] = q4.x; s[5] = q4.y; }
        } else {
            const float4 *p = reinterpret_cast<const float4 *>(a.rec) + (unsigned long long)jg * (unsigned)(a.nrec >> 2);
            const float4 q0 = p[0], q1 = p[1];
            pj.x = q0.x; pj.y = q0.y; pj.z = q0.z; pj.w = 0.f; rho = q0.w;
            s[0] = q1.x; s[1] = q1.y; s[2] = q1.z; s[3] = q1.w; s[4] = s[5] = 0.f;
            if (fl & F_TAS) { const float4 q2 = p[2]; s[4] = q2.x; s[5] = q2.y; }
        }
        s[6] = rho;
        s[7] = (T)a.e_p0 * (rho * (T)a.e_rho01 - (T)a.e_B); // StateEquation, as k_nosrc computes it
        s[8] = T(0.0);
        s[9] = mu;
        const T vj = mu * fast_rcp(rho);                     // 1 / V_j with V = sum W = rho / m (transport_velocity.py:52-58): Vj2 = (m / rho)^2, :303-306
        s[10] = vj * vj;
        s[11] = T(0.0);
    }
};

// ---- EDAC force group (pysph/sph/wc/edac.py:301-488 with transport_velocity.py:328-545 and basic_equations.py:260-300)
//      Everything EDACScheme puts on a fluid destination in its force group, in ONE sweep: the pressure gradient
//      (external form :320-343, or the internal one :443-478 with pb, the transport accelerations and the
//      destination's pavg taken off both pressures), the artificial and the physical viscosity, the artificial stress
//      (internal branch), the pressure rate ap (:365-386: a continuity-like term with cs^2 and a damping term with
//      its OWN viscosity edac_nu) and the XSPH correction (external branch; it reads the fluid only, which the
//      per-source flags express).  INT = the internal branch: the two branches are two instantiations, each with its
//      scheme's default flag set as a compile-time constant and without the other branch's terms and accumulators.
//      Records: the generic [x y z h | u v w uhat vhat what rho p V m Vj2 -] of FamTVF_T; under uniform h k_pack's
//      compact layout 3 in its seven-piece form, which carries m (load_record_edac below).  p is integrated state
//      here, not a function of rho, so the records that leave p and V out (FamTVFE_T) do not apply.
enum { F_EP = 1, /* F_TVISC = 2, F_TAV = 4, F_TAS = 8 as in FamTVF_T */ F_EINT = 16, F_EDAC = 32, F_EXS = 64 };
template <class T, bool INT> struct FamEDAC_T {
    typedef T Real;
    static constexpr bool PRED = true; // every term carries DWIJ or WIJ, both zero for a pair outside the criterion
    static constexpr uint32_t CF0 = INT ? (F_EP | F_EINT | F_TVISC | F_TAS | F_EDAC) : (F_EP | F_TVISC | F_EDAC | F_EXS);
    static constexpr uint32_t MASK = INT ? ~(uint32_t)F_EXS : ~(uint32_t)(F_TAS | F_EINT);
    static constexpr int MINB = 4;
    static constexpr int NA = 12; // u v w uhat vhat what rho p V m Vj2 pad
    static constexpr int NR = 16;
    struct Params {
        T pb, gx, gy, gz, tdamp, nu, c0, alpha, cs2, enu, eps;
        const double *m, *pavg; // the destination's own mass and average pressure
        double *au, *av, *aw, *auhat, *avhat, *awhat, *ap, *ax, *ay, *az;
    };
    struct Dest {
        T u, v, w, uh, vh, wh, rho, p, pavg, Vi2, mi1;
        T au, av, aw, auh, avh, awh, ap, ax, ay, az;
    };
    template <class A> static __device__ __forceinline__ void load(Dest &D, const T *a, const A &A_, uint32_t o)
    {
        D.u = a[0]; D.v = a[1]; D.w = a[2]; D.uh = a[3]; D.vh = a[4]; D.wh = a[5];
        D.rho = a[6]; D.p = a[7]; D.Vi2 = a[10]; D.mi1 = T(1.0) / T(A_.p.m[o]);
        D.pavg = T(0.0); // the destination's, taken off both pressures (edac.py:450-454)
        if (INT && (A_.dflags & F_EP)) D.pavg = T(A_.p.pavg[o]);
        D.uh = INT ? D.uh : T(0.0); D.vh = INT ? D.vh : T(0.0); D.wh = INT ? D.wh : T(0.0);
        D.au = D.av = D.aw = D.auh = D.avh = D.awh = D.ap = D.ax = D.ay = D.az = T(0.0);
    }
    template <int KK, bool UH, class A>
    static __device__ __forceinline__ void pair(Dest &D, const real4<T> &pi, const real4<T> &pj, T r2,
                                                const T (&s)[NA], uint32_t fl_, const A &a, bool pass = true)
    {
        const uint32_t fl = fl_ & MASK;
        PairGeomT<T> g;
        pair_geom<KK, UH>(g, pi, pj, r2, a);
        T tg = pair_gradfac<KK, UH>(g);
        tg = pass ? tg : T(0.0);
        const T dw0 = tg * g.xij[0], dw1 = tg * g.xij[1], dw2 = tg * g.xij[2];
        const T rhoj = s[6], Vj2 = s[10];
        const T vsum = D.Vi2 + Vj2;
        const T vij0 = D.u - s[0], vij1 = D.v - s[1], vij2 = D.w - s[2];
        const T xdw = dw0 * g.xij[0] + dw1 * g.xij[1] + dw2 * g.xij[2]; // XIJ . DWIJ
        const T rsum1 = fast_rcp(rhoj + D.rho);
        if (fl & F_EP) { // edac.py:323-343 / :448-478
            T pij = rhoj * (D.p - D.pavg) + D.rho * (s[7] - D.pavg);
            pij *= rsum1;
            T tmp = -pij * D.mi1 * vsum;
            D.au += tmp * dw0; D.av += tmp * dw1; D.aw += tmp * dw2;
            if (INT) {
                tmp = -a.p.pb * D.mi1 * vsum;
                D.auh += tmp * dw0; D.avh += tmp * dw1; D.awh += tmp * dw2;
            }
        }
        if (fl & F_TAV) { // transport_velocity.py:420-436
            const T vijdotrij = vij0 * g.xij[0] + vij1 * g.xij[1] + vij2 * g.xij[2];
            T piij = T(0.0);
            if (vijdotrij < 0) {
                const T muij = (g.hij * vijdotrij) * fast_rcp(r2 + g.eps);
                piij = -a.p.alpha * a.p.c0 * muij;
                piij = s[9] * piij * fast_rcp(T(0.5) * (D.rho + rhoj));
            }
            D.au += -piij * dw0; D.av += -piij * dw1; D.aw += -piij * dw2;
        }
        if (fl & (F_TVISC | F_EDAC)) {
            // 2 rho_i rho_j / (rho_i + rho_j) / (r^2 + eps) (Vi2 + Vj2) / m_i (XIJ . DWIJ): shared by the physical
            // viscosity (transport_velocity.py:363-384, times nu) and the pressure damping (edac.py:375,384-386, times edac_nu)
            const T common = T(2.0) * (D.rho * rhoj) * rsum1 * D.mi1 * vsum * xdw * fast_rcp(r2 + g.eps);
            if (fl & F_TVISC) {
                const T tmp = a.p.nu * common;
                D.au += tmp * vij0; D.av += tmp * vij1; D.aw += tmp * vij2;
            }
            if (fl & F_EDAC) {
                const T vijdotdwij = dw0 * vij0 + dw1 * vij1 + dw2 * vij2;
                D.ap += D.rho * fast_rcp(rhoj) * a.p.cs2 * s[9] * vijdotdwij; // :380-381
                D.ap += a.p.enu * common * (D.p - s[7]);
            }
        }
        if (INT && (fl & F_TAS)) { // transport_velocity.py:473-545, as FamTVF_T
            const T ddi = (D.uh - D.u) * dw0 + (D.vh - D.v) * dw1 + (D.wh - D.w) * dw2;
            const T ddj = (s[3] - s[0]) * dw0 + (s[4] - s[1]) * dw1 + (s[5] - s[2]) * dw2;
            const T ci = D.rho * ddi, cj = rhoj * ddj;
            const T tmp = T(0.5) * D.mi1 * vsum;
            D.au += tmp * (ci * D.u + cj * s[0]);
            D.av += tmp * (ci * D.v + cj * s[1]);
            D.aw += tmp * (ci * D.w + cj * s[2]);
        }
        if (!INT && (fl & F_EXS)) { // basic_equations.py:290-295
            T wij = pair_w<KK, UH>(g);
            wij = pass ? wij : T(0.0);
            const T tmp = -a.p.eps * s[9] * wij * fast_rcp(T(0.5) * (D.rho + rhoj));
            D.ax += tmp * vij0; D.ay += tmp * vij1; D.az += tmp * vij2;
        }
    }
    template <class A> static __device__ __forceinline__ void finish(Dest &D, const A &a, uint32_t o)
    {
        if (a.dflags & (F_EP | F_TVISC | F_TAV | F_TAS)) {
            T gx = T(0.0), gy = T(0.0), gz = T(0.0);
            if (a.dflags & F_EP) { // post_loop edac.py:345-351 / :480-488
                T damp = T(1.0);
                if (a.t < a.p.tdamp) damp = T(0.5) * (sin((-T(0.5) + a.t / a.p.tdamp) * M_PI) + T(1.0));
                gx = a.p.gx * damp; gy = a.p.gy * damp; gz = a.p.gz * damp;
            }
            a.p.au[o] = D.au + gx; a.p.av[o] = D.av + gy; a.p.aw[o] = D.aw + gz;
        }
        if (INT && (a.dflags & F_EP)) { a.p.auhat[o] = D.auh; a.p.avhat[o] = D.avh; a.p.awhat[o] = D.awh; }
        if (a.dflags & F_EDAC) a.p.ap[o] = D.ap;
        if (!INT && (a.dflags & F_EXS)) { // post_loop basic_equations.py:297-300: with eps = 0 still ax = u (EDACStep moves x with it)
            a.p.ax[o] = D.ax + D.u; a.p.ay[o] = D.ay + D.v; a.p.az[o] = D.az + D.w;
        }
    }
};

// EDAC records of the aggregated kernel under uniform h: k_pack layout 3 in its seven-piece form
// [x y | z rho | u v | w p | Vj2 what | uhat vhat | m -] (112 B instead of the generic 128 B); the sixth piece is
// read only where the artificial stress acts, the seventh (m: the pressure rate reads it) always.
template <bool INT>
__device__ __forceinline__ void load_record_edac(const double *__restrict__ rj, uint32_t fl, double4 &pj, double (&s)[12])
{
    const double2 *r2 = reinterpret_cast<const double2 *>(rj);
    const double2 a0 = r2[0], a1 = r2[1], b0 = r2[2], b1 = r2[3], c0 = r2[4], e0 = r2[6];
    pj.x = a0.x; pj.y = a0.y; pj.z = a1.x; pj.w = 0.0;
    s[0] = b0.x; s[1] = b0.y; s[2] = b1.x; s[6] = a1.y; s[7] = b1.y; s[8] = 0.0; s[9] = e0.x; s[10] = c0.x; s[11] = 0.0;
    s[3] = s[4] = 0.0; s[5] = c0.y;
    if (INT && (fl & F_TAS)) {
        const double2 d0 = r2[5];
        s[3] = d0.x; s[4] = d0.y;
    }
}
template <> __device__ __forceinline__ void load_record<FamEDAC_T<double, true>, true>(const double *__restrict__ rj, uint32_t fl, double4 &pj, double (&s)[12]) { load_record_edac<true>(rj, fl, pj, s); }
template <> __device__ __forceinline__ void load_record<FamEDAC_T<double, false>, true>(const double *__restrict__ rj, uint32_t fl, double4 &pj, double (&s)[12]) { load_record_edac<false>(rj, fl, pj, s); }

// ---- ComputeAveragePressure (edac.py:62-79), with the density summations when they share its destination and
//      group (EDACScheme without solids).  pavg = sum of the neighbours' p, nnbr = their number -- the pairs that
//      pass the exact criterion, as FamNbr counts them -- and the division.  Records [x y z h | m p].
enum { F_AVGP = 4 }; // next to F_SD = 1, F_TVFSD = 2
template <class T> struct FamAvgP_T {
    typedef T Real;
    static constexpr bool PRED = true;
    static constexpr uint32_t CF0 = F_TVFSD | F_AVGP;
    static constexpr int MINB = 4;
    static constexpr int NA = 2; // m p
    static constexpr int NR = 6; // x y z h m p
    struct Params { double *rho, *V, *pavg, *nnbr; };
    struct Dest { T m, rho, V, ps, nn; };
    template <class A> static __device__ __forceinline__ void load(Dest &D, const T *a, const A &, uint32_t)
    {
        D.m = a[0]; D.rho = T(0.0); D.V = T(0.0); D.ps = T(0.0); D.nn = T(0.0);
    }
    template <int KK, bool UH, class A>
    static __device__ __forceinline__ void pair(Dest &D, const real4<T> &pi, const real4<T> &pj, T r2,
                                                const T (&s)[NA], uint32_t fl, const A &a, bool pass = true)
    {
        if (fl & (F_SD | F_TVFSD)) {
            PairGeomT<T> g;
            pair_geom<KK, UH>(g, pi, pj, r2, a);
            T wij = pair_w<KK, UH>(g);
            wij = pass ? wij : T(0.0);
            if (fl & F_SD) D.rho += s[0] * wij;
            if (fl & F_TVFSD) { D.V += wij; D.rho += D.m * wij; }
        }
        if (fl & F_AVGP) { D.ps += pass ? s[1] : T(0.0); D.nn += pass ? T(1.0) : T(0.0); }
    }
    template <class A> static __device__ __forceinline__ void finish(Dest &D, const A &a, uint32_t o)
    {
        if (a.dflags & (F_SD | F_TVFSD)) a.p.rho[o] = D.rho;
        if (a.dflags & F_TVFSD) a.p.V[o] = D.V;
        if (a.dflags & F_AVGP) {
            a.p.pavg[o] = D.nn > T(0.0) ? D.ps / D.nn : D.ps; // post_loop :77-79
            a.p.nnbr[o] = D.nn;
        }
    }
};

// ---- gas dynamics (pysph/sph/gas_dynamics/basic.py) -------------------------------------------------------------
// The geometry of a pair at ONE smoothing length: WI / DWI / GHI of the reference are the kernel at the
// destination's own h, DWJ at the source's (equation.py:214-224), where `gij` holds the pair at HIJ.  Under uniform h
// the three lengths are one and `gij` is returned as it is.
template <int KK, bool UH, class T, class A>
__device__ __forceinline__ void pair_geom_at(PairGeomT<T> &g, const PairGeomT<T> &gij, T h, const A &a)
{
    g = gij;
    if (!UH) {
        g.hij = h;
        g.h1 = SphKernel<KK>::CUTOFF ? T(1) / h : fast_rcp(h);
        g.fac = kernel_norm((T)a.k.sigma, g.h1, a.k.dim);
        g.q = g.rij * g.h1;
    }
}

// SummationDensity (:74-219): the sums rho, arho, grhox..z, dwdh with WI / DWI / GHI and, in finish(), the whole
// post_loop -- one Newton-Raphson step for h of every particle that has not converged, the 0.8 / 1.2 clamp, the
// fallback, the convergence test and the group's convergence word -- in ONE launch.  The post_loop runs in fp64 whatever
// the arithmetic of the sums.  A particle that converged in an EARLIER iteration is summed again every iteration and
// leaves with the raw arho (its post_loop block is skipped); one that converges in this launch leaves with arho * omega:
// the reference's behaviour, kept.  The new h goes to the property column only: the records every wavefront reads were
// packed before the launch.  Records [x y z h | m u v w].
enum { F_GSD = 1 };
template <class T> struct FamGasSD_T {
    typedef T Real;
    static constexpr bool PRED = true; // every sum carries WI, DWI or GHI, masked for a pair outside the criterion
    static constexpr uint32_t CF0 = F_GSD;
    static constexpr int MINB = 4;
    static constexpr int NA = 4; // m u v w
    static constexpr int NR = 8;
    static constexpr bool WAVE_SKIP = true;
    struct Params {
        double dim, k, htol;
        int iterate, once;     // density_iterations, iterate_only_once
        int skip;              // option gasd_skip in a repeated call: wavefronts without an unconverged destination leave early
        double *araw;          // ... the raw arho of every row, as the last full sweep summed it (null: not kept)
        const double *m, *h0;
        double *h, *rho, *arho, *grhox, *grhoy, *grhoz, *dwdh, *div, *omega, *ah, *converged;
        uint32_t *flag;        // the convergence word: 1 = some particle has not converged; flag[1]: wavefronts skipped
    };
    struct Dest { T u, v, w, rho, arho, gx, gy, gz, dwdh; };
    // Option gasd_skip: with positions, velocities, masses and its own h unchanged since the previous sweep, a converged
    // particle's sums come out the same again; what the reference's re-summation changes is arho (raw again, where the
    // sweep in which the particle converged left arho * omega) and div.  The wave-tile kernel only.
    template <class A> static __device__ __forceinline__ bool wave_skip(const A &a, uint32_t o, bool active)
    {
        if (!a.p.skip) return false;
        if (!__all(!active || a.p.converged[o] == 1.0)) return false;
        if ((threadIdx.x & 63) == 0) atomicAdd(a.p.flag + 1, 1u); // wavefronts that left here ("n_gasd_skipped")
        if (active) {
            const double ar = a.p.araw[o];
            a.p.arho[o] = ar;
            a.p.div[o] = -ar / a.p.rho[o];
        }
        return true;
    }
    template <class A> static __device__ __forceinline__ void load(Dest &D, const T *a, const A &, uint32_t)
    {
        D.u = a[1]; D.v = a[2]; D.w = a[3];
        D.rho = D.arho = D.gx = D.gy = D.gz = D.dwdh = T(0.0);
    }
    template <int KK, bool UH, class A>
    static __device__ __forceinline__ void pair(Dest &D, const real4<T> &pi, const real4<T> &pj, T r2,
                                                const T (&s)[NA], uint32_t, const A &a, bool pass = true)
    {
        PairGeomT<T> gij, g;
        pair_geom<KK, UH>(gij, pi, pj, r2, a);
        pair_geom_at<KK, UH>(g, gij, pi.w, a);
        T wi = pair_w<KK, UH>(g), tg = pair_gradfac<KK, UH>(g), ghi = pair_gradh<KK, UH>(g, a.k.dim);
        wi = pass ? wi : T(0.0); tg = pass ? tg : T(0.0); ghi = pass ? ghi : T(0.0);
        const T mj = s[0];
        const T dw0 = tg * g.xij[0], dw1 = tg * g.xij[1], dw2 = tg * g.xij[2];
        const T vijdotdwij = (D.u - s[1]) * dw0 + (D.v - s[2]) * dw1 + (D.w - s[3]) * dw2;
        D.rho += mj * wi;
        D.arho += mj * vijdotdwij;
        D.gx += mj * dw0; D.gy += mj * dw1; D.gz += mj * dw2;
        D.dwdh += mj * ghi;
    }
    template <class A> static __device__ __forceinline__ void finish(Dest &D, const A &a, uint32_t o)
    {
        const double rho = (double)D.rho, dwdh = (double)D.dwdh;
        double arho = (double)D.arho;
        if (a.p.araw) a.p.araw[o] = arho;
        if (a.p.iterate && !(a.p.converged[o] == 1.0)) { // :150-213
            const double mi = a.p.m[o], hi = a.p.h[o], hi0 = a.p.h0[o];
            const double rhoi = mi / pow(hi / a.p.k, a.p.dim);
            const double dhdrhoi = -hi / (a.p.dim * rho);
            double omegai = 1.0 - dhdrhoi * dwdh;
            if (omegai < 0) omegai = 1.0;
            const double gradhi = 1.0 / omegai;
            a.p.omega[o] = gradhi;
            const double func = rhoi - rho, dfdh = omegai / dhdrhoi;
            double hnew = hi - func / dfdh;
            if (hnew > 1.2 * hi) hnew = 1.2 * hi;
            else if (hnew < 0.8 * hi) hnew = 0.8 * hi;
            if (hnew <= 1e-6 || gradhi < 1e-6) hnew = a.p.k * pow(mi / rho, 1.0 / a.p.dim);
            const double diff = fabs(hnew - hi) / hi0;
            if (!((diff < a.p.htol && omegai > 0) || a.p.once)) {
                *a.p.flag = 1u; // the same constant from every lane that fails; the host reads the word once per call
                a.p.h[o] = hnew;
                a.p.converged[o] = 0.0;
            } else {
                arho *= gradhi;
                a.p.ah[o] = arho * dhdrhoi;
                a.p.converged[o] = 1.0;
            }
        }
        a.p.rho[o] = rho;
        a.p.arho[o] = arho;
        a.p.grhox[o] = (double)D.gx; a.p.grhoy[o] = (double)D.gy; a.p.grhoz[o] = (double)D.gz;
        a.p.dwdh[o] = dwdh;
        a.p.div[o] = -arho / rho;
    }
};

// MPMAccelerations (:356-483): everything its loop does in one sweep -- the grad-h pressure terms with DWI and DWJ (each
// at its own h), the artificial viscosity and its heating under dot <= 0, the thermal conduction with the signal
// velocity sqrt(|p_i - p_j| / RHOIJ), del2e and dt_cfl -- and the post_loop's sources of alpha1 / alpha2.  XIJ is
// normalised (zeroed below RIJ = 1e-8) AFTER the kernel gradients were formed from it, as in the reference, so Fij is
// the normalised XIJ against DWIJ at HIJ; the self pair adds to dt_cfl only.
// Records [x y z h | u v w rho p cs e m omega alpha1 alpha2 -]: 128 B in fp64 (eight 16-B pieces), 64 B in fp32.
enum { F_MPM = 1 };
template <class T> struct FamMPM_T {
    typedef T Real;
    static constexpr bool PRED = true; // the sums carry a kernel gradient, masked outside the criterion; dt_cfl is selected
    static constexpr uint32_t CF0 = F_MPM;
    static constexpr int MINB = 3;
    static constexpr int NA = 12; // u v w rho p cs e m omega alpha1 alpha2 pad
    static constexpr int NR = 16;
    struct Params {
        T beta;
        double sigma, alpha1_min, alpha2_min;
        int update_alpha1, update_alpha2;
        const double *h, *cs, *e, *div, *alpha1, *alpha2;
        double *au, *av, *aw, *ae, *del2e, *dt_cfl, *aalpha1, *aalpha2;
    };
    struct Dest {
        T u, v, w, rho, p, cs, e, al1, al2, pwi; // pwi = p_i / rho_i^2 omega_i
        T au, av, aw, ae, del2e, dtc;
    };
    template <class A> static __device__ __forceinline__ void load(Dest &D, const T *a, const A &, uint32_t)
    {
        D.u = a[0]; D.v = a[1]; D.w = a[2]; D.rho = a[3]; D.p = a[4]; D.cs = a[5]; D.e = a[6];
        D.al1 = a[9]; D.al2 = a[10];
        D.pwi = a[4] / (a[3] * a[3]) * a[8];
        D.au = D.av = D.aw = D.ae = D.del2e = D.dtc = T(0.0);
    }
    template <int KK, bool UH, class A>
    static __device__ __forceinline__ void pair(Dest &D, const real4<T> &pi, const real4<T> &pj, T r2,
                                                const T (&s)[NA], uint32_t, const A &a, bool pass = true)
    {
        PairGeomT<T> g, gi, gj;
        pair_geom<KK, UH>(g, pi, pj, r2, a);
        pair_geom_at<KK, UH>(gi, g, pi.w, a);
        pair_geom_at<KK, UH>(gj, g, pj.w, a);
        T tij = pair_gradfac<KK, UH>(g), ti = pair_gradfac<KK, UH>(gi), tj = pair_gradfac<KK, UH>(gj);
        tij = pass ? tij : T(0.0); ti = pass ? ti : T(0.0); tj = pass ? tj : T(0.0);
        const T mj = s[7], rhoj = s[3];
        const T pjw = s[4] / (rhoj * rhoj) * s[8]; // p_j / rho_j^2 omega_j
        const T cij = T(0.5) * (D.cs + s[5]);
        // :412-420: the normalised interaction vector
        const T rn = g.rij < T(1e-8) ? T(0.0) : g.rinv;
        const T x0 = g.xij[0] * rn, x1 = g.xij[1] * rn, x2 = g.xij[2] * rn;
        const T v0 = D.u - s[0], v1 = D.v - s[1], v2 = D.w - s[2];
        const T dot = v0 * x0 + v1 * x1 + v2 * x2;
        const T dwij0 = tij * g.xij[0], dwij1 = tij * g.xij[1], dwij2 = tij * g.xij[2];
        const T Fij = x0 * dwij0 + x1 * dwij1 + x2 * dwij2;
        const T rhoij1 = fast_rcp(T(0.5) * (D.rho + rhoj)); // 1 / RHOIJ
        const T pdiff = fabs(D.p - s[4]);
        const T vsig1 = T(0.5) * raw_max(T(2.0) * cij - a.p.beta * dot, T(0.0));
        const T vsig2 = sqrt(pdiff * rhoij1);
        const T cfl = cij + a.p.beta * dot;
        D.dtc = (pass && cfl > D.dtc) ? cfl : D.dtc;
        if (dot <= T(0.0)) { // :437-447
            const T alpha1 = T(0.5) * (D.al1 + s[9]);
            const T tmpv = mj * rhoij1 * alpha1 * vsig1 * dot;
            D.au += tmpv * dwij0; D.av += tmpv * dwij1; D.aw += tmpv * dwij2;
            D.ae += T(-0.5) * tmpv * dot * Fij;
        }
        // :455-461: the grad-h terms, DWI at h_i and DWJ at h_j
        const T gsum = D.pwi * ti + pjw * tj;
        D.au -= mj * gsum * g.xij[0]; D.av -= mj * gsum * g.xij[1]; D.aw -= mj * gsum * g.xij[2];
        const T vijdotdwi = ti * (v0 * g.xij[0] + v1 * g.xij[1] + v2 * g.xij[2]);
        D.ae += mj * D.pwi * vijdotdwi;
        // :463-469: conduction and the Laplacian of e
        const T alpha2 = T(0.5) * (D.al2 + s[10]);
        const T eij = D.e - s[6];
        D.ae += mj * rhoij1 * alpha2 * vsig2 * eij * Fij;
        D.del2e += mj / rhoj * eij * fast_rcp(g.rij + g.eps) * Fij;
    }
    template <class A> static __device__ __forceinline__ void finish(Dest &D, const A &a, uint32_t o)
    {
        a.p.au[o] = (double)D.au; a.p.av[o] = (double)D.av; a.p.aw[o] = (double)D.aw; a.p.ae[o] = (double)D.ae;
        const double del2e = (double)D.del2e;
        a.p.del2e[o] = del2e;
        a.p.dt_cfl[o] = (double)D.dtc;
        double aa1 = 0.0, aa2 = 0.0; // :471-483
        if (a.p.update_alpha1 || a.p.update_alpha2) {
            const double hi = a.p.h[o];
            const double tau = hi / (a.p.sigma * a.p.cs[o]);
            if (a.p.update_alpha1) aa1 = (a.p.alpha1_min - a.p.alpha1[o]) / tau + fmax(-a.p.div[o], 0.0);
            if (a.p.update_alpha2) aa2 = (a.p.alpha2_min - a.p.alpha2[o]) / tau + 0.01 * hi * fabs(del2e) / sqrt(a.p.e[o]);
        }
        a.p.aalpha1[o] = aa1; a.p.aalpha2[o] = aa2;
    }
};

// ---- ADKE (gas_dynamics/basic.py:32-71, :274-353; boundary_equations.py) -----------------------------------------
// SummationDensityADKE (:32-71): rho with WIJ at HIJ, arho with DWI at the destination's own h (which is its h0: the
// host driver runs the reference's `h = h0` over the destinations before the records are packed), and in finish() the
// post_loop: div, arho = 0, logrho.  The reduce hook -- the sum of logrho and the new h of every row -- is two further
// launches behind this one (run_adke_sd).  Records [x y z h | m u v w]: 64 B in fp64 (four 16-B pieces), 32 B in fp32.
// MINB 4, as FamGasSD_T, of which this is the shorter body: 105..128 VGPRs in fp64 under variable h (the only h it runs
// with), 20 B of scratch in kernel id 10 alone.
enum { F_ASD = 1 };
template <class T> struct FamADKESD_T {
    typedef T Real;
    static constexpr bool PRED = true; // both sums are selected on the criterion
    static constexpr uint32_t CF0 = F_ASD;
    static constexpr int MINB = 4;
    static constexpr int NA = 4; // m u v w
    static constexpr int NR = 8;
    struct Params { double *rho, *arho, *div, *logrho; };
    struct Dest { T u, v, w, rho, arho; };
    template <class A> static __device__ __forceinline__ void load(Dest &D, const T *a, const A &, uint32_t)
    {
        D.u = a[1]; D.v = a[2]; D.w = a[3];
        D.rho = D.arho = T(0.0);
    }
    template <int KK, bool UH, class A>
    static __device__ __forceinline__ void pair(Dest &D, const real4<T> &pi, const real4<T> &pj, T r2,
                                                const T (&s)[NA], uint32_t, const A &a, bool pass = true)
    {
        PairGeomT<T> gij, g;
        pair_geom<KK, UH>(gij, pi, pj, r2, a);
        pair_geom_at<KK, UH>(g, gij, pi.w, a);
        const T wij = pair_w<KK, UH>(gij), tg = pair_gradfac<KK, UH>(g);
        const T mj = s[0];
        const T vijdotdwi = tg * ((D.u - s[1]) * g.xij[0] + (D.v - s[2]) * g.xij[1] + (D.w - s[3]) * g.xij[2]);
        D.rho += pass ? mj * wij : T(0.0);
        D.arho += pass ? mj * vijdotdwi : T(0.0);
    }
    template <class A> static __device__ __forceinline__ void finish(Dest &D, const A &a, uint32_t o)
    {
        const double rho = (double)D.rho;
        a.p.rho[o] = rho;
        a.p.div[o] = -(double)D.arho / rho; // :59-62
        a.p.arho[o] = 0.0;
        a.p.logrho[o] = log(rho);
    }
};

// ADKEAccelerations (:274-353): the pressure term, the Monaghan viscosity under XIJ.VIJ < 0 (HIJ, EPS, RHOIJ1) and the
// conduction Hij of h, cs, div, e of both particles (RHOIJ), all with DWIJ at HIJ.  A source may be a wall row that no
// fluid particle reached (rho = 0, cs = NaN: IdealGasEOS on WallBoundary's raw sums): it is never inside the criterion,
// and the four increments are SELECTED on the criterion, not multiplied by a masked gradient, so that its NaN stays where
// it is.  Records [x y z h | u v w rho p cs e m div -]: 112 B in fp64 (seven 16-B pieces), 64 B in fp32.
// MINB 3, as FamMPM_T: 121..139 VGPRs in fp64 under variable h, no scratch; the budget of four blocks is 128.
enum { F_ADKE = 1 };
template <class T> struct FamADKE_T {
    typedef T Real;
    static constexpr bool PRED = true;
    static constexpr uint32_t CF0 = F_ADKE;
    static constexpr int MINB = 3;
    static constexpr int NA = 9; // u v w rho p cs e m div
    static constexpr int NR = 14;
    struct Params {
        T alpha, beta, g1, g2;
        double *au, *av, *aw, *ae;
    };
    struct Dest {
        T u, v, w, rho, cs, e, div, pib; // pib = p_i / rho_i^2
        T au, av, aw, ae;
    };
    template <class A> static __device__ __forceinline__ void load(Dest &D, const T *a, const A &, uint32_t)
    {
        D.u = a[0]; D.v = a[1]; D.w = a[2]; D.rho = a[3]; D.cs = a[5]; D.e = a[6]; D.div = a[8];
        D.pib = a[4] / (a[3] * a[3]);
        D.au = D.av = D.aw = D.ae = T(0.0);
    }
    template <int KK, bool UH, class A>
    static __device__ __forceinline__ void pair(Dest &D, const real4<T> &pi, const real4<T> &pj, T r2,
                                                const T (&s)[NA], uint32_t, const A &a, bool pass = true)
    {
        PairGeomT<T> g;
        pair_geom<KK, UH>(g, pi, pj, r2, a);
        const T tg = pair_gradfac<KK, UH>(g);
        const T rhoj = s[3], mj = s[7];
        const T pjb = s[4] / (rhoj * rhoj);
        const T cij = T(0.5) * (D.cs + s[5]);
        const T hi = pi.w, hj = pj.w;
        // :319-322: thermal conduction
        const T Hi = a.p.g1 * hi * D.cs + a.p.g2 * hi * hi * (fabs(D.div) - D.div);
        const T Hj = a.p.g1 * hj * s[5] + a.p.g2 * hj * hj * (fabs(s[8]) - s[8]);
        const T rhoij = T(0.5) * (D.rho + rhoj);
        const T r2e = r2 + g.eps;
        const T Hij = (Hi + Hj) * (D.e - s[6]) / (rhoij * r2e);
        const T v0 = D.u - s[0], v1 = D.v - s[1], v2 = D.w - s[2];
        const T xv = g.xij[0] * v0 + g.xij[1] * v1 + g.xij[2] * v2;
        const T muij = g.hij * xv / r2e;
        const T pi_v = muij * (a.p.beta * muij - a.p.alpha * cij) / rhoij; // :324-328
        const T piij = xv < T(0.0) ? pi_v : T(0.0);
        const T tmpv = D.pib + pjb + piij;
        const T f = -mj * tmpv * tg;
        const T vijdotdwij = tg * xv;
        const T xijdotdwij = tg * (g.xij[0] * g.xij[0] + g.xij[1] * g.xij[1] + g.xij[2] * g.xij[2]);
        const T de = T(0.5) * mj * (tmpv * vijdotdwij + T(2.0) * xijdotdwij * Hij);
        D.au += pass ? f * g.xij[0] : T(0.0);
        D.av += pass ? f * g.xij[1] : T(0.0);
        D.aw += pass ? f * g.xij[2] : T(0.0);
        D.ae += pass ? de : T(0.0);
    }
    template <class A> static __device__ __forceinline__ void finish(Dest &D, const A &a, uint32_t o)
    {
        a.p.au[o] = (double)D.au; a.p.av[o] = (double)D.av; a.p.aw[o] = (double)D.aw; a.p.ae[o] = (double)D.ae;
    }
};

// WallBoundary (boundary_equations.py:5-48): the destination is a wall, the sources are the fluids.  Eleven sums with WI
// at the wall row's own h (its h0: the host driver runs `h = h0` first, as for SummationDensityADKE); finish() is the
// post_loop: every sum over wij where wij > 1e-30 and h = htmp / wij there, else the raw sums and h stays h0.  The
// records are FamADKE_T's, [x y z h | u v w rho p cs e m div -], read on the fluids' side only.
// MINB 3: eleven accumulators; up to 136 VGPRs in fp64 under variable h, no scratch; the budget of four blocks is 128.
enum { F_GWALL = 1 };
template <class T> struct FamGasWall_T {
    typedef T Real;
    static constexpr bool PRED = true; // every sum carries WI, selected on the criterion
    static constexpr uint32_t CF0 = F_GWALL;
    static constexpr int MINB = 3;
    static constexpr int NA = 9; // u v w rho p cs e m div
    static constexpr int NR = 14;
    struct Params { double *wij, *p, *u, *v, *w, *m, *rho, *e, *cs, *div, *htmp, *h; };
    struct Dest { T wij, q[9], htmp; };
    template <class A> static __device__ __forceinline__ void load(Dest &D, const T *, const A &, uint32_t)
    {
        D.wij = D.htmp = T(0.0);
        for (int k = 0; k < 9; k++) D.q[k] = T(0.0);
    }
    template <int KK, bool UH, class A>
    static __device__ __forceinline__ void pair(Dest &D, const real4<T> &pi, const real4<T> &pj, T r2,
                                                const T (&s)[NA], uint32_t, const A &a, bool pass = true)
    {
        PairGeomT<T> gij, g;
        pair_geom<KK, UH>(gij, pi, pj, r2, a);
        pair_geom_at<KK, UH>(g, gij, pi.w, a);
        T wi = pair_w<KK, UH>(g);
        wi = pass ? wi : T(0.0);
        D.wij += wi;
#pragma unroll
        for (int k = 0; k < 9; k++) D.q[k] += pass ? s[k] * wi : T(0.0);
        D.htmp += pass ? pj.w * wi : T(0.0);
    }
    template <class A> static __device__ __forceinline__ void finish(Dest &D, const A &a, uint32_t o)
    {
        const double wij = (double)D.wij, htmp = (double)D.htmp;
        const bool reached = wij > 1e-30;
        double q[9];
#pragma unroll
        for (int k = 0; k < 9; k++) q[k] = reached ? (double)D.q[k] / wij : (double)D.q[k];
        a.p.wij[o] = wij;
        a.p.u[o] = -q[0]; a.p.v[o] = -q[1]; a.p.w[o] = -q[2]; // (d_u -= s_u WI)
        a.p.rho[o] = q[3]; a.p.p[o] = q[4]; a.p.cs[o] = q[5]; a.p.e[o] = q[6]; a.p.m[o] = q[7]; a.p.div[o] = q[8];
        a.p.htmp[o] = htmp;
        if (reached) a.p.h[o] = htmp / wij;
    }
};

// ---- Godunov SPH (pysph/sph/gas_dynamics/gsph.py, riemann_solver.py) --------------------------------------------
// GSPHGradients (:61-101): the twelve sums px..pz ux..uz vx..vz wx..wz with DWI, one launch; finish() writes all of
// them, which is the reference's initialize.  Records [x y z h | p u v w m/rho -].
enum { F_GGRAD = 1 };
template <class T> struct FamGSPHGrad_T {
    typedef T Real;
    static constexpr bool PRED = true; // every sum carries DWI, masked for a pair outside the criterion
    static constexpr uint32_t CF0 = F_GGRAD;
    static constexpr int MINB = 3; // (4 spills twelve VGPRs in fp64 under variable h: DESIGN.md section 7h)
    static constexpr int NA = 5; // p u v w m/rho
    static constexpr int NR = 10;
    struct Params { double *g[12]; }; // px py pz ux uy uz vx vy vz wx wy wz
    struct Dest { T q[4]; T g[12]; };
    template <class A> static __device__ __forceinline__ void load(Dest &D, const T *a, const A &, uint32_t)
    {
        for (int k = 0; k < 4; k++) D.q[k] = a[k];
        for (int k = 0; k < 12; k++) D.g[k] = T(0.0);
    }
    template <int KK, bool UH, class A>
    static __device__ __forceinline__ void pair(Dest &D, const real4<T> &pi, const real4<T> &pj, T r2,
                                                const T (&s)[NA], uint32_t, const A &a, bool pass = true)
    {
        PairGeomT<T> gij, g;
        pair_geom<KK, UH>(gij, pi, pj, r2, a);
        pair_geom_at<KK, UH>(g, gij, pi.w, a);
        T tg = pair_gradfac<KK, UH>(g);
        tg = pass ? tg : T(0.0);
        const T dw[3] = {tg * g.xij[0], tg * g.xij[1], tg * g.xij[2]};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const T tmp = s[4] * (s[i] - D.q[i]);
#pragma unroll
            for (int j = 0; j < 3; j++) D.g[3 * i + j] += tmp * dw[j];
        }
    }
    template <class A> static __device__ __forceinline__ void finish(Dest &D, const A &a, uint32_t o)
    {
#pragma unroll
        for (int k = 0; k < 12; k++) a.p.g[k][o] = (double)D.g[k];
    }
};

// The Riemann solvers of riemann_solver.py, in the arithmetic of the sweep.  Each returns 0 with (pstar, ustar) set, or 1
// where the reference's returns 1 WITHOUT writing its result: the caller's zero-initialised pair stands.  No printing.
template <class T> __device__ __forceinline__ T gs_pow(T x, T y);
template <> __device__ __forceinline__ double gs_pow<double>(double x, double y) { return pow(x, y); }
template <> __device__ __forceinline__ float gs_pow<float>(float x, float y) { return powf(x, y); }
template <class T> __device__ __forceinline__ T gs_sign(T x, T y) { return y >= T(0) ? fabs(x) : -fabs(x); } // SIGN :12-16
template <class T> __device__ __forceinline__ T gs_max(T x, T y) { return y > x ? y : x; } // max(x, y) as Python and Cython spell it: x unless y > x
template <class T> __device__ __forceinline__ T gs_min(T x, T y) { return y < x ? y : x; }

template <class T> __device__ __forceinline__ int gs_van_leer(T rhol, T rhor, T pl, T pr, T ul, T ur, T gamma, int niter, T tol, T &ps, T &us)
{ // :54-151
    if (rhol < T(0) || rhor < T(0) || pl < T(0) || pr < T(0)) { ps = T(0); us = T(0); return 1; }
    const T gamma2 = T(1) + gamma, gamma1 = T(0.5) * gamma2 / gamma, smallp = T(1e-25);
    T wl = T(0), wr = T(0), zl, zr, ustar_l, ustar_r;
    const T Vl = T(1) / rhol, Vr = T(1) / rhor;
    const T cl = sqrt(gamma * pl * rhol), cr = sqrt(gamma * pr * rhor);
    T pstar = pr - pl - cr * (ur - ul);
    pstar = pl + pstar * cl / (cl + cr);
    pstar = gs_max(pstar, smallp);
    for (int it = 0; it < niter; it++) {
        const T pstar_old = pstar;
        wl = T(1) + gamma1 * (pstar - pl) / pl;
        wl = cl * sqrt(wl);
        wr = T(1) + gamma1 * (pstar - pr) / pr;
        wr = cr * sqrt(wr);
        zl = T(4) * Vl * wl * wl;
        zl = -zl * wl / (zl - gamma2 * (pstar - pl));
        zr = T(4) * Vr * wr * wr;
        zr = zr * wr / (zr - gamma2 * (pstar - pr));
        ustar_l = ul - (pstar - pl) / wl;
        ustar_r = ur + (pstar - pr) / wr;
        pstar = pstar + (ustar_r - ustar_l) * (zl * zr) / (zr - zl);
        pstar = gs_max(smallp, pstar);
        if (fabs(pstar - pstar_old) / pstar < tol) break;
    }
    ustar_l = ul - (pstar - pl) / wl;
    ustar_r = ur + (pstar - pr) / wr;
    ps = pstar;
    us = T(0.5) * (ustar_l + ustar_r);
    return 0; // (not converged: the reference returns 1 but has written its result)
}

template <class T> __device__ __forceinline__ void gs_prefun(T p, T dk, T pk, T ck, T g1, T g2, T g4, T g5, T g6, T &f, T &fd)
{ // :154-173
    if (p <= pk) {
        const T pratio = p / pk;
        f = g4 * ck * (gs_pow(pratio, g1) - T(1));
        fd = (T(1) / (dk * ck)) * gs_pow(pratio, -g2);
    } else {
        const T ak = g5 / dk, bk = g6 * pk;
        const T qrt = sqrt(ak / (bk + p));
        f = (p - pk) * qrt;
        fd = (T(1) - T(0.5) * (p - pk) / (bk + p)) * qrt;
    }
}

template <class T> __device__ __forceinline__ int gs_exact(T rhol, T rhor, T pl, T pr, T ul, T ur, T gamma, int niter, T tol, T &ps, T &us)
{ // :176-286
    const T tmp1 = T(1) / (T(2) * gamma), tmp2 = T(1) / (gamma - T(1)), tmp3 = T(1) / (gamma + T(1));
    const T gamma1 = (gamma - T(1)) * tmp1, gamma2 = (gamma + T(1)) * tmp1, gamma3 = T(2) * gamma * tmp2, gamma4 = T(2) * tmp2,
            gamma5 = T(2) * tmp3, gamma6 = tmp3 / tmp2, gamma7 = T(0.5) * (gamma - T(1));
    const T cl = sqrt(gamma * pl / rhol), cr = sqrt(gamma * pr / rhor);
    if (gamma4 * (cl + cr) <= (ur - ul)) return 1; // vacuum
    const T cup = T(0.25) * (rhol + rhor) * (cl + cr);
    T ppv = T(0.5) * (pl + pr) + T(0.5) * (ul - ur) * cup;
    const T pmin = gs_min(pl, pr), pmax = gs_max(pl, pr), qmax = pmax / pmin;
    ppv = gs_max(T(0), ppv);
    T pm;
    if (qmax <= T(2) && pmin <= ppv && ppv <= pmax) {
        pm = ppv;
    } else if (ppv < pmin) {
        const T pq = gs_pow(pl / pr, gamma1);
        const T um = (pq * ul / cl + ur / cr + gamma4 * (pq - T(1))) / (pq / cl + T(1) / cr);
        const T ptl = T(1) + gamma7 * (ul - um) / cl, ptr = T(1) + gamma7 * (um - ur) / cr;
        pm = T(0.5) * (pl * gs_pow(ptl, gamma3) + pr * gs_pow(ptr, gamma3));
    } else {
        const T gel = sqrt((gamma5 / rhol) / (gamma6 * pl + ppv)), ger = sqrt((gamma5 / rhor) / (gamma6 * pr + ppv));
        pm = (gel * pl + ger * pr - (ur - ul)) / (gel + ger);
    }
    T pold = pm, p = T(0), fl = T(0), fld = T(0), fr = T(0), frd = T(0);
    const T udiff = ur - ul;
    int last = 0; // the reference's loop index after the loop
    for (int i = 0; i < niter; i++) {
        last = i;
        gs_prefun(pold, rhol, pl, cl, gamma1, gamma2, gamma4, gamma5, gamma6, fl, fld);
        gs_prefun(pold, rhor, pr, cr, gamma1, gamma2, gamma4, gamma5, gamma6, fr, frd);
        p = pold - (fl + fr + udiff) / (fld + frd);
        const T change = T(2) * fabs((p - pold) / (p + pold));
        if (change <= tol) break;
        pold = p;
    }
    if (last == niter - 1) return 1; // (also when it converged in the last iteration allowed: kept)
    ps = p;
    us = T(0.5) * (ul + ur + fr - fl);
    return 0;
}

template <class T> __device__ __forceinline__ int gs_ducowicz(T rhol, T rhor, T pl, T pr, T ul, T ur, T gamma, T &ps, T &us)
{ // :431-525
    // a, b, c and d are differences of products of order (rho cs)^2 that cancel down to order rho p: a fused multiply-add
    // rounds them otherwise than the reference's separately rounded products, and at rho = 1e10, p = 1e20 that moved pstar
    // by more than four times the reference's own distance from the exact value.  Every product here is rounded on its own.
#pragma clang fp contract(off)
    const T al = T(0.5) * (gamma + T(1)), ar = al;
    const T csl = sqrt(gamma * pl * rhol), csr = sqrt(gamma * pr * rhor);
    const T umin = ur - T(0.5) * csr / ar, umax = ul + T(0.5) * csl / al;
    const T plmin = pl - T(0.25) * rhol * csl * csl / al, prmin = pr - T(0.25) * rhor * csr * csr / ar;
    const T bl = rhol * al, br = rhor * ar;
    T a = (br - bl) * (prmin - plmin), b = br * umin * umin - bl * umax * umax, c = br * umin - bl * umax;
    const T d = br * bl * (umin - umax) * (umin - umax);
    auto pstar_of = [&](T ustar) {
#pragma clang fp contract(off)
        const T v = T(0.5) * (plmin + prmin + br * fabs(ustar - umin) * (ustar - umin) - bl * fabs(ustar - umax) * (ustar - umax));
        return gs_max(v, T(0));
    };
    T dd = sqrt(gs_max(T(0), d - a));
    T ustar = (b + prmin - plmin) / (c - gs_sign(dd, umax - umin));
    if ((ustar - umin) >= T(0) && (ustar - umax) <= T(0)) { ps = pstar_of(ustar); us = ustar; return 0; } // case A
    dd = sqrt(gs_max(T(0), d + a));
    ustar = (b - prmin + plmin) / (c - gs_sign(dd, umax - umin));
    if ((ustar - umin) <= T(0) && (ustar - umax) >= T(0)) { ps = pstar_of(ustar); us = ustar; return 0; } // case B
    a = (bl + br) * (plmin - prmin);
    b = bl * umax + br * umin;
    c = T(1) / (bl + br);
    dd = sqrt(gs_max(T(0), a - d));
    ustar = (b + dd) * c;
    if ((ustar - umin) >= T(0) && (ustar - umax) >= T(0)) { ps = pstar_of(ustar); us = ustar; return 0; } // case C
    dd = sqrt(gs_max(T(0), -a - d));
    ustar = (b - dd) * c; // case D
    ps = pstar_of(ustar);
    us = ustar;
    return 0;
}

template <class T> __device__ __forceinline__ int gs_hllc(T rhol, T rhor, T pl, T pr, T ul, T ur, T gamma, T &ps, T &us)
{ // :622-717
    const T gamma1 = T(1) / (gamma - T(1));
    const T rrhol = sqrt(rhol), rrhor = sqrt(rhor);
    const T ulr = (rrhol * ul + rrhor * ur) / (rrhol + rrhor);
    const T vl = ul - ulr, vr = ur - ulr;
    const T csl = sqrt(gamma * pl / rhol), csr = sqrt(gamma * pr / rhor);
    const T cslr = (rrhol * csl + rrhor * csr) / (rrhol + rrhor);
    const T sl = gs_min(vl - csl, T(0) - cslr), sr = gs_max(vr + csr, T(0) + cslr);
    T sm = rhor * vr * (sr - vr) - rhol * vl * (sl - vl) + pl - pr;
    sm /= (rhor * (sr - vr) - rhol * (sl - vl));
    const T phat = rhol * (vl - sl) * (vl - sm) + pl;
    const T el = pl * gamma1 / rhol, El = rhol * (el + T(0.5) * ul * ul);
    const T er = pr * gamma1 / rhor, Er = rhor * (er + T(0.5) * ur * ur);
    const T Ml = rhol * ul, Mr = rhor * ur;
    T pstar, ustar;
    if (sl > T(0)) {
        pstar = pl; ustar = ul;
    } else if (sl <= T(0) && T(0) < sm) {
        const T mstar = T(1) / (sl - sm) * ((sl - vl) * Ml + (phat - pl));
        const T estar = T(1) / (sl - sm) * ((sl - vl) * El - pl * vl + phat * sm);
        pstar = sm * mstar + phat;
        ustar = sm * estar + (sm + ulr) * phat;
        ustar /= pstar;
    } else if (sm <= T(0) && T(0) < sr) {
        const T mstar = T(1) / (sr - sm) * ((sr - vr) * Mr + (phat - pr));
        const T estar = T(1) / (sr - sm) * ((sr - vr) * Er - pr * vr + phat * sm);
        pstar = sm * mstar + phat;
        ustar = sm * estar + (sm + ulr) * phat;
        ustar /= pstar;
    } else if (sr < T(0)) {
        pstar = pr; ustar = ur;
    } else {
        return 1; // "Incorrect wave speeds" (a NaN among them)
    }
    ps = pstar; us = ustar;
    return 0;
}

// riemann_solve (:19-44): `method` is a launch parameter, uniform over the wavefront
template <class T> __device__ __forceinline__ int gs_riemann(int method, T rhol, T rhor, T pl, T pr, T ul, T ur, T gamma, int niter, T tol, T &ps, T &us)
{
    switch (method) {
    case 0: ps = T(0.5) * (pl + pr); us = T(0.5) * (ul + ur); return 0; // non_diffusive :47-51
    case 1: return gs_van_leer(rhol, rhor, pl, pr, ul, ur, gamma, niter, tol, ps, us);
    case 2: return gs_exact(rhol, rhor, pl, pr, ul, ur, gamma, niter, tol, ps, us);
    case 3: return gs_hllc(rhol, rhor, pl, pr, ul, ur, gamma, ps, us);
    case 4: return gs_ducowicz(rhol, rhor, pl, pr, ul, ur, gamma, ps, us);
    case 5: { // hlle :788-851
        const T gamma1 = T(1) / (gamma - T(1));
        const T rrhol = sqrt(rhol), rrhor = sqrt(rhor);
        const T csl = sqrt(gamma * pl * rhol), csr = sqrt(gamma * pr * rhor);
        const T cslr = (rrhol * csl + rrhor * csr) / (rrhol + rrhor);
        const T sl = gs_min(ul - csl, -cslr), sr = gs_max(ur + csr, +cslr);
        const T smax = gs_max(sl, sr), smin = gs_min(sl, sr);
        const T El = pl * gamma1 / rhol + T(0.5) * ul * ul, Er = pr * gamma1 / rhor + T(0.5) * ur * ur;
        const T pstar = (smax * pl - smin * pr) / (smax - smin) + smax * smin / (smax - smin) * (ur - ul);
        const T ustar = (smax * pl * ul - smin * pr * ur) / (smax - smin) + smax * smin / (smax - smin) * (Er - El);
        ps = pstar; us = ustar / pstar;
        return 0;
    }
    case 6: { // roe :528-572
        const T rrhol = sqrt(rhol), rrhor = sqrt(rhor);
        const T denominator = T(1) / (rrhor + rrhol);
        const T plr = (rrhol * pl + rrhor * pr) * denominator;
        const T vlr = (rrhol / rhol + rrhor / rhor) * denominator;
        const T ulr = (rrhol * ul + rrhor * ur) * denominator;
        const T cslr = sqrt(gamma * plr / vlr), cslr1 = T(1) / cslr;
        ps = plr - T(0.5) * (ur - ul) * cslr;
        us = ulr - T(0.5) * (pr - pl) * cslr1;
        return 0;
    }
    case 7: { // llxf :575-619
        const T gamma1 = T(1) / (gamma - T(1));
        const T csl = sqrt(gamma * pl * rhol), csr = sqrt(gamma * pr * rhor);
        const T cslr = gs_max(csr, csl);
        const T El = pl * gamma1 / rhol + T(0.5) * ul * ul, Er = pr * gamma1 / rhor + T(0.5) * ur * ur;
        const T pstar = T(0.5) * (pl + pr - cslr * (ur - ul));
        ps = pstar;
        us = T(1) / pstar * (T(0.5) * ((pl * ul + pr * ur) - cslr * (Er - El)));
        return 0;
    }
    case 8: { // hllc_ball :720-785
        const T gamma1 = T(0.5) * (gamma + T(1)) / gamma;
        const T csl = sqrt(gamma * pl / rhol), csr = sqrt(gamma * pr / rhor), cslr = T(0.5) * (csl + csr);
        const T rholr = T(0.5) * (rhol + rhor);
        T pstar = T(0.5) * (pl + pr - rholr * cslr * (ur - ul));
        const T ustar = T(0.5) * (ul + ur - T(1) / (rholr * cslr) * (pr - pl));
        const T Hl = pstar / pl, Hr = pstar / pr;
        T ql = T(1), qr = T(1);
        if (Hl > T(1)) ql = sqrt(T(1) + gamma1 * (Hl - T(1)));
        if (Hr > T(1)) qr = sqrt(T(1) + gamma1 * (Hr - T(1)));
        const T Sl = ul - csl * ql, Sr = ur + csr * qr;
        const T pstar_l = pl + rhol * (ul - Sl) * (ul - ustar), pstar_r = pr + rhor * (ur - Sr) * (ur - ustar);
        ps = T(0.5) * (pstar_l + pstar_r);
        us = ustar;
        return 0;
    }
    case 9: { // hll_ball :854-913
        const T rrhol = sqrt(rhol), rrhor = sqrt(rhor);
        const T denominator = T(1) / (rrhor + rrhol);
        const T csl = sqrt(gamma * pl / rhol), csr = sqrt(gamma * pr / rhor);
        const T eta = T(0.5) * (gamma - T(1)) * (rrhor * rrhol) * denominator * denominator;
        const T betal = fabs(ul), betar = fabs(ur);
        const T ulr = (rrhol * ul + rrhor * ur) / (rrhol * rrhor);
        const T cslr2 = (rrhol * csl * csl + rrhor * csr * csr) / (rrhol * rrhor);
        const T cslr = sqrt(cslr2 + eta * (betar - betal) * (betar - betal));
        const T Sl = gs_min(ulr - cslr, ul - csl), Sr = gs_max(ulr + cslr, ur + csr);
        const T ustar = (Sr * Sl * (rhor - rhol) + rhol * ul * Sr - rhor * ur * Sl) / (rhol * (ul - Sl) + rhor * (Sr - ur));
        T pstar = pr * (ustar - Sl) - pl * (ustar - Sr) + rhor * ur * (ustar - Sl) * (ur - Sr) - rhol * ul * (ustar - Sr) * (ul - Sl);
        ps = pstar / (Sr - Sl);
        us = ustar;
        return 0;
    }
    case 10: { // hllsy :916-972
        const T gamma1 = T(1) / (gamma - T(1));
        const T rrhol = sqrt(rhol), rrhor = sqrt(rhor);
        const T denominator = T(1) / (rrhor + rrhol);
        const T csl = sqrt(gamma * pl * rhol), csr = sqrt(gamma * pr * rhor);
        const T cslr = denominator * (rrhol * csl + rrhor * csr);
        const T bl = gs_max(csl, cslr), br = gs_max(csr, cslr);
        const T wl = br / (bl + br), wr = bl / (bl + br), wlr = bl * br / (bl + br);
        const T El = pl * gamma1 / rhol + T(0.5) * ul * ul, Er = pr * gamma1 / rhor + T(0.5) * ur * ur;
        const T pstar = wl * pl + wr * pr - wlr * (ur - ul);
        const T ustar = wl * (pl * ul) + wr * (pr * ur) - wlr * (Er - El);
        ps = pstar; us = ustar / pstar;
        return 0;
    }
    default: return 0; // (riemann_solve falls through: the result stays as it was)
    }
}

template <class T> __device__ __forceinline__ T gs_sgn(T x) { return T((x > T(0)) - (x < T(0))); }
template <class T> __device__ __forceinline__ T gs_monotonicity_min(T _x1, T _x2, T _x3)
{ // gsph.py:34-58
    const T x1 = T(2) * fabs(_x1), x2 = fabs(_x2), x3 = T(2) * fabs(_x3);
    const T sx1 = gs_sgn(_x1), sx2 = gs_sgn(_x2), sx3 = gs_sgn(_x3);
    if (sx1 != sx2 || sx2 != sx3) return T(0);
    T m;
    if (x2 < x1) m = x3 < x2 ? x3 : x2;
    else m = x3 < x1 ? x3 : x1;
    return sx1 * m;
}

// GSPHAcceleration (:148-541): the whole loop in one sweep -- local frame, specific-volume interpolation, monotonicity
// limiter, left and right states with their fallbacks, the Riemann solve (and the second one of `hybrid`), au av aw ae with
// DWI and DWJ each at its own h, the ADKE conduction with DWIJ.  Solver, limiter, interpolation, hybrid and conduction are
// launch parameters: branches on them are uniform over the wavefront.  A pair whose solve fails contributes with the zero
// pair and adds one to a device word.  Not PRED: the body is long and, for two solvers, iterates; lanes without a hit wait.
// Records [x y z h | u v w rho p cs m e div grhox grhoy grhoz px py pz ux uy+vx uz+wx vy vz+wy wz -]: a velocity gradient is
// read through eij . G . eij only, so its six symmetric sums are formed once at packing (k_pack, derived 6).
enum { F_GSPH = 1 };
template <class T> struct FamGSPH_T {
    typedef T Real;
    static constexpr bool PRED = false;
    static constexpr uint32_t CF0 = F_GSPH;
    static constexpr int MINB = 2;
    static constexpr int NA = 21;
    static constexpr int NR = 26;
    struct Params {
        T g1, g2, gamma, tol, blend; // blend = exp(-blend_alpha t / tf), computed by the host once per launch
        int monotonicity, rsolver, interpolation, interface_zero, hybrid, niter, conduction;
        double *au, *av, *aw, *ae;
        unsigned long long *fail;
    };
    struct Dest {
        T u, v, w, rho, p, cs, e, div, gr[3], gp[3], gv[6];
        T au, av, aw, ae;
    };
    template <class A> static __device__ __forceinline__ void load(Dest &D, const T *a, const A &, uint32_t)
    {
        D.u = a[0]; D.v = a[1]; D.w = a[2]; D.rho = a[3]; D.p = a[4]; D.cs = a[5]; D.e = a[7]; D.div = a[8];
        for (int k = 0; k < 3; k++) { D.gr[k] = a[9 + k]; D.gp[k] = a[12 + k]; }
        for (int k = 0; k < 6; k++) D.gv[k] = a[15 + k];
        D.au = D.av = D.aw = D.ae = T(0.0);
    }
    template <int KK, bool UH, class A>
    static __device__ __forceinline__ void pair(Dest &D, const real4<T> &pi, const real4<T> &pj, T r2,
                                                const T (&s)[NA], uint32_t, const A &a, bool pass = true)
    {
        if (!pass) return;
        PairGeomT<T> g, gi, gj;
        pair_geom<KK, UH>(g, pi, pj, r2, a);
        pair_geom_at<KK, UH>(gi, g, pi.w, a);
        pair_geom_at<KK, UH>(gj, g, pj.w, a);
        const T ti = pair_gradfac<KK, UH>(gi), tj = pair_gradfac<KK, UH>(gj); // DWI = ti XIJ, DWJ = tj XIJ
        const T hi = pi.w, hj = pj.w, RIJ = g.rij, dt = (T)a.dt;
        T e0 = T(0), e1 = T(0), e2 = T(0), sij; // :237-247
        if (RIJ < T(1e-14)) {
            sij = T(1) / (RIJ + g.eps);
        } else {
            sij = T(1) / RIJ;
            e0 = g.xij[0] * sij; e1 = g.xij[1] * sij; e2 = g.xij[2] * sij;
        }
        const T vl = s[0] * e0 + s[1] * e1 + s[2] * e2;
        const T vr = D.u * e0 + D.v * e1 + D.w * e2;
        const T csi = D.cs, csj = s[5], rhoi = D.rho, rhoj = s[3], p_i = D.p, p_j = s[4];
        // gradients in the local coordinate system (:254-284)
        T rsi = D.gr[0] * e0 + D.gr[1] * e1 + D.gr[2] * e2;
        T rsj = s[9] * e0 + s[10] * e1 + s[11] * e2;
        T psi = D.gp[0] * e0 + D.gp[1] * e1 + D.gp[2] * e2;
        T psj = s[12] * e0 + s[13] * e1 + s[14] * e2;
        T vsi = e0 * e0 * D.gv[0] + e0 * e1 * D.gv[1] + e0 * e2 * D.gv[2] + e1 * e1 * D.gv[3] + e1 * e2 * D.gv[4] + e2 * e2 * D.gv[5];
        T vsj = e0 * e0 * s[15] + e0 * e1 * s[16] + e0 * e2 * s[17] + e1 * e1 * s[18] + e1 * e2 * s[19] + e2 * e2 * s[20];
        // interpolate (:429-541) with sij = RIJ, gri_eij = rsi, grj_eij = rsj
        T vij_i, vij_j, sstar = T(0);
        {
            const T Vi = T(1) / rhoi, Vj = T(1) / rhoj;
            const T hij = T(0.5) * (hi + hj);
            if (a.p.interpolation == 0) {
                vij_i = T(1) / (rhoi * rhoi);
                vij_j = T(1) / (rhoj * rhoj);
            } else if (a.p.interpolation == 1) {
                const T cij = RIJ < T(1e-8) ? T(0) : (Vi - Vj) / RIJ;
                const T dij = T(0.5) * (Vi + Vj);
                vij_i = T(0.25) * hi * hi * cij * cij + dij * dij;
                vij_j = T(0.25) * hj * hj * cij * cij + dij * dij;
                if (!a.p.interface_zero) {
                    const T vij = T(0.5) * (vij_i + vij_j);
                    sstar = T(0.5) * hij * hij * cij * dij / vij;
                }
            } else {
                const T Vip = T(-1) / (rhoi * rhoi) * rsi, Vjp = T(-1) / (rhoj * rhoj) * rsj;
                T aij = T(0), bij = T(0), cij = T(0), dij = T(0.5) * (Vi + Vj);
                if (!(RIJ < T(1e-8))) {
                    aij = T(-2) * (Vi - Vj) / (RIJ * RIJ * RIJ) + (Vip + Vjp) / (RIJ * RIJ);
                    bij = T(0.5) * (Vip - Vjp) / RIJ;
                    cij = T(1.5) * (Vi - Vj) / RIJ - T(0.25) * (Vip + Vjp);
                    dij = T(0.5) * (Vi + Vj) - T(0.125) * (Vip - Vjp) * RIJ;
                }
                const T hi2 = hi * hi, hj2 = hj * hj, hi4 = hi2 * hi2, hj4 = hj2 * hj2, hi6 = hi4 * hi2, hj6 = hj4 * hj2;
                vij_i = T(15.0 / 64.0) * hi6 * aij * aij + T(3.0 / 16.0) * hi4 * (T(2) * aij * cij + bij * bij) +
                        T(0.25) * hi2 * (T(2) * bij * dij + cij * cij) + dij * dij;
                vij_j = T(15.0 / 64.0) * hj6 * aij * aij + T(3.0 / 16.0) * hj4 * (T(2) * aij * cij + bij * bij) +
                        T(0.25) * hj2 * (T(2) * bij * dij + cij * cij) + dij * dij;
                if (!a.p.interface_zero) {
                    const T hij2 = hij * hij, hij4 = hij2 * hij2;
                    const T vij = T(0.5) * (vij_i + vij_j);
                    sstar = (T(15.0 / 32.0) * hij4 * hij2 * aij * bij + T(3.0 / 8.0) * hij4 * (aij * dij + bij * cij) +
                             T(0.5) * hij2 * cij * dij) / vij;
                }
            }
        }
        // monotonicity (:293-349)
        if (a.p.monotonicity == 0) {
            rsi = rsj = psi = psj = vsi = vsj = T(0);
        } else if (a.p.monotonicity == 1) {
            if (vsi * vsj < T(0)) { vsi = T(0); vsj = T(0); }
            if (gs_min(csi, csj) < T(3) * (vl - vr)) rsi = rsj = psi = psj = vsi = vsj = T(0); // first order near a shock
        } else if (a.p.monotonicity == 2) {
            if (RIJ > T(1e-14)) {
                const T qijr = rhoi - rhoj, qijp = p_i - p_j, qiju = vr - vl;
                T delr = rsi * RIJ, delp = psi * RIJ, delv = vsi * RIJ;
                rsi = gs_monotonicity_min(qijr, delr, T(2) * delr - qijr) / RIJ;
                psi = gs_monotonicity_min(qijp, delp, T(2) * delp - qijp) / RIJ;
                vsi = gs_monotonicity_min(qiju, delv, T(2) * delv - qiju) / RIJ;
                delr = rsj * RIJ; delp = psj * RIJ; delv = vsj * RIJ;
                rsj = gs_monotonicity_min(qijr, delr, T(2) * delr - qijr) / RIJ;
                psj = gs_monotonicity_min(qijp, delp, T(2) * delp - qijp) / RIJ;
                vsj = gs_monotonicity_min(qiju, delv, T(2) * delv - qiju) / RIJ;
            } else if (RIJ < T(1e-14)) {
                rsi = rsj = psi = psj = vsi = vsj = T(0);
            }
        }
        // the states either side of the interface (:351-376)
        sstar *= T(2);
        const T fj = T(1) - csj * dt * sij + sstar, fi = T(1) - csi * dt * sij + sstar;
        T rhol = rhoj + T(0.5) * rsj * RIJ * fj;
        T rhor = rhoi - T(0.5) * rsi * RIJ * fi;
        if (rhol < T(0)) rhol = rhoj;
        if (rhor < T(0)) rhor = rhoi;
        T pl = p_j + T(0.5) * psj * RIJ * fj;
        T pr = p_i - T(0.5) * psi * RIJ * fi;
        if (pl < T(0)) pl = p_j;
        if (pr < T(0)) pr = p_i;
        const T ul = vl + T(0.5) * vsj * RIJ * fj;
        const T ur = vr - T(0.5) * vsi * RIJ * fi;
        T pstar = T(0), ustar = T(0);
        int failed = gs_riemann(a.p.rsolver, rhol, rhor, pl, pr, ul, ur, a.p.gamma, a.p.niter, a.p.tol, pstar, ustar);
        if (a.p.hybrid) { // :388-396: the second solve writes into the result of the first
            T pstar2 = pstar, ustar2 = ustar;
            failed += gs_riemann(10, rhoj, rhoi, pl, pr, vl, vr, a.p.gamma, a.p.niter, a.p.tol, pstar2, ustar2);
            ustar = ustar + a.p.blend * (ustar2 - ustar);
            pstar = pstar + a.p.blend * (pstar2 - pstar);
        }
        if (failed) atomicAdd(a.p.fail, 1ull);
        // :398-416
        const T mj = s[6];
        const T ci = vij_i * ti, cj = vij_j * tj;
        const T f = -mj * pstar * (ci + cj);
        D.au += f * g.xij[0]; D.av += f * g.xij[1]; D.aw += f * g.xij[2];
        const T edotx = e0 * g.xij[0] + e1 * g.xij[1] + e2 * g.xij[2];
        D.ae += f * (ustar * edotx);
        if (a.p.conduction) { // :418-427
            const T divi = D.div, divj = s[8];
            const T Hi = a.p.g1 * hi * csi + a.p.g2 * hi * hi * (fabs(divi) - divi);
            const T Hj = a.p.g1 * hj * csj + a.p.g2 * hj * hj * (fabs(divj) - divj);
            T Hij = (Hi + Hj) * (D.e - s[7]);
            Hij /= (T(0.5) * (rhoi + rhoj) * (RIJ * RIJ + g.eps));
            const T tij = pair_gradfac<KK, UH>(g);
            D.ae += mj * Hij * (tij * (g.xij[0] * g.xij[0] + g.xij[1] * g.xij[1] + g.xij[2] * g.xij[2]));
        }
    }
    template <class A> static __device__ __forceinline__ void finish(Dest &D, const A &a, uint32_t o)
    {
        a.p.au[o] = (double)D.au; a.p.av[o] = (double)D.av; a.p.aw[o] = (double)D.aw; a.p.ae[o] = (double)D.ae;
    }
};

// ---- velocity gradient (basic_equations.py:63-148) -------------------------
template <class T> struct FamVGrad_T {
    typedef T Real; // arithmetic type of the pair loop
    static constexpr bool PRED = true; // see FamWCSPH
    static constexpr uint32_t CF0 = F_VG3; // flag set compiled as a constant (variant 6)
    static constexpr int MINB = 4; // wavefronts per SIMD the pair kernel is compiled for (VGPR budget)
    static constexpr int NA = 4; // u v w m/rho
    static constexpr int NR = 8;
    struct Params { double *v[9]; };
    struct Dest { T u, v, w; T g[9]; };
    template <class A> static __device__ __forceinline__ void load(Dest &D, const T *a, const A &, uint32_t)
    {
        D.u = a[0]; D.v = a[1]; D.w = a[2];
        for (int k = 0; k < 9; k++) D.g[k] = T(0.0);
    }
    template <int KK, bool UH, class A>
    static __device__ __forceinline__ void pair(Dest &D, const real4<T> &pi, const real4<T> &pj, T r2,
                                                const T (&s)[NA], uint32_t fl, const A &a, bool pass = true)
    {
        PairGeomT<T> g;
        pair_geom<KK, UH>(g, pi, pj, r2, a);
        T tg = pair_gradfac<KK, UH>(g);
        tg = pass ? tg : T(0.0); // PRED
        const T dw[3] = {tg * g.xij[0], tg * g.xij[1], tg * g.xij[2]};
        const T tmp = s[3]; // m/rho (divided once per particle by k_pack)
        const T nv[3] = {-(D.u - s[0]), -(D.v - s[1]), -(D.w - s[2])};
        const int n = (fl & F_VG3) ? 3 : 2;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++)
                if (i < n && j < n) D.g[3 * i + j] += tmp * nv[i] * dw[j];
    }
    template <class A> static __device__ __forceinline__ void finish(Dest &D, const A &a, uint32_t o)
    {
        const int n = (a.dflags & F_VG3) ? 3 : 2;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++)
                if (i < n && j < n) a.p.v[3 * i + j][o] = D.g[3 * i + j];
    }
};
typedef FamVGrad_T<double> FamVGrad;

// ---- elastic rates: Continuity + MomentumEquationWithStress +
//      MonaghanArtificialViscosity + XSPH  (solid_mech/basic.py:245-387,
//      basic_equations.py:177-300) -------------------------------------------
template <class T> struct FamElastic_T {
    typedef T Real; // arithmetic type of the pair loop
    static constexpr bool PRED = true; // see FamWCSPH
    static constexpr uint32_t CF0 = F_ECONT | F_ESTRESS | F_EAV | F_EXSPH; // flag set compiled as a constant (variant 6)
    // wavefronts per SIMD the pair kernel is compiled for (VGPR budget): fp32 120 registers; fp64 215-227, and at 3
    // (168 registers + 190 B of scratch) the rings take the same 2.99 ms
    static constexpr int MINB = sizeof(T) == 4 ? 4 : 2;
    static constexpr int NA = 18; // u v w m rho cs | t00 t01 t02 t11 t12 t22 (= sigma/rho^2) | r00 r01 r02 r11 r12 r22
    static constexpr int NR = 22;
    struct Params {
        T wdeltap, n, alpha, beta, eps;
        double *arho, *au, *av, *aw, *ax, *ay, *az;
        const uint32_t *tension; // FamElasticU_T: the source array's "a particle is in tension" word, or null (always gather r_ij)
    };
    // The destination's own tensors are NOT live in the pair loop: with S = sum_j m_j DWIJ and F = sum_j m_j f^n DWIJ,
    //   sum_j m_j ((t_i + t_j) + f^n (r_i + r_j)) . DWIJ = t_i . S + r_i . F + sum_j m_j (t_j + f^n r_j) . DWIJ,
    // so t_i, r_i (24 registers in fp64) wait in scratch until finish() and the loop carries S and F (12) instead.
    struct Dest {
        T u, v, w, rho, cs, t[6], r[6];
        T arho, au, av, aw, ax, ay, az;
        T s[3], f[3];
    };
    template <class A> static __device__ __forceinline__ void load(Dest &D, const T *a, const A &, uint32_t)
    {
        D.u = a[0]; D.v = a[1]; D.w = a[2]; D.rho = a[4]; D.cs = a[5];
        for (int k = 0; k < 6; k++) { D.t[k] = a[6 + k]; D.r[k] = a[12 + k]; }
        D.arho = D.au = D.av = D.aw = D.ax = D.ay = D.az = T(0.0);
        for (int k = 0; k < 3; k++) D.s[k] = D.f[k] = T(0.0);
    }
    template <int KK, bool UH, class A>
    static __device__ __forceinline__ void pair(Dest &D, const real4<T> &pi, const real4<T> &pj, T r2,
                                                const T (&s)[NA], uint32_t fl, const A &a, bool pass = true)
    {
        PairGeomT<T> g;
        pair_geom<KK, UH>(g, pi, pj, r2, a);
        T tg = pair_gradfac<KK, UH>(g);
        tg = pass ? tg : T(0.0); // PRED: terms carry DWIJ, the XSPH one WIJ
        const T dw0 = tg * g.xij[0], dw1 = tg * g.xij[1], dw2 = tg * g.xij[2];
        const T vij0 = D.u - s[0], vij1 = D.v - s[1], vij2 = D.w - s[2];
        const T vdotx = vij0 * g.xij[0] + vij1 * g.xij[1] + vij2 * g.xij[2];
        const T mj = s[3];
        if (fl & F_ECONT) D.arho = fma(mj * tg, vdotx, D.arho);
        T wij = T(0.0);
        if (fl & (F_ESTRESS | F_EXSPH)) wij = pair_w<KK, UH>(g);
        wij = pass ? wij : T(0.0);
        if (fl & F_ESTRESS) { // solid_mech/basic.py:267-387
            T fab = T(0.0);
            if (a.p.wdeltap > T(0.)) {
                const T f = wij * fast_rcp(a.p.wdeltap);
                if (a.p.n == T(4.0)) { const T f2 = f * f; fab = f2 * f2; }
                else if (a.p.n == T(2.0)) fab = f * f;
                else if (a.p.n == T(1.0)) fab = f;
                else fab = pow(f, a.p.n);
            }
            const T m0 = mj * dw0, m1 = mj * dw1, m2 = mj * dw2;
            D.s[0] += m0; D.s[1] += m1; D.s[2] += m2;
            D.f[0] = fma(fab, m0, D.f[0]); D.f[1] = fma(fab, m1, D.f[1]); D.f[2] = fma(fab, m2, D.f[2]);
            const T a00 = fma(fab, s[12], s[6]), a01 = fma(fab, s[13], s[7]), a02 = fma(fab, s[14], s[8]);
            const T a11 = fma(fab, s[15], s[9]), a12 = fma(fab, s[16], s[10]), a22 = fma(fab, s[17], s[11]);
            D.au += a00 * m0 + a01 * m1 + a02 * m2;
            D.av += a01 * m0 + a11 * m1 + a12 * m2;
            D.aw += a02 * m0 + a12 * m1 + a22 * m2;
        }
        if (fl & (F_EAV | F_EXSPH)) {
            const T rhoij = T(0.5) * (D.rho + s[4]);
            T rhoij1;
            if (fl & F_EAV) { // basic_equations.py:236-257
                const T re = r2 + g.eps;
                const T tt = fast_rcp(re * rhoij);
                rhoij1 = re * tt;
                const T muij = (g.hij * vdotx) * (rhoij * tt);
                const T cij = T(0.5) * (D.cs + s[5]);
                T piij = (a.p.beta * muij - a.p.alpha * cij) * muij * rhoij1;
                piij = vdotx < 0 ? piij : T(0.0);
                const T f = -mj * piij;
                D.au = fma(f, dw0, D.au); D.av = fma(f, dw1, D.av); D.aw = fma(f, dw2, D.aw);
            } else rhoij1 = fast_rcp(rhoij);
            if (fl & F_EXSPH) { // basic_equations.py:290-295
                const T tmp = -a.p.eps * mj * wij * rhoij1;
                D.ax = fma(tmp, vij0, D.ax); D.ay = fma(tmp, vij1, D.ay); D.az = fma(tmp, vij2, D.az);
            }
        }
    }
    template <class A> static __device__ __forceinline__ void finish(Dest &D, const A &a, uint32_t o)
    {
        if (a.dflags & F_ECONT) a.p.arho[o] = D.arho;
        if (a.dflags & F_ESTRESS) { // the destination's own share of the stress term
            D.au += D.t[0] * D.s[0] + D.t[1] * D.s[1] + D.t[2] * D.s[2] + D.r[0] * D.f[0] + D.r[1] * D.f[1] + D.r[2] * D.f[2];
            D.av += D.t[1] * D.s[0] + D.t[3] * D.s[1] + D.t[4] * D.s[2] + D.r[1] * D.f[0] + D.r[3] * D.f[1] + D.r[4] * D.f[2];
            D.aw += D.t[2] * D.s[0] + D.t[4] * D.s[1] + D.t[5] * D.s[2] + D.r[2] * D.f[0] + D.r[4] * D.f[1] + D.r[5] * D.f[2];
        }
        if (a.dflags & (F_ESTRESS | F_EAV)) { a.p.au[o] = D.au; a.p.av[o] = D.av; a.p.aw[o] = D.aw; }
        if (a.dflags & F_EXSPH) { a.p.ax[o] = D.ax + D.u; a.p.ay[o] = D.ay + D.v; a.p.az[o] = D.az + D.w; }
    }
};
typedef FamElastic_T<double> FamElastic;

// The same terms on records without h and m (uniform h, ONE mass per source array -- seen by the neighbour update's
// reduction, as for the WCSPH uniform-mass records): [x y | z u | v w | rho cs | t00 t01 | t02 t11 | t12 t22 | r00 r01 |
// r02 r11 | r12 r22], 160 bytes = ten 16-B pieces instead of eleven; fp32 [x y z u | v w rho cs | t00 t01 t02 t11 |
// t12 t22 r00 r01 | r02 r11 r12 r22], 80 bytes = five pieces instead of six.
template <class T> struct FamElasticU_T : FamElastic_T<T> {
    static constexpr bool EOSF = true;  // own record decoding (load_fused)
    static constexpr bool TOKEN = true; // wave token: 1 = gather the r_ij, 0 = no particle of the source is in tension (r_ij = 0:
                                        // MonaghanArtificialStress, solid_mech/basic.py:170-242, leaves them zero under compression)
    static constexpr int NA = 18;
    template <class A> static __device__ __forceinline__ uint32_t wave_token(const A &a)
    {
        return a.p.tension ? (uint32_t)__builtin_amdgcn_readfirstlane((int)*a.p.tension) : 1u;
    }
    // 16-B pieces of one record, and the record decoded from wherever its pieces are (the packed buffer, or the LDS copy
    // of a row tile: k_pair_rowlds)
    static constexpr int PIECES = sizeof(T) == 8 ? 10 : 5;
    static constexpr bool ROWLDS = true;
    typedef typename std::conditional<sizeof(T) == 8, double2, float4>::type Piece;
    template <class P> static __device__ __forceinline__ void decode(P p, T mu, real4<T> &pj, T (&s)[18], uint32_t with_r)
    {
        if constexpr (sizeof(T) == 8) {
            double2 q[10];
#pragma unroll
            for (int k = 0; k < 7; k++) q[k] = p[k];
            if (with_r) { q[7] = p[7]; q[8] = p[8]; q[9] = p[9]; }
            else q[7] = q[8] = q[9] = make_double2(0.0, 0.0);
            pj.x = q[0].x; pj.y = q[0].y; pj.z = q[1].x; pj.w = 0.0;
            s[0] = q[1].y; s[1] = q[2].x; s[2] = q[2].y; s[3] = mu; s[4] = q[3].x; s[5] = q[3].y;
#pragma unroll
            for (int k = 0; k < 6; k++) { s[6 + 2 * k] = q[4 + k].x; s[7 + 2 * k] = q[4 + k].y; }
        } else {
            float4 q[5];
#pragma unroll
            for (int k = 0; k < 4; k++) q[k] = p[k];
            if (with_r) q[4] = p[4];
            else { q[4] = make_float4(0.f, 0.f, 0.f, 0.f); q[3].z = 0.f; q[3].w = 0.f; }
            pj.x = q[0].x; pj.y = q[0].y; pj.z = q[0].z; pj.w = 0.f;
            s[0] = q[0].w; s[1] = q[1].x; s[2] = q[1].y; s[3] = mu; s[4] = q[1].z; s[5] = q[1].w;
#pragma unroll
            for (int k = 0; k < 3; k++) { s[6 + 4 * k] = q[2 + k].x; s[7 + 4 * k] = q[2 + k].y; s[8 + 4 * k] = q[2 + k].z; s[9 + 4 * k] = q[2 + k].w; }
        }
    }
    template <class A> static __device__ __forceinline__ void load_fused(const A &a, uint32_t jg, uint32_t, T mu, real4<T> &pj, T (&s)[18],
                                                                         uint32_t with_r = 1u)
    {
        decode(reinterpret_cast<const Piece *>(a.rec) + (unsigned long long)jg * PIECES, mu, pj, s, with_r);
    }
};

// ---------------------------------------------------------------------------
// variant 0: per-lane walk over the 3x3 rows of cells (x-contiguous ranges)
// ---------------------------------------------------------------------------
template <class Fam> __device__ __forceinline__ void load_aux(double (&s)[Fam::NA], const double *__restrict__ p)
{
#pragma unroll
    for (int k = 0; k < Fam::NA; k++) s[k] = p[k];
}

template <class Fam, int KK, bool UH> __global__ __launch_bounds__(256) void k_pair_direct(PairArgs<Fam> a)
{
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.nd) return;
    uint32_t o = a.d_perm[i];
    if (o < a.d_start || o >= a.d_stop) return;
    double4 pi = a.posh[a.d_off + i];
    typename Fam::Dest D;
    Fam::load(D, a.aux + (size_t)(a.d_off + i) * Fam::NA, a, o);
    uint32_t key = a.d_keys[i];
    int cx = key % a.nc[0];
    int t = key / a.nc[0];
    int cy = t % a.nc[1], cz = t / a.nc[1];
    double hi2 = a.radius_scale * pi.w;
    hi2 *= hi2;
    for (int s = 0; s < a.nsrc; s++) {
        const SrcDesc sd = a.src[s];
        for (int oz = -1; oz <= 1; oz++)
            for (int oy = -1; oy <= 1; oy++) {
                int yy = cy + oy, zz = cz + oz;
                if (yy < 0 || yy >= a.nc[1] || zz < 0 || zz >= a.nc[2]) continue;
                int xa = max(cx - 1, 0), xb = min(cx + 1, a.nc[0] - 1);
                uint32_t row = (uint32_t)(a.nc[0] * (yy + a.nc[1] * zz));
                uint32_t j0 = sd.cell_start[row + xa], j1 = sd.cell_start[row + xb + 1];
                for (uint32_t j = j0; j < j1; j++) {
                    double4 pj = a.posh[sd.off + j];
                    double hj2 = a.radius_scale * pj.w;
                    hj2 *= hj2;
                    double r2 = r2_exact(pi.x - pj.x, pi.y - pj.y, pi.z - pj.z);
                    if ((r2 < hi2) || (r2 < hj2)) {
                        double sj[Fam::NA];
                        load_aux<Fam>(sj, a.aux + (size_t)(sd.off + j) * Fam::NA);
                        Fam::template pair<KK, UH>(D, pi, pj, r2, sj, sd.flags, a);
                    }
                }
            }
    }
    Fam::finish(D, a, o);
}

// ---------------------------------------------------------------------------
// host driver
// ---------------------------------------------------------------------------
#if SPH_PRIMARY_UNIT
static bool is_nosrc_kind(int k)
{
    return k == SPH_EQ_TAIT_EOS || k == SPH_EQ_TAIT_EOS_HG || k == SPH_EQ_TVF_STATE_EQUATION ||
           k == SPH_EQ_ISOTHERMAL_EOS || k == SPH_EQ_SOLID_ISOTHERMAL_EOS || k == SPH_EQ_MONAGHAN_ART_STRESS ||
           k == SPH_EQ_HOOKES_DEVIATORIC_STRESS_RATE || k == SPH_EQ_UPDATE_H_FERRARI || k == SPH_EQ_IDEAL_GAS_EOS ||
           k == SPH_EQ_SCALE_SMOOTHING_LENGTH || k == SPH_EQ_UPDATE_H_FROM_VOLUME || k == SPH_EQ_MPM_UPDATE_GHOST_PROPS ||
           k == SPH_EQ_GSPH_UPDATE_GHOST_PROPS || k == SPH_EQ_ADKE_UPDATE_GHOST_PROPS;
}

static int need_prop(sph_ctx *c, int id, int prop, const char *who)
{
    if (!c->arr[id].prop[prop]) {
        sph_set_error("%s: array %d has no device copy of a required property (id %d); push it first", who, id, prop);
        return SPH_ERR_MISSING_PROP;
    }
    return SPH_OK;
}

static int run_nosrc(sph_ctx *c, const sph_equation &e, size_t start, size_t stop)
{
    if (stop <= start) return SPH_OK;
    DevArray &A = c->arr[e.dest];
    EosArgs a;
    a.kind = e.kind;
    memcpy(a.par, e.par, sizeof a.par);
    for (int &gc : a.gcol) gc = 0;
    const bool writes_h = e.kind == SPH_EQ_UPDATE_H_FERRARI || e.kind == SPH_EQ_SCALE_SMOOTHING_LENGTH || e.kind == SPH_EQ_UPDATE_H_FROM_VOLUME;
    if (e.kind == SPH_EQ_MPM_UPDATE_GHOST_PROPS || e.kind == SPH_EQ_ADKE_UPDATE_GHOST_PROPS) {
        const int po = sph_prop_register("orig_idx");
        if (po < 0) return po;
        SPH_TRY(need_prop(c, e.dest, po, "MPMUpdateGhostProps / ADKEUpdateGhostProps (orig_idx)"));
        SPH_TRY(need_prop(c, e.dest, SPH_P, "MPMUpdateGhostProps / ADKEUpdateGhostProps (p)"));
        SPH_TRY(need_prop(c, e.dest, SPH_CS, "MPMUpdateGhostProps / ADKEUpdateGhostProps (cs)"));
        if (e.kind == SPH_EQ_ADKE_UPDATE_GHOST_PROPS) SPH_TRY(need_prop(c, e.dest, SPH_RHO, "ADKEUpdateGhostProps (rho)"));
        a.par[0] = (double)A.n_real;
        a.par[1] = (double)po;
        if (start < A.n_real) start = A.n_real; // nothing to do on the real rows
        if (stop <= start) return SPH_OK;
    } else if (e.kind == SPH_EQ_GSPH_UPDATE_GHOST_PROPS) {
        static const char *names[17] = {"px", "py", "pz", "ux", "uy", "uz", "vx", "vy", "vz", "wx", "wy", "wz",
                                        "grhox", "grhoy", "grhoz", "dwdh", "div"};
        const int po = sph_prop_register("orig_idx");
        if (po < 0) return po;
        SPH_TRY(need_prop(c, e.dest, po, "GSPHUpdateGhostProps (orig_idx)"));
        for (int k = 0; k < 17; k++) { a.gcol[k] = sph_prop_register(names[k]); if (a.gcol[k] < 0) return a.gcol[k]; }
        a.gcol[17] = SPH_RHO; a.gcol[18] = SPH_P; a.gcol[19] = SPH_CS;
        for (int k = 0; k < 20; k++) SPH_TRY(need_prop(c, e.dest, a.gcol[k], "GSPHUpdateGhostProps"));
        a.par[0] = (double)A.n_real;
        a.par[1] = (double)po;
        if (start < A.n_real) start = A.n_real; // nothing to do on the real rows
        if (stop <= start) return SPH_OK;
    } else if (e.kind == SPH_EQ_SCALE_SMOOTHING_LENGTH) {
        SPH_TRY(need_prop(c, e.dest, SPH_H, "ScaleSmoothingLength"));
    } else if (writes_h) { // reads m and rho, writes h
        for (int p : {SPH_RHO, SPH_M, SPH_H}) SPH_TRY(need_prop(c, e.dest, p, "UpdateSmoothingLengthFerrari / FromVolume"));
    } else if (e.kind != SPH_EQ_HOOKES_DEVIATORIC_STRESS_RATE) { // (reads v_ij, s_ij and G only: alone in a group, rho and p are not on the device)
        SPH_TRY(need_prop(c, e.dest, SPH_RHO, "EOS"));
        SPH_TRY(sph_array_ensure_prop(c, e.dest, SPH_P));
    }
    a.rho = A.prop[SPH_RHO];
    a.p = A.prop[SPH_P];
    a.cs = nullptr;
    if (e.kind == SPH_EQ_IDEAL_GAS_EOS) SPH_TRY(need_prop(c, e.dest, SPH_E, "IdealGasEOS"));
    if (e.kind == SPH_EQ_TAIT_EOS || e.kind == SPH_EQ_TAIT_EOS_HG || e.kind == SPH_EQ_IDEAL_GAS_EOS) {
        SPH_TRY(sph_array_ensure_prop(c, e.dest, SPH_CS));
        a.cs = A.prop[SPH_CS];
    }
    a.start = start;
    a.stop = stop;
    if (e.kind == SPH_EQ_MONAGHAN_ART_STRESS) {
        for (int p : {SPH_S00, SPH_S01, SPH_S02, SPH_S11, SPH_S12, SPH_S22}) SPH_TRY(need_prop(c, e.dest, p, "MonaghanArtificialStress"));
        for (int p : {SPH_R00, SPH_R01, SPH_R02, SPH_R11, SPH_R12, SPH_R22}) SPH_TRY(sph_array_ensure_prop(c, e.dest, p));
    }
    if (e.kind == SPH_EQ_HOOKES_DEVIATORIC_STRESS_RATE) {
        for (int p : {SPH_S00, SPH_S01, SPH_S02, SPH_S11, SPH_S12, SPH_S22}) SPH_TRY(need_prop(c, e.dest, p, "HookesDeviatoricStressRate"));
        for (int p : {SPH_V00, SPH_V01, SPH_V02, SPH_V10, SPH_V11, SPH_V12, SPH_V20, SPH_V21, SPH_V22, SPH_AS00, SPH_AS01, SPH_AS02,
                      SPH_AS11, SPH_AS12, SPH_AS22})
            SPH_TRY(sph_array_ensure_prop(c, e.dest, p));
    }
    for (int k = 0; k < SPH_PROP_COUNT; k++) a.q[k] = A.prop[k];
    a.rho = A.prop[SPH_RHO];
    a.p = A.prop[SPH_P];
    if (e.kind == SPH_EQ_MPM_UPDATE_GHOST_PROPS || e.kind == SPH_EQ_ADKE_UPDATE_GHOST_PROPS) a.cs = A.prop[SPH_CS];
    a.tflag = nullptr;
    if (e.kind == SPH_EQ_MONAGHAN_ART_STRESS) {
        // "no particle in tension" for the rates kernel: valid when this launch covers every particle of the array
        SPH_TRY(A.tflag.reserve(64));
        if (start == 0) HIP_TRY(hipMemsetAsync(A.tflag.ptr, 0, 4, c->stream)); // (a phase-2 launch over the ghosts only adds to the word)
        a.tflag = A.tflag.as<uint32_t>();
        A.tflag_valid = (start == 0 && stop == A.n) || (A.tflag_valid && start <= A.n_binned && stop == A.n);
    }
    ScopedTimer tm(c, T_EOS);
    hipLaunchKernelGGL(k_nosrc, dim3(div_up(stop - start, 256)), dim3(256), 0, c->stream, a);
    if (writes_h) {
        // h changed behind the neighbour grid: the next sph_nnps_update looks at the values again, and until then no
        // pair loop may take "every particle has the h the last update saw" as a launch constant or a record layout
        sph_mark_written(A, SPH_H);
        c->uniform_h = false;
    }
    return SPH_OK;
}

enum Family { FAM_NONE, FAM_WCSPH, FAM_DENSITY, FAM_TVF, FAM_VGRAD, FAM_ELASTIC, FAM_NBR, FAM_WCSPHX, FAM_DSPRE, FAM_EDAC, FAM_AVGP, FAM_GASSD, FAM_MPM,
              FAM_GSPHGRAD, FAM_GSPH, FAM_ADKESD, FAM_ADKE, FAM_GASWALL };

static bool is_wcsph_option_kind(int k)
{
    return k == SPH_EQ_CONTINUITY_DELTA_SPH || k == SPH_EQ_MOMENTUM_DELTA_SPH || k == SPH_EQ_LAMINAR_VISCOSITY ||
           k == SPH_EQ_LAMINAR_VISCOSITY_DELTA_SPH;
}

static bool is_edac_force_kind(int k) { return k == SPH_EQ_EDAC_MOMENTUM || k == SPH_EQ_EDAC_MOM_PRESSURE || k == SPH_EQ_EDAC; }

// wcsphx: the destination carries a delta-SPH or laminar-viscosity term: its Continuity / Momentum / XSPH go with it
// edac: it carries an EDAC force equation: the TVF viscosity / artificial viscosity / artificial stress and XSPH go with it
// avgp: it carries ComputeAveragePressure: a density summation goes with it
static int eq_family(int kind, uint32_t *flag, bool elastic, bool wcsphx = false, bool edac = false, bool avgp = false)
{
    switch (kind) {
    case SPH_EQ_EDAC_MOMENTUM: *flag = F_EP; return FAM_EDAC;
    case SPH_EQ_EDAC_MOM_PRESSURE: *flag = F_EP | F_EINT; return FAM_EDAC;
    case SPH_EQ_EDAC: *flag = F_EDAC; return FAM_EDAC;
    case SPH_EQ_EDAC_AVG_PRESSURE: *flag = F_AVGP; return FAM_AVGP;
    case SPH_EQ_GASD_SUMMATION_DENSITY: *flag = F_GSD; return FAM_GASSD;
    case SPH_EQ_MPM_ACCELERATIONS: *flag = F_MPM; return FAM_MPM;
    case SPH_EQ_GSPH_GRADIENTS: *flag = F_GGRAD; return FAM_GSPHGRAD;
    case SPH_EQ_GSPH_ACCELERATION: *flag = F_GSPH; return FAM_GSPH;
    case SPH_EQ_SUMMATION_DENSITY_ADKE: *flag = F_ASD; return FAM_ADKESD;
    case SPH_EQ_ADKE_ACCELERATIONS: *flag = F_ADKE; return FAM_ADKE;
    case SPH_EQ_GASD_WALL_BOUNDARY: *flag = F_GWALL; return FAM_GASWALL;
    default: break;
    }
    if (edac && !elastic) {
        switch (kind) {
        case SPH_EQ_TVF_MOM_VISCOSITY: *flag = F_TVISC; return FAM_EDAC;
        case SPH_EQ_TVF_MOM_ART_VISCOSITY: *flag = F_TAV; return FAM_EDAC;
        case SPH_EQ_TVF_MOM_ART_STRESS: *flag = F_TAS; return FAM_EDAC;
        case SPH_EQ_XSPH: *flag = F_EXS; return FAM_EDAC;
        default: break;
        }
    }
    if (avgp) {
        switch (kind) {
        case SPH_EQ_SUMMATION_DENSITY: *flag = F_SD; return FAM_AVGP;
        case SPH_EQ_TVF_SUMMATION_DENSITY: *flag = F_TVFSD; return FAM_AVGP;
        default: break;
        }
    }
    switch (kind) {
    case SPH_EQ_CONTINUITY_DELTA_SPH: *flag = F_DCONT; return FAM_WCSPHX;
    case SPH_EQ_MOMENTUM_DELTA_SPH: *flag = F_DMOM; return FAM_WCSPHX;
    case SPH_EQ_LAMINAR_VISCOSITY: *flag = F_LAM; return FAM_WCSPHX;
    case SPH_EQ_LAMINAR_VISCOSITY_DELTA_SPH: *flag = F_LAMD; return FAM_WCSPHX;
    case SPH_EQ_GRADIENT_CORRECTION_PRESTEP: *flag = F_MOMENT; return FAM_DSPRE;
    case SPH_EQ_GRADIENT_CORRECTION: *flag = F_GCORR; return FAM_DSPRE;
    case SPH_EQ_CONTINUITY_DELTA_SPH_PRESTEP: *flag = F_GRADRHO; return FAM_DSPRE;
    default: break;
    }
    if (wcsphx && !elastic) {
        switch (kind) {
        case SPH_EQ_CONTINUITY: *flag = F_CONT; return FAM_WCSPHX;
        case SPH_EQ_MOMENTUM: *flag = F_MOM; return FAM_WCSPHX;
        case SPH_EQ_XSPH: *flag = F_XSPH; return FAM_WCSPHX;
        default: break;
        }
    }
    if (elastic) {
        switch (kind) {
        case SPH_EQ_CONTINUITY: *flag = F_ECONT; return FAM_ELASTIC;
        case SPH_EQ_MOMENTUM_WITH_STRESS: *flag = F_ESTRESS; return FAM_ELASTIC;
        case SPH_EQ_MONAGHAN_ART_VISCOSITY: *flag = F_EAV; return FAM_ELASTIC;
        case SPH_EQ_XSPH: *flag = F_EXSPH; return FAM_ELASTIC;
        default: break;
        }
    }
    switch (kind) {
    case SPH_EQ_CONTINUITY: *flag = F_CONT; return FAM_WCSPH;
    case SPH_EQ_MOMENTUM: *flag = F_MOM; return FAM_WCSPH;
    case SPH_EQ_XSPH: *flag = F_XSPH; return FAM_WCSPH;
    case SPH_EQ_SUMMATION_DENSITY: *flag = F_SD; return FAM_DENSITY;
    case SPH_EQ_TVF_SUMMATION_DENSITY: *flag = F_TVFSD; return FAM_DENSITY;
    case SPH_EQ_TVF_MOM_PRESSURE: *flag = F_TP; return FAM_TVF;
    case SPH_EQ_TVF_MOM_VISCOSITY: *flag = F_TVISC; return FAM_TVF;
    case SPH_EQ_TVF_MOM_ART_VISCOSITY: *flag = F_TAV; return FAM_TVF;
    case SPH_EQ_TVF_MOM_ART_STRESS: *flag = F_TAS; return FAM_TVF;
    case SPH_EQ_VELOCITY_GRADIENT_2D: *flag = F_VG2; return FAM_VGRAD;
    case SPH_EQ_VELOCITY_GRADIENT_3D: *flag = F_VG3; return FAM_VGRAD;
    default: return FAM_NONE;
    }
}

struct PackPlan {
    int nr; // doubles per interleaved record (== Fam::NR)
    int na;
    int props[MAX_AUX]; // sph_prop or -1
    int derived;
};

static PackPlan pack_plan(int fam)
{
    PackPlan p;
    for (auto &v : p.props) v = -1;
    p.derived = 0;
    if (fam == FAM_WCSPH) {
        p.nr = FamWCSPH::NR;
        p.na = 8;
        int pr[8] = {SPH_U, SPH_V, SPH_W, SPH_M, SPH_RHO, -1, SPH_CS, SPH_P};
        for (int k = 0; k < 8; k++) p.props[k] = pr[k];
        p.derived = 1;
    } else if (fam == FAM_WCSPHX) { // the WCSPH slots; with a delta-SPH continuity term (sph_eval_group) + gradrho
        p.nr = 12;
        p.na = 8;
        int pr[8] = {SPH_U, SPH_V, SPH_W, SPH_M, SPH_RHO, -1, SPH_CS, SPH_P};
        for (int k = 0; k < 8; k++) p.props[k] = pr[k];
        p.derived = 1;
    } else if (fam == FAM_DSPRE) {
        p.nr = 6;
        p.na = 2;
        p.props[0] = SPH_M; p.props[1] = SPH_RHO;
    } else if (fam == FAM_DENSITY) {
        p.nr = FamDensity::NR;
        p.na = 1;
        p.props[0] = SPH_M;
    } else if (fam == FAM_AVGP) {
        p.nr = 6;
        p.na = 2;
        p.props[0] = SPH_M; p.props[1] = SPH_P;
    } else if (fam == FAM_GASSD || fam == FAM_ADKESD) {
        p.nr = 8;
        p.na = 4;
        int pr[4] = {SPH_M, SPH_U, SPH_V, SPH_W};
        for (int k = 0; k < 4; k++) p.props[k] = pr[k];
    } else if (fam == FAM_MPM) { // omega, alpha1, alpha2: user properties by name (run_mpm refuses the launch should the slots have run out)
        p.nr = 16;
        p.na = 12;
        int pr[12] = {SPH_U, SPH_V, SPH_W, SPH_RHO, SPH_P, SPH_CS, SPH_E, SPH_M, sph_prop_register("omega"),
                      sph_prop_register("alpha1"), sph_prop_register("alpha2"), -1};
        for (int k = 0; k < 12; k++) p.props[k] = pr[k];
    } else if (fam == FAM_ADKE || fam == FAM_GASWALL) { // div: a user property by name (the binders refuse the launch should the slots have run out)
        p.nr = 14;
        p.na = 9;
        int pr[9] = {SPH_U, SPH_V, SPH_W, SPH_RHO, SPH_P, SPH_CS, SPH_E, SPH_M, sph_prop_register("div")};
        for (int k = 0; k < 9; k++) p.props[k] = pr[k];
    } else if (fam == FAM_GSPHGRAD) { // [p u v w m/rho]
        p.nr = 10;
        p.na = 5;
        int pr[6] = {SPH_P, SPH_U, SPH_V, SPH_W, SPH_M, SPH_RHO};
        for (int k = 0; k < 6; k++) p.props[k] = pr[k];
        p.derived = 7;
    } else if (fam == FAM_GSPH) { // the gradients: user properties by name (run_gsph refuses the launch should the slots have run out)
        p.nr = 26;
        p.na = 21;
        static const char *un[16] = {"div", "grhox", "grhoy", "grhoz", "px", "py", "pz", "ux", "uy", "uz", "vx", "vy", "vz", "wx", "wy", "wz"};
        int pr[8] = {SPH_U, SPH_V, SPH_W, SPH_RHO, SPH_P, SPH_CS, SPH_M, SPH_E};
        for (int k = 0; k < 8; k++) p.props[k] = pr[k];
        for (int k = 0; k < 16; k++) p.props[8 + k] = sph_prop_register(un[k]);
        p.derived = 6;
    } else if (fam == FAM_NBR) {
        p.nr = FamNbr::NR;
        p.na = 1;
        p.derived = 5; // aux[0] = the particle's original index
    } else if (fam == FAM_VGRAD) {
        p.nr = FamVGrad::NR;
        p.na = 4;
        int pr[5] = {SPH_U, SPH_V, SPH_W, SPH_M, SPH_RHO};
        for (int k = 0; k < 5; k++) p.props[k] = pr[k];
        p.derived = 4;
    } else if (fam == FAM_ELASTIC) {
        p.nr = FamElastic::NR;
        p.na = 18;
        int pr[19] = {SPH_U, SPH_V, SPH_W, SPH_M, SPH_RHO, SPH_CS, SPH_S00, SPH_S01, SPH_S02, SPH_S11, SPH_S12, SPH_S22,
                      SPH_R00, SPH_R01, SPH_R02, SPH_R11, SPH_R12, SPH_R22, SPH_P};
        for (int k = 0; k < 19; k++) p.props[k] = pr[k];
        p.derived = 3;
    } else { // FAM_TVF and FAM_EDAC
        p.nr = FamTVF::NR;
        p.na = 12;
        int pr[12] = {SPH_U, SPH_V, SPH_W, SPH_UHAT, SPH_VHAT, SPH_WHAT, SPH_RHO, SPH_P, SPH_VOL, SPH_M, -1, -1};
        for (int k = 0; k < 12; k++) p.props[k] = pr[k];
        p.derived = 2;
    }
    return p;
}

// The packed records of one (destination, sources) block.  choose_records decides them for a destination of
// sph_eval_group; the callers that are fp64 by contract (neighbour lists, the interpolator) start from RecordLayout(fam),
// whatever the options say.  pack_array, the pack cache, fill_common and the choice of the family instantiation read the
// decision from here and from nowhere else.
enum RecordKind {
    REC_PLAIN, // the family's own records (PackPlan; compact under uniform h where pack_layout has a layout for them)
    REC_EOSF,  // 64-byte WCSPH records, uniform h: p and cs recomputed per record (sph_group.src_eos)
    REC_EOSV,  // 64-byte WCSPH records with variable h [x y z h u v w rho], one mass per source array
    REC_TVFF,  // state-fused TVF records: p and V recomputed from rho
    REC_ELU,   // elastic-rates records without h and m (uniform h, one mass per source array)
};
struct RecordLayout {
    PackPlan pl;             // nr: doubles per record (floats with record_f32 / arith_f32)
    bool record_f32 = false; // the precision, as the options of these names: fp32 records read by fp64 arithmetic ...
    bool arith_f32 = false;  // ... fp32 records, arithmetic and accumulators
    RecordKind kind = REC_PLAIN;
    bool umass = false;      // REC_EOSF: p / rho^2 in the mass slot (every source array has one mass)
    bool eos_abs = false;    // REC_EOSF / REC_EOSV: the pack computes the Tait EOS that has not run (PackArgs::eos_abs) ...
    double eos_par[4] = {};  // ... with these parameters: rho0 c0 gamma p0
    explicit RecordLayout(int fam) : pl(pack_plan(fam)) {}
    bool eos_fused() const { return kind == REC_EOSF || kind == REC_EOSV; }
    // what the pack cache compares: records packed under another signature cannot be reused
    int sig() const
    {
        return pl.nr * 32 + (record_f32 ? 1 : 0) + (arith_f32 ? 2 : 0) + (kind == REC_EOSF ? 4 : 0) + (umass ? 8 : 0) +
               (kind == REC_TVFF || kind == REC_ELU || kind == REC_EOSV ? 16 : 0);
    }
};

// PackArgs::layout of these records
static int pack_layout(const RecordLayout &rl, int fam, bool wave)
{
    static const int special[] = {0, 6, 12, 8, 10}; // by RecordKind, in fp64; the fp32 form of each is the next number
    if (rl.kind != REC_PLAIN) return special[rl.kind] + (rl.arith_f32 ? 1 : 0);
    if (!wave) return 0;
    if (rl.record_f32 || rl.arith_f32) return 5;
    if (fam == FAM_WCSPH) return 1;
    if ((fam == FAM_DENSITY || fam == FAM_NBR) && rl.pl.nr == 4) return 2;
    if ((fam == FAM_TVF || fam == FAM_EDAC) && (rl.pl.nr == 14 || rl.pl.nr == 12)) return 3;
    return 0;
}

// which aux slots a family really needs given the union of flags (others may be absent -> 0)
static bool slot_required(int fam, uint32_t flags, int prop)
{
    if (fam == FAM_WCSPH) {
        if (prop == SPH_M || prop == SPH_U || prop == SPH_V || prop == SPH_W) return true;
        if (prop == SPH_RHO) return flags & (F_MOM | F_XSPH);
        if (prop == SPH_P || prop == SPH_CS) return flags & F_MOM;
        return false;
    }
    if (fam == FAM_WCSPHX) {
        if (prop == SPH_M || prop == SPH_U || prop == SPH_V || prop == SPH_W || prop == SPH_RHO) return true;
        if (prop == SPH_P || prop == SPH_CS) return flags & F_MOM;
        return flags & F_DCONT; // SPH_GRADRHO0..2
    }
    if (fam == FAM_DSPRE) return true;
    if (fam == FAM_DENSITY) return prop == SPH_M;
    if (fam == FAM_NBR) return false;
    if (fam == FAM_VGRAD) return true;
    if (fam == FAM_ELASTIC) {
        if (prop == SPH_U || prop == SPH_V || prop == SPH_W || prop == SPH_M) return true;
        if (prop == SPH_RHO) return flags & (F_ESTRESS | F_EAV | F_EXSPH);
        if (prop == SPH_CS) return flags & F_EAV;
        if (prop == SPH_P) return flags & F_ESTRESS;
        if (prop >= SPH_S00 && prop <= SPH_S22) return flags & F_ESTRESS;
        return false; // r_ij default to 0 when absent
    }
    if (fam == FAM_TVF || fam == FAM_EDAC) {
        if (prop == SPH_UHAT || prop == SPH_VHAT || prop == SPH_WHAT) return flags & F_TAS;
        return true;
    }
    if (fam == FAM_AVGP) return prop == SPH_M ? (flags & (F_SD | F_TVFSD)) != 0 : (flags & F_AVGP) != 0;
    if (fam == FAM_GASSD || fam == FAM_MPM || fam == FAM_GSPHGRAD || fam == FAM_GSPH) return true;
    if (fam == FAM_ADKESD || fam == FAM_ADKE || fam == FAM_GASWALL) return true;
    return false;
}

// 16-B pieces of one packed record, as k_pack counts them; 0: records that are not a whole number of
// pieces (no LDS transposition, per-lane stores)
static int pack_pieces(const PackArgs &pa)
{
    if (!pa.rec) return 0;
    // values per piece: four floats (layout 5 and the odd ones of 7 .. 13) or two doubles
    const int per = (pa.layout == 5 || (pa.layout >= 7 && pa.layout <= 13 && (pa.layout & 1))) ? 4 : 2;
    return (pa.nr % per) ? 0 : pa.nr / per;
}

// `launch` false: validate only (the records of this array are already in the packed buffer, see
// the pack cache in sph_eval_group)
// k_pack with the layout as a compile-time constant where the library has an instantiation
static void launch_pack(sph_ctx *c, const PackArgs &pa, size_t n)
{
    const dim3 g(div_up(n, 256)), b(256);
    const size_t lds = (size_t)pa.lds_np * 256 * 16;
    switch (pa.rec ? pa.layout : -1) {
    case 2: hipLaunchKernelGGL(k_pack<2>, g, b, lds, c->stream, pa); break;
    case 3: hipLaunchKernelGGL(k_pack<3>, g, b, lds, c->stream, pa); break;
    case 8: hipLaunchKernelGGL(k_pack<8>, g, b, lds, c->stream, pa); break;
    case 9: hipLaunchKernelGGL(k_pack<9>, g, b, lds, c->stream, pa); break;
    case 6: hipLaunchKernelGGL(k_pack<6>, g, b, lds, c->stream, pa); break;
    case 7: hipLaunchKernelGGL(k_pack<7>, g, b, lds, c->stream, pa); break;
    case 10: hipLaunchKernelGGL(k_pack<10>, g, b, lds, c->stream, pa); break;
    case 11: hipLaunchKernelGGL(k_pack<11>, g, b, lds, c->stream, pa); break;
    case 12: hipLaunchKernelGGL(k_pack<12>, g, b, lds, c->stream, pa); break;
    case 13: hipLaunchKernelGGL(k_pack<13>, g, b, lds, c->stream, pa); break;
    default: hipLaunchKernelGGL(k_pack<-1>, g, b, lds, c->stream, pa); break;
    }
}

static int pack_array(sph_ctx *c, int id, size_t off, const RecordLayout &rl, int fam, uint32_t flags, bool dest_only = false,
                      bool launch = true, int seg = 0)
{
    DevArray &A = c->arr[id];
    const PackPlan &pl = rl.pl;
    // seg 0: the particles sph_nnps_update binned, through their cell order; seg 1: the ghosts binned after it
    // (sph_nnps_update_ghosts), through theirs, behind the first segment's records
    const size_t nseg = seg ? A.g_n : A.n_binned;
    if (nseg == 0) return SPH_OK;
    PackArgs pa;
    memset(&pa, 0, sizeof pa);
    pa.perm = seg ? A.g_perm.as<uint32_t>() : A.perm.as<uint32_t>();
    pa.n = nseg;
    pa.off = off + (seg ? A.n_binned : 0);
    pa.x = A.prop[SPH_X]; pa.y = A.prop[SPH_Y]; pa.z = A.prop[SPH_Z]; pa.h = A.prop[SPH_H];
    pa.na = pl.na;
    for (int k = 0; k < MAX_AUX; k++) {
        if ((k < pl.na || (pl.derived == 3 && k == 18) || (pl.derived == 4 && k == 4) || (pl.derived == 6 && k < 24) ||
             (pl.derived == 7 && k == 5)) && pl.props[k] >= 0) {
            pa.src[k] = A.prop[pl.props[k]];
            // a destination that is not among the sources is only read through Fam::load:
            // it does not need a mass unless the equation uses the destination's own
            // (transport_velocity.SummationDensity: rho_i = m_i sum W)
            const bool mass_free = dest_only && pl.props[k] == SPH_M &&
                                   (fam == FAM_WCSPH || fam == FAM_WCSPHX || (fam == FAM_DENSITY && !(flags & F_TVFSD)));
            if (!pa.src[k] && !mass_free && slot_required(fam, flags, pl.props[k])) return need_prop(c, id, pl.props[k], "pair loop");
        }
    }
    pa.derived = pl.derived;
    pa.posh = c->posh.as<double4>();
    pa.aux = c->aux.as<double>();
    pa.rec = wave_tiles(c) ? c->posh.as<double>() : nullptr;
    pa.nr = pl.nr;
    pa.fpos = wave_tiles(c) ? c->fposb.as<float4>() : nullptr;
    for (int k = 0; k < 3; k++) pa.gmin[k] = c->xmin[k];
    pa.radius_scale = c->radius_scale;
    pa.layout = pack_layout(rl, fam, wave_tiles(c));
    if (rl.kind == REC_EOSF) {
        // p, cs (and p / rho^2) are recomputed by the pair kernel: not read here
        pa.src[5] = pa.src[6] = nullptr;
        if (rl.umass) { // ... except p / rho^2, which takes the place of the (uniform) mass: derived 1 reads p
            pa.umass = 1;
            pa.src[3] = nullptr; // the record holds no mass
        } else {
            pa.src[7] = nullptr;
            pa.derived = 0;
        }
        // ... and no h: the prefilter's radius_scale * h from the launch constant of the pair kernel (fill_common: hu)
        pa.h = nullptr;
        pa.hu = 0.5 * (c->h_uniform + c->h_uniform);
    }
    // REC_ELU: h and m are launch / source constants
    if (rl.kind == REC_EOSV) { // p, cs, p / rho^2 recomputed, m a source constant: none of them read here
        pa.src[3] = pa.src[5] = pa.src[6] = pa.src[7] = nullptr;
        pa.derived = 0;
    }
    if (rl.kind == REC_TVFF) { // p and V are functions of rho (and the one mass): not read here
        pa.src[7] = pa.src[8] = pa.src[9] = nullptr;
        pa.derived = 0;
    }
    if (rl.eos_abs) { // the Tait EOS of this array has not run: p and cs leave from here
        pa.eos_abs = 1;
        for (int k = 0; k < 4; k++) pa.eos_par[k] = rl.eos_par[k];
        pa.p_out = A.prop[SPH_P];
        pa.cs_out = A.prop[SPH_CS];
        pa.src[7] = nullptr; // p is computed, not read
    }
    pa.lds_np = pack_pieces(pa);
    if ((size_t)pa.lds_np * 256 * 16 > 48 * 1024) pa.lds_np = 0; // the widest records (GSPH, 13 pieces) leave per lane
    if (launch) launch_pack(c, pa, nseg);
    return SPH_OK;
}

#endif // SPH_PRIMARY_UNIT

// ---------------------------------------------------------------------------
// launch entry points, one smoothing kernel each.  The pair kernels of SphKernel<1..4> are instantiated by the primary
// compile of this file; those of SphKernel<5..10> by one further compile per id (-DSPH_KERNEL_UNIT=<id>, Makefile),
// which emits nothing but the externally linked *_ext functions below for the families listed at the end of the
// file.  The primary compile only declares them and forwards ids 5..10.
// ---------------------------------------------------------------------------
// rec_f32: an fp64 family reads fp32 records (RecordLayout::record_f32)
template <class Fam, int K> static int launch_pair_k(sph_ctx *c, const PairArgs<Fam> &a, bool rec_f32)
{
    const bool uh = c->uniform_h && c->use_uniform_h;
    constexpr bool FP32 = sizeof(typename Fam::Real) == 4;
    if (wave_tiles(c)) {
        dim3 g2(div_up(4 * div_up(a.nd, 256), WPB)), b2(64 * WPB);
        // equation flags as a compile-time constant when every source carries the same set
        uint32_t cf = a.src[0].flags;
        for (int j = 1; j < a.nsrc; j++) if (a.src[j].flags != cf) cf = 0;
        if (c->const_flags == 0) cf = 0;
#define LAUNCH6F(UHV, F32V, CFV) hipLaunchKernelGGL((k_pair_wave<Fam, K, UHV, F32V, CFV>), g2, b2, (size_t)c->lds_pad, c->stream, a)
#define LAUNCH6U(F32V)                                                                              \
        if (uh) { if (cf == Fam::CF0) LAUNCH6F(true, F32V, Fam::CF0); else LAUNCH6F(true, F32V, 0); }  \
        else { if (cf == Fam::CF0) LAUNCH6F(false, F32V, Fam::CF0); else LAUNCH6F(false, F32V, 0); }
        if constexpr (FP32) { LAUNCH6U(true) }
        else { if (rec_f32) { LAUNCH6U(true) } else { LAUNCH6U(false) } }
#undef LAUNCH6U
#undef LAUNCH6F
        return SPH_OK;
    }
    if constexpr (FP32) {
        sph_set_error("fp32 arithmetic (arith_f32) needs pair_variant 6");
        return SPH_ERR_UNSUPPORTED;
    } else {
        dim3 gd(div_up(a.nd, 256)), bd(256);
        if (uh) hipLaunchKernelGGL((k_pair_direct<Fam, K, true>), gd, bd, 0, c->stream, a);
        else hipLaunchKernelGGL((k_pair_direct<Fam, K, false>), gd, bd, 0, c->stream, a);
        return SPH_OK;
    }
}

// the EOS-fused WCSPH family: uniform h, variant 6 only (sph_eval_group checks)
template <class Fam, bool UHV, int K> static int launch_pair_fused_k(sph_ctx *c, const PairArgs<Fam> &a)
{
    constexpr bool FP32 = sizeof(typename Fam::Real) == 4;
    dim3 g2(div_up(4 * div_up(a.nd, 256), WPB)), b2(64 * WPB);
    uint32_t cf = a.src[0].flags;
    for (int j = 1; j < a.nsrc; j++) if (a.src[j].flags != cf) cf = 0;
    if (c->const_flags == 0) cf = 0;
    if constexpr (fam_rowlds<Fam>::value && UHV) {
        if (c->row_lds && !a.nl_mode && !a.face_mode) { // the experiment of round 6: source records of a row tile in LDS
            dim3 g1(4 * div_up(a.nd, 256)), b1(64);
            if (cf == Fam::CF0) hipLaunchKernelGGL((k_pair_rowlds<Fam, K, Fam::CF0>), g1, b1, 0, c->stream, a);
            else hipLaunchKernelGGL((k_pair_rowlds<Fam, K, 0>), g1, b1, 0, c->stream, a);
            c->timers[T_N_ROWLDS].count++;
            return SPH_OK;
        }
    }
    if (cf == Fam::CF0) hipLaunchKernelGGL((k_pair_wave<Fam, K, UHV, FP32, Fam::CF0>), g2, b2, (size_t)c->lds_pad, c->stream, a);
    else hipLaunchKernelGGL((k_pair_wave<Fam, K, UHV, FP32, 0>), g2, b2, (size_t)c->lds_pad, c->stream, a);
    return SPH_OK;
}

template <class T> struct FamWCSPHMV_T;
// the merged multi-array WCSPH family (eval_group_merged)
template <class Fm, int K> static int launch_pair_merged_k(sph_ctx *c, const PairArgs<Fm> &a)
{
    constexpr bool FP32 = sizeof(typename Fm::Real) == 4;
    dim3 g2(div_up(4 * div_up(a.nd, 256), WPB)), b2(64 * WPB);
    constexpr bool UHM = !std::is_base_of<FamWCSPHMV_T<typename Fm::Real>, Fm>::value; // uniform h unless the family carries h
    hipLaunchKernelGGL((k_pair_wave<Fm, K, UHM, FP32, Fm::CF0>), g2, b2, (size_t)c->lds_pad, c->stream, a);
    return SPH_OK;
}

// the interpolator's families (sph_interp.h): fp64, run-time equation flags
template <class Fam, int K> static int launch_interp_k(sph_ctx *c, const PairArgs<Fam> &a)
{
    const bool uh = c->uniform_h && c->use_uniform_h;
    dim3 g2(div_up(4 * div_up(a.nd, 256), WPB)), b2(64 * WPB);
    if (uh) hipLaunchKernelGGL((k_pair_wave<Fam, K, true, false, 0>), g2, b2, 0, c->stream, a);
    else hipLaunchKernelGGL((k_pair_wave<Fam, K, false, false, 0>), g2, b2, 0, c->stream, a);
    return SPH_OK;
}

template <class Fam, int K> int launch_pair_ext(sph_ctx *c, const PairArgs<Fam> &a, bool rec_f32);
template <class Fam, bool UHV, int K> int launch_pair_fused_ext(sph_ctx *c, const PairArgs<Fam> &a);
template <class Fm, int K> int launch_pair_merged_ext(sph_ctx *c, const PairArgs<Fm> &a);
template <class Fam, int K> int launch_interp_ext(sph_ctx *c, const PairArgs<Fam> &a);

#if SPH_KERNEL_UNIT == 0
static int bad_kernel_kind(const char *who, int kk)
{
    sph_set_error("%s: unknown smoothing kernel kind %d (1..10, sphhip.h enum sph_kernel_kind)", who, kk);
    return SPH_ERR_UNSUPPORTED;
}
// kind and dimension, checked once per entry point: the 1-D Wendlands exist in one dimension only, the 2-D / 3-D
// ones not in one (kernels.py raises ValueError for these)
static int check_kernel(const char *who, const sph_kernel *K)
{
    const int kk = K->kind;
    if (kk < 1 || kk > 10) return bad_kernel_kind(who, kk);
    if (K->dim < 1 || K->dim > 3) { sph_set_error("%s: kernel dimension %d (1..3)", who, K->dim); return SPH_ERR_UNSUPPORTED; }
    const bool only1 = kk == SPH_K_WENDLAND_QUINTIC_C2_1D || kk == SPH_K_WENDLAND_QUINTIC_C4_1D || kk == SPH_K_WENDLAND_QUINTIC_C6_1D;
    const bool not1 = kk == SPH_K_WENDLAND_QUINTIC_C4 || kk == SPH_K_WENDLAND_QUINTIC_C6;
    if ((only1 && K->dim != 1) || (not1 && K->dim == 1)) {
        sph_set_error("%s: smoothing kernel kind %d: Dim %d not supported", who, kk, K->dim);
        return SPH_ERR_UNSUPPORTED;
    }
    return SPH_OK;
}

// SPH_KERNEL_SWITCH(kk, who, F): F<1..4> from this compile, F<5..10> from the kernel units
#define SPH_KERNEL_SWITCH(KK, WHO, LOCAL, EXT)                        \
    switch (KK) {                                                     \
    case 1: return LOCAL(1);                                          \
    case 2: return LOCAL(2);                                          \
    case 3: return LOCAL(3);                                          \
    case 4: return LOCAL(4);                                          \
    case 5: return EXT(5);                                            \
    case 6: return EXT(6);                                            \
    case 7: return EXT(7);                                            \
    case 8: return EXT(8);                                            \
    case 9: return EXT(9);                                            \
    case 10: return EXT(10);                                          \
    default: return bad_kernel_kind(WHO, KK);                         \
    }

template <class Fam> static int launch_pair(sph_ctx *c, int kk, const PairArgs<Fam> &a, bool rec_f32)
{
    if (a.nd == 0) return SPH_OK;
#define L_(K) launch_pair_k<Fam, K>(c, a, rec_f32)
#define E_(K) launch_pair_ext<Fam, K>(c, a, rec_f32)
    SPH_KERNEL_SWITCH(kk, "pair loop", L_, E_)
#undef L_
#undef E_
}
template <class Fam, bool UHV = true> static int launch_pair_fused(sph_ctx *c, int kk, const PairArgs<Fam> &a)
{
    if (a.nd == 0) return SPH_OK;
#define L_(K) launch_pair_fused_k<Fam, UHV, K>(c, a)
#define E_(K) launch_pair_fused_ext<Fam, UHV, K>(c, a)
    SPH_KERNEL_SWITCH(kk, "fused pair loop", L_, E_)
#undef L_
#undef E_
}
template <class Fm> static int launch_pair_merged(sph_ctx *c, int kk, const PairArgs<Fm> &a)
{
#define L_(K) launch_pair_merged_k<Fm, K>(c, a)
#define E_(K) launch_pair_merged_ext<Fm, K>(c, a)
    SPH_KERNEL_SWITCH(kk, "merged pair loop", L_, E_)
#undef L_
#undef E_
}
// a hand-written family on plain fp64 records, whatever the options say (the interpolator's private density sweep)
template <class Fam> static int launch_pair_fp64(sph_ctx *c, int kk, const PairArgs<Fam> &a) { return launch_pair<Fam>(c, kk, a, false); }
template <class Fam> static int interp_launch(sph_ctx *c, int kk, const PairArgs<Fam> &a)
{
    if (a.nd == 0) return SPH_OK;
#define L_(K) launch_interp_k<Fam, K>(c, a)
#define E_(K) launch_interp_ext<Fam, K>(c, a)
    SPH_KERNEL_SWITCH(kk, "sph_interpolate", L_, E_)
#undef L_
#undef E_
}

// nrec: doubles per packed record of this launch (RecordLayout::pl.nr; floats with fp32 records)
template <class Fam>
static void fill_common(sph_ctx *c, PairArgs<Fam> &a, const sph_kernel *K, double t, double dt, int nrec)
{
    a.posh = c->posh.as<double4>();
    a.aux = c->aux.as<double>();
    a.rec = c->posh.as<double>();
    a.nrec = nrec;
    a.fpos = c->fposb.as<float4>();
    a.dom_extent = fmax(fmax(c->xmax[0] - c->xmin[0], c->xmax[1] - c->xmin[1]), c->xmax[2] - c->xmin[2]);
    for (int k = 0; k < 3; k++) { a.nc[k] = c->nc[k]; a.xmin[k] = c->xmin[k]; }
    a.cell_size = c->cell_size;
    a.radius_scale = c->radius_scale;
    a.k.sigma = K->fac;
    a.k.deltap = K->deltap;
    a.k.dim = K->dim;
    a.t = t;
    a.dt = dt;
    a.ablate = (int)c->ablate;
    a.dbg = c->count_iters ? c->dbgc.as<unsigned long long>() : nullptr;
    // uniform-h constants, computed as the general path would per pair
    a.hu = 0.5 * (c->h_uniform + c->h_uniform);
    a.h1u = 1.0 / a.hu;
    a.facu = K->fac * a.h1u;
    if (K->dim > 1) a.facu *= a.h1u;
    if (K->dim > 2) a.facu *= a.h1u;
    a.epsu = 0.01 * a.hu * a.hu;
    a.hr2u = (c->radius_scale * c->h_uniform) * (c->radius_scale * c->h_uniform);
    a.norm_masks = (int)c->norm_masks;
    a.face_mode = 0;
    a.gfx_lo = c->gfx_lo; // (no faces named: -/+ INT_MAX, no face wavefronts)
    a.gfx_hi = c->gfx_hi;
}

// traversal order of the destination's tiles (sph_nnps_update builds it; option tile_block_rows) and of a tile's rows
template <class Fam> static void set_tile_order(sph_ctx *c, PairArgs<Fam> &a, const DevArray &D)
{
    a.d_tile_order = D.n_tiles ? D.tile_order.as<uint32_t>() : nullptr;
    a.row_mod3 = (int)c->row_mod3;
}
// the destinations of this launch are exactly the real particles of D's order: wave tiles from D.dlist (no idle ghost lanes)
template <class Fam> static void use_dest_list(sph_ctx *c, PairArgs<Fam> &a, const DevArray &D)
{
    if (!c->dest_list || !wave_tiles(c) || D.dlist_n == 0 || a.nl_mode || a.face_mode) return;
    a.d_list = D.dlist.as<uint32_t>();
    a.nd = (uint32_t)D.dlist_n;
    c->timers[T_N_DLIST].count++; // (pair launches whose wave tiles came from the list: sph_timer_get "n_dest_list")
    a.d_tile_order = D.n_ctiles ? D.ctile_order.as<uint32_t>() : nullptr;
}

static int ensure_out(sph_ctx *c, int id, std::initializer_list<int> props)
{
    for (int p : props) SPH_TRY(sph_array_ensure_prop(c, id, p));
    return SPH_OK;
}

// Neighbour lists of `dst` among `src` through the wave-tile pair kernel (nnps_build_csr_device /
// sph_nnps_get_csr): count pass (count[nd] filled, start == nullptr) or fill pass (start[nd], nbrs filled).
int nnps_csr_pair_kernel(sph_ctx *c, int src, int dst, uint32_t *count, const uint32_t *start, uint32_t *nbrs)
{
    SPH_TRY(nnps_need_tables(c));
    DevArray &S = c->arr[src], &D = c->arr[dst];
    if (D.n == 0) return SPH_OK;
    // ghost split: the source's ghosts are its second segment; the destinations are the particles the update binned (the
    // ghosts behind them have no lists: the callers zero their counts)
    if (count && D.n > D.n_binned) HIP_TRY(hipMemsetAsync(count + D.n_binned, 0, (D.n - D.n_binned) * 4, c->stream));
    const bool uh = c->uniform_h && c->use_uniform_h;
    const bool dest_is_src = src == dst;
    const size_t total = S.n + (dest_is_src ? 0 : D.n);
    if (total >= (1ull << 32)) { sph_set_error("too many particles for 32-bit packed indices"); return SPH_ERR_ARG; }
    RecordLayout rl(FAM_NBR); // lists are exact: fp64 records, whatever the options say
    if (uh) rl.pl.nr = 4;
    for (auto &pc : c->pack_cache) pc.epoch = 0;
    SPH_TRY(c->posh.reserve((total + 64) * sizeof(double) * rl.pl.nr));
    SPH_TRY(c->aux.reserve(64));
    SPH_TRY(c->fposb.reserve((total + 64) * sizeof(float4)));
    SPH_TRY(pack_array(c, src, 0, rl, FAM_NBR, 1u, false, true, 0));
    if (S.g_n > 0) SPH_TRY(pack_array(c, src, 0, rl, FAM_NBR, 1u, false, true, 1));
    if (!dest_is_src) SPH_TRY(pack_array(c, dst, S.n, rl, FAM_NBR, 1u, true, true, 0));
    sph_kernel K;
    K.kind = 1; K.dim = c->dim; K.fac = 1.0; K.radius_scale = c->radius_scale; K.deltap = 0.0;
    PairArgs<FamNbr> a;
    memset(&a, 0, sizeof a);
    fill_common(c, a, &K, 0.0, 0.0, rl.pl.nr);
    a.ablate = 0; a.dbg = nullptr;
    a.nsrc = 1;
    a.src[0] = {S.cell_start.as<uint32_t>(), 0u, 1u, S.fine_start.as<uint32_t>(), 0.0, 0u};
    if (S.g_n > 0) a.src[a.nsrc++] = {S.g_cell_start.as<uint32_t>(), (uint32_t)S.n_binned, 1u, S.g_fine_start.as<uint32_t>(), 0.0, 1u};
    a.d_off = dest_is_src ? 0u : (uint32_t)S.n;
    a.nd = (uint32_t)D.n_binned;
    a.d_keys = D.keys_sorted.as<uint32_t>(); a.d_fkeys = D.fkeys_sorted.as<uint32_t>(); a.d_perm = D.perm.as<uint32_t>();
    set_tile_order(c, a, D);
    a.d_start = 0; a.d_stop = (uint32_t)D.n; a.dflags = 1u;
    a.p.count = count; a.p.start = start; a.p.nbrs = nbrs;
    dim3 g2(div_up(4 * div_up(a.nd, 256), WPB)), b2(64 * WPB);
    if (uh) hipLaunchKernelGGL((k_pair_wave<FamNbr, 1, true, false, 1>), g2, b2, 0, c->stream, a);
    else hipLaunchKernelGGL((k_pair_wave<FamNbr, 1, false, false, 1>), g2, b2, 0, c->stream, a);
    return SPH_OK;
}

// ---------------------------------------------------------------------------
// A WCSPH group over several arrays as ONE launch on the merged order (sph_ctx::merged, FamWCSPHM_T): applicable
// when the group is nothing but Continuity / Momentum / XSPH equations whose (destination, source) flag matrix is a
// two-class table the library has a kernel for, over exactly the arrays of the grid, under the conditions of the
// EOS-fused uniform-mass records (uniform h, sph_group.src_eos, gamma = 7, no tensile correction, one mass per class).
// *done = false: not applicable, the caller takes the per-destination path.
// ---------------------------------------------------------------------------
static int eval_group_merged(sph_ctx *c, const sph_kernel *K, const sph_group *g, double t, double dt, bool *done)
{
    *done = false;
    if (!c->merged_valid || !c->merge_arrays || !c->nnps_valid || !wave_tiles(c) || c->ablate || c->count_iters) return SPH_OK;
    if (c->merge_blocked || !c->xflag.ptr) return SPH_OK; // a non-positive density was seen: the sign of rho cannot carry the class
    if (g->phase != 0 || c->ghosts_binned) return SPH_OK; // ghost segments: the per-destination path reads them as extra sources
    if (!(g->src_eos == 1 && c->eos_fuse && c->mass_fuse && c->const_flags &&
          tait_gk(g->eos_par[2]) == 3 && g->eos_par[0] > 0.0 && !c->record_f32 && !c->wcsph_nr)) // (gamma = 7: the merged decoders fold it)
        return SPH_OK;
    const bool vh = !(c->uniform_h && c->use_uniform_h); // variable h: FamWCSPHMV_T on records that carry h (round 5)
    const int na = c->narrays;
    uint32_t F[SPH_MAX_ARRAYS][SPH_MAX_ARRAYS] = {};
    const sph_equation *me = nullptr, *xe = nullptr;
    for (int i = 0; i < g->neq; i++) {
        const sph_equation &e = g->eqs[i];
        uint32_t flag;
        if (e.kind == SPH_EQ_CONTINUITY) flag = F_CONT;
        else if (e.kind == SPH_EQ_MOMENTUM) flag = F_MOM;
        else if (e.kind == SPH_EQ_XSPH) flag = F_XSPH;
        else return SPH_OK;
        if (e.nsrc <= 0 || e.dest < 0 || e.dest >= SPH_MAX_ARRAYS || !c->arr[e.dest].used || c->arr[e.dest].nnps_slot < 0) return SPH_OK;
        if (e.kind == SPH_EQ_MOMENTUM) {
            if (e.par[6] != 0.0) return SPH_OK; // tensile correction reads p of the neighbours
            if (me && memcmp(me->par, e.par, 7 * sizeof(double)) != 0) return SPH_OK; // one parameter set per launch
            me = &e;
        }
        if (e.kind == SPH_EQ_XSPH) {
            if (xe && xe->par[0] != e.par[0]) return SPH_OK;
            xe = &e;
        }
        const int ds = c->arr[e.dest].nnps_slot;
        for (int k = 0; k < e.nsrc; k++) {
            const int sid = e.src[k];
            if (sid < 0 || sid >= SPH_MAX_ARRAYS || !c->arr[sid].used || c->arr[sid].nnps_slot < 0) return SPH_OK;
            const int ss = c->arr[sid].nnps_slot;
            if (F[ds][ss] & flag) return SPH_OK; // the same equation twice: the general path reports it
            F[ds][ss] |= flag;
        }
    }
    // every array of the grid is in the record stream: it must take part (an array without equations would act
    // as a source of whatever its class says)
    for (int a = 0; a < na; a++) {
        bool used = false;
        for (int b = 0; b < na; b++) used |= F[a][b] != 0 || F[b][a] != 0;
        if (!used) return SPH_OK;
    }
    // two classes: arrays a, b are alike when they see and are seen by every array -- each other included -- the same way
    auto alike = [&](int a, int b) {
        if (F[a][a] != F[b][b] || F[a][b] != F[b][a] || F[a][a] != F[a][b]) return false;
        for (int x = 0; x < na; x++)
            if (x != a && x != b && (F[a][x] != F[b][x] || F[x][a] != F[x][b])) return false;
        return true;
    };
    int cls[SPH_MAX_ARRAYS], rep[2] = {0, -1};
    for (int a = 0; a < na; a++) {
        if (a == rep[0] || alike(a, rep[0])) cls[a] = 0;
        else if (rep[1] < 0 || alike(a, rep[1])) { cls[a] = 1; if (rep[1] < 0) rep[1] = a; }
        else return SPH_OK;
    }
    if (rep[1] < 0) return SPH_OK; // one class of several arrays: the per-destination path has constant flags already
    auto tab = [&](int i, int j) {
        // an entry of the class table from two representatives (two DIFFERENT members when the class has them)
        for (int a = 0; a < na; a++) for (int b = 0; b < na; b++)
            if (cls[a] == i && cls[b] == j && (a != b || i != j)) return F[a][b];
        return F[rep[i]][rep[j]];
    };
    uint32_t T4[2][2] = {{tab(0, 0), tab(0, 1)}, {tab(1, 0), tab(1, 1)}};
    for (int a = 0; a < na; a++) for (int b = 0; b < na; b++) if (F[a][b] != T4[cls[a]][cls[b]]) return SPH_OK;
    if (T4[1][1] > T4[0][0]) { // class 0 = the one with the richer self-interaction (the fluids)
        for (int a = 0; a < na; a++) cls[a] ^= 1;
        std::swap(T4[0][0], T4[1][1]); std::swap(T4[0][1], T4[1][0]);
    }
    const uint32_t ct = WCSPHM_CT(T4[0][0], T4[0][1], T4[1][0], T4[1][1]);
    if (ct != FamWCSPHM_T<double>::CF0) return SPH_OK; // the class table the library has a kernel for (WCSPHScheme's)
    // one mass per class, seen by the last neighbour update
    c->want_mrange = true;
    double mu[2] = {0.0, 0.0};
    bool have[2] = {false, false};
    for (int a = 0; a < na; a++) {
        const DevArray &A = c->arr[c->ids[a]];
        if (A.n == 0) continue;
        if (!A.m_known) return SPH_OK;
        if (have[cls[a]] && mu[cls[a]] != A.m_value) return SPH_OK;
        mu[cls[a]] = A.m_value; have[cls[a]] = true;
    }
    DevArray &M = c->merged;
    if (M.n == 0) { *done = true; return SPH_OK; }

    // outputs and properties
    static const int outp[9] = {SPH_ARHO, SPH_AU, SPH_AV, SPH_AW, SPH_AX, SPH_AY, SPH_AZ, SPH_DT_CFL, SPH_DT_FORCE};
    static const int inp[9] = {SPH_X, SPH_Y, SPH_Z, SPH_U, SPH_V, SPH_W, SPH_RHO, SPH_P, SPH_H};
    const bool f32 = c->arith_f32 != 0;
    PackMArgs pa;
    memset(&pa, 0, sizeof pa);
    for (int a = 0; a < na; a++) {
        const int id = c->ids[a];
        DevArray &A = c->arr[id];
        for (int k = 0; k < 9; k++) {
            if (A.n && !A.prop[inp[k]]) return need_prop(c, id, inp[k], "pair loop");
            pa.prop[k][a] = A.prop[inp[k]];
        }
        if (cls[a]) pa.cls |= 1u << a;
    }
    SPH_TRY(c->posh.reserve((M.n + 64) * (f32 ? 32 : 64)));
    SPH_TRY(c->aux.reserve(64));
    SPH_TRY(c->fposb.reserve((M.n + 64) * sizeof(float4)));
    for (auto &pc : c->pack_cache) pc.epoch = 0; // the shared slots of the per-destination path are overwritten
    {
        ScopedTimer tm(c, T_PACK);
        pa.perm = M.perm.as<uint32_t>(); pa.slot = M.slot8.as<uint8_t>();
        pa.n = M.n; pa.off = 0;
        pa.rec = c->posh.as<double>(); pa.fpos = c->fposb.as<float4>();
        pa.f32 = f32 ? 1 : 0; pa.lds_np = f32 ? 2 : 4;
        for (int k = 0; k < 3; k++) pa.gmin[k] = c->xmin[k];
        pa.vh = vh ? 1 : 0;
        pa.hr = vh ? c->radius_scale : c->radius_scale * c->h_uniform;
        pa.rho_flag = c->xflag.as<uint32_t>();
        const dim3 pg(div_up(M.n, 256)), pb(256);
        const size_t plds = (size_t)pa.lds_np * 256 * 16;
        if (f32 && vh) hipLaunchKernelGGL((k_pack_merged<true, true>), pg, pb, plds, c->stream, pa);
        else if (f32) hipLaunchKernelGGL((k_pack_merged<true, false>), pg, pb, plds, c->stream, pa);
        else if (vh) hipLaunchKernelGGL((k_pack_merged<false, true>), pg, pb, plds, c->stream, pa);
        else hipLaunchKernelGGL((k_pack_merged<false, false>), pg, pb, plds, c->stream, pa);
    }
    ScopedTimer tm(c, T_PAIR);
    ScopedTimer tmf(c, T_PAIR_FAM + FAM_WCSPH);
    c->timers[T_N_EOSF].count++; c->timers[T_N_UMASS].count++; c->timers[T_N_MERGED].count++;
    auto run = [&](auto tag) -> int {
        typedef decltype(tag) Fm;
        PairArgs<Fm> a;
        memset(&a, 0, sizeof a);
        fill_common(c, a, K, t, dt, 8); // k_pack_merged: 8 doubles per record, or 8 floats
        a.nsrc = 1;
        a.src[0] = {nullptr, 0u, ct, M.fine_start.as<uint32_t>(), mu[0]};
        a.d_off = 0; a.nd = (uint32_t)M.n;
        a.d_mu = mu[0];
        a.d_keys = M.keys_sorted.as<uint32_t>(); a.d_fkeys = M.fkeys_sorted.as<uint32_t>(); a.d_perm = M.perm.as<uint32_t>();
        a.d_slot = M.slot8.as<uint8_t>();
        set_tile_order(c, a, M);
        a.d_start = 0; a.d_stop = 0xffffffffu; a.dflags = ct;
        a.e_rho01 = 1.0 / g->eos_par[0]; a.e_c0 = g->eos_par[1];
        a.e_B = g->eos_par[0] * g->eos_par[1] * g->eos_par[1] / g->eos_par[2];
        a.e_gk = tait_gk(g->eos_par[2]);
        a.e_p0 = g->eos_par[3];
        if (me) { a.p.c0 = me->par[0]; a.p.alpha = me->par[1]; a.p.beta = me->par[2]; a.p.gx = me->par[3]; a.p.gy = me->par[4]; a.p.gz = me->par[5]; }
        if (xe) a.p.eps = xe->par[0];
        a.p.mu1 = mu[1];
        for (int s = 0; s < na; s++) {
            const int id = c->ids[s];
            DevArray &A = c->arr[id];
            uint32_t row = 0;
            for (int b = 0; b < na; b++) row |= F[s][b];
            // NP_DEST / D_START_IDX (acceleration_eval_cython_helper.py:259-280), per destination array
            size_t start = g->start_idx > 0 ? (size_t)g->start_idx : 0;
            size_t stop = g->stop_idx >= 0 ? (size_t)g->stop_idx : (g->real ? A.n_real : A.n);
            if (stop > A.n) stop = A.n;
            if (!row || stop < start) start = stop = 0;
            a.p.rng[s][0] = (uint32_t)start; a.p.rng[s][1] = (uint32_t)stop;
            if (row & F_CONT) { SPH_TRY(ensure_out(c, id, {SPH_ARHO})); }
            if (row & F_MOM) { SPH_TRY(ensure_out(c, id, {SPH_AU, SPH_AV, SPH_AW, SPH_DT_CFL, SPH_DT_FORCE})); }
            if (row & F_XSPH) { SPH_TRY(ensure_out(c, id, {SPH_AX, SPH_AY, SPH_AZ})); }
            for (int k = 0; k < 9; k++) a.p.out[s][k] = A.prop[outp[k]];
        }
        {   // every destination range is [0, n_real) of its array (or empty): the wave tiles are the real particles' ones
            bool all_real = true;
            for (int s = 0; s < na; s++) {
                const DevArray &A = c->arr[c->ids[s]];
                all_real &= (a.p.rng[s][0] == 0 && a.p.rng[s][1] == (uint32_t)A.n_real) || A.n == 0;
            }
            if (all_real) use_dest_list(c, a, M);
        }
        return launch_pair_merged<Fm>(c, K->kind, a);
    };
    if (vh) SPH_TRY(f32 ? run(FamWCSPHMV_T<float>()) : run(FamWCSPHMV_T<double>()));
    else SPH_TRY(f32 ? run(FamWCSPHM_T<float>()) : run(FamWCSPHM_T<double>()));
    HIP_TRY(hipGetLastError());
    *done = true;
    return SPH_OK;
}

// sph_group.src_eos = 3 where the records cannot absorb the equation: the Tait EOS over every particle of every array the
// group touches, as the group the host left out would have run it
static int run_pending_eos(sph_ctx *c, const sph_group *g)
{
    bool seen[SPH_MAX_ARRAYS] = {};
    auto one = [&](int id) -> int {
        if (id < 0 || id >= SPH_MAX_ARRAYS || !c->arr[id].used || seen[id]) return SPH_OK; // (bad ids: reported by the caller)
        seen[id] = true;
        sph_equation e;
        memset(&e, 0, sizeof e);
        e.kind = SPH_EQ_TAIT_EOS;
        e.dest = id;
        for (int k = 0; k < 4; k++) e.par[k] = g->eos_par[k];
        SPH_TRY(run_nosrc(c, e, 0, c->arr[id].n));
        c->pack_cache[id].epoch = 0;
        return SPH_OK;
    };
    for (int i = 0; i < g->neq; i++) {
        SPH_TRY(one(g->eqs[i].dest));
        for (int k = 0; k < g->eqs[i].nsrc && k < SPH_MAX_ARRAYS; k++) SPH_TRY(one(g->eqs[i].src[k]));
    }
    return SPH_OK;
}

// ---------------------------------------------------------------------------
// sph_eval_group, one destination at a time: plan -> records -> pack -> neighbour lists -> bind and launch.  Every
// stage is a function below; what one stage decides reaches the next as a value (DestPlan, RecordLayout), never
// through the context.
// ---------------------------------------------------------------------------

// destinations in first-appearance order (acceleration_eval.py:126-131)
static int resolve_destinations(sph_ctx *c, const sph_group *g, int *dests, int *ndest)
{
    *ndest = 0;
    for (int i = 0; i < g->neq; i++) {
        int d = g->eqs[i].dest;
        if (d < 0 || d >= SPH_MAX_ARRAYS || !c->arr[d].used) { sph_set_error("equation %d: bad dest array %d", i, d); return SPH_ERR_ARG; }
        bool seen = false;
        for (int j = 0; j < *ndest; j++) seen |= dests[j] == d;
        if (!seen) dests[(*ndest)++] = d;
    }
    if (g->phase < 0 || g->phase > 2 || (g->phase != 0 && *ndest != 1)) {
        sph_set_error("sph_eval_group: phase %d needs a group with one destination array", g->phase);
        return SPH_ERR_ARG;
    }
    return SPH_OK;
}

// equations without sources run first (mako :50-58); phase 2: over the particles that arrived since phase 1
static int run_nosrc_equations(sph_ctx *c, const sph_group *g, int dst, size_t start, size_t stop)
{
    const size_t ns_start = g->phase == 2 ? std::max(start, c->arr[dst].n_binned) : start;
    for (int i = 0; i < g->neq; i++) {
        const sph_equation &e = g->eqs[i];
        if (e.dest != dst || e.nsrc != 0) continue;
        if (!is_nosrc_kind(e.kind)) { sph_set_error("equation kind %d needs sources", e.kind); return SPH_ERR_UNSUPPORTED; }
        SPH_TRY(run_nosrc(c, e, ns_start, stop));
        c->pack_cache[dst].epoch = 0; // its properties changed: records packed for an earlier destination are stale
    }
    return SPH_OK;
}

// What the pair loop of one destination evaluates.  plan_destination builds it once (the caller sets dst, ndest, phase,
// start and stop); every later stage reads it as const.
struct DestPlan {
    int dst = -1, ndest = 0, phase = 0;
    size_t start = 0, stop = 0;           // NP_DEST / D_START_IDX (acceleration_eval_cython_helper.py:259-280)
    int fam = FAM_NONE;                   // FAM_NONE: this destination has no pair launch
    int nsrcs = 0, srcs[SPH_MAX_ARRAYS];  // sources in first-appearance order (acceleration_eval.py:136-151) ...
    uint32_t sflags[SPH_MAX_ARRAYS] = {}; // ... the flags of the equations that read each ...
    uint32_t dflags = 0;                  // ... and their union
    const sph_equation *eq_of[64] = {};   // the equation of a kind on this destination ...
    int eq_pos[64] = {};                  // ... and its position in the group
    // records in the packed buffer: all of them, the first of every source, the first of the destination
    size_t total = 0, off_of[SPH_MAX_ARRAYS], d_off = 0;
    bool dest_is_src = false;
    bool share = false;                   // one buffer slot per neighbour-grid array, shared by the destinations of a group
    bool any_ghosts = false;              // a ghost segment (sph_nnps_update_ghosts) among the arrays read
};

static int plan_destination(sph_ctx *c, const sph_group *g, DestPlan &P)
{
    const int dst = P.dst;
    const DevArray &D = c->arr[dst];
    // what the equations with sources on this destination say about the family of the ones several families have: an
    // elastic-rates term; a delta-SPH / laminar-viscosity term (the WCSPH-options family); an EDAC force equation;
    // ComputeAveragePressure
    bool elastic = false, wcsphx = false, edac = false, avgp = false;
    for (int i = 0; i < g->neq; i++) {
        const int kind = g->eqs[i].kind;
        if (g->eqs[i].dest != dst || g->eqs[i].nsrc <= 0) continue;
        elastic |= kind == SPH_EQ_MOMENTUM_WITH_STRESS || kind == SPH_EQ_MONAGHAN_ART_VISCOSITY;
        wcsphx |= is_wcsph_option_kind(kind);
        edac |= is_edac_force_kind(kind);
        avgp |= kind == SPH_EQ_EDAC_AVG_PRESSURE;
    }
    for (int i = 0; i < g->neq; i++) {
        const sph_equation &e = g->eqs[i];
        if (e.dest != dst || e.nsrc == 0) continue;
        if (e.kind < 0 || e.kind >= 64) { sph_set_error("bad equation kind %d", e.kind); return SPH_ERR_ARG; }
        uint32_t flag = 0;
        int f = eq_family(e.kind, &flag, elastic, wcsphx, edac, avgp);
        P.eq_pos[e.kind] = i;
        if (f == FAM_NONE) { sph_set_error("equation kind %d has no hand-written pair kernel", e.kind); return SPH_ERR_UNSUPPORTED; }
        if (P.fam != FAM_NONE && f != P.fam) {
            sph_set_error("group mixes equation families on destination %d (kinds are fused per family)", dst);
            return SPH_ERR_UNSUPPORTED;
        }
        P.fam = f;
        if (P.eq_of[e.kind]) {
            sph_set_error("equation kind %d appears twice for destination %d in one group", e.kind, dst);
            return SPH_ERR_UNSUPPORTED;
        }
        P.eq_of[e.kind] = &e;
        for (int k = 0; k < e.nsrc; k++) {
            int s = e.src[k], pos = -1;
            if (s < 0 || s >= SPH_MAX_ARRAYS || !c->arr[s].used) { sph_set_error("bad source array %d", s); return SPH_ERR_ARG; }
            for (int j = 0; j < P.nsrcs; j++) if (P.srcs[j] == s) pos = j;
            if (pos < 0) { pos = P.nsrcs; P.srcs[P.nsrcs++] = s; }
            P.sflags[pos] |= flag;
        }
    }
    if (P.fam == FAM_NONE) return SPH_OK;
    const int fam = P.fam, nsrcs = P.nsrcs;
    uint32_t *sflags = P.sflags, &dflags = P.dflags;
    if (!c->nnps_valid) { sph_set_error("sph_eval_group: neighbour grid is stale; call sph_nnps_update"); return SPH_ERR_STATE; }
    if (D.nnps_slot < 0) { sph_set_error("destination array %d is not part of the neighbour grid", dst); return SPH_ERR_STATE; }
    SPH_TRY(nnps_need_tables(c)); // the per-destination path reads every array's own cell order
    for (int j = 0; j < nsrcs; j++) {
        dflags |= sflags[j];
        if (c->arr[P.srcs[j]].nnps_slot < 0) { sph_set_error("source array %d is not part of the neighbour grid", P.srcs[j]); return SPH_ERR_STATE; }
    }
    if (fam == FAM_WCSPHX) {
        // the extra terms add into the sums of the Continuity / Momentum equations, whose finish() writes them
        if ((dflags & F_DCONT) && !(dflags & F_CONT)) { sph_set_error("ContinuityEquationDeltaSPH needs a ContinuityEquation on destination %d", dst); return SPH_ERR_UNSUPPORTED; }
        if ((dflags & (F_DMOM | F_LAM | F_LAMD)) && !(dflags & F_MOM)) { sph_set_error("the delta-SPH / laminar viscosity terms need a MomentumEquation on destination %d", dst); return SPH_ERR_UNSUPPORTED; }
        if ((dflags & F_LAM) && (dflags & F_LAMD)) { sph_set_error("both LaminarViscosity and LaminarViscosityDeltaSPH on destination %d", dst); return SPH_ERR_UNSUPPORTED; }
    }
    if (fam == FAM_EDAC) {
        if (P.eq_of[SPH_EQ_EDAC_MOMENTUM] && P.eq_of[SPH_EQ_EDAC_MOM_PRESSURE]) { sph_set_error("both EDAC pressure-gradient forms on destination %d", dst); return SPH_ERR_UNSUPPORTED; }
        if ((dflags & F_EINT) && (dflags & F_EXS)) { sph_set_error("XSPHCorrection next to the internal-flow EDAC pressure gradient on destination %d", dst); return SPH_ERR_UNSUPPORTED; }
        if (!(dflags & F_EINT) && (dflags & F_TAS)) { sph_set_error("MomentumEquationArtificialStress next to the external-flow EDAC equations on destination %d", dst); return SPH_ERR_UNSUPPORTED; }
        // the branch is a property of the destination: one instantiation per branch, and equal flag sets on the
        // sources of a default group so that the compile-time set applies
        if (dflags & F_EINT) for (int j = 0; j < nsrcs; j++) sflags[j] |= F_EINT;
    }
    if (fam == FAM_DSPRE) {
        // the moment matrix must be complete before a corrected gradient reads it: a group of its own, as in WCSPHScheme
        if ((dflags & F_MOMENT) && (dflags & (F_GRADRHO | F_GCORR))) {
            sph_set_error("GradientCorrectionPreStep shares a group with GradientCorrection / ContinuityEquationDeltaSPHPreStep on destination %d; put it in a group of its own before them", dst);
            return SPH_ERR_UNSUPPORTED;
        }
        // GradientCorrection rewrites DWIJ for the equations AFTER it: behind the pre-step it corrects nothing
        if ((dflags & F_GCORR) && (!(dflags & F_GRADRHO) || P.eq_pos[SPH_EQ_GRADIENT_CORRECTION] > P.eq_pos[SPH_EQ_CONTINUITY_DELTA_SPH_PRESTEP])) {
            dflags &= ~(uint32_t)F_GCORR;
            for (int j = 0; j < nsrcs; j++) sflags[j] &= ~(uint32_t)F_GCORR;
        }
        if (!dflags) { P.fam = FAM_NONE; return SPH_OK; }
        for (int j = 0; j < nsrcs; j++) if ((sflags[j] & F_GCORR) && !(sflags[j] & F_GRADRHO)) sflags[j] &= ~(uint32_t)F_GCORR;
    }
    if ((fam == FAM_WCSPH || fam == FAM_WCSPHX) && P.eq_of[SPH_EQ_MOMENTUM] && P.eq_of[SPH_EQ_MOMENTUM]->par[6] != 0.0) {
        dflags |= F_TENSILE;
        for (int j = 0; j < nsrcs; j++) if (sflags[j] & F_MOM) sflags[j] |= F_TENSILE;
    }

    // where the records go: every source, then the destination unless it is a source
    for (int j = 0; j < nsrcs; j++) { P.off_of[j] = P.total; P.total += c->arr[P.srcs[j]].n; P.dest_is_src |= P.srcs[j] == dst; }
    P.d_off = P.total;
    if (!P.dest_is_src) P.total += D.n;
    else for (int j = 0; j < nsrcs; j++) if (P.srcs[j] == dst) P.d_off = P.off_of[j];
    // WCSPH groups with several destinations (a dam break: fluid, boundary, obstacle) read the
    // SAME source records, and nothing the family writes (accelerations) is part of a record:
    // one buffer slot per neighbour-grid array, each array packed once per group instead of
    // once per destination that reads it (dam break C2: 7 -> 3 k_pack launches per evaluation).
    // The host brackets the per-destination calls of one group with option pack_group 1 / 0.
    P.share = fam == FAM_WCSPH && wave_tiles(c) && (P.ndest > 1 || c->pack_group);
    if (P.share) {
        size_t goff[SPH_MAX_ARRAYS] = {};
        P.total = 0;
        for (int a = 0; a < c->narrays; a++) { goff[c->ids[a]] = P.total; P.total += c->arr[c->ids[a]].n; }
        for (int j = 0; j < nsrcs; j++) P.off_of[j] = goff[P.srcs[j]];
        P.d_off = goff[dst];
    }
    if (P.total >= (1ull << 32)) { sph_set_error("too many particles for 32-bit packed indices"); return SPH_ERR_ARG; }
    // ghost split (sph_nnps_update_ghosts): arrays whose ghosts were binned after the real particles carry them as a
    // second record segment and a second source; the destinations are the particles the update binned (a
    // destination-only array is read through its own records only: its ghosts are no destinations)
    for (int j = 0; j < nsrcs; j++) P.any_ghosts |= c->arr[P.srcs[j]].g_n > 0;
    P.any_ghosts |= D.g_n > 0;
    if (P.phase != 0 && !(nsrcs == 1 && P.srcs[0] == dst && !P.share)) {
        sph_set_error("sph_eval_group: phases need a group over ONE array (destination == its only source)");
        return SPH_ERR_UNSUPPORTED;
    }
    if ((P.any_ghosts || P.phase != 0) && !wave_tiles(c)) {
        sph_set_error("ghost segments (sph_nnps_update_ghosts) need pair_variant 6");
        return SPH_ERR_UNSUPPORTED;
    }
    return SPH_OK;
}

// The records of this destination's block.  eos_pending: the Tait EOS the host left to this call (sph_group.src_eos = 3)
// has not run; RecordLayout::eos_abs says whether the pack of these records takes it over.
static RecordLayout choose_records(sph_ctx *c, const sph_group *g, const DestPlan &P, bool eos_pending)
{
    const int fam = P.fam, nsrcs = P.nsrcs;
    const uint32_t dflags = P.dflags;
    const DevArray &D = c->arr[P.dst];
    const bool wave = wave_tiles(c), uh = c->uniform_h && c->use_uniform_h;
    RecordLayout rl(fam);
    PackPlan &pl = rl.pl;
    rl.record_f32 = c->record_f32 != 0;
    rl.arith_f32 = c->arith_f32 != 0;
    if (fam == FAM_WCSPHX && (dflags & F_DCONT)) { // the records carry the sources' gradrho
        for (int k = 0; k < 3; k++) pl.props[8 + k] = SPH_GRADRHO0 + k;
        pl.na = 11; pl.nr = 16;
    }
    // compact 80-B WCSPH records when neither h nor p of a neighbour is read
    if (wave && fam == FAM_WCSPH && uh && !(dflags & F_TENSILE)) pl.nr = c->wcsph_nr ? (int)c->wcsph_nr : 10;
    if (wave && fam == FAM_DENSITY && uh) pl.nr = 4;
    if (wave && fam == FAM_TVF && uh) pl.nr = (dflags & F_TAV) ? 14 : 12;
    if (wave && fam == FAM_EDAC && uh) pl.nr = 14; // (m always: load_record_edac)
    if (wave && (rl.record_f32 || rl.arith_f32)) pl.nr = (4 + pl.na + 3) & ~3; // floats
    // The caller promised (sph_group.src_eos) that p, cs of every array read here are the Tait EOS of its
    // rho: with gamma = 7 (powers by multiplication), uniform h and no tensile correction the pair kernel
    // recomputes them and the records shrink to 64 bytes (32 in fp32).
    const bool eosf = g->src_eos == 1 && c->eos_fuse && fam == FAM_WCSPH && wave && uh && !(dflags & F_TENSILE) &&
                      tait_gk(g->eos_par[2]) >= 0 && g->eos_par[0] > 0.0 && !rl.record_f32 && !c->wcsph_nr;
    if (eosf) pl.nr = 8; // doubles, or floats with arith_f32
    // ... and when every array read here had ONE mass at the last neighbour update, the record's mass slot
    // carries p / rho^2 and most of the per-record EOS goes as well (FamWCSPHE_T<T, true>)
    // (only with the equation flags as a compile-time constant: the run-time-flag kernel of a dam break's three
    // sources is at its scalar-register limit and 1-3 % slower with a mass per source)
    bool umass = eosf && c->mass_fuse && c->const_flags;
    for (int j = 0; j < nsrcs && umass; j++) umass = P.sflags[j] == FamWCSPH::CF0;
    if (umass) c->want_mrange = true; // the reduction of the neighbour updates from now on includes m (8 B per particle)
    for (int j = 0; j < nsrcs && umass; j++) umass = c->arr[P.srcs[j]].m_known;
    // ... and with VARIABLE h the same promise plus one mass per source array gives 64-byte records [x y z h u v w rho]
    bool eosv = !eosf && g->src_eos == 1 && c->eos_fuse && c->mass_fuse && fam == FAM_WCSPH && wave && !uh &&
                !(dflags & F_TENSILE) && tait_gk(g->eos_par[2]) == 3 && g->eos_par[0] > 0.0 && !rl.record_f32 && !c->wcsph_nr;
    if (eosv) c->want_mrange = true;
    for (int j = 0; j < nsrcs && eosv; j++) eosv = c->arr[P.srcs[j]].m_known;
    if (eosv) pl.nr = 8;
    // TVF force pass after StateEquation + density summation (sph_group.src_eos = 2): p and V leave the records
    // when every array read here has ONE mass (V = rho / m)
    bool tvff = g->src_eos == 2 && c->eos_fuse && c->mass_fuse && fam == FAM_TVF && wave && uh && !rl.record_f32 &&
                g->eos_par[1] != 0.0; // (the artificial viscosity's m_j is the source's one mass)
    if (tvff) c->want_mrange = true;
    for (int j = 0; j < nsrcs && tvff; j++) tvff = c->arr[P.srcs[j]].m_known;
    if (tvff && !P.dest_is_src) tvff = D.m_known;
    if (tvff) pl.nr = rl.arith_f32 ? ((dflags & F_TAS) ? 12 : 8) : ((dflags & F_TAS) ? 10 : 8);
    // elastic rates: uniform h and ONE mass per source array -> neither travels in the records
    bool elu = fam == FAM_ELASTIC && c->mass_fuse && wave && uh && !rl.record_f32;
    if (elu) c->want_mrange = true;
    for (int j = 0; j < nsrcs && elu; j++) elu = c->arr[P.srcs[j]].m_known;
    if (elu) pl.nr = 20; // doubles, or floats with arith_f32
    rl.kind = eosf ? REC_EOSF : eosv ? REC_EOSV : tvff ? REC_TVFF : elu ? REC_ELU : REC_PLAIN; // (one family each: exclusive)
    rl.umass = umass;
    // The pending Tait EOS is absorbed by the records when they are the EOS-fused ones of ONE array and the pack
    // launches visit every particle of it (both segments) (gamma = 7 only: the other odd exponents keep the EOS kernel)
    rl.eos_abs = eos_pending && rl.eos_fused() && c->eos_absorb && tait_gk(g->eos_par[2]) == 3 && P.phase == 0 && P.ndest == 1 &&
                 nsrcs == 1 && P.srcs[0] == P.dst && D.n > 0 && D.n_binned + D.g_n == D.n;
    if (rl.eos_abs) for (int k = 0; k < 4; k++) rl.eos_par[k] = g->eos_par[k];
    return rl;
}

// Room for the records, then the pack launches: every source and the destination's own record, once per group where the
// destinations of a group share them (the pack cache), per segment in a split evaluation
static int pack_records(sph_ctx *c, const DestPlan &P, const RecordLayout &rl)
{
    const int phase = P.phase, fam = P.fam;
    const void *rec_was = c->posh.ptr, *fpos_was = c->fposb.ptr;
    // phase 1 leaves room for the ghosts phase 2 packs behind the real particles' records (the array's capacity bounds
    // them); phase 2 keeps what phase 1 packed should the buffers have to grow after all
    const size_t total_res = phase == 1 ? std::max(P.total, c->arr[P.dst].cap) : P.total;
    SPH_TRY(c->posh.reserve((total_res + 64) * sizeof(double) * (wave_tiles(c) ? rl.pl.nr : 4), phase == 2, c->stream));
    SPH_TRY(c->aux.reserve((total_res + 64) * sizeof(double) * rl.pl.na));
    if (wave_tiles(c)) SPH_TRY(c->fposb.reserve((total_res + 64) * sizeof(float4), phase == 2, c->stream));
    if (c->posh.ptr != rec_was || c->fposb.ptr != fpos_was) // the buffers moved: nothing packed earlier is there
        for (auto &pc : c->pack_cache) pc.epoch = 0;
    ScopedTimer tm(c, T_PACK);
    const int sig = rl.sig();
    // The shared slots live in the same buffers every other unit packs into from offset 0:
    // a unit that does not share (another family, a single-destination call), or one whose
    // record layout differs from what the cache holds, overwrites them -- nothing cached survives.
    // a split evaluation: the second half must read the layout the first half packed -- when what is known of the
    // masses changed in between (a ghost with another mass: sph_nnps_update_ghosts), it packs both segments again
    if (phase == 1) c->phase_sig = sig;
    const bool repack = phase == 2 && c->phase_sig != sig;
    bool keep = P.share;
    if (P.share)
        for (auto &pc : c->pack_cache)
            if (pc.epoch == c->pack_epoch && (pc.fam != fam || pc.sig != sig)) keep = false;
    if (!keep)
        for (auto &pc : c->pack_cache) pc.epoch = 0;
    auto pack_once = [&](int id, size_t off, uint32_t fl, bool dest_only) -> int {
        PackCache &pc = c->pack_cache[id];
        const bool hit = P.share && pc.epoch == c->pack_epoch && pc.fam == fam && pc.sig == sig;
        // phase 1: the particles present (the real ones); phase 2: the ghosts that arrived since; else both segments
        if (phase != 2 || repack) SPH_TRY(pack_array(c, id, off, rl, fam, fl, dest_only, !hit, 0)); // a hit still validates
        if (phase != 1 && c->arr[id].g_n > 0) SPH_TRY(pack_array(c, id, off, rl, fam, fl, dest_only, !hit, 1));
        pc.epoch = P.share ? c->pack_epoch : 0; pc.fam = fam; pc.sig = sig;
        return SPH_OK;
    };
    // a source must hold what ITS equations read; the destination's own record what all of them read
    for (int j = 0; j < P.nsrcs; j++) SPH_TRY(pack_once(P.srcs[j], P.off_of[j], P.srcs[j] == P.dst ? P.dflags : P.sflags[j], false));
    if (!P.dest_is_src) SPH_TRY(pack_once(P.dst, P.d_off, P.dflags, true));
    return SPH_OK;
}

// Neighbour-list reuse between the pair passes of one evaluation (sph_group.nl_mode): one source,
// the wave-tile kernel, same grid.  A pass that keeps its lists (1) records what they belong to; a pass
// that wants them (2) gets them only if that record matches -- otherwise it runs its own phase 1.
static int choose_nl_mode(sph_ctx *c, const sph_group *g, const DestPlan &P, int *nl_mode)
{
    const DevArray &D = c->arr[P.dst];
    *nl_mode = 0;
    if (c->nl_reuse && !c->row_lds && wave_tiles(c) && P.nsrcs == 1 && g->nl_mode && !c->ablate && !P.any_ghosts && P.phase == 0) {
        const size_t n_wt = (size_t)4 * div_up(D.n, 256);
        if (g->nl_mode == 1) {
            SPH_TRY(c->nlbuf.reserve(n_wt * NLW * sizeof(uint32_t)));
            c->nl.valid = true; c->nl.epoch = c->nnps_epoch; c->nl.dst = P.dst; c->nl.src = P.srcs[0];
            c->nl.start = P.start; c->nl.stop = P.stop; c->nl.nd = D.n;
            *nl_mode = 1;
        } else if (g->nl_mode == 2 && c->nl.valid && c->nl.epoch == c->nnps_epoch && c->nl.dst == P.dst && c->nl.src == P.srcs[0] &&
                   c->nl.nd == D.n && c->nl.start <= P.start && c->nl.stop >= P.stop && c->nlbuf.bytes >= n_wt * NLW * sizeof(uint32_t)) {
            *nl_mode = 2;
        }
    } else if (g->nl_mode != 2) {
        c->nl.valid = c->nl.valid && !(g->nl_mode == 1); // a keeping pass that could not keep: nothing to reuse
    }
    return SPH_OK;
}

// one pair launch of sph_eval_group: what the family binders below read
struct PairLaunch {
    sph_ctx *c;
    const sph_kernel *K;
    const sph_group *g;
    double t, dt;
    const DestPlan &P;
    const RecordLayout &rl;
    int nl_mode;
};

// the launch arguments of a family, zeroed, with the part every family shares filled in
template <class F> static PairArgs<F> pair_args(const PairLaunch &L)
{
    sph_ctx *c = L.c;
    const DestPlan &P = L.P;
    const sph_group *g = L.g;
    const DevArray &D = c->arr[P.dst];
    PairArgs<F> a;
    memset(&a, 0, sizeof a);
    fill_common(c, a, L.K, L.t, L.dt, L.rl.pl.nr);
    for (int j = 0; j < P.nsrcs; j++) {
        const DevArray &S = c->arr[P.srcs[j]];
        a.src[a.nsrc++] = {S.cell_start.as<uint32_t>(), (uint32_t)P.off_of[j], P.sflags[j], S.fine_start.as<uint32_t>(), S.m_value, 0u};
    }
    for (int j = 0; j < P.nsrcs && P.phase != 1; j++) { // the ghost segments, after every array's first segment
        const DevArray &S = c->arr[P.srcs[j]];
        if (S.g_n == 0) continue;
        a.src[a.nsrc++] = {S.g_cell_start.as<uint32_t>(), (uint32_t)(P.off_of[j] + S.n_binned), P.sflags[j],
                           S.g_fine_start.as<uint32_t>(), S.m_value, 1u};
    }
    a.face_mode = c->split_pair ? P.phase : 0;
    a.d_off = (uint32_t)P.d_off; a.nd = (uint32_t)D.n_binned;
    a.d_mu = D.m_value;
    a.d_keys = D.keys_sorted.as<uint32_t>(); a.d_fkeys = D.fkeys_sorted.as<uint32_t>(); a.d_perm = D.perm.as<uint32_t>();
    set_tile_order(c, a, D);
    a.d_start = (uint32_t)P.start; a.d_stop = (uint32_t)P.stop; a.dflags = P.dflags;
    a.nl_mode = L.nl_mode;
    if (L.nl_mode) a.nl = c->nlbuf.as<uint32_t>();
    // Group.real = True without start / stop: the destinations are the real particles
    if (P.start == 0 && P.stop == D.n_real && D.n_binned == D.n && !P.any_ghosts) use_dest_list(c, a, D);
    if (L.rl.eos_fused()) {
        a.e_rho01 = 1.0 / g->eos_par[0]; a.e_c0 = g->eos_par[1];
        a.e_B = g->eos_par[0] * g->eos_par[1] * g->eos_par[1] / g->eos_par[2];
        a.e_gk = tait_gk(g->eos_par[2]);
        a.e_p0 = g->eos_par[3];
    }
    if (L.rl.kind == REC_TVFF) { a.e_p0 = g->eos_par[0]; a.e_rho01 = 1.0 / g->eos_par[1]; a.e_B = g->eos_par[2]; } // StateEquation: p0 rho0 b
    return a;
}

// output properties of the destination: created where missing, then bound to the launch arguments
struct OutBind { int prop; double **to; };
static int bind_out(const PairLaunch &L, std::initializer_list<OutBind> outs)
{
    for (const OutBind &o : outs) SPH_TRY(sph_array_ensure_prop(L.c, L.P.dst, o.prop));
    for (const OutBind &o : outs) *o.to = L.c->arr[L.P.dst].prop[o.prop];
    return SPH_OK;
}

// Continuity / Momentum / XSPH: parameters and outputs, the same for the WCSPH families and the WCSPH-options family
template <class F> static int bind_wcsph(const PairLaunch &L, PairArgs<F> &a)
{
    const uint32_t dflags = L.P.dflags;
    const sph_equation *me = L.P.eq_of[SPH_EQ_MOMENTUM], *xe = L.P.eq_of[SPH_EQ_XSPH];
    if (me) { a.p.c0 = me->par[0]; a.p.alpha = me->par[1]; a.p.beta = me->par[2]; a.p.gx = me->par[3]; a.p.gy = me->par[4]; a.p.gz = me->par[5]; }
    if (xe) a.p.eps = xe->par[0];
    if (dflags & F_CONT) SPH_TRY(bind_out(L, {{SPH_ARHO, &a.p.arho}}));
    if (dflags & F_MOM)
        SPH_TRY(bind_out(L, {{SPH_AU, &a.p.au}, {SPH_AV, &a.p.av}, {SPH_AW, &a.p.aw}, {SPH_DT_CFL, &a.p.dt_cfl}, {SPH_DT_FORCE, &a.p.dt_force}}));
    if (dflags & F_XSPH) SPH_TRY(bind_out(L, {{SPH_AX, &a.p.ax}, {SPH_AY, &a.p.ay}, {SPH_AZ, &a.p.az}}));
    return SPH_OK;
}
template <class F> static int run_wcsph(const PairLaunch &L)
{
    PairArgs<F> a = pair_args<F>(L);
    SPH_TRY(bind_wcsph(L, a));
    if constexpr (std::is_same<F, FamWCSPHV_T<typename F::Real>>::value) return launch_pair_fused<F, false>(L.c, L.K->kind, a);
    else if constexpr (fam_eosf<F>::value) return launch_pair_fused<F>(L.c, L.K->kind, a);
    else return launch_pair<F>(L.c, L.K->kind, a, L.rl.record_f32);
}
// the WCSPH-options family: FamWCSPH_T's arguments + the parameters of the extra terms
template <class F> static int run_wcsphx(const PairLaunch &L)
{
    PairArgs<F> a = pair_args<F>(L);
    const sph_equation *dc = L.P.eq_of[SPH_EQ_CONTINUITY_DELTA_SPH], *dm = L.P.eq_of[SPH_EQ_MOMENTUM_DELTA_SPH],
                       *lv = L.P.eq_of[SPH_EQ_LAMINAR_VISCOSITY], *ld = L.P.eq_of[SPH_EQ_LAMINAR_VISCOSITY_DELTA_SPH];
    if (dc) a.p.dfac = dc->par[1] * dc->par[0];                  // par c0 delta
    if (dm) a.p.mfac = dm->par[2] * dm->par[1] * dm->par[0];     // par rho0 c0 alpha
    if (lv) { a.p.nu4 = 4.0 * lv->par[0]; a.p.eta = lv->par[1]; } // par nu eta
    if (ld) a.p.lfac = 2.0 * (ld->par[0] + 2.0) * ld->par[2] * ld->par[1]; // par dim rho0 nu
    SPH_TRY(bind_wcsph(L, a));
    return launch_pair<F>(L.c, L.K->kind, a, L.rl.record_f32);
}
// the delta-SPH pre-passes: the moment matrix, or the (renormalised) density gradient
template <class F> static int run_dspre(const PairLaunch &L)
{
    const uint32_t dflags = L.P.dflags;
    const DevArray &D = L.c->arr[L.P.dst];
    PairArgs<F> a = pair_args<F>(L);
    const sph_equation *pe = L.P.eq_of[SPH_EQ_GRADIENT_CORRECTION_PRESTEP], *ge = L.P.eq_of[SPH_EQ_GRADIENT_CORRECTION];
    a.p.mdim = pe ? (int)pe->par[0] : 0;
    a.p.n = 0;
    if (dflags & F_GCORR) { a.p.n = (int)ge->par[0]; a.p.tol = ge->par[1]; }
    if (a.p.mdim < 0 || a.p.mdim > 3 || ((dflags & F_GCORR) && (a.p.n < 1 || a.p.n > 3))) {
        sph_set_error("GradientCorrection / GradientCorrectionPreStep: dim must be 1, 2 or 3");
        return SPH_ERR_ARG;
    }
    if (dflags & (F_MOMENT | F_GCORR)) {
        for (int k = 0; k < 9; k++) {
            const int pid = SPH_MMAT0 + k;
            if (dflags & F_MOMENT) SPH_TRY(sph_array_ensure_prop(L.c, L.P.dst, pid));
            else if (!D.prop[pid]) return need_prop(L.c, L.P.dst, pid, "GradientCorrection (m_mat)");
            a.p.mm[k] = D.prop[pid];
        }
    }
    if (dflags & F_GRADRHO)
        for (int k = 0; k < 3; k++) SPH_TRY(bind_out(L, {{SPH_GRADRHO0 + k, &a.p.gr[k]}}));
    return launch_pair<F>(L.c, L.K->kind, a, L.rl.record_f32);
}
template <class F> static int run_density(const PairLaunch &L)
{
    const uint32_t dflags = L.P.dflags;
    PairArgs<F> a = pair_args<F>(L);
    SPH_TRY(bind_out(L, {{SPH_RHO, &a.p.rho}}));
    if (dflags & F_TVFSD) SPH_TRY(bind_out(L, {{SPH_VOL, &a.p.V}}));
    if ((dflags & F_SD) && (dflags & F_TVFSD)) { sph_set_error("both SummationDensity flavours on one destination"); return SPH_ERR_UNSUPPORTED; }
    return launch_pair<F>(L.c, L.K->kind, a, L.rl.record_f32);
}
template <class F> static int run_vgrad(const PairLaunch &L)
{
    const uint32_t dflags = L.P.dflags;
    PairArgs<F> a = pair_args<F>(L);
    static const int vp[9] = {SPH_V00, SPH_V01, SPH_V02, SPH_V10, SPH_V11, SPH_V12, SPH_V20, SPH_V21, SPH_V22};
    if ((dflags & F_VG2) && (dflags & F_VG3)) { sph_set_error("both VelocityGradient2D and 3D on one destination"); return SPH_ERR_UNSUPPORTED; }
    for (int k = 0; k < 9; k++) {
        const bool used = (dflags & F_VG3) || (k == 0 || k == 1 || k == 3 || k == 4);
        if (used) SPH_TRY(bind_out(L, {{vp[k], &a.p.v[k]}}));
    }
    return launch_pair<F>(L.c, L.K->kind, a, L.rl.record_f32);
}
template <class F> static int run_elastic(const PairLaunch &L)
{
    sph_ctx *c = L.c;
    const DestPlan &P = L.P;
    const uint32_t dflags = P.dflags;
    PairArgs<F> a = pair_args<F>(L);
    const sph_equation *se = P.eq_of[SPH_EQ_MOMENTUM_WITH_STRESS], *ae = P.eq_of[SPH_EQ_MONAGHAN_ART_VISCOSITY],
                       *xe = P.eq_of[SPH_EQ_XSPH];
    if (se) { a.p.wdeltap = se->par[0]; a.p.n = se->par[1]; }
    a.p.tension = nullptr;
    if (L.rl.kind == REC_ELU && c->tension_flag && P.nsrcs == 1 && c->arr[P.srcs[0]].tflag_valid && c->arr[P.srcs[0]].tflag.ptr) {
        a.p.tension = c->arr[P.srcs[0]].tflag.as<uint32_t>();
        c->timers[T_N_TFLAG].count++;
    }
    if (ae) { a.p.alpha = ae->par[0]; a.p.beta = ae->par[1]; }
    if (xe) a.p.eps = xe->par[0];
    if (dflags & F_ECONT) SPH_TRY(bind_out(L, {{SPH_ARHO, &a.p.arho}}));
    if (dflags & (F_ESTRESS | F_EAV)) SPH_TRY(bind_out(L, {{SPH_AU, &a.p.au}, {SPH_AV, &a.p.av}, {SPH_AW, &a.p.aw}}));
    if (dflags & F_EXSPH) SPH_TRY(bind_out(L, {{SPH_AX, &a.p.ax}, {SPH_AY, &a.p.ay}, {SPH_AZ, &a.p.az}}));
    if constexpr (fam_eosf<F>::value) return launch_pair_fused<F>(c, L.K->kind, a);
    else return launch_pair<F>(c, L.K->kind, a, L.rl.record_f32);
}
// The TVF force terms, which the EDAC force group carries too.  pe: the family's pressure-gradient equation of the
// transport-velocity form (par pb gx gy gz tdamp); force / hat: the launch writes au av aw / auhat avhat awhat
template <class F> static int bind_tvf(const PairLaunch &L, PairArgs<F> &a, const sph_equation *pe, bool force, bool hat)
{
    const sph_equation *ve = L.P.eq_of[SPH_EQ_TVF_MOM_VISCOSITY], *ae = L.P.eq_of[SPH_EQ_TVF_MOM_ART_VISCOSITY];
    if (pe) { a.p.pb = pe->par[0]; a.p.gx = pe->par[1]; a.p.gy = pe->par[2]; a.p.gz = pe->par[3]; a.p.tdamp = pe->par[4]; }
    if (ve) a.p.nu = ve->par[0];
    if (ae) { a.p.c0 = ae->par[0]; a.p.alpha = ae->par[1]; }
    if (force) SPH_TRY(bind_out(L, {{SPH_AU, &a.p.au}, {SPH_AV, &a.p.av}, {SPH_AW, &a.p.aw}}));
    a.p.m = L.c->arr[L.P.dst].prop[SPH_M];
    if (hat) SPH_TRY(bind_out(L, {{SPH_AUHAT, &a.p.auhat}, {SPH_AVHAT, &a.p.avhat}, {SPH_AWHAT, &a.p.awhat}}));
    return SPH_OK;
}
template <class F> static int run_tvf(const PairLaunch &L)
{
    PairArgs<F> a = pair_args<F>(L);
    SPH_TRY(bind_tvf(L, a, L.P.eq_of[SPH_EQ_TVF_MOM_PRESSURE], true, (L.P.dflags & F_TP) != 0));
    if constexpr (fam_eosf<F>::value) return launch_pair_fused<F>(L.c, L.K->kind, a);
    else return launch_pair<F>(L.c, L.K->kind, a, L.rl.record_f32);
}
// the EDAC force group: parameters of its up to six equations; ap and pavg are user properties by name
template <class F> static int run_edac(const PairLaunch &L)
{
    sph_ctx *c = L.c;
    const DestPlan &P = L.P;
    const uint32_t dflags = P.dflags;
    PairArgs<F> a = pair_args<F>(L);
    const sph_equation *me = P.eq_of[SPH_EQ_EDAC_MOMENTUM], *ee = P.eq_of[SPH_EQ_EDAC], *xe = P.eq_of[SPH_EQ_XSPH];
    if (me) { a.p.gx = me->par[1]; a.p.gy = me->par[2]; a.p.gz = me->par[3]; a.p.tdamp = me->par[4]; } // par c0 gx gy gz tdamp
    if (ee) { a.p.cs2 = ee->par[0] * ee->par[0]; a.p.enu = ee->par[1]; } // par cs nu rho0
    if (xe) a.p.eps = xe->par[0];
    SPH_TRY(bind_tvf(L, a, P.eq_of[SPH_EQ_EDAC_MOM_PRESSURE], (dflags & (F_EP | F_TVISC | F_TAV | F_TAS)) != 0, (dflags & F_EINT) != 0));
    if (dflags & F_EINT) {
        const int ppavg = sph_prop_register("pavg");
        if (ppavg < 0) return ppavg;
        SPH_TRY(need_prop(c, P.dst, ppavg, "MomentumEquationPressureGradient of EDAC (pavg)"));
        a.p.pavg = c->arr[P.dst].prop[ppavg];
    }
    if (dflags & F_EDAC) {
        const int pap = sph_prop_register("ap");
        if (pap < 0) return pap;
        SPH_TRY(bind_out(L, {{pap, &a.p.ap}}));
    }
    if (dflags & F_EXS) SPH_TRY(bind_out(L, {{SPH_AX, &a.p.ax}, {SPH_AY, &a.p.ay}, {SPH_AZ, &a.p.az}}));
    return launch_pair<F>(c, L.K->kind, a, L.rl.record_f32);
}
template <class F> static int run_avgp(const PairLaunch &L)
{
    const uint32_t dflags = L.P.dflags;
    PairArgs<F> a = pair_args<F>(L);
    if ((dflags & F_SD) && (dflags & F_TVFSD)) { sph_set_error("both SummationDensity flavours on one destination"); return SPH_ERR_UNSUPPORTED; }
    if (dflags & (F_SD | F_TVFSD)) SPH_TRY(bind_out(L, {{SPH_RHO, &a.p.rho}}));
    if (dflags & F_TVFSD) SPH_TRY(bind_out(L, {{SPH_VOL, &a.p.V}}));
    const int ppavg = sph_prop_register("pavg"), pnn = sph_prop_register("nnbr");
    if (ppavg < 0 || pnn < 0) return SPH_ERR_ARG;
    SPH_TRY(bind_out(L, {{ppavg, &a.p.pavg}, {pnn, &a.p.nnbr}}));
    return launch_pair<F>(L.c, L.K->kind, a, L.rl.record_f32);
}
// the gas-dynamics density sweep: when it iterates, the convergence word is cleared before the launch and read
// back behind it (one word, one synchronise per call), and h counts as written
template <class F> static int run_gassd(const PairLaunch &L)
{
    sph_ctx *c = L.c;
    const int dst = L.P.dst;
    DevArray &D = c->arr[dst];
    PairArgs<F> a = pair_args<F>(L);
    const sph_equation *se = L.P.eq_of[SPH_EQ_GASD_SUMMATION_DENSITY]; // par dim k htol density_iterations iterate_only_once
    a.p.dim = se->par[0]; a.p.k = se->par[1]; a.p.htol = se->par[2];
    a.p.iterate = se->par[3] != 0.0; a.p.once = se->par[4] != 0.0;
    const char *names[5] = {"grhox", "grhoy", "grhoz", "dwdh", "div"};
    int ids[5];
    for (int k = 0; k < 5; k++) { ids[k] = sph_prop_register(names[k]); if (ids[k] < 0) return ids[k]; }
    SPH_TRY(bind_out(L, {{SPH_RHO, &a.p.rho}, {SPH_ARHO, &a.p.arho}, {ids[0], &a.p.grhox}, {ids[1], &a.p.grhoy},
                              {ids[2], &a.p.grhoz}, {ids[3], &a.p.dwdh}, {ids[4], &a.p.div}}));
    if (a.p.iterate) {
        const int ph0 = sph_prop_register("h0"), pom = sph_prop_register("omega"), pah = sph_prop_register("ah"),
                  pcv = sph_prop_register("converged");
        if (ph0 < 0 || pom < 0 || pah < 0 || pcv < 0) return SPH_ERR_ARG;
        SPH_TRY(need_prop(c, dst, ph0, "SummationDensity of gas dynamics (h0)"));
        SPH_TRY(need_prop(c, dst, pcv, "SummationDensity of gas dynamics (converged)"));
        SPH_TRY(need_prop(c, dst, SPH_M, "SummationDensity of gas dynamics (m)"));
        SPH_TRY(bind_out(L, {{pom, &a.p.omega}, {pah, &a.p.ah}}));
        a.p.m = D.prop[SPH_M]; a.p.h0 = D.prop[ph0]; a.p.h = D.prop[SPH_H];
        a.p.converged = D.prop[pcv];
        if (c->gasd_skip && wave_tiles(c)) {
            // the raw arho of every row is kept by every sweep; a repeated call may use what the previous one kept
            const bool had = D.gasd_araw.ptr && D.gasd_araw.bytes >= D.n * sizeof(double);
            SPH_TRY(D.gasd_araw.reserve(D.n * sizeof(double), true, c->stream));
            a.p.araw = D.gasd_araw.as<double>();
            a.p.skip = c->gasd_repeat && had;
        }
        SPH_TRY(c->gen_state.reserve(SPH_GEN_MAX_STATE * sizeof(double)));
        a.p.flag = c->gen_state.as<uint32_t>();
        HIP_TRY(hipMemsetAsync(a.p.flag, 0, 2 * sizeof(uint32_t), c->stream));
    }
    SPH_TRY(launch_pair<F>(c, L.K->kind, a, L.rl.record_f32));
    if (a.p.iterate) {
        uint32_t word[2] = {0, 0};
        HIP_TRY(hipMemcpyAsync(word, a.p.flag, sizeof word, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->gasd_unconverged |= word[0];
        c->timers[T_N_GASD_SKIP].count += word[1];
        // h changed behind the neighbour grid (as UpdateSmoothingLengthFerrari in run_nosrc)
        sph_mark_written(D, SPH_H);
        c->uniform_h = false;
    }
    return SPH_OK;
}
template <class F> static int run_mpm(const PairLaunch &L)
{
    const DevArray &D = L.c->arr[L.P.dst];
    PairArgs<F> a = pair_args<F>(L);
    const sph_equation *me = L.P.eq_of[SPH_EQ_MPM_ACCELERATIONS]; // par beta sigma alpha1_min alpha2_min update_alpha1 update_alpha2
    a.p.beta = me->par[0]; a.p.sigma = me->par[1]; a.p.alpha1_min = me->par[2]; a.p.alpha2_min = me->par[3];
    a.p.update_alpha1 = me->par[4] != 0.0; a.p.update_alpha2 = me->par[5] != 0.0;
    const int pa1 = sph_prop_register("alpha1"), pa2 = sph_prop_register("alpha2"), paa1 = sph_prop_register("aalpha1"),
              paa2 = sph_prop_register("aalpha2"), pd2 = sph_prop_register("del2e"), pdv = sph_prop_register("div"),
              pom = sph_prop_register("omega");
    if (pa1 < 0 || pa2 < 0 || paa1 < 0 || paa2 < 0 || pd2 < 0 || pdv < 0 || pom < 0) return SPH_ERR_ARG; // (the records carry omega, alpha1, alpha2)
    SPH_TRY(bind_out(L, {{SPH_AU, &a.p.au}, {SPH_AV, &a.p.av}, {SPH_AW, &a.p.aw}, {SPH_AE, &a.p.ae}, {SPH_DT_CFL, &a.p.dt_cfl},
                              {paa1, &a.p.aalpha1}, {paa2, &a.p.aalpha2}, {pd2, &a.p.del2e}}));
    if (a.p.update_alpha1) SPH_TRY(need_prop(L.c, L.P.dst, pdv, "MPMAccelerations (div)"));
    a.p.h = D.prop[SPH_H]; a.p.cs = D.prop[SPH_CS]; a.p.e = D.prop[SPH_E]; a.p.div = D.prop[pdv];
    a.p.alpha1 = D.prop[pa1]; a.p.alpha2 = D.prop[pa2];
    return launch_pair<F>(L.c, L.K->kind, a, L.rl.record_f32);
}

// ---- ADKE: what runs around its sweeps ---------------------------------------------------------------------------
// `h = h0` of SummationDensityADKE.initialize / WallBoundary.initialize over the destinations, BEFORE their records are
// packed: the sweep then reads the destination's h0 as its h, from the record
__global__ __launch_bounds__(256) void k_adke_h_reset(double *__restrict__ h, const double *__restrict__ h0, size_t start, size_t stop)
{
    const size_t i = start + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < stop) h[i] = h0[i];
}
// The sum of a column in a FIXED order: thread t of block b takes rows b * 256 + t, + gridDim * 256, ...; a wavefront
// folds by xor-shuffles, a block adds its four wavefronts in order, and one further block folds the partial sums the
// same way.  The grid is a function of n alone, so two runs add in the same order; no floating-point atomics.
__global__ __launch_bounds__(256) void k_adke_sum(const double *__restrict__ v, size_t n, double *__restrict__ out)
{
    double s = 0.0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) s += v[i];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    __shared__ double sh[4];
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}
// SummationDensityADKE.reduce (:64-71) for every row: h = k (exp(S / n) / rho)^eps h0, S read from the device word
__global__ __launch_bounds__(256) void k_adke_h(double *__restrict__ h, const double *__restrict__ h0, const double *__restrict__ rho,
                                                const double *__restrict__ sum, size_t n, double k, double eps)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double g = exp(*sum / (double)n);
    h[i] = k * pow(g / rho[i], eps) * h0[i];
}

// h changed behind the neighbour grid (as UpdateSmoothingLengthFerrari in run_nosrc): no pair loop may take "every
// particle has the h the last update saw" as a launch constant or a record layout, no records packed before and no
// neighbour lists kept before may be read again
static void adke_h_written(sph_ctx *c, int id)
{
    sph_mark_written(c->arr[id], SPH_H);
    c->uniform_h = false;
    c->pack_cache[id].epoch = 0;
    c->nl.valid = false;
}

// before the records of a SummationDensityADKE / WallBoundary destination are chosen and packed: h = h0 on the
// destinations; the wall's output columns exist from here on (its own record is read for x y z h only)
static int adke_before_records(sph_ctx *c, const DestPlan &P)
{
    DevArray &D = c->arr[P.dst];
    const char *who = P.fam == FAM_GASWALL ? "WallBoundary" : "SummationDensityADKE";
    if (P.phase != 0) { sph_set_error("%s: not in a split evaluation (sph_group.phase)", who); return SPH_ERR_UNSUPPORTED; }
    const int ph0 = sph_prop_register("h0");
    if (ph0 < 0) return ph0;
    SPH_TRY(need_prop(c, P.dst, ph0, who));
    SPH_TRY(need_prop(c, P.dst, SPH_H, who));
    if (P.fam == FAM_GASWALL) {
        const int pdiv = sph_prop_register("div");
        if (pdiv < 0) return pdiv;
        for (int p : {(int)SPH_U, (int)SPH_V, (int)SPH_W, (int)SPH_RHO, (int)SPH_P, (int)SPH_CS, (int)SPH_E, (int)SPH_M, pdiv}) SPH_TRY(sph_array_ensure_prop(c, P.dst, p));
    }
    if (P.stop > P.start) {
        ScopedTimer tm(c, T_EOS);
        hipLaunchKernelGGL(k_adke_h_reset, dim3(div_up(P.stop - P.start, 256)), dim3(256), 0, c->stream, D.prop[SPH_H], D.prop[ph0], P.start, P.stop);
    }
    adke_h_written(c, P.dst);
    return SPH_OK;
}

// the ADKE density sweep, then what the reference's reduce hook does, on the device: the sum of logrho over EVERY row of
// the destination (the rows behind the real ones with whatever logrho they hold, as `serial_reduce_array(dst.logrho)`
// sums them) into one device word, and the new h of every row from it.  Nothing is read back.
template <class F> static int run_adke_sd(const PairLaunch &L)
{
    sph_ctx *c = L.c;
    const int dst = L.P.dst;
    DevArray &D = c->arr[dst];
    PairArgs<F> a = pair_args<F>(L);
    const sph_equation *se = L.P.eq_of[SPH_EQ_SUMMATION_DENSITY_ADKE]; // par k eps
    const int ph0 = sph_prop_register("h0"), pdiv = sph_prop_register("div"), plr = sph_prop_register("logrho");
    if (ph0 < 0 || pdiv < 0 || plr < 0) return SPH_ERR_ARG;
    SPH_TRY(bind_out(L, {{SPH_RHO, &a.p.rho}, {SPH_ARHO, &a.p.arho}, {pdiv, &a.p.div}, {plr, &a.p.logrho}}));
    SPH_TRY(launch_pair<F>(c, L.K->kind, a, L.rl.record_f32));
    const size_t n = D.n;
    if (n == 0) return SPH_OK;
    const int nb = (int)std::min<size_t>(512, div_up(n, 256));
    SPH_TRY(c->red_part.reserve(1024 * sizeof(double)));
    double *part = c->red_part.as<double>();
    {
        ScopedTimer tm(c, T_EOS);
        hipLaunchKernelGGL(k_adke_sum, dim3(nb), dim3(256), 0, c->stream, D.prop[plr], n, part);
        hipLaunchKernelGGL(k_adke_sum, dim3(1), dim3(256), 0, c->stream, part, (size_t)nb, part + 512);
        hipLaunchKernelGGL(k_adke_h, dim3(div_up(n, 256)), dim3(256), 0, c->stream, D.prop[SPH_H], D.prop[ph0], D.prop[SPH_RHO],
                           part + 512, n, se->par[0], se->par[1]);
    }
    adke_h_written(c, dst);
    return SPH_OK;
}
template <class F> static int run_adke(const PairLaunch &L)
{
    typedef typename F::Real T;
    PairArgs<F> a = pair_args<F>(L);
    const sph_equation *ae = L.P.eq_of[SPH_EQ_ADKE_ACCELERATIONS]; // par alpha beta g1 g2 k eps
    a.p.alpha = (T)ae->par[0]; a.p.beta = (T)ae->par[1]; a.p.g1 = (T)ae->par[2]; a.p.g2 = (T)ae->par[3];
    if (L.rl.pl.props[8] < 0) { sph_set_error("ADKEAccelerations: no user property slot left for div"); return SPH_ERR_ARG; }
    SPH_TRY(bind_out(L, {{SPH_AU, &a.p.au}, {SPH_AV, &a.p.av}, {SPH_AW, &a.p.aw}, {SPH_AE, &a.p.ae}}));
    return launch_pair<F>(L.c, L.K->kind, a, L.rl.record_f32);
}
// the wall sweep writes h and m of the wall array: both count as written
template <class F> static int run_gas_wall(const PairLaunch &L)
{
    sph_ctx *c = L.c;
    PairArgs<F> a = pair_args<F>(L);
    const int pdiv = sph_prop_register("div"), pwij = sph_prop_register("wij"), pht = sph_prop_register("htmp");
    if (pdiv < 0 || pwij < 0 || pht < 0 || L.rl.pl.props[8] < 0) { sph_set_error("WallBoundary: no user property slot left for div, wij, htmp"); return SPH_ERR_ARG; }
    SPH_TRY(bind_out(L, {{pwij, &a.p.wij}, {SPH_P, &a.p.p}, {SPH_U, &a.p.u}, {SPH_V, &a.p.v}, {SPH_W, &a.p.w}, {SPH_M, &a.p.m},
                              {SPH_RHO, &a.p.rho}, {SPH_E, &a.p.e}, {SPH_CS, &a.p.cs}, {pdiv, &a.p.div}, {pht, &a.p.htmp}, {SPH_H, &a.p.h}}));
    SPH_TRY(launch_pair<F>(c, L.K->kind, a, L.rl.record_f32));
    adke_h_written(c, L.P.dst);
    sph_mark_written(c->arr[L.P.dst], SPH_M);
    return SPH_OK;
}

template <class F> static int run_gsph_grad(const PairLaunch &L)
{
    PairArgs<F> a = pair_args<F>(L);
    static const char *names[12] = {"px", "py", "pz", "ux", "uy", "uz", "vx", "vy", "vz", "wx", "wy", "wz"};
    for (int k = 0; k < 12; k++) {
        const int id = sph_prop_register(names[k]);
        if (id < 0) return id;
        SPH_TRY(bind_out(L, {{id, &a.p.g[k]}}));
    }
    return launch_pair<F>(L.c, L.K->kind, a, L.rl.record_f32);
}
// the GSPH force sweep; the failure word is cleared by the first such launch of a call (sph_gsph_failures reads it)
template <class F> static int run_gsph(const PairLaunch &L)
{
    typedef typename F::Real T;
    sph_ctx *c = L.c;
    PairArgs<F> a = pair_args<F>(L);
    // par g1 g2 monotonicity rsolver interpolation interface_zero hybrid blend_alpha tf gamma niter tol
    const sph_equation *ge = L.P.eq_of[SPH_EQ_GSPH_ACCELERATION];
    const double *par = ge->par;
    a.p.g1 = (T)par[0]; a.p.g2 = (T)par[1];
    a.p.monotonicity = (int)par[2]; a.p.rsolver = (int)par[3]; a.p.interpolation = (int)par[4];
    a.p.interface_zero = par[5] != 0.0; a.p.hybrid = par[6] != 0.0;
    a.p.blend = (T)exp(-par[7] * L.t / par[8]); // gsph.py:232, once per launch
    a.p.gamma = (T)par[9]; a.p.niter = (int)par[10]; a.p.tol = (T)par[11];
    a.p.conduction = !(par[0] == 0.0 && par[1] == 0.0);
    if (a.p.rsolver < 0 || a.p.rsolver > 10 || a.p.monotonicity < 0 || a.p.monotonicity > 2 || a.p.interpolation < 0 || a.p.interpolation > 2) {
        sph_set_error("GSPHAcceleration: rsolver %d (0..10), monotonicity %d (0..2) or interpolation %d (0..2) out of range",
                      a.p.rsolver, a.p.monotonicity, a.p.interpolation);
        return SPH_ERR_ARG;
    }
    for (int k = 8; k < 24; k++) if (L.rl.pl.props[k] < 0) { sph_set_error("GSPHAcceleration: no user property slot left for its gradient columns"); return SPH_ERR_ARG; }
    SPH_TRY(bind_out(L, {{SPH_AU, &a.p.au}, {SPH_AV, &a.p.av}, {SPH_AW, &a.p.aw}, {SPH_AE, &a.p.ae}}));
    SPH_TRY(c->gsph_word.reserve(64));
    a.p.fail = c->gsph_word.as<unsigned long long>();
    if (!c->gsph_cleared && !c->gsph_keep) {
        HIP_TRY(hipMemsetAsync(a.p.fail, 0, sizeof(unsigned long long), c->stream));
        c->gsph_cleared = true;
    }
    return launch_pair<F>(c, L.K->kind, a, L.rl.record_f32);
}

// the family instantiation the plan and the records name, in the arithmetic type of the records
static int launch_family(const PairLaunch &L)
{
    const int fam = L.P.fam;
    const RecordKind kind = L.rl.kind;
    const bool g7 = tait_gk(L.g->eos_par[2]) == 3; // the usual exponent: kernels that fold it
// RUN(binder, family in T): T = float with fp32 arithmetic (option arith_f32), else double
#define RUN(BIND, ...)                                                      \
    do {                                                                    \
        if (L.rl.arith_f32) { using T = float; return BIND<__VA_ARGS__>(L); } \
        else { using T = double; return BIND<__VA_ARGS__>(L); }               \
    } while (0)
    if (fam == FAM_WCSPH && kind == REC_EOSF && L.rl.umass && g7) RUN(run_wcsph, FamWCSPHE_T<T, true>);
    if (fam == FAM_WCSPH && kind == REC_EOSF && g7) RUN(run_wcsph, FamWCSPHE_T<T>);
    if (fam == FAM_WCSPH && kind == REC_EOSF && L.rl.umass) RUN(run_wcsph, FamWCSPHEG_T<T, true>);
    if (fam == FAM_WCSPH && kind == REC_EOSF) RUN(run_wcsph, FamWCSPHEG_T<T>);
    if (fam == FAM_WCSPH && kind == REC_EOSV) RUN(run_wcsph, FamWCSPHV_T<T>);
    if (fam == FAM_WCSPH) RUN(run_wcsph, FamWCSPH_T<T>);
    if (fam == FAM_WCSPHX && (L.P.dflags & F_DCONT)) RUN(run_wcsphx, FamWCSPHX_T<T, true>); // (the records carry gradrho)
    if (fam == FAM_WCSPHX) RUN(run_wcsphx, FamWCSPHX_T<T, false>);
    if (fam == FAM_DSPRE) RUN(run_dspre, FamDSPre_T<T>);
    if (fam == FAM_DENSITY) RUN(run_density, FamDensity_T<T>);
    if (fam == FAM_AVGP) RUN(run_avgp, FamAvgP_T<T>);
    if (fam == FAM_GASSD) RUN(run_gassd, FamGasSD_T<T>);
    if (fam == FAM_MPM) RUN(run_mpm, FamMPM_T<T>);
    if (fam == FAM_GSPHGRAD) RUN(run_gsph_grad, FamGSPHGrad_T<T>);
    if (fam == FAM_GSPH) RUN(run_gsph, FamGSPH_T<T>);
    if (fam == FAM_ADKESD) RUN(run_adke_sd, FamADKESD_T<T>);
    if (fam == FAM_ADKE) RUN(run_adke, FamADKE_T<T>);
    if (fam == FAM_GASWALL) RUN(run_gas_wall, FamGasWall_T<T>);
    if (fam == FAM_EDAC && (L.P.dflags & F_EINT)) RUN(run_edac, FamEDAC_T<T, true>);
    if (fam == FAM_EDAC) RUN(run_edac, FamEDAC_T<T, false>);
    if (fam == FAM_VGRAD) RUN(run_vgrad, FamVGrad_T<T>);
    if (fam == FAM_ELASTIC && kind == REC_ELU) RUN(run_elastic, FamElasticU_T<T>);
    if (fam == FAM_ELASTIC) RUN(run_elastic, FamElastic_T<T>);
    if (kind == REC_TVFF) RUN(run_tvf, FamTVFE_T<T>);
    RUN(run_tvf, FamTVF_T<T>);
#undef RUN
}

extern "C" int sph_eval_group(sph_ctx *c, const sph_kernel *K, const sph_group *g, double t, double dt)
{
    if (!c || !K || !g) { sph_set_error("sph_eval_group: NULL argument"); return SPH_ERR_ARG; }
    c->gasd_unconverged = 0;
    c->gsph_cleared = false;
    if (g->neq > SPH_MAX_EQS) { sph_set_error("sph_eval_group: too many equations"); return SPH_ERR_ARG; }
    SPH_TRY(check_kernel("sph_eval_group", K));
    HIP_TRY(hipSetDevice(c->device));
    if (!c->pack_group) c->pack_epoch++; // packed records are reused between the destinations of ONE group only (option pack_group)
    // src_eos = 3: the promise of 1, but the Tait EOS has not run yet.  The EOS-fused records of ONE array compute it while
    // they are packed (pack_array); everything else runs it here, first, and goes on as for 1.
    sph_group g_run;
    bool eos_pending = false;
    if (g->src_eos == 3) {
        g_run = *g;
        g_run.src_eos = 1;
        g = &g_run;
        eos_pending = true;
        if (c->merged_valid || g->phase != 0) { SPH_TRY(run_pending_eos(c, g)); eos_pending = false; }
    }
    {
        bool done = false;
        SPH_TRY(eval_group_merged(c, K, g, t, dt, &done));
        if (done) return SPH_OK;
    }
    int dests[SPH_MAX_ARRAYS], ndest = 0;
    SPH_TRY(resolve_destinations(c, g, dests, &ndest));
    for (int di = 0; di < ndest; di++) {
        DestPlan plan;
        plan.dst = dests[di]; plan.ndest = ndest; plan.phase = g->phase;
        const DevArray &D = c->arr[plan.dst];
        plan.start = g->start_idx > 0 ? (size_t)g->start_idx : 0;
        plan.stop = g->stop_idx >= 0 ? (size_t)g->stop_idx : (g->real ? D.n_real : D.n);
        if (plan.stop > D.n) plan.stop = D.n;
        SPH_TRY(run_nosrc_equations(c, g, plan.dst, plan.start, plan.stop));
        SPH_TRY(plan_destination(c, g, plan));
        const DestPlan &P = plan;
        if (P.fam == FAM_NONE) continue;
        if (P.fam == FAM_ADKESD || P.fam == FAM_GASWALL) SPH_TRY(adke_before_records(c, P)); // h = h0: the records and their layout see it
        const RecordLayout rl = choose_records(c, g, P, eos_pending);
        if (eos_pending) { // the Tait EOS the host left to this call: with the records (pack_array), or now, over all of every array
            eos_pending = false;
            if (rl.eos_abs) {
                SPH_TRY(need_prop(c, P.dst, SPH_RHO, "EOS"));
                SPH_TRY(sph_array_ensure_prop(c, P.dst, SPH_P));
                SPH_TRY(sph_array_ensure_prop(c, P.dst, SPH_CS));
                c->pack_cache[P.dst].epoch = 0; // the records are packed now, whatever an earlier destination left
                c->timers[T_N_EOSABS].count++;
            } else {
                SPH_TRY(run_pending_eos(c, g));
            }
        }
        SPH_TRY(pack_records(c, P, rl));
        int nl_mode = 0;
        SPH_TRY(choose_nl_mode(c, g, P, &nl_mode));
        // Split evaluations (sph_group.phase): by default the first half only prepares (equations without sources, records
        // of the particles present) and the second half launches EVERY wave tile once the ghosts are in -- the ghost
        // segments guarded per wavefront; option split_pair 1: the interior tiles in the first half, the face tiles in
        // the second (hides a transfer longer than the neighbour update + packing; costs a second, sparse launch)
        if (P.phase == 1 && !c->split_pair) continue;
        // the fused pair kernel, in the arithmetic type of the records (fp64, or fp32 with option arith_f32)
        ScopedTimer tm(c, T_PAIR);
        ScopedTimer tmf(c, T_PAIR_FAM + P.fam);
        if (P.phase == 2) c->timers[T_N_PHASE2].count++;
        if (rl.eos_fused() || rl.kind == REC_TVFF) c->timers[T_N_EOSF].count++;
        if (rl.umass || rl.kind == REC_TVFF || rl.kind == REC_ELU || rl.kind == REC_EOSV) c->timers[T_N_UMASS].count++;
        if (nl_mode == 1) c->timers[T_N_NLKEEP].count++;
        if (nl_mode == 2) c->timers[T_N_NLREUSE].count++;
        int nseg = P.nsrcs;
        for (int j = 0; j < P.nsrcs; j++) nseg += c->arr[P.srcs[j]].g_n > 0 && P.phase != 1;
        if (nseg > SPH_MAX_ARRAYS) { sph_set_error("too many source segments (%d arrays with ghost segments)", P.nsrcs); return SPH_ERR_UNSUPPORTED; }
        SPH_TRY(launch_family(PairLaunch{c, K, g, t, dt, P, rl, nl_mode}));
    }
    if (eos_pending) SPH_TRY(run_pending_eos(c, g)); // (no destination came as far as its records)
    HIP_TRY(hipGetLastError());
    return SPH_OK;
}

extern "C" int sph_gasd_unconverged(sph_ctx *c, int *flag)
{
    if (!c || !flag) { sph_set_error("sph_gasd_unconverged: NULL argument"); return SPH_ERR_ARG; }
    *flag = c->gasd_unconverged ? 1 : 0;
    return SPH_OK;
}

extern "C" int sph_gsph_failures(sph_ctx *c, unsigned long long *count)
{
    if (!c || !count) { sph_set_error("sph_gsph_failures: NULL argument"); return SPH_ERR_ARG; }
    *count = 0;
    if (!c->gsph_word.ptr) return SPH_OK; // no GSPH force sweep has run
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(count, c->gsph_word.ptr, sizeof *count, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SPH_OK;
}

// ---------------------------------------------------------------------------
// generated equation families (pysph_amd/codegen.py): pack the sources'
// records with the properties the generated bodies read, then call the
// module's launch function with plain pointers.
// ---------------------------------------------------------------------------
static int pack_generic(sph_ctx *c, int id, size_t off, int nprops, const int *props, int nr, int layout)
{
    DevArray &A = c->arr[id];
    if (A.n == 0) return SPH_OK;
    PackArgs pa;
    memset(&pa, 0, sizeof pa);
    pa.perm = A.perm.as<uint32_t>();
    pa.n = A.n;
    pa.off = off;
    pa.x = A.prop[SPH_X]; pa.y = A.prop[SPH_Y]; pa.z = A.prop[SPH_Z]; pa.h = A.prop[SPH_H];
    pa.na = nprops;
    for (int k = 0; k < nprops; k++) {
        pa.src[k] = A.prop[props[k]];
        if (!pa.src[k]) return need_prop(c, id, props[k], "generated pair loop");
    }
    pa.posh = c->posh.as<double4>();
    pa.aux = c->aux.as<double>();
    pa.rec = c->posh.as<double>();
    pa.nr = nr;
    pa.layout = layout;
    pa.fpos = c->fposb.as<float4>();
    for (int k = 0; k < 3; k++) pa.gmin[k] = c->xmin[k];
    pa.radius_scale = c->radius_scale;
    pa.lds_np = pack_pieces(pa);
    launch_pack(c, pa, A.n);
    return SPH_OK;
}

// the loop nest of one generated family; sph_eval_generated wraps it with the
// round trip of the equation attributes the device code assigns
static int eval_generated_launches(sph_ctx *c, const sph_kernel *K, const sph_gen_family *f, double t, double dt, double *d_state);

extern "C" int sph_eval_generated(sph_ctx *c, const sph_kernel *K, sph_gen_family *f, double t, double dt)
{
    if (!c || !K || !f || !f->launch) { sph_set_error("sph_eval_generated: NULL argument"); return SPH_ERR_ARG; }
    if (f->nstate < 0 || f->nstate > SPH_GEN_MAX_STATE) { sph_set_error("sph_eval_generated: nstate out of range"); return SPH_ERR_ARG; }
    double *d_state = nullptr;
    if (f->nstate > 0) {
        // self.<attr> = ... in an equation body (e.g. the convergence flag of an iterated group,
        // gas_dynamics/basic.py:121-160): values go in before the launches and come back after
        HIP_TRY(hipSetDevice(c->device));
        SPH_TRY(c->gen_state.reserve(SPH_GEN_MAX_STATE * sizeof(double)));
        d_state = c->gen_state.as<double>();
        HIP_TRY(hipMemcpyAsync(d_state, f->state, f->nstate * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    int rc = eval_generated_launches(c, K, f, t, dt, d_state);
    if (rc == SPH_OK && f->nstate > 0) {
        HIP_TRY(hipMemcpyAsync(f->state, d_state, f->nstate * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return rc;
}

static int eval_generated_launches(sph_ctx *c, const sph_kernel *K, const sph_gen_family *f, double t, double dt, double *d_state)
{
    if (!c || !K || !f || !f->launch) { sph_set_error("sph_eval_generated: NULL argument"); return SPH_ERR_ARG; }
    SPH_TRY(check_kernel("sph_eval_generated", K));
    if (f->dest < 0 || f->dest >= SPH_MAX_ARRAYS || !c->arr[f->dest].used) { sph_set_error("sph_eval_generated: bad dest array %d", f->dest); return SPH_ERR_ARG; }
    if (f->nsrc < 0 || f->nsrc > SPH_MAX_ARRAYS || f->n_sprops < 0 || f->n_sprops > SPH_GEN_MAX_SPROPS || f->n_sprops > MAX_AUX ||
        f->n_din < 0 || f->n_din > SPH_GEN_MAX_PROPS || f->n_dout < 0 || f->n_dout > SPH_GEN_MAX_PROPS || f->npar < 0 ||
        f->npar > SPH_GEN_MAX_PAR) {
        sph_set_error("sph_eval_generated: family descriptor out of range");
        return SPH_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(c->device));
    c->nl.valid = false; // a generated body may write positions or h: kept neighbour lists are not trusted across it
    const int dst = f->dest;
    DevArray &D = c->arr[dst];
    size_t start = f->start_idx > 0 ? (size_t)f->start_idx : 0;
    size_t stop = f->stop_idx >= 0 ? (size_t)f->stop_idx : (f->real ? D.n_real : D.n);
    if (stop > D.n) stop = D.n;
    if (f->transposed) {
        // the companion of a family that adds to source properties: every row of that source array (here: the
        // destination) which is in the neighbour grid takes part, ghosts included -- the reference writes to them too
        if (f->nsrc != 1 || f->loop_all || f->init_pair || f->split_init || f->nstate) {
            sph_set_error("sph_eval_generated: a transposed family has one source and pair loops only");
            return SPH_ERR_ARG;
        }
        start = 0; stop = D.n;
    }

    sph_gen_args g;
    memset(&g, 0, sizeof g);
    g.stream = (void *)c->stream;
    g.kernel_kind = K->kind;
    g.uniform_h = (c->uniform_h && c->use_uniform_h) ? 1 : 0;
    g.nsrc = f->nsrc;
    g.t = t; g.dt = dt;
    g.state = d_state;
    g.n_din = f->n_din; g.n_dout = f->n_dout; g.npar = f->npar;
    for (int k = 0; k < f->npar; k++) g.par[k] = f->par[k];
    for (int k = 0; k < f->n_dout; k++) {
        int p = f->dout[k];
        if (p < 0 || p >= SPH_PROP_COUNT) { sph_set_error("sph_eval_generated: bad output property %d", p); return SPH_ERR_ARG; }
        SPH_TRY(sph_array_ensure_prop(c, dst, p));
        g.dout[k] = D.prop[p];
        sph_mark_written(D, p); // a generated body writes h or m: the next neighbour update looks at them again
        if (p >= SPH_R00 && p <= SPH_R22) D.tflag_valid = false;
    }
    for (int k = 0; k < f->n_din; k++) {
        int p = f->din[k];
        if (p < 0 || p >= SPH_PROP_COUNT) { sph_set_error("sph_eval_generated: bad input property %d", p); return SPH_ERR_ARG; }
        if (!D.prop[p]) return need_prop(c, dst, p, "generated equation (destination)");
        g.din[k] = D.prop[p];
    }
    g.d_start = (uint32_t)start; g.d_stop = (uint32_t)stop;
    g.nd = (uint32_t)D.n;
    g.sigma = K->fac; g.deltap = K->deltap; g.dim = K->dim;
    g.row_mod3 = (int)c->row_mod3; g.norm_masks = (int)c->norm_masks;
    if (D.n == 0 || stop <= start) return SPH_OK;

    if (f->split_init) { // initialize for ALL particles before anything reads it as a source
        sph_gen_args gi = g;
        gi.mode = 1;
        gi.nsrc = 0;
        ScopedTimer tm(c, T_EOS);
        int rc = f->launch(&gi);
        if (rc != 0) { sph_set_error("generated family initialize launch failed (code %d)", rc); return SPH_ERR_HIP; }
        g.skip_init = 1;
    }

    // The per-source part of the loop nest.  `only` < 0: every source in one fused pass (the
    // normal case); otherwise just source `only` (families with initialize_pair and several
    // sources, which the reference sequences source by source: mako :62-110).
    auto loops = [&](int only, bool last) -> int {
        int idx[SPH_MAX_ARRAYS], ns = 0;
        for (int j = 0; j < f->nsrc; j++) if (only < 0 || only == j) idx[ns++] = j;
        sph_gen_args q = g;
        q.nsrc = ns;
        q.dflags = 0;
        if (ns > 0 && f->loop_all) {
            if (!c->nnps_valid) { sph_set_error("sph_eval_generated: neighbour grid is stale; call sph_nnps_update"); return SPH_ERR_STATE; }
            for (int jj = 0; jj < ns; jj++) {
                const int j = idx[jj], s = f->src[j];
                size_t total = 0;
                SPH_TRY(nnps_build_csr_device(c, s, dst, c->csr_start[jj], c->csr_nbrs[jj], &total));
                q.csr_start[jj] = c->csr_start[jj].as<uint32_t>();
                q.csr_nbrs[jj] = c->csr_nbrs[jj].as<uint32_t>();
                q.src_flags[jj] = f->src_flags[j];
                q.dflags |= f->src_flags[j];
                for (int k = 0; k < f->n_sprops; k++) {
                    const double *p = c->arr[s].prop[f->sprops[k]];
                    if (!p && c->arr[s].n) return need_prop(c, s, f->sprops[k], "generated loop_all");
                    q.sraw[jj][k] = p;
                }
            }
            q.mode = 2;
            q.radius_scale = c->radius_scale;
            q.skip_post = (f->also_pair || !last) ? 1 : 0;
            {
                ScopedTimer tm(c, T_PAIR);
                int rc = f->launch(&q);
                if (rc != 0) { sph_set_error("generated loop_all launch failed (code %d)", rc); return SPH_ERR_HIP; }
            }
            if (!f->also_pair) return SPH_OK;
            // the same family's pair loops follow (mako :62-110: loop_all, then loop, per source);
            // initialize has run (split launch), post_loop runs at the end of the pair launch
            q.mode = 0;
            q.skip_init = 1;
            q.dflags = 0;
        }
        q.skip_post = last ? 0 : 1;
        bool a32 = false;

        if (ns > 0) {
            if (!c->nnps_valid) { sph_set_error("sph_eval_generated: neighbour grid is stale; call sph_nnps_update"); return SPH_ERR_STATE; }
            if (D.nnps_slot < 0) { sph_set_error("destination array %d is not part of the neighbour grid", dst); return SPH_ERR_STATE; }
            if (c->ghosts_binned) { sph_set_error("generated families do not read ghost segments (ghost split): use the plain exchange -> sph_nnps_update order"); return SPH_ERR_UNSUPPORTED; }
            SPH_TRY(nnps_need_tables(c));
            size_t total = 0, off_of[SPH_MAX_ARRAYS];
            bool dest_is_src = false;
            for (int jj = 0; jj < ns; jj++) {
                const int s = f->src[idx[jj]];
                if (c->arr[s].nnps_slot < 0) { sph_set_error("source array %d is not part of the neighbour grid", s); return SPH_ERR_STATE; }
                off_of[jj] = total; total += c->arr[s].n; dest_is_src |= s == dst;
            }
            size_t d_off = total;
            if (!dest_is_src) total += D.n;
            else for (int jj = 0; jj < ns; jj++) if (f->src[idx[jj]] == dst) d_off = off_of[jj];
            if (total >= (1ull << 32)) { sph_set_error("too many particles for 32-bit packed indices"); return SPH_ERR_ARG; }
            const int na = f->n_sprops;
            // whole 16-byte pieces; under uniform h the records drop h: [x y z | aux...]
            const bool compact = q.uniform_h != 0;
            const int na_fam = ((na + 1) & ~1) < 2 ? 2 : ((na + 1) & ~1); // FamGen::NA
            // option arith_f32: the family's float build (fp32 records, arithmetic and accumulators), when the host gave one
            a32 = c->arith_f32 && f->launch_f32 != nullptr;
            const bool rf32 = c->record_f32 || a32;
            const int nr = rf32 ? ((4 + na_fam + 3) & ~3) /* floats */
                         : compact ? ((3 + na + 1) & ~1) : 4 + ((na + 1) & ~1);
            const int layout = rf32 ? 5 : (compact ? 4 : 0);
            q.rec_f32 = rf32 ? 1 : 0;
            SPH_TRY(c->posh.reserve((total + 64) * sizeof(double) * nr));
            for (auto &pc : c->pack_cache) pc.epoch = 0; // the generated family's records overwrite the shared WCSPH slots
            SPH_TRY(c->aux.reserve(64));
            SPH_TRY(c->fposb.reserve((total + 64) * sizeof(float4)));
            {
                ScopedTimer tm(c, T_PACK);
                for (int jj = 0; jj < ns; jj++) SPH_TRY(pack_generic(c, f->src[idx[jj]], off_of[jj], na, f->sprops, nr, layout));
                if (!dest_is_src) {
                    // the destination only needs its position record; properties it lacks are not read
                    int have[SPH_GEN_MAX_SPROPS], nh = 0;
                    for (int k = 0; k < na; k++) if (D.prop[f->sprops[k]]) have[nh++] = f->sprops[k];
                    SPH_TRY(pack_generic(c, dst, d_off, nh == na ? na : 0, f->sprops, nr, layout));
                }
            }
            q.rec = c->posh.as<double>();
            q.nrec = nr;
            q.fpos = c->fposb.as<float4>();
            q.dom_extent = fmax(fmax(c->xmax[0] - c->xmin[0], c->xmax[1] - c->xmin[1]), c->xmax[2] - c->xmin[2]);
            for (int k = 0; k < 3; k++) { q.nc[k] = c->nc[k]; q.xmin[k] = c->xmin[k]; }
            q.cell_size = c->cell_size;
            q.radius_scale = c->radius_scale;
            q.hu = 0.5 * (c->h_uniform + c->h_uniform);
            q.h1u = 1.0 / q.hu;
            q.facu = K->fac * q.h1u;
            if (K->dim > 1) q.facu *= q.h1u;
            if (K->dim > 2) q.facu *= q.h1u;
            q.epsu = 0.01 * q.hu * q.hu;
            q.hr2u = (c->radius_scale * c->h_uniform) * (c->radius_scale * c->h_uniform);
            for (int jj = 0; jj < ns; jj++) {
                const int j = idx[jj];
                q.src_cell_start[jj] = c->arr[f->src[j]].cell_start.as<uint32_t>();
                q.src_fine_start[jj] = c->arr[f->src[j]].fine_start.as<uint32_t>();
                q.src_off[jj] = (uint32_t)off_of[jj];
                q.src_flags[jj] = f->src_flags[j];
                q.dflags |= f->src_flags[j];
                q.src_perm[jj] = c->arr[f->src[j]].perm.as<uint32_t>();
            }
            q.d_off = (uint32_t)d_off;
            q.d_keys = D.keys_sorted.as<uint32_t>();
            q.d_fkeys = D.fkeys_sorted.as<uint32_t>();
            q.d_perm = D.perm.as<uint32_t>();
            q.d_tile_order = D.n_tiles ? D.tile_order.as<uint32_t>() : nullptr;
        }
        ScopedTimer tm(c, ns > 0 ? T_PAIR : T_EOS);
        int rc = (a32 ? f->launch_f32 : f->launch)(&q);
        if (rc != 0) { sph_set_error("generated family launch failed (code %d)", rc); return SPH_ERR_HIP; }
        return SPH_OK;
    };

    for (int j = 0; j < f->nsrc; j++) {
        const int s = f->src[j];
        if (s < 0 || s >= SPH_MAX_ARRAYS || !c->arr[s].used) { sph_set_error("bad source array %d", s); return SPH_ERR_ARG; }
        for (int i = 0; i < j; i++) if (f->src[i] == s) { sph_set_error("source array %d listed twice", s); return SPH_ERR_ARG; }
    }
    if (f->transposed) {
        // neighbours are the rows the forward loop visits as destinations: [start_idx, stop_idx) of the ORIGINAL group,
        // n_real under Group(real=True).  The cell tables of that array hold its other rows as well (ghosts of a
        // periodic domain, rows outside a start/stop range): the generated pair() looks the original index of a hit
        // up and drops those -- unless the range is the whole array
        const DevArray &N = c->arr[f->src[0]];
        size_t lo = f->t_start_idx > 0 ? (size_t)f->t_start_idx : 0;
        size_t hi = f->t_stop_idx >= 0 ? (size_t)f->t_stop_idx : (f->t_real ? N.n_real : N.n);
        if (hi > N.n) hi = N.n;
        if (N.n == 0 || hi <= lo) return SPH_OK; // the forward loop visits no row: nothing to add
        g.src_lo[0] = (uint32_t)lo; g.src_hi[0] = (uint32_t)hi;
        g.src_filter = (lo > 0 || hi < N.n) ? 1 : 0;
    }
    if (f->nsrc > 0 && f->init_pair) {
        // initialize_pair (mako :62-75): per source, before that source's loops, one sweep over
        // the destinations with the source's ARRAYS in view (mode 3; initialize ran as a split launch)
        g.skip_init = 1;
        for (int j = 0; j < f->nsrc; j++) {
            sph_gen_args gp = g;
            gp.mode = 3;
            gp.nsrc = 1;
            gp.src_flags[0] = f->src_flags[j];
            for (int k = 0; k < f->n_sprops; k++) gp.sraw[0][k] = c->arr[f->src[j]].prop[f->sprops[k]];
            const bool last = j == f->nsrc - 1;
            gp.skip_post = (f->init_pair == 2 && last) ? 0 : 1;
            {
                ScopedTimer tm(c, T_EOS);
                int rc = f->launch(&gp);
                if (rc != 0) { sph_set_error("generated initialize_pair launch failed (code %d)", rc); return SPH_ERR_HIP; }
            }
            if (f->init_pair == 1) SPH_TRY(loops(j, last));
        }
        return SPH_OK;
    }
    return loops(-1, true);
}

// ---------------------------------------------------------------------------
// max reduction (adaptive time step inputs: integrator.py:161-200)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_max(const double *__restrict__ v, size_t n, double *__restrict__ part, double sgn)
{
    double m = -INFINITY; // the identity of max: a range of nothing but -inf (min: +inf) reduces to that infinity
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        m = fmax(m, sgn * v[i]);
    for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
    __shared__ double s[4];
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = fmax(fmax(s[0], s[1]), fmax(s[2], s[3]));
}

static int reduce_minmax(sph_ctx *c, int id, int prop, double *out, bool want_max);

extern "C" int sph_reduce_max(sph_ctx *c, int id, int prop, double *out) { return reduce_minmax(c, id, prop, out, true); }
extern "C" int sph_reduce_min(sph_ctx *c, int id, int prop, double *out) { return reduce_minmax(c, id, prop, out, false); }

static int reduce_minmax(sph_ctx *c, int id, int prop, double *out, bool want_max)
{
    if (id < 0 || id >= SPH_MAX_ARRAYS || prop < 0 || prop >= SPH_PROP_COUNT || !c->arr[id].prop[prop]) {
        sph_set_error("sph_reduce_max: array %d has no device property %d", id, prop);
        return SPH_ERR_MISSING_PROP;
    }
    HIP_TRY(hipSetDevice(c->device));
    DevArray &A = c->arr[id];
    size_t n = A.n_real;
    const double sgn = want_max ? 1.0 : -1.0;
    if (n == 0) { *out = want_max ? -DBL_MAX : DBL_MAX; return SPH_OK; }
    int nb = (int)std::min<size_t>(512, (n + 255) / 256);
    SPH_TRY(c->red_part.reserve(1024 * sizeof(double)));
    hipLaunchKernelGGL(k_max, dim3(nb), dim3(256), 0, c->stream, A.prop[prop], n, c->red_part.as<double>(), sgn);
    hipLaunchKernelGGL(k_max, dim3(1), dim3(256), 0, c->stream, c->red_part.as<double>(), (size_t)nb,
                       c->red_part.as<double>() + 512, 1.0);
    HIP_TRY(hipMemcpyAsync(c->pinned, c->red_part.as<double>() + 512, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *out = sgn * c->pinned[0];
    return SPH_OK;
}

#endif // SPH_KERNEL_UNIT == 0

// ---------------------------------------------------------------------------
// interpolation of particle fields onto points (sph_interpolate)
// ---------------------------------------------------------------------------
#include "sph_interp.h"

// ---------------------------------------------------------------------------
// a kernel unit: the *_ext launch functions of ONE smoothing kernel, for every family the primary compile forwards
// (a family missing here is an undefined symbol when libsphhip.so is linked: the Makefile links with -z defs)
// ---------------------------------------------------------------------------
#if !SPH_PRIMARY_UNIT
template <class Fam, int K> int launch_pair_ext(sph_ctx *c, const PairArgs<Fam> &a, bool rec_f32) { return launch_pair_k<Fam, K>(c, a, rec_f32); }
template <class Fam, bool UHV, int K> int launch_pair_fused_ext(sph_ctx *c, const PairArgs<Fam> &a) { return launch_pair_fused_k<Fam, UHV, K>(c, a); }
template <class Fm, int K> int launch_pair_merged_ext(sph_ctx *c, const PairArgs<Fm> &a) { return launch_pair_merged_k<Fm, K>(c, a); }
template <class Fam, int K> int launch_interp_ext(sph_ctx *c, const PairArgs<Fam> &a) { return launch_interp_k<Fam, K>(c, a); }

#define UNIT_PAIR(F) template int launch_pair_ext<F, SPH_KERNEL_UNIT>(sph_ctx *, const PairArgs<F> &, bool)
#define UNIT_FUSED(F, UHV) template int launch_pair_fused_ext<F, UHV, SPH_KERNEL_UNIT>(sph_ctx *, const PairArgs<F> &)
#define UNIT_MERGED(F) template int launch_pair_merged_ext<F, SPH_KERNEL_UNIT>(sph_ctx *, const PairArgs<F> &)
#define UNIT_INTERP(F) template int launch_interp_ext<F, SPH_KERNEL_UNIT>(sph_ctx *, const PairArgs<F> &)
#define UNIT_BOTH(M, F) M(F<double>); M(F<float>)
UNIT_BOTH(UNIT_PAIR, FamWCSPH_T);
UNIT_BOTH(UNIT_PAIR, FamDensity_T);
UNIT_BOTH(UNIT_PAIR, FamTVF_T);
UNIT_BOTH(UNIT_PAIR, FamAvgP_T);
UNIT_BOTH(UNIT_PAIR, FamGasSD_T);
UNIT_BOTH(UNIT_PAIR, FamMPM_T);
UNIT_BOTH(UNIT_PAIR, FamGSPHGrad_T);
UNIT_BOTH(UNIT_PAIR, FamGSPH_T);
UNIT_BOTH(UNIT_PAIR, FamADKESD_T);
UNIT_BOTH(UNIT_PAIR, FamADKE_T);
UNIT_BOTH(UNIT_PAIR, FamGasWall_T);
template <class T> using FamEDACInt_T = FamEDAC_T<T, true>;
template <class T> using FamEDACExt_T = FamEDAC_T<T, false>;
UNIT_BOTH(UNIT_PAIR, FamEDACInt_T);
UNIT_BOTH(UNIT_PAIR, FamEDACExt_T);
UNIT_BOTH(UNIT_PAIR, FamVGrad_T);
UNIT_BOTH(UNIT_PAIR, FamElastic_T);
UNIT_BOTH(UNIT_PAIR, FamDSPre_T);
typedef FamWCSPHX_T<double, false> UnitX_d; typedef FamWCSPHX_T<double, true> UnitXD_d;
typedef FamWCSPHX_T<float, false> UnitX_f; typedef FamWCSPHX_T<float, true> UnitXD_f;
UNIT_PAIR(UnitX_d); UNIT_PAIR(UnitXD_d); UNIT_PAIR(UnitX_f); UNIT_PAIR(UnitXD_f);
#define UNIT_FUSED_UH(F) UNIT_FUSED(F, true)
#define UNIT_FUSED_VH(F) UNIT_FUSED(F, false)
typedef FamWCSPHE_T<double, false> UnitE_d; typedef FamWCSPHE_T<double, true> UnitEU_d;
typedef FamWCSPHE_T<float, false> UnitE_f; typedef FamWCSPHE_T<float, true> UnitEU_f;
typedef FamWCSPHEG_T<double, false> UnitEG_d; typedef FamWCSPHEG_T<double, true> UnitEGU_d;
typedef FamWCSPHEG_T<float, false> UnitEG_f; typedef FamWCSPHEG_T<float, true> UnitEGU_f;
UNIT_FUSED_UH(UnitE_d); UNIT_FUSED_UH(UnitEU_d); UNIT_FUSED_UH(UnitE_f); UNIT_FUSED_UH(UnitEU_f);
UNIT_FUSED_UH(UnitEG_d); UNIT_FUSED_UH(UnitEGU_d); UNIT_FUSED_UH(UnitEG_f); UNIT_FUSED_UH(UnitEGU_f);
UNIT_BOTH(UNIT_FUSED_VH, FamWCSPHV_T);
UNIT_BOTH(UNIT_FUSED_UH, FamTVFE_T);
UNIT_BOTH(UNIT_FUSED_UH, FamElasticU_T);
UNIT_BOTH(UNIT_MERGED, FamWCSPHM_T);
UNIT_BOTH(UNIT_MERGED, FamWCSPHMV_T);
UNIT_INTERP(FamInterpSum); UNIT_INTERP(FamInterpMom); UNIT_INTERP(FamInterpRhs);
#endif
