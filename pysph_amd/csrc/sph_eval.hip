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
// equation families, then the packer of their records (it names the record sizes the families' loaders export)
// ---------------------------------------------------------------------------
#include "sph_fam_wcsph.h"
#include "sph_fam_tvf.h"
#include "sph_fam_gas.h"
#include "sph_fam_elastic.h"
#include "sph_pack.h"

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
              FAM_GSPHGRAD, FAM_GSPH, FAM_ADKESD, FAM_ADKE, FAM_GASWALL, FAM_COUNT };

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

#include "sph_pack_plan.h" // PackPlan .. pack_array, pack_generic

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
    if (uh) rl.pl.nr = FamNbr::NR_COMPACT;
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
        pl.na = FamWCSPHX_T<double, true>::NA; pl.nr = FamWCSPHX_T<double, true>::NR;
    }
    // compact 80-B WCSPH records when neither h nor p of a neighbour is read
    if (wave && fam == FAM_WCSPH && uh && !(dflags & F_TENSILE)) pl.nr = c->wcsph_nr ? (int)c->wcsph_nr : FamWCSPH::NR_COMPACT;
    if (wave && fam == FAM_DENSITY && uh) pl.nr = FamDensity::NR_COMPACT;
    if (wave && fam == FAM_TVF && uh) pl.nr = (dflags & F_TAV) ? FamTVF::NR_COMPACT_M : FamTVF::NR_COMPACT;
    if (wave && fam == FAM_EDAC && uh) pl.nr = FamEDAC_T<double, true>::NR_COMPACT; // (m always: load_record_edac)
    if (wave && (rl.record_f32 || rl.arith_f32)) pl.nr = (4 + pl.na + 3) & ~3; // floats
    // The caller promised (sph_group.src_eos) that p, cs of every array read here are the Tait EOS of its
    // rho: with gamma = 7 (powers by multiplication), uniform h and no tensile correction the pair kernel
    // recomputes them and the records shrink to 64 bytes (32 in fp32).
    const bool eosf = g->src_eos == 1 && c->eos_fuse && fam == FAM_WCSPH && wave && uh && !(dflags & F_TENSILE) &&
                      tait_gk(g->eos_par[2]) >= 0 && g->eos_par[0] > 0.0 && !rl.record_f32 && !c->wcsph_nr;
    if (eosf) pl.nr = FamWCSPHE_T<double>::NR; // doubles, or floats with arith_f32
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
    if (eosv) pl.nr = FamWCSPHV_T<double>::NR;
    // TVF force pass after StateEquation + density summation (sph_group.src_eos = 2): p and V leave the records
    // when every array read here has ONE mass (V = rho / m)
    bool tvff = g->src_eos == 2 && c->eos_fuse && c->mass_fuse && fam == FAM_TVF && wave && uh && !rl.record_f32 &&
                g->eos_par[1] != 0.0; // (the artificial viscosity's m_j is the source's one mass)
    if (tvff) c->want_mrange = true;
    for (int j = 0; j < nsrcs && tvff; j++) tvff = c->arr[P.srcs[j]].m_known;
    if (tvff && !P.dest_is_src) tvff = D.m_known;
    if (tvff) pl.nr = !(dflags & F_TAS) ? FamTVFE_T<double>::NR_FUSED : rl.arith_f32 ? FamTVFE_T<float>::NR_FUSED_AS : FamTVFE_T<double>::NR_FUSED_AS;
    // elastic rates: uniform h and ONE mass per source array -> neither travels in the records
    bool elu = fam == FAM_ELASTIC && c->mass_fuse && wave && uh && !rl.record_f32;
    if (elu) c->want_mrange = true;
    for (int j = 0; j < nsrcs && elu; j++) elu = c->arr[P.srcs[j]].m_known;
    if (elu) pl.nr = FamElasticU_T<double>::NR_U; // doubles, or floats with arith_f32
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
            const int layout = rf32 ? PL_F32 : (compact ? PL_GEN_UH : PL_PLAIN);
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
