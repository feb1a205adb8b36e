// sph_integrate.hip -- integrator stage sweeps on the device.
//
// Replaces the per-particle loops the reference generates from
// pysph/sph/integrator_cython.mako:87-113 around the IntegratorStep methods of
// pysph/sph/integrator_step.py (WCSPHStep :38-93, TransportVelocityStep
// :257-299).  Real particles only, as in the template (:103-104).  Purely
// streaming (HBM-bound): ~112 B (initialize) / ~168 B (stage) per particle.
#include "sph_internal.h"

struct StageArgs {
    int stepper, stage;
    double dt;
    size_t n;
    int ip0, iap; // EDAC steppers: the user properties p0 and ap
    int gd[10];   // GasDFluidStep: h0 ah converged omega alpha1 alpha2 alpha10 alpha20 aalpha1 aalpha2
    double *p[SPH_PROP_COUNT];
};

__global__ __launch_bounds__(256) void k_stage(StageArgs a)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    double **p = a.p;
    const double dt = a.dt, dtb2 = 0.5 * a.dt;
    if (a.stepper == SPH_STEP_WCSPH) {
        if (a.stage == 0) { // integrator_step.py:51-61
            p[SPH_X0][i] = p[SPH_X][i]; p[SPH_Y0][i] = p[SPH_Y][i]; p[SPH_Z0][i] = p[SPH_Z][i];
            p[SPH_U0][i] = p[SPH_U][i]; p[SPH_V0][i] = p[SPH_V][i]; p[SPH_W0][i] = p[SPH_W][i];
            p[SPH_RHO0][i] = p[SPH_RHO][i];
        } else { // stage1 :63-76 (dt/2), stage2 :78-92 (dt)
            const double f = a.stage == 1 ? dtb2 : dt;
            p[SPH_U][i] = p[SPH_U0][i] + f * p[SPH_AU][i];
            p[SPH_V][i] = p[SPH_V0][i] + f * p[SPH_AV][i];
            p[SPH_W][i] = p[SPH_W0][i] + f * p[SPH_AW][i];
            p[SPH_X][i] = p[SPH_X0][i] + f * p[SPH_AX][i];
            p[SPH_Y][i] = p[SPH_Y0][i] + f * p[SPH_AY][i];
            p[SPH_Z][i] = p[SPH_Z0][i] + f * p[SPH_AZ][i];
            p[SPH_RHO][i] = p[SPH_RHO0][i] + f * p[SPH_ARHO][i];
        }
    } else if (a.stepper == SPH_STEP_SOLID_MECH) { // integrator_step.py:175-255
        constexpr int q[]  = {SPH_X, SPH_Y, SPH_Z, SPH_U, SPH_V, SPH_W, SPH_RHO, SPH_E,
                                 SPH_S00, SPH_S01, SPH_S02, SPH_S11, SPH_S12, SPH_S22};
        constexpr int q0[] = {SPH_X0, SPH_Y0, SPH_Z0, SPH_U0, SPH_V0, SPH_W0, SPH_RHO0, SPH_E0,
                                 SPH_S000, SPH_S010, SPH_S020, SPH_S110, SPH_S120, SPH_S220};
        constexpr int aq[] = {SPH_AX, SPH_AY, SPH_AZ, SPH_AU, SPH_AV, SPH_AW, SPH_ARHO, SPH_AE,
                                 SPH_AS00, SPH_AS01, SPH_AS02, SPH_AS11, SPH_AS12, SPH_AS22};
        if (a.stage == 0) {
#pragma unroll
            for (int k = 0; k < 14; k++) p[q0[k]][i] = p[q[k]][i];
        } else {
            const double f = a.stage == 1 ? dtb2 : dt;
#pragma unroll
            for (int k = 0; k < 14; k++) p[q[k]][i] = p[q0[k]][i] + f * p[aq[k]][i];
        }
    } else if (a.stepper == SPH_STEP_TVF) {
        if (a.stage == 1) { // :268-285
            double u = p[SPH_U][i] + dtb2 * p[SPH_AU][i];
            double v = p[SPH_V][i] + dtb2 * p[SPH_AV][i];
            double w = p[SPH_W][i] + dtb2 * p[SPH_AW][i];
            p[SPH_U][i] = u; p[SPH_V][i] = v; p[SPH_W][i] = w;
            double uh = u + dtb2 * p[SPH_AUHAT][i];
            double vh = v + dtb2 * p[SPH_AVHAT][i];
            double wh = w + dtb2 * p[SPH_AWHAT][i];
            p[SPH_UHAT][i] = uh; p[SPH_VHAT][i] = vh; p[SPH_WHAT][i] = wh;
            p[SPH_X][i] += dt * uh;
            p[SPH_Y][i] += dt * vh;
            p[SPH_Z][i] += dt * wh;
        } else if (a.stage == 2) { // :287-299
            double u = p[SPH_U][i] + dtb2 * p[SPH_AU][i];
            double v = p[SPH_V][i] + dtb2 * p[SPH_AV][i];
            double w = p[SPH_W][i] + dtb2 * p[SPH_AW][i];
            p[SPH_U][i] = u; p[SPH_V][i] = v; p[SPH_W][i] = w;
            p[SPH_VMAG2][i] = u * u + v * v + w * w;
        }
    } else if (a.stepper == SPH_STEP_EDAC || a.stepper == SPH_STEP_EDAC_TVF) {
        if (a.stage == 0) { // wc/edac.py:95-105, :493-503
            p[SPH_X0][i] = p[SPH_X][i]; p[SPH_Y0][i] = p[SPH_Y][i]; p[SPH_Z0][i] = p[SPH_Z][i];
            p[SPH_U0][i] = p[SPH_U][i]; p[SPH_V0][i] = p[SPH_V][i]; p[SPH_W0][i] = p[SPH_W][i];
            p[a.ip0][i] = p[SPH_P][i];
        } else { // stage1 (dt/2), stage2 (dt)
            const double f = a.stage == 1 ? dtb2 : dt;
            const double u = p[SPH_U0][i] + f * p[SPH_AU][i];
            const double v = p[SPH_V0][i] + f * p[SPH_AV][i];
            const double w = p[SPH_W0][i] + f * p[SPH_AW][i];
            p[SPH_U][i] = u; p[SPH_V][i] = v; p[SPH_W][i] = w;
            if (a.stepper == SPH_STEP_EDAC) { // :107-133: positions move with ax (u + the XSPH correction)
                p[SPH_X][i] = p[SPH_X0][i] + f * p[SPH_AX][i];
                p[SPH_Y][i] = p[SPH_Y0][i] + f * p[SPH_AY][i];
                p[SPH_Z][i] = p[SPH_Z0][i] + f * p[SPH_AZ][i];
            } else { // :505-540: with the transport velocity
                const double uh = u + f * p[SPH_AUHAT][i];
                const double vh = v + f * p[SPH_AVHAT][i];
                const double wh = w + f * p[SPH_AWHAT][i];
                p[SPH_UHAT][i] = uh; p[SPH_VHAT][i] = vh; p[SPH_WHAT][i] = wh;
                p[SPH_X][i] = p[SPH_X0][i] + f * uh;
                p[SPH_Y][i] = p[SPH_Y0][i] + f * vh;
                p[SPH_Z][i] = p[SPH_Z0][i] + f * wh;
            }
            p[SPH_P][i] = p[a.ip0][i] + f * p[a.iap][i];
        }
    } else if (a.stepper == SPH_STEP_GASD) {
        enum { H0, AH, CONV, OMEGA, AL1, AL2, AL10, AL20, AAL1, AAL2 };
        const int *g = a.gd;
        if (a.stage == 0) { // integrator_step.py:353-378
            p[SPH_X0][i] = p[SPH_X][i]; p[SPH_Y0][i] = p[SPH_Y][i]; p[SPH_Z0][i] = p[SPH_Z][i];
            p[SPH_U0][i] = p[SPH_U][i]; p[SPH_V0][i] = p[SPH_V][i]; p[SPH_W0][i] = p[SPH_W][i];
            p[SPH_E0][i] = p[SPH_E][i];
            p[g[H0]][i] = p[SPH_H][i];
            p[SPH_RHO0][i] = p[SPH_RHO][i];
            p[g[CONV]][i] = 0.0;  // no particle has converged at the beginning of an evaluation
            p[g[OMEGA]][i] = 1.0; // the grad-h factor until the density iteration sets it
            p[g[AL10]][i] = p[g[AL1]][i];
            p[g[AL20]][i] = p[g[AL2]][i];
        } else { // stage1 :380-407 (dt/2), stage2 :409-428 (dt)
            const double f = a.stage == 1 ? dtb2 : dt;
            const double u = p[SPH_U0][i] + f * p[SPH_AU][i];
            const double v = p[SPH_V0][i] + f * p[SPH_AV][i];
            const double w = p[SPH_W0][i] + f * p[SPH_AW][i];
            p[SPH_U][i] = u; p[SPH_V][i] = v; p[SPH_W][i] = w;
            p[SPH_X][i] = p[SPH_X0][i] + f * u;
            p[SPH_Y][i] = p[SPH_Y0][i] + f * v;
            p[SPH_Z][i] = p[SPH_Z0][i] + f * w;
            p[SPH_E][i] = p[SPH_E0][i] + f * p[SPH_AE][i];
            if (a.stage == 1) { // h and rho are predicted for a faster convergence of the next density iteration
                p[SPH_H][i] = p[g[H0]][i] + f * p[g[AH]][i];
                p[SPH_RHO][i] = p[SPH_RHO0][i] + f * p[SPH_ARHO][i];
            }
            p[g[AL1]][i] = p[g[AL10]][i] + f * p[g[AAL1]][i];
            p[g[AL2]][i] = p[g[AL20]][i] + f * p[g[AAL2]][i];
        }
    } else if (a.stepper == SPH_STEP_GSPH) {
        if (a.stage == 1) { // integrator_step.py:433-449: one stage; the energy moves with the half-step velocities
#pragma clang fp contract(off) // every product rounded on its own, as the reference's expressions are
            const double au = p[SPH_AU][i], av = p[SPH_AV][i], aw = p[SPH_AW][i];
            const double u = p[SPH_U][i], v = p[SPH_V][i], w = p[SPH_W][i];
            const double ustar = u + dtb2 * au, vstar = v + dtb2 * av, wstar = w + dtb2 * aw;
            p[SPH_U][i] = u + dt * au;
            p[SPH_V][i] = v + dt * av;
            p[SPH_W][i] = w + dt * aw;
            p[SPH_E][i] = p[SPH_E][i] + dt * (p[SPH_AE][i] - ustar * au - vstar * av - wstar * aw);
            p[SPH_X][i] = p[SPH_X][i] + dt * ustar;
            p[SPH_Y][i] = p[SPH_Y][i] + dt * vstar;
            p[SPH_Z][i] = p[SPH_Z][i] + dt * wstar;
        }
    } else if (a.stepper == SPH_STEP_ADKE) {
        if (a.stage == 0) { // integrator_step.py:454-467
            p[SPH_X0][i] = p[SPH_X][i]; p[SPH_Y0][i] = p[SPH_Y][i]; p[SPH_Z0][i] = p[SPH_Z][i];
            p[SPH_U0][i] = p[SPH_U][i]; p[SPH_V0][i] = p[SPH_V][i]; p[SPH_W0][i] = p[SPH_W][i];
            p[SPH_E0][i] = p[SPH_E][i];
            p[SPH_RHO0][i] = p[SPH_RHO][i];
        } else { // stage1 :470-484 (dt/2), stage2 :486-499 (dt): the positions move with the NEW velocities
#pragma clang fp contract(off) // every product rounded on its own, as the reference's expressions are
            const double f = a.stage == 1 ? dtb2 : dt;
            const double u = p[SPH_U0][i] + f * p[SPH_AU][i];
            const double v = p[SPH_V0][i] + f * p[SPH_AV][i];
            const double w = p[SPH_W0][i] + f * p[SPH_AW][i];
            p[SPH_U][i] = u; p[SPH_V][i] = v; p[SPH_W][i] = w;
            p[SPH_X][i] = p[SPH_X0][i] + f * u;
            p[SPH_Y][i] = p[SPH_Y0][i] + f * v;
            p[SPH_Z][i] = p[SPH_Z0][i] + f * w;
            p[SPH_E][i] = p[SPH_E0][i] + f * p[SPH_AE][i];
        }
    }
}

extern "C" int sph_integrate_stage(sph_ctx *c, int id, int stepper, int stage, double dt)
{
    if (!c || id < 0 || id >= SPH_MAX_ARRAYS || stage < 0 || stage > 2) { sph_set_error("sph_integrate_stage: bad arguments"); return SPH_ERR_ARG; }
    HIP_TRY(hipSetDevice(c->device));
    if (stepper == SPH_STEP_RIGID_RK2 || stepper == SPH_STEP_RIGID_EULER) return sph_rigid_stage(c, id, stepper, stage, dt); // sph_rigid.hip
    DevArray &A = c->arr[id];
    static const int wc0[] = {SPH_X, SPH_Y, SPH_Z, SPH_U, SPH_V, SPH_W, SPH_RHO, SPH_X0, SPH_Y0, SPH_Z0, SPH_U0, SPH_V0, SPH_W0, SPH_RHO0, -1};
    static const int wc1[] = {SPH_X, SPH_Y, SPH_Z, SPH_U, SPH_V, SPH_W, SPH_RHO, SPH_X0, SPH_Y0, SPH_Z0, SPH_U0, SPH_V0, SPH_W0, SPH_RHO0,
                              SPH_AU, SPH_AV, SPH_AW, SPH_AX, SPH_AY, SPH_AZ, SPH_ARHO, -1};
    static const int tv1[] = {SPH_X, SPH_Y, SPH_Z, SPH_U, SPH_V, SPH_W, SPH_AU, SPH_AV, SPH_AW, SPH_UHAT, SPH_VHAT, SPH_WHAT,
                              SPH_AUHAT, SPH_AVHAT, SPH_AWHAT, -1};
    static const int tv2[] = {SPH_U, SPH_V, SPH_W, SPH_AU, SPH_AV, SPH_AW, SPH_VMAG2, -1};
    static const int sm0[] = {SPH_X, SPH_Y, SPH_Z, SPH_U, SPH_V, SPH_W, SPH_RHO, SPH_E, SPH_S00, SPH_S01, SPH_S02, SPH_S11, SPH_S12, SPH_S22,
                              SPH_X0, SPH_Y0, SPH_Z0, SPH_U0, SPH_V0, SPH_W0, SPH_RHO0, SPH_E0, SPH_S000, SPH_S010, SPH_S020, SPH_S110,
                              SPH_S120, SPH_S220, -1};
    static const int sm1[] = {SPH_X, SPH_Y, SPH_Z, SPH_U, SPH_V, SPH_W, SPH_RHO, SPH_E, SPH_S00, SPH_S01, SPH_S02, SPH_S11, SPH_S12, SPH_S22,
                              SPH_X0, SPH_Y0, SPH_Z0, SPH_U0, SPH_V0, SPH_W0, SPH_RHO0, SPH_E0, SPH_S000, SPH_S010, SPH_S020, SPH_S110,
                              SPH_S120, SPH_S220, SPH_AX, SPH_AY, SPH_AZ, SPH_AU, SPH_AV, SPH_AW, SPH_ARHO, SPH_AE, SPH_AS00, SPH_AS01,
                              SPH_AS02, SPH_AS11, SPH_AS12, SPH_AS22, -1};
    const int ip0 = sph_prop_register("p0"), iap = sph_prop_register("ap");
    if (ip0 < 0 || iap < 0) return SPH_ERR_ARG;
    const int ed0[] = {SPH_X, SPH_Y, SPH_Z, SPH_U, SPH_V, SPH_W, SPH_P, SPH_X0, SPH_Y0, SPH_Z0, SPH_U0, SPH_V0, SPH_W0, ip0, -1};
    const int ed1[] = {SPH_X, SPH_Y, SPH_Z, SPH_U, SPH_V, SPH_W, SPH_P, SPH_X0, SPH_Y0, SPH_Z0, SPH_U0, SPH_V0, SPH_W0, ip0,
                       SPH_AU, SPH_AV, SPH_AW, SPH_AX, SPH_AY, SPH_AZ, iap, -1};
    const int et1[] = {SPH_X, SPH_Y, SPH_Z, SPH_U, SPH_V, SPH_W, SPH_P, SPH_X0, SPH_Y0, SPH_Z0, SPH_U0, SPH_V0, SPH_W0, ip0,
                       SPH_AU, SPH_AV, SPH_AW, SPH_UHAT, SPH_VHAT, SPH_WHAT, SPH_AUHAT, SPH_AVHAT, SPH_AWHAT, iap, -1};
    int gd[10] = {}, gd0[32], gd1[40];
    if (stepper == SPH_STEP_GASD) {
        const char *names[10] = {"h0", "ah", "converged", "omega", "alpha1", "alpha2", "alpha10", "alpha20", "aalpha1", "aalpha2"};
        for (int k = 0; k < 10; k++) { gd[k] = sph_prop_register(names[k]); if (gd[k] < 0) return SPH_ERR_ARG; }
        const int b0[] = {SPH_X, SPH_Y, SPH_Z, SPH_U, SPH_V, SPH_W, SPH_E, SPH_H, SPH_RHO, SPH_X0, SPH_Y0, SPH_Z0, SPH_U0, SPH_V0, SPH_W0,
                          SPH_E0, SPH_RHO0, gd[0], gd[2], gd[3], gd[4], gd[5], gd[6], gd[7], -1};
        const int b1[] = {SPH_X, SPH_Y, SPH_Z, SPH_U, SPH_V, SPH_W, SPH_E, SPH_H, SPH_RHO, SPH_X0, SPH_Y0, SPH_Z0, SPH_U0, SPH_V0, SPH_W0,
                          SPH_E0, SPH_RHO0, SPH_AU, SPH_AV, SPH_AW, SPH_AE, SPH_ARHO, gd[0], gd[1], gd[4], gd[5], gd[6], gd[7], gd[8], gd[9], -1};
        memcpy(gd0, b0, sizeof b0);
        memcpy(gd1, b1, sizeof b1);
    }
    static const int gs1[] = {SPH_X, SPH_Y, SPH_Z, SPH_U, SPH_V, SPH_W, SPH_E, SPH_AU, SPH_AV, SPH_AW, SPH_AE, -1};
    static const int ad0[] = {SPH_X, SPH_Y, SPH_Z, SPH_U, SPH_V, SPH_W, SPH_E, SPH_RHO, SPH_X0, SPH_Y0, SPH_Z0, SPH_U0, SPH_V0, SPH_W0,
                              SPH_E0, SPH_RHO0, -1};
    static const int ad1[] = {SPH_X, SPH_Y, SPH_Z, SPH_U, SPH_V, SPH_W, SPH_E, SPH_X0, SPH_Y0, SPH_Z0, SPH_U0, SPH_V0, SPH_W0, SPH_E0,
                              SPH_AU, SPH_AV, SPH_AW, SPH_AE, -1};
    const int *need = nullptr;
    if (stepper == SPH_STEP_GASD) need = stage == 0 ? gd0 : gd1;
    else if (stepper == SPH_STEP_GSPH) { if (stage != 1) return SPH_OK; need = gs1; }
    else if (stepper == SPH_STEP_ADKE) need = stage == 0 ? ad0 : ad1;
    else if (stepper == SPH_STEP_EDAC) need = stage == 0 ? ed0 : ed1;
    else if (stepper == SPH_STEP_EDAC_TVF) need = stage == 0 ? ed0 : et1;
    else if (stepper == SPH_STEP_WCSPH) need = stage == 0 ? wc0 : wc1;
    else if (stepper == SPH_STEP_SOLID_MECH) need = stage == 0 ? sm0 : sm1;
    else if (stepper == SPH_STEP_TVF) { if (stage == 0) return SPH_OK; need = stage == 1 ? tv1 : tv2; }
    else { sph_set_error("sph_integrate_stage: unknown stepper %d", stepper); return SPH_ERR_UNSUPPORTED; }
    for (const int *q = need; *q >= 0; q++) SPH_TRY(sph_array_ensure_prop(c, id, *q));
    if (A.n_real == 0) return SPH_OK;
    StageArgs a;
    a.stepper = stepper; a.stage = stage; a.dt = dt; a.n = A.n_real; a.ip0 = ip0; a.iap = iap;
    for (int k = 0; k < 10; k++) a.gd[k] = gd[k];
    for (int k = 0; k < SPH_PROP_COUNT; k++) a.p[k] = A.prop[k];
    ScopedTimer tm(c, T_STAGE);
    hipLaunchKernelGGL(k_stage, dim3(div_up(A.n_real, 256)), dim3(256), 0, c->stream, a);
    if (stepper == SPH_STEP_TVF ? stage == 1 : stage > 0) c->nnps_valid = false; // positions moved
    if (stepper == SPH_STEP_GASD && stage == 1) { sph_mark_written(A, SPH_H); c->uniform_h = false; } // h predicted: the next neighbour update looks at it
    return SPH_OK;
}
