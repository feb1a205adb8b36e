// sph_fam_gas.h -- equation families of the pair loop: gas dynamics (summation density, MPM, ADKE, walls) and Godunov
// SPH with its Riemann solvers and limiters.  Part of the sph_eval.hip translation units (included there).

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
// read through eij . G . eij only, so its six symmetric sums are formed once at packing (k_pack, PD_GSPH_SYM).
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
