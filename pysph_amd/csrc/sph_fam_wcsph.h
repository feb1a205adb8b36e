// sph_fam_wcsph.h -- equation families of the pair loop: WCSPH (with its EOS-fused, variable-h and merged-order forms),
// the WCSPHScheme options, the delta-SPH pre-passes, the density summations and the neighbour lists, each with the
// load_record that reads its compact records.  Part of the sph_eval.hip translation units (included there).

// flag bits of the families (eq_family in sph_eval.hip assigns them); shared with sph_fam_tvf.h and sph_fam_elastic.h
enum { F_VG2 = 1, F_VG3 = 2,                                            // velocity gradient
       F_ECONT = 1, F_ESTRESS = 2, F_EAV = 4, F_EXSPH = 8 };            // elastic rates
enum { F_DCONT = 16, F_DMOM = 32, F_LAM = 64, F_LAMD = 128,             // WCSPH options (next to the WCSPH flags below)
       F_MOMENT = 1, F_GRADRHO = 2, F_GCORR = 4 };                      // delta-SPH pre-passes
enum { F_CONT = 1, F_MOM = 2, F_XSPH = 4, F_TENSILE = 8,               // WCSPH
       F_SD = 1, F_TVFSD = 2,                                           // density
       F_TP = 1, F_TVISC = 2, F_TAV = 4, F_TAS = 8 };                   // TVF force

template <class T> struct FamWCSPH_T {
    typedef T Real; // arithmetic type of the pair loop
    static constexpr uint32_t CF0 = F_CONT | F_MOM | F_XSPH; // flag set compiled as a constant (variant 6)
#ifndef SPH_WCSPH_MINB
#define SPH_WCSPH_MINB 4
#endif
    static constexpr int MINB = SPH_WCSPH_MINB; // wavefronts per SIMD the pair kernel is compiled for (VGPR budget)
    static constexpr int NA = 8; // u v w m rho tmpj(=p/rho^2) cs p
    static constexpr int NR = 12; // x y z h + NA (128-B padded records measured slower: larger L2 footprint)
    static constexpr int NR_COMPACT = 10; // uniform h, no tensile correction: the records end before [h p] (load_record_wcsph)
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
    static constexpr int NR_COMPACT = 4; // uniform h: [x y z m] (load_record<FamDensity, true>)
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
    static constexpr int NR_COMPACT = 4; // (load_record<FamNbr, true>)
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
