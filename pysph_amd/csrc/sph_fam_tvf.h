// sph_fam_tvf.h -- equation families of the pair loop: TVF force (and its state-fused form), EDAC force, average
// pressure.  Part of the sph_eval.hip translation units (included there, after sph_fam_wcsph.h).

// ---- TVF momentum terms (transport_velocity.py:219-545) -------------------
template <class T> struct FamTVF_T {
    typedef T Real; // arithmetic type of the pair loop
    static constexpr bool PRED = true; // see FamWCSPH
    static constexpr uint32_t CF0 = F_TP | F_TVISC | F_TAS; // flag set compiled as a constant (variant 6)
    static constexpr int MINB = 4; // wavefronts per SIMD the pair kernel is compiled for (VGPR budget; fp64: 125-129 registers)
    static constexpr int NA = 12; // u v w uhat vhat what rho p V m Vj2 pad
    static constexpr int NR = 16; // x y z h + NA
    static constexpr int NR_COMPACT = 12, NR_COMPACT_M = 14; // uniform h: six 16-B pieces, seven with the mass of the artificial viscosity (load_record<FamTVF, true>)
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

// TVF records of the aggregated kernel under uniform h (k_pack, PL_TVF):
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
    // values per record as load_fused reads them: without / with the piece(s) of the artificial stress
    static constexpr int NR_FUSED = 8, NR_FUSED_AS = sizeof(T) == 8 ? 10 : 12;
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
//      compact layout PL_TVF in its seven-piece form, which carries m (load_record_edac below).  p is integrated state
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
    static constexpr int NR_COMPACT = FamTVF_T<T>::NR_COMPACT_M; // uniform h: TVF's seven-piece form, m always (load_record_edac)
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

// EDAC records of the aggregated kernel under uniform h: k_pack, PL_TVF in its seven-piece form
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
