// sph_fam_elastic.h -- equation families of the pair loop: velocity gradient and the elastic rates.  Part of the
// sph_eval.hip translation units (included there, after sph_fam_wcsph.h).

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
    static constexpr int NR_U = 20; // values per record (doubles, or floats with arith_f32)
    static_assert(PIECES * (16 / (int)sizeof(T)) == NR_U, "decode reads PIECES 16-B pieces of NR_U values");
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
