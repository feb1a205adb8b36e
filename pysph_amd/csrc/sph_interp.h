// sph_interp.h -- particle fields onto interpolation points (pysph/tools/interpolator.py:18-172) on the pair-loop
// skeleton of sph_pair.h.  Included at the end of sph_eval.hip: it uses that file's record packer and launch helpers.
//
// The destination is the array of interpolation points, the sources are particle arrays; fp64 only.
//   FamInterpSum   the four summation methods (InterpolateFunction :18-29, InterpolateSPH :32-37,
//                  SPLASHInterpolateProperty :40-45, SPLASHInterpolatePropertyNormalized :48-61): INTERP_W properties
//                  per sweep over records [x y z h | v f_1..f_W], v = m / rho
//   FamInterpMom   the moment matrix of the first-order method (SPHFirstOrderApproximationPreStep :64-103)
//                  over records [x y z h | v -]
//   FamInterpRhs   its right-hand sides for INTERP_W properties and the solve (SPHFirstOrderApproximation :106-172)
//                  over the records of FamInterpSum
#pragma once

#define INTERP_W 4 // properties per sweep

// equation flags of FamInterpSum: the weight is WIJ (h_ij = (h_i + h_j) / 2) unless one of the first two is set
enum { F_IW_DEST = 1,  // WI: the kernel with the destination's h
       F_IW_SRC = 2,   // WJ: ... with the source's h
       F_IVOL = 4,     // v = m / rho multiplies the weight
       F_INORM = 8 };  // finish divides by the accumulated weights when they exceed 1e-12

// the pair geometry with the smoothing length the flags ask for: WI / WJ are WIJ of a pair whose two h are the same
template <int KK, bool UH, class A>
__device__ __forceinline__ void interp_geom(PairGeom &g, const double4 &pi, const double4 &pj, double r2, uint32_t fl, const A &a)
{
    if (UH) { pair_geom<KK, UH>(g, pi, pj, r2, a); return; }
    double4 qi = pi, qj = pj;
    if (fl & F_IW_DEST) qj.w = pi.w;
    if (fl & F_IW_SRC) qi.w = pj.w;
    pair_geom<KK, UH>(g, qi, qj, r2, a);
}

struct FamInterpSum {
    typedef double Real;
    static constexpr bool PRED = true; // see FamWCSPH
    static constexpr uint32_t CF0 = F_INORM; // shepard
    static constexpr int MINB = 4;
    static constexpr int NA = 1 + INTERP_W; // v f_1..f_W
    static constexpr int NR = 4 + NA + 1;   // x y z h | v f_1..f_W | pad
    struct Params { double *out[INTERP_W]; }; // per property, indexed by the destination's original index (null: slot not in use)
    struct Dest { double den, P[INTERP_W]; };
    template <class A> static __device__ __forceinline__ void load(Dest &D, const double *, const A &, uint32_t)
    {
        D.den = 0.0;
#pragma unroll
        for (int k = 0; k < INTERP_W; k++) D.P[k] = 0.0;
    }
    template <int KK, bool UH, class A>
    static __device__ __forceinline__ void pair(Dest &D, const double4 &pi, const double4 &pj, double r2,
                                                const double (&s)[NA], uint32_t fl, const A &a, bool pass = true)
    {
        PairGeom g;
        interp_geom<KK, UH>(g, pi, pj, r2, fl, a);
        double w = pair_w<KK, UH>(g);
        // PRED: a pair outside the criterion adds exactly zero -- its record's values are not looked at (they may be
        // inf or NaN: m / rho of a particle with rho = 0 just outside the support)
        w = pass ? w : 0.0;
        if (fl & F_IVOL) w *= pass ? s[0] : 0.0;
        D.den += w;
#pragma unroll
        for (int k = 0; k < INTERP_W; k++) D.P[k] += w * (pass ? s[1 + k] : 0.0);
    }
    template <class A> static __device__ __forceinline__ void finish(Dest &D, const A &a, uint32_t o)
    {
        const bool norm = (a.dflags & F_INORM) && D.den > 1e-12;
#pragma unroll
        for (int k = 0; k < INTERP_W; k++)
            if (a.p.out[k]) a.p.out[k][o] = norm ? D.P[k] / D.den : D.P[k];
    }
};

// ---- first order (Liu & Liu 2006): 16 accumulators, one Dest layout for both passes
struct InterpDest16 { double A[16]; };

struct FamInterpMom {
    typedef double Real;
    static constexpr bool PRED = true;
    static constexpr uint32_t CF0 = 1u;
    static constexpr int MINB = 2;
    static constexpr int NA = 1; // v
    static constexpr int NR = 6; // x y z h | v pad
    struct Params { double *mom; }; // [16 * original index + 4 * row + column]
    typedef InterpDest16 Dest;
    template <class A> static __device__ __forceinline__ void load(Dest &D, const double *, const A &, uint32_t)
    {
#pragma unroll
        for (int k = 0; k < 16; k++) D.A[k] = 0.0;
    }
    template <int KK, bool UH, class A>
    static __device__ __forceinline__ void pair(Dest &D, const double4 &pi, const double4 &pj, double r2,
                                                const double (&s)[NA], uint32_t fl, const A &a, bool pass = true)
    {
        PairGeom g;
        pair_geom<KK, UH>(g, pi, pj, r2, a);
        const double V = pass ? s[0] : 0.0;
        const double wv = pair_w<KK, UH>(g) * V;
        const double gv = pair_gradfac<KK, UH>(g) * V; // DWIJ[b] V = gv XIJ[b]
        D.A[0] += wv;
#pragma unroll
        for (int c = 0; c < 3; c++) D.A[1 + c] += -g.xij[c] * wv;
#pragma unroll
        for (int b = 0; b < 3; b++) {
            const double dv = gv * g.xij[b];
            D.A[4 + 4 * b] += dv;
#pragma unroll
            for (int c = 0; c < 3; c++) D.A[5 + 4 * b + c] += -g.xij[c] * dv;
        }
    }
    template <class A> static __device__ __forceinline__ void finish(Dest &D, const A &a, uint32_t o)
    {
        double2 *const m = reinterpret_cast<double2 *>(a.p.mom + 16ull * o);
#pragma unroll
        for (int k = 0; k < 8; k++) m[k] = make_double2(D.A[2 * k], D.A[2 * k + 1]);
    }
};

// Gauss-Jordan elimination WITHOUT row exchange of the leading N x N system for INTERP_W right-hand sides at once
// (gj_solve, pysph/sph/wc/linalg.py:94-166: its pivot search swaps an entry with itself).  B[4 k + r]: row r of
// right-hand side k; on return the solutions, or zeros when a pivot is smaller than 1e-12 in magnitude.
template <int N> __device__ __forceinline__ void interp_solve(const double (&M)[16], double (&B)[16])
{
    constexpr int NC = N + INTERP_W;
    double m[N][NC];
#pragma unroll
    for (int r = 0; r < N; r++) {
#pragma unroll
        for (int c = 0; c < N; c++) m[r][c] = M[4 * r + c];
#pragma unroll
        for (int k = 0; k < INTERP_W; k++) m[r][N + k] = B[4 * k + r];
    }
    bool ok = true;
#pragma unroll
    for (int col = 0; col < N; col++) {
        const double dnr = m[col][col];
        ok = ok && fabs(dnr) >= 1e-12;
#pragma unroll
        for (int rr = col + 1; rr < N; rr++) {
            const double cc = -m[rr][col] / dnr;
#pragma unroll
            for (int j = col + 1; j < NC; j++) m[rr][j] = m[rr][j] + cc * m[col][j];
        }
    }
#pragma unroll
    for (int rb = N - 1; rb >= 0; rb--) {
        const double piv = m[rb][rb];
#pragma unroll
        for (int j = rb + 1; j < NC; j++) m[rb][j] = m[rb][j] / piv;
#pragma unroll
        for (int kup = rb - 1; kup >= 0; kup--) {
            const double kk = -m[kup][rb];
#pragma unroll
            for (int j = rb + 1; j < NC; j++) m[kup][j] = m[kup][j] + kk * m[rb][j];
        }
    }
#pragma unroll
    for (int k = 0; k < INTERP_W; k++) {
#pragma unroll
        for (int r = 0; r < 4; r++) B[4 * k + r] = (ok && r < N) ? m[r < N ? r : 0][N + k] : 0.0;
    }
}

struct FamInterpRhs {
    typedef double Real;
    static constexpr bool PRED = true;
    static constexpr uint32_t CF0 = 1u;
    static constexpr int MINB = 2;
    static constexpr int NA = FamInterpSum::NA;
    static constexpr int NR = FamInterpSum::NR;
    struct Params { const double *mom; double *out[INTERP_W][4]; }; // value and gradient per property (null: slot not in use)
    typedef InterpDest16 Dest; // A[4 k + r]: row r of the right-hand side of property k
    template <class A> static __device__ __forceinline__ void load(Dest &D, const double *, const A &, uint32_t)
    {
#pragma unroll
        for (int k = 0; k < 16; k++) D.A[k] = 0.0;
    }
    template <int KK, bool UH, class A>
    static __device__ __forceinline__ void pair(Dest &D, const double4 &pi, const double4 &pj, double r2,
                                                const double (&s)[NA], uint32_t fl, const A &a, bool pass = true)
    {
        PairGeom g;
        pair_geom<KK, UH>(g, pi, pj, r2, a);
        const double V = pass ? s[0] : 0.0;
        const double wv = pair_w<KK, UH>(g) * V;
        const double gv = pair_gradfac<KK, UH>(g) * V;
        const double d0 = gv * g.xij[0], d1 = gv * g.xij[1], d2 = gv * g.xij[2];
#pragma unroll
        for (int k = 0; k < INTERP_W; k++) {
            const double f = pass ? s[1 + k] : 0.0;
            D.A[4 * k] += f * wv;
            D.A[4 * k + 1] += f * d0;
            D.A[4 * k + 2] += f * d1;
            D.A[4 * k + 3] += f * d2;
        }
    }
    template <class A> static __device__ __forceinline__ void finish(Dest &D, const A &a, uint32_t o)
    {
        double M[16];
        const double2 *const m = reinterpret_cast<const double2 *>(a.p.mom + 16ull * o);
#pragma unroll
        for (int k = 0; k < 8; k++) { const double2 v = m[k]; M[2 * k] = v.x; M[2 * k + 1] = v.y; }
        if (a.k.dim == 1) interp_solve<2>(M, D.A);
        else if (a.k.dim == 2) interp_solve<3>(M, D.A);
        else interp_solve<4>(M, D.A);
#pragma unroll
        for (int k = 0; k < INTERP_W; k++) {
#pragma unroll
            for (int r = 0; r < 4; r++)
                if (a.p.out[k][r]) a.p.out[k][r][o] = D.A[4 * k + r];
        }
    }
};

#if SPH_PRIMARY_UNIT   // the host side and its element-wise kernel: the primary compile of sph_eval.hip only
// m / rho per particle (original order): the v of the records
__global__ __launch_bounds__(256) void k_interp_vol(const double *__restrict__ m, const double *__restrict__ rho, double *__restrict__ out, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = m[i] / rho[i];
}

// records [x y z h | src[0..na-1] pad] of one array through its cell order (k_pack, PL_PLAIN); a null source is 0
static int interp_pack(sph_ctx *c, int id, size_t off, int na, const double *const *src, int nr)
{
    DevArray &A = c->arr[id];
    if (A.n == 0) return SPH_OK;
    PackArgs pa;
    memset(&pa, 0, sizeof pa);
    pa.perm = A.perm.as<uint32_t>();
    pa.n = A.n;
    pa.off = off;
    pa.x = A.prop[SPH_X]; pa.y = A.prop[SPH_Y]; pa.z = A.prop[SPH_Z]; pa.h = A.prop[SPH_H];
    pa.na = na;
    for (int k = 0; k < na; k++) pa.src[k] = src ? src[k] : nullptr;
    pa.posh = c->posh.as<double4>();
    pa.aux = c->aux.as<double>();
    pa.rec = c->posh.as<double>();
    pa.nr = nr;
    pa.layout = PL_PLAIN;
    pa.fpos = c->fposb.as<float4>();
    for (int k = 0; k < 3; k++) pa.gmin[k] = c->xmin[k];
    pa.radius_scale = c->radius_scale;
    pa.lds_np = pack_pieces(pa);
    launch_pack(c, pa, A.n);
    return SPH_OK;
}

// interp_launch: sph_eval.hip, with the other kernel-kind switches

extern "C" int sph_interpolate(sph_ctx *c, const sph_kernel *K, int method, int dest, int nsrc, const int *srcs,
                               int nprops, const int *props, const int *out_props, double *host_out, size_t n_pull)
{
    if (!c || !K || !srcs || !props || (!out_props && !host_out)) { sph_set_error("sph_interpolate: NULL argument"); return SPH_ERR_ARG; }
    if (method < SPH_INTERP_SHEPARD || method > SPH_INTERP_SPLASH_NORM) { sph_set_error("sph_interpolate: unknown method %d", method); return SPH_ERR_ARG; }
    SPH_TRY(check_kernel("sph_interpolate", K));
    if (dest < 0 || dest >= SPH_MAX_ARRAYS || !c->arr[dest].used) { sph_set_error("sph_interpolate: bad destination array %d", dest); return SPH_ERR_ARG; }
    if (nsrc < 1 || nsrc + 1 > SPH_MAX_ARRAYS) { sph_set_error("sph_interpolate: %d source arrays (1..%d)", nsrc, SPH_MAX_ARRAYS - 1); return SPH_ERR_ARG; }
    for (int j = 0; j < nsrc; j++) {
        const int s = srcs[j];
        if (s < 0 || s >= SPH_MAX_ARRAYS || !c->arr[s].used || s == dest) { sph_set_error("sph_interpolate: bad source array %d", s); return SPH_ERR_ARG; }
        for (int i = 0; i < j; i++) if (srcs[i] == s) { sph_set_error("sph_interpolate: source array %d listed twice", s); return SPH_ERR_ARG; }
    }
    const bool order1 = method == SPH_INTERP_ORDER1;
    const int nout = order1 ? 4 : 1;
    if (nprops < 1 || nprops > SPH_INTERP_MAX_PROPS) { sph_set_error("sph_interpolate: %d properties (1..%d)", nprops, SPH_INTERP_MAX_PROPS); return SPH_ERR_ARG; }
    for (int k = 0; k < nprops; k++)
        if (props[k] < 0 || props[k] >= SPH_PROP_COUNT) { sph_set_error("sph_interpolate: bad property %d", props[k]); return SPH_ERR_ARG; }
    for (int k = 0; out_props && k < nprops * nout; k++)
        if (out_props[k] < -1 || out_props[k] >= SPH_PROP_COUNT) { sph_set_error("sph_interpolate: bad output property %d", out_props[k]); return SPH_ERR_ARG; }
    if (!c->nnps_valid) { sph_set_error("sph_interpolate: neighbour grid is stale; call sph_nnps_update"); return SPH_ERR_STATE; }
    DevArray &D = c->arr[dest];
    if (D.nnps_slot < 0) { sph_set_error("sph_interpolate: destination array %d is not part of the neighbour grid", dest); return SPH_ERR_STATE; }
    for (int j = 0; j < nsrc; j++)
        if (c->arr[srcs[j]].nnps_slot < 0) { sph_set_error("sph_interpolate: source array %d is not part of the neighbour grid", srcs[j]); return SPH_ERR_STATE; }
    if (c->ghosts_binned) { sph_set_error("sph_interpolate does not read ghost segments (ghost split): use the plain exchange -> sph_nnps_update order"); return SPH_ERR_UNSUPPORTED; }
    if (!wave_tiles(c)) { sph_set_error("sph_interpolate needs pair_variant 6"); return SPH_ERR_UNSUPPORTED; }
    HIP_TRY(hipSetDevice(c->device));
    SPH_TRY(nnps_need_tables(c));
    if (host_out && n_pull > D.n) { sph_set_error("sph_interpolate: n_pull %zu > %zu points", n_pull, D.n); return SPH_ERR_ARG; }
    if (D.n == 0) return SPH_OK;

    // fp64 only: arith_f32 / record_f32 do not apply here (the records are packed and read as fp64 whatever they say)
    c->nl.valid = false;

    size_t total = 0, off_of[SPH_MAX_ARRAYS];
    for (int j = 0; j < nsrc; j++) { off_of[j] = total; total += c->arr[srcs[j]].n; }
    const size_t d_off = total;
    total += D.n;
    if (total >= (1ull << 32)) { sph_set_error("too many particles for 32-bit packed indices"); return SPH_ERR_ARG; }
    SPH_TRY(c->posh.reserve((total + 64) * sizeof(double) * FamInterpSum::NR));
    SPH_TRY(c->aux.reserve(64));
    SPH_TRY(c->fposb.reserve((total + 64) * sizeof(float4)));
    for (auto &pc : c->pack_cache) pc.epoch = 0; // these records overwrite the shared WCSPH slots

    auto common = [&](auto &a, int nrec, uint32_t flags) {
        fill_common(c, a, K, 0.0, 0.0, nrec);
        a.ablate = 0; a.dbg = nullptr;
        a.nsrc = 0;
        for (int j = 0; j < nsrc; j++) {
            const DevArray &S = c->arr[srcs[j]];
            if (S.n == 0) continue;
            a.src[a.nsrc++] = {S.cell_start.as<uint32_t>(), (uint32_t)off_of[j], flags, S.fine_start.as<uint32_t>(), 0.0, 0u};
        }
        a.d_off = (uint32_t)d_off; a.nd = (uint32_t)D.n;
        a.d_keys = D.keys_sorted.as<uint32_t>(); a.d_fkeys = D.fkeys_sorted.as<uint32_t>(); a.d_perm = D.perm.as<uint32_t>();
        set_tile_order(c, a, D);
        a.d_start = 0; a.d_stop = (uint32_t)D.n; a.dflags = flags;
    };

    // v = m / rho of every source, in original order: the user's rho, or (order1) the summation density over all sources
    const bool need_vol = method != SPH_INTERP_SHEPARD;
    const double *vol[SPH_MAX_ARRAYS] = {};
    bool mom_cached = false;
    if (order1) {
        // the moments (and the densities behind them) depend on positions, h and m only: kept until the next neighbour
        // update, or until something writes h or m
        auto &mc = c->interp_mc;
        unsigned hm = 0;
        for (int j = 0; j < nsrc; j++) hm += c->arr[srcs[j]].hm_writes;
        hm += D.hm_writes; // (the points' h)
        mom_cached = mc.valid && mc.epoch == c->nnps_epoch && mc.dest == dest && mc.nsrc == nsrc && mc.kind == K->kind && mc.dim == K->dim &&
                     mc.fac == K->fac && mc.nd == D.n && mc.hm_writes == hm && memcmp(mc.srcs, srcs, nsrc * sizeof(int)) == 0;
        if (!mom_cached) {
            mc.valid = false;
            for (int j = 0; j < nsrc; j++) {
                SPH_TRY(need_prop(c, srcs[j], SPH_M, "sph_interpolate"));
                SPH_TRY(c->interp_rho[srcs[j]].reserve((c->arr[srcs[j]].n + 64) * sizeof(double)));
                SPH_TRY(c->interp_vol1[srcs[j]].reserve((c->arr[srcs[j]].n + 64) * sizeof(double)));
            }
            SPH_TRY(c->interp_mom.reserve((D.n + 64) * 16 * sizeof(double)));
            // SummationDensity(dest = every source, sources = all of them, real = False) with the library's density
            // kernel into private buffers: the sources' own rho stays what it is
            RecordLayout rl(FAM_DENSITY);
            if (c->uniform_h && c->use_uniform_h) rl.pl.nr = FamDensity::NR_COMPACT;
            {
                ScopedTimer tm(c, T_PACK);
                for (int j = 0; j < nsrc; j++) SPH_TRY(pack_array(c, srcs[j], off_of[j], rl, FAM_DENSITY, F_SD, false, true, 0));
            }
            for (int i = 0; i < nsrc; i++) {
                DevArray &S = c->arr[srcs[i]];
                if (S.n == 0) continue;
                PairArgs<FamDensity> a;
                memset(&a, 0, sizeof a);
                fill_common(c, a, K, 0.0, 0.0, rl.pl.nr);
                a.ablate = 0; a.dbg = nullptr;
                for (int j = 0; j < nsrc; j++) {
                    const DevArray &T = c->arr[srcs[j]];
                    if (T.n == 0) continue;
                    a.src[a.nsrc++] = {T.cell_start.as<uint32_t>(), (uint32_t)off_of[j], (uint32_t)F_SD, T.fine_start.as<uint32_t>(), T.m_value, 0u};
                }
                a.d_off = (uint32_t)off_of[i]; a.nd = (uint32_t)S.n;
                a.d_mu = S.m_value;
                a.d_keys = S.keys_sorted.as<uint32_t>(); a.d_fkeys = S.fkeys_sorted.as<uint32_t>(); a.d_perm = S.perm.as<uint32_t>();
                set_tile_order(c, a, S);
                a.d_start = 0; a.d_stop = (uint32_t)S.n; a.dflags = F_SD;
                a.p.rho = c->interp_rho[srcs[i]].as<double>();
                ScopedTimer tm(c, T_PAIR);
                SPH_TRY(launch_pair_fp64<FamDensity>(c, K->kind, a));
                hipLaunchKernelGGL(k_interp_vol, dim3(div_up(S.n, 256)), dim3(256), 0, c->stream, S.prop[SPH_M],
                                   c->interp_rho[srcs[i]].as<double>(), c->interp_vol1[srcs[i]].as<double>(), S.n);
            }
        }
        for (int j = 0; j < nsrc; j++) vol[srcs[j]] = c->interp_vol1[srcs[j]].as<double>(); // (its own buffers: the sum methods do not touch them)
        if (!mom_cached) {
            {
                ScopedTimer tm(c, T_PACK);
                for (int j = 0; j < nsrc; j++) SPH_TRY(interp_pack(c, srcs[j], off_of[j], 1, &vol[srcs[j]], FamInterpMom::NR));
                SPH_TRY(interp_pack(c, dest, d_off, 0, nullptr, FamInterpMom::NR));
            }
            PairArgs<FamInterpMom> a;
            memset(&a, 0, sizeof a);
            common(a, FamInterpMom::NR, 1u);
            a.p.mom = c->interp_mom.as<double>();
            {
                ScopedTimer tm(c, T_PAIR);
                SPH_TRY(interp_launch<FamInterpMom>(c, K->kind, a));
            }
            c->timers[T_N_INTERP_MOM].count++;
            mc.valid = true; mc.epoch = c->nnps_epoch; mc.dest = dest; mc.nsrc = nsrc; mc.kind = K->kind; mc.dim = K->dim;
            mc.fac = K->fac; mc.nd = D.n; mc.hm_writes = hm;
            memcpy(mc.srcs, srcs, nsrc * sizeof(int));
        }
    } else if (need_vol) {
        for (int j = 0; j < nsrc; j++) {
            DevArray &S = c->arr[srcs[j]];
            if (S.n == 0) continue;
            SPH_TRY(need_prop(c, srcs[j], SPH_M, "sph_interpolate"));
            SPH_TRY(need_prop(c, srcs[j], SPH_RHO, "sph_interpolate"));
            SPH_TRY(c->interp_vol[srcs[j]].reserve((S.n + 64) * sizeof(double)));
            hipLaunchKernelGGL(k_interp_vol, dim3(div_up(S.n, 256)), dim3(256), 0, c->stream, S.prop[SPH_M], S.prop[SPH_RHO],
                               c->interp_vol[srcs[j]].as<double>(), S.n);
            vol[srcs[j]] = c->interp_vol[srcs[j]].as<double>();
        }
    }

    uint32_t flags = 0;
    switch (method) {
    case SPH_INTERP_SHEPARD: flags = F_INORM; break;
    case SPH_INTERP_SPH: flags = F_IVOL; break;
    case SPH_INTERP_SPLASH: flags = F_IVOL | F_IW_DEST; break;
    case SPH_INTERP_SPLASH_NORM: flags = F_IVOL | F_IW_SRC | F_INORM; break;
    default: flags = 1u; break;
    }
    // where result row k (property k / nout, component k % nout) goes: a destination property, or a row of the private
    // block that travels to host_out
    double *out_ptr[SPH_INTERP_MAX_PROPS * 4] = {};
    if (host_out) SPH_TRY(c->interp_out.reserve((size_t)nprops * nout * (D.n + 8) * sizeof(double)));
    for (int k = 0; k < nprops * nout; k++) {
        if (host_out) { out_ptr[k] = c->interp_out.as<double>() + (size_t)k * D.n; continue; }
        if (out_props[k] < 0) continue;
        SPH_TRY(sph_array_ensure_prop(c, dest, out_props[k]));
        sph_mark_written(D, out_props[k]);
        out_ptr[k] = D.prop[out_props[k]];
    }
    // ceil(nprops / W) sweeps; a slot past the last property carries zeros and writes nothing
    for (int p0 = 0; p0 < nprops; p0 += INTERP_W) {
        const int np = std::min(INTERP_W, nprops - p0);
        {
            ScopedTimer tm(c, T_PACK);
            for (int j = 0; j < nsrc; j++) {
                // a source without device storage for a property contributes the value 0 (interpolator.py:360-366: data = 0.0)
                const double *src[1 + INTERP_W] = {};
                src[0] = vol[srcs[j]];
                for (int k = 0; k < np; k++) src[1 + k] = c->arr[srcs[j]].prop[props[p0 + k]];
                SPH_TRY(interp_pack(c, srcs[j], off_of[j], 1 + INTERP_W, src, FamInterpSum::NR));
            }
            SPH_TRY(interp_pack(c, dest, d_off, 0, nullptr, FamInterpSum::NR));
        }
        ScopedTimer tm(c, T_PAIR);
        if (order1) {
            PairArgs<FamInterpRhs> a;
            memset(&a, 0, sizeof a);
            common(a, FamInterpRhs::NR, flags);
            a.p.mom = c->interp_mom.as<double>();
            for (int k = 0; k < np; k++)
                for (int r = 0; r < 4; r++) a.p.out[k][r] = out_ptr[4 * (p0 + k) + r];
            SPH_TRY(interp_launch<FamInterpRhs>(c, K->kind, a));
        } else {
            PairArgs<FamInterpSum> a;
            memset(&a, 0, sizeof a);
            common(a, FamInterpSum::NR, flags);
            for (int k = 0; k < np; k++) a.p.out[k] = out_ptr[p0 + k];
            SPH_TRY(interp_launch<FamInterpSum>(c, K->kind, a));
        }
        c->timers[T_N_INTERP_SWEEP].count++;
    }
    HIP_TRY(hipGetLastError());
    if (host_out && n_pull) {
        for (int k = 0; k < nprops * nout; k++)
            HIP_TRY(hipMemcpyAsync(host_out + (size_t)k * n_pull, out_ptr[k], n_pull * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return SPH_OK;
}
#endif // SPH_PRIMARY_UNIT
