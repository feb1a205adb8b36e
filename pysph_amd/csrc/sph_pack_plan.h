// sph_pack_plan.h -- host side of the record packer: which properties a family packs (pack_plan), the records chosen
// for a block (RecordLayout), their PackArgs::layout, and the launches of k_pack (sph_pack.h).  Included by the primary
// compile of sph_eval.hip after Family / eq_family; host code only.

struct PackPlan {
    int nr; // doubles per interleaved record (== Fam::NR)
    int na;
    int props[MAX_AUX]; // sph_prop or -1
    int derived;        // a PackDerived
};

// What each family packs, one row per Family: `props` are the sph_prop of aux slots 0 .. nprops-1 (-1: a slot k_pack
// derives or leaves zero), `user` the user properties, by name, of the nuser slots behind them.  The slots beyond na are
// the inputs of the derived ones (pack_reads_slot).  A family whose user properties found no free slot is refused by its
// binder (run_mpm, run_adke, run_gas_wall, run_gsph).
struct PackRow {
    int fam, nr, na, derived;
    int nprops, props[19];
    int nuser;
    const char *user[16];
};
typedef FamWCSPHX_T<double, false> RowWCSPHX; // (without the gradrho slots)
typedef FamEDAC_T<double, true> RowEDAC;
#define ROW_OF(FAM, F, DERIVED) FAM, F::NR, F::NA, DERIVED
#define WCSPH_SLOTS 8, {SPH_U, SPH_V, SPH_W, SPH_M, SPH_RHO, -1, SPH_CS, SPH_P}, 0, {}
#define TVF_SLOTS 12, {SPH_U, SPH_V, SPH_W, SPH_UHAT, SPH_VHAT, SPH_WHAT, SPH_RHO, SPH_P, SPH_VOL, SPH_M, -1, -1}, 0, {}
#define GAS_SLOTS 8, {SPH_U, SPH_V, SPH_W, SPH_RHO, SPH_P, SPH_CS, SPH_E, SPH_M}
static constexpr PackRow PACK_ROWS[] = {
    {FAM_NONE, 0, 0, PD_NONE, 0, {}, 0, {}},
    {ROW_OF(FAM_WCSPH, FamWCSPH, PD_P_RHO2), WCSPH_SLOTS},
    {ROW_OF(FAM_DENSITY, FamDensity, PD_NONE), 1, {SPH_M}, 0, {}},
    {ROW_OF(FAM_TVF, FamTVF, PD_VJ2), TVF_SLOTS},
    {ROW_OF(FAM_VGRAD, FamVGrad, PD_M_RHO_VGRAD), 5, {SPH_U, SPH_V, SPH_W, SPH_M, SPH_RHO}, 0, {}},
    {ROW_OF(FAM_ELASTIC, FamElastic, PD_SIGMA_RHO2), 19, {SPH_U, SPH_V, SPH_W, SPH_M, SPH_RHO, SPH_CS, SPH_S00, SPH_S01, SPH_S02,
     SPH_S11, SPH_S12, SPH_S22, SPH_R00, SPH_R01, SPH_R02, SPH_R11, SPH_R12, SPH_R22, SPH_P}, 0, {}},
    {ROW_OF(FAM_NBR, FamNbr, PD_ORIG_INDEX), 0, {}, 0, {}},
    // the WCSPH slots; with a delta-SPH continuity term choose_records adds the sources' gradrho
    {ROW_OF(FAM_WCSPHX, RowWCSPHX, PD_P_RHO2), WCSPH_SLOTS},
    {ROW_OF(FAM_DSPRE, FamDSPre_T<double>, PD_NONE), 2, {SPH_M, SPH_RHO}, 0, {}},
    {ROW_OF(FAM_EDAC, RowEDAC, PD_VJ2), TVF_SLOTS},
    {ROW_OF(FAM_AVGP, FamAvgP_T<double>, PD_NONE), 2, {SPH_M, SPH_P}, 0, {}},
    {ROW_OF(FAM_GASSD, FamGasSD_T<double>, PD_NONE), 4, {SPH_M, SPH_U, SPH_V, SPH_W}, 0, {}},
    {ROW_OF(FAM_MPM, FamMPM_T<double>, PD_NONE), GAS_SLOTS, 3, {"omega", "alpha1", "alpha2"}},
    {ROW_OF(FAM_GSPHGRAD, FamGSPHGrad_T<double>, PD_M_RHO_GGRAD), 6, {SPH_P, SPH_U, SPH_V, SPH_W, SPH_M, SPH_RHO}, 0, {}}, // [p u v w m/rho]
    {ROW_OF(FAM_GSPH, FamGSPH_T<double>, PD_GSPH_SYM), 8, {SPH_U, SPH_V, SPH_W, SPH_RHO, SPH_P, SPH_CS, SPH_M, SPH_E}, 16,
     {"div", "grhox", "grhoy", "grhoz", "px", "py", "pz", "ux", "uy", "uz", "vx", "vy", "vz", "wx", "wy", "wz"}},
    {ROW_OF(FAM_ADKESD, FamADKESD_T<double>, PD_NONE), 4, {SPH_M, SPH_U, SPH_V, SPH_W}, 0, {}},
    {ROW_OF(FAM_ADKE, FamADKE_T<double>, PD_NONE), GAS_SLOTS, 1, {"div"}},
    {ROW_OF(FAM_GASWALL, FamGasWall_T<double>, PD_NONE), GAS_SLOTS, 1, {"div"}},
};
#undef ROW_OF
#undef WCSPH_SLOTS
#undef TVF_SLOTS
#undef GAS_SLOTS
static_assert(sizeof PACK_ROWS / sizeof PACK_ROWS[0] == FAM_COUNT, "one row per Family");
constexpr bool pack_rows_sound()
{
    for (int f = 0; f < FAM_COUNT; f++) {
        const PackRow &r = PACK_ROWS[f];
        if (r.fam != f) return false;                                         // the rows stand in the order of the enum
        if (r.nprops + r.nuser > MAX_AUX) return false;
        if (f != FAM_NONE && r.nr < 4 + r.na) return false;                   // x y z h + the aux slots
        if ((r.nr + 1) / 2 > PACK_MAXP) return false;                         // 16-B pieces of the family's own records
        for (int k = 0; k < MAX_AUX; k++)                                     // every slot k_pack reads beyond na is in the row
            if (k >= r.na && k >= r.nprops + r.nuser && pack_reads_slot(r.derived, r.na, k)) return false;
    }
    return true;
}
static_assert(pack_rows_sound(), "PACK_ROWS disagrees with Family, MAX_AUX, PACK_MAXP or pack_reads_slot");

// the row of `fam` with its user properties resolved (once, on the first use of that family)
static PackPlan pack_plan(int fam)
{
    static PackPlan plans[FAM_COUNT];
    static bool resolved[FAM_COUNT];
    if (fam <= FAM_NONE || fam >= FAM_COUNT) {
        sph_set_error("pack_plan: no family %d", fam);
        fam = FAM_NONE; // an empty plan: nothing is packed
    }
    PackPlan &p = plans[fam];
    if (!resolved[fam]) {
        const PackRow &r = PACK_ROWS[fam];
        p.nr = r.nr; p.na = r.na; p.derived = r.derived;
        for (auto &v : p.props) v = -1;
        for (int k = 0; k < r.nprops; k++) p.props[k] = r.props[k];
        for (int k = 0; k < r.nuser; k++) p.props[r.nprops + k] = sph_prop_register(r.user[k]);
        resolved[fam] = true;
    }
    return p;
}

// which aux slots a family really needs given the union of flags (others may be absent -> 0); an error code for no family
static int slot_required(int fam, uint32_t flags, int prop)
{
    switch (fam) {
    case FAM_WCSPH:
        if (prop == SPH_M || prop == SPH_U || prop == SPH_V || prop == SPH_W) return 1;
        if (prop == SPH_RHO) return (flags & (F_MOM | F_XSPH)) != 0;
        if (prop == SPH_P || prop == SPH_CS) return (flags & F_MOM) != 0;
        return 0;
    case FAM_WCSPHX:
        if (prop == SPH_M || prop == SPH_U || prop == SPH_V || prop == SPH_W || prop == SPH_RHO) return 1;
        if (prop == SPH_P || prop == SPH_CS) return (flags & F_MOM) != 0;
        return (flags & F_DCONT) != 0; // SPH_GRADRHO0..2
    case FAM_DENSITY: return prop == SPH_M;
    case FAM_NBR: return 0;
    case FAM_ELASTIC:
        if (prop == SPH_U || prop == SPH_V || prop == SPH_W || prop == SPH_M) return 1;
        if (prop == SPH_RHO) return (flags & (F_ESTRESS | F_EAV | F_EXSPH)) != 0;
        if (prop == SPH_CS) return (flags & F_EAV) != 0;
        if (prop == SPH_P) return (flags & F_ESTRESS) != 0;
        if (prop >= SPH_S00 && prop <= SPH_S22) return (flags & F_ESTRESS) != 0;
        return 0; // r_ij default to 0 when absent
    case FAM_TVF:
    case FAM_EDAC:
        if (prop == SPH_UHAT || prop == SPH_VHAT || prop == SPH_WHAT) return (flags & F_TAS) != 0;
        return 1;
    case FAM_AVGP: return prop == SPH_M ? (flags & (F_SD | F_TVFSD)) != 0 : (flags & F_AVGP) != 0;
    case FAM_DSPRE: case FAM_VGRAD: case FAM_GASSD: case FAM_MPM: case FAM_GSPHGRAD: case FAM_GSPH: case FAM_ADKESD: case FAM_ADKE:
    case FAM_GASWALL:
        return 1;
    default: sph_set_error("slot_required: no family %d", fam); return SPH_ERR_UNSUPPORTED;
    }
}

// A destination that is not among the sources is only read through Fam::load: it does not need a mass unless the
// equation uses the destination's own (transport_velocity.SummationDensity: rho_i = m_i sum W)
static int dest_mass_free(int fam, uint32_t flags)
{
    switch (fam) {
    case FAM_WCSPH: case FAM_WCSPHX: return 1;
    case FAM_DENSITY: return !(flags & F_TVFSD);
    case FAM_TVF: case FAM_VGRAD: case FAM_ELASTIC: case FAM_NBR: case FAM_DSPRE: case FAM_EDAC: case FAM_AVGP: case FAM_GASSD: case FAM_MPM:
    case FAM_GSPHGRAD: case FAM_GSPH: case FAM_ADKESD: case FAM_ADKE: case FAM_GASWALL:
        return 0;
    default: sph_set_error("dest_mass_free: no family %d", fam); return SPH_ERR_UNSUPPORTED;
    }
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

// the layouts with a fixed piece count hold exactly the record their family's loader reads
#define PIECES_ARE(ID, NR) static_assert(pack_traits(ID).pieces * pack_traits(ID).per == (NR), #ID ": pieces x values per piece is not " #NR)
PIECES_ARE(PL_DENSITY, FamDensity::NR_COMPACT);
PIECES_ARE(PL_DENSITY, FamNbr::NR_COMPACT);
PIECES_ARE(PL_WCSPH_EOS, FamWCSPHE_T<double>::NR);
PIECES_ARE(PL_WCSPH_EOS_F32, FamWCSPHE_T<float>::NR);
PIECES_ARE(PL_WCSPH_EOSV, FamWCSPHV_T<double>::NR);
PIECES_ARE(PL_WCSPH_EOSV_F32, FamWCSPHV_T<float>::NR);
PIECES_ARE(PL_ELASTIC_U, FamElasticU_T<double>::NR_U);
PIECES_ARE(PL_ELASTIC_U_F32, FamElasticU_T<float>::NR_U);
#undef PIECES_ARE
static_assert(pack_traits(PL_ELASTIC_U).pieces == FamElasticU_T<double>::PIECES && pack_traits(PL_ELASTIC_U_F32).pieces == FamElasticU_T<float>::PIECES,
              "k_pack and FamElasticU_T::decode count the same pieces");
static_assert(FamTVF::NR_COMPACT_M / pack_traits(PL_TVF).per <= PACK_MAXP && FamTVFE_T<double>::NR_FUSED_AS / pack_traits(PL_TVF_STATE).per <= PACK_MAXP &&
              FamTVFE_T<float>::NR_FUSED_AS / pack_traits(PL_TVF_STATE_F32).per <= PACK_MAXP, "PACK_MAXP is the piece count of the widest record");

// PackArgs::layout of these records
static int pack_layout(const RecordLayout &rl, int fam, bool wave)
{
    static const int fused[] = {PL_PLAIN, PL_WCSPH_EOS, PL_WCSPH_EOSV, PL_TVF_STATE, PL_ELASTIC_U}; // by RecordKind, in fp64
    if (rl.kind != REC_PLAIN) return rl.arith_f32 ? pack_traits(fused[rl.kind]).f32 : fused[rl.kind];
    if (!wave) return PL_PLAIN;
    if (rl.record_f32 || rl.arith_f32) return PL_F32;
    if (fam == FAM_WCSPH) return PL_WCSPH;
    if ((fam == FAM_DENSITY || fam == FAM_NBR) && rl.pl.nr == FamDensity::NR_COMPACT) return PL_DENSITY;
    if ((fam == FAM_TVF || fam == FAM_EDAC) && (rl.pl.nr == FamTVF::NR_COMPACT_M || rl.pl.nr == FamTVF::NR_COMPACT)) return PL_TVF;
    return PL_PLAIN;
}

// 16-B pieces of one packed record, as k_pack counts them; 0: records that are not a whole number of
// pieces (no LDS transposition, per-lane stores)
static int pack_pieces(const PackArgs &pa)
{
    if (!pa.rec) return 0;
    const int per = pack_traits(pa.layout).per;
    return (pa.nr % per) ? 0 : pa.nr / per;
}

// k_pack with the layout as a compile-time constant where the library has an instantiation (PACK_LAYOUT_TABLE: COMPILED)
static void launch_pack(sph_ctx *c, const PackArgs &pa, size_t n)
{
    const dim3 g(div_up(n, 256)), b(256);
    const size_t lds = (size_t)pa.lds_np * 256 * 16;
    switch (pa.rec ? pa.layout : -1) {
#define X(ID, PER, PIECES, NV, COMPILED, F32) \
    case ID: hipLaunchKernelGGL(k_pack<(COMPILED) ? (int)ID : -1>, g, b, lds, c->stream, pa); break;
        PACK_LAYOUT_TABLE(X)
#undef X
    default: hipLaunchKernelGGL(k_pack<-1>, g, b, lds, c->stream, pa); break;
    }
}

// `launch` false: validate only (the records of this array are already in the packed buffer, see
// the pack cache in sph_eval_group)
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
        if (pack_reads_slot(pl.derived, pl.na, k) && pl.props[k] >= 0) {
            pa.src[k] = A.prop[pl.props[k]];
            if (pa.src[k]) continue;
            const int required = slot_required(fam, flags, pl.props[k]), mass_free = dest_mass_free(fam, flags);
            if (required < 0 || mass_free < 0) return SPH_ERR_UNSUPPORTED;
            if (required && !(dest_only && pl.props[k] == SPH_M && mass_free)) return need_prop(c, id, pl.props[k], "pair loop");
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
        if (rl.umass) { // ... except p / rho^2, which takes the place of the (uniform) mass: PD_P_RHO2 reads p
            pa.umass = 1;
            pa.src[3] = nullptr; // the record holds no mass
        } else {
            pa.src[7] = nullptr;
            pa.derived = PD_NONE;
        }
        // ... and no h: the prefilter's radius_scale * h from the launch constant of the pair kernel (fill_common: hu)
        pa.h = nullptr;
        pa.hu = 0.5 * (c->h_uniform + c->h_uniform);
    }
    // REC_ELU: h and m are launch / source constants
    if (rl.kind == REC_EOSV) { // p, cs, p / rho^2 recomputed, m a source constant: none of them read here
        pa.src[3] = pa.src[5] = pa.src[6] = pa.src[7] = nullptr;
        pa.derived = PD_NONE;
    }
    if (rl.kind == REC_TVFF) { // p and V are functions of rho (and the one mass): not read here
        pa.src[7] = pa.src[8] = pa.src[9] = nullptr;
        pa.derived = PD_NONE;
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
