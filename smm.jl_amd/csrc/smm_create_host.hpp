// context creation as a sequence of steps, smm_ctx_destroy, smm_describe (included once by smmhip.hip, last; DESIGN.md, "The forms and context creation")
#pragma once

namespace {

// workgroups per CU of F's candidate persistent kernel, its dynamic LDS set first; a user objective's kernel is compiled and loaded here.  0: not available
int persist_occupancy(Ctx* c, const Forms& F, int objective_id) {
    if (F.persist_user || (F.persist == PERSIST_TILE && c->obj == SMM_OBJ_USER)) {   // (user_form_compile)
        const UserForm form = user_form_wanted(F, c->has_chol);
        {
            std::lock_guard<std::mutex> lock(g_user_mutex);
            UserObjective& u = g_user_objectives[objective_id - SMM_OBJ_USER_BASE];
            if (!user_form_compile(u, form)) {
                if (getenv("SMMHIP_VERBOSE"))
                    fprintf(stderr, "libsmmhip: the persistent form of this user objective is not available:\n%s\n", u.form[form].log.c_str());
                return 0;
            }
            HIPCHK(hipModuleLoadData(&c->pmod, u.form[form].code.data()));
        }
        HIPCHK(hipModuleGetFunction(&c->pfn, c->pmod, user_form_kernel(form)));
    }
    const PersistKernel K = persist_kernel(c, F);
    int per_cu = 0;
    if (K.mfn) {
        // (a module's function: not every runtime takes the attribute this way; the launch asks for what it needs)
        (void)hipFuncSetAttribute((const void*)K.mfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)K.smem);
        (void)hipGetLastError();
        HIPCHK(hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, K.mfn, K.block.x, K.smem));
    } else {
        HIPCHK(hipFuncSetAttribute(K.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)K.smem));
        HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, K.fn, K.block.x, K.smem));
    }
    return per_cu;
}

// one set of cone tables for the plan window, per iteration: the tiles' headers, sub-levels' pairs and, with_gather, gather lists; cone_ok zeroed
void alloc_cones(Ctx* c, LevelTables& S, size_t tiles, bool with_gather) {
    const size_t W = (size_t)c->F.plan_cap;
    S.cone_ok = dalloc<uint32_t>(c, W);
    S.cone_hdr = dalloc<uint32_t>(c, W * tiles * CONE_HDRW);
    S.cone_pairs = dalloc<uint32_t>(c, W * tiles * (CONE_LEVELS * 64) + 1024);   // (+: whole 1 KB pieces are fetched)
    S.cone_gather = with_gather ? dalloc<uint16_t>(c, W * tiles * CONE_GCAP + 512) : nullptr;
    HIPCHK(hipMemset((void*)S.cone_ok, 0, W * 4));
}
// ... and of its level tables: the levels' pairs, thresholds and offsets; rows: those of k_exch_resolve_rows; tiles > 0: the cone tables
void alloc_level_tables(Ctx* c, LevelTables& S, bool rows, size_t tiles, bool with_gather) {
    const size_t W = (size_t)c->F.plan_cap, K = (size_t)c->P.plan_K;
    S.lv_pairs = dalloc<uint32_t>(c, W * K);
    S.lv_mi = dalloc<double>(c, W * K);
    S.lv_off = dalloc<uint32_t>(c, W * (K + 2));
    if (rows) S.lv_rows = dalloc<uint32_t>(c, W * c->P.rows_cap * XWG);
    if (rows) S.lv_rowinfo = dalloc<uint32_t>(c, W * 4);
    if (tiles) alloc_cones(c, S, tiles, with_gather);
}

// the persistent form's ring (a shard's lives in its p2p window) and the state persist_repair rolls back to (hist_fill: a row of the history's fill)
void alloc_persist(Ctx* c) {
    KParams& P = c->P;
    const size_t N = P.N;
    if (!c->F.persist_sh) {
        const PrWin WL = pr_win_layout(P.Ng, P.RW, 1, persist_tiles_rank(c->F, P.N));
        c->prw = dalloc<unsigned char>(c, WL.total);
        HIPCHK(hipMemset(c->prw, 0, WL.total));
    }
    c->snap_cs = dalloc<double>(c, N * CSW);
    c->snap_rec = dalloc<double>(c, N * P.RW);
    for (int b = 0; b < 2; ++b) { c->snap_vals[b] = dalloc<double>(c, N + 4); c->snap_slot8[b] = dalloc<uint2>(c, N + 4 + 128); }
    c->snap_xres = dalloc<unsigned long long>(c, P.Ng);
    c->hist_fill = dalloc<double>(c, N * P.HW);
    HIPCHK(hipMemcpy(c->hist_fill, P.hrec, N * P.HW * 8, hipMemcpyDeviceToDevice));   // (a row of the constructor's fill)
}

// every refusal of smm_ctx_create that needs no device, in this order
int check_create_args(const smm_problem_t* prob, const smm_bgp_opts_t* opts, const smm_tables_t* tab, void** out) {
    if (!prob || !opts || !out) return fail(nullptr, SMM_ERR_INVALID_ARG, "null argument");
    const int np = prob->np, nm = prob->nm, ns = prob->ns, N = opts->N, T = opts->maxiter, Ng = opts->N_global;
    if (np < 1 || nm < 1 || ns < 1 || np > MAX_DIM || nm > MAX_DIM)
        return fail(nullptr, SMM_ERR_INVALID_ARG, "need 1 <= np,nm <= 64 and ns >= 1");
    if (N < 1 || T < 1 || Ng < N || opts->chain_offset < 0 || opts->chain_offset + N > Ng || (Ng % N) != 0)
        return fail(nullptr, SMM_ERR_INVALID_ARG, "bad N / N_global / chain_offset / maxiter");
    if (prob->objective_id >= SMM_OBJ_USER_BASE) {
        std::lock_guard<std::mutex> lock(g_user_mutex);
        if (prob->objective_id - SMM_OBJ_USER_BASE >= (int)g_user_objectives.size())
            return fail(nullptr, SMM_ERR_INVALID_ARG, "unknown user objective handle");
    } else if (prob->objective_id < 0 || (prob->objective_id > SMM_OBJ_DENSE && prob->objective_id != SMM_OBJ_DENSE2))
        return fail(nullptr, SMM_ERR_INVALID_ARG, "unknown objective_id");
    if (is_sim(prob->objective_id) && np != nm)
        return fail(nullptr, SMM_ERR_INVALID_ARG, "objfunc_norm needs one moment per parameter (ObjExamples.jl:66-78)");
    if (opts->batch_size < 1 || opts->batch_size > np || (np % opts->batch_size) != 0)
        return fail(nullptr, SMM_ERR_BAD_BATCH, "batch_size must divide the number of parameters (AlgoBGP.jl:95-103)");
    if (opts->sigma_update_steps < 1) return fail(nullptr, SMM_ERR_INVALID_ARG, "sigma_update_steps < 1");
    if (opts->smpl_iters < 1) return fail(nullptr, SMM_ERR_INVALID_ARG, "smpl_iters < 1 (AlgoBGP.jl:521: at least one proposal try)");
    // the exchange of iteration t reads the history of iteration t-1: the reference starts at algo.i >= 2 (AlgoBGP.jl:637)
    if (opts->exchange_from_iter < 2) return fail(nullptr, SMM_ERR_INVALID_ARG, "exchange_from_iter < 2 (AlgoBGP.jl:637)");
    if (!prob->init || !prob->lb || !prob->ub || !prob->mom || !prob->w)
        return fail(nullptr, SMM_ERR_INVALID_ARG, "smm_problem_t: init / lb / ub / mom / w must not be NULL");
    if (!opts->sigma || !opts->acc_tuner || !opts->min_improve)
        return fail(nullptr, SMM_ERR_INVALID_ARG, "smm_bgp_opts_t: sigma / acc_tuner / min_improve must not be NULL (length N_global)");
    if (prob->n_obj_params > 0 && !prob->obj_params) return fail(nullptr, SMM_ERR_INVALID_ARG, "n_obj_params > 0 but obj_params is NULL");
    if (tab && tab->pairs && tab->n_pairs > 0) {   // injected pair lists: 0 <= i < j < N_global (16-bit packing in the plans)
        for (size_t q = 0; q < (size_t)T * tab->n_pairs; ++q) {
            const int32_t i = tab->pairs[2 * q], j = tab->pairs[2 * q + 1];
            if (i < 0 || j <= i || j >= Ng) return fail(nullptr, SMM_ERR_INVALID_ARG, "smm_tables_t.pairs: need 0 <= i < j < N_global");
        }
    }
    if (tab && tab->prop_normals && tab->prop_tries < 1) return fail(nullptr, SMM_ERR_INVALID_ARG, "prop_normals given but prop_tries < 1");
    if (opts->dist_fun < SMM_DIST_MINUS || opts->dist_fun > SMM_DIST_RELDIFF)
        return fail(nullptr, SMM_ERR_INVALID_ARG, "smm_bgp_opts_t.dist_fun: SMM_DIST_MINUS, SMM_DIST_ABSDIFF or SMM_DIST_RELDIFF");
    if (opts->chol_L && opts->batch_size != np)
        return fail(nullptr, SMM_ERR_BAD_BATCH, "Cholesky proposals (chol_L) draw all parameters in one batch: batch_size must equal np");
    return SMM_OK;
}

// what select_forms, the size functions and smm_describe read, from the arguments, hooks and registry alone: no device.  nullptr, or why refused (SMM_ERR_HIP)
const char* create_facts(Ctx* c, const smm_problem_t* prob, const smm_bgp_opts_t* opts, const smm_tables_t* tab) {
    KParams& P = c->P;
    const int np = prob->np, nm = prob->nm, N = opts->N, T = opts->maxiter, Ng = opts->N_global;
    const bool user_obj = prob->objective_id >= SMM_OBJ_USER_BASE;
    c->device = opts->device;
    c->obj = user_obj ? SMM_OBJ_USER : prob->objective_id == SMM_OBJ_DENSE2 ? SMM_OBJ_DENSE : prob->objective_id;   // (spec v2: the dense kind with its 256 x 256 stage)
    c->dense2 = prob->objective_id == SMM_OBJ_DENSE2;
    c->exchange_from = P.exch_from = opts->exchange_from_iter;
    const char* d = getenv("SMMHIP_DBG");
    P.dbg = d ? atoi(d) : 0;
    P.scout_after = c->H.scout_after; P.scout_gl = c->H.scout_gl;
    P.np = np; P.nm = nm; P.ns = prob->ns; P.obj = c->obj;
    c->n_objp = prob->n_obj_params > 0 ? prob->n_obj_params : 0;
    if (user_obj) {
        std::lock_guard<std::mutex> lock(g_user_mutex);
        const UserObjective& u = g_user_objectives[prob->objective_id - SMM_OBJ_USER_BASE];
        c->u_lanes = u.lanes; c->u_nsums = u.n_sums; c->u_rng = u.rng;
    }
    if (c->obj == SMM_OBJ_DENSE) {   // [B, A2, A]: with the 256 x 256 stage in spec v2
        const size_t nB = (size_t)DENSE_D * np, n2 = c->dense2 ? (size_t)DENSE_D * DENSE_D : 0, nA = (size_t)nm * DENSE_D;
        if (prob->n_obj_params != 0 && (size_t)prob->n_obj_params != nB + n2 + nA)
            return c->dense2 ? "SMM_OBJ_DENSE2: obj_params must hold B (256 x np), A2 (256 x 256) and A (nm x 256), or be empty"
                             : "SMM_OBJ_DENSE: obj_params must hold B (256 x np) and A (nm x 256), or be empty";
        P.dense_nOt = (nm + 15) / 16;
    }
    P.N = N; P.Ng = Ng; P.offset = opts->chain_offset; P.T = T;
    P.sigma_update_steps = opts->sigma_update_steps; P.smpl_iters = opts->smpl_iters;
    P.batch_size = opts->batch_size; P.sigma_adjust_by = opts->sigma_adjust_by; P.seed = opts->seed;
    c->has_chol = opts->chol_L != nullptr;
    if (c->has_chol) P.chol_per_chain = opts->chol_per_chain ? 1 : 0;
    P.dist_fun = opts->dist_fun; P.mi_uniform = 1; P.mi_value = opts->min_improve[0];
    for (int i = 1; i < Ng; ++i)
        if (!(opts->min_improve[i] == P.mi_value || (opts->min_improve[i] != opts->min_improve[i] && P.mi_value != P.mi_value))) P.mi_uniform = 0;   // (NaN everywhere is one threshold too: nothing ever swaps)
    // per-chain thresholds (AlgoBGP.jl:522): the persistent forms walk them too (smm_walk_lean.hpp PCT) where every one is >= 0 or NaN and dist_fun is `-`
    P.mi_pct = !P.mi_uniform && opts->dist_fun == SMM_DIST_MINUS;
    for (int i = 0; i < Ng; ++i) if (opts->min_improve[i] < 0.0) P.mi_pct = 0;
    c->has_utab = tab && tab->probs_acc; c->has_ntab = tab && tab->prop_normals && tab->prop_tries > 0;
    // tries of mysample whose normals are made ahead of time (k_pregen_rng; later ones are drawn in the chain kernel): past 8 parameters two (C4: four cost 9 %)
    P.user_n = c->has_ntab; P.rb_tries = c->has_ntab ? tab->prop_tries : np <= 8 ? 8 : 2;
    if ((size_t)P.rb_tries * (size_t)((np + 1) / 2) * (size_t)N >= ((size_t)1 << 31))   // (k_pregen_rng indexes one iteration's pieces in 32 bits)
        return "injected proposal normals: tries x parameters x chains of one iteration must stay below 2^31 pieces";
    if (tab && tab->pairs && tab->n_pairs > 0) {
        P.n_pairs_tab = tab->n_pairs;
        // dependency depth of the injected lists (pairs sharing a chain keep their order): the lean walks hold LV_MAXLEV levels
        std::vector<int> last((size_t)Ng);
        for (int it = 0; it < T && !c->deep_plan; ++it) {
            std::fill(last.begin(), last.end(), 0);
            for (int q = 0; q < tab->n_pairs; ++q) {
                const int32_t i = tab->pairs[2 * ((size_t)it * tab->n_pairs + q)], j = tab->pairs[2 * ((size_t)it * tab->n_pairs + q) + 1];
                const int lv = std::max(last[i], last[j]) + 1;
                last[i] = last[j] = lv;
                if (lv > LV_MAXLEV) { c->deep_plan = true; break; }
            }
        }
    }
    P.RW = even_up(3 + np + nm); P.HW = even_up(H_PARAMS + np + nm); P.RBW = even_up(1 + P.rb_tries * np);
    P.plan_K = exchange_K(c);
    return nullptr;
}

// the dense objective's operands M = [B (256 x np) | A2 (256 x 256: v2) | A (nm x 256)] in fragment order: Bf [row tile][parameter step][lane],
// Af [moment tile][row tile][k-step][lane], A2f [wave][k-step][lane][the wave's two row tiles] (smm_chain.hpp: dense2_tile_n)
void dense_operands(const std::vector<double>& M, int np, int nm, bool v2, std::vector<double>& Bf, std::vector<double>& Af, std::vector<double>& A2f) {
    const size_t nB = (size_t)DENSE_D * np, n2 = v2 ? (size_t)DENSE_D * DENSE_D : 0;
    const int nPs = (np + 3) / 4, nOt = (nm + 15) / 16;
    Bf.assign((size_t)(DENSE_D / 16) * nPs * 64, 0.0);
    Af.assign((size_t)nOt * (DENSE_D / 16) * 4 * 64, 0.0);
    for (int T = 0; T < DENSE_D / 16; ++T)
        for (int s = 0; s < nPs; ++s)
            for (int l = 0; l < 64; ++l) {
                const int d = 16 * T + (l & 15), p = 4 * s + (l >> 4);
                if (p < np) Bf[((size_t)T * nPs + s) * 64 + l] = M[(size_t)d * np + p];
            }
    for (int o = 0; o < nOt; ++o)
        for (int T = 0; T < DENSE_D / 16; ++T)
            for (int s = 0; s < 4; ++s)
                for (int l = 0; l < 64; ++l) {
                    const int k = 16 * o + (l & 15), d = 16 * T + 4 * s + (l >> 4);
                    if (k < nm) Af[(((size_t)o * (DENSE_D / 16) + T) * 4 + s) * 64 + l] = M[nB + n2 + (size_t)k * DENSE_D + d];
                }
    if (!v2) return;
    A2f.resize((size_t)DENSE_D * DENSE_D);
    for (int wv = 0; wv < 8; ++wv)
        for (int s = 0; s < DENSE_D / 4; ++s)
            for (int l = 0; l < 64; ++l)
                for (int tt = 0; tt < 2; ++tt) {
                    const int j = 16 * (2 * wv + tt) + (l & 15), d = 4 * s + (l >> 4);
                    A2f[(((size_t)wv * (DENSE_D / 4) + s) * 64 + l) * 2 + tt] = M[nB + (size_t)j * DENSE_D + d];
                }
}
// the device (stream, events, compute units) and the uploads: the problem, a user objective's module, the dense operands, the shock table, the options, the injected tables
void upload_inputs(Ctx* c, const smm_problem_t* prob, const smm_bgp_opts_t* opts, const smm_tables_t* tab) {
    KParams& P = c->P;
    const size_t N = (size_t)P.N, TN = (size_t)P.T * P.N;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreate(&c->ev0));
    HIPCHK(hipEventCreate(&c->ev1));
    (void)hipDeviceGetAttribute(&c->dev.n_cus, hipDeviceAttributeMultiprocessorCount, c->device);
    const char* tsv = getenv("SMMHIP_TS");
    if (tsv && (tsv[0] == '1' || tsv[0] == '2')) P.ts = dalloc<unsigned long long>(c, (size_t)8 * 65536);
    P.ts_levels = tsv && tsv[0] == '2';   // also a stamp per level of the inline walk (the stamps stretch the levels: not with '1')
    P.init = dupload(c, prob->init, P.np); P.lb = dupload(c, prob->lb, P.np); P.ub = dupload(c, prob->ub, P.np);
    P.mom = dupload(c, prob->mom, P.nm); P.w = dupload(c, prob->w, P.nm);
    P.objp = prob->n_obj_params > 0 ? dupload(c, prob->obj_params, prob->n_obj_params) : nullptr;
    if (c->obj == SMM_OBJ_USER) {
        {
            std::lock_guard<std::mutex> lock(g_user_mutex);
            HIPCHK(hipModuleLoadData(&c->umod, g_user_objectives[prob->objective_id - SMM_OBJ_USER_BASE].code.data()));
        }
        HIPCHK(hipModuleGetFunction(&c->ufn, c->umod, "smm_user_eval_kernel"));
        if (c->u_rng) HIPCHK(hipModuleGetFunction(&c->ufn_noseed, c->umod, "smm_user_eval_noseed_kernel"));
        P.u_theta = dalloc<double>(c, N * P.np); P.u_simM = dalloc<double>(c, N * P.nm);
        P.u_value = dalloc<double>(c, N); P.u_status = dalloc<int>(c, N);
    }
    if (c->obj == SMM_OBJ_DENSE) {   // its operands: the caller's (obj_params), or N(0,1)/sqrt(fan-in) from the counter RNG, stream 5
        const size_t nB = (size_t)DENSE_D * P.np;
        std::vector<double> M(nB + (c->dense2 ? (size_t)DENSE_D * DENSE_D : 0) + (size_t)P.nm * DENSE_D);
        if (prob->n_obj_params) memcpy(M.data(), prob->obj_params, M.size() * 8);
        else {
            for (size_t i = 0; i < M.size(); i += 2) {
                double z0, z1;
                box_muller(philox_stream(P.seed, 5, (uint32_t)(i >> 1), (uint32_t)((i >> 1) >> 32), 0, 0), z0, z1);
                M[i] = z0 / sqrt(i < nB ? (double)P.np : (double)DENSE_D);
                if (i + 1 < M.size()) M[i + 1] = z1 / sqrt(i + 1 < nB ? (double)P.np : (double)DENSE_D);
            }
        }
        std::vector<double> Bf, Af, A2f;
        dense_operands(M, P.np, P.nm, c->dense2, Bf, Af, A2f);
        P.dense_Bf = dupload(c, Bf.data(), Bf.size());
        P.dense_Af = dupload(c, Af.data(), Af.size());
        if (c->dense2) P.dense_A2f = dupload(c, A2f.data(), A2f.size());
    }
    // the shock table Z [nm][zstride]: the caller's, or the counter RNG's
    const int rows = (P.ns + WG - 1) / WG;
    P.zstride = ((rows + ZU) / ZU) * ZU * WG;  // at least one chunk beyond the last full one
    std::vector<double> Z((size_t)P.nm * P.zstride, 0.0);
    for (int k = 0; k < P.nm; ++k)
        for (int s = 0; s < P.ns; ++s)
            Z[(size_t)k * P.zstride + s] = (tab && tab->Z) ? tab->Z[(size_t)k * P.ns + s] : rng_Z(P.seed, (uint32_t)k, (uint32_t)s);
    P.Z = dupload(c, Z.data(), Z.size());
    P.min_improve_g = dupload(c, opts->min_improve, P.Ng);
    if (c->has_chol) P.chol_L = dupload(c, opts->chol_L, (size_t)(P.chol_per_chain ? P.Ng : 1) * P.np * P.np);
    if (c->has_utab) P.user_utab = dupload(c, tab->probs_acc, TN);
    if (c->has_ntab) P.user_ntab = dupload(c, tab->prop_normals, TN * (size_t)tab->prop_tries * P.np);
    if (P.n_pairs_tab > 0) P.pairtab = dupload(c, tab->pairs, (size_t)P.T * tab->n_pairs * 2);
}

// the forms: on the compute units, then on the candidate persistent kernel's occupancy (ask: the device's; else as given, -1: none), and what KParams says of them
void choose_forms(Ctx* c, int objective_id, bool ask = true, int per_cu = -1) {
    KParams& P = c->P;
    Forms& F = c->F;
    F = select_forms(c, c->H, c->dev);
    if (F.persist != PERSIST_NONE && (ask || per_cu >= 0)) {
        c->dev.per_cu = ask ? persist_occupancy(c, F, objective_id) : per_cu;
        F = select_forms(c, c->H, c->dev);
    }
    P.tile_off = F.tile_off;
    P.gen_lean = F.gen_keys ? 2 : F.gen_lean ? 1 : 0;
    P.rows_cap = F.rows_cap;
    if (F.lean_plan) {
        P.lean_wide = F.lean_wide ? 1 : 0;
        P.plan_Kp = lean_walk_Kp(P.plan_K);
        P.lean_unit = F.lean_wide ? LeanLayout<LEAN_WIDE>::unit(P.Ng) : LeanLayout<LEAN_KEYS>::unit(P.Ng);
    }
    if (F.cone_tiles) { P.cone_tiles = F.cone_tiles; P.cone_ct = F.cone_ct; }
}

// Does the context plan its next window BESIDE its persistent chain kernel (k_exch_plan_bg on a second stream) instead of ahead of it on the
// main stream?  A single shard on k_chain_persist_loc with the LDS plan, whose pairs' state fits that kernel's LDS (plan_bg_fits: up to
// some 4390 chains), and one chain workgroup plus one background workgroup resident on a compute unit by arithmetic:
//   registers   4 waves x 120 (PL_VGPR_HALF) + 1 wave x 32 (PBG_VGPR_HALF) = 512 per lane and SIMD, the whole file;
//   wave slots  16 + 4 of 32;
//   LDS         persist_loc_smem_bytes(np) + PBG_LDS, each rounded up to the granule of 1280 bytes, within the unit's 160 KiB;
//   PBG_LDS     more than half the unit's: a second background workgroup never takes the room of a chain workgroup.
// (tests/test_plan_beside_budget.py holds the kernels to these figures.)  SMMHIP_PLAN_AHEAD=0 of the test build switches the path off.
constexpr size_t LDS_GRANULE = 1280;
bool plan_beside_resident(int np) {
    auto up = [](size_t b) { return (b + LDS_GRANULE - 1) / LDS_GRANULE * LDS_GRANULE; };
    return up(persist_loc_smem_bytes(np)) + up(PBG_LDS + PBG_LDS_STATIC) <= LDS_CU && PBG_LDS > LDS_HALF && 4 * 2 * PL_VGPR_HALF + 2 * PBG_VGPR_HALF <= 512;
}
void choose_plan_beside(Ctx* c) {
    const Forms& F = c->F;
    const KParams& P = c->P;
    c->plan_beside = F.plan == PLAN_LDS && F.persist == PERSIST_LOC && !F.persist_sh && P.N == P.Ng && F.cone_tiles > 0 && F.cone_gather && F.plan_cap >= 2 &&
                     !c->H.plan_ahead_off && plan_bg_fits(P.Ng, P.plan_K) && plan_beside_resident(P.np);
}

// the look-ahead tables: the window of randomness blocks, the plan window's set of level tables (c->win) and what the forms add to it
void alloc_windows(Ctx* c) {
    KParams& P = c->P;
    const Forms& F = c->F;
    const size_t N = (size_t)P.N, Ng = (size_t)P.Ng, K = (size_t)P.plan_K, W = (size_t)F.plan_cap;
    c->win_rb = dalloc<double>(c, (size_t)F.win_cap * N * P.RBW);
    HIPCHK(hipMemset(c->win_rb, 0, (size_t)F.win_cap * N * P.RBW * 8));
    if (F.plan != PLAN_NONE) alloc_level_tables(c, c->win, F.xk == XK_ROWS, (size_t)F.cone_tiles, F.cone_gather);
    P.cone_ok = c->win.cone_ok; P.cone_hdr = c->win.cone_hdr; P.cone_pairs = c->win.cone_pairs; P.cone_gather = c->win.cone_gather;
    if (F.plan == PLAN_BIG) c->big_scratch = dalloc<uint32_t>(c, W * BigPlanScratch::words(P.Ng, P.plan_K));
    if (F.xk == XK_ROWS) {
        c->slots17 = dalloc<uint32_t>(c, Ng + 4);
        c->nan_flags = dalloc<uint32_t>(c, 4);
        HIPCHK(hipMemset(c->nan_flags, 0, 16));
    }
    if (F.plan == PLAN_LDS) {
        c->win_plan = dalloc<unsigned long long>(c, W * K);
        c->win_plan_mi = dalloc<double>(c, W * K);
    }
    if (F.lean_plan) {
        c->win_lv_pairs_p = dalloc<uint32_t>(c, W * P.plan_Kp + 512);   // (+512: whole 1 KB pieces may be read past the last iteration's words)
        c->win_lv_offp = dalloc<uint32_t>(c, W * LV_OFFP);
    }
    if (F.walk_slots) {   // the lean key walk's slots, written by the accept step
        for (int b = 0; b < 2; ++b) c->slot8_buf[b] = dalloc<uint2>(c, N + 4 + 128);
        P.slot8 = c->slot8_buf[0];
        P.walk_flags = dalloc<uint32_t>(c, 4);
        HIPCHK(hipMemset(P.walk_flags, 0, 16));
    }
    if (F.cone_big || F.persist_sh_big) c->cb_scratch = dalloc<uint32_t>(c, W * cone_big_scratch_words(P.Ng, P.plan_K));
    if (c->plan_beside) {   // the LDS plan's second set of tables (the first: the window's own): twice the plan tables' memory, nothing else
        HIPCHK(hipStreamCreateWithFlags(&c->pstream, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&c->ev_free, hipEventDisableTiming));
        static_cast<LevelTables&>(c->ps[0]) = c->win;
        c->ps[0].plan = c->win_plan; c->ps[0].plan_mi = c->win_plan_mi; c->ps[0].lv_pairs_p = c->win_lv_pairs_p; c->ps[0].lv_offp = c->win_lv_offp;
        alloc_level_tables(c, c->ps[1], false, (size_t)F.cone_tiles, F.cone_gather);
        c->ps[1].plan = dalloc<unsigned long long>(c, W * K);
        c->ps[1].plan_mi = dalloc<double>(c, W * K);
        if (F.lean_plan) {
            c->ps[1].lv_pairs_p = dalloc<uint32_t>(c, W * P.plan_Kp + 512);
            c->ps[1].lv_offp = dalloc<uint32_t>(c, W * LV_OFFP);
        }
        for (Ctx::PlanSet& S : c->ps) HIPCHK(hipEventCreateWithFlags(&S.done, hipEventDisableTiming));
    }
    if (F.plan_ahead) {   // the big plan's second set of tables (the first: the window's own)
        HIPCHK(hipStreamCreateWithFlags(&c->pstream, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&c->ev_free, hipEventDisableTiming));
        static_cast<LevelTables&>(c->ps[0]) = c->win;
        alloc_level_tables(c, c->ps[1], true, (size_t)F.cone_tiles, true);
        for (Ctx::PlanSet& S : c->ps) {
            HIPCHK(hipHostMalloc((void**)&S.ok_host, W * 4, hipHostMallocDefault));
            HIPCHK(hipEventCreateWithFlags(&S.done, hipEventDisableTiming));
        }
    }
}

// chain state and records (BGPChain ctor, AlgoBGP.jl:78-109), the exchange's arrays, the history's fill (NaN values, curr/best = Inf, best_id = -1) and the error word
void init_state(Ctx* c, const smm_bgp_opts_t* opts) {
    KParams& P = c->P;
    const int N = P.N, Ng = P.Ng, T = P.T;
    std::vector<double> cs((size_t)N * CSW, 0.0);
    for (int i = 0; i < N; ++i) {
        double* b = cs.data() + (size_t)i * CSW;
        b[CS_SIGMA] = opts->sigma[opts->chain_offset + i];
        b[CS_BEST] = INFINITY; b[CS_BESTID] = -1.0; b[CS_BESTP] = INFINITY; b[CS_BESTPID] = -1.0;
        b[CS_ATUN] = opts->acc_tuner[opts->chain_offset + i];
    }
    P.cs = dupload(c, cs.data(), cs.size());
    std::vector<double> rec((size_t)N * P.RW, 0.0);
    for (int i = 0; i < N; ++i) rec[(size_t)i * P.RW] = INFINITY;  // value: Inf until the first accept
    for (int b = 0; b < 2; ++b) c->rec[b] = dupload(c, rec.data(), rec.size());
    P.xres = dalloc<unsigned long long>(c, Ng);
    if (N > 0 && Ng % N == 0 && opts->chain_offset % N == 0) {   // equal shards: the values form of the sharded exchange is available
        c->a2a_G = Ng / N;
        c->a2a_cap = c->H.a2a_cap ? c->H.a2a_cap : a2a_capacity(N, c->a2a_G);
        c->a2a_send_idx = dalloc<int32_t>(c, (size_t)c->a2a_G * c->a2a_cap);
        c->a2a_send_cnt = dalloc<int32_t>(c, (size_t)c->a2a_G);
        c->a2a_rowidx = dalloc<int32_t>(c, (size_t)N);
    }
    for (int b = 0; b < 2; ++b) c->vals_buf[b] = dalloc<double>(c, (size_t)N + 4);   // (+4: read as 16-byte pieces)
    P.vals = c->vals_buf[0];
    if (c->F.plan != PLAN_LDS) {
        const int Kmax = std::max(P.plan_K, 1);
        P.xval = dalloc<double>(c, Ng); P.xnext = dalloc<int32_t>(c, Ng); P.xpairs = dalloc<int32_t>(c, (size_t)Kmax * 2);
        P.xsrc = dalloc<int32_t>(c, Ng); P.xpartner = dalloc<int32_t>(c, Ng);
        P.xslot = dalloc<double>(c, (size_t)Ng * 2);
    }
    std::vector<double> row((size_t)N * P.HW, NAN);
    for (int i = 0; i < N; ++i) history_head(row.data() + (size_t)i * P.HW, NAN, NAN, INFINITY, INFINITY, -1.0, 0.0, 0.0, 0.0);
    P.hrec = dalloc<double>(c, (size_t)T * N * P.HW);
    // (one row from the host, then doubling copies on the device: a long history is filled at HBM speed instead of row by row over PCIe)
    HIPCHK(hipMemcpy(P.hrec, row.data(), row.size() * 8, hipMemcpyHostToDevice));
    for (size_t have = 1; have < (size_t)T; have *= 2) {
        const size_t n = std::min(have, (size_t)T - have);
        HIPCHK(hipMemcpy(P.hrec + have * N * P.HW, P.hrec, n * N * P.HW * 8, hipMemcpyDeviceToDevice));
    }
    P.err = dalloc<unsigned long long>(c, 1);
    const unsigned long long e = ERR_NONE;
    HIPCHK(hipMemcpy(P.err, &e, 8, hipMemcpyHostToDevice));
}

// the dynamic LDS every kernel of this context may ask for beyond the default 64 KiB
void lds_limits(Ctx* c) {
    const Forms& F = c->F;
    const bool on[] = {F.plan == PLAN_BIG, F.xk == XK_ROWS || F.xk == XK_KEY, F.plan == PLAN_LDS, F.cone_big};   // (by ExchGroup: the rows of exch_instance's table this context's forms include)
    for (int id = 0; id < XI_COUNT; ++id) {
        const ExchInstance I = exch_instance(id, c->P.Ng);
        if (I.fn && I.cap && on[I.group]) HIPCHK(hipFuncSetAttribute(I.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)I.cap));
    }
    for (int family = 0; family < EF_COUNT; ++family)   // (every row of eval_instance)
        for (int kind = 0; kind < 3; ++kind) HIPCHK(hipFuncSetAttribute(eval_instance(family, kind).fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_CU));
    // (every kernel chain_kernel / chain_kernel_p2p can pick: what chain_instance names)
    for (int family = 0; family < CF_COUNT; ++family)
        for (int np = 1; np <= 4; ++np)
            for (int b = 0; b < 2; ++b) HIPCHK(hipFuncSetAttribute(chain_instance(family, np, b != 0).fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_CU));
    if (tile_smem(c, F, is_sim(c->obj) ? F.ct : (c->obj == SMM_OBJ_DENSE ? 16 : 8)) > LDS_CU) throw std::string("tile does not fit the 160 KiB LDS");
}

#ifdef SMM_TEST_HOOKS
// smm_describe's text, every field of Forms as name=value, the DeviceFacts they were chosen with (smm_debug_forms)
std::string forms_line(const Ctx* c, const DeviceFacts& dev) {
    std::string s = describe_text(c);
    const Forms& F = c->F;
    auto add = [&s](const char* name, long long v) { s += std::string(" ") + name + "=" + std::to_string(v); };
#define FIELD(f) add("F." #f, (long long)F.f)
    FIELD(plan); FIELD(xk); FIELD(rows_cap); FIELD(lean_plan); FIELD(lean_wide); FIELD(plan_ahead); FIELD(win_cap); FIELD(plan_cap);
    FIELD(ct); FIELD(norm_fast); FIELD(norm_narrow); FIELD(tpw); FIELD(tile_off);
    FIELD(inline_walk); FIELD(gen_lean); FIELD(gen_keys); FIELD(dense_keys); FIELD(cone); FIELD(cone_big); FIELD(walk_slots);
    FIELD(cone_tiles); FIELD(cone_ct); FIELD(cone_gather);
    FIELD(persist); FIELD(persist_wide); FIELD(persist_sh); FIELD(persist_sh_big); FIELD(persist_user); FIELD(max_tiles); FIELD(defer_resolve);
#undef FIELD
    add("n_cus", dev.n_cus); add("per_cu", dev.per_cu);
    return s;
}
#endif

}  // namespace

extern "C" {

void smm_ctx_destroy(void* ctx) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->pstream) { (void)hipStreamSynchronize(c->pstream); (void)hipStreamDestroy(c->pstream); }
    if (c->ev_free) (void)hipEventDestroy(c->ev_free);
    for (Ctx::PlanSet& S : c->ps) { if (S.done) (void)hipEventDestroy(S.done); if (S.ok_host) (void)hipHostFree(S.ok_host); }
    for (void* p : c->allocs) (void)hipFree(p);
    for (void* w : c->p2p_opened) if (w) (void)hipIpcCloseMemHandle(w);
    if (c->p2p_mine) (void)hipFree(c->p2p_mine);
    if (c->st_scr) (void)hipFree(c->st_scr);
    if (c->red_res) (void)hipFree(c->red_res);
    if (c->umod) (void)hipModuleUnload(c->umod);
    if (c->pmod) (void)hipModuleUnload(c->pmod);
    for (const auto& tm : c->tmods) (void)hipModuleUnload(tm.second);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    for (hipEvent_t e : c->pev) (void)hipEventDestroy(e);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int smm_ctx_create(const smm_problem_t* prob, const smm_bgp_opts_t* opts, const smm_tables_t* tab, void** out) {
    if (const int rc = check_create_args(prob, opts, tab, out)) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(nullptr, SMM_ERR_NO_DEVICE, "no HIP device available: libsmmhip has no CPU fallback");
    if (opts->device < 0 || opts->device >= ndev) return fail(nullptr, SMM_ERR_INVALID_ARG, "bad device ordinal");
    Ctx* c = new Ctx();
    try {
        c->H = read_hooks();
        if (const char* why = create_facts(c, prob, opts, tab)) throw std::string(why);
        upload_inputs(c, prob, opts, tab);
        choose_forms(c, prob->objective_id);
        choose_plan_beside(c);
        alloc_windows(c);
        init_state(c, opts);
        if (c->F.persist != PERSIST_NONE) alloc_persist(c);
        lds_limits(c);
        reducer_kernel_attributes();
        HIPCHK(hipDeviceSynchronize());
    } catch (const std::string& m) {
        g_create_err = m;
        smm_ctx_destroy(c);
        return SMM_ERR_HIP;
    }
    *out = c;
    return SMM_OK;
}

int smm_describe(void* ctx, char* out, int32_t cap) {
    Ctx* c = (Ctx*)ctx;
    if (!c || !out || cap < 1) return SMM_ERR_INVALID_ARG;
    snprintf(out, (size_t)cap, "%s", describe_text(c).c_str());
    return SMM_OK;
}

#ifdef SMM_TEST_HOOKS
// debug (test build only, not part of the public header): the forms as one line (forms_line).  Of a live context: its own, with the
// DeviceFacts it was created with.  With ctx == NULL, touching no device: what creation would choose for prob / opts / tab on a device of
// n_cus compute units that holds per_cu workgroups of the candidate persistent kernel per unit (-1: one pass of select_forms, the
// occupancy never asked) — check_create_args, create_facts, choose_forms with the occupancy as given
int smm_debug_forms(void* ctx, const smm_problem_t* prob, const smm_bgp_opts_t* opts, const smm_tables_t* tab, int n_cus, int per_cu, char* out, int cap) {
    if (!out || cap < 1) return SMM_ERR_INVALID_ARG;
    std::string line;
    if (ctx) {
        const Ctx* c = (Ctx*)ctx;
        line = forms_line(c, c->dev);
    } else {
        void* none = nullptr;
        if (const int rc = check_create_args(prob, opts, tab, &none)) return rc;
        Ctx c;
        c.H = read_hooks();
        if (const char* why = create_facts(&c, prob, opts, tab)) return fail(nullptr, SMM_ERR_HIP, why);
        c.dev = DeviceFacts{n_cus, -1};
        choose_forms(&c, 0, false, per_cu);
        line = forms_line(&c, c.dev);
    }
    snprintf(out, (size_t)cap, "%s", line.c_str());
    return SMM_OK;
}
#endif

}  // extern "C"
