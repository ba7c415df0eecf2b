// which forms a context runs and the LDS they take, without a HIP call (included once by smmhip.hip; DESIGN.md, "The forms and context creation")
#pragma once

namespace {

constexpr size_t LDS_CU = (size_t)160 * 1024;   // the LDS of a compute unit: what one workgroup can be given
constexpr size_t LDS_HALF = LDS_CU / 2;         // ... and what each of two workgroups that share the unit can
// the objective as the LDS layouts see it: 3 = the dense objective's spec v2 (SMM_OBJ_DENSE2), 4 = a user objective in its map-reduce form
int lay_kind(const Ctx* c) { const int k = obj_kind(c->obj); return k == 2 && c->dense2 ? 3 : (c->obj == SMM_OBJ_USER && c->u_lanes > 0) ? 4 : k; }
size_t tile_smem_base(const Ctx* c, int ct) { return tile_smem_doubles(ct, c->P.np, c->P.nm, c->P.RW, c->P.HW, c->P.RBW, lay_kind(c)) * sizeof(double); }
// dynamic LDS of k_chain_persist_tile for this context (a user objective's wave totals: 16 chains x lanes / 64 groups x its sums)
size_t persist_tile_smem(const Ctx* c) {
    const KParams& P = c->P;
    return pt_layout(P.np, P.nm, P.RW, P.HW, P.RBW, lay_kind(c), P.dense_nOt, PT_CT * (c->u_lanes / 64) * c->u_nsums).total;
}
// ... of k_chain_persist_gen (user: compiled with a user's objective inside)
size_t persist_gen_smem(const Ctx* c, bool user) { return persist_gen_smem_bytes(c->P.Ng, c->P.np, c->P.RW, c->P.HW) + (user ? persist_gen_user_bytes() : 0); }
// tiles (workgroups) of one rank's launch of F's persistent kernel: gen has PG_CT chains per tile (whole tiles), loc NORM_CT, tile PT_CT
int persist_tiles_rank(const Forms& F, int N) {
    const int ct = F.persist == PERSIST_TILE ? PT_CT : NORM_CT;
    return F.persist == PERSIST_GEN ? N / PG_CT : (N + ct - 1) / ct;
}
size_t key_slot_bytes(int Ng) { return LeanLayout<LEAN_KEYS>::slot_bytes(Ng); }   // the key walk's 8-byte chain slots
size_t lean_bytes(int Ng, int K, bool wide) { return wide ? LeanLayout<LEAN_WIDE>::bytes(Ng, K) : LeanLayout<LEAN_KEYS>::bytes(Ng, K); }   // slots and padded pair list of a lean walk
// what k_chain_iter_norm keeps in front of its tile for the inline walk: pair list NOT overlaid; room for either walk (16-byte slots, or the lean walk)
size_t norm_walk_bytes(int Ng, int K, bool wide) {
    return std::max(walk_slot_bytes(Ng) + (((size_t)K * 4 + 15) & ~(size_t)15), (lean_bytes(Ng, K, wide) + 15) & ~(size_t)15);
}
size_t norm_smem(const Ctx* c, const Forms& F) {   // k_chain_iter_norm: [walk: chain slots | pair list] theta, partial sums, parked state
    const size_t b = (size_t)F.tile_off * sizeof(double) + norm_tile_doubles(c->P.np) * sizeof(double);
    return F.cone_big ? std::max(b, cone_local_lds_bytes()) : b;   // (the local cone walk lies UNDER the tile's blocks)
}
size_t tile_smem(const Ctx* c, const Forms& F, int ct, int tpw = 1) {   // dynamic LDS of k_chain_iter: tpw tiles; with the inline exchange
    if (F.norm_fast) return norm_smem(c, F);
    const size_t base = tile_smem_base(c, ct);           // walk its chain slots in front and its pair list under the tiles
    const size_t tiles = (size_t)tpw * ((base + 15) & ~(size_t)15), Kp4 = (size_t)lean_walk_Kp(c->P.plan_K) * 4;
    if (!F.inline_walk) return tiles;
    if (F.dense_keys) return std::max(tiles, key_slot_bytes(c->P.Ng) + std::max((size_t)CONE_LEVELS * 64 * 4, Kp4));
    if (F.gen_keys) return key_slot_bytes(c->P.Ng) + std::max(tiles, Kp4);
    return F.gen_lean ? LeanLayout<LEAN_TILE16>::slot_bytes(c->P.Ng) + std::max(tiles, Kp4) : walk_slot_bytes(c->P.Ng) + std::max(tiles, (size_t)c->P.plan_K * 4);
}
size_t cone_chains_lds_bytes(int Ng) { return (size_t)Ng * 4; }   // k_cone_chains: a word per chain
size_t plan_lds_bytes(int Ng, int K) { return (size_t)(Ng + 2) * 4 + (size_t)K * 8 + (size_t)K * 4 + 128 + 16; }
size_t resolve_lds_bytes(int Ng) { return (size_t)Ng * 16 + 16; }   // (the ticket kernel: test build only)
size_t resolve_lvl_soa_bytes(int Ng, int K) { return (size_t)Ng * 12 + (size_t)K * 4 + 16; }
size_t resolve_lvl_bytes(int Ng, int K) { return (size_t)Ng * 16 + (size_t)K * 12 + 64 * 8 + 64; }
size_t resolve_lean_bytes(int Ng, int K, bool wide) { return std::max(lean_bytes(Ng, K, wide), resolve_lvl_soa_bytes(Ng, K)); }
// the rules select_forms states once
bool one_threshold(const KParams& P) { return P.mi_uniform && !(P.mi_value < 0.0); }   // one threshold >= 0 (or NaN: nothing ever swaps) for all chains
bool one_threshold_nonzero(const KParams& P) { return one_threshold(P) && P.mi_value != 0.0; }   // ... and not 0: the walks on 16-byte slots of values
bool loc_shape(const Forms& F, const KParams& P) { return F.norm_fast && P.np <= 2 && P.ns <= WG * PR_ZR; }   // what k_chain_persist_loc simulates
// this context is one of several shards of one size, of a run the p2p windows can hold
bool equal_shards(const KParams& P) { return P.N < P.Ng && P.N > 0 && P.Ng % P.N == 0 && P.offset % P.N == 0 && P.Ng / P.N <= P2P_MAXG; }
// F without its persistent kernel (what F.max_tiles says stays: how many tiles the device would have held)
void clear_persist(Forms& F) { F.persist = PERSIST_NONE; F.persist_wide = F.persist_sh = F.persist_sh_big = F.persist_user = F.defer_resolve = false; }

// Every form a context runs, from what create_facts made of the arguments, the hooks and the device.  Decides and allocates nothing.  The order of
// preference between the persistent forms: gen -> gen_user -> gen_small / user -> loc / shard -> tile, each only where none before it was taken.
Forms select_forms(const Ctx* c, const Hooks& H, const DeviceFacts& dev) {
    const KParams& P = c->P;
    const int np = P.np, nm = P.nm, N = P.N, Ng = P.Ng, K = P.plan_K, n_cus = dev.n_cus;
    const bool user_obj = c->obj == SMM_OBJ_USER, minus = P.dist_fun == SMM_DIST_MINUS, chol = c->has_chol;
    const bool mi0 = P.mi_uniform && P.mi_value == 0.0;   // one threshold 0 for all chains
    // the lean walk on 16-byte slots of values (one threshold > 0, or thresholds by chain): as far as a CU's LDS reaches (~7400 chains)
    const bool wide_fits = resolve_lean_bytes(Ng, K, true) <= LDS_CU;
    Forms F;
    // the level plan in LDS, or in global memory
    bool lds = Ng > 1 && Ng <= XLDS_MAX && K >= 1 && K <= Ng && !H.any_exchange;
    bool lvl = lds && Ng <= XLVL_MAX && !H.dataflow;
    bool lvl_soa = lds && !lvl && !H.dataflow;
    // (a SHARD of a population past the wide lean walk's LDS, e.g. 2 x 4096 with the default threshold: the big plan lists its tiles' cones for the persistent form)
    const bool shard_wide_big = N < Ng && lds && one_threshold_nonzero(P) && minus && !wide_fits;
    const bool big = Ng > 1 && Ng <= 65535 && K >= 1 && K <= Ng && !H.any_exchange && (H.big_exchange || shard_wide_big || !lds);
    if (big) lds = lvl = lvl_soa = false;
    const bool key = big && Ng <= XKEY_MAX && K <= XKEY_MAX && !H.key_exchange_off && minus;   // (the keys order value_i - value_j)
    F.plan = big ? PLAN_BIG : lds ? PLAN_LDS : PLAN_NONE;
    const int tile_ct = is_sim(c->obj) ? F.ct : (c->obj == SMM_OBJ_DENSE ? 16 : 8);
    F.norm_fast = is_sim(c->obj) && np == nm && np <= 4 && P.batch_size == np && P.dbg == 0 && !chol && !H.norm_fast_off;
    // more tiles than CUs: the walk-free kernel on half-size workgroups, two to a CU (k_chain_iter_norm_narrow)
    F.norm_narrow = F.norm_fast && ((N + NORM_CT - 1) / NORM_CT > n_cus || H.norm_narrow == 1) && H.norm_narrow != 0;
    // the inline exchange walk.  A candidate is F with the walk on (front: bytes of LDS in front of the tile), admitted where its launch's tile_smem fits
    auto walking = [&F](bool keys, bool under, bool lean, int tpw, size_t front) {
        Forms G = F; G.inline_walk = true; G.gen_keys = keys; G.dense_keys = under; G.gen_lean = lean; G.tpw = tpw; G.tile_off = (int)(front / sizeof(double));
        return G;
    };
    // single shard, level plan: k_chain_iter_norm with the walk in front of its tile (for `-`), k_chain_iter with the slots in front, the list under
    const Forms walk = walking(false, false, false, 1, F.norm_fast ? norm_walk_bytes(Ng, K, one_threshold_nonzero(P)) : walk_slot_bytes(Ng));
    if (!H.inline_walk_off && lvl && N == Ng && !user_obj && (!F.norm_fast || minus) && tile_smem(c, walk, tile_ct) <= (F.norm_fast ? LDS_CU : LDS_HALF)) F = walk;
    // two tiles per workgroup share one walk (the 8-chain simulation tile only), where two tiles would share a CU anyway
    F.tpw = (F.inline_walk && !F.norm_fast && (is_sim(c->obj) ? F.ct == 8 : c->obj != SMM_OBJ_DENSE) && ((N + 7) / 8 > n_cus || H.tpw == 2) &&
             H.tpw != 1 && tile_smem(c, F, tile_ct, 2) <= LDS_CU) ? 2 : 1;
    // k_chain_iter on the lean walk (16-byte slots, padded pair list) where its somewhat larger LDS keeps the same budget
    const Forms lean = walking(false, false, true, F.tpw, LeanLayout<LEAN_TILE16>::slot_bytes(Ng));
    if (F.inline_walk && !F.norm_fast && one_threshold(P) && minus && K <= XLDS_MAX && !H.key_walk_off && (mi0 || wide_fits) &&
        tile_smem(c, lean, tile_ct, F.tpw) <= (F.tpw == 2 ? LDS_CU : LDS_HALF)) F = lean;
    // single shards of 4096 < N <= 8192 chains without a simulation (C4): the key walk inline, two 16-chain tiles per workgroup
    const Forms keys = walking(true, false, false, 2, key_slot_bytes(Ng));
    if (!F.inline_walk && !H.inline_walk_off && obj_kind(c->obj) == 0 && !user_obj && N == Ng && Ng > XLVL_MAX && Ng <= XLDS_MAX && K <= XLDS_MAX &&
        lds && mi0 && minus && !H.key_walk_off && tile_smem(c, keys, 16, 2) <= LDS_CU) F = keys;
    // the dense objective (C5): its tile fills a CU's LDS, so the key walk's slots and lists lie UNDER the tile's blocks
    const Forms under = walking(true, true, false, 1, 0);
    if (!F.inline_walk && !H.inline_walk_off && !H.dense_keys_off && c->obj == SMM_OBJ_DENSE && N == Ng && Ng >= 2 && Ng <= XLVL_MAX && K <= XLVL_MAX &&
        lds && mi0 && minus && !H.key_walk_off && LeanLayout<LEAN_KEYS>::unit(Ng) == 8 && tile_smem(c, under, 16, 1) <= LDS_CU) F = under;
    // the candidates for the cone tables and the persistent kernels.  The workgroups' cones of the inline key walk (smm_cone.hpp):
    const bool want_cone = F.gen_keys && !H.no_cone && (F.dense_keys ? (N % 16 == 0 && N / 16 <= 256) : (F.tpw == 2 && N % 32 == 0 && N / 32 <= 256));
    const int cone_ct = F.dense_keys ? 16 : 32;
    const bool persist_ok = !c->deep_plan && P.dbg == 0 && !H.persist_off;
    const bool gen_ok = np <= PG_MAXP && nm <= PG_MAXP && P.batch_size == np && !chol && N == Ng && persist_ok;
    const bool gen_fits = persist_gen_smem(c, false) <= LDS_CU;
    // k_chain_persist_gen: where k_chain_iter walks its workgroups' cones inline (whole workgroups of 32, one per CU), one batch, isotropic
    const bool want_gen = want_cone && !F.dense_keys && c->obj == SMM_OBJ_BANANA && gen_ok && N / PG_CT <= n_cus && gen_fits;
    // ... and for smaller populations of the same objective (whole groups of 32): the cones are listed behind the lean plan either way
    const bool gen_small_ok = gen_ok && N % PG_CT == 0 && N / PG_CT >= 1 && N / PG_CT <= n_cus && lds && mi0 && minus && K <= XLDS_MAX;
    const bool want_gen_small = !want_cone && c->obj == SMM_OBJ_BANANA && F.inline_walk && gen_small_ok && gen_fits;
    // ... and a USER objective (one thread per evaluation) in the same loop, compiled with the user's source inside (user_form_compile)
    const bool want_user = user_obj && c->u_lanes == 0 && gen_small_ok && persist_gen_smem(c, true) <= LDS_CU;
    // ... and on LOCALLY NUMBERED cones (smm_chain_persist_loc.hpp): objfunc_norm of the loc shape, thresholds >= 0 (or NaN), any population size
    const bool mi_ok = one_threshold(P) || P.mi_pct;   // one threshold >= 0 (or NaN) for all chains, or one per chain, each >= 0 (or NaN)
    const bool loc_ok = loc_shape(F, P) && minus && persist_ok && !H.persist_loc_off;
    const bool want_loc = loc_ok && N == Ng && Ng >= 2 && F.inline_walk && mi_ok && K <= XLDS_MAX && Ng <= XLDS_MAX && (N + NORM_CT - 1) / NORM_CT <= n_cus;
    // ... and as a shard of a sharded run (one process per GPU: smm_bgp_p2p_step): the same kernel, the ring in the ranks' windows
    const bool want_sh = loc_ok && equal_shards(P) && N % NORM_CT == 0 && one_threshold(P) && N / NORM_CT <= n_cus &&
                         (lds ? K <= XLDS_MAX : (big && Ng <= 32768 && K <= 65535 && cone_chains_lds_bytes(Ng) <= LDS_CU));
    // ... and for the objectives a whole tile evaluates (smm_chain_persist_tile.hpp): any objfunc_norm, the dense simulation; one 16-chain tile per workgroup, all resident
    const int tile_kind = obj_kind(c->obj);
    // ... and a USER objective in its map-reduce form (smm_register_user_objective_lanes) whose lanes are a whole share of the tile's 512
    const bool user_tile = user_obj && c->u_lanes > 0 && c->u_lanes <= WG && WG % c->u_lanes == 0 && PT_CT % (WG / c->u_lanes) == 0 && !P.mi_pct;   // (compiled for ONE threshold)
    const bool tile_ok = (tile_kind == 1 || tile_kind == 2 || user_tile) && !loc_shape(F, P) && lds && minus && K <= XLDS_MAX && Ng <= XLDS_MAX &&
                         persist_ok && !H.persist_tile_off && P.RW <= PT_LPC * PT_NJ && persist_tile_smem(c) <= LDS_CU;
    const bool want_tile = tile_ok && N == Ng && Ng >= 2 && mi_ok && (tile_kind != 2 || N % PT_CT == 0) && (N + PT_CT - 1) / PT_CT <= 2 * n_cus;
    // ... and as a shard (SH of smm_chain_persist_tile.hpp): equal shards of whole tiles, the LDS plan, one threshold >= 0 (or NaN)
    const bool want_tile_sh = tile_ok && equal_shards(P) && N % PT_CT == 0 && one_threshold(P) && !P.mi_pct && !chol && N / PT_CT <= 2 * n_cus;
    const size_t persist_tiles = (want_gen || want_gen_small || want_user) ? (size_t)N / PG_CT : (size_t)(N + NORM_CT - 1) / NORM_CT;
    // large single shards of objfunc_norm (C3 on one GPU): the narrow kernel's tiles walk their own, locally numbered cones (smm_cone_big.hpp)
    const bool rows = key && mi0 && !H.key_walk_off;
    const bool want_cone_big = big && rows && F.norm_fast && F.norm_narrow && N == Ng && N % NORM_CT == 0 && Ng <= 32768 && K <= 65535 &&
                               P.dbg == 0 && !H.cone_big_off && cone_chains_lds_bytes(Ng) <= LDS_CU;
    // look-ahead windows, at most 256 iterations each, with budgets of their own; the plan's counts the tables of every candidate, taken or not, one line each
    const bool pregen = !(F.norm_fast && !c->has_ntab && !c->has_utab);   // (k_chain_iter_norm draws in the kernel)
    const size_t rb_iter = (size_t)P.RBW * N * 8;
    const size_t cone_iter = (size_t)(CONE_LEVELS * 64 + CONE_HDRW) * 4;   // one tile's header and sub-levels
    const size_t cone_gather_iter = cone_iter + CONE_GCAP * 2;              // ... with its gather list
    size_t plan_iter = 0;   // bytes per iteration of the plan window
    plan_iter += (size_t)K * 36;                                                                            // win_plan, win_plan_mi, win_lv_pairs, win_lv_mi, win_lv_off: 32 bytes a pair, and 4 to spare
    plan_iter += (size_t)lean_walk_Kp(K) * 4 + 1024;                                                        // win_lv_pairs_p, win_lv_offp
    if (big) plan_iter += BigPlanScratch::words(Ng, K) * 4;                                                 // big_scratch
    if (big) plan_iter += (size_t)(XROWS_MAX + 1) * XWG * 4;                                                // win_lv_rows, win_lv_rowinfo
    if (want_cone_big) plan_iter += (size_t)(N / NORM_CT) * cone_gather_iter;                               // cone tables: the local cones'
    if (want_cone_big) plan_iter += cone_big_scratch_words(Ng, K) * 4;                                      // cb_scratch: for the local cones
    if (want_sh && big) plan_iter += cone_big_scratch_words(Ng, K) * 4;                                     // cb_scratch: for a shard's cones behind the big plan
    if (want_cone) plan_iter += (size_t)(N / cone_ct) * cone_iter + 4;                                      // cone tables: the inline key walk's
    if (want_loc || want_sh || want_tile || want_tile_sh) plan_iter += persist_tiles * cone_gather_iter + 4;   // cone tables: the loc and tile forms'
    if (want_gen) plan_iter += persist_tiles * (CONE_GCAP * 2);                                             // cone_gather beside the inline key walk's cones: the gen form's
    if (want_gen_small || want_user) plan_iter += persist_tiles * cone_gather_iter + 4;                     // cone tables: the small gen form's
    F.win_cap = pregen ? (int)std::max<size_t>(1, std::min<size_t>(256, ((size_t)768 << 20) / rb_iter)) : 1;
    F.win_cap = std::min(F.win_cap, P.T);
    // (one set of tables is counted: a context that plans beside its persistent kernel — choose_plan_beside, smm_create_host.hpp — allocates a second set
    // of the LDS plan's, so up to twice this budget; at 4096 chains 2 x 0.65 GB, and the window stays at its 256 iterations)
    F.plan_cap = (int)std::max<size_t>(1, std::min<size_t>(256, ((size_t)1536 << 20) / plan_iter));
    F.plan_cap = std::max(1, std::min(std::min(F.plan_cap, P.T), H.plan_cap));
    // the exchange: the big plan's forms
    if (big && rows) {
        F.rows_cap = std::min(XROWS_MAX, (K + XWG - 1) / XWG + LV_MAXLEV);
        if (want_cone_big) { F.cone_big = true; F.plan_ahead = !H.plan_ahead_off; F.walk_slots = true; }
    }
    if (big && want_sh) {   // a shard of a large population: its own tiles' cones, locally numbered (smm_cone_big.hpp)
        F.persist = PERSIST_LOC; F.persist_wide = P.mi_value != 0.0; F.persist_sh = true; F.persist_sh_big = true;
    }
    // ... the lean walk behind the LDS plan: one threshold 0 (8-byte keys) or > 0 / NaN (16-byte values, while wide_fits); by chain: the lean PLAN only, for the persistent launches
    const bool wide = one_threshold_nonzero(P) && wide_fits;
    const bool pct = P.mi_pct != 0 && (want_loc || want_tile);
    F.lean_plan = lds && (mi0 || wide || pct) && K <= XLDS_MAX && !H.key_walk_off && minus;
    F.lean_wide = F.lean_plan && (wide || pct);
    if (F.lean_plan) {
        // ... walked in the prologue of k_chain_iter_norm, or of k_chain_iter (key form)
        if (mi0 && ((F.norm_fast && F.inline_walk && Ng <= XLVL_MAX && K <= XLVL_MAX) || F.gen_keys)) {
            F.walk_slots = true;
            F.cone = want_cone;
            if (want_gen) F.persist = PERSIST_GEN;
        }
        const bool user_ok = want_user && mi0 && F.persist == PERSIST_NONE;
        if ((want_gen_small || user_ok) && mi0 && F.persist == PERSIST_NONE) {
            F.persist = PERSIST_GEN; F.persist_user = user_ok; F.defer_resolve = user_ok;
        }
        if ((want_loc || want_sh) && F.persist == PERSIST_NONE && F.norm_fast) {   // (k_exch_plan lists the tiles' cones behind the lean plan)
            F.persist = PERSIST_LOC; F.persist_wide = wide || pct; F.persist_sh = want_sh;
        }
        // (the dense tiles of the per-iteration kernel walk the same cones: want_cone above)
        if (want_tile && F.persist == PERSIST_NONE &&
            (!F.cone || (cone_ct == PT_CT && (size_t)(N / cone_ct) == (size_t)(N + PT_CT - 1) / PT_CT))) {
            F.persist = PERSIST_TILE; F.persist_wide = true;
            F.defer_resolve = !F.inline_walk;   // (the exchange of an iteration is left to the next launch: it may be this kernel's)
        }
        if (want_tile_sh && F.persist == PERSIST_NONE) { F.persist = PERSIST_TILE; F.persist_wide = true; F.persist_sh = true; }
    }
    // ... all of its tiles resident at once, or it is not taken (per_cu 0 also where a user objective's kernel did not compile)
    if (F.persist != PERSIST_NONE && dev.per_cu >= 0) {
        if (F.persist != PERSIST_GEN) F.max_tiles = dev.per_cu * n_cus;
        if (persist_tiles_rank(F, N) > dev.per_cu * n_cus) clear_persist(F);
    }
    // the cone tables: the persistent form's (with gather lists), the local cones', or the inline key walk's
    if (F.cone_big) { F.cone_tiles = N / NORM_CT; F.cone_ct = NORM_CT; F.cone_gather = true; }
    else if (F.persist == PERSIST_GEN) { F.cone_tiles = N / PG_CT; F.cone_ct = PG_CT; F.cone_gather = true; }
    else if (F.persist == PERSIST_LOC) { F.cone_tiles = (int)persist_tiles; F.cone_ct = NORM_CT; F.cone_gather = true; }
    else if (F.persist == PERSIST_TILE) { F.cone_tiles = (N + PT_CT - 1) / PT_CT; F.cone_ct = PT_CT; F.cone_gather = true; }
    else if (F.cone) { F.cone_tiles = N / cone_ct; F.cone_ct = cone_ct; }
    // the stand-alone resolution
    F.xk = (F.lean_plan && !pct) ? XK_LEAN : lvl ? XK_LVL : lvl_soa ? XK_LVL_SOA : lds ? XK_TICKETS   // (XK_TICKETS: test build only, SMMHIP_DATAFLOW_EXCHANGE)
         : key ? (rows ? XK_ROWS : XK_KEY) : big ? XK_LVL_BIG : XK_ANY;
    return F;
}

// (the choosers and the exchange's table: smm_launch_host.hpp, behind this file)
ChainKernel chain_kernel(const Ctx* c, int flags); PersistKernel persist_kernel(const Ctx* c, const Forms& F); ExchLaunch resolve_kernel(const Ctx* c, const KParams& P); ExchInstance exch_instance(int id, int Ng);
// which forms this context was given at creation (one line; tests/test_gpu_forms.py pins the table)
std::string describe_text(const Ctx* c) {
    const KParams& P = c->P;
    const Forms& F = c->F;
    // the kernel of the iterations that walk inline where a kernel is made for them (narrow_cone, any, wide), else the others' ("iter_norm" or the narrow one)
    const bool walks = F.inline_walk || F.cone_big;
    ChainKernel chain = chain_kernel(c, walks ? F_WALK_INLINE : 0);
    if (walks && !strcmp(chain.name, "iter_norm")) chain = chain_kernel(c, 0);
    const char* walk = F.cone_big ? "cone_local" : !F.inline_walk ? "standalone" : F.dense_keys ? "inline_keys_under_tile" : F.gen_keys ? (F.cone ? "inline_keys_cone" : "inline_keys")
                     : F.norm_fast ? ((P.lean_wide && !P.mi_pct) ? "inline_lean_wide" : (F.lean_plan && !P.mi_pct) ? "inline_lean" : "inline_slots") : F.gen_lean ? "inline_lean16" : "inline_slots";
    char b[160];
    std::string s = std::string("chain=") + chain.name + " walk=" + walk + " exchange=" + exch_instance(resolve_kernel(c, P).id, 0).name + " persistent=" + persist_kernel(c, F).name +
                    " plan=" + (F.plan == PLAN_BIG ? (F.plan_ahead ? "big_ahead" : "big") : F.plan == PLAN_LDS ? "lds" : "none") + " window=" + std::to_string(F.plan_cap);
    if (c->obj == SMM_OBJ_USER) s += " ct=" + std::to_string(chain.ct);   // (the three launches' tile width)
    // (only once a starting population has been installed: smm_set_population / smm_scatter_population)
    if (c->pop_kind == 1) s += " population=set";
    if (c->pop_kind == 2) { snprintf(b, sizeof b, " population=scatter pop_M=%d pop_spread=%.17g", c->pop_M, c->pop_spread); s += b; }
    return s;
}

}  // namespace
