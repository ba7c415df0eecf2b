// which kernel a launch takes and how it is launched — part of libsmmhip (included once by smmhip.hip, between smm_forms_host.hpp and
// smm_run_host.hpp; hiprtc never sees it): the look-ahead windows (ensure_windows), the four tables that name every instantiation of
// a kernel family a launch can take (chain_instance, eval_instance, exch_instance, persist_instance), the choosers that pick a row and decide nothing
// else (chain_kernel*, resolve_*, persist_kernel), and the launchers.  The tables stand in this order, and their rows in theirs: the
// kernels are emitted, and a few numbered, in the order in which the host code names them.
#pragma once

namespace {

int exchange_K(const Ctx* c) { return c->P.n_pairs_tab > 0 ? c->P.n_pairs_tab : n_exchange_pairs(c->P.Ng); }   // (an injected pair list: its length)
bool exchange_active(const Ctx* c, int t) { return t >= c->exchange_from && c->P.Ng > 1; }  // AlgoBGP.jl:637

ExchInstance exch_instance(int id, int Ng = 0);   // (the table stands behind the chain kernels': the kernels are emitted in the order in which they are named)
// row `id` of that table onto stream st: every launch of the exchange family (args: exactly the kernel's parameter types — they travel as addresses)
template <class... Args>
void launch_exch(Ctx* c, int id, dim3 grid, size_t smem, hipStream_t st, const Args&... args) {
    const ExchInstance I = exch_instance(id);
    if (!I.fn) throw std::string("exchange kernel ") + I.name + " is not part of this build";
    void* a[] = {(void*)&args...};
    launch_fn(c, I.fn, grid, dim3(I.block), smem, st, a, I.stamped);
}
size_t plan_smem(int Ng, int K, bool cones) { return cones ? std::max(plan_lds_bytes(Ng, K), plan_cone_bytes()) : plan_lds_bytes(Ng, K); }   // k_exch_plan's dynamic LDS (cones: it lists the tiles' cones too)
// the big plan of W iterations from t on into the tables L on stream st; cones: and the tiles' locally numbered cones, from the plan's scratch (pairs in list order, their levels)
void launch_plan_big(Ctx* c, const KParams& P, int t, int W, const LevelTables& L, hipStream_t st, bool cones) {
    launch_exch(c, XI_PLAN_BIG, dim3(W), plan_big_lds_bytes(P.Ng), st, P, t, c->big_scratch, L.lv_pairs, L.lv_mi, L.lv_off, L.lv_rows, L.lv_rowinfo);
    if (!cones) return;
    launch_exch(c, XI_CONE_CHAINS, dim3(W), cone_chains_lds_bytes(P.Ng), st, P, (const uint32_t*)L.lv_pairs, (const uint32_t*)L.lv_off, c->cb_scratch);
    const unsigned blocks = ((P.cone_tiles + CONEB_WAVES - 1) / CONEB_WAVES) * ((W + 7) & ~7);
    launch_exch(c, XI_CONE_TILES, dim3(blocks), cone_tiles_lds_bytes(P.plan_K), st, P, W, (const uint32_t*)c->cb_scratch);
}
// P reads the plan window's tables in L: the levels' (with the rows of k_exch_resolve_rows) and the tiles' cones (null where L has none: a
// context's sets all hold the same kinds of table, and its P starts with the cones of its own set, c->win)
void point_tables(KParams& P, const LevelTables& L) {
    P.lv_pairs = L.lv_pairs; P.lv_mi = L.lv_mi; P.lv_off = L.lv_off; P.lv_rows = L.lv_rows; P.lv_rowinfo = L.lv_rowinfo;
    P.cone_ok = L.cone_ok; P.cone_hdr = L.cone_hdr; P.cone_pairs = L.cone_pairs; P.cone_gather = L.cone_gather;
}
// the plan window starting at iteration t into set k, on the plan stream (the kernels' scratch is theirs alone: one window at a time
// there) — behind every launch enqueued on the main stream so far: the ones that read set k are all among them (k is not the active set)
void plan_window_into(Ctx* c, int k, int t) {
    Ctx::PlanSet& S = c->ps[k];
    KParams Pw = c->P;
    HIPCHK(hipEventRecord(c->ev_free, c->stream));
    HIPCHK(hipStreamWaitEvent(c->pstream, c->ev_free, 0));
    point_tables(Pw, S);   // (k_cone_tiles writes the cones where its P says)
    const int W = std::min(c->F.plan_cap, Pw.T - t + 1);
    launch_plan_big(c, Pw, t, W, S, c->pstream, true);
    HIPCHK(hipMemcpyAsync(S.ok_host, S.cone_ok, (size_t)W * 4, hipMemcpyDeviceToHost, c->pstream));
    HIPCHK(hipEventRecord(S.done, c->pstream));
    S.t0 = t; S.w = W;
}

// the same for the LDS plan of a context that plans beside its persistent chain kernel (Ctx::plan_beside): one launch of k_exch_plan_bg, one
// small workgroup per iteration, which the chain kernel's workgroups leave room for on every compute unit (smm_lookahead.hpp).  No copy
// of the cone flags to the host: the persistent kernel looks at them itself, the per-iteration forms never did
void plan_beside_into(Ctx* c, int k, int t) {
    Ctx::PlanSet& S = c->ps[k];
    KParams Pw = c->P;
    HIPCHK(hipEventRecord(c->ev_free, c->stream));
    HIPCHK(hipStreamWaitEvent(c->pstream, c->ev_free, 0));
    point_tables(Pw, S);
    const int W = std::min(c->F.plan_cap, Pw.T - t + 1);
    launch_exch(c, XI_PLAN_BG, dim3(W), PBG_LDS, c->pstream, Pw, t, S.plan, S.plan_mi, S.lv_pairs, S.lv_mi, S.lv_off, S.lv_pairs_p, S.lv_offp);
    HIPCHK(hipEventRecord(S.done, c->pstream));
    S.t0 = t; S.w = W;
}

// iteration t lies behind the plan window, the exchange of t - 1 is still to be walked: does the window planned ahead hold both?
bool plan_ahead_covers(const Ctx* c, int t) {
    const Ctx::PlanSet& S = c->ps[c->ps_act ^ 1];
    return c->F.plan_ahead && S.w >= 2 && S.t0 == t - 1;
}

// make the look-ahead tables cover iteration t (1-based): a new window simply starts at t
void ensure_windows(Ctx* c, int t, bool rng = true) {
    KParams& P = c->P;
    // (k_chain_iter_norm generates its randomness itself unless tables are injected: no randomness blocks)
    const bool pregen = rng && !(c->F.norm_fast && !P.user_ntab && !P.user_utab);
    if (pregen && !(t >= c->rng_t0 && t < c->rng_t0 + c->rng_w)) {
        int W = std::min(c->F.win_cap, P.T - t + 1);
        // (k_chain_persist_gen draws in the kernel too: blocks only for the iterations between its launches)
        // — and only where such launches are really being made: a caller that steps one iteration at a time (the reference's run! loop
        // over computeNextIteration!, AlgoAbstract.jl:38-45) never takes the persistent form and keeps its full windows
        if ((c->F.persist == PERSIST_GEN || c->F.persist == PERSIST_TILE) && c->persist_on && !c->persist_broken && !c->in_repair && !P.user_ntab && !P.user_utab &&
            c->persist_launches != c->pregen_seen_launches) W = std::min(W, 2);
        c->pregen_seen_launches = c->persist_launches;
        const size_t Q = (size_t)(P.np + 1) / 2;
        const size_t per_iter = (size_t)P.rb_tries * Q * P.N;   // (< 2^31: checked at creation)
        hipLaunchKernelGGL(k_pregen_rng, dim3((unsigned)((per_iter + 255) / 256), (unsigned)W), dim3(256), 0, c->stream, P, t, W, c->win_rb);
        c->rng_t0 = t; c->rng_w = W;
        P.rb = c->win_rb; P.rb_t0 = t;
    }
    if (c->F.plan_ahead && !(t >= c->plan_t0 && t < c->plan_t0 + c->plan_w)) {
        const int nx = c->ps_act ^ 1;
        Ctx::PlanSet& S = c->ps[nx];
        // (the window planned ahead starts with the LAST iteration of the one before it, so that an exchange of that iteration still
        // to be walked by this launch's tiles finds its cones in the new window: plan_ahead_covers)
        if (!(S.w > 0 && (S.t0 == t || (S.t0 == t - 1 && S.w >= 2)))) plan_window_into(c, nx, t);   // (the first window, a jump: not the window planned ahead)
        HIPCHK(hipEventSynchronize(S.done));                         // the host reads the window's flags (long there when planned ahead)
        HIPCHK(hipStreamWaitEvent(c->stream, S.done, 0));
        c->ps_act = nx; c->plan_t0 = S.t0; c->plan_w = S.w;
        P.plan_t0 = S.t0;
        point_tables(P, S);
        c->cone_big_ok.assign(S.ok_host, S.ok_host + S.w);
        // the next window, into the set the launches enqueued so far read
        c->ps[nx ^ 1].w = 0;
        if (S.t0 + S.w <= P.T) plan_window_into(c, nx ^ 1, S.t0 + S.w - (S.w >= 2 && c->F.plan_cap >= 2 ? 1 : 0));
    }
    if (c->F.plan == PLAN_BIG && !c->F.plan_ahead && !(t >= c->plan_t0 && t < c->plan_t0 + c->plan_w)) {
        const int W = std::min(c->F.plan_cap, P.T - t + 1);
        launch_plan_big(c, P, t, W, c->win, c->stream, c->F.cone_big || c->F.persist_sh_big);
        c->plan_t0 = t; c->plan_w = W;
        P.plan_t0 = t;
        if (c->F.cone_big) {   // (the persistent kernel of a shard looks at the window's flags itself: no synchronisation)
            // a cone that does not fit its caps (a pair list of very deep dependency chains: the user's, or an unlucky sample) sends its
            // iteration to the stand-alone resolution: the host looks at the window's flags once (one synchronisation per window)
            c->cone_big_ok.resize((size_t)W);
            HIPCHK(hipMemcpyAsync(c->cone_big_ok.data(), P.cone_ok, (size_t)W * 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
        }
        point_tables(P, c->win);
    }
    if (c->F.plan == PLAN_LDS && c->plan_beside && P.Ng > 1 && !(t >= c->plan_t0 && t < c->plan_t0 + c->plan_w)) {
        // the window planned beside the chain kernels of the one before it, if it is the one needed (the same rule as the big plans'); else
        // — the first window, a jump, a step pattern that asks for another start — k_exch_plan on the main stream into the active set, as
        // ever.  The host waits for neither: the persistent kernel reads the cone flags itself
        const int nx = c->ps_act ^ 1;
        Ctx::PlanSet& A = c->ps[nx];
        if (A.w > 0 && (A.t0 == t || (A.t0 == t - 1 && A.w >= 2))) {
            HIPCHK(hipStreamWaitEvent(c->stream, A.done, 0));
            c->ps_act = nx;
            ++c->windows_beside;
        } else {
            Ctx::PlanSet& S = c->ps[c->ps_act];
            KParams Pw = P;
            point_tables(Pw, S);
            const int W = std::min(c->F.plan_cap, P.T - t + 1);
            launch_exch(c, XI_PLAN, dim3(W), plan_smem(P.Ng, P.plan_K, true), c->stream, Pw, t, S.plan, S.plan_mi, S.lv_pairs, S.lv_mi, S.lv_off, S.lv_pairs_p, S.lv_offp);
            S.t0 = t; S.w = W;
            ++c->windows_instream;
        }
        Ctx::PlanSet& S = c->ps[c->ps_act];
        c->plan_t0 = S.t0; c->plan_w = S.w;
        P.plan = S.plan; P.plan_mi = S.plan_mi; P.plan_t0 = S.t0;
        point_tables(P, S);
        P.lv_pairs_p = S.lv_pairs_p; P.lv_offp = S.lv_offp;
        // the next window, into the set that the launches enqueued so far read: it starts with the LAST iteration of this one, where the
        // persistent kernel's next launch finds the exchange it left pending (launch_chain_persist)
        c->ps[c->ps_act ^ 1].w = 0;
        if (S.t0 + S.w <= P.T) plan_beside_into(c, c->ps_act ^ 1, S.t0 + S.w - (S.w >= 2 && c->F.plan_cap >= 2 ? 1 : 0));
    } else if (c->F.plan == PLAN_LDS && P.Ng > 1 && !(t >= c->plan_t0 && t < c->plan_t0 + c->plan_w)) {
        const int W = std::min(c->F.plan_cap, P.T - t + 1);
        launch_exch(c, XI_PLAN, dim3(W), plan_smem(P.Ng, P.plan_K, c->F.cone || c->F.persist != PERSIST_NONE), c->stream, P, t, c->win_plan, c->win_plan_mi,
                    c->win.lv_pairs, c->win.lv_mi, c->win.lv_off, c->win_lv_pairs_p, c->win_lv_offp);
        c->plan_t0 = t; c->plan_w = W;
        P.plan = c->win_plan; P.plan_mi = c->win_plan_mi; P.plan_t0 = t;
        point_tables(P, c->win);
        P.lv_pairs_p = c->win_lv_pairs_p; P.lv_offp = c->win_lv_offp;
    }
}

// ---- which per-iteration chain kernel (smm_chain.hpp, smm_chain_norm.hpp) ----
// Every instantiation of the chain kernels' templates that a launch can take is named in chain_instance() and nowhere else: chain_kernel()
// and chain_kernel_p2p() pick one for a launch, smm_ctx_create raises the dynamic LDS limit of every one of them, smm_describe prints the
// pick's name.  A new instantiation is one line in chain_instance() (a new family: one more name in ChainFamily).
enum ChainFamily {
    CF_SIM, CF_SIM_2, CF_DENSE, CF_GEN_KEYS, CF_GEN_64, CF_GEN_2, CF_GEN,   // k_chain_iter<KIND, CT, TPW, b>: b = compiled with the inline walk
    CF_NORM_NARROW_CONE, CF_NORM_ANY, CF_NORM_WIDE, CF_NORM_NARROW,        // k_chain_iter_norm_*<np>
    CF_NORM,                                                               // k_chain_iter_norm<np, b>: b = this launch walks
    CF_P2P_ROWS_NARROW, CF_P2P_ROWS,                                       // k_chain_iter_norm_p2p_rows*<np>
    CF_P2P,                                                                // k_chain_iter_norm_p2p<np, b>: b = staging loops for more than XLVL_MAX chains or pairs
    CF_COUNT
};
// f(std::integral_constant<int, np>) for a parameter count known at run time: 1 .. 4, as the norm kernels are instantiated
template <class F>
const void* by_np(int np, F f) {
    switch (np) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        default: return f(std::integral_constant<int, 4>{});
    }
}
// (np counts for the norm and p2p families only.  The order in which the kernels are named here is the order in which the compiler emits
// them, and the register numbering of a few of them follows it: kept as the launchers named them before there was this table)
ChainKernel chain_instance(int family, int np, bool b) {
#define ITER(KIND, CT, TPW, NAME) \
    ChainKernel{b ? (const void*)k_chain_iter<KIND, CT, TPW, true> : (const void*)k_chain_iter<KIND, CT, TPW, false>, NAME, WG * TPW, CT, TPW}
#define NORM(KERN, NAME, BLOCK) ChainKernel{by_np(np, [](auto NP) { return (const void*)KERN<decltype(NP)::value>; }), NAME, BLOCK, NORM_CT, 1}
#define NORM_B(KERN, NAME) \
    ChainKernel{by_np(np, [b](auto NP) { return !b ? (const void*)KERN<decltype(NP)::value, false> : (const void*)KERN<decltype(NP)::value, true>; }), NAME, NORM_WG, NORM_CT, 1}
    switch (family) {
        case CF_SIM: return ITER(1, 8, 1, "iter<sim,8>");
        case CF_SIM_2: return ITER(1, 8, 2, "iter<sim,8,2>");
        case CF_DENSE: return ITER(2, 16, 1, "iter<dense,16>");
        case CF_GEN_KEYS: return ITER(0, 16, 2, "iter<gen,16,2>");
        case CF_GEN_64: return ITER(0, 64, 1, "iter<gen,8>");   // (smm_describe has always filed the 64-chain tile under the 8-chain tile's name)
        case CF_GEN_2: return ITER(0, 8, 2, "iter<gen,8,2>");
        case CF_GEN: return ITER(0, 8, 1, "iter<gen,8>");
        case CF_NORM_NARROW_CONE: return NORM(k_chain_iter_norm_narrow_cone, "iter_norm_narrow_cone", NORM_WG / 2);
        case CF_NORM_ANY: return NORM(k_chain_iter_norm_any, "iter_norm_any", NORM_WG);
        case CF_NORM_WIDE: return NORM(k_chain_iter_norm_wide, "iter_norm_wide", NORM_WG);
        case CF_NORM_NARROW: return NORM(k_chain_iter_norm_narrow, "iter_norm_narrow", NORM_WG / 2);
        case CF_NORM: return NORM_B(k_chain_iter_norm, "iter_norm");
        case CF_P2P_ROWS_NARROW: return NORM(k_chain_iter_norm_p2p_rows_narrow, "iter_norm_p2p_rows_narrow", NORM_WG / 2);
        case CF_P2P_ROWS: return NORM(k_chain_iter_norm_p2p_rows, "iter_norm_p2p_rows", NORM_WG);
        default: return NORM_B(k_chain_iter_norm_p2p, "iter_norm_p2p");
    }
#undef ITER
#undef NORM
#undef NORM_B
}
// what launch_chain_iter launches for this context as it stands now; flags & F_WALK_INLINE: the launch walks the previous iteration's
// exchange.  Decides only: allocates nothing, launches nothing.
ChainKernel chain_kernel(const Ctx* c, int flags) {
    const KParams& P = c->P;
    const Forms& F = c->F;
    const bool walk = (flags & F_WALK_INLINE) != 0, user = c->obj == SMM_OBJ_USER;
    if (F.norm_fast && !user) {   // k_chain_iter_norm and its variants: one 16-chain tile per workgroup
        // large single shards: every tile walks its own, locally numbered cone (smm_cone_big.hpp)
        if (walk && F.cone_big) return chain_instance(CF_NORM_NARROW_CONE, P.np, false);
        // the lean walks need a padded plan of at most 31 levels and values without NaN: where that is not given — per-chain or
        // negative thresholds (no padded plan), an injected pair list that goes deeper, an uploaded state with NaN values — the
        // kernel with the walk on 16-byte slots {value, src, partner} runs
        // (mi_pct: the lean plan stands for the persistent launches only)
        if (walk && (!F.lean_plan || c->deep_plan || c->nan_values || P.mi_pct)) return chain_instance(CF_NORM_ANY, P.np, false);
        if (walk && P.lean_wide) return chain_instance(CF_NORM_WIDE, P.np, false);   // one min_improve > 0 for all chains: the lean walk on 16-byte slots
        // more than one round of tiles: two half-size workgroups per CU (k_chain_iter_norm_narrow)
        if (!walk && F.norm_narrow) return chain_instance(CF_NORM_NARROW, P.np, false);
        return chain_instance(CF_NORM, P.np, walk);
    }
    // the general kernel (contexts that never walk inline run it compiled without the walk).  Objectives without a simulation take tiles
    // of 64 chains where such a tile's LDS fits in 60 KB — a user objective's three launches per iteration wherever it does, ct says which
    const bool fits64 = tile_smem_base(c, 64) <= (size_t)60 * 1024;
    const int family = is_sim(c->obj) ? (F.tpw == 2 ? CF_SIM_2 : CF_SIM) : c->obj == SMM_OBJ_DENSE ? CF_DENSE : user ? (fits64 ? CF_GEN_64 : CF_GEN)
                     : F.gen_keys ? CF_GEN_KEYS : (fits64 && !F.inline_walk) ? CF_GEN_64 : F.tpw == 2 ? CF_GEN_2 : CF_GEN;
    ChainKernel K = chain_instance(family, P.np, F.inline_walk);
    if (user) K.name = c->u_lanes ? "user_lanes_3launches" : "user_3launches";
    if (c->obj == SMM_OBJ_DENSE && c->dense2) K.name = "iter<dense2,16>";
    // an objective without a simulation (banana, user objectives) has work for the tile's control wave only: unless the exchange
    // walk runs inline (all lanes stage its inputs) the tile is launched as that one wave, so that every tile of a large
    // population is resident at once instead of queueing behind 448 idle lanes each
    if (obj_kind(c->obj) == 0 && K.tpw == 1 && !walk && !F.inline_walk) K.block = 64;
    return K;
}
// ... and launch_chain_iter_norm_p2p (smm_p2p.hpp)
ChainKernel chain_kernel_p2p(const Ctx* c) {
    const KParams& P = c->P;
    // the kernel without a walk, whose accept step stores the 4-byte slots of k_exch_resolve_rows<., true>: on half-size workgroups for a
    // shard of more than one round of tiles
    if (c->p2p_rows) return chain_instance(c->F.norm_narrow ? CF_P2P_ROWS_NARROW : CF_P2P_ROWS, P.np, false);
    // (BIG: staging loops for up to 8192 chains — two shards of 4096; the small form serves populations up to 4096)
    return chain_instance(CF_P2P, P.np, P.Ng > XLVL_MAX || P.plan_K > XLVL_MAX);
}
// K over the chains of P onto the context's stream, with `smem` bytes of dynamic LDS: every kernel of these families takes (P, t, rec_in, rec_out, flags)
void launch_chain_kernel(Ctx* c, const ChainKernel& K, size_t smem, const KParams& P, int t, const double* rec_in, double* rec_out, int flags) {
    const dim3 grid((unsigned)(((P.N + K.ct - 1) / K.ct + K.tpw - 1) / K.tpw)), block(K.block);
    void* args[] = {(void*)&P, (void*)&t, (void*)&rec_in, (void*)&rec_out, (void*)&flags};
    launch_fn(c, K.fn, grid, block, smem, c->stream, args);
}

// one thread per evaluation: theta [n][np] -> simM [n][nm], value [n], status [n].  An objective with the library's stream draws from
// the context's seed, or with base_seed (smm_eval_batch_noseed) evaluation i from base_seed + i
void launch_user_kernel(Ctx* c, const double* theta, int n, double* simM, double* value, int* status, const uint64_t* base_seed = nullptr) {
    const KParams& P = c->P;
    int np = P.np, nm = P.nm, nud = c->n_objp;
    const double *mom = P.mom, *w = P.w, *ud = P.objp;
    uint64_t seed = base_seed ? *base_seed : P.seed;
    void* args[] = {(void*)&theta, (void*)&n, (void*)&np, (void*)&mom, (void*)&w, (void*)&nm, (void*)&ud, (void*)&nud,
                    (void*)&simM, (void*)&value, (void*)&status, (void*)&seed};
    const hipFunction_t fn = base_seed ? c->ufn_noseed : c->ufn;
    if (c->u_lanes > 0)   // map-reduce form: one workgroup of u_lanes threads per evaluation
        HIPCHK(hipModuleLaunchKernel(fn, (unsigned)n, 1, 1, (unsigned)c->u_lanes, 1, 1, 0, c->stream, args, nullptr));
    else
        HIPCHK(hipModuleLaunchKernel(fn, (unsigned)((n + 127) / 128), 1, 1, 128, 1, 1, 0, c->stream, args, nullptr));
}

// ---- the batched evaluation kernels of the built-in objectives (eval_tile, smm_chain.hpp) ----
// Every instantiation of them is named in eval_instance() and nowhere else: a family — k_eval_batch on candidates that were written, the
// estimators' k_eval_slice, k_eval_lm and k_eval_sobol on points that never are — by obj_kind() (1: simulated, 2: dense, 0: closed form), and the tile
// it takes.  launch_eval_tiles launches the context's row of a family, lds_limits raises every row's dynamic LDS limit.
enum EvalFamily { EF_BATCH, EF_SLICE, EF_LM, EF_SOBOL, EF_COUNT };
struct EvalKernel { const void* fn; int ct; };
EvalKernel eval_instance(int family, int kind) {
#define EVAL(KERN) (kind == 1 ? EvalKernel{(const void*)KERN<1, 8>, 8} : kind == 2 ? EvalKernel{(const void*)KERN<2, 16>, 16} : EvalKernel{(const void*)KERN<0, 8>, 8})
    switch (family) {
        case EF_BATCH: return EVAL(k_eval_batch);
        case EF_SLICE: return EVAL(k_eval_slice);
        case EF_LM: return EVAL(k_eval_lm);
        default: return EVAL(k_eval_sobol);
    }
#undef EVAL
}
// n evaluations by the context's row of `family`, onto its stream (args: the kernel's own)
void launch_eval_tiles(Ctx* c, int family, int n, void** args) {
    const EvalKernel K = eval_instance(family, obj_kind(c->obj));
    HIPCHK(hipLaunchKernel(K.fn, dim3((unsigned)((n + K.ct - 1) / K.ct)), dim3(WG), args, tile_smem_base(c, K.ct), c->stream));
}

// n evaluations on device pointers, onto the context's stream (smm_eval_batch and the estimators share it), in the layouts EvalScratch
// states (smm_evalscratch.hpp): the built-in objectives' k_eval_batch, or a user objective's kernel (launch_user_kernel)
void launch_eval_dev(Ctx* c, const double* params, int n, double* value, double* simM, void* status) {
    if (c->obj == SMM_OBJ_USER) {
        launch_user_kernel(c, params, n, simM, value, (int*)status);
        return;
    }
    const KParams& P = c->P;
    int8_t* st = (int8_t*)status;
    void* args[] = {(void*)&P, (void*)&params, (void*)&n, (void*)&value, (void*)&simM, (void*)&st};
    launch_eval_tiles(c, EF_BATCH, n, args);
}

void launch_chain_iter(Ctx* c, int t, int flags) {
    point_values(c, c->P, t - 1, t);   // the inline walk reads what the accept step of t-1 wrote; this accept step writes the other array
    if (c->ext_vals_out) { c->P.vals_out = c->ext_vals_out; c->P.slot8_out = nullptr; }
    // large single shards (k_exch_resolve_rows): the accept step writes the resolution's initial slots itself
    const bool own_slots = c->F.xk == XK_ROWS && c->P.N == c->P.Ng && !c->ext_rec_out && !c->ext_vals_out && c->obj != SMM_OBJ_USER;
    c->P.slots17_out = own_slots ? c->slots17 : nullptr;
    c->P.nan_flags_out = own_slots ? c->nan_flags + (t & 1) : nullptr;
    if (own_slots) c->run.slots_iter = t;
    const ChainKernel K = chain_kernel(c, flags);
    const size_t smem = tile_smem(c, c->F, K.ct, K.tpw);
    const double* rin = c->ext_rec_in ? c->ext_rec_in : (const double*)c->rec[c->run.cur];
    double* rout = c->ext_rec_out ? c->ext_rec_out : c->rec[c->run.cur ^ 1];
    if (c->obj == SMM_OBJ_USER) {
        // proposal launch (stores nothing but the proposals) -> the user's kernel -> accept launch (repeats the
        // deterministic prologue, takes value / moments / status from the user's kernel)
        const KParams& P = c->P;
        launch_chain_kernel(c, K, smem, P, t, rin, rout, flags | F_PROPOSE_ONLY);
        launch_user_kernel(c, P.u_theta, P.N, P.u_simM, P.u_value, P.u_status);
    }
    launch_chain_kernel(c, K, smem, c->P, t, rin, rout, flags);
    if (!c->ext_rec_out) c->run.cur ^= 1;
}

// ---- the stand-alone kernels of the exchange (smm_lookahead.hpp, smm_exchange.hpp, smm_cone_big.hpp) ----
// Every instantiation of them that a launch can take is named in exch_instance() and nowhere else: launch_exch launches a row, resolve_kernel()
// and resolve_rows_window_kernel() pick the resolution's, lds_limits raises every row's dynamic LDS limit, smm_describe prints the pick's name.
// A new instantiation is one row here and one name in ExchId.  What resolves exchangeMoves! (F.xk: select_forms):
//   N_global        min_improve                      dist_fun   F.xk        rows                slots / where
//   <= 8192 (~7400) one value >= 0 for all chains    -          XK_LEAN     lean                8-byte keys (0) or 16-byte values (> 0), LDS
//   <= 4096         anything else                    any        XK_LVL      lvl<1024>           16-byte slots, LDS
//   <= 8192         anything else                    any        XK_LVL_SOA  lvl_soa             split slots, LDS
//   <= 32768        0 for all chains                 -          XK_ROWS     keys + rows<PLDS>   4-byte slots (17-bit keys), rows of 1024 pairs, LDS
//   <= 32768        anything else                    -          XK_KEY      keys + key<PLDS>    4-byte slots (16-bit keys, intervals), LDS
//   <= 65535        anything else / other dist_fun   any        XK_LVL_BIG  lvl_big             16-byte slots, global memory
//   above, or K > N_global                           any        XK_ANY      any                 barrier rounds, global atomics
// (PLDS: the partners in LDS up to XKEY_PARTNER_MAX chains, else the ballot replay.  The p2p form of a sharded run launches the rows kernel itself
//  where this table says XK_ROWS — resolve_rows_window_kernel: <., true> reads the tagged slots of its window instead of a key pre-pass, <false,
//  true, true> keeps the partners of the rank's own chains only; every other p2p population resolves from the window's plain values through this
//  table.  Single shards of objfunc_norm up to 4096 chains do not get here in steady state: their chain kernel walks inline.  The test build can
//  force an entry (SMM_TEST_HOOKS: Hooks) and adds the ticket kernel and two workgroups of lvl.  The rows stand in the order in which the host code
//  named these kernels before there was this table, behind chain_instance's: kernels are emitted, and a few numbered, in that order.  Ng: for k_cone_chains' cap.)
constexpr size_t ROWS_OWN_MAX = (size_t)158 * 1024;   // <false, true, true>: the slots, the rows and the own chains' partners of one workgroup
ExchInstance exch_instance(int id, int Ng) {
    const size_t rows_all = resolve_rows_bytes(XKEY_MAX, XKEY_MAX, XROWS_MAX), rows_part = resolve_rows_bytes(XKEY_PARTNER_MAX, XKEY_PARTNER_MAX, XROWS_MAX),
                 lvl = resolve_lvl_bytes(XLVL_MAX, XLVL_MAX);
    switch (id) {
        case XI_CONE_CHAINS: return {(const void*)k_cone_chains, XWG, cone_chains_lds_bytes(Ng), XG_CONE_BIG, "cone_chains", false};
        case XI_CONE_TILES: return {(const void*)k_cone_tiles, 64 * CONEB_WAVES, 0, XG_CONE_BIG, "cone_tiles", false};
        case XI_PLAN_BIG: return {(const void*)k_exch_plan_big, XWG, plan_big_lds_bytes(65535), XG_BIG, "plan_big", false};
        case XI_PLAN: return {(const void*)k_exch_plan, XWG, plan_smem(XLDS_MAX, XLDS_MAX, true), XG_LDS, "plan", false};
        case XI_LEAN: return {(const void*)k_exch_resolve_lean, XWG, LDS_CU, XG_LDS, "lean", true};
#ifdef SMM_TEST_HOOKS
        case XI_LVL_256: return {(const void*)k_exch_resolve_lvl<256>, 256, lvl, XG_LDS, "lvl", false};
        case XI_LVL_512: return {(const void*)k_exch_resolve_lvl<512>, 512, lvl, XG_LDS, "lvl", false};
        case XI_TICKETS: return {(const void*)k_exch_resolve_lds, XWG, resolve_lds_bytes(XLDS_MAX), XG_LDS, "tickets", false};
#endif
        case XI_LVL: return {(const void*)k_exch_resolve_lvl<1024>, 1024, lvl, XG_LDS, "lvl", true};
        case XI_LVL_SOA: return {(const void*)k_exch_resolve_lvl_soa<1024>, 1024, resolve_lvl_soa_bytes(XLDS_MAX, XLDS_MAX), XG_LDS, "lvl_soa", false};
        case XI_KEYS: return {(const void*)k_exch_keys, 256, 0, XG_KEYS, "keys", false};   // (values and initial slots: the pre-pass of rows and key)
        case XI_ROWS_PLDS: return {(const void*)k_exch_resolve_rows<true>, XWG, rows_part, XG_KEYS, "rows", false};
        case XI_ROWS: return {(const void*)k_exch_resolve_rows<false>, XWG, rows_all, XG_KEYS, "rows", false};
        case XI_KEY_PLDS: return {(const void*)k_exch_resolve_key<true>, XWG, resolve_key_bytes(XKEY_PARTNER_MAX, XKEY_PARTNER_MAX), XG_KEYS, "key", false};
        case XI_KEY: return {(const void*)k_exch_resolve_key<false>, XWG, resolve_key_bytes(XKEY_MAX, XKEY_MAX), XG_KEYS, "key", false};
        case XI_LVL_BIG: return {(const void*)k_exch_resolve_lvl_big, XWG, 0, XG_BIG, "lvl_big", false};
        case XI_ANY: return {(const void*)k_exch_resolve_any, XWG, 0, XG_BIG, "any", false};
        case XI_ROWS_WIN_OWN: return {(const void*)k_exch_resolve_rows<false, true, true>, XWG, ROWS_OWN_MAX, XG_KEYS, "rows_window_own", true};
        case XI_ROWS_WIN_PLDS: return {(const void*)k_exch_resolve_rows<true, true>, XWG, rows_part, XG_KEYS, "rows_window", true};
        case XI_ROWS_WIN: return {(const void*)k_exch_resolve_rows<false, true>, XWG, rows_all, XG_KEYS, "rows_window", true};
        case XI_APPLY: return {(const void*)k_exch_apply, 256, 0, XG_BIG, "apply", false};   // (the three-phase calls: the resolved swaps into the records)
        case XI_PLAN_BG: return {(const void*)k_exch_plan_bg, PBG_WG, PBG_LDS, XG_LDS, "plan_bg", false};   // (the next window's plan, beside the persistent chain kernel)
        default: return {nullptr, 0, 0, XG_LDS, id == XI_TICKETS ? "tickets" : "lvl", false};   // (a row of the test build)
    }
}
// what launch_resolve_p launches for this context as it stands (P: its parameters or the caller's copy): F.xk, the partners-in-LDS split, the hooks' workgroup of lvl.  Decides only.
ExchLaunch resolve_kernel(const Ctx* c, const KParams& P) {
    const bool plds = P.Ng <= XKEY_PARTNER_MAX;   // partners in LDS, else the ballot replay
    switch (c->F.xk) {
        case XK_LEAN: return {XI_LEAN, resolve_lean_bytes(P.Ng, P.plan_K, P.lean_wide != 0)};
        case XK_LVL: return {c->H.lvl_wg == 256 ? XI_LVL_256 : c->H.lvl_wg == 512 ? XI_LVL_512 : XI_LVL, resolve_lvl_bytes(P.Ng, P.plan_K)};
        case XK_LVL_SOA: return {XI_LVL_SOA, resolve_lvl_soa_bytes(P.Ng, P.plan_K)};
        case XK_TICKETS: return {XI_TICKETS, resolve_lds_bytes(P.Ng)};
        case XK_ROWS: return {plds ? XI_ROWS_PLDS : XI_ROWS, resolve_rows_bytes(P.Ng, P.plan_K, P.rows_cap)};
        case XK_KEY: return {plds ? XI_KEY_PLDS : XI_KEY, resolve_key_bytes(P.Ng, P.plan_K)};
        case XK_LVL_BIG: return {XI_LVL_BIG, 0};
        default: return {XI_ANY, 0};
    }
}
// ... and launch_resolve_rows_window.  A shard of a population past XKEY_PARTNER_MAX keeps its own chains' partners only (written by the swaps), where that fits
ExchLaunch resolve_rows_window_kernel(const Ctx* c) {
    const KParams& P = c->P;
    const size_t own = resolve_rows_bytes(P.Ng, P.plan_K, P.rows_cap, P.N);
    if (P.Ng > XKEY_PARTNER_MAX && P.N < P.Ng && own <= ROWS_OWN_MAX) return {XI_ROWS_WIN_OWN, own};
    return {P.Ng <= XKEY_PARTNER_MAX ? XI_ROWS_WIN_PLDS : XI_ROWS_WIN, resolve_rows_bytes(P.Ng, P.plan_K, P.rows_cap)};
}
// Profiling mode 2, stated once: does the resolution take the dispatch's own stamps (a KernelEvents scope around its launch, pev_exch set), or do
// event brackets stand around the iteration and the exchange reports 0?  Only `stamped` rows ever do; a single shard's steps also ask for a population
// of the level walk (its chain kernel is stamped under the same condition), a shard's stamp the lean kernel only (the cases: DESIGN.md section 3)
bool resolve_stamped(const Ctx* c, bool shard) {
    const int id = resolve_kernel(c, c->P).id;
    return exch_instance(id).stamped && (shard ? id == XI_LEAN : c->P.Ng <= XLVL_MAX && !c->H.dataflow && c->H.lvl_wg == 1024);
}

// (P: the context's parameters, or a copy whose RW is the stride of the value column in `gathered`)
void launch_resolve_p(Ctx* c, const KParams& P_in, int t, const double* gathered) {
    KParams P = P_in;
    point_values(c, P, t, t);   // (single shard: the values the accept step of iteration t wrote)
    const ExchLaunch L = resolve_kernel(c, P);
    if (c->F.xk != XK_ROWS && c->F.xk != XK_KEY) return launch_exch(c, L.id, dim3(1), L.smem, c->stream, P, t, gathered);
    // values and initial slots by the whole chip (gathered records: their value column; single shard: the compact array)
    const bool prepass = gathered || c->run.slots_iter != t;   // (a single shard's accept step of iteration t has made the slots already)
    const double* vals = gathered ? P.xval : P.vals;
    const uint32_t *slots16 = prepass ? (const uint32_t*)P.xsrc : nullptr, *slots17 = c->slots17;
    if (prepass)
        launch_exch(c, XI_KEYS, dim3((P.Ng + 255) / 256), 0, c->stream, gathered ? gathered : (const double*)P.vals, gathered ? P.RW : 1, P.Ng, (double*)vals, (uint32_t*)P.xsrc,
                    c->F.xk == XK_ROWS ? c->slots17 : (uint32_t*)nullptr, c->nan_flags, t);
    if (c->F.xk == XK_ROWS) launch_exch(c, L.id, dim3(1), L.smem, c->stream, P, t, vals, slots16, slots17, c->nan_flags);
    else launch_exch(c, L.id, dim3(1), L.smem, c->stream, P, t, vals, (const uint32_t*)P.xsrc);
}
void launch_resolve(Ctx* c, int t, const double* gathered) { launch_resolve_p(c, c->P, t, gathered); }

// ---- the p2p form of the sharded iteration (smm_p2p.hpp, include/smmhip.h) ----
size_t p2p_walk_bytes(const Ctx* c) { return (LeanLayout<LEAN_KEYS>::bytes(c->P.Ng, c->P.plan_K) + 15) & ~(size_t)15; }
void launch_chain_iter_norm_p2p(Ctx* c, int t, int flags) {
    KParams P = c->P;
    point_values(c, P, t - 1, t);
    const bool walk = (flags & F_WALK_INLINE) != 0;
    P.tile_off = walk ? (int)(p2p_walk_bytes(c) / sizeof(double)) : 0;
    const size_t smem = (size_t)P.tile_off * sizeof(double) + norm_tile_doubles(P.np) * sizeof(double);
    launch_chain_kernel(c, chain_kernel_p2p(c), smem, P, t, nullptr, nullptr, flags);
}
// this rank's slice after iteration t -> every rank's window (parity t & 1); rec_src: out of the context's own record array (a
// publication), else out of its own window (generic form, after a chain kernel); ll: the self-validating form of the inline kernels
void launch_p2p_push(Ctx* c, int t, const double* rec_src, bool ll) {
    KParams P = c->P;
    const dim3 grid(p2p_units(P.N)), block(256);
    if (ll) hipLaunchKernelGGL((k_p2p_push<true, true>), grid, block, 0, c->stream, P, t, rec_src);
    else if (rec_src) hipLaunchKernelGGL((k_p2p_push<true, false>), grid, block, 0, c->stream, P, t, rec_src);
    else hipLaunchKernelGGL((k_p2p_push<false, false>), grid, block, 0, c->stream, P, t, (const double*)nullptr);
    if (!ll) { c->p2p_seq += 1; c->p2p_unwaited = true; }
}
void launch_p2p_wait(Ctx* c) {
    KParams P = c->P;
    P.p2p_want = (unsigned long long)p2p_units(P.N) * c->p2p_seq;
    hipLaunchKernelGGL(k_p2p_wait, dim3(1), dim3(64), 0, c->stream, P, c->run.iter);
    c->p2p_unwaited = false;
}
// inline form: everybody's records and values after iteration t, out of their self-validating form into this rank's plain arrays
void launch_p2p_unpack(Ctx* c, int t) {
    hipLaunchKernelGGL(k_p2p_unpack, dim3((c->P.Ng + 255) / 256), dim3(256), 0, c->stream, c->P, t);
}
// exchangeMoves! of iteration t from the values in this rank's window (complete: somebody has waited for the arrivals)
void launch_resolve_window(Ctx* c, int t) {
    const P2PLayout L = p2p_layout(c->P.Ng, c->P.RW);
    KParams P1 = c->P;
    P1.RW = 1;   // (the resolve kernels read value s at gathered[s * RW])
    launch_resolve_p(c, P1, t, (const double*)(c->p2p_mine + L.val[t & 1]));
}
// the same straight from the window's tagged slots and self-validating values (p2p form of large norm populations): no wait, no unpacking, no key pre-pass
void launch_resolve_rows_window(Ctx* c, int t) {
    const ExchLaunch L = resolve_rows_window_kernel(c);
    launch_exch(c, L.id, dim3(1), L.smem, c->stream, c->P, t, (const double*)nullptr, (const uint32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr);
}
// ---- the persistent chain kernels (smm_chain_persist*.hpp) ----
// Every instantiation of them that a launch can take is named in persist_instance() and nowhere else: persist_kernel() picks a row for a
// context's forms, persist_occupancy sets the pick's LDS attribute and asks for its occupancy, launch_persist launches it, smm_describe
// prints its name.  A row: the kernel, its workgroup, and the name without what persist_kernel appends for the forms that share the row.
//   PI_GEN                                        k_chain_persist_gen
//   PI_LOC_PCT + (np - 1)                         k_chain_persist_loc<np, true, false, true>: thresholds by chain
//   PI_LOC + 4 (np - 1) + 2 !wide + !shard        k_chain_persist_loc<np, wide, shard>
//   PI_TILE + 2 variant + !dense                  k_chain_persist_tile<kind, pct, shard, chol>, variant: PT_SHARD .. PT_PLAIN
// (The rows stand in the order in which the host code named these kernels before there was this table, behind exch_instance's: kernels are
// emitted, and a few numbered, in that order.)
enum PersistId { PI_GEN, PI_LOC_PCT, PI_LOC = PI_LOC_PCT + 2, PI_TILE = PI_LOC + 8, PI_COUNT = PI_TILE + 10 };
enum PersistTileVariant { PT_SHARD, PT_CHOL_PCT, PT_CHOL, PT_PCT, PT_PLAIN };
struct PersistInstance { const void* fn; unsigned block; const char* name; };
PersistInstance persist_instance(int id) {
    static const PersistInstance rows[PI_COUNT] = {
        {(const void*)k_chain_persist_gen, 1024, "gen"},
        {(const void*)k_chain_persist_loc<1, true, false, true>, NORM_WG, "loc"},
        {(const void*)k_chain_persist_loc<2, true, false, true>, NORM_WG, "loc"},
        {(const void*)k_chain_persist_loc<1, true, true>, NORM_WG, "loc"},
        {(const void*)k_chain_persist_loc<1, true, false>, NORM_WG, "loc"},
        {(const void*)k_chain_persist_loc<1, false, true>, NORM_WG, "loc"},
        {(const void*)k_chain_persist_loc<1, false, false>, NORM_WG, "loc"},
        {(const void*)k_chain_persist_loc<2, true, true>, NORM_WG, "loc"},
        {(const void*)k_chain_persist_loc<2, true, false>, NORM_WG, "loc"},
        {(const void*)k_chain_persist_loc<2, false, true>, NORM_WG, "loc"},
        {(const void*)k_chain_persist_loc<2, false, false>, NORM_WG, "loc"},
        {(const void*)k_chain_persist_tile<2, false, true>, WG, "tile_dense"},
        {(const void*)k_chain_persist_tile<1, false, true>, WG, "tile_sim"},
        {(const void*)k_chain_persist_tile<2, true, false, true>, WG, "tile_dense"},
        {(const void*)k_chain_persist_tile<1, true, false, true>, WG, "tile_sim"},
        {(const void*)k_chain_persist_tile<2, false, false, true>, WG, "tile_dense"},
        {(const void*)k_chain_persist_tile<1, false, false, true>, WG, "tile_sim"},
        {(const void*)k_chain_persist_tile<2, true>, WG, "tile_dense"},
        {(const void*)k_chain_persist_tile<1, true>, WG, "tile_sim"},
        {(const void*)k_chain_persist_tile<2>, WG, "tile_dense"},
        {(const void*)k_chain_persist_tile<1>, WG, "tile_sim"},
    };
    return rows[id];
}
// what launches F's persistent kernel: a row of the table (fn) or, with a user's objective inside, the same kernel out of the objective's
// module (mfn: loaded by persist_occupancy; user_form_compile), its grid, block and dynamic LDS.  Decides only.
PersistKernel persist_kernel(const Ctx* c, const Forms& F) {
    const KParams& P = c->P;
    PersistKernel K{nullptr, nullptr, dim3(persist_tiles_rank(F, P.N)), dim3(1), 0, "none"};
    if (F.persist == PERSIST_NONE) return K;
    const bool gen = F.persist == PERSIST_GEN, loc = F.persist == PERSIST_LOC, tile = F.persist == PERSIST_TILE;
    const bool sh = F.persist_sh, wd = F.persist_wide, dense = obj_kind(c->obj) == 2, user = gen ? F.persist_user : tile && c->obj == SMM_OBJ_USER;
    const int id = gen ? PI_GEN
                 : loc ? (P.mi_pct ? PI_LOC_PCT + (P.np == 1 ? 0 : 1) : PI_LOC + (P.np == 1 ? 0 : 4) + (wd ? 0 : 2) + (sh ? 0 : 1))
                       : PI_TILE + 2 * (sh ? PT_SHARD : c->has_chol ? (P.mi_pct ? PT_CHOL_PCT : PT_CHOL) : P.mi_pct ? PT_PCT : PT_PLAIN) + (dense ? 0 : 1);
    const PersistInstance I = persist_instance(id);
    K.block = dim3(I.block);
    K.smem = gen ? persist_gen_smem(c, user) : loc ? persist_loc_smem_bytes(P.np) : persist_tile_smem(c);
    if (user) K.mfn = c->pfn;
    else K.fn = I.fn;
    // the name: the row's, then what tells apart the forms that share the row
    K.name = tile && user ? "tile_user" : gen && user ? "gen_user" : I.name;
    if (tile && dense && c->dense2) K.name += "2";
    if (loc && wd) K.name += "_wide";
    if (!gen && sh) K.name += loc && F.persist_sh_big ? "_shard_bigplan" : "_shard";
    return K;
}
// K onto the context's stream with the argument block A; in profiling mode 2 with the begin/end of this dispatch as the command processor stamps them
void launch_persist(Ctx* c, const PersistKernel& K, PersistArgs A) {
    void* args[] = {(void*)&A};
    if (K.mfn && c->kev0)
        HIPCHK(hipExtModuleLaunchKernel(K.mfn, K.grid.x * K.block.x, 1, 1, K.block.x, 1, 1, K.smem, c->stream, args, nullptr, c->kev0, c->kev1, 0));
    else if (K.mfn) HIPCHK(hipModuleLaunchKernel(K.mfn, K.grid.x, 1, 1, K.block.x, 1, 1, (unsigned)K.smem, c->stream, args, nullptr));
    else launch_fn(c, K.fn, K.grid, K.block, K.smem, c->stream, args);
}

}  // namespace
