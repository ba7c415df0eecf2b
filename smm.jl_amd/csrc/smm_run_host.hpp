// the host side of a run — part of libsmmhip (included once by smmhip.hip, behind the launchers and kernel choosers of smm_launch_host.hpp and ahead of
// smm_reducers_host.hpp, whose prelude settles and flushes through this file; hiprtc never sees it).  Everything that advances or settles
// a run: the error path (told, persist_give_up, p2p_agree_error, check_device_error), the run's launches and their bookkeeping
// (persist_usable .. launch_chain_persist, enqueue_iterations, persist_repair, settle_persist, p2p_publish, p2p_to_plain, p2p_enqueue,
// resolve_now, flush) and the stepping entry points: smm_sync, smm_bgp_step / _step_async, the three-phase calls (smm_bgp_local_step,
// smm_bgp_export_records_dev, smm_bgp_exchange_dev), the two-enqueue calls (smm_bgp_sharded_step / _finish), the p2p calls
// (smm_bgp_p2p_init / _attach / _step / _finish) and the values form (smm_bgp_export_values_dev, smm_bgp_a2a_pack_dev / _apply_dev).
// What they share is stated here once: the prelude of a call that needs the run settled (settled), the refusals of the sharded protocol
// that more than one call gives (in_gather_buffer, beyond_maxiter, in_p2p_windows, p2p_init_first, before_first_local_step,
// already_resolved: code and text; the condition stays with the call), the profiling events of a step (profiling_events), the pointers a
// single launch is given and must not keep (KernelEvents, ExternalRecords), the bookkeeping behind a persistent launch
// (advanced_by_persist) and the launch of k_flush (launch_flush).  The frame of an entry point is api_call of smmhip.hip, which also
// keeps Ctx and Run, the launch helpers, the kernel choosers, the look-ahead windows and the forms.
#pragma once

namespace {

void persist_repair(Ctx* c, int n_replay = -1);
void p2p_enqueue(Ctx* c, int n_iters);
// The ranks of a sharded run agree on what their launches of the persistent form ended with: every rank writes its error word into
// every rank's window — {word, number of its last launch} — and reads its own window until all ranks' words of that launch are there
// (the host side of a rendezvous every rank reaches: smm_sync / smm_bgp_p2p_finish behind the same steps).  The smallest word wins,
// as it does among the chains of one device: the first failing iteration, the first failing chain of the population.
unsigned long long p2p_agree_error(Ctx* c, unsigned long long e_local) {
    const KParams& P = c->P;
    const int G = P.p2p_G;
    const PrWin WL = pr_win_layout(P.Ng, P.RW, G, persist_tiles_rank(c->F, c->P.N));
    const uint32_t seq = c->pr_epoch;
    for (int r = 0; r < G; ++r)
        HIPCHK(hipMemcpy(P.p2p_win[r] + c->prw_off + WL.fin + 128 * (size_t)P.p2p_rank, &e_local, 8, hipMemcpyHostToDevice));
    for (int r = 0; r < G; ++r)   // (the word is there before the number that says so)
        HIPCHK(hipMemcpy(P.p2p_win[r] + c->prw_off + WL.fin + 128 * (size_t)P.p2p_rank + 8, &seq, 4, hipMemcpyHostToDevice));
    std::vector<unsigned char> buf((size_t)128 * G);
    const auto t0 = std::chrono::steady_clock::now();
    unsigned long long e = e_local;
    for (;;) {
        HIPCHK(hipMemcpy(buf.data(), c->p2p_mine + c->prw_off + WL.fin, buf.size(), hipMemcpyDeviceToHost));
        bool all = true;
        e = e_local;
        for (int r = 0; r < G; ++r) {
            uint32_t s_r; unsigned long long e_r;
            memcpy(&e_r, buf.data() + 128 * (size_t)r, 8); memcpy(&s_r, buf.data() + 128 * (size_t)r + 8, 4);
            if (s_r != seq) { all = false; break; }
            e = std::min(e, e_r);
        }
        if (all) {
            // (word and number arrive by two copies and are read by one unfenced DMA: a number seen with the word of the launch before is
            // possible in theory — ADVICE r5 —: every number is there now, so one more look holds every word that was written before its number)
            HIPCHK(hipMemcpy(buf.data(), c->p2p_mine + c->prw_off + WL.fin, buf.size(), hipMemcpyDeviceToHost));
            e = e_local;
            for (int r = 0; r < G; ++r) { unsigned long long e_r; memcpy(&e_r, buf.data() + 128 * (size_t)r, 8); e = std::min(e, e_r); }
            return e;
        }
        if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(30)) throw std::string("sharded run: a rank did not report the end of its step within 30 s (is every rank calling smm_sync / smm_bgp_p2p_finish?)");
        std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
}
// the second launch of the persistent form that gave up (its tiles not resident together: a masked or shared device; a cone that did not fit;
// a state the form cannot walk): the form is off for this context from here on — said ONCE on stderr, since nothing else changes for the
// caller but the speed (smm_get_persistent / smm_describe report it too)
void persist_give_up(Ctx* c) {
    if (!c->persist_broken)
        fprintf(stderr, "libsmmhip: context %p (device %d, chains %d of %d): the persistent form gave up twice (iteration %d) and is OFF for this context; "
                        "the per-iteration kernels run instead (same results, more launches). smm_get_persistent reports it.\n",
                (void*)c, c->device, c->P.N, c->P.Ng, c->run.iter);
    c->persist_broken = true;
}
// (an entry point hands the sticky failure to its caller)
int told(Ctx* c) { c->failed_told = true; return c->failed; }
int told(Ctx* c, int rc) { if (rc != SMM_OK && rc == c->failed) c->failed_told = true; return rc; }
int check_device_error(Ctx* c) {
    if (c->failed) return c->failed;   // err holds the message of the first failure
    unsigned long long e = ERR_NONE;
    HIPCHK(hipMemcpy(&e, c->P.err, sizeof e, hipMemcpyDeviceToHost));
    if (c->F.persist_sh && c->snap_valid && !c->in_repair && c->p2p_mine) {
        // launches of the persistent form ran on every rank: what one of them ended with concerns all (its tiles did not stop either)
        const unsigned long long eg = p2p_agree_error(c, e);
        if (eg != ERR_NONE) {
            const int kind = (int)(eg & 3), it = (int)(eg >> 34);
            if (kind == ERRK_FORM && ++c->persist_strikes >= 2) persist_give_up(c);
            // a hard error (AlgoBGP.jl:341,409): every rank replays up to and including the failing iteration — which completes for all
            // chains, as everywhere — and stands there; a time-out or a cone that did not fit: the whole step again, on the other forms
            // (a hard error raised BEFORE the first of these launches — by a one-iteration launch ahead of them on the stream —: they saw the word at
            // their entry and stored nothing; n = 0 puts the host's bookkeeping back to the snapshot and replays nothing)
            persist_repair(c, (kind == ERRK_NO_DRAW || kind == ERRK_NEGATIVE) ? std::max(0, it - c->snap.iter) : -1);
            HIPCHK(hipMemcpy(&e, c->P.err, sizeof e, hipMemcpyDeviceToHost));
            if (kind == ERRK_NO_DRAW || kind == ERRK_NEGATIVE) e = std::min(e, eg);   // (the first failing chain of the POPULATION — maybe another rank's: every rank reports the same)
        }
        c->snap_valid = false;
        if (eg == ERR_NONE) c->persist_proven = true;
    } else if (e != ERR_NONE && c->snap_valid && !c->in_repair) {
        // launches of the persistent kernel ran since the last check: their tiles do not stop at the failing iteration.  Back to the
        // state before the first of them, and the same iterations again on the one-launch-per-iteration path, which does.
        // (a tile gave up waiting, or a cone did not fit.  Once may be somebody else's doing — another context or process held compute
        // units while the tiles wanted to be resident together —: the form is tried again; the second time it is off for the context)
        if ((e & 3) != 3 && (int)(e >> 34) <= c->snap.iter) {
            // ... unless the word was raised BEFORE the first of them, by a one-iteration launch ahead of them on the stream that nobody had
            // looked at yet: they saw the word at their entry and stored nothing.  Nothing to replay — rolling back, clearing the word and
            // running on LOST the error (tools/fuzz_errors.py, 2 of 600 cases) —: the host's bookkeeping back to the snapshot, the word stays
            const unsigned long long keep = e;
            persist_repair(c, 0);
            HIPCHK(hipMemcpy(c->P.err, &keep, sizeof keep, hipMemcpyHostToDevice));
            e = keep;
        } else {
            if ((e & 3) == 3 && ++c->persist_strikes >= 2) persist_give_up(c);
            persist_repair(c);
            HIPCHK(hipMemcpy(&e, c->P.err, sizeof e, hipMemcpyDeviceToHost));
        }
    }
    if (!c->in_repair) {
        if (e == ERR_NONE && c->snap_valid) c->persist_proven = true;   // launches of the persistent form came through: its tiles ARE resident together
        c->snap_valid = false;
    }
    if (e == ERR_NONE) return SMM_OK;
    const int kind = (int)(e & 3), chain = (int)((e >> 2) & 0xffffffffu), it = (int)(e >> 34);
    char b[256];
    int rc;
    if (kind == ERRK_FORM) {
        snprintf(b, sizeof b, "internal error: the exchange of iteration %d could not be resolved in the form chosen for it (chain %d)", it, chain + 1);
        rc = SMM_ERR_HIP;
    } else if (kind == ERRK_CAPACITY) {
        snprintf(b, sizeof b, "values form of the sharded exchange: more than %d records between one pair of ranks (chain %d, iteration %d): "
                 "use the record all-gather (smm_bgp_exchange_dev / smm_bgp_sharded_step)", c->a2a_cap, chain + 1, it);
        rc = SMM_ERR_EXCHANGE_CAPACITY;
    } else if (kind == ERRK_NEGATIVE) {
        snprintf(b, sizeof b, "AlgoBGP assumes that your objective function returns a non-negative number "
                 "(chain %d, iteration %d)", chain + 1, it);
        rc = SMM_ERR_NEGATIVE_OBJECTIVE;
    } else {
        snprintf(b, sizeof b, "no draw in support after %d trials (chain %d, iteration %d): increase smpl_iters",
                 c->P.user_n ? std::min(c->P.rb_tries, c->P.smpl_iters) : c->P.smpl_iters, chain + 1, it);
        rc = SMM_ERR_NO_DRAW_IN_SUPPORT;
    }
    c->err = b;
    // The reference aborts inside the failing iteration (AlgoBGP.jl:341,409).  Here that iteration completes for all chains
    // and every later launch of the step sees the error word and stores nothing: the run stands at the failing iteration,
    // its exchange is never applied, and the context refuses to go on until smm_set_state.
    if (kind != ERRK_FORM && it >= 1 && it <= c->run.iter) {   // (kind 0, a block of the values form overflowed: the exchange of iteration `it` was not applied either)
        c->run.iter = it;
        c->run.pending = false; c->run.prev_open = false; c->run.unresolved = false; c->pending_ext = false; c->rec_external = false;
        c->a2a_open = false; c->p2p_current = false;
    }
    c->failed = rc;
    return rc;
}

// ---- the rules the stepping calls share ----
// the refusals more than one entry point gives: code and text, once (the condition is the caller's)
const char* const IN_GATHER_BUFFER = "records are in the gather buffer: call smm_bgp_sharded_finish first";
int in_gather_buffer(Ctx* c) { return fail(c, SMM_ERR_STATE, IN_GATHER_BUFFER); }
int beyond_maxiter(Ctx* c) { return fail(c, SMM_ERR_MAXITER, "step beyond maxiter (history capacity)"); }
int in_p2p_windows(Ctx* c) { return fail(c, SMM_ERR_STATE, "the records of the last iteration are in the p2p windows: call smm_bgp_p2p_finish first"); }
int p2p_init_first(Ctx* c) { return fail(c, SMM_ERR_STATE, "smm_bgp_p2p_init comes first"); }
int before_first_local_step(Ctx* c) { return fail(c, SMM_ERR_STATE, "exchange before the first local step"); }
int already_resolved(Ctx* c) { return fail(c, SMM_ERR_STATE, "exchange already resolved for this iteration"); }

void settle_persist(Ctx* c);
// the prelude of a call that reads or changes the run other than by stepping on: the device, the persistent launches settled, and the
// sticky failure handed to the caller (SMM_OK: go on)
int settled(Ctx* c) {
    HIPCHK(hipSetDevice(c->device));
    settle_persist(c);
    return c->failed ? told(c) : SMM_OK;
}

// the profiling events of a step of n iterations: 4 each
void profiling_events(Ctx* c, int n) {
    while ((int)c->pev.size() < 4 * n) {
        hipEvent_t e;
        HIPCHK(hipEventCreate(&e));
        c->pev.push_back(e);
    }
}
// profiling mode 2: the launches inside the scope are stamped with the events pev[first], pev[first + 1] (on: else they are not); no
// launch behind it is, whichever way the scope is left
struct KernelEvents {
    Ctx* c;
    KernelEvents(Ctx* c_, bool on, int first) : c(c_) { if (on) { c->kev0 = c->pev[first]; c->kev1 = c->pev[first + 1]; } }
    ~KernelEvents() { c->kev0 = c->kev1 = nullptr; }
    KernelEvents(const KernelEvents&) = delete;
    KernelEvents& operator=(const KernelEvents&) = delete;
};
// the chain kernel launched inside the scope reads the donors' records from / writes its records and values to the caller's buffers or
// the p2p window (null: the context's own); no launch behind it does
struct ExternalRecords {
    Ctx* c;
    ExternalRecords(Ctx* c_, const double* rec_in, double* rec_out, double* vals_out = nullptr) : c(c_) { c->ext_rec_in = rec_in; c->ext_rec_out = rec_out; c->ext_vals_out = vals_out; }
    ~ExternalRecords() { c->ext_rec_in = nullptr; c->ext_rec_out = nullptr; c->ext_vals_out = nullptr; }
    ExternalRecords(const ExternalRecords&) = delete;
    ExternalRecords& operator=(const ExternalRecords&) = delete;
};

// a launch of the persistent form has covered the next n iterations: the run stands behind the last of them
void advanced_by_persist(Ctx* c, int n) {
    const int t1 = c->run.iter + n;
    c->run.prev_open = true;
    c->run.pending = false; c->run.unresolved = false;
    if (exchange_active(c, t1)) { c->run.unresolved = true; c->run.pending = true; }   // resolved in the prologue of the next chain kernel (or by resolve_now)
    c->run.iter = t1; c->run.exch_done = false;
}

// k_flush settles iteration `run.iter` from the records at src into the context's other record array (the caller flips run.cur and resets its flags)
void launch_flush(Ctx* c, const double* src, int flags) {
    const KParams& P = c->P;
    hipLaunchKernelGGL(k_flush, dim3((P.N + 255) / 256), dim3(256), 0, c->stream, P, c->run.iter + 1, src, c->rec[c->run.cur ^ 1], flags);
}

// settle the open end of the last iteration (no-op when nothing is open)
// the exchange of iteration c->run.iter has been left to the next chain kernel, but something else needs it now
void resolve_now(Ctx* c) {
    if (!c->run.unresolved) return;
    launch_resolve(c, c->run.iter, nullptr);
    c->run.unresolved = false;
}

void flush(Ctx* c) {
    if (c->rec_external) throw std::string(IN_GATHER_BUFFER);
    if (c->run.unresolved && c->P.N < c->P.Ng) throw std::string("the exchange of the last iteration needs every shard's records: call smm_bgp_p2p_finish first");
    if (!c->run.pending && !c->run.prev_open) return;
    resolve_now(c);
    launch_flush(c, c->rec[c->run.cur], (c->run.prev_open ? F_CLOSE_PREV : 0) | (c->run.pending ? F_HAS_PENDING : 0));
    c->run.cur ^= 1;
    c->run.pending = false;
    c->run.prev_open = false;
}

// can the iterations from c->run.iter + 1 on run as one launch of it?  At least two (a single iteration is the ordinary kernel's), behind
// an iteration some chain kernel has completed (the launch continues from the plain state blocks: no first iteration, no uploaded
// state, no exchange applied by the three-phase calls), and an exchange left to "the next chain kernel" must have its plan in the
// current window together with this iteration's.
bool persist_usable(const Ctx* c, int n_left) {
    if (!(c->F.persist != PERSIST_NONE && c->persist_on && !c->persist_broken && !c->in_repair && !c->nan_values && n_left >= 2 && !c->ext_rec_in && !c->ext_rec_out &&
          !c->ext_vals_out && !c->rec_external && c->P.N == c->P.Ng))
        return false;
    if (c->run.iter < 1 || !c->run.prev_open || c->run.exch_done || (c->run.pending && !c->run.unresolved)) return false;
    const int t0 = c->run.iter + 1;
    // (the locally numbered form starts a new plan window at the pending exchange's iteration instead: launch_chain_persist)
    if (c->F.persist != PERSIST_LOC && c->F.persist != PERSIST_TILE && c->run.unresolved && !(t0 - 1 >= c->plan_t0 && t0 + 1 < c->plan_t0 + c->plan_w)) return false;
    return true;
}
// ... as a shard (smm_bgp_p2p_step): from the p2p state — the records after iteration `iter` in the windows, its exchange not resolved
// yet — or behind a launch of its own; the first iteration of a run, the iteration behind a settled state are the per-iteration forms'
bool persist_sh_usable(const Ctx* c, int n_left) {
    // (NOT c->nan_values: that flag is this shard's own — smm_set_state saw a NaN among ITS values — and the form must be chosen from what every
    // rank knows, or one rank would take the per-iteration kernels while its peers wait at the launches' start barrier.  The launch reports such a
    // state itself — kind 3 at its first iteration, smm_chain_persist_loc.hpp —, the ranks agree on the word and replay the step on the other forms)
    if (!(c->F.persist_sh && c->persist_on && !c->persist_broken && !c->in_repair && n_left >= 2 && c->p2p_mine)) return false;
    if (c->p2p_ranks_here * persist_tiles_rank(c->F, c->P.N) > c->F.max_tiles) return false;   // (ranks sharing this device: not resident together)
    if (c->run.iter < 1 || !c->run.prev_open || c->run.exch_done || c->a2a_open) return false;
    if (c->p2p_current) return c->rec_external && (c->pending_ext || !exchange_active(c, c->run.iter));
    return !c->rec_external && (c->run.unresolved || !c->run.pending);
}
// the state a failed launch of the persistent kernel is rolled back to (device copies on the stream, before anything of the step runs)
void persist_snapshot(Ctx* c) {
    const KParams& P = c->P;
    const size_t N = P.N;
    HIPCHK(hipMemcpyAsync(c->snap_cs, P.cs, N * CSW * 8, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->snap_rec, c->rec[c->run.cur], N * P.RW * 8, hipMemcpyDeviceToDevice, c->stream));
    for (int b = 0; b < 2; ++b) {
        HIPCHK(hipMemcpyAsync(c->snap_vals[b], c->vals_buf[b], (N + 4) * 8, hipMemcpyDeviceToDevice, c->stream));
        if (c->slot8_buf[b]) HIPCHK(hipMemcpyAsync(c->snap_slot8[b], c->slot8_buf[b], (N + 4 + 128) * 8, hipMemcpyDeviceToDevice, c->stream));
    }
    HIPCHK(hipMemcpyAsync(c->snap_xres, P.xres, (size_t)P.Ng * 8, hipMemcpyDeviceToDevice, c->stream));
    c->snap = c->run;
    c->snap_valid = true;
}
// the argument block of a launch of the persistent kernel over iterations t0 .. t1 (pregen: the randomness comes from the window's blocks;
// tmo: ticks a spin may last)
PersistArgs persist_args(const Ctx* c, int t0, int t1, bool pregen, unsigned long long tmo) {
    const KParams& P = c->P;
    const bool sh = c->F.persist_sh;
    const int G = sh ? P.p2p_G : 1;
    const PrWin WL = pr_win_layout(P.Ng, P.RW, G, persist_tiles_rank(c->F, P.N));
    PersistArgs A{};
    A.cone_hdr = P.cone_hdr; A.cone_pairs = P.cone_pairs; A.cone_gather = P.cone_gather; A.cone_ok = P.cone_ok;
    if (sh) {
        for (int r = 0; r < G; ++r) A.win[r] = P.p2p_win[r] + c->prw_off;
        A.self = c->p2p_mine + c->prw_off;
    } else { A.win[0] = c->prw; A.self = c->prw; }
    A.o_ctl = WL.ctl; A.o_arrive = WL.arrive; A.o_progress = WL.progress; A.o_slot = WL.slot; A.o_rec = WL.rec;
    A.cs = P.cs; A.rec_in = c->rec[c->run.cur]; A.rec_out = c->rec[c->run.cur ^ 1]; A.vals_out = P.vals_out; A.slot8_out = P.slot8_out; A.walk_flags = P.walk_flags;
    A.hrec = P.hrec; A.err = P.err; A.ts = P.ts;
    A.Z = P.Z; A.lb = P.lb; A.ub = P.ub; A.mom = P.mom; A.w = P.w; A.objp = P.objp; A.dense_Bf = P.dense_Bf; A.dense_Af = P.dense_Af; A.dense_A2f = P.dense_A2f;
    A.rb = pregen ? P.rb : nullptr;
    A.mi_g = P.min_improve_g;
    A.N = P.N; A.Ng = P.Ng; A.np = P.np; A.nm = P.nm; A.ns = P.ns; A.zstride = P.zstride; A.RW = P.RW; A.HW = P.HW; A.RBW = P.RBW; A.dense_nOt = P.dense_nOt;
    A.batch_size = P.batch_size; A.failbox = (P.obj == SMM_OBJ_NORM_FAILBOX && P.objp) ? 1 : 0;
    A.G = G; A.rank = sh ? P.p2p_rank : 0; A.offset = P.offset;
    A.plan_t0 = P.plan_t0; A.exch_from = c->exchange_from; A.sigma_update_steps = P.sigma_update_steps; A.smpl_iters = P.smpl_iters; A.t0 = t0; A.t1 = t1;
    A.rb_t0 = P.rb_t0; A.rb_tries = P.rb_tries; A.user_n = P.user_n;
    A.ring_k = c->H.pr_ring_k; A.slow_tile = c->H.pr_slow_tile; A.slow_ticks = c->H.pr_slow_ticks; A.walk_first = c->run.unresolved ? 1 : 0;
    A.slow_read = c->H.pr_slow_read;
    A.tables_local = c->F.persist_sh_big ? 1 : 0; A.unit_sh = P.lean_unit == 16 ? 4 : (P.lean_unit == 8 ? 3 : 2); A.scout_after = P.scout_after; A.scout_gl = P.scout_gl;
    A.u_lanes = c->u_lanes; A.n_udata = c->n_objp;
    A.chol_L = P.chol_L; A.chol_per_chain = P.chol_per_chain;
    A.epoch = c->pr_epoch; A.sigma_adjust_by = P.sigma_adjust_by; A.thr = P.mi_value; A.seed = P.seed; A.tmo = tmo;
    return A;
}
// iterations c->run.iter + 1 .. as ONE launch, as far as the look-ahead windows reach; returns how many it covers (0: not this time)
int launch_chain_persist(Ctx* c, int n_left) {
    const int t0 = c->run.iter + 1;
    // (k_chain_persist_norm and _gen draw in the kernel unless tables are injected)
    // (k_chain_persist_tile too, since round 5: its 512 lanes draw the next iteration's randomness behind the publication, where the tile waits for
    // its peers' stores anyway — k_pregen_rng was 2.2 us per iteration of C5 on the main stream)
    const bool pregen = (c->F.persist == PERSIST_GEN || c->F.persist == PERSIST_TILE) ? (c->P.user_ntab || c->P.user_utab) : !(c->F.norm_fast && !c->P.user_ntab && !c->P.user_utab);
    if ((c->F.persist == PERSIST_LOC || c->F.persist == PERSIST_TILE) && c->run.unresolved && !(t0 - 1 >= c->plan_t0 && t0 + 1 < c->plan_t0 + c->plan_w)) {
        // the pending exchange's plan is not in a window that also reaches past this iteration: a new window from ITS iteration on (one
        // iteration planned twice per window; no per-iteration launch, no stand-alone resolution at the windows' ends)
        c->plan_w = 0;
        ensure_windows(c, t0 - 1, pregen);
    } else if (!c->run.unresolved) ensure_windows(c, t0, pregen);   // (with an exchange pending the window holds its plan and this iteration's: persist_usable)
    if (pregen && !(t0 >= c->rng_t0 && t0 < c->rng_t0 + c->rng_w)) ensure_windows(c, t0);
    int t1 = std::min(c->run.iter + n_left, c->plan_t0 + c->plan_w - 1);
    if (pregen) t1 = std::min(t1, c->rng_t0 + c->rng_w - 1);
    t1 = std::min(t1, t0 + PR_MAX_ITERS - 1);
    if (t1 - t0 + 1 < 2) return 0;
    if (!c->snap_valid) persist_snapshot(c);
    ++c->pr_epoch;
    if ((c->pr_epoch & 0x7fu) == 0u) {   // the slot tags' epoch bits start over: nothing older may look current
        // (a shard zeroes its own window's ring: its peers store into it only behind the launch's start barrier)
        const PrWin WL = pr_win_layout(c->P.Ng, c->P.RW, c->F.persist_sh ? c->P.p2p_G : 1, persist_tiles_rank(c->F, c->P.N));
        unsigned char* base = c->F.persist_sh ? c->p2p_mine + c->prw_off : c->prw;
        HIPCHK(hipMemsetAsync(base + WL.slot, 0, WL.total - WL.slot, c->stream));
    }
    KParams& P = c->P;
    P.pr_epoch = c->pr_epoch;
    point_values(c, P, t0 - 1, t1);   // (nothing is read from the value arrays: the last iteration writes them)
    // (a spin of the form may last 4 s — a peer is gone, not late — once a launch of this context has come through; until then a
    // tenth of that: tiles that are not resident together, a masked or partitioned device, must not look like a hang)
    // (a shard waits for its PEERS' launches at the start barrier: processes that start a second apart are late, not gone — 4 s from the start)
    const unsigned long long tmo = (c->persist_proven || c->F.persist_sh) ? P2P_TIMEOUT_TICKS : PERSIST_TMO_FIRST;
    launch_persist(c, persist_kernel(c, c->F), persist_args(c, t0, t1, pregen, tmo));
    c->run.cur ^= 1;
    ++c->persist_launches;
    return t1 - t0 + 1;
}

// n_iters iterations onto the stream (smm_bgp_step_async, and persist_repair with the persistent kernel off)
void enqueue_iterations(Ctx* c, int n_iters) {
    int slot = 0;   // profiling: events of this launch
    for (int it = 0; it < n_iters;) {
        const int t = c->run.iter + 1;
        int n = 0;
        if (persist_usable(c, n_iters - it)) {
            if (c->profiling == 1) HIPCHK(hipEventRecord(c->pev[4 * slot], c->stream));
            const KernelEvents stamped(c, c->profiling == 2, 4 * slot);
            n = launch_chain_persist(c, n_iters - it);
        }
        if (n > 0) {
            if (c->profiling == 1) { for (int e = 1; e < 4; ++e) HIPCHK(hipEventRecord(c->pev[4 * slot + e], c->stream)); }
            if (c->profiling) c->pev_exch[slot] = 0;
            ++slot;
            advanced_by_persist(c, n);
            it += n;
            continue;
        }
        // an exchange left to this chain kernel needs its plan: resolve it now if the plan window is about to move on
        if (c->run.unresolved && !(t >= c->plan_t0 && t < c->plan_t0 + c->plan_w) && !plan_ahead_covers(c, t)) resolve_now(c);
        // ... or if this chain kernel cannot walk (a user objective's launches): the resolution was only put off in case the persistent
        // kernel came next (defer_resolve)
        if (c->run.unresolved && c->F.defer_resolve && !c->F.inline_walk) resolve_now(c);
        ensure_windows(c, t);
        const int flags = (c->run.prev_open ? F_CLOSE_PREV : 0) | (c->run.pending ? F_HAS_PENDING : 0) | (c->run.unresolved ? F_WALK_INLINE : 0);
        const bool kscoped = c->profiling == 2 && resolve_stamped(c, false);   // (where the stand-alone resolution takes the profiling events itself, the chain kernel does too)
        if (c->profiling && !kscoped) HIPCHK(hipEventRecord(c->pev[4 * slot], c->stream));
        {
            const KernelEvents stamped(c, kscoped, 4 * slot);
            launch_chain_iter(c, t, flags);
        }
        if (c->profiling && !kscoped) HIPCHK(hipEventRecord(c->pev[4 * slot + 1], c->stream));
        c->run.prev_open = true;
        c->run.pending = false;
        if (c->profiling) c->pev_exch[slot] = 0;
        c->run.unresolved = false;
        if (exchange_active(c, t)) {
            const bool cone_next = c->F.cone_big && !c->nan_values && !c->ext_rec_in && !c->ext_rec_out && !c->ext_vals_out && !c->rec_external &&
                                   t >= c->plan_t0 && t < c->plan_t0 + c->plan_w && c->cone_big_ok[(size_t)(t - c->plan_t0)] != 0u;
            if (cone_next || (c->F.inline_walk && !(c->F.gen_keys && (c->deep_plan || c->nan_values))) ||
                (c->F.defer_resolve && c->persist_on && !c->persist_broken && !c->in_repair && !c->nan_values)) {   // (the key form has no second walk to fall back to)
                c->run.unresolved = true;   // resolved in the prologue of the next chain kernel (or by resolve_now)
            } else {
                if (kscoped) c->pev_exch[slot] = 1;
                const KernelEvents stamped(c, kscoped, 4 * slot + 2);
                launch_resolve(c, t, (c->F.plan == PLAN_LDS || c->F.xk == XK_ROWS || c->F.xk == XK_KEY) ? nullptr : c->rec[c->run.cur]);
            }
            c->run.pending = true;
        }
        if (c->profiling && !kscoped) { HIPCHK(hipEventRecord(c->pev[4 * slot + 2], c->stream)); HIPCHK(hipEventRecord(c->pev[4 * slot + 3], c->stream)); }
        c->run.iter = t; c->run.exch_done = false;
        ++slot; ++it;
    }
    if (c->profiling) c->pev_iters = slot;
}

// A launch of the persistent kernel ended with the error word set (a hard error of the algorithm, AlgoBGP.jl:341,409 — or a tile gave
// up waiting).  Its tiles do not stop at the failing iteration, so: the state of before (persist_snapshot), the history rows of the
// iterations since filled as the constructor fills them, the error word cleared, and the same iterations again, one launch each —
// that path stops at the failing iteration with the documented state (include/smmhip.h), or runs through if the failure was the form's.
void persist_repair(Ctx* c, int n_replay) {
    KParams& P = c->P;
    const size_t N = P.N;
    const int n = n_replay >= 0 ? std::min(n_replay, c->run.iter - c->snap.iter) : c->run.iter - c->snap.iter;
    c->in_repair = true;
    ++c->persist_repairs;
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(P.cs, c->snap_cs, N * CSW * 8, hipMemcpyDeviceToDevice));
    HIPCHK(hipMemcpy(c->rec[c->snap.cur], c->snap_rec, N * P.RW * 8, hipMemcpyDeviceToDevice));
    for (int b = 0; b < 2; ++b) {
        HIPCHK(hipMemcpy(c->vals_buf[b], c->snap_vals[b], (N + 4) * 8, hipMemcpyDeviceToDevice));
        if (c->slot8_buf[b]) HIPCHK(hipMemcpy(c->slot8_buf[b], c->snap_slot8[b], (N + 4 + 128) * 8, hipMemcpyDeviceToDevice));
    }
    HIPCHK(hipMemcpy(P.xres, c->snap_xres, (size_t)P.Ng * 8, hipMemcpyDeviceToDevice));
    // (an exchanged chain's row of iteration snap.iter may have been rewritten by the first launch's prologue: the replay rewrites it identically)
    for (int t = c->snap.iter; t < c->run.iter; ++t)
        HIPCHK(hipMemcpy(P.hrec + (size_t)t * N * P.HW, c->hist_fill, N * P.HW * 8, hipMemcpyDeviceToDevice));
    const unsigned long long e = ERR_NONE;
    HIPCHK(hipMemcpy(P.err, &e, 8, hipMemcpyHostToDevice));
    c->run = c->snap;
    c->plan_w = 0; c->rng_w = 0; c->ps[0].w = c->ps[1].w = 0;   // (the windows are rebuilt: cheap, and nothing assumes where the failed run left them)
    // ... with the exchange of the snapshot's iteration still to be applied, its plan must be in the window the replay starts with: the
    // failed launches may have moved the window on (a step across a window boundary), and what enqueue_iterations does for an
    // iteration outside the window — resolve the pending exchange from "the window that just ended" — would read another window's plan
    if (c->run.unresolved) ensure_windows(c, c->run.iter);
    const int prof = c->profiling;
    c->profiling = 0;
    if (P.N < P.Ng) {   // a shard: the same iterations through the windows, one (or two) launches each — every rank does (smm_sync agrees on the error first)
        c->rec_external = false; c->pending_ext = false; c->p2p_current = false; c->p2p_unwaited = false;
        p2p_enqueue(c, n);
    } else enqueue_iterations(c, n);
    c->profiling = prof;
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    c->in_repair = false;
    c->snap_valid = false;
}
// calls that read or change the run's state other than by stepping: first make sure that what stands there is final (see persist_repair)
void settle_persist(Ctx* c) {
    if (!c->snap_valid) return;
    HIPCHK(hipStreamSynchronize(c->stream));
    (void)check_device_error(c);
}

// ---- a shard between its two states (smm_bgp_p2p_step) ----
// "p2p": the records after iteration `iter` are in the ranks' windows (rec_external), the exchange of `iter` not resolved yet (pending_ext);
// "plain": they are in the context's own array, as the persistent form reads and leaves them (unresolved: the exchange still pending).
// plain -> p2p: a publication.  With the exchange of `iter` still pending it travels as it is — a shard cannot settle it alone.
void p2p_publish(Ctx* c) {
    if (c->p2p_current) return;
    const bool carry = c->run.unresolved && c->P.N < c->P.Ng;
    if (!carry) flush(c);
    // the form is decided from what EVERY rank knows (population, objective, thresholds): a rank that looked at its own shard's
    // values here (an uploaded state with a NaN) could choose differently from its peers, and each side would wait for words the
    // other never sends.  A NaN in any shard reaches every window with the publication (in the slot words themselves, and the NaN word
    // tagged with the epoch): the rows form resolves such an iteration on the exact values inside its launch, the inline form
    // (N_global <= 8192) reports it — on every rank, in the same iteration (include/smmhip.h).
    c->p2p_mode_inline = c->p2p_inline || c->p2p_rows;
    c->P.p2p_epoch += 1;   // (a new generation of tags: words of an earlier publication are nobody's any more)
    launch_p2p_push(c, c->run.iter, c->rec[c->run.cur], c->p2p_mode_inline);
    c->p2p_current = true;
    c->pending_ext = false;
    if (carry) { c->pending_ext = true; c->rec_external = true; c->run.pending = false; c->run.unresolved = false; }
}
// p2p -> plain: this rank's own records after iteration `iter` out of its window into the context's array (its own stores: complete)
void p2p_to_plain(Ctx* c) {
    if (!c->p2p_current) return;
    const KParams& P = c->P;
    const P2PLayout L = p2p_layout(P.Ng, P.RW);
    if (c->p2p_mode_inline)
        hipLaunchKernelGGL(k_p2p_own_records, dim3((unsigned)((P.N * P.RW + 255) / 256)), dim3(256), 0, c->stream, P, c->run.iter, c->rec[c->run.cur]);
    else
        HIPCHK(hipMemcpyAsync(c->rec[c->run.cur], (const double*)(c->p2p_mine + L.rec[c->run.iter & 1]) + (size_t)P.offset * P.RW, (size_t)P.N * P.RW * 8,
                              hipMemcpyDeviceToDevice, c->stream));
    c->run.unresolved = c->pending_ext; c->run.pending = c->pending_ext;
    c->pending_ext = false; c->rec_external = false; c->p2p_current = false; c->p2p_unwaited = false;
}

// n iterations of a shard onto the stream (smm_bgp_p2p_step; persist_repair with the persistent form off)
void p2p_enqueue(Ctx* c, int n_iters) {
    KParams& P = c->P;
    const P2PLayout L = p2p_layout(P.Ng, P.RW);
    int slot = 0;   // profiling: events of this launch
    for (int it = 0; it < n_iters; ++it) {
        if (persist_sh_usable(c, n_iters - it)) {   // as many of the remaining iterations as the look-ahead windows hold, in ONE launch
            p2p_to_plain(c);
            int n = 0;
            {
                const KernelEvents stamped(c, c->profiling == 2, 4 * slot);
                n = launch_chain_persist(c, n_iters - it);
            }
            if (n > 0) {
                advanced_by_persist(c, n);
                it += n - 1; ++slot;
                continue;
            }
        }
        p2p_publish(c);
        const int t = c->run.iter + 1;
        const bool prof = c->profiling == 2;
        int flags = (c->run.prev_open ? F_CLOSE_PREV : 0) | F_GLOBAL_REC;
        if (c->p2p_mode_inline) {
            if (c->pending_ext) {
                flags |= F_HAS_PENDING;
                // the walk of iteration t-1 needs that iteration's plan: where the plan window is about to move on, the
                // exchange is resolved by the stand-alone kernel first (once per window of 256 iterations)
                if (c->p2p_rows) {
                    if (prof) c->pev_exch[slot] = 1;
                    {
                        const KernelEvents stamped(c, prof, 4 * slot + 2);
                        launch_resolve_rows_window(c, t - 1);
                    }
#ifdef SMM_TEST_HOOKS
                    if (c->H.rows_win_check) {   // the same exchange through the unpacked values and the plain kernels
                        std::vector<unsigned long long> a((size_t)P.Ng), b((size_t)P.Ng);
                        HIPCHK(hipStreamSynchronize(c->stream));
                        HIPCHK(hipMemcpy(a.data(), P.xres, a.size() * 8, hipMemcpyDeviceToHost));
                        launch_p2p_unpack(c, t - 1);
                        launch_resolve_window(c, t - 1);
                        HIPCHK(hipStreamSynchronize(c->stream));
                        HIPCHK(hipMemcpy(b.data(), P.xres, b.size() * 8, hipMemcpyDeviceToHost));
                        int bad = 0;
                        for (int g = 0; g < P.Ng; ++g)
                            if (a[g] != b[g] && bad++ < 8) fprintf(stderr, "rows window check: iteration %d chain %d: %llx != %llx\n", t - 1, g, a[g], b[g]);
                        fprintf(stderr, "rows window check: iteration %d: %d of %d differ\n", t - 1, bad, P.Ng);
                    }
#endif
                } else if (t >= c->plan_t0 && t < c->plan_t0 + c->plan_w) flags |= F_WALK_INLINE;
                else {
                    launch_p2p_unpack(c, t - 1);
                    launch_resolve_window(c, t - 1);
                }
            }
            ensure_windows(c, t);
            const KernelEvents stamped(c, prof, 4 * slot);
            launch_chain_iter_norm_p2p(c, t, flags);
        } else {
            if (c->pending_ext) {   // exchangeMoves! of iteration t-1 (before its plan window can move on)
                if (c->p2p_unwaited) launch_p2p_wait(c);
                const bool xprof = prof && resolve_stamped(c, true);
                if (xprof) c->pev_exch[slot] = 1;
                const KernelEvents stamped(c, xprof, 4 * slot + 2);
                launch_resolve_window(c, t - 1);
                flags |= F_HAS_PENDING;
            }
            ensure_windows(c, t);
            {
                const ExternalRecords window(c, (const double*)(c->p2p_mine + L.rec[(t - 1) & 1]), (double*)(c->p2p_mine + L.rec[t & 1]) + (size_t)P.offset * P.RW,
                                             (double*)(c->p2p_mine + L.val[t & 1]) + P.offset);
                const KernelEvents stamped(c, prof, 4 * slot);
                launch_chain_iter(c, t, flags);
            }
            launch_p2p_push(c, t, nullptr, false);
        }
        c->run.prev_open = true;
        c->run.pending = false;
        c->rec_external = true;
        c->pending_ext = exchange_active(c, t);
        c->run.iter = t; c->run.exch_done = false;
        ++slot;
    }
    HIPCHK(hipEventRecord(c->ev1, c->stream));
    HIPCHK(hipGetLastError());
    if (c->profiling == 2) c->pev_iters = slot;
}

}  // namespace

extern "C" {

int smm_sync(void* ctx) {
    return api_call(ctx, true, [&](Ctx* c) -> int {
        HIPCHK(hipSetDevice(c->device));
        HIPCHK(hipStreamSynchronize(c->stream));
        if (c->pending_timing) {
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
            c->timing.step_ms = ms;
            c->pending_timing = false;
            c->timing.iter_kernel_ms = 0.0;
            c->timing.exch_kernel_ms = 0.0;
            c->timing.null_bracket_ms = 0.0;
            for (int i = 0; i < c->pev_iters; ++i) {
                float a = 0.f, b = 0.f, n = 0.f;
                HIPCHK(hipEventElapsedTime(&a, c->pev[4 * i], c->pev[4 * i + 1]));
                if (c->profiling == 2) {
                    if (c->pev_exch[i]) HIPCHK(hipEventElapsedTime(&b, c->pev[4 * i + 2], c->pev[4 * i + 3]));
                } else {
                    HIPCHK(hipEventElapsedTime(&b, c->pev[4 * i + 1], c->pev[4 * i + 2]));
                    HIPCHK(hipEventElapsedTime(&n, c->pev[4 * i + 2], c->pev[4 * i + 3]));
                }
                c->timing.iter_kernel_ms += a;
                c->timing.exch_kernel_ms += b;
                c->timing.null_bracket_ms += n;
            }
            c->pev_iters = 0;
        }
        return told(c, check_device_error(c));
    });
}

int smm_bgp_step_async(void* ctx, int32_t n_iters) {
    return api_call(ctx, n_iters >= 0, [&](Ctx* c) -> int {
        if (c->failed) return told(c);
        if (c->P.N != c->P.Ng) return fail(c, SMM_ERR_STATE, "smm_bgp_step needs a single shard (N == N_global); use the sharded calls");
        if (c->run.iter + n_iters > c->P.T) return beyond_maxiter(c);
        if (c->rec_external) return in_gather_buffer(c);
        HIPCHK(hipSetDevice(c->device));
        if (c->profiling) {
            profiling_events(c, n_iters);
            c->pev_exch.assign((size_t)n_iters, 0);
        }
        c->pev_iters = 0;
        HIPCHK(hipEventRecord(c->ev0, c->stream));
        enqueue_iterations(c, n_iters);
        HIPCHK(hipEventRecord(c->ev1, c->stream));
        HIPCHK(hipGetLastError());
        c->pending_timing = true;
        c->timing.iters = n_iters;
        c->timing.chain_evals = (int64_t)n_iters * c->P.N;
        return SMM_OK;
    });
}

int smm_bgp_step(void* ctx, int32_t n_iters) {
    const int rc = smm_bgp_step_async(ctx, n_iters);
    if (rc != SMM_OK) return rc;
    return smm_sync(ctx);
}

int smm_bgp_local_step(void* ctx) {
    return api_call(ctx, true, [&](Ctx* c) -> int {
        if (c->failed) return told(c);
        if (c->rec_external) return in_gather_buffer(c);
        if (c->a2a_open) return fail(c, SMM_ERR_STATE, "smm_bgp_a2a_pack_dev without smm_bgp_a2a_apply_dev: the exchange of this iteration would be dropped");
        if (c->run.iter + 1 > c->P.T) return beyond_maxiter(c);
        if (const int rc = settled(c)) return rc;
        const int t = c->run.iter + 1;
        // smm_bgp_step leaves the exchange of its last iteration to the next chain kernel (inline walk): the three-phase
        // form reads P.xres, so resolve it now (local_step after step read an unresolved xres)
        resolve_now(c);
        ensure_windows(c, t);
        const int flags = (c->run.prev_open ? F_CLOSE_PREV : 0) | (c->run.pending ? F_HAS_PENDING : 0);
        launch_chain_iter(c, t, flags);
        HIPCHK(hipGetLastError());
        c->run.prev_open = true;
        c->run.pending = false;
        c->run.iter = t; c->run.exch_done = false;
        return SMM_OK;
    });
}

// Sharded iteration in two enqueues (instead of local_step / export / exchange = five): the exchange of the previous
// iteration is resolved from gathered_prev, the chain kernel takes every chain's continuation record (its own or the
// donor's) straight from gathered_prev and writes the new records into this shard's slice of gathered_next.
int smm_bgp_sharded_step(void* ctx, const void* gathered_prev_dev, void* gathered_next_dev) {
    return api_call(ctx, gathered_next_dev != nullptr, [&](Ctx* c) -> int {
        if (c->failed) return told(c);
        if (c->run.iter + 1 > c->P.T) return beyond_maxiter(c);
        if (c->rec_external && !gathered_prev_dev) return fail(c, SMM_ERR_INVALID_ARG, "gathered_prev required: the last records live there");
        if (c->run.unresolved) return fail(c, SMM_ERR_STATE, "mixing smm_bgp_step and smm_bgp_sharded_step without a flush");
        if (c->p2p_current) return in_p2p_windows(c);
        if (const int rc = settled(c)) return rc;
        const int t = c->run.iter + 1;
        const KParams& P = c->P;
        int flags = (c->run.prev_open ? F_CLOSE_PREV : 0);
        // profiling mode 2: this call is one more iteration of the "step" smm_sync sums up (the kernels' own begin/end stamps)
        const bool prof = c->profiling == 2;
        const int it = c->pev_iters;
        if (prof) {
            profiling_events(c, it + 1);
            c->pev_exch.resize((size_t)it + 1, 0);
            c->pev_exch[it] = 0;
            if (it == 0) HIPCHK(hipEventRecord(c->ev0, c->stream));
        }
        const double* donors = nullptr;   // (null: the chains continue from the context's own records)
        if (c->rec_external) {
            if (c->pending_ext) {   // exchangeMoves! of iteration t-1 over the gathered records (before its plan window can move on)
                const bool xprof = prof && resolve_stamped(c, true);
                if (xprof) c->pev_exch[it] = 1;
                const KernelEvents stamped(c, xprof, 4 * it + 2);
                launch_resolve(c, t - 1, (const double*)gathered_prev_dev);
                flags |= F_HAS_PENDING;
            }
            flags |= F_GLOBAL_REC;
            donors = (const double*)gathered_prev_dev;
        } else if (c->run.pending) {
            flags |= F_HAS_PENDING;   // resolved earlier through the three-phase calls
        }
        ensure_windows(c, t);
        {
            const ExternalRecords gathered(c, donors, (double*)gathered_next_dev + (size_t)P.offset * P.RW);
            const KernelEvents stamped(c, prof, 4 * it);
            launch_chain_iter(c, t, flags);
        }
        if (prof) {
            HIPCHK(hipEventRecord(c->ev1, c->stream));
            c->pev_iters = it + 1;
            c->pending_timing = true;
            c->timing.iters = it + 1;
            c->timing.chain_evals = (int64_t)(it + 1) * P.N;
        }
        HIPCHK(hipGetLastError());
        c->run.prev_open = true;
        c->run.pending = false;
        c->rec_external = true;
        c->pending_ext = exchange_active(c, t);
        c->run.iter = t; c->run.exch_done = false;
        return SMM_OK;
    });
}

// settle the last sharded_step: resolve its exchange from the gathered records and bring records, history and
// counters into the context (afterwards history/state can be read, or stepping continues in either form)
int smm_bgp_sharded_finish(void* ctx, const void* gathered_dev) {
    return api_call(ctx, true, [&](Ctx* c) -> int {
        if (!c->rec_external) return SMM_OK;
        if (!gathered_dev) return SMM_ERR_INVALID_ARG;
        if (c->p2p_current) return in_p2p_windows(c);
        if (const int rc = settled(c)) return rc;
        int flags = (c->run.prev_open ? F_CLOSE_PREV : 0) | F_GLOBAL_REC;
        if (c->pending_ext) {
            launch_resolve(c, c->run.iter, (const double*)gathered_dev);
            flags |= F_HAS_PENDING;
        }
        launch_flush(c, (const double*)gathered_dev, flags);
        HIPCHK(hipGetLastError());
        c->run.cur ^= 1;
        c->run.pending = false; c->run.prev_open = false; c->rec_external = false; c->pending_ext = false;
        return SMM_OK;
    });
}

int smm_bgp_p2p_init(void* ctx, void* ipc_handle_out, void** window_dev_out) {
    return api_call(ctx, true, [&](Ctx* c) -> int {
        if (c->a2a_G < 1) return fail(c, SMM_ERR_STATE, "the p2p form needs equal shards (N_global a multiple of N, chain_offset a multiple of N)");
        if (c->a2a_G > P2P_MAXG) return fail(c, SMM_ERR_INVALID_ARG, "the p2p form serves up to 8 ranks (one node)");
        HIPCHK(hipSetDevice(c->device));
        KParams& P = c->P;
        const P2PLayout L = p2p_layout(P.Ng, P.RW);
        if (!c->p2p_mine) {
            // Plain device memory — what the receive buffers of the collective libraries are.  (An UNCACHED allocation,
            // hipDeviceMallocUncached, looked like the natural choice and was the first one: it passed every test of its own file and
            // failed in the full suite, in both forms, whenever the process had run other contexts before — later kernels were served
            // lines that an earlier allocation at the same address had left behind; the cache maintenance at kernel boundaries, which
            // plain memory gets, does not seem to cover it.  Within a launch nothing relies on the caches: stores into a window are
            // system-scope stores, self-validating words are re-read past the caches until their tag is the wanted one.)
            // (a shard that can run the persistent form keeps its ring behind the p2p window proper: one allocation, one IPC handle)
            size_t total = L.total;
            if (c->F.persist_sh) {
                c->prw_off = (L.total + 255) & ~(size_t)255;
                total = c->prw_off + pr_win_layout(P.Ng, P.RW, c->a2a_G, persist_tiles_rank(c->F, c->P.N)).total;   // (the ring: RW granules of this context's records)
            }
            void* w = nullptr;
            HIPCHK(hipMalloc(&w, total));
            c->p2p_mine = (unsigned char*)w;
            HIPCHK(hipMemset(w, 0, total));
            HIPCHK(hipDeviceSynchronize());
            P.p2p_G = c->a2a_G;
            P.p2p_rank = P.offset / P.N;
            for (int r = 0; r < P2P_MAXG; ++r) P.p2p_win[r] = nullptr;
            P.p2p_win[P.p2p_rank] = c->p2p_mine;
            P.p2p_self = c->p2p_mine;
            for (int b = 0; b < 2; ++b) {
                P.p2p_off[b] = (uint32_t)L.rec[b]; P.p2p_off[2 + b] = (uint32_t)L.val[b]; P.p2p_off[4 + b] = (uint32_t)L.slot[b];
                P.p2p_off[6 + b] = (uint32_t)L.llrec[b]; P.p2p_off[8 + b] = (uint32_t)L.llval[b];
                P.p2p_off[10 + b] = (uint32_t)L.slot4[b];
            }
            if (L.total >= ((size_t)1 << 32)) throw std::string("p2p window larger than 4 GiB");
            c->p2p_attached = 1u << P.p2p_rank;
            c->p2p_seq = 0;
            c->p2p_current = false;
            // one launch per iteration (the lean key walk in the chain kernel's prologue, the push in its epilogue) where the
            // single shard has it too: objfunc_norm with np == nm <= 4, min_improve == 0, N_global <= 8192
            c->p2p_inline = c->F.norm_fast && c->F.lean_plan && !P.lean_wide && P.Ng <= XLDS_MAX && P.plan_K <= XLDS_MAX && !c->deep_plan &&
                            P.dist_fun == SMM_DIST_MINUS && p2p_walk_bytes(c) + norm_tile_doubles(P.np) * 8 <= (size_t)160 * 1024;
            // two launches per iteration for the large norm populations (8192 < N_global <= 32768, min_improve == 0: BASELINE
            // configs[2], 4 and 8 shards of 4096): k_exch_resolve_rows reads the window's tagged slots itself, the chain kernel
            // pushes from its epilogue like the inline form's
            c->p2p_rows = c->F.norm_fast && !c->p2p_inline && c->F.xk == XK_ROWS;
        }
        if (ipc_handle_out) {
            hipIpcMemHandle_t h;
            HIPCHK(hipIpcGetMemHandle(&h, c->p2p_mine));
            static_assert(sizeof(hipIpcMemHandle_t) == SMM_P2P_HANDLE_BYTES, "hipIpcMemHandle_t is 64 bytes");
            memcpy(ipc_handle_out, &h, sizeof h);
        }
        if (window_dev_out) *window_dev_out = c->p2p_mine;
        return SMM_OK;
    });
}

int smm_bgp_p2p_attach(void* ctx, int32_t rank, const void* ipc_handle, void* window_dev) {
    return api_call(ctx, (!ipc_handle) != (!window_dev), [&](Ctx* c) -> int {
        if (!c->p2p_mine) return p2p_init_first(c);
        if (rank < 0 || rank >= c->P.p2p_G || rank == c->P.p2p_rank) return fail(c, SMM_ERR_INVALID_ARG, "smm_bgp_p2p_attach: rank of ANOTHER shard, 0 <= rank < N_global / N");
        if (c->p2p_attached & (1u << rank)) return fail(c, SMM_ERR_STATE, "smm_bgp_p2p_attach: this rank's window is attached already");
        HIPCHK(hipSetDevice(c->device));
        void* w = window_dev;
        if (ipc_handle) {
            hipIpcMemHandle_t h;
            memcpy(&h, ipc_handle, sizeof h);
            HIPCHK(hipIpcOpenMemHandle(&w, h, hipIpcMemLazyEnablePeerAccess));
            c->p2p_opened[rank] = w;
            // (a peer PROCESS on this very device — several ranks on one GPU, the tests' way: its tiles compete with this rank's for
            // the compute units, and the persistent form needs all of them resident at once)
            hipPointerAttribute_t at;
            if (hipPointerGetAttributes(&at, w) == hipSuccess && at.device == c->device) c->p2p_ranks_here += 1;
            (void)hipGetLastError();
        } else {   // a context of this process: on another device the two must see each other
            hipPointerAttribute_t at;
            HIPCHK(hipPointerGetAttributes(&at, w));
            if (at.device == c->device) c->p2p_ranks_here += 1;
            if (at.device != c->device) {
                const hipError_t e = hipDeviceEnablePeerAccess(at.device, 0);
                if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) HIPCHK(e);
                (void)hipGetLastError();
            }
        }
        c->P.p2p_win[rank] = (unsigned char*)w;
        c->p2p_attached |= 1u << rank;
        return SMM_OK;
    });
}

int smm_bgp_p2p_step(void* ctx, int32_t n_iters) {
    return api_call(ctx, n_iters >= 0, [&](Ctx* c) -> int {
        if (c->failed) return told(c);
        if (!c->p2p_mine) return p2p_init_first(c);
        if (c->p2p_attached != (1u << c->P.p2p_G) - 1u) return fail(c, SMM_ERR_STATE, "smm_bgp_p2p_step: not every rank's window is attached");
        if (c->run.iter + n_iters > c->P.T) return beyond_maxiter(c);
        if (c->rec_external && !c->p2p_current) return in_gather_buffer(c);
        if (c->a2a_open) return fail(c, SMM_ERR_STATE, "smm_bgp_a2a_apply_dev comes first");
        HIPCHK(hipSetDevice(c->device));
        // (launches of the persistent form that this step simply continues are looked at — and agreed upon by the ranks — when the run is
        // synchronised, not between two steps: the host stays out of the way)
        if (!(!c->p2p_current && persist_sh_usable(c, n_iters))) settle_persist(c);
        if (c->failed) return told(c);
        KParams& P = c->P;
        if (c->profiling == 2) {
            profiling_events(c, n_iters);
            c->pev_exch.assign((size_t)n_iters, 0);
        }
        c->pev_iters = 0;
        HIPCHK(hipEventRecord(c->ev0, c->stream));
        p2p_enqueue(c, n_iters);
        c->pending_timing = true;
        c->timing.iters = n_iters;
        c->timing.chain_evals = (int64_t)n_iters * P.N;
        return SMM_OK;
    });
}

// settle the last p2p step (its exchange, history, counters) into the context, like smm_bgp_sharded_finish
int smm_bgp_p2p_finish(void* ctx) {
    return api_call(ctx, true, [&](Ctx* c) -> int {
        if (c->p2p_current && !c->rec_external) return SMM_OK;
        if (!c->p2p_current && !(c->p2p_mine && c->run.unresolved && c->P.N < c->P.Ng)) return SMM_OK;
        if (const int rc = settled(c)) return rc;
        p2p_publish(c);   // (behind a launch of the persistent form: the records after `iter` into the windows, their exchange still to be resolved)
        const KParams& P = c->P;
        const P2PLayout L = p2p_layout(P.Ng, P.RW);
        int flags = (c->run.prev_open ? F_CLOSE_PREV : 0) | F_GLOBAL_REC;
        // the donors' records of the last iteration must have landed, in plain form
        if (c->p2p_mode_inline) launch_p2p_unpack(c, c->run.iter);
        else if (c->p2p_unwaited) launch_p2p_wait(c);
        if (c->pending_ext) {
            launch_resolve_window(c, c->run.iter);
            flags |= F_HAS_PENDING;
        }
        launch_flush(c, (const double*)(c->p2p_mine + L.rec[c->run.iter & 1]), flags);
        HIPCHK(hipGetLastError());
        c->run.cur ^= 1;
        c->run.pending = false; c->run.prev_open = false; c->rec_external = false; c->pending_ext = false; c->p2p_current = false;
        return SMM_OK;
    });
}

int smm_bgp_record_doubles(void* ctx) {
    Ctx* c = (Ctx*)ctx;
    return c ? c->P.RW : SMM_ERR_INVALID_ARG;
}

int smm_bgp_export_records_dev(void* ctx, void* rec_dev) {
    return api_call(ctx, rec_dev != nullptr, [&](Ctx* c) -> int {
        if (c->failed) return told(c);
        if (c->rec_external) return in_gather_buffer(c);
        if (const int rc = settled(c)) return rc;
        // after smm_bgp_step the exchange of the last iteration is still pending (resolved or not): the exported records must
        // be the ones AFTER that exchange, as the three-phase protocol defines them
        if (c->run.pending || c->run.unresolved) flush(c);
        HIPCHK(hipMemcpyAsync(rec_dev, c->rec[c->run.cur], (size_t)c->P.RW * c->P.N * sizeof(double), hipMemcpyDeviceToDevice,
                              c->stream));
        return SMM_OK;
    });
}

int smm_bgp_exchange_dev(void* ctx, const void* gathered_dev) {
    return api_call(ctx, gathered_dev != nullptr, [&](Ctx* c) -> int {
        if (c->failed) return told(c);
        if (c->run.iter < 1) return before_first_local_step(c);
        if (c->run.pending || c->run.exch_done || c->a2a_open) return already_resolved(c);
        if (const int rc = settled(c)) return rc;
        c->run.exch_done = true;
        if (exchange_active(c, c->run.iter)) {
            const KParams& P = c->P;
            launch_resolve(c, c->run.iter, (const double*)gathered_dev);
            launch_exch(c, XI_APPLY, dim3((P.N + 255) / 256), 0, c->stream, P, c->run.iter, (const double*)gathered_dev, c->rec[c->run.cur]);
        }
        HIPCHK(hipGetLastError());
        return SMM_OK;
    });
}

// ---- the values form of the sharded exchange (include/smmhip.h) ----
int smm_bgp_a2a_capacity(void* ctx) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return SMM_ERR_INVALID_ARG;
    return c->a2a_cap;
}

int smm_bgp_export_values_dev(void* ctx, void* vals_dev) {
    return api_call(ctx, vals_dev != nullptr, [&](Ctx* c) -> int {
        if (c->failed) return told(c);
        if (c->rec_external) return in_gather_buffer(c);
        if (c->run.iter < 1) return fail(c, SMM_ERR_STATE, "no iteration yet");
        if (const int rc = settled(c)) return rc;
        if (c->run.pending || c->run.unresolved) flush(c);
        HIPCHK(hipMemcpyAsync(vals_dev, c->vals_buf[c->run.iter & 1], (size_t)c->P.N * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        return SMM_OK;
    });
}

int smm_bgp_a2a_pack_dev(void* ctx, const void* vals_all_dev, void* send_dev) {
    return api_call(ctx, vals_all_dev && send_dev, [&](Ctx* c) -> int {
        if (c->failed) return told(c);
        if (c->a2a_cap <= 0) return fail(c, SMM_ERR_STATE, "the values form needs equal shards (N_global a multiple of N, chain_offset a multiple of N)");
        if (c->run.iter < 1) return before_first_local_step(c);
        if (c->run.pending || c->a2a_open || c->run.exch_done) return already_resolved(c);
        if (const int rc = settled(c)) return rc;
        if (exchange_active(c, c->run.iter)) {
            KParams P1 = c->P;
            P1.RW = 1;   // (the resolve kernels read value s at gathered[s * RW])
            launch_resolve_p(c, P1, c->run.iter, (const double*)vals_all_dev);
            const KParams& P = c->P;
            hipLaunchKernelGGL(k_a2a_index, dim3(c->a2a_G), dim3(XWG), 0, c->stream, P, c->run.iter, c->a2a_G, c->a2a_cap, c->a2a_send_idx,
                               c->a2a_send_cnt, c->a2a_rowidx);
            const size_t ne = (size_t)c->a2a_G * c->a2a_cap * P.RW;
            hipLaunchKernelGGL(k_a2a_pack, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, c->stream, P, c->a2a_G, c->a2a_cap,
                               (const int32_t*)c->a2a_send_idx, (const int32_t*)c->a2a_send_cnt, (const double*)c->rec[c->run.cur], (double*)send_dev);
        }
        HIPCHK(hipGetLastError());
        c->a2a_open = true;
        return SMM_OK;
    });
}

int smm_bgp_a2a_apply_dev(void* ctx, const void* recv_dev) {
    return api_call(ctx, recv_dev != nullptr, [&](Ctx* c) -> int {
        if (c->failed) return told(c);
        if (!c->a2a_open) return fail(c, SMM_ERR_STATE, "smm_bgp_a2a_pack_dev comes first");
        if (const int rc = settled(c)) return rc;
        if (exchange_active(c, c->run.iter)) {
            const KParams& P = c->P;
            hipLaunchKernelGGL(k_a2a_apply, dim3((P.N + 255) / 256), dim3(256), 0, c->stream, P, c->run.iter, (const double*)recv_dev,
                               (const int32_t*)c->a2a_rowidx, c->rec[c->run.cur]);
        }
        HIPCHK(hipGetLastError());
        c->a2a_open = false;
        c->run.exch_done = true;
        return SMM_OK;
    });
}

}  // extern "C"
