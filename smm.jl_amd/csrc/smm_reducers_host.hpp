// the host side of the history reducers — part of libsmmhip (included once by smmhip.hip, behind its host helpers; hiprtc never sees it).
// The family: smm_get_chain_stats, smm_get_chain_cov, smm_get_proposal / _set_ / _adapt_, smm_get_chain_diag, smm_get_group_stats,
// smm_get_histogram, smm_get_trace, smm_get_rank_diag, smm_get_draws, smm_get_moment_stats, smm_get_adjustment, smm_get_reweighted,
// smm_get_profile, smm_get_density, smm_get_derived (kernels:
// smm_stats.hpp, smm_cov.hpp, smm_diag.hpp, smm_group.hpp, smm_moments.hpp, smm_adjust.hpp, smm_reweight.hpp, smm_hist.hpp, smm_trace.hpp, smm_rank.hpp,
// smm_draws.hpp, smm_profile.hpp, smm_density.hpp, smm_derived.hpp and, around a user's transform, smm_user_host.hpp's kernel text;
// the walk over a chain's window that their gathers share: smm_window.hpp).
// What they share is stated here once: the frame of a call (api_call of smmhip.hip), the checks of the arguments they have in common (check_groups,
// check_probs, check_select), the prelude and the window behind them (settled_window: reader_prelude and check_window of smmhip.hip), the
// members of the groups (Groups), one result buffer per context (reducer_result, laid out by Carve / Slice, copied by up / down), one
// scratch per context for the compacted columns (reducer_scratch, chain_batches), the cap on the scratch and on a batch of results
// (reducer_batch_cap: REDUCER_BATCH_CAP, or what the test seam SMMHIP_STATS_SCRATCH gives, so that small cases reach the batched paths),
// and the pooled columns of groups: the members' counts, where the pooled rows and their chunks lie, the plan of the order statistics,
// both on the device and the order statistics' launches (pool_counts, PoolPlan, OrderPlan, PoolDev, pool_order).
// A call's own batch plan, result layout, launches, empty-window branch and host-side finish stay in the call.
#pragma once

namespace {

static_assert(STATS_WG == WINDOW_WG && DIAG_WG == WINDOW_WG && HIST_WG == WINDOW_WG && TRACE_WG == WINDOW_WG && DRAWS_WG == WINDOW_WG &&
                  PROF_WG == WINDOW_WG && RANK_WG == WINDOW_WG && WINDOW_WG == 256,
              "smm_window.hpp walks a window 256 rows at a time, four waves' totals through LDS; k_draws_mask splits a tile over four waves");

// the prelude, then the window: what a call over a window does once its arguments have passed
int settled_window(Ctx* c, int t0, int t1) { reader_prelude(c); return check_window(c, t0, t1); }

// the group vector [N] (-1: in no group) and its count; without a vector GROUPS_OPTIONAL is no group at all (the diagnostics: no R-hat),
// GROUPS_DEFAULT_ONE every chain in one group
enum GroupNull { GROUPS_OPTIONAL, GROUPS_DEFAULT_ONE };
int check_groups(Ctx* c, const int32_t* group, int n_groups, GroupNull null_is) {
    if (null_is == GROUPS_OPTIONAL) {
        if (n_groups < 0 || (n_groups > 0 && !group)) return fail(c, SMM_ERR_INVALID_ARG, "n_groups < 0, or group NULL with n_groups > 0");
    } else if (n_groups < 0 || (!group && n_groups != 1))
        return fail(c, SMM_ERR_INVALID_ARG, "n_groups < 0, or group NULL with n_groups != 1");
    for (int i = 0; group && i < c->P.N; ++i)
        if (group[i] < -1 || group[i] >= n_groups) return fail(c, SMM_ERR_INVALID_ARG, "a group id outside [-1, n_groups)");
    return SMM_OK;
}

int check_probs(Ctx* c, const double* probs, int n_probs, bool wants_quantile) {
    if (n_probs < 0 || (n_probs > 0 && !probs)) return fail(c, SMM_ERR_INVALID_ARG, "n_probs < 0, or probs NULL with n_probs > 0");
    if (wants_quantile && n_probs == 0) return fail(c, SMM_ERR_INVALID_ARG, "quantile requested without probs");
    for (int p = 0; p < n_probs; ++p)
        if (!(probs[p] >= 0.0 && probs[p] <= 1.0)) return fail(c, SMM_ERR_INVALID_ARG, "probs must lie in [0, 1]");
    return SMM_OK;
}

int check_select(Ctx* c, int select) {
    return select < 0 || select > 2 ? fail(c, SMM_ERR_INVALID_ARG, "select must be 0 (all), 1 (accepted) or 2 (state)") : SMM_OK;
}

// the groups of a checked group vector (NULL: every chain in group 0)
struct Groups {
    std::vector<int> gid;          // [N] each local chain's group, -1: none
    std::vector<int> n_chains;     // [G] members per group
    std::vector<int> gmem0, mem;   // group g's members are mem[gmem0[g] .. gmem0[g + 1]), in ascending local index
    int M = 0, longest = 0;        // members of all groups, and of the largest
};
Groups group_members(const int32_t* group, size_t G, size_t N) {
    Groups g;
    g.gid.assign(N, 0);
    if (group) std::copy(group, group + N, g.gid.begin());
    g.n_chains.assign(G, 0);
    for (size_t i = 0; i < N; ++i)
        if (g.gid[i] >= 0) ++g.n_chains[g.gid[i]];
    g.gmem0.assign(G + 1, 0);
    for (size_t k = 0; k < G; ++k) { g.gmem0[k + 1] = g.gmem0[k] + g.n_chains[k]; g.longest = std::max(g.longest, g.n_chains[k]); }
    g.M = g.gmem0[G];
    g.mem.resize(g.M);
    std::vector<int> at(g.gmem0.begin(), g.gmem0.end() - 1);
    for (size_t i = 0; i < N; ++i)
        if (g.gid[i] >= 0) g.mem[at[g.gid[i]]++] = (int)i;
    return g;
}

// the results of a reducer call on the device, one buffer grown to the largest call's
void* reducer_result(Ctx* c, size_t bytes) {
    if (bytes > c->red_res_bytes) {
        if (c->red_res) { HIPCHK(hipFree(c->red_res)); c->red_res = nullptr; c->red_res_bytes = 0; }
        HIPCHK(hipMalloc(&c->red_res, bytes));
        c->red_res_bytes = bytes;
    }
    return c->red_res;
}

// a reducer's result layout, stated once: consecutive typed slices, placed in the device buffer and in its host copy alike
template <class T>
struct Slice {
    size_t off;
    T* in(void* base) const { return (T*)((char*)base + off); }
    Slice at(size_t n) const { return Slice{off + n * sizeof(T)}; }   // the slice from its n-th element on
};
struct Carve {
    size_t bytes = 0;
    template <class T>
    Slice<T> take(size_t n) { const Slice<T> s{bytes}; bytes += n * sizeof(T); return s; }
};

// count elements of a slice of the device buffer d from / to the host, on the context's stream; nothing where there is nothing to copy
template <class T>
void up(Ctx* c, void* d, Slice<T> sl, const void* src, size_t count) {
    if (src && count) HIPCHK(hipMemcpyAsync(sl.in(d), src, count * sizeof(T), hipMemcpyHostToDevice, c->stream));
}
template <class T>
void up(Ctx* c, void* d, Slice<T> sl, const std::vector<T>& v) { up(c, d, sl, v.data(), v.size()); }
template <class T>
void down(Ctx* c, void* d, Slice<T> sl, void* dst, size_t count) {
    if (dst && count) HIPCHK(hipMemcpyAsync(dst, sl.in(d), count * sizeof(T), hipMemcpyDeviceToHost, c->stream));
}

// bytes of the scratch and of a batch of results (the test seam SMMHIP_STATS_SCRATCH replaces the cap)
constexpr size_t REDUCER_BATCH_CAP = (size_t)256 << 20;
size_t reducer_batch_cap(const Ctx* c) { return c->H.stats_scratch ? c->H.stats_scratch : REDUCER_BATCH_CAP; }

// the compacted columns of every chain for the context's whole capacity, at most reducer_batch_cap (but always one parameter column +
// one partner column of maxiter draws: 12 x maxiter bytes)
size_t chain_stats_scratch_bytes(const Ctx* c) {
    const KParams& P = c->P;
    const size_t T = (size_t)P.T, all = (size_t)P.N * T * (8 * (size_t)P.np + 4);
    return std::min(all, std::max(reducer_batch_cap(c), 12 * T));
}

// the reducers' shared scratch st_scr: chain_stats_scratch_bytes, but never less than one_chain_bytes (one chain's columns of the whole
// capacity, for a reducer that takes them all at once; 0: no minimum).  One that is smaller is freed and allocated anew.
void reducer_scratch(Ctx* c, size_t one_chain_bytes) {
    if (c->st_scr && c->st_scr_bytes < one_chain_bytes) { HIPCHK(hipFree(c->st_scr)); c->st_scr = nullptr; c->st_scr_bytes = 0; }
    if (!c->st_scr) {
        c->st_scr_bytes = std::max(chain_stats_scratch_bytes(c), one_chain_bytes);
        HIPCHK(hipMalloc(&c->st_scr, c->st_scr_bytes));
    }
}

// the local chains in batches of as many as the scratch holds at per_chain bytes each: body(c0, nb)
template <class Body>
void chain_batches(Ctx* c, size_t per_chain, Body body) {
    const int N = c->P.N, Nb = (int)std::min((size_t)N, c->st_scr_bytes / per_chain);
    for (int c0 = 0; c0 < N; c0 += Nb) body(c0, std::min(Nb, N - c0));
}

// a reducer kernel onto the context's stream, its launch checked
template <class Kern, class... Args>
void launch_checked(Ctx* c, Kern kern, dim3 grid, dim3 block, size_t smem, const Args&... args) {
    hipLaunchKernelGGL(kern, grid, block, smem, c->stream, args...);
    HIPCHK(hipGetLastError());
}

// the keys a workgroup sorts in LDS for a column of n draws: the power of two at or above n (and 2), at most STATS_LDS_N
int sort_lds_n(int n) { return std::min(STATS_LDS_N, 1 << (int)ceil(log2((double)std::max(n, 2)))); }

// --- the pooled columns of groups (smm_group.hpp; smm_get_group_stats over the parameters, smm_get_moment_stats over the joint columns) ---

// the members' selected rows of the window [t0, t0 + n): k_group_gather's counting form for select 1, n otherwise.  dci [2][N] on the
// device gets the chains' groups, then these counts.
std::vector<int> pool_counts(Ctx* c, const Groups& grp, int t0, int n, int sel, int* dci) {
    const KParams& P = c->P;
    const size_t N = P.N;
    std::vector<int> cnt(N, n);
    HIPCHK(hipMemcpyAsync(dci, grp.gid.data(), N * 4, hipMemcpyHostToDevice, c->stream));
    if (sel == 1) {
        launch_checked(c, k_group_gather, dim3(N), dim3(STATS_WG), 0, (const double*)P.hrec, (int)N, P.HW, t0, n, 1, (const int*)dci,
                       (const long long*)nullptr, (const int*)nullptr, 0, 0, 0ll, 0, 0, (const double*)nullptr, 0, (double*)nullptr, dci + N, 1,
                       (int*)nullptr);
        HIPCHK(hipMemcpyAsync(cnt.data(), dci + N, N * 4, hipMemcpyDeviceToHost, c->stream));
    } else
        HIPCHK(hipMemcpyAsync(dci + N, cnt.data(), N * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return cnt;
}

// where the pooled rows lie: group g's column is rows [G0[g], G0[g] + gm[g]) of the pooled index space, its members one after another
// (member i from off[i], roff[i] within the group), cut into chunks of STATS_LDS_N rows from its own first row (chunk ch: clen[ch] rows
// from cst[ch]; group g's are [gch0[g], gch0[g + 1]), cch0[i] the first of member i's group)
struct PoolPlan {
    std::vector<long long> gm, G0, off, roff, cst;
    std::vector<int> clen, gch0, cch0;
    long long Mtot = 0;
    int NC = 0;
};
PoolPlan pool_plan(const Groups& grp, const std::vector<int>& cnt) {
    const size_t N = cnt.size(), G = grp.n_chains.size();
    const std::vector<int>& gid = grp.gid;
    PoolPlan p;
    p.gm.assign(G, 0); p.G0.assign(G + 1, 0); p.off.assign(N, 0); p.roff.assign(N, 0);
    p.gch0.assign(G + 1, 0); p.cch0.assign(N, 0);
    for (size_t i = 0; i < N; ++i)
        if (gid[i] >= 0) { p.roff[i] = p.gm[gid[i]]; p.gm[gid[i]] += cnt[i]; }
    for (size_t g = 0; g < G; ++g) {
        p.G0[g + 1] = p.G0[g] + p.gm[g];
        for (long long q = 0; q < p.gm[g]; q += STATS_LDS_N) {
            p.cst.push_back(p.G0[g] + q);
            p.clen.push_back((int)std::min<long long>(STATS_LDS_N, p.gm[g] - q));
        }
        p.gch0[g + 1] = (int)p.cst.size();
    }
    for (size_t i = 0; i < N; ++i)
        if (gid[i] >= 0) { p.off[i] = p.G0[gid[i]] + p.roff[i]; p.cch0[i] = p.gch0[gid[i]]; }
    p.Mtot = p.G0[G];
    p.NC = (int)p.cst.size();
    return p;
}

// the order statistics of the pooled columns: short columns (sgrp) sorted in LDS, the others (wgrp, the longest wmax) selected grid-wide
// at R ranks per column: rk [wgrp][R], the median's and stats_quantile's indexes of the nq probs (-1: unused)
struct OrderPlan {
    const double* probs; size_t nq;   // (the caller's, on the host)
    std::vector<int> sgrp, wgrp;
    long long wmax = 0;
    int R = 0;
    std::vector<long long> rk;
};
OrderPlan order_plan(const Ctx* c, const PoolPlan& pp, bool med, const double* probs, size_t nq) {
    OrderPlan o{probs, nq};
    for (size_t g = 0; g < pp.gm.size(); ++g)
        if (pp.gm[g] < c->H.group_wide_min) o.sgrp.push_back((int)g);
        else { o.wgrp.push_back((int)g); o.wmax = std::max(o.wmax, pp.gm[g]); }
    o.R = (med ? 2 : 0) + 2 * (int)nq;
    o.rk.assign(o.wgrp.size() * o.R, -1);
    for (size_t wi = 0; wi < o.wgrp.size() && o.R; ++wi) {
        const long long m = pp.gm[o.wgrp[wi]];
        long long* r = o.rk.data() + wi * o.R;
        if (med) { r[0] = (m & 1) ? m / 2 : m / 2 - 1; r[1] = (m & 1) ? -1 : m / 2; r += 2; }
        for (size_t p = 0; p < nq; ++p, r += 2) {
            const double h = (double)(m - 1) * probs[p];
            if (h >= (double)(m - 1)) r[0] = m - 1;
            else { r[0] = (long long)floor(h); r[1] = r[0] + 1; }
        }
    }
    return o;
}

// both plans on the device, and the grid-wide select's work space for nwc long columns at a time (their histograms WB columns at a
// time): carved behind the call's own 8-byte slices and ahead of its 4-byte ones, uploaded once the result buffer is there
struct PoolDev {
    Slice<double> probs;
    Slice<long long> off, G0, gm, cst, rk, rem;
    Slice<unsigned long long> pre, ghist;
    Slice<int> cch0, gch0, clen, sgrp, wgrp;
    int WB;
    PoolDev(Carve& Rv, const PoolPlan& pp, const OrderPlan& op, size_t nwc) {
        const size_t N = pp.off.size(), G = pp.gm.size(), R = op.R;
        WB = R ? (int)std::min(nwc, std::max((size_t)1, GROUP_HIST_CAP / (R * GROUP_BINS * 8))) : 0;
        probs = Rv.take<double>(op.nq);
        off = Rv.take<long long>(2 * N); G0 = Rv.take<long long>(G + 1); gm = Rv.take<long long>(G); cst = Rv.take<long long>(pp.NC);
        rk = Rv.take<long long>(op.rk.size()); rem = Rv.take<long long>(nwc * R);
        pre = Rv.take<unsigned long long>(nwc * R); ghist = Rv.take<unsigned long long>((size_t)WB * R * GROUP_BINS);
        cch0 = Rv.take<int>(N); gch0 = Rv.take<int>(G + 1); clen = Rv.take<int>(pp.NC);
        sgrp = Rv.take<int>(op.sgrp.size()); wgrp = Rv.take<int>(op.wgrp.size());
    }
    void upload(Ctx* c, void* d, const PoolPlan& pp, const OrderPlan& op) const {
        std::vector<long long> offs(pp.off);   // off [N], then roff [N]
        offs.insert(offs.end(), pp.roff.begin(), pp.roff.end());
        up(c, d, off, offs); up(c, d, G0, pp.G0); up(c, d, gm, pp.gm); up(c, d, cst, pp.cst); up(c, d, rk, op.rk);
        up(c, d, cch0, pp.cch0); up(c, d, gch0, pp.gch0); up(c, d, clen, pp.clen); up(c, d, sgrp, op.sgrp); up(c, d, wgrp, op.wgrp);
        up(c, d, probs, op.probs, op.nq);
    }
};

// the six digits of a grid-wide radix select of nw columns at R ranks each, WB columns' histograms ghist [WB][R][GROUP_BINS] at a time:
// hist(w0, wn, dg) counts digit dg of the columns [w0, w0 + wn) into them, k_group_pick finds each rank's digit (rem, pre [nw][R]) and
// zeroes them again.  The counts are k_group_hist's (pool_order) or the integer weights of k_adjust_hist (smm_get_adjustment).
template <class Hist>
void radix_digits(Ctx* c, int nw, int R, int WB, unsigned long long* ghist, long long* rem, unsigned long long* pre, Hist hist) {
    for (int w0 = 0; w0 < nw; w0 += WB) {
        const int wn = std::min(WB, nw - w0);
        for (int dg = 0; dg < 6; ++dg) {
            hist(w0, wn, dg);
            launch_checked(c, k_group_pick, dim3(wn * R), dim3(STATS_WG), 0, dg, w0 * R, ghist, rem, pre);
        }
    }
}

// median (omed NULL: none) and quantiles of the km packed columns col [km][Mtot], the result columns [ks, ks + km) of D: the short ones
// by k_group_small; the long ones by the six digits of the radix select, WB columns' histograms at a time, then k_group_finish
void pool_order(Ctx* c, void* d, const PoolDev& pd, const PoolPlan& pp, const OrderPlan& op, const double* col, int km, int ks, int D,
                const int* gnan, double* omed, double* quant) {
    const int G = (int)pp.gm.size(), R = op.R, nq = (int)op.nq;
    const long long *dG0 = pd.G0.in(d), *dgm = pd.gm.in(d);
    const double* dprobs = pd.probs.in(d);
    if (!op.sgrp.empty())
        launch_checked(c, k_group_small, dim3((unsigned)op.sgrp.size(), km), dim3(STATS_WG), (size_t)STATS_LDS_N * 8, col, pp.Mtot,
                       (const int*)pd.sgrp.in(d), dG0, dgm, G, ks, D, gnan, dprobs, nq, omed, quant);
    if (op.wgrp.empty()) return;
    const int nw = (int)op.wgrp.size() * km, WB = pd.WB;
    const int B = (int)std::min<long long>(1024, std::max<long long>(1, (op.wmax + STATS_WG * 16 - 1) / (STATS_WG * 16)));
    std::vector<long long> remh((size_t)nw * R);
    for (int w = 0; w < nw; ++w)
        for (int r = 0; r < R; ++r) remh[(size_t)w * R + r] = op.rk[(size_t)(w / km) * R + r];
    up(c, d, pd.rem, remh);
    HIPCHK(hipMemsetAsync(pd.pre.in(d), 0, (size_t)nw * R * 8, c->stream));
    HIPCHK(hipMemsetAsync(pd.ghist.in(d), 0, (size_t)WB * R * GROUP_BINS * 8, c->stream));   // (k_group_pick zeroes it again)
    radix_digits(c, nw, R, WB, pd.ghist.in(d), pd.rem.in(d), pd.pre.in(d), [&](int w0, int wn, int dg) {
        launch_checked(c, k_group_hist, dim3(wn, B, (R + GROUP_RB - 1) / GROUP_RB), dim3(STATS_WG), 0, col, pp.Mtot,
                       (const int*)pd.wgrp.in(d), dG0, dgm, km, R, dg, w0, (const long long*)pd.rem.in(d),
                       (const unsigned long long*)pd.pre.in(d), pd.ghist.in(d));
    });
    launch_checked(c, k_group_finish, dim3((nw + 63) / 64), dim3(64), 0, nw, (const int*)pd.wgrp.in(d), dgm, G, ks, km, D, R,
                   (const long long*)pd.rk.in(d), (const unsigned long long*)pd.pre.in(d), gnan, dprobs, nq, omed, quant);
}

// the segmented radix sort of smm_rank.hpp over the batch's columns (b: smm_get_rank_diag's split chains, or smm_get_density's plain
// column table): the keys KA with their indexes IA sorted in place through KB / IB; columns of at most RANK_SMALL values by one
// workgroup each, the longer ones (any_large; table: their digit counts) pass by pass over the grid
void rank_sort_columns(Ctx* c, const RankBatch& b, bool any_large, unsigned long long* KA, unsigned* IA, unsigned long long* KB, unsigned* IB,
                       int* table) {
    const dim3 cols(b.gn, b.sb), blocks(b.gn, b.sb, RANK_NBLK);
    launch_checked(c, k_rank_sort_small, cols, dim3(RANK_WG), 0, b, KA, IA, KB, IB);
    for (int pass = 0; pass < 8 && any_large; ++pass) {
        unsigned long long* Kin = (pass & 1) ? KB : KA;
        unsigned long long* Kout = (pass & 1) ? KA : KB;
        unsigned* Iin = (pass & 1) ? IB : IA;
        unsigned* Iout = (pass & 1) ? IA : IB;
        launch_checked(c, k_rank_count, blocks, dim3(RANK_WG), 0, b, pass, (const unsigned long long*)Kin, table);
        launch_checked(c, k_rank_scan, cols, dim3(RANK_WG), 0, b, table);
        launch_checked(c, k_rank_scatter, blocks, dim3(RANK_WG), 0, b, pass, (const unsigned long long*)Kin, (const unsigned*)Iin, Kout, Iout,
                       (const int*)table);
    }
}

// the reducers' dynamic LDS (smm_ctx_create): a chunk of draws (k_stats_column, k_cov_center, k_diag_acov, k_group_*, k_trace_column),
// the partner ids of a pass (k_stats_mode), the counters and edges of a batch of parameters or pairs (k_hist_count, k_hist_pairs), a
// split chain (k_rank_chain_mom, k_rank_acov), the three matrices of a group (k_moment_solve: 3 x 64 x 65 doubles), the two of
// k_adjust_solve, a chunk of a chain's weights (k_rw_chain), a chunk of a segment (k_prof_chunk)
void reducer_kernel_attributes() {
    HIPCHK(hipFuncSetAttribute((const void*)k_stats_column, hipFuncAttributeMaxDynamicSharedMemorySize, STATS_LDS_N * 8));
    HIPCHK(hipFuncSetAttribute((const void*)k_cov_center, hipFuncAttributeMaxDynamicSharedMemorySize, STATS_LDS_N * 8));
    HIPCHK(hipFuncSetAttribute((const void*)k_diag_acov, hipFuncAttributeMaxDynamicSharedMemorySize, STATS_LDS_N * 8));
    HIPCHK(hipFuncSetAttribute((const void*)k_stats_mode, hipFuncAttributeMaxDynamicSharedMemorySize, STATS_MODE_BINS * 4));
    HIPCHK(hipFuncSetAttribute((const void*)k_group_chunk_sum, hipFuncAttributeMaxDynamicSharedMemorySize, STATS_LDS_N * 8));
    HIPCHK(hipFuncSetAttribute((const void*)k_group_small, hipFuncAttributeMaxDynamicSharedMemorySize, STATS_LDS_N * 8));
    HIPCHK(hipFuncSetAttribute((const void*)k_hist_count, hipFuncAttributeMaxDynamicSharedMemorySize, (int)HIST_LDS_BYTES));
    HIPCHK(hipFuncSetAttribute((const void*)k_hist_pairs, hipFuncAttributeMaxDynamicSharedMemorySize, (int)HIST_LDS_BYTES));
    HIPCHK(hipFuncSetAttribute((const void*)k_trace_column, hipFuncAttributeMaxDynamicSharedMemorySize, STATS_LDS_N * 8));
    HIPCHK(hipFuncSetAttribute((const void*)k_rank_chain_mom, hipFuncAttributeMaxDynamicSharedMemorySize, STATS_LDS_N * 8));
    HIPCHK(hipFuncSetAttribute((const void*)k_rank_acov, hipFuncAttributeMaxDynamicSharedMemorySize, STATS_LDS_N * 8));
    HIPCHK(hipFuncSetAttribute((const void*)k_moment_solve, hipFuncAttributeMaxDynamicSharedMemorySize, 3 * MAX_DIM * (MAX_DIM + 1) * 8));
    HIPCHK(hipFuncSetAttribute((const void*)k_adjust_solve, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * MAX_DIM * (MAX_DIM + 1) * 8));
    HIPCHK(hipFuncSetAttribute((const void*)k_rw_chain, hipFuncAttributeMaxDynamicSharedMemorySize, STATS_LDS_N * 8));
    HIPCHK(hipFuncSetAttribute((const void*)k_prof_chunk, hipFuncAttributeMaxDynamicSharedMemorySize, STATS_LDS_N * 8));
    HIPCHK(hipFuncSetAttribute((const void*)k_dens_small, hipFuncAttributeMaxDynamicSharedMemorySize, STATS_LDS_N * 8));
    HIPCHK(hipFuncSetAttribute((const void*)k_dens_mode_fin, hipFuncAttributeMaxDynamicSharedMemorySize, STATS_LDS_N * 8));
    HIPCHK(hipFuncSetAttribute((const void*)k_dens_chunk_dev, hipFuncAttributeMaxDynamicSharedMemorySize, STATS_LDS_N * 8));
    HIPCHK(hipFuncSetAttribute((const void*)k_dens_kde, hipFuncAttributeMaxDynamicSharedMemorySize, STATS_LDS_N * 8));
}

}  // namespace

extern "C" {

// mean / median / CI / best / summary of AlgoBGP.jl:117-206 for every local chain, reduced where the history lives (smm_stats.hpp)
int smm_get_chain_stats(void* ctx, int32_t t0, int32_t t1, int32_t accepted_only, const double* probs, int32_t n_probs,
                        smm_chain_stats_t* out) {
    return api_call(ctx, out != nullptr, [&](Ctx* c) -> int {
        if (const int rc = check_probs(c, probs, n_probs, out->quantile != nullptr)) return rc;
        if (const int rc = settled_window(c, t0, t1)) return rc;
        const KParams& P = c->P;
        const size_t N = P.N, np = P.np, nq = n_probs;
        const int n = t1 - t0;
        Carve R;   // the doubles first (NaN for an empty window), then the ints (0)
        const auto bestv = R.take<double>(N), dprobs = R.take<double>(nq), mean = R.take<double>(np * N), median = R.take<double>(np * N),
                   quant = R.take<double>(nq * np * N);
        const auto count = R.take<int>(N), nex = R.take<int>(N), besti = R.take<int>(N), most = R.take<int>(N);
        void* d = reducer_result(c, R.bytes);
        std::vector<char> hres(R.bytes);
        if (n == 0) {   // nothing selected, nothing to find
            std::fill(bestv.in(hres.data()), (double*)count.in(hres.data()), NAN);
            memset(count.in(hres.data()), 0, R.bytes - count.off);
        } else {
            reducer_scratch(c, 0);
            up(c, d, dprobs, probs, nq);
            const bool cols = out->mean || out->median || out->quantile;
            auto per_chain = [&](size_t kb) { return (size_t)n * (8 * kb + 4); };
            size_t kb = cols ? np : 0;
            while (kb > 1 && per_chain(kb) > c->st_scr_bytes) kb = (kb + 1) / 2;
            const int lds_n = sort_lds_n(n);
            const int bins = std::min(c->H.stats_mode_bins, std::max(P.Ng, 64));   // (STATS_MODE_BINS but for the test seam)
            for (size_t k0 = 0; k0 < std::max(np, (size_t)1); k0 += std::max(kb, (size_t)1)) {
                const int kbb = (int)std::min(kb, np - k0);
                const int first = k0 == 0;
                if (!first && !cols) break;
                chain_batches(c, per_chain(kb), [&](int c0, int nb) {
                    double* col = (double*)c->st_scr;
                    int* pcol = (int*)(col + (size_t)kbb * nb * n);
                    launch_checked(c, k_stats_gather, dim3(nb), dim3(STATS_WG), 0, (const double*)P.hrec, (int)N, P.HW, t0, n,
                                   (int)(accepted_only != 0), c0, nb, (int)k0, kbb, first, col, pcol, count.in(d), nex.in(d), bestv.in(d),
                                   besti.in(d));
                    if (kbb > 0)
                        launch_checked(c, k_stats_column, dim3(nb, kbb), dim3(STATS_WG), (size_t)lds_n * 8, (const double*)col, n, (int)N, c0,
                                       nb, (int)k0, (const int*)count.in(d), (const double*)dprobs.in(d), (int)nq, (int)np, mean.in(d),
                                       median.in(d), quant.in(d));
                    if (first)
                        launch_checked(c, k_stats_mode, dim3(nb), dim3(STATS_WG), (size_t)bins * 4, (const int*)pcol, n, c0, bins,
                                       (const int*)nex.in(d), most.in(d));
                });
            }
            HIPCHK(hipMemcpyAsync(hres.data(), d, R.bytes, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
        }
        void* h = hres.data();
        if (out->best_value) memcpy(out->best_value, bestv.in(h), N * 8);
        if (out->mean) memcpy(out->mean, mean.in(h), np * N * 8);
        if (out->median) memcpy(out->median, median.in(h), np * N * 8);
        if (out->quantile) memcpy(out->quantile, quant.in(h), nq * np * N * 8);
        if (out->count) memcpy(out->count, count.in(h), N * 4);
        if (out->n_exchanged) memcpy(out->n_exchanged, nex.in(h), N * 4);
        if (out->best_iter) memcpy(out->best_iter, besti.in(h), N * 4);
        if (out->most_exchanged_with) memcpy(out->most_exchanged_with, most.in(h), N * 4);
        return SMM_OK;
    });
}

// --- covariances of the chains' draws, and the proposal factor between steps (smm_cov.hpp) ---------------------------------------------

// the covariance of every local chain's selected draws over [t0, t1) on the device: count [N], mean [np][N], cov [np][np][N] in the
// reducers' result buffer (status [N] behind them, for smm_adapt_proposal).  The caller has run the prelude and checked the window.
struct CovRes { int* count; double* mean; double* cov; int* status; };
static CovRes chain_cov_device(Ctx* c, int t0, int t1, int accepted_only, int unit_space) {
    const KParams& P = c->P;
    const size_t N = P.N, np = P.np;
    const int n = t1 - t0;
    Carve R;
    const auto mean = R.take<double>(np * N), cov = R.take<double>(np * np * N), bestv = R.take<double>(N);
    const auto count = R.take<int>(N), nex = R.take<int>(N), besti = R.take<int>(N), status = R.take<int>(N);
    void* d = reducer_result(c, R.bytes);
    const CovRes r{count.in(d), mean.in(d), cov.in(d), status.in(d)};
    if (n == 0) {   // nothing selected: count 0, mean and cov NaN
        HIPCHK(hipMemsetAsync(r.count, 0, N * 4, c->stream));
        std::vector<double> nan((np + np * np) * N, NAN);
        HIPCHK(hipMemcpyAsync(r.mean, nan.data(), nan.size() * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return r;
    }
    reducer_scratch(c, (size_t)P.T * (8 * np + 4));   // every parameter of a chain at once
    const int lds_n = sort_lds_n(n);
    const int nt = ((int)np + COV_T - 1) / COV_T, ntiles = nt * (nt + 1) / 2;
    chain_batches(c, (size_t)n * (8 * np + 4), [&](int c0, int nb) {
        double* col = (double*)c->st_scr;
        int* pcol = (int*)(col + np * nb * n);
        launch_checked(c, k_stats_gather, dim3(nb), dim3(STATS_WG), 0, (const double*)P.hrec, (int)N, P.HW, t0, n, (int)(accepted_only != 0),
                       c0, nb, 0, (int)np, 1, col, pcol, r.count, nex.in(d), bestv.in(d), besti.in(d));
        launch_checked(c, k_cov_center, dim3(nb, np), dim3(STATS_WG), (size_t)lds_n * 8, col, n, (int)N, c0, nb, (int)(unit_space != 0), P.lb,
                       P.ub, (const int*)r.count, r.mean);
        launch_checked(c, k_cov_pairs, dim3(nb, ntiles), dim3(COV_WG), 0, (const double*)col, n, (int)N, c0, nb, (int)np, (const int*)r.count,
                       r.cov, 0);
    });
    return r;
}

int smm_get_chain_cov(void* ctx, int32_t t0, int32_t t1, int32_t accepted_only, int32_t unit_space, int32_t* count, double* mean,
                      double* cov) {
    return api_call(ctx, true, [&](Ctx* c) -> int {
        if (const int rc = settled_window(c, t0, t1)) return rc;
        const size_t N = c->P.N, np = c->P.np;
        const CovRes r = chain_cov_device(c, t0, t1, accepted_only, unit_space);
        if (count) HIPCHK(hipMemcpyAsync(count, r.count, N * 4, hipMemcpyDeviceToHost, c->stream));
        if (mean) HIPCHK(hipMemcpyAsync(mean, r.mean, np * N * 8, hipMemcpyDeviceToHost, c->stream));
        if (cov) HIPCHK(hipMemcpyAsync(cov, r.cov, np * np * N * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return SMM_OK;
    });
}

// doubles of the factor(s) a caller reads or writes: [np][np] shared, [N][np][np] per chain (the local chains' rows)
static size_t proposal_doubles(const KParams& P) { return (size_t)(P.chol_per_chain ? P.N : 1) * P.np * P.np; }
static double* proposal_rows(const KParams& P) {
    return (double*)P.chol_L + (P.chol_per_chain ? (size_t)P.offset * P.np * P.np : 0);
}

int smm_get_proposal(void* ctx, double* L) {
    return api_call(ctx, L != nullptr, [&](Ctx* c) -> int {
        const KParams& P = c->P;
        if (!P.chol_L) return fail(c, SMM_ERR_INVALID_ARG, "the context has no proposal factor: create it with chol_L");
        HIPCHK(hipSetDevice(c->device));   // (reads the factor as it stands: no prelude)
        const size_t n = proposal_doubles(P), np = P.np;
        HIPCHK(hipMemcpyAsync(L, proposal_rows(P), n * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        for (size_t b = 0; b < n; b += np * np)   // (what lies above the diagonal was never read)
            for (size_t k = 0; k < np; ++k)
                for (size_t j = k + 1; j < np; ++j) L[b + k * np + j] = 0.0;
        return SMM_OK;
    });
}

// the mutating calls: settled, flushed and synchronised; a hard failure standing on the context is handed to the caller (and marked told)
static int proposal_prelude(Ctx* c) {
    reader_prelude(c);
    (void)check_device_error(c);
    return c->failed ? told(c) : SMM_OK;
}

int smm_set_proposal(void* ctx, const double* L) {
    return api_call(ctx, L != nullptr, [&](Ctx* c) -> int {
        const KParams& P = c->P;
        if (!P.chol_L) return fail(c, SMM_ERR_INVALID_ARG, "the context has no proposal factor: create it with chol_L");
        const size_t n = proposal_doubles(P), np = P.np;
        std::vector<double> h(n);
        for (size_t b = 0; b < n; b += np * np)
            for (size_t k = 0; k < np; ++k)
                for (size_t j = 0; j < np; ++j) {
                    const double v = j <= k ? L[b + k * np + j] : 0.0;
                    if (!std::isfinite(v)) return fail(c, SMM_ERR_INVALID_ARG, "smm_set_proposal: a non-finite entry on or below the diagonal");
                    if (j == k && !(v > 0.0)) return fail(c, SMM_ERR_INVALID_ARG, "smm_set_proposal: a diagonal entry is not > 0");
                    h[b + k * np + j] = v;
                }
        if (const int rc = proposal_prelude(c)) return rc;
        HIPCHK(hipMemcpyAsync(proposal_rows(P), h.data(), n * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return SMM_OK;
    });
}

int smm_adapt_proposal(void* ctx, int32_t t0, int32_t t1, int32_t accepted_only, int32_t min_draws, int32_t normalize, double ridge,
                       int32_t* status) {
    return api_call(ctx, true, [&](Ctx* c) -> int {
        const KParams& P = c->P;
        if (!P.chol_L) return fail(c, SMM_ERR_INVALID_ARG, "the context has no proposal factor: create it with chol_L (per chain)");
        if (!P.chol_per_chain)
            return fail(c, SMM_ERR_INVALID_ARG, "smm_adapt_proposal needs per-chain factors (chol_per_chain = 1): a shared factor has no own history");
        if (min_draws < 2) return fail(c, SMM_ERR_INVALID_ARG, "min_draws must be >= 2");
        if (!(ridge >= 0.0) || !std::isfinite(ridge)) return fail(c, SMM_ERR_INVALID_ARG, "ridge must be finite and >= 0");
        if (const int rc = proposal_prelude(c)) return rc;   // (a failure standing on the context comes before the window)
        if (const int rc = check_window(c, t0, t1)) return rc;
        const size_t N = P.N;
        const CovRes r = chain_cov_device(c, t0, t1, accepted_only, 1);
        launch_checked(c, k_cov_chol, dim3(N), dim3(64), 0, (const double*)r.cov, (const int*)r.count, (int)N, P.np, (int)min_draws,
                       (int)(normalize != 0), ridge, P.chol_per_chain ? P.offset : 0, (double*)P.chol_L, r.status);
        if (status) HIPCHK(hipMemcpyAsync(status, r.status, N * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return SMM_OK;
    });
}

// --- autocorrelation, ESS and split R-hat of the chains (smm_diag.hpp) --------------------------------------------------------------

// the chain-stats sum on the host: numpy's pairwise sum over chunks of 8192 (include/smmhip.h), every operation rounded on its own
static double host_pw(const double* x, size_t n) {
    if (n < 8) {
        double r = 0.0;
        for (size_t i = 0; i < n; ++i) r = r + x[i];
        return r;
    }
    if (n <= 128) {
        double r[8];
        for (int k = 0; k < 8; ++k) r[k] = x[k];
        const size_t m = n - n % 8;
        for (size_t i = 8; i < m; i += 8)
            for (int k = 0; k < 8; ++k) r[k] = r[k] + x[i + k];
        double s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (size_t i = m; i < n; ++i) s = s + x[i];
        return s;
    }
    size_t n2 = n / 2;
    n2 -= n2 % 8;
    const double lf = host_pw(x, n2), rt = host_pw(x + n2, n - n2);
    return lf + rt;
}
static double host_sum(const std::vector<double>& x) {
    double S = 0.0;
    for (size_t c = 0; c < x.size(); c += STATS_LDS_N) S = S + host_pw(x.data() + c, std::min((size_t)STATS_LDS_N, x.size() - c));
    return S;
}

int smm_get_chain_diag(void* ctx, int32_t t0, int32_t t1, int32_t max_lag, int32_t n_acf, const int32_t* group, int32_t n_groups,
                       smm_chain_diag_t* out) {
    return api_call(ctx, out != nullptr, [&](Ctx* c) -> int {
        // (between check_groups' NULL rule and its ids; ahead of both it decides the same, as no count fails this and the NULL rule)
        if (out->rhat && n_groups == 0) return fail(c, SMM_ERR_INVALID_ARG, "rhat requested without groups");
        if (const int rc = check_groups(c, group, n_groups, GROUPS_OPTIONAL)) return rc;
        if (const int rc = settled_window(c, t0, t1)) return rc;
        const size_t N = c->P.N;
        const int n = t1 - t0;
        if (n < 4) return fail(c, SMM_ERR_INVALID_ARG, "the window must hold at least 4 iterations");
        if (max_lag < 1 || max_lag > n - 1) return fail(c, SMM_ERR_INVALID_ARG, "max_lag must lie in [1, t1 - t0 - 1]");
        if (n_acf < 0 || n_acf > max_lag + 1) return fail(c, SMM_ERR_INVALID_ARG, "n_acf must lie in [0, max_lag + 1]");
        const KParams& P = c->P;
        const size_t np = P.np, S = np + 1, SN = S * N, nacf = out->acf ? (size_t)n_acf : 0;
        const bool halves = out->rhat != nullptr;
        Carve R;
        const auto ess = R.take<double>(SN), acf = R.take<double>(nacf * SN), hmu = R.take<double>(2 * SN), hvar = R.take<double>(2 * SN);
        const auto status = R.take<int>(SN), nacc = R.take<int>(N), noex = R.take<int>(N);
        void* d = reducer_result(c, R.bytes);
        reducer_scratch(c, (size_t)P.T * 8 * S);   // the S columns of a chain at once
        const int lds_n = std::min(STATS_LDS_N, n);
        chain_batches(c, (size_t)n * 8 * S, [&](int c0, int nb) {
            double* col = (double*)c->st_scr;
            launch_checked(c, k_diag_gather, dim3(nb), dim3(DIAG_WG), 0, (const double*)P.hrec, (int)N, P.HW, (int)np, t0, n, c0, nb, col,
                           nacc.in(d), noex.in(d));
            launch_checked(c, k_diag_acov, dim3(nb, S), dim3(DIAG_WG), (size_t)lds_n * 8, col, n, (int)N, c0, nb, (int)S, (int)max_lag,
                           (int)nacf, (int)halves, ess.in(d), status.in(d), nacf ? acf.in(d) : nullptr, hmu.in(d), hvar.in(d));
        });
        std::vector<char> hres(R.bytes);
        HIPCHK(hipMemcpyAsync(hres.data(), d, R.bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        void* h = hres.data();
        const int* hs = status.in(h);
        if (out->accept_rate)
            for (size_t i = 0; i < N; ++i) out->accept_rate[i] = (double)nacc.in(h)[i] / (double)noex.in(h)[i];
        if (out->ess) memcpy(out->ess, ess.in(h), SN * 8);
        if (out->status) memcpy(out->status, hs, SN * 4);
        if (out->acf) memcpy(out->acf, acf.in(h), nacf * SN * 8);
        if (out->rhat) {   // split R-hat of each group and series, the members in ascending local index (include/smmhip.h)
            const double* hm = hmu.in(h);
            const double* hv = hvar.in(h);
            const int hl = n / 2;
            std::vector<double> mus, vars, e;
            for (int g = 0; g < n_groups; ++g)
                for (size_t s = 0; s < S; ++s) {
                    mus.clear(); vars.clear();
                    bool bad = false;
                    for (size_t i = 0; i < N; ++i) {
                        if (group[i] != g) continue;
                        bad |= hs[s * N + i] == 3;
                        for (int hf = 0; hf < 2; ++hf) {
                            mus.push_back(hm[hf * SN + s * N + i]);
                            vars.push_back(hv[hf * SN + s * N + i]);
                        }
                    }
                    double r = NAN;
                    if (!mus.empty() && !bad) {
                        const double k2 = (double)mus.size();
                        const double W = host_sum(vars) / k2, mm = host_sum(mus) / k2;
                        e.resize(mus.size());
                        for (size_t q = 0; q < mus.size(); ++q) { const double dv = mus[q] - mm; e[q] = dv * dv; }
                        const double v = host_sum(e) / (k2 - 1.0);
                        const double vp = ((hl - 1.0) / hl) * W + v;
                        r = sqrt(vp / W);
                    }
                    out->rhat[(size_t)g * S + s] = r;
                }
        }
        return SMM_OK;
    });
}

// --- pooled summaries of groups of chains (smm_group.hpp) -------------------------------------------------------------------------------

int smm_get_group_stats(void* ctx, int32_t t0, int32_t t1, int32_t accepted_only, const int32_t* group, int32_t n_groups,
                        const double* probs, int32_t n_probs, smm_group_stats_t* out) {
    return api_call(ctx, out != nullptr, [&](Ctx* c) -> int {
        if (const int rc = check_groups(c, group, n_groups, GROUPS_DEFAULT_ONE)) return rc;
        if (const int rc = check_probs(c, probs, n_probs, out->quantile != nullptr)) return rc;
        if (const int rc = settled_window(c, t0, t1)) return rc;
        const KParams& P = c->P;
        const size_t N = P.N, np = P.np, G = n_groups, nq = out->quantile ? n_probs : 0;
        const int n = t1 - t0;
        const bool med = out->median != nullptr, ord = med || nq > 0, cov = out->cov != nullptr, cols = out->mean || ord || cov;
        const Groups grp = group_members(group, G, N);
        DevBuf<int> dci(2 * N);
        const PoolPlan pp = pool_plan(grp, pool_counts(c, grp, t0, n, accepted_only != 0, dci.p));
        const OrderPlan op = order_plan(c, pp, med, probs, nq);
        const long long Mtot = pp.Mtot;
        const int NC = pp.NC;
        if (Mtot > 0 && cols) reducer_scratch(c, std::max(N * (size_t)P.T * 8, cov ? np * STATS_LDS_N * 8 : 0));
        const size_t kb = Mtot > 0 && cols ? std::min(np, c->st_scr_bytes / ((size_t)Mtot * 8)) : 0;
        Carve Rv;   // 8-byte slices first
        const auto mean = Rv.take<double>(G * np), median = Rv.take<double>(G * np), quant = Rv.take<double>(nq * G * np),
                   covo = Rv.take<double>(cov ? G * np * np : 0), csum = Rv.take<double>(kb * NC),
                   csum2 = Rv.take<double>(cov ? np * np * NC : 0);
        const PoolDev pd(Rv, pp, op, op.wgrp.size() * kb);   // (the long columns of a parameter batch)
        const auto cnan = Rv.take<int>(kb * NC), gnan = Rv.take<int>(G * np);
        void* d = reducer_result(c, Rv.bytes);
        pd.upload(c, d, pp, op);
        const int sel = accepted_only != 0;
        const int *dgid = dci.p, *dgch0 = pd.gch0.in(d), *dclen = pd.clen.in(d);
        int* dcnt = dci.p + N;
        const long long* dgm = pd.gm.in(d);
        if (kb > 0) {
            double* col = (double*)c->st_scr;
            for (size_t k0 = 0; k0 < np; k0 += kb) {   // batches of parameters: the packed columns [kbb][Mtot]
                const int kbb = (int)std::min(kb, np - k0);
                launch_checked(c, k_group_gather, dim3(N), dim3(STATS_WG), 0, (const double*)P.hrec, (int)N, P.HW, t0, n, sel, dgid,
                               (const long long*)pd.off.in(d), (const int*)nullptr, (int)k0, kbb, Mtot, 0, 0, (const double*)nullptr, (int)np,
                               col, dcnt, 0, (int*)nullptr);
                if (NC > 0)
                    launch_checked(c, k_group_chunk_sum, dim3(NC, kbb), dim3(STATS_WG), (size_t)STATS_LDS_N * 8, (const double*)col, Mtot,
                                   (const long long*)pd.cst.in(d), dclen, NC, csum.in(d), cnan.in(d));
                launch_checked(c, k_group_mean, dim3((unsigned)((G * kbb + 255) / 256)), dim3(256), 0, (const double*)csum.in(d),
                               (const int*)cnan.in(d), NC, dgch0, dgm, (int)G, (int)k0, kbb, (int)np, mean.in(d), gnan.in(d));
                if (ord)
                    pool_order(c, d, pd, pp, op, col, kbb, (int)k0, (int)np, gnan.in(d), med ? median.in(d) : nullptr, quant.in(d));
            }
            if (cov) {   // batches of chunks: every parameter centred, [np][nb][STATS_LDS_N]; each chunk's pair sums, then the groups'
                const int Nbc = (int)std::min<size_t>(NC, c->st_scr_bytes / (np * STATS_LDS_N * 8));
                const int nt = ((int)np + COV_T - 1) / COV_T, ntiles = nt * (nt + 1) / 2;
                for (int cb0 = 0; cb0 < NC; cb0 += Nbc) {
                    const int nb = std::min(Nbc, NC - cb0);
                    launch_checked(c, k_group_gather, dim3(N), dim3(STATS_WG), 0, (const double*)P.hrec, (int)N, P.HW, t0, n, sel, dgid,
                                   (const long long*)pd.off.in(d) + N, (const int*)pd.cch0.in(d), 0, (int)np, Mtot, cb0, nb,
                                   (const double*)mean.in(d), (int)np, col, dcnt, 0, (int*)nullptr);
                    launch_checked(c, k_cov_pairs, dim3(nb, ntiles), dim3(COV_WG), 0, (const double*)col, STATS_LDS_N, NC, cb0, nb, (int)np,
                                   dclen, csum2.in(d), 1);
                }
            }
        }
        if (cov && G > 0)
            launch_checked(c, k_group_cov, dim3((unsigned)((G * np * (np + 1) / 2 + 255) / 256)), dim3(256), 0, (const double*)csum2.in(d),
                           NC, dgch0, dgm, (int)G, (int)np, covo.in(d));
        if (kb > 0) {   // (no draw in any group: every output NaN, filled below)
            down(c, d, mean, out->mean, G * np);
            down(c, d, median, out->median, G * np);
            down(c, d, quant, out->quantile, nq * G * np);
        }
        down(c, d, covo, out->cov, G * np * np);
        HIPCHK(hipStreamSynchronize(c->stream));
        if (kb == 0) {
            if (out->mean) std::fill(out->mean, out->mean + G * np, NAN);
            if (out->median) std::fill(out->median, out->median + G * np, NAN);
            if (out->quantile) std::fill(out->quantile, out->quantile + nq * G * np, NAN);
        }
        if (out->count) std::copy(pp.gm.begin(), pp.gm.end(), out->count);
        if (out->n_chains) std::copy(grp.n_chains.begin(), grp.n_chains.end(), out->n_chains);
        return SMM_OK;
    });
}

// --- histograms of groups of chains (smm_hist.hpp) ---------------------------------------------------------------------------------------

int smm_get_histogram(void* ctx, int32_t t0, int32_t t1, int32_t select, const int32_t* group, int32_t n_groups, int32_t bins,
                      const double* range, const int32_t* pairs, int32_t n_pairs, int32_t bins2, smm_histogram_t* out) {
    return api_call(ctx, out != nullptr, [&](Ctx* c) -> int {
        const size_t N = c->P.N, np = c->P.np;
        if (const int rc = check_select(c, select)) return rc;
        if (const int rc = check_groups(c, group, n_groups, GROUPS_DEFAULT_ONE)) return rc;
        if (bins < 1 || bins > 65536) return fail(c, SMM_ERR_INVALID_ARG, "bins must lie in [1, 65536]");
        if (range)
            for (size_t k = 0; k < np; ++k)
                if (!(std::isfinite(range[2 * k]) && std::isfinite(range[2 * k + 1]) && range[2 * k] <= range[2 * k + 1]))
                    return fail(c, SMM_ERR_INVALID_ARG, "a range row must be finite with lo <= hi");
        if (n_pairs < 0 || (size_t)n_pairs > np * np || (n_pairs > 0 && !pairs))
            return fail(c, SMM_ERR_INVALID_ARG, "n_pairs outside [0, np np], or pairs NULL with n_pairs > 0");
        for (int p = 0; p < 2 * n_pairs; ++p)
            if (pairs[p] < 0 || (size_t)pairs[p] >= np) return fail(c, SMM_ERR_INVALID_ARG, "a pair entry outside [0, np)");
        if (n_pairs > 0 && (bins2 < 1 || bins2 > 512)) return fail(c, SMM_ERR_INVALID_ARG, "bins2 must lie in [1, 512]");
        if (n_pairs == 0 && (out->hist2 || out->edges2)) return fail(c, SMM_ERR_INVALID_ARG, "hist2 or edges2 requested without pairs");
        if (const int rc = settled_window(c, t0, t1)) return rc;
        const KParams& P = c->P;
        const size_t G = n_groups, B = bins, B2 = n_pairs > 0 ? bins2 : 0, NP = n_pairs;
        const int n = t1 - t0;
        const bool two = NP > 0 && (out->hist2 || out->edges2);
        const Groups grp = group_members(group, G, N);
        const int M = grp.M;
        const bool autor = range == nullptr, cnt_pass = autor || (out->count && select == 1);
        // a batch of groups: the edges (always: the counting reads them), the counts asked for, the 2-D axes and cells
        const size_t per_group = np * (B + 1) * 8 + (out->hist ? np * B * 8 : 0) + (two ? np * (B2 + 1) * 8 : 0) +
                                 (two && out->hist2 ? NP * B2 * B2 * 8 : 0);
        const size_t gb = G ? std::max((size_t)1, std::min(G, reducer_batch_cap(c) / per_group)) : 0;
        Carve Rv;   // 8-byte slices first
        const auto cmin = Rv.take<double>(autor ? N * np : 0), cmax = Rv.take<double>(autor ? N * np : 0), drng = Rv.take<double>(autor ? 0 : 2 * np),
                   dlo = Rv.take<double>(G * np), dhi = Rv.take<double>(G * np), edges = Rv.take<double>(gb * np * (B + 1)),
                   edges2 = Rv.take<double>(two ? gb * np * (B2 + 1) : 0);
        const auto hist = Rv.take<unsigned long long>(out->hist ? gb * np * B : 0),
                   hist2 = Rv.take<unsigned long long>(two && out->hist2 ? gb * NP * B2 * B2 : 0);
        const auto cbad = Rv.take<int>(autor ? N * np : 0), dcnt = Rv.take<int>(N), dst = Rv.take<int>(G * np), dgid = Rv.take<int>(N),
                   dgm0 = Rv.take<int>(G + 1), dmem = Rv.take<int>(M), dpairs = Rv.take<int>(2 * NP);
        void* d = reducer_result(c, Rv.bytes);
        up(c, d, dgid, grp.gid); up(c, d, dgm0, grp.gmem0); up(c, d, dmem, grp.mem); up(c, d, dpairs, pairs, 2 * NP);
        up(c, d, drng, range, 2 * np);
        if (cnt_pass && M > 0)
            launch_checked(c, k_hist_range, dim3(M, autor ? (unsigned)((np + HIST_KMAX - 1) / HIST_KMAX) : 1), dim3(HIST_WG), 0,
                           (const double*)P.hrec, (int)N, P.HW, t0, n, (int)select, (const int*)dmem.in(d), 0, (int)np, dcnt.in(d),
                           autor ? cmin.in(d) : (double*)nullptr, cmax.in(d), cbad.in(d));
        const int lb = c->H.hist_lds_bins;
        const bool lds1 = (int)B <= lb && 12 * B + 8 <= HIST_LDS_BYTES, lds2 = two && (int)B2 <= lb && 16 * (B2 + 1) + 4 * B2 * B2 <= HIST_LDS_BYTES;
        const int kb = lds1 ? (int)std::min({np, (size_t)HIST_KMAX, HIST_LDS_BYTES / (12 * B + 8)}) : (int)std::min(np, (size_t)HIST_KMAX);
        const int kp = !two ? 0 : lds2 ? (int)std::min({NP, (size_t)HIST_KMAX, HIST_LDS_BYTES / (16 * (B2 + 1) + 4 * B2 * B2)})
                                       : (int)std::min(NP, (size_t)HIST_KMAX);
        for (size_t g0 = 0; g0 < G; g0 += gb) {
            const size_t gn = std::min(gb, G - g0);
            const int m0 = grp.gmem0[g0], mb = grp.gmem0[g0 + gn] - m0;
            launch_checked(c, k_hist_edges, dim3((unsigned)gn, (unsigned)np), dim3(HIST_WG), 0, (const int*)dgm0.in(d), (const int*)dmem.in(d),
                           (int)g0, (int)np, (const int*)dcnt.in(d), (const double*)cmin.in(d), (const double*)cmax.in(d),
                           (const int*)cbad.in(d), autor ? (const double*)nullptr : (const double*)drng.in(d), (int)B, (int)B2, dlo.in(d),
                           dhi.in(d), dst.in(d), edges.in(d), two ? edges2.in(d) : (double*)nullptr);
            if (out->hist) {
                HIPCHK(hipMemsetAsync(hist.in(d), 0, gn * np * B * 8, c->stream));
                if (mb > 0)
                    launch_checked(c, k_hist_count, dim3(mb, (unsigned)((np + kb - 1) / kb)), dim3(HIST_WG),
                                   lds1 ? (size_t)kb * (12 * B + 8) : 0, (const double*)P.hrec, (int)N, P.HW, t0, n, (int)select,
                                   (const int*)dmem.in(d), (const int*)dgid.in(d), (const int*)dgm0.in(d), m0, (int)g0, (int)np, kb, (int)B,
                                   (int)lds1, (const double*)dlo.in(d), (const double*)dhi.in(d), (const int*)dst.in(d),
                                   (const double*)edges.in(d), hist.in(d));
            }
            if (two && out->hist2) {
                HIPCHK(hipMemsetAsync(hist2.in(d), 0, gn * NP * B2 * B2 * 8, c->stream));
                if (mb > 0)
                    launch_checked(c, k_hist_pairs, dim3(mb, (unsigned)((NP + kp - 1) / kp)), dim3(HIST_WG),
                                   lds2 ? (size_t)kp * (16 * (B2 + 1) + 4 * B2 * B2) : 0, (const double*)P.hrec, (int)N, P.HW, t0, n,
                                   (int)select, (const int*)dmem.in(d), (const int*)dgid.in(d), (const int*)dgm0.in(d), m0, (int)g0, (int)np,
                                   (const int*)dpairs.in(d), (int)NP, kp, (int)B2, (int)lds2, (const int*)dst.in(d),
                                   (const double*)edges2.in(d), hist2.in(d));
            }
            down(c, d, edges, out->edges ? out->edges + g0 * np * (B + 1) : nullptr, gn * np * (B + 1));
            down(c, d, hist, out->hist ? out->hist + g0 * np * B : nullptr, gn * np * B);
            if (two) {
                down(c, d, edges2, out->edges2 ? out->edges2 + g0 * np * (B2 + 1) : nullptr, gn * np * (B2 + 1));
                down(c, d, hist2, out->hist2 ? out->hist2 + g0 * NP * B2 * B2 : nullptr, gn * NP * B2 * B2);
            }
            HIPCHK(hipStreamSynchronize(c->stream));   // (the next batch reuses the tables)
        }
        std::vector<int> cnt(N, n);
        if (out->count && select == 1 && M > 0) down(c, d, dcnt, cnt.data(), N);
        down(c, d, dlo, out->lo, G * np); down(c, d, dhi, out->hi, G * np); down(c, d, dst, out->status, G * np);
        HIPCHK(hipStreamSynchronize(c->stream));
        if (out->count) {
            std::fill(out->count, out->count + G, (int64_t)0);
            for (size_t i = 0; i < N; ++i)
                if (grp.gid[i] >= 0) out->count[grp.gid[i]] += cnt[i];
        }
        return SMM_OK;
    });
}

// --- the population per iteration (smm_trace.hpp) ----------------------------------------------------------------------------------------

int smm_get_trace(void* ctx, int32_t t0, int32_t t1, int32_t stride, int32_t select, int32_t moments, const int32_t* group, int32_t n_groups,
                  const double* probs, int32_t n_probs, smm_trace_t* out) {
    return api_call(ctx, out != nullptr, [&](Ctx* c) -> int {
        if (stride < 1) return fail(c, SMM_ERR_INVALID_ARG, "stride must be at least 1");
        if (const int rc = check_select(c, select)) return rc;
        if (const int rc = check_groups(c, group, n_groups, GROUPS_DEFAULT_ONE)) return rc;
        if (const int rc = check_probs(c, probs, n_probs, out->quantile != nullptr)) return rc;
        if (const int rc = settled_window(c, t0, t1)) return rc;
        const KParams& P = c->P;
        const size_t N = P.N, np = P.np, S = np + 1 + (moments ? (size_t)P.nm : 0), G = n_groups, nq = out->quantile ? n_probs : 0;
        const int nt = (int)(((long long)(t1 - t0) + stride - 1) / stride);
        const Groups grp = group_members(group, G, N);
        if (out->n_chains) std::copy(grp.n_chains.begin(), grp.n_chains.end(), out->n_chains);
        for (int i = 0; i < nt && out->iter; ++i) out->iter[i] = t0 + (int32_t)((long long)i * stride);
        if (nt == 0 || G == 0) return SMM_OK;
        const int M = grp.M;
        const size_t Mx = std::max(M, 1), Me = (Mx + 1) & ~(size_t)1;   // (the state table's rows keep the columns behind them 8-byte aligned)
        const bool cols = out->mean || out->var || out->median || out->quantile;
        // a batch of kept iterations: the state table and the columns in the scratch, the results in the result buffer; a batch of one
        // kept iteration whose columns do not fit goes in batches of series
        auto per_iter = [&](size_t sb) { return Me * 4 + sb * Mx * 8; };
        reducer_scratch(c, per_iter(1));
        const size_t hook = c->H.stats_scratch;
        const size_t budget = hook ? std::min(c->st_scr_bytes, std::max(hook, per_iter(1))) : c->st_scr_bytes;
        const size_t res_iter = G * ((3 + nq) * S * 8 + 8 + 5 * 4), res_cap = reducer_batch_cap(c);
        const size_t nib = std::min<size_t>(nt, std::max<size_t>(1, std::min(budget / per_iter(cols ? S : 0), res_cap / res_iter)));
        const size_t sb = !cols ? 0 : per_iter(S) <= budget ? S : std::max<size_t>(1, (budget - Me * 4) / (Mx * 8));
        Carve Rv;   // 8-byte slices first
        const auto dprobs = Rv.take<double>(nq), mean = Rv.take<double>(nib * G * S), var = Rv.take<double>(nib * G * S),
                   median = Rv.take<double>(nib * G * S), quant = Rv.take<double>(nq * nib * G * S), bestv = Rv.take<double>(nib * G);
        const auto count = Rv.take<int>(nib * G), nacc = Rv.take<int>(nib * G), nex = Rv.take<int>(nib * G), nfail = Rv.take<int>(nib * G),
                   bestc = Rv.take<int>(nib * G), dgm0 = Rv.take<int>(G + 1), dmem = Rv.take<int>(M);
        void* d = reducer_result(c, Rv.bytes);
        up(c, d, dgm0, grp.gmem0); up(c, d, dmem, grp.mem); up(c, d, dprobs, probs, nq);
        int* tab = (int*)c->st_scr;
        const int lds_n = sort_lds_n(grp.longest);
        for (size_t i0 = 0; i0 < (size_t)nt; i0 += nib) {
            const int nk = (int)std::min(nib, (size_t)nt - i0), tb = t0 + (int)((long long)i0 * stride);
            double* col = (double*)((char*)c->st_scr + (size_t)nk * Me * 4);
            if (select == 2 && M > 0)
                launch_checked(c, k_trace_state, dim3(M), dim3(TRACE_WG), 0, (const double*)P.hrec, (int)N, P.HW, (const int*)dmem.in(d), (int)Me,
                               tb, nk, (int)stride, tab);
            for (size_t s0 = 0; s0 < (cols ? S : 1); s0 += std::max(sb, (size_t)1)) {   // (no column asked for: the counts and the best only)
                const int sbb = (int)std::min(sb, S - s0);
                launch_checked(c, k_trace_gather, dim3((unsigned)(nk * G), (unsigned)std::max(1, (sbb + TRACE_KMAX - 1) / TRACE_KMAX)),
                               dim3(TRACE_WG), 0, (const double*)P.hrec, (int)N, P.HW, (int)np, (const int*)dmem.in(d), (const int*)dgm0.in(d),
                               (int)G, M, (int)Me, P.offset, tb, (int)stride, (int)select, (const int*)tab, (int)s0, sbb, (int)(s0 == 0), col,
                               count.in(d), nacc.in(d), nex.in(d), nfail.in(d), bestv.in(d), bestc.in(d));
                if (sbb > 0)
                    launch_checked(c, k_trace_column, dim3((unsigned)(nk * G), (unsigned)sbb), dim3(TRACE_WG), (size_t)lds_n * 8,
                                   (const double*)col, M, (const int*)dgm0.in(d), (int)G, (int)s0, sbb, (int)S, (const int*)count.in(d),
                                   (const double*)dprobs.in(d), (int)nq, nib * G * S, mean.in(d), out->var ? var.in(d) : (double*)nullptr,
                                   out->median ? median.in(d) : (double*)nullptr, quant.in(d));
            }
            // this batch's nk rows of per elements each, to their place among the nt rows of the caller's array
            auto down_rows = [&](auto sl, auto* dst, size_t per, size_t src_off = 0, size_t dst_off = 0) {
                if (dst) down(c, d, sl.at(src_off), dst + dst_off + i0 * per, (size_t)nk * per);
            };
            down_rows(mean, out->mean, G * S); down_rows(var, out->var, G * S); down_rows(median, out->median, G * S);
            for (size_t p = 0; p < nq; ++p) down_rows(quant, out->quantile, G * S, p * nib * G * S, p * (size_t)nt * G * S);
            down_rows(bestv, out->best_value, G); down_rows(count, out->count, G); down_rows(nacc, out->n_accepted, G);
            down_rows(nex, out->n_exchanged, G); down_rows(nfail, out->n_failed, G); down_rows(bestc, out->best_chain, G);
            HIPCHK(hipStreamSynchronize(c->stream));   // (the next batch reuses the scratch and the results)
        }
        return SMM_OK;
    });
}

// --- rank-normalised R-hat, bulk / tail / mean ESS and rank histograms of groups of chains (smm_rank.hpp) -----------------------------------

int smm_get_rank_diag(void* ctx, int32_t t0, int32_t t1, int32_t max_lag, int32_t n_bins, const int32_t* group, int32_t n_groups,
                      smm_rank_diag_t* out) {
    return api_call(ctx, out != nullptr, [&](Ctx* c) -> int {
        if (n_groups == 0) return fail(c, SMM_ERR_INVALID_ARG, "n_groups must be at least 1");
        if (const int rc = check_groups(c, group, n_groups, GROUPS_DEFAULT_ONE)) return rc;
        if (n_bins < 0) return fail(c, SMM_ERR_INVALID_ARG, "n_bins must be >= 0");
        if (out->rank_hist && n_bins == 0) return fail(c, SMM_ERR_INVALID_ARG, "rank_hist requested with n_bins == 0");
        if (const int rc = settled_window(c, t0, t1)) return rc;
        const int n = t1 - t0, h = n / 2;
        if (n < 8) return fail(c, SMM_ERR_INVALID_ARG, "the window must hold at least 8 iterations");
        if (max_lag < 1 || max_lag > h - 1) return fail(c, SMM_ERR_INVALID_ARG, "max_lag must lie in [1, (t1 - t0) / 2 - 1]");
        const KParams& P = c->P;
        const size_t N = P.N, np = P.np, S = np + 1, G = n_groups, GS = G * S;
        const Groups grp = group_members(group, G, N);
        if (2ll * grp.longest * h > 0x7fffffffll) return fail(c, SMM_ERR_INVALID_ARG, "a group's pooled column holds more than 2^31 - 1 values");
        // the plan: bytes of one series of group g (the value arrays, keys, indices and ranks of its M = 2 k h pooled values, the moments
        // and a block of LB lags of its 2 k split chains, a long column's digit table), the batches of groups and the series per batch
        const int LB = std::min(RANK_WG, max_lag + 1);
        auto col_len = [&](size_t g) { return (size_t)2 * grp.n_chains[g] * h; };
        auto per_g = [&](size_t g) {
            return col_len(g) * 72 + (size_t)2 * grp.n_chains[g] * (80 + 32 * (size_t)LB) + (col_len(g) > (size_t)RANK_SMALL ? (size_t)RANK_TABLE * 4 : 0);
        };
        size_t one = 0, all = 0;
        for (size_t g = 0; g < G; ++g) { one = std::max(one, per_g(g)); all += per_g(g); }
        reducer_scratch(c, one);
        const size_t hook = c->H.stats_scratch;
        const size_t budget = hook ? std::min(c->st_scr_bytes, std::max(hook, one)) : c->st_scr_bytes;
        std::vector<int> bg0{0};   // batch i: the groups [bg0[i], bg0[i + 1])
        size_t sb = S;
        if (all <= budget) {
            bg0.push_back((int)G);
            if (all > 0) sb = std::min(S, budget / all);
        } else {
            sb = 1;
            size_t used = 0;
            for (size_t g = 0; g < G; ++g) {
                if (used > 0 && used + per_g(g) > budget) { bg0.push_back((int)g); used = 0; }
                used += per_g(g);
            }
            bg0.push_back((int)G);
        }
        std::vector<int> qgrp(2 * (size_t)grp.M), large(G, 0);
        for (size_t g = 0; g < G; ++g)
            for (int q = 2 * grp.gmem0[g]; q < 2 * grp.gmem0[g + 1]; ++q) qgrp[q] = (int)g;
        for (size_t i = 0; i + 1 < bg0.size(); ++i) {
            int nl = 0;
            for (int g = bg0[i]; g < bg0[i + 1]; ++g) large[g] = col_len(g) > (size_t)RANK_SMALL ? nl++ : 0;
        }
        const size_t nh = out->rank_hist ? (size_t)n_bins * S * N : 0;
        Carve Rv;   // 8-byte slices first
        const auto o_rr = Rv.take<double>(GS), o_rb = Rv.take<double>(GS), o_rf = Rv.take<double>(GS), o_eb = Rv.take<double>(GS),
                   o_et = Rv.take<double>(GS), o_em = Rv.take<double>(GS), ord = Rv.take<double>(3 * GS), cW = Rv.take<double>(RANK_KINDS * GS),
                   cvp = Rv.take<double>(RANK_KINDS * GS), gQ = Rv.take<double>(RANK_ESS_KINDS * GS), gT = Rv.take<double>(RANK_ESS_KINDS * GS);
        const auto hist = Rv.take<unsigned long long>(nh);
        const auto o_st = Rv.take<int>(4 * GS), gst = Rv.take<int>(RANK_ESS_KINDS * GS), flag = Rv.take<int>(GS), dgm0 = Rv.take<int>(G + 1),
                   dmem = Rv.take<int>(grp.M), dq = Rv.take<int>(qgrp.size()), dlarge = Rv.take<int>(G);
        void* d = reducer_result(c, Rv.bytes);
        up(c, d, dgm0, grp.gmem0); up(c, d, dmem, grp.mem); up(c, d, dq, qgrp); up(c, d, dlarge, large);
        HIPCHK(hipMemsetAsync(flag.in(d), 0, GS * 4, c->stream));
        if (nh) HIPCHK(hipMemsetAsync(hist.in(d), 0, nh * 8, c->stream));
        unsigned long long* dh = nh ? hist.in(d) : nullptr;
        for (size_t bi = 0; bi + 1 < bg0.size(); ++bi) {
            const int g0 = bg0[bi], gn = bg0[bi + 1] - g0;
            const int q0 = 2 * grp.gmem0[g0], mtot = 2 * grp.gmem0[g0 + gn] - q0;
            const size_t Mtot = (size_t)mtot * h;
            size_t Mmax = 0, nlarge = 0;
            for (int g = g0; g < g0 + gn; ++g) { Mmax = std::max(Mmax, col_len(g)); nlarge += col_len(g) > (size_t)RANK_SMALL; }
            const unsigned nbz = (unsigned)std::min<size_t>(RANK_NBLK, std::max<size_t>(1, (Mmax + RANK_SMALL - 1) / RANK_SMALL));
            for (size_t s0 = 0; s0 < S; s0 += sb) {
                const int sbb = (int)std::min(sb, S - s0);
                const size_t E = (size_t)sbb * Mtot, Qn = (size_t)sbb * mtot;
                // the scratch of the batch: the kinds' values, the two key buffers, the ranks, the chains' moments and lags; then the 4-byte ones
                double* Y = (double*)c->st_scr;
                unsigned long long* KA = (unsigned long long*)(Y + RANK_KINDS * E);
                unsigned long long* KB = KA + E;
                long long* R2 = (long long*)(KB + E);
                double* cmu = (double*)(R2 + E);
                double* cvar = cmu + RANK_KINDS * Qn;
                double* acov = cvar + RANK_KINDS * Qn;
                unsigned* IA = (unsigned*)(acov + RANK_ESS_KINDS * Qn * LB);
                unsigned* IB = IA + E;
                int* table = (int*)(IB + E);
                const RankBatch b{dgm0.in(d), dmem.in(d), dq.in(d), dlarge.in(d), g0, gn, (int)s0, sbb, (int)S, q0, mtot, h, n, (long long)Mtot};
                const dim3 cols(gn, sbb), cells((gn * sbb + 63) / 64);
                if (mtot > 0)
                    launch_checked(c, k_rank_gather, dim3(mtot / 2), dim3(RANK_WG), 0, (const double*)P.hrec, (int)N, P.HW, (int)np, t0, b, Y + E);
                auto rank_columns = [&](int fold) {   // rank2 of every column of the batch: of x, or of |x - med|
                    launch_checked(c, k_rank_keys, dim3(gn, sbb, nbz), dim3(RANK_WG), 0, b, fold, (const double*)(Y + E), (const double*)ord.in(d),
                                   KA, IA, flag.in(d));
                    rank_sort_columns(c, b, nlarge > 0, KA, IA, KB, IB, table);
                    launch_checked(c, k_rank_ties, dim3(gn, sbb, nbz), dim3(RANK_WG), 0, b, (const unsigned long long*)KA, (const unsigned*)IA, R2);
                };
                rank_columns(0);
                launch_checked(c, k_rank_order, cells, dim3(64), 0, b, (const unsigned long long*)KA, ord.in(d));
                if (mtot > 0)
                    launch_checked(c, k_rank_scores, dim3(mtot, sbb), dim3(RANK_WG), 0, b, 0, (const long long*)R2, (const double*)ord.in(d),
                                   (const int*)flag.in(d), Y, (int)n_bins, (int)N, dh);
                rank_columns(1);
                const size_t lds = (size_t)std::min(h, STATS_LDS_N) * 8;
                if (mtot > 0) {
                    launch_checked(c, k_rank_scores, dim3(mtot, sbb), dim3(RANK_WG), 0, b, 1, (const long long*)R2, (const double*)ord.in(d),
                                   (const int*)flag.in(d), Y, (int)n_bins, (int)N, dh);
                    launch_checked(c, k_rank_chain_mom, dim3(mtot, sbb, RANK_KINDS), dim3(RANK_WG), lds, b, Y, cmu, cvar);
                }
                launch_checked(c, k_rank_cell_mom, dim3((gn * sbb * RANK_KINDS + 63) / 64), dim3(64), 0, b, (int)GS, (const double*)cmu,
                               (const double*)cvar, cW.in(d), cvp.in(d), gQ.in(d), gT.in(d), gst.in(d), o_rb.in(d), o_rf.in(d));
                for (int kb = 0; kb <= max_lag && mtot > 0; kb += RANK_WG) {   // (a cell whose sequence is truncated computes no further lag)
                    launch_checked(c, k_rank_acov, dim3(mtot, sbb, RANK_ESS_KINDS), dim3(RANK_WG), lds, b, (int)GS, kb, (int)max_lag, LB,
                                   (const double*)Y, (const int*)gst.in(d), acov);
                    launch_checked(c, k_rank_geyer, dim3(gn * sbb, RANK_ESS_KINDS), dim3(RANK_WG), 0, b, (int)GS, kb, (int)max_lag, LB,
                                   (const double*)acov, (const double*)cW.in(d), (const double*)cvp.in(d), gQ.in(d), gT.in(d), gst.in(d));
                }
                launch_checked(c, k_rank_finish, cells, dim3(64), 0, b, (int)GS, (const int*)flag.in(d), (const double*)cW.in(d),
                               (const double*)cvp.in(d), (const double*)gT.in(d), (const int*)gst.in(d), o_rr.in(d), o_rb.in(d), o_rf.in(d),
                               o_eb.in(d), o_et.in(d), o_em.in(d), o_st.in(d));
            }
        }
        down(c, d, o_rr, out->rhat_rank, GS); down(c, d, o_rb, out->rhat_bulk, GS); down(c, d, o_rf, out->rhat_folded, GS);
        down(c, d, o_eb, out->ess_bulk, GS); down(c, d, o_et, out->ess_tail, GS); down(c, d, o_em, out->ess_mean, GS);
        down(c, d, o_st, out->status, 4 * GS); down(c, d, hist, out->rank_hist, nh);
        HIPCHK(hipStreamSynchronize(c->stream));
        return SMM_OK;
    });
}

// --- the thinned draws of groups of chains, row by row (smm_draws.hpp) ---------------------------------------------------------------------

int smm_get_draws(void* ctx, int32_t t0, int32_t t1, int32_t select, const int32_t* group, int32_t n_groups, int32_t thin, int32_t max_rows,
                  int64_t rows_cap, smm_draws_t* out) {
    return api_call(ctx, out != nullptr, [&](Ctx* c) -> int {
        if (const int rc = check_select(c, select)) return rc;
        if (const int rc = check_groups(c, group, n_groups, GROUPS_DEFAULT_ONE)) return rc;
        if (thin < 1) return fail(c, SMM_ERR_INVALID_ARG, "thin must be at least 1");
        if (max_rows < 1 || max_rows > (1 << 24)) return fail(c, SMM_ERR_INVALID_ARG, "max_rows must lie in [1, 1 << 24]");
        const bool sizing = !out->params && !out->value && !out->sim_moments && !out->chain && !out->iter && !out->src_iter;
        if (!sizing && rows_cap < 0) return fail(c, SMM_ERR_INVALID_ARG, "rows_cap must be >= 0");
        if (const int rc = settled_window(c, t0, t1)) return rc;
        const KParams& P = c->P;
        const size_t N = P.N, np = P.np, nm = P.nm, G = n_groups;
        const int n = t1 - t0;
        const Groups grp = group_members(group, G, N);
        const size_t M = grp.M;
        // the masks of a chain: W words and their running popcounts over the window (select 1) or over [0, t1) (select 2); none for select 0
        const int tb = select == 1 ? t0 : 0, W = select == 0 ? 0 : (t1 - tb + 63) / 64;
        const size_t per_chain = (size_t)W * 12;
        // the sizes first: the members' prefixes, m_g and min(m_g, K) on the device, the scan across the groups here
        Carve Rh;   // 8-byte slices first
        const auto prefix = Rh.take<long long>(M), dgm = Rh.take<long long>(G), dtake = Rh.take<long long>(G), drow0 = Rh.take<long long>(G + 1);
        const auto dmc = Rh.take<int>(N), dgm0 = Rh.take<int>(G + 1), dmem = Rh.take<int>(M);
        const size_t head = (Rh.bytes + 7) & ~(size_t)7;
        void* d = reducer_result(c, head);
        up(c, d, dgm0, grp.gmem0); up(c, d, dmem, grp.mem);
        int resident_c0 = -1, n_chain_batches = 0;   // the chains whose masks the scratch holds
        auto masks = [&](int c0, int nb) {
            unsigned long long* mk = (unsigned long long*)c->st_scr;
            launch_checked(c, k_draws_mask, dim3((nb + 63) / 64), dim3(DRAWS_WG), 0, (const double*)P.hrec, (int)N, P.HW, tb, t1, c0, nb, W, mk,
                           (unsigned*)(mk + (size_t)nb * W), dmc.in(d));
            resident_c0 = c0;
        };
        if (W > 0) {
            reducer_scratch(c, per_chain);
            chain_batches(c, per_chain, [&](int, int) { ++n_chain_batches; });
        }
        if (select == 1) {
            HIPCHK(hipMemsetAsync(dmc.in(d), 0, N * 4, c->stream));   // (an empty window: no word, no set bit)
            if (W > 0) chain_batches(c, per_chain, masks);
        }
        std::vector<long long> gm(G, 0), take(G, 0), row0(G + 1, 0);
        if (G > 0) {
            launch_checked(c, k_draws_offsets, dim3((unsigned)G), dim3(DRAWS_WG), 0, (const int*)dmem.in(d), (const int*)dgm0.in(d),
                           select == 1 ? (const int*)dmc.in(d) : (const int*)nullptr, n, (int)thin, (long long)max_rows, prefix.in(d), dgm.in(d),
                           dtake.in(d));
            down(c, d, dgm, gm.data(), G); down(c, d, dtake, take.data(), G);
        }
        HIPCHK(hipStreamSynchronize(c->stream));
        for (size_t g = 0; g < G; ++g) row0[g + 1] = row0[g] + take[g];
        const long long R = row0[G];
        if (!sizing && R > rows_cap)
            return fail(c, SMM_ERR_INVALID_ARG, "smm_get_draws: the call writes " + std::to_string(R) + " rows, rows_cap is " + std::to_string(rows_cap));
        if (out->count) std::copy(gm.begin(), gm.end(), out->count);
        if (out->n_chains) std::copy(grp.n_chains.begin(), grp.n_chains.end(), out->n_chains);
        if (out->row0) std::copy(row0.begin(), row0.end(), out->row0);
        if (sizing || R == 0) return SMM_OK;
        // the rows, in batches that fit the cap of the result buffer (at least one row); a batch's rows of every chain batch's chains
        const size_t row_bytes = 8 * (np + 1 + nm) + 12;
        const size_t rb = (size_t)std::min<long long>(R, (long long)std::max<size_t>(1, reducer_batch_cap(c) / row_bytes));
        Carve Rv;
        Rv.bytes = head;
        const auto o_par = Rv.take<double>(out->params ? rb * np : 0), o_val = Rv.take<double>(out->value ? rb : 0),
                   o_mom = Rv.take<double>(out->sim_moments ? rb * nm : 0);
        const auto o_chain = Rv.take<int>(out->chain ? rb : 0), o_iter = Rv.take<int>(out->iter ? rb : 0), o_src = Rv.take<int>(out->src_iter ? rb : 0);
        if (Rv.bytes > c->red_res_bytes) {   // (growing the buffer frees it: the head's tables move with it)
            std::vector<char> keep(head);
            HIPCHK(hipMemcpy(keep.data(), d, head, hipMemcpyDeviceToHost));
            d = reducer_result(c, Rv.bytes);
            HIPCHK(hipMemcpy(d, keep.data(), head, hipMemcpyHostToDevice));
        }
        up(c, d, drow0, row0);
        for (long long r0 = 0; r0 < R; r0 += (long long)rb) {
            const int rn = (int)std::min<long long>((long long)rb, R - r0);
            auto gather = [&](int c0, int nb) {
                if (W > 0 && (n_chain_batches > 1 || resident_c0 != c0)) masks(c0, nb);
                const unsigned long long* mk = (const unsigned long long*)c->st_scr;
                launch_checked(c, k_draws_gather, dim3((rn + DRAWS_WG - 1) / DRAWS_WG), dim3(DRAWS_WG), 0, (const double*)P.hrec, (int)N, P.HW,
                               (int)np, (int)nm, t0, (int)select, (int)thin, (const int*)dmem.in(d), (const int*)dgm0.in(d), (int)G,
                               (const long long*)drow0.in(d), (const long long*)prefix.in(d), (const long long*)dgm.in(d), c0, nb, W, tb,
                               W > 0 ? mk : nullptr, W > 0 ? (const unsigned*)(mk + (size_t)nb * W) : nullptr, P.offset, r0, rn,
                               out->params ? o_par.in(d) : (double*)nullptr, out->value ? o_val.in(d) : (double*)nullptr,
                               out->sim_moments ? o_mom.in(d) : (double*)nullptr, out->chain ? o_chain.in(d) : (int*)nullptr,
                               out->iter ? o_iter.in(d) : (int*)nullptr, out->src_iter ? o_src.in(d) : (int*)nullptr);
            };
            if (W > 0) chain_batches(c, per_chain, gather);
            else gather(0, (int)N);
            down(c, d, o_par, out->params ? out->params + (size_t)r0 * np : nullptr, (size_t)rn * np);
            down(c, d, o_val, out->value ? out->value + r0 : nullptr, (size_t)rn);
            down(c, d, o_mom, out->sim_moments ? out->sim_moments + (size_t)r0 * nm : nullptr, (size_t)rn * nm);
            down(c, d, o_chain, out->chain ? out->chain + r0 : nullptr, (size_t)rn);
            down(c, d, o_iter, out->iter ? out->iter + r0 : nullptr, (size_t)rn);
            down(c, d, o_src, out->src_iter ? out->src_iter + r0 : nullptr, (size_t)rn);
            HIPCHK(hipStreamSynchronize(c->stream));   // (the next batch reuses the rows)
        }
        return SMM_OK;
    });
}

// --- simulated moments per group: fit, Jacobian, sensitivity, standard errors (smm_moments.hpp) -------------------------------------------

int smm_get_moment_stats(void* ctx, int32_t t0, int32_t t1, int32_t select, const int32_t* group, int32_t n_groups, const double* probs,
                         int32_t n_probs, double ridge, smm_moment_stats_t* out) {
    return api_call(ctx, out != nullptr, [&](Ctx* c) -> int {
        if (const int rc = check_select(c, select)) return rc;
        if (const int rc = check_groups(c, group, n_groups, GROUPS_DEFAULT_ONE)) return rc;
        if (const int rc = check_probs(c, probs, n_probs, out->m_quantile != nullptr)) return rc;
        if (!(ridge >= 0.0) || !std::isfinite(ridge)) return fail(c, SMM_ERR_INVALID_ARG, "ridge must be finite and >= 0");
        if (const int rc = settled_window(c, t0, t1)) return rc;
        const KParams& P = c->P;
        const size_t N = P.N, np = P.np, nm = P.nm, D = np + nm, G = n_groups, nq = out->m_quantile ? n_probs : 0;
        const int n = t1 - t0;
        const bool med = out->m_median != nullptr, ord = med || nq > 0;
        const bool solve = out->status || out->jac || out->sens || out->se;
        const bool cov = solve || out->cov_pp || out->cov_pm || out->cov_mm || out->fit_z;
        const bool cols = cov || ord || out->p_mean || out->m_mean;
        const Groups grp = group_members(group, G, N);
        DevBuf<int> dci(2 * N);
        const PoolPlan pp = pool_plan(grp, pool_counts(c, grp, t0, n, select, dci.p));
        const long long Mtot = pp.Mtot;
        const int NC = pp.NC;
        if (out->count) std::copy(pp.gm.begin(), pp.gm.end(), out->count);
        if (out->n_chains) std::copy(grp.n_chains.begin(), grp.n_chains.end(), out->n_chains);
        if (!cols || G == 0) return SMM_OK;
        if (Mtot == 0) {   // no row in any group: status 1, everything else NaN
            auto nan = [](double* p, size_t k) { if (p) std::fill(p, p + k, NAN); };
            if (out->status) std::fill(out->status, out->status + G, 1);
            nan(out->p_mean, G * np); nan(out->m_mean, G * nm); nan(out->m_median, G * nm); nan(out->m_quantile, nq * G * nm);
            nan(out->cov_pp, G * np * np); nan(out->cov_pm, G * np * nm); nan(out->cov_mm, G * nm * nm); nan(out->fit_z, G * nm);
            nan(out->jac, G * nm * np); nan(out->sens, G * np * nm); nan(out->se, G * np);
            return SMM_OK;
        }
        const OrderPlan op = order_plan(c, pp, med, probs, nq);
        // the batch plan: kb packed joint columns at a time in the scratch; the covariance Nbc chunks at a time, every joint column of a
        // chunk in the scratch and the chunks' D x D pair sums in the result buffer, both under the cap
        reducer_scratch(c, std::max(N * (size_t)P.T * 8, cov ? D * STATS_LDS_N * 8 : 0));
        const size_t hook = c->H.stats_scratch;
        const size_t budget = hook ? std::min(c->st_scr_bytes, std::max({hook, (size_t)Mtot * 8, cov ? D * STATS_LDS_N * 8 : 0})) : c->st_scr_bytes;
        const size_t kb = std::min(D, budget / ((size_t)Mtot * 8));
        const int Nbc = !cov ? 0 : (int)std::max<size_t>(1, std::min({(size_t)NC, budget / (D * STATS_LDS_N * 8), reducer_batch_cap(c) / (D * D * 8)}));
        Carve Rv;   // 8-byte slices first
        const auto mean = Rv.take<double>(G * D), median = Rv.take<double>(G * D), quant = Rv.take<double>(nq * G * D),
                   acc = Rv.take<double>(cov ? G * D * D : 0), csum = Rv.take<double>(kb * NC),
                   csum2 = Rv.take<double>(cov ? D * D * (size_t)Nbc : 0);
        const auto o_pmean = Rv.take<double>(G * np), o_mmean = Rv.take<double>(G * nm), o_mmed = Rv.take<double>(G * nm),
                   o_mq = Rv.take<double>(nq * G * nm), o_cpp = Rv.take<double>(G * np * np), o_cpm = Rv.take<double>(G * np * nm),
                   o_cmm = Rv.take<double>(G * nm * nm), o_z = Rv.take<double>(G * nm), o_jac = Rv.take<double>(G * nm * np),
                   o_sens = Rv.take<double>(G * np * nm), o_se = Rv.take<double>(G * np);
        const PoolDev pd(Rv, pp, op, op.wgrp.size() * std::min(kb, nm));   // (the long moment columns of a batch)
        const auto cnan = Rv.take<int>(kb * NC), gnan = Rv.take<int>(G * D), gbad = Rv.take<int>(G), o_st = Rv.take<int>(G);
        void* d = reducer_result(c, Rv.bytes);
        pd.upload(c, d, pp, op);
        HIPCHK(hipMemsetAsync(gbad.in(d), 0, G * 4, c->stream));
        const int *dgid = dci.p, *dgch0 = pd.gch0.in(d), *dclen = pd.clen.in(d);
        int* dcnt = dci.p + N;
        const long long* dgm = pd.gm.in(d);
        double* col = (double*)c->st_scr;
        double* omed = med ? median.in(d) : nullptr;
        for (size_t k0 = 0; k0 < D; k0 += kb) {   // batches of joint columns: the packed columns [kbb][Mtot]
            const int kbb = (int)std::min(kb, D - k0);
            launch_checked(c, k_group_gather, dim3(N), dim3(STATS_WG), 0, (const double*)P.hrec, (int)N, P.HW, t0, n, (int)select, dgid,
                           (const long long*)pd.off.in(d), (const int*)nullptr, (int)k0, kbb, Mtot, 0, 0, (const double*)nullptr, (int)D, col,
                           dcnt, 0, gbad.in(d));
            launch_checked(c, k_group_chunk_sum, dim3(NC, kbb), dim3(STATS_WG), (size_t)STATS_LDS_N * 8, (const double*)col, Mtot,
                           (const long long*)pd.cst.in(d), dclen, NC, csum.in(d), cnan.in(d));
            launch_checked(c, k_group_mean, dim3((unsigned)((G * kbb + 255) / 256)), dim3(256), 0, (const double*)csum.in(d),
                           (const int*)cnan.in(d), NC, dgch0, dgm, (int)G, (int)k0, kbb, (int)D, mean.in(d), gnan.in(d));
            const size_t ks = std::max(k0, np);   // the batch's moment columns [ks, k0 + kbb): the order statistics are theirs alone
            if (ord && ks < k0 + kbb)
                pool_order(c, d, pd, pp, op, col + (ks - k0) * (size_t)Mtot, (int)(k0 + kbb - ks), (int)ks, (int)D, gnan.in(d), omed, quant.in(d));
        }
        if (cov) {   // batches of chunks: every joint column centred, [D][nb][STATS_LDS_N]; each chunk's pair sums, added onto the groups'
            HIPCHK(hipMemsetAsync(acc.in(d), 0, G * D * D * 8, c->stream));
            const int nt = ((int)D + COV_T - 1) / COV_T, ntiles = nt * (nt + 1) / 2;
            for (int cb0 = 0; cb0 < NC; cb0 += Nbc) {
                const int nb = std::min(Nbc, NC - cb0);
                launch_checked(c, k_group_gather, dim3(N), dim3(STATS_WG), 0, (const double*)P.hrec, (int)N, P.HW, t0, n, (int)select, dgid,
                               (const long long*)pd.off.in(d) + N, (const int*)pd.cch0.in(d), 0, (int)D, Mtot, cb0, nb, (const double*)mean.in(d),
                               (int)D, col, dcnt, 0, (int*)nullptr);
                launch_checked(c, k_cov_pairs, dim3(nb, ntiles), dim3(COV_WG), 0, (const double*)col, STATS_LDS_N, nb, 0, nb, (int)D,
                               dclen + cb0, csum2.in(d), 1);
                launch_checked(c, k_moment_cov_acc, dim3((unsigned)((G * D * (D + 1) / 2 + 255) / 256)), dim3(256), 0,
                               (const double*)csum2.in(d), nb, cb0, dgch0, (int)G, (int)D, acc.in(d));
            }
        }
        auto want = [&](const void* p, auto sl) { return p ? sl.in(d) : nullptr; };
        const MomentOut mo{want(out->status, o_st), want(out->p_mean, o_pmean), want(out->m_mean, o_mmean), want(out->m_median, o_mmed),
                           want(out->m_quantile, o_mq), want(out->cov_pp, o_cpp), want(out->cov_pm, o_cpm), want(out->cov_mm, o_cmm),
                           want(out->fit_z, o_z), want(out->jac, o_jac), want(out->sens, o_sens), want(out->se, o_se)};
        launch_checked(c, k_moment_solve, dim3((unsigned)G), dim3(MOMENT_WG), (2 * np + nm) * (np + 1) * 8,
                       cov ? (const double*)acc.in(d) : (const double*)nullptr, (const double*)mean.in(d), (const double*)omed,
                       (const double*)quant.in(d), dgm, (const int*)gbad.in(d), (int)G, (int)np, (int)nm, (int)nq, ridge,
                       P.mom, P.w, (int)solve, mo);
        down(c, d, o_st, out->status, G); down(c, d, o_pmean, out->p_mean, G * np); down(c, d, o_mmean, out->m_mean, G * nm);
        down(c, d, o_mmed, out->m_median, G * nm); down(c, d, o_mq, out->m_quantile, nq * G * nm);
        down(c, d, o_cpp, out->cov_pp, G * np * np); down(c, d, o_cpm, out->cov_pm, G * np * nm); down(c, d, o_cmm, out->cov_mm, G * nm * nm);
        down(c, d, o_z, out->fit_z, G * nm); down(c, d, o_jac, out->jac, G * nm * np); down(c, d, o_sens, out->sens, G * np * nm);
        down(c, d, o_se, out->se, G * np);
        HIPCHK(hipStreamSynchronize(c->stream));
        return SMM_OK;
    });
}

// --- the regression-adjusted posterior of groups of chains (smm_adjust.hpp) ---------------------------------------------------------------

int smm_get_adjustment(void* ctx, int32_t t0, int32_t t1, int32_t select, const int32_t* group, int32_t n_groups, double tol, int32_t kernel,
                       const double* scale, double ridge, const double* probs, int32_t n_probs, smm_adjustment_t* out) {
    return api_call(ctx, out != nullptr, [&](Ctx* c) -> int {
        if (const int rc = check_select(c, select)) return rc;
        if (const int rc = check_groups(c, group, n_groups, GROUPS_DEFAULT_ONE)) return rc;
        if (const int rc = check_probs(c, probs, n_probs, out->adj_quantile != nullptr)) return rc;
        if (!(tol > 0.0 && tol <= 1.0)) return fail(c, SMM_ERR_INVALID_ARG, "tol must lie in (0, 1]");
        if (kernel != 0 && kernel != 1) return fail(c, SMM_ERR_INVALID_ARG, "kernel must be 0 (uniform) or 1 (Epanechnikov)");
        for (int k = 0; scale && k < c->P.nm; ++k)
            if (!(std::isfinite(scale[k]) && scale[k] > 0.0)) return fail(c, SMM_ERR_INVALID_ARG, "a scale must be finite and > 0");
        if (!(ridge >= 0.0) || !std::isfinite(ridge)) return fail(c, SMM_ERR_INVALID_ARG, "ridge must be finite and >= 0");
        if (const int rc = settled_window(c, t0, t1)) return rc;
        const KParams& P = c->P;
        const size_t N = P.N, np = P.np, nm = P.nm, D = np + nm, DC = D + 2, G = n_groups, nq = out->adj_quantile ? n_probs : 0;
        const int n = t1 - t0;
        const bool pass4 = nq > 0 || out->n_outside;
        const bool cols = pass4 || out->status || out->n_kept || out->bandwidth || out->sum_w || out->ess || out->x_mean || out->raw_mean ||
                          out->beta || out->adj_mean || out->adj_sd;
        const Groups grp = group_members(group, G, N);
        DevBuf<int> dci(2 * N);
        const PoolPlan pp = pool_plan(grp, pool_counts(c, grp, t0, n, select, dci.p));
        const long long Mtot = pp.Mtot;
        const int NC = pp.NC;
        if (out->count) std::copy(pp.gm.begin(), pp.gm.end(), out->count);
        if (out->n_chains) std::copy(grp.n_chains.begin(), grp.n_chains.end(), out->n_chains);
        if (!cols || G == 0) return SMM_OK;
        if (Mtot == 0) {   // no row in any group: status 1, the doubles NaN, the integers 0
            auto nan = [](double* p, size_t k) { if (p) std::fill(p, p + k, NAN); };
            if (out->status) std::fill(out->status, out->status + G, 1);
            if (out->n_kept) std::fill(out->n_kept, out->n_kept + G, 0);
            if (out->n_outside) std::fill(out->n_outside, out->n_outside + G * np, 0);
            nan(out->bandwidth, G); nan(out->sum_w, G); nan(out->ess, G); nan(out->x_mean, G * nm); nan(out->raw_mean, G * np);
            nan(out->beta, G * nm * np); nan(out->adj_mean, G * np); nan(out->adj_sd, G * np); nan(out->adj_quantile, nq * G * np);
            return SMM_OK;
        }
        const OrderPlan op = order_plan(c, pp, false, &tol, 1);   // the bandwidth: the quantile tol of the distance column
        // the batch plan.  The scratch: one packed column (the distances, later the integer weights), Nbc chunks of the D + 2 columns
        // (whose D x D pair sums stay under the result cap), and for the select jb packed columns of adjusted parameters
        const size_t col8 = (size_t)Mtot * 8, chunk8 = DC * STATS_LDS_N * 8;
        reducer_scratch(c, 2 * N * (size_t)P.T * 8 + chunk8);
        const size_t hook = c->H.stats_scratch;
        const size_t budget = hook ? std::min(c->st_scr_bytes, std::max(hook, 2 * col8 + chunk8)) : c->st_scr_bytes;
        const size_t avail = budget - 2 * col8;   // (at least one chunk)
        const int Nbc = (int)std::max<size_t>(1, std::min({(size_t)NC, avail / 2 / chunk8, reducer_batch_cap(c) / (D * D * 8)}));
        const size_t jb = std::min(np, 1 + (avail - Nbc * chunk8) / col8);
        std::vector<int> cgrp(NC);
        for (size_t g = 0; g < G; ++g) std::fill(cgrp.begin() + pp.gch0[g], cgrp.begin() + pp.gch0[g + 1], (int)g);
        std::vector<long long> lcst(Nbc);
        for (int i = 0; i < Nbc; ++i) lcst[i] = (long long)i * STATS_LDS_N;
        // the weighted select: every group's columns of a batch of parameters, R = nq targets each
        const int R = (int)nq;
        const size_t nwc = pass4 && R ? G * jb : 0;
        const int WB = nwc ? (int)std::min(nwc, std::max((size_t)1, GROUP_HIST_CAP / ((size_t)R * GROUP_BINS * 8))) : 0;
        Carve Rv;   // 8-byte slices first
        const auto delta = Rv.take<double>(G), sums = Rv.take<double>(G * DC), mu = Rv.take<double>(G * D), zero = Rv.take<double>(G * D),
                   acc = Rv.take<double>(G * D * D), csum = Rv.take<double>(DC * Nbc), csum2 = Rv.take<double>(D * D * (size_t)Nbc),
                   betai = Rv.take<double>(G * nm * np), dscale = Rv.take<double>(scale ? nm : 0), dprobs = Rv.take<double>(nq);
        const auto o_bw = Rv.take<double>(G), o_sw = Rv.take<double>(G), o_ess = Rv.take<double>(G), o_xm = Rv.take<double>(G * nm),
                   o_rm = Rv.take<double>(G * np), o_beta = Rv.take<double>(G * nm * np), o_am = Rv.take<double>(G * np),
                   o_sd = Rv.take<double>(G * np), o_q = Rv.take<double>(nq * G * np);
        const auto o_kept = Rv.take<long long>(G), dlcst = Rv.take<long long>(Nbc), srem = Rv.take<long long>(nwc * R);
        const auto nkept = Rv.take<unsigned long long>(G), qsum = Rv.take<unsigned long long>(G), nout = Rv.take<unsigned long long>(G * np),
                   spre = Rv.take<unsigned long long>(nwc * R), sghist = Rv.take<unsigned long long>((size_t)WB * R * GROUP_BINS);
        const PoolDev pd(Rv, pp, op, op.wgrp.size());
        const auto cnan = Rv.take<int>(DC * Nbc), dcgrp = Rv.take<int>(NC), gbad = Rv.take<int>(G), st = Rv.take<int>(G);
        void* d = reducer_result(c, Rv.bytes);
        pd.upload(c, d, pp, op);
        up(c, d, dscale, scale, scale ? nm : 0); up(c, d, dprobs, probs, nq); up(c, d, dlcst, lcst); up(c, d, dcgrp, cgrp);
        auto clear = [&](auto sl, size_t count) { HIPCHK(hipMemsetAsync(sl.in(d), 0, count * sizeof(*sl.in(d)), c->stream)); };
        clear(sums, G * DC); clear(zero, G * D); clear(acc, G * D * D);   // (the running sums from 0.0; the gather's mean of zeros)
        clear(nkept, G); clear(qsum, G); clear(nout, G * np); clear(gbad, G);
        const int *dgid = dci.p, *dgch0 = pd.gch0.in(d), *dclen = pd.clen.in(d);
        int* dcnt = dci.p + N;
        const long long *dgm = pd.gm.in(d), *dG0 = pd.G0.in(d);
        double* d2col = (double*)c->st_scr;                       // [Mtot]; the select's integer weights once the bandwidth is known
        long long* qcol = (long long*)c->st_scr;
        double* buf = d2col + Mtot;                               // [DC][Nbc][STATS_LDS_N]
        double* ts = buf + (size_t)DC * Nbc * STATS_LDS_N;        // [jb][Mtot]
        // the chunks [cb0, cb0 + nb) as k_group_gather's chunked form gathers them, centred by zeros: body(rows); flag: the groups'
        // not-finite flags of the first sweep (NULL: not tested again)
        auto chunk_batches = [&](int* flag, auto body) {
            for (int cb0 = 0; cb0 < NC; cb0 += Nbc) {
                const int nb = std::min(Nbc, NC - cb0);
                launch_checked(c, k_group_gather, dim3(N), dim3(STATS_WG), 0, (const double*)P.hrec, (int)N, P.HW, t0, n, (int)select, dgid,
                               (const long long*)pd.off.in(d) + N, (const int*)pd.cch0.in(d), 0, (int)D, Mtot, cb0, nb, (const double*)zero.in(d),
                               (int)D, buf, dcnt, 0, flag);
                body(AdjRows{buf, nb, cb0, (int)np, (int)nm, dclen, (const int*)dcgrp.in(d), (const long long*)pd.cst.in(d), (const double*)P.mom,
                             (const double*)P.w, scale ? (const double*)dscale.in(d) : (const double*)nullptr, (const double*)delta.in(d),
                             (int)kernel});
            }
        };
        auto rows = [&](const AdjRows& a, int mode) {
            launch_checked(c, k_adjust_rows, dim3(STATS_LDS_N / ADJ_WG, a.nb), dim3(ADJ_WG), 0, a, mode, d2col,
                           (const double*)mu.in(d), nkept.in(d), qsum.in(d));
        };
        chunk_batches(gbad.in(d), [&](const AdjRows& a) { rows(a, 0); });
        pool_order(c, d, pd, pp, op, d2col, 1, 0, 1, gbad.in(d), nullptr, delta.in(d));
        chunk_batches(nullptr, [&](const AdjRows& a) {   // the weights; the sums of w v, w and w w
            rows(a, 1);
            launch_checked(c, k_group_chunk_sum, dim3(a.nb, DC), dim3(STATS_WG), (size_t)STATS_LDS_N * 8, (const double*)buf,
                           (long long)a.nb * STATS_LDS_N, (const long long*)dlcst.in(d), dclen + a.cb0, a.nb, csum.in(d), cnan.in(d));
            launch_checked(c, k_adjust_sum_acc, dim3((unsigned)((G * DC + 255) / 256)), dim3(256), 0, (const double*)csum.in(d), a.nb, a.cb0,
                           dgch0, (int)G, (int)DC, sums.in(d));
        });
        launch_checked(c, k_adjust_means, dim3((unsigned)((G * D + 255) / 256)), dim3(256), 0, (const double*)sums.in(d), (int)G, (int)D,
                       mu.in(d));
        const int nt = ((int)D + COV_T - 1) / COV_T, ntiles = nt * (nt + 1) / 2;
        chunk_batches(nullptr, [&](const AdjRows& a) {   // the centred, weighted columns; their pair sums
            rows(a, 2);
            launch_checked(c, k_cov_pairs, dim3(a.nb, ntiles), dim3(COV_WG), 0, (const double*)buf, STATS_LDS_N, a.nb, 0, a.nb, (int)D,
                           dclen + a.cb0, csum2.in(d), 1);
            launch_checked(c, k_moment_cov_acc, dim3((unsigned)((G * D * (D + 1) / 2 + 255) / 256)), dim3(256), 0, (const double*)csum2.in(d),
                           a.nb, a.cb0, dgch0, (int)G, (int)D, acc.in(d));
        });
        auto want = [&](const void* p, auto sl) { return p ? sl.in(d) : nullptr; };
        const AdjustOut ao{want(out->n_kept, o_kept), want(out->bandwidth, o_bw), want(out->sum_w, o_sw), want(out->ess, o_ess),
                           want(out->x_mean, o_xm), want(out->raw_mean, o_rm), want(out->beta, o_beta), want(out->adj_mean, o_am),
                           want(out->adj_sd, o_sd)};
        launch_checked(c, k_adjust_solve, dim3((unsigned)G), dim3(MOMENT_WG), (nm + np) * (nm + 1) * 8, (const double*)acc.in(d),
                       (const double*)sums.in(d), (const double*)mu.in(d), (const double*)delta.in(d), dgm, (const int*)gbad.in(d),
                       (const unsigned long long*)nkept.in(d), (int)np, (int)nm, (int)kernel, ridge, st.in(d), betai.in(d), ao);
        if (pass4) {   // batches of parameters: the adjusted columns of every group, then their weighted quantiles
            long long wmax = 0;
            for (size_t g = 0; g < G; ++g) wmax = std::max(wmax, pp.gm[g]);
            // a workgroup of a column counts blocks of per = STATS_WG x 16 consecutive rows (the seam SMMHIP_GROUP_WIDE_MIN: as few as
            // one row, so that the weights of a short column are added across workgroups)
            const long long per = std::min<long long>(STATS_WG * 16, std::max<long long>(1, c->H.group_wide_min - 1));
            const int B = (int)std::min<long long>(1024, std::max<long long>(1, (wmax + per - 1) / per));
            for (size_t j0 = 0; j0 < np; j0 += jb) {
                const int jbb = (int)std::min(jb, np - j0);
                chunk_batches(nullptr, [&](const AdjRows& a) {
                    launch_checked(c, k_adjust_apply, dim3(STATS_LDS_N / ADJ_WG, a.nb), dim3(ADJ_WG), nm * jbb * 8 + (size_t)jbb * 4, a, (int)j0,
                                   jbb, Mtot, (const int*)st.in(d), (const double*)betai.in(d), (const double*)P.lb, (const double*)P.ub, ts,
                                   qcol, nout.in(d));
                });
                if (!R) continue;
                const int nw = (int)G * jbb;
                launch_checked(c, k_adjust_targets, dim3((unsigned)((nw * R + 255) / 256)), dim3(256), 0, (const unsigned long long*)qsum.in(d),
                               (const int*)st.in(d), (const double*)dprobs.in(d), (int)G, jbb, R, srem.in(d), spre.in(d));
                HIPCHK(hipMemsetAsync(sghist.in(d), 0, (size_t)WB * R * GROUP_BINS * 8, c->stream));   // (k_group_pick zeroes it again)
                radix_digits(c, nw, R, WB, sghist.in(d), srem.in(d), spre.in(d), [&](int w0, int wn, int dg) {
                    launch_checked(c, k_adjust_hist, dim3(wn, B, (R + ADJ_RB - 1) / ADJ_RB), dim3(STATS_WG), 0, (const double*)ts,
                                   (const long long*)qcol, Mtot, dG0, dgm, jbb, R, dg, w0, per, (const long long*)srem.in(d),
                                   (const unsigned long long*)spre.in(d), sghist.in(d));
                });
                launch_checked(c, k_adjust_finish, dim3((unsigned)((nw * R + 255) / 256)), dim3(256), 0, (const unsigned long long*)spre.in(d),
                               (const int*)st.in(d), (int)G, (int)np, (int)j0, jbb, R, o_q.in(d));
            }
        }
        down(c, d, st, out->status, G); down(c, d, o_kept, out->n_kept, G); down(c, d, o_bw, out->bandwidth, G);
        down(c, d, o_sw, out->sum_w, G); down(c, d, o_ess, out->ess, G); down(c, d, o_xm, out->x_mean, G * nm);
        down(c, d, o_rm, out->raw_mean, G * np); down(c, d, o_beta, out->beta, G * nm * np); down(c, d, o_am, out->adj_mean, G * np);
        down(c, d, o_sd, out->adj_sd, G * np); down(c, d, o_q, out->adj_quantile, nq * G * np); down(c, d, nout, out->n_outside, G * np);
        HIPCHK(hipStreamSynchronize(c->stream));
        return SMM_OK;
    });
}

// --- the target posterior from every temperature (smm_reweight.hpp) ----------------------------------------------------------------------

int smm_get_reweighted(void* ctx, int32_t t0, int32_t t1, int32_t select, const int32_t* group, int32_t n_groups, const double* targets,
                       int32_t n_targets, const double* probs, int32_t n_probs, smm_reweighted_t* out) {
    return api_call(ctx, out != nullptr, [&](Ctx* c) -> int {
        if (const int rc = check_select(c, select)) return rc;
        if (const int rc = check_groups(c, group, n_groups, GROUPS_DEFAULT_ONE)) return rc;
        if (n_targets < 1 || n_targets > 64 || !targets) return fail(c, SMM_ERR_INVALID_ARG, "n_targets must lie in [1, 64], targets not NULL");
        for (int r = 0; r < n_targets; ++r)
            if (!(std::isfinite(targets[r]) && targets[r] >= 0.0)) return fail(c, SMM_ERR_INVALID_ARG, "a target must be finite and >= 0");
        if (const int rc = check_probs(c, probs, n_probs, out->quantile != nullptr)) return rc;
        if (const int rc = settled_window(c, t0, t1)) return rc;
        const KParams& P = c->P;
        const size_t N = P.N, np = P.np, nm = P.nm, D = np + nm, D1 = D + 1, DC = D + 3, G = n_groups, R = n_targets,
                     nq = out->quantile ? n_probs : 0;
        const int n = t1 - t0;
        const bool wants_cov = out->cov != nullptr;
        const bool grp_out = nq > 0 || wants_cov || out->status || out->n_kept || out->sum_u || out->ess || out->mean || out->value_mean ||
                             out->m_mean;
        const bool chain_out = out->chain_ess || out->chain_logz;
        const Groups grp = group_members(group, G, N);
        // the counting walk: every chain's selected and scored rows
        DevBuf<int> dci(3 * N);   // the chains' groups, then cnt [2][N]
        int *dgid = dci.p, *dcnt = dci.p + N, *dnsc = dci.p + 2 * N;
        std::vector<int> cnt(2 * N);
        HIPCHK(hipMemcpyAsync(dgid, grp.gid.data(), N * 4, hipMemcpyHostToDevice, c->stream));
        launch_checked(c, k_rw_walk, dim3(N), dim3(RW_WG), 0, (const double*)P.hrec, (int)N, P.HW, t0, n, (int)select, (const int*)dgid,
                       (const long long*)nullptr, 1, dcnt, (int*)nullptr, (int*)nullptr, (double*)nullptr);
        HIPCHK(hipMemcpyAsync(cnt.data(), dcnt, 2 * N * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        const std::vector<int> nsc(cnt.begin() + N, cnt.end());
        const PoolPlan pp = pool_plan(grp, nsc);   // the pooled index space of the scored rows
        const long long Mtot = pp.Mtot;
        const int NC = pp.NC;
        for (size_t g = 0; g < G && out->count; ++g) {
            out->count[g] = 0;
            for (int i = grp.gmem0[g]; i < grp.gmem0[g + 1]; ++i) out->count[g] += cnt[grp.mem[i]];
        }
        if (out->n_scored) std::copy(pp.gm.begin(), pp.gm.end(), out->n_scored);
        if (out->n_chains) std::copy(grp.n_chains.begin(), grp.n_chains.end(), out->n_chains);
        if (out->chain_n) std::copy(nsc.begin(), nsc.end(), out->chain_n);
        if (!grp_out && !chain_out) return SMM_OK;
        // a chain without a scored row (or in no group) takes no part: chain_ess 0, chain_logz NaN
        auto idle_chains = [&] {
            for (size_t r = 0; r < R; ++r)
                for (size_t i = 0; i < N; ++i)
                    if (nsc[i] == 0) {
                        if (out->chain_ess) out->chain_ess[r * N + i] = 0.0;
                        if (out->chain_logz) out->chain_logz[r * N + i] = NAN;
                    }
        };
        if (Mtot == 0) {   // no scored row in any group: status 1, the doubles NaN, the integers 0
            auto nan = [](double* p, size_t k) { if (p) std::fill(p, p + k, NAN); };
            if (out->status) std::fill(out->status, out->status + R * G, 1);
            if (out->n_kept) std::fill(out->n_kept, out->n_kept + R * G, 0);
            nan(out->sum_u, R * G); nan(out->ess, R * G); nan(out->mean, R * G * np); nan(out->cov, R * G * np * np);
            nan(out->value_mean, R * G); nan(out->m_mean, R * G * nm); nan(out->quantile, nq * R * G * np);
            idle_chains();
            return SMM_OK;
        }
        std::vector<int> act;   // the member chains with a scored row
        for (int i : grp.mem)
            if (nsc[i] > 0) act.push_back(i);
        // the batch plan.  The scratch: four packed columns (history row and chain, v, w, q), Nbc chunks of the D + 3 columns (whose
        // np x np pair sums stay under the result cap), and for the select jb packed columns of parameters.  Five columns and one
        // chunk are the minimum; up to the batch cap more is asked for, so that a window that fills the capacity is not taken one
        // chunk and one parameter at a time
        const size_t col8 = (size_t)Mtot * 8, chunk8 = DC * STATS_LDS_N * 8, cap8 = N * (size_t)P.T * 8;
        const size_t room = std::min(reducer_batch_cap(c), 2 * ((cap8 / 8 / STATS_LDS_N + N) * chunk8 + np * cap8));
        reducer_scratch(c, 5 * cap8 + chunk8 + room);
        const size_t hook = c->H.stats_scratch;
        const size_t budget = hook ? std::min(c->st_scr_bytes, std::max(hook, 5 * col8 + chunk8)) : c->st_scr_bytes;
        const size_t avail = budget - 5 * col8;   // (at least one chunk)
        const int Nbc = (int)std::max<size_t>(1, std::min({(size_t)NC, avail / 2 / chunk8, reducer_batch_cap(c) / (np * np * 8)}));
        const size_t jb = std::min(np, 1 + (avail - Nbc * chunk8) / col8);
        std::vector<int> cgrp(NC);
        for (size_t g = 0; g < G; ++g) std::fill(cgrp.begin() + pp.gch0[g], cgrp.begin() + pp.gch0[g + 1], (int)g);
        std::vector<long long> lcst(Nbc);
        for (int i = 0; i < Nbc; ++i) lcst[i] = (long long)i * STATS_LDS_N;
        const int Rq = (int)nq;   // the weighted select: every group's columns of a batch of parameters, nq targets each
        const size_t nwc = Rq ? G * jb : 0;
        const int WB = nwc ? (int)std::min(nwc, std::max((size_t)1, GROUP_HIST_CAP / ((size_t)Rq * GROUP_BINS * 8))) : 0;
        Carve Rv;   // 8-byte slices first
        const auto sums = Rv.take<double>(G * DC), mu = Rv.take<double>(G * D1), acc = Rv.take<double>(G * np * np),
                   csum = Rv.take<double>(DC * Nbc), csum2 = Rv.take<double>(np * np * (size_t)Nbc), fc = Rv.take<double>(N),
                   Lc = Rv.take<double>(N), F = Rv.take<double>(G), dprobs = Rv.take<double>(nq), tq = Rv.take<double>(nq * G * np);
        const auto o_cess = Rv.take<double>(R * N), o_clz = Rv.take<double>(R * N), o_su = Rv.take<double>(R * G), o_ess = Rv.take<double>(R * G),
                   o_mean = Rv.take<double>(R * G * np), o_cov = Rv.take<double>(wants_cov ? R * G * np * np : 0),
                   o_vm = Rv.take<double>(R * G), o_mm = Rv.take<double>(R * G * nm);
        const auto o_kept = Rv.take<long long>(R * G), dlcst = Rv.take<long long>(Nbc), srem = Rv.take<long long>(nwc * Rq),
                   doff = Rv.take<long long>(N), dG0 = Rv.take<long long>(G + 1), dgm = Rv.take<long long>(G), dcst = Rv.take<long long>(NC);
        const auto nkept = Rv.take<unsigned long long>(G), qsum = Rv.take<unsigned long long>(G),
                   spre = Rv.take<unsigned long long>(nwc * Rq), sghist = Rv.take<unsigned long long>((size_t)WB * Rq * GROUP_BINS);
        const auto dact = Rv.take<int>(act.size()), dmem = Rv.take<int>(grp.mem.size()), dgmem0 = Rv.take<int>(G + 1),
                   dgch0 = Rv.take<int>(G + 1), dclen = Rv.take<int>(NC), dcgrp = Rv.take<int>(NC), cnan = Rv.take<int>(DC * Nbc),
                   gbad = Rv.take<int>(G), bad3 = Rv.take<int>(G), st = Rv.take<int>(G), o_st = Rv.take<int>(R * G);
        void* d = reducer_result(c, Rv.bytes);
        up(c, d, dprobs, probs, nq); up(c, d, dlcst, lcst); up(c, d, doff, pp.off); up(c, d, dG0, pp.G0); up(c, d, dgm, pp.gm);
        up(c, d, dcst, pp.cst); up(c, d, dact, act); up(c, d, dmem, grp.mem); up(c, d, dgmem0, grp.gmem0); up(c, d, dgch0, pp.gch0);
        up(c, d, dclen, pp.clen); up(c, d, dcgrp, cgrp);
        auto clear = [&](auto sl, size_t count) { HIPCHK(hipMemsetAsync(sl.in(d), 0, count * sizeof(*sl.in(d)), c->stream)); };
        clear(gbad, G);
        int* src = (int*)c->st_scr;                                // [Mtot] the history row of a pooled row
        int* rowc = src + Mtot;                                    // [Mtot] its chain
        double* vcol = (double*)c->st_scr + Mtot;                  // [Mtot] its value
        double* wcol = vcol + Mtot;                                // [Mtot] its weight w (of the target at hand)
        long long* qcol = (long long*)(wcol + Mtot);               // [Mtot] its integer weight q
        double* buf = wcol + 2 * Mtot;                             // [DC][Nbc][STATS_LDS_N]
        double* ts = buf + (size_t)DC * Nbc * STATS_LDS_N;         // [jb][Mtot]
        launch_checked(c, k_rw_walk, dim3(N), dim3(RW_WG), 0, (const double*)P.hrec, (int)N, P.HW, t0, n, (int)select, (const int*)dgid,
                       (const long long*)doff.in(d), 0, dcnt, src, rowc, vcol);
        auto chunk_batches = [&](auto body) {
            for (int cb0 = 0; cb0 < NC; cb0 += Nbc) {
                const int nb = std::min(Nbc, NC - cb0);
                body(RwRows{buf, nb, cb0, (int)np, (int)nm, (int)N, P.HW, (const int*)dclen.in(d), (const int*)dcgrp.in(d),
                            (const long long*)dcst.in(d), (const double*)P.hrec, (const int*)src, (const int*)rowc, (const double*)vcol,
                            (const double*)wcol, (const double*)fc.in(d), (const double*)F.in(d)});
            }
        };
        auto rows = [&](const RwRows& a, int mode, int j0, int jbb) {
            launch_checked(c, k_rw_rows, dim3(STATS_LDS_N / RW_WG, a.nb), dim3(RW_WG), 0, a, mode, (const double*)mu.in(d), qcol,
                           nkept.in(d), qsum.in(d), gbad.in(d), j0, jbb, Mtot, ts);
        };
        long long wmax = 0;
        for (size_t g = 0; g < G; ++g) wmax = std::max(wmax, pp.gm[g]);
        const long long per = std::min<long long>(STATS_WG * 16, std::max<long long>(1, c->H.group_wide_min - 1));   // (smm_get_adjustment's)
        const int B = (int)std::min<long long>(1024, std::max<long long>(1, (wmax + per - 1) / per));
        const int nt = ((int)np + COV_T - 1) / COV_T, ntiles = nt * (nt + 1) / 2;
        auto want = [&](const void* p, auto sl) { return p ? sl.in(d) : nullptr; };
        for (size_t r = 0; r < R; ++r) {   // the targets one after another over the same packed columns
            launch_checked(c, k_rw_chain, dim3((unsigned)act.size()), dim3(RW_WG), (size_t)STATS_LDS_N * 8, (const int*)dact.in(d),
                           (const long long*)doff.in(d), (const int*)dnsc, (const double*)P.cs, (const double*)vcol, targets[r], wcol,
                           fc.in(d), Lc.in(d), out->chain_ess ? o_cess.in(d) + r * N : nullptr,
                           out->chain_logz ? o_clz.in(d) + r * N : nullptr);
            if (!grp_out) continue;
            launch_checked(c, k_rw_group, dim3((unsigned)((G + 63) / 64)), dim3(64), 0, (const int*)dmem.in(d), (const int*)dgmem0.in(d),
                           (const int*)dnsc, (const double*)fc.in(d), (const double*)Lc.in(d), (int)G, F.in(d), bad3.in(d));
            clear(sums, G * DC); clear(nkept, G); clear(qsum, G);   // (the running sums from 0.0)
            chunk_batches([&](const RwRows& a) {   // the weights; the sums of u theta, u s, u v, u and u u
                rows(a, 1, 0, 0);
                launch_checked(c, k_group_chunk_sum, dim3(a.nb, DC), dim3(STATS_WG), (size_t)STATS_LDS_N * 8, (const double*)buf,
                               (long long)a.nb * STATS_LDS_N, (const long long*)dlcst.in(d), (const int*)dclen.in(d) + a.cb0, a.nb,
                               csum.in(d), cnan.in(d));
                launch_checked(c, k_adjust_sum_acc, dim3((unsigned)((G * DC + 255) / 256)), dim3(256), 0, (const double*)csum.in(d), a.nb,
                               a.cb0, (const int*)dgch0.in(d), (int)G, (int)DC, sums.in(d));
            });
            launch_checked(c, k_adjust_means, dim3((unsigned)((G * D1 + 255) / 256)), dim3(256), 0, (const double*)sums.in(d), (int)G,
                           (int)D1, mu.in(d));
            if (wants_cov) {
                clear(acc, G * np * np);
                chunk_batches([&](const RwRows& a) {   // the centred, weighted parameter columns; their pair sums
                    rows(a, 2, 0, 0);
                    launch_checked(c, k_cov_pairs, dim3(a.nb, ntiles), dim3(COV_WG), 0, (const double*)buf, STATS_LDS_N, a.nb, 0, a.nb,
                                   (int)np, (const int*)dclen.in(d) + a.cb0, csum2.in(d), 1);
                    launch_checked(c, k_moment_cov_acc, dim3((unsigned)((G * np * (np + 1) / 2 + 255) / 256)), dim3(256), 0,
                                   (const double*)csum2.in(d), a.nb, a.cb0, (const int*)dgch0.in(d), (int)G, (int)np, acc.in(d));
                });
            }
            const RwOut ro{want(out->status, o_st.at(r * G)), want(out->n_kept, o_kept.at(r * G)), want(out->sum_u, o_su.at(r * G)),
                           want(out->ess, o_ess.at(r * G)), want(out->mean, o_mean.at(r * G * np)),
                           want(out->cov, o_cov.at(wants_cov ? r * G * np * np : 0)), want(out->value_mean, o_vm.at(r * G)),
                           want(out->m_mean, o_mm.at(r * G * nm))};
            launch_checked(c, k_rw_finish, dim3((unsigned)G), dim3(64), 0, (const double*)sums.in(d), (const double*)mu.in(d),
                           (const double*)acc.in(d), (const long long*)dgm.in(d), (const int*)gbad.in(d), (const int*)bad3.in(d),
                           (const unsigned long long*)nkept.in(d), (int)np, (int)nm, st.in(d), ro);
            if (!Rq) continue;
            for (size_t j0 = 0; j0 < np; j0 += jb) {   // batches of parameters: their packed columns, then their weighted quantiles
                const int jbb = (int)std::min(jb, np - j0);
                if (r == 0 || jb < np)
                    for (int cb0 = 0; cb0 < NC; cb0 += 65535) {   // (every chunk at once: the packed columns need no chunk buffer)
                        RwRows a{buf, std::min(65535, NC - cb0), cb0, (int)np, (int)nm, (int)N, P.HW, (const int*)dclen.in(d),
                                 (const int*)dcgrp.in(d), (const long long*)dcst.in(d), (const double*)P.hrec, (const int*)src,
                                 (const int*)rowc, (const double*)vcol, (const double*)wcol, (const double*)fc.in(d), (const double*)F.in(d)};
                        rows(a, 3, (int)j0, jbb);
                    }
                const int nw = (int)G * jbb;
                launch_checked(c, k_adjust_targets, dim3((unsigned)((nw * Rq + 255) / 256)), dim3(256), 0, (const unsigned long long*)qsum.in(d),
                               (const int*)st.in(d), (const double*)dprobs.in(d), (int)G, jbb, Rq, srem.in(d), spre.in(d));
                HIPCHK(hipMemsetAsync(sghist.in(d), 0, (size_t)WB * Rq * GROUP_BINS * 8, c->stream));   // (k_group_pick zeroes it again)
                radix_digits(c, nw, Rq, WB, sghist.in(d), srem.in(d), spre.in(d), [&](int w0, int wn, int dg) {
                    launch_checked(c, k_adjust_hist, dim3(wn, B, (Rq + ADJ_RB - 1) / ADJ_RB), dim3(STATS_WG), 0, (const double*)ts,
                                   (const long long*)qcol, Mtot, (const long long*)dG0.in(d), (const long long*)dgm.in(d), jbb, Rq, dg, w0,
                                   per, (const long long*)srem.in(d), (const unsigned long long*)spre.in(d), sghist.in(d));
                });
                launch_checked(c, k_adjust_finish, dim3((unsigned)((nw * Rq + 255) / 256)), dim3(256), 0,
                               (const unsigned long long*)spre.in(d), (const int*)st.in(d), (int)G, (int)np, (int)j0, jbb, Rq, tq.in(d));
            }
            // the target's quantiles [nq][G][np] into the caller's [nq][R][G][np]
            HIPCHK(hipMemcpy2DAsync(out->quantile + r * G * np, R * G * np * 8, tq.in(d), G * np * 8, G * np * 8, nq, hipMemcpyDeviceToHost,
                                    c->stream));
        }
        down(c, d, o_cess, out->chain_ess, R * N); down(c, d, o_clz, out->chain_logz, R * N); down(c, d, o_st, out->status, R * G);
        down(c, d, o_kept, out->n_kept, R * G); down(c, d, o_su, out->sum_u, R * G); down(c, d, o_ess, out->ess, R * G);
        down(c, d, o_mean, out->mean, R * G * np); down(c, d, o_cov, out->cov, R * G * np * np); down(c, d, o_vm, out->value_mean, R * G);
        down(c, d, o_mm, out->m_mean, R * G * nm);
        HIPCHK(hipStreamSynchronize(c->stream));
        idle_chains();
        return SMM_OK;
    });
}

// --- the objective and the moments binned along parameters (smm_profile.hpp) ------------------------------------------------------------

int smm_get_profile(void* ctx, int32_t t0, int32_t t1, int32_t select, const int32_t* group, int32_t n_groups, int32_t bins,
                    const double* range, const int32_t* pairs, int32_t n_pairs, int32_t bins2, smm_profile_t* out) {
    return api_call(ctx, out != nullptr, [&](Ctx* c) -> int {
        const size_t N = c->P.N, np = c->P.np, nm = c->P.nm;
        if (const int rc = check_select(c, select)) return rc;
        if (const int rc = check_groups(c, group, n_groups, GROUPS_DEFAULT_ONE)) return rc;
        if (bins < 1 || bins > 4096) return fail(c, SMM_ERR_INVALID_ARG, "bins must lie in [1, 4096]");
        if (range)
            for (size_t k = 0; k < np; ++k)
                if (!(std::isfinite(range[2 * k]) && std::isfinite(range[2 * k + 1]) && range[2 * k] <= range[2 * k + 1]))
                    return fail(c, SMM_ERR_INVALID_ARG, "a range row must be finite with lo <= hi");
        if (n_pairs < 0 || (size_t)n_pairs > np * np || (n_pairs > 0 && !pairs))
            return fail(c, SMM_ERR_INVALID_ARG, "n_pairs outside [0, np np], or pairs NULL with n_pairs > 0");
        for (int p = 0; p < 2 * n_pairs; ++p)
            if (pairs[p] < 0 || (size_t)pairs[p] >= np) return fail(c, SMM_ERR_INVALID_ARG, "a pair entry outside [0, np)");
        if (n_pairs > 0 && (bins2 < 1 || bins2 > 256)) return fail(c, SMM_ERR_INVALID_ARG, "bins2 must lie in [1, 256]");
        const bool cells = out->n2 || out->n_scored2 || out->v_min2 || out->min_chain2 || out->min_iter2 || out->v_mean2;
        if (n_pairs == 0 && (cells || out->edges2)) return fail(c, SMM_ERR_INVALID_ARG, "a 2-D output requested without pairs");
        if (const int rc = settled_window(c, t0, t1)) return rc;
        const KParams& P = c->P;
        const size_t G = n_groups, B = bins, B2 = n_pairs > 0 ? bins2 : 0, NP = n_pairs;
        const int n = t1 - t0;
        const bool one = out->n || out->n_scored || out->v_min || out->min_chain || out->min_iter || out->theta_at_min || out->v_mean ||
                         out->m_mean;
        const bool two = NP > 0 && (cells || out->edges2);
        const Groups grp = group_members(group, G, N);
        const int M = grp.M;
        if ((size_t)grp.longest * (size_t)n > (size_t)INT_MAX)
            return fail(c, SMM_ERR_INVALID_ARG, "a group whose pooled rows would number more than 2^31 - 1");
        const bool autor = range == nullptr, cnt_pass = autor || (out->count && select == 1);
        // the plan.  Scratch of a batch of mb members x an axes of nseg segments: mb n 12 (tab, val) + an mb (8 n + 4 nseg) (code, list,
        // table).  Results of gn groups x an axes: seg_bytes per segment.  Groups are taken while one axis of them fits both; then as many
        // axes as fit
        const size_t nseg1 = one ? B : 0, nseg2 = two && cells ? B2 * B2 : 0, nsegx = std::max(nseg1, nseg2);
        const size_t ncolx = 1 + (out->m_mean ? nm : 0);
        const size_t seg_bytes = 8 * 3 + 4 * 3 + 8 * 2 + 4 * 2 + 8 * np + 8 * nm + (8 + 4 + 8 * ncolx) /* a chunk */;
        auto scratch_of = [&](size_t mb, size_t an, size_t nseg) { return mb * (size_t)n * 12 + an * mb * (8 * (size_t)n + 4 * nseg); };
        const size_t least = scratch_of(grp.longest, 1, nsegx);
        reducer_scratch(c, least);
        const size_t hook = c->H.stats_scratch;
        const size_t budget = hook ? std::min(c->st_scr_bytes, std::max(hook, least)) : c->st_scr_bytes, rcap = reducer_batch_cap(c);
        struct GB { size_t g0, gn, mb, an1, an2; };
        std::vector<GB> plan;
        size_t segx = 0, gnx = 0, rowx = 0;
        auto axes = [&](const GB& b, size_t A, size_t nseg) {
            if (A == 0 || nseg == 0) return (size_t)0;
            size_t an = A;
            if (b.mb > 0) {
                const size_t fixed = b.mb * (size_t)n * 12, per = b.mb * (8 * (size_t)n + 4 * nseg);
                an = std::min(an, budget > fixed ? (budget - fixed) / per : 0);
            }
            an = std::max<size_t>(1, std::min(an, rcap / (b.gn * nseg * seg_bytes)));
            segx = std::max(segx, b.gn * an * nseg);
            rowx = std::max(rowx, an * b.mb * (size_t)n);
            return an;
        };
        for (size_t g0 = 0; g0 < G;) {
            GB b{g0, 0, 0, 0, 0};
            while (b.g0 + b.gn < G) {
                const size_t mb = b.mb + grp.n_chains[b.g0 + b.gn];
                if (b.gn > 0 && (scratch_of(mb, 1, nsegx) > budget || mb * (size_t)n > (size_t)INT_MAX ||
                                 (b.gn + 1) * std::max<size_t>(nsegx, 1) * seg_bytes > rcap))
                    break;
                b.mb = mb; ++b.gn;
            }
            b.an1 = axes(b, one ? np : 0, nseg1);
            b.an2 = axes(b, nseg2 ? NP : 0, nseg2);
            gnx = std::max(gnx, b.gn);
            plan.push_back(b);
            g0 += b.gn;
        }
        const size_t NCx = segx + rowx / STATS_LDS_N + 1;
        Carve Rv;   // 8-byte slices first
        const auto cmin = Rv.take<double>(autor ? N * np : 0), cmax = Rv.take<double>(autor ? N * np : 0), drng = Rv.take<double>(autor ? 0 : 2 * np),
                   dlo = Rv.take<double>(G * np), dhi = Rv.take<double>(G * np), edges = Rv.take<double>(gnx * np * (B + 1)),
                   edges2 = Rv.take<double>(two ? gnx * np * (B2 + 1) : 0), vmin = Rv.take<double>(segx), vmean = Rv.take<double>(segx),
                   theta = Rv.take<double>(out->theta_at_min ? segx * np : 0), mmean = Rv.take<double>(out->m_mean ? segx * nm : 0),
                   csum = Rv.take<double>(NCx * ncolx);
        const auto dn = Rv.take<unsigned long long>(segx), dnsc = Rv.take<unsigned long long>(segx), minkey = Rv.take<unsigned long long>(segx),
                   dcst = Rv.take<unsigned long long>(NCx);
        const auto minpos = Rv.take<unsigned>(segx), segstart = Rv.take<unsigned>(segx);
        const auto chain = Rv.take<int>(segx), iter = Rv.take<int>(segx), segch0 = Rv.take<int>(segx + 1), dclen = Rv.take<int>(NCx),
                   cbad = Rv.take<int>(autor ? N * np : 0), dcnt = Rv.take<int>(N), dst = Rv.take<int>(G * np), dgid = Rv.take<int>(N),
                   dgm0 = Rv.take<int>(G + 1), dmem = Rv.take<int>(M), dpairs = Rv.take<int>(2 * NP);
        void* d = reducer_result(c, Rv.bytes);
        up(c, d, dgid, grp.gid); up(c, d, dgm0, grp.gmem0); up(c, d, dmem, grp.mem); up(c, d, dpairs, pairs, 2 * NP);
        up(c, d, drng, range, 2 * np);
        if (cnt_pass && M > 0)
            launch_checked(c, k_hist_range, dim3(M, autor ? (unsigned)((np + HIST_KMAX - 1) / HIST_KMAX) : 1), dim3(HIST_WG), 0,
                           (const double*)P.hrec, (int)N, P.HW, t0, n, (int)select, (const int*)dmem.in(d), 0, (int)np, dcnt.in(d),
                           autor ? cmin.in(d) : (double*)nullptr, cmax.in(d), cbad.in(d));
        std::vector<unsigned long long> hnsc(segx), hcst;
        std::vector<unsigned> hstart(segx);
        std::vector<int> hch0(segx + 1), hclen;
        // a [gn][an][per] block of the batch into the caller's [G][A][per] array
        auto block = [&](auto sl, auto* dst, const GB& b, size_t a0, size_t an, size_t A, size_t per) {
            if (!dst) return;
            for (size_t gl = 0; gl < b.gn; ++gl)
                down(c, d, sl.at(gl * an * per), dst + ((b.g0 + gl) * A + a0) * per, an * per);
        };
        for (const GB& b : plan) {
            const int m0 = grp.gmem0[b.g0], mb = (int)b.mb;
            launch_checked(c, k_hist_edges, dim3((unsigned)b.gn, (unsigned)np), dim3(HIST_WG), 0, (const int*)dgm0.in(d), (const int*)dmem.in(d),
                           (int)b.g0, (int)np, (const int*)dcnt.in(d), (const double*)cmin.in(d), (const double*)cmax.in(d),
                           (const int*)cbad.in(d), autor ? (const double*)nullptr : (const double*)drng.in(d), (int)B, (int)B2, dlo.in(d),
                           dhi.in(d), dst.in(d), edges.in(d), two ? edges2.in(d) : (double*)nullptr);
            down(c, d, edges, out->edges ? out->edges + b.g0 * np * (B + 1) : nullptr, b.gn * np * (B + 1));
            if (two) down(c, d, edges2, out->edges2 ? out->edges2 + b.g0 * np * (B2 + 1) : nullptr, b.gn * np * (B2 + 1));
            double* val = (double*)c->st_scr;
            int* tab = (int*)(val + (size_t)mb * n);
            if (mb > 0 && (one || nseg2))
                launch_checked(c, k_prof_rows, dim3(mb), dim3(PROF_WG), 0, (const double*)P.hrec, (int)N, P.HW, t0, n, (int)select,
                               (const int*)dmem.in(d), m0, tab, val);
            for (int ph = 0; ph < 2; ++ph) {
                const size_t A = ph ? NP : np, an_max = ph ? b.an2 : b.an1, nseg = ph ? nseg2 : nseg1;
                if (an_max == 0) continue;
                const bool means = ph ? out->v_mean2 != nullptr : (out->v_mean || out->m_mean);
                const bool where = ph ? (out->v_min2 || out->min_chain2 || out->min_iter2)
                                      : (out->v_min || out->min_chain || out->min_iter || out->theta_at_min);
                const int ncol = ph ? 1 : (int)ncolx;
                for (size_t a0 = 0; a0 < A; a0 += an_max) {
                    const size_t an = std::min(an_max, A - a0), segs = b.gn * an * nseg, rows = an * (size_t)mb * n;
                    ProfBatch pb{};
                    pb.hrec = (const double*)P.hrec; pb.N = (int)N; pb.HW = P.HW; pb.np = (int)np; pb.nm = (int)nm; pb.t0 = t0; pb.n = n; pb.offset = P.offset;
                    pb.mem = dmem.in(d); pb.gmem0 = dgm0.in(d); pb.gid = dgid.in(d); pb.m0 = m0; pb.mb = mb; pb.g0 = (int)b.g0; pb.gn = (int)b.gn;
                    pb.two = ph; pb.a0 = (int)a0; pb.an = (int)an; pb.nseg = (int)nseg; pb.B = (int)(ph ? B2 : B);
                    pb.lds = nseg <= (size_t)std::min(PROF_LDS_SEGS, c->H.hist_lds_bins);
                    pb.pairs = dpairs.in(d); pb.st = dst.in(d); pb.lo = dlo.in(d); pb.hi = dhi.in(d); pb.edges = ph ? edges2.in(d) : edges.in(d);
                    pb.tab = tab; pb.val = val; pb.code = tab + (size_t)mb * n; pb.list = (unsigned*)pb.code + rows; pb.table = pb.list + rows;
                    pb.cnt = dn.in(d); pb.nsc = dnsc.in(d); pb.minkey = minkey.in(d); pb.minpos = minpos.in(d);
                    pb.segstart = segstart.in(d); pb.segch0 = segch0.in(d); pb.cst = dcst.in(d); pb.clen = dclen.in(d); pb.csum = csum.in(d);
                    pb.ncol = ncol;
                    pb.vmin = (ph ? out->v_min2 : out->v_min) ? vmin.in(d) : nullptr;
                    pb.chain = (ph ? out->min_chain2 : out->min_chain) ? chain.in(d) : nullptr;
                    pb.iter = (ph ? out->min_iter2 : out->min_iter) ? iter.in(d) : nullptr;
                    pb.theta = !ph && out->theta_at_min ? theta.in(d) : nullptr;
                    pb.vmean = (ph ? out->v_mean2 : out->v_mean) ? vmean.in(d) : nullptr;
                    pb.mmean = !ph && out->m_mean ? mmean.in(d) : nullptr;
                    HIPCHK(hipMemsetAsync(dn.in(d), 0, segs * 8, c->stream));
                    HIPCHK(hipMemsetAsync(minkey.in(d), 0xff, segs * 8, c->stream));
                    HIPCHK(hipMemsetAsync(minpos.in(d), 0xff, segs * 4, c->stream));
                    const unsigned sblocks = (unsigned)((segs + 255) / 256);
                    if (mb > 0) {
                        if (!pb.lds) HIPCHK(hipMemsetAsync(pb.table, 0, an * (size_t)mb * nseg * 4, c->stream));
                        launch_checked(c, k_prof_count, dim3(mb, (unsigned)an), dim3(PROF_WG), pb.lds ? nseg * 8 : 0, pb);
                    }
                    launch_checked(c, k_prof_scan, dim3(sblocks), dim3(256), 0, pb);
                    int NC = 0, longest = 1;
                    if (means) {   // the segments' starts in the axis' list and their chunks, planned on the host from the scored counts
                        HIPCHK(hipMemcpyAsync(hnsc.data(), dnsc.in(d), segs * 8, hipMemcpyDeviceToHost, c->stream));
                        HIPCHK(hipStreamSynchronize(c->stream));
                        hcst.clear(); hclen.clear();
                        for (size_t al = 0; al < an; ++al) {
                            size_t run = 0;
                            for (size_t gl = 0; gl < b.gn; ++gl)
                                for (size_t s = 0; s < nseg; ++s) { hstart[(gl * an + al) * nseg + s] = (unsigned)run; run += hnsc[(gl * an + al) * nseg + s]; }
                        }
                        for (size_t e = 0; e < segs; ++e) {
                            const size_t al = (e / nseg) % an;
                            hch0[e] = (int)hcst.size();
                            for (size_t q = 0; q < hnsc[e]; q += STATS_LDS_N) {
                                hcst.push_back(al * (size_t)mb * n + hstart[e] + q);
                                hclen.push_back((int)std::min<size_t>(STATS_LDS_N, hnsc[e] - q));
                                longest = std::max(longest, hclen.back());
                            }
                        }
                        hch0[segs] = NC = (int)hcst.size();
                        up(c, d, segstart, hstart.data(), segs); up(c, d, segch0, hch0.data(), segs + 1);
                        up(c, d, dcst, hcst.data(), (size_t)NC); up(c, d, dclen, hclen.data(), (size_t)NC);
                    }
                    if (mb > 0 && (means || where))
                        launch_checked(c, k_prof_scatter, dim3(mb, (unsigned)an), dim3(PROF_WG), pb.lds && means ? nseg * 4 : 0, pb, (int)means);
                    if (NC > 0)
                        launch_checked(c, k_prof_chunk, dim3(NC, ncol), dim3(STATS_WG), (size_t)longest * 8, pb);
                    launch_checked(c, k_prof_finish, dim3(sblocks), dim3(256), 0, pb);
                    const auto dn64 = Slice<int64_t>{dn.off}, dnsc64 = Slice<int64_t>{dnsc.off};
                    if (!ph) {
                        block(dn64, out->n, b, a0, an, A, nseg); block(dnsc64, out->n_scored, b, a0, an, A, nseg);
                        block(vmin, out->v_min, b, a0, an, A, nseg); block(chain, out->min_chain, b, a0, an, A, nseg);
                        block(iter, out->min_iter, b, a0, an, A, nseg); block(theta, out->theta_at_min, b, a0, an, A, nseg * np);
                        block(vmean, out->v_mean, b, a0, an, A, nseg); block(mmean, out->m_mean, b, a0, an, A, nseg * nm);
                    } else {
                        block(dn64, out->n2, b, a0, an, A, nseg); block(dnsc64, out->n_scored2, b, a0, an, A, nseg);
                        block(vmin, out->v_min2, b, a0, an, A, nseg); block(chain, out->min_chain2, b, a0, an, A, nseg);
                        block(iter, out->min_iter2, b, a0, an, A, nseg); block(vmean, out->v_mean2, b, a0, an, A, nseg);
                    }
                    HIPCHK(hipStreamSynchronize(c->stream));   // (the next batch reuses the tables)
                }
            }
            HIPCHK(hipStreamSynchronize(c->stream));
        }
        std::vector<int> cnt(N, n);
        if (out->count && select == 1 && M > 0) down(c, d, dcnt, cnt.data(), N);
        down(c, d, dst, out->status, G * np);
        HIPCHK(hipStreamSynchronize(c->stream));
        if (out->count) {
            std::fill(out->count, out->count + G, (int64_t)0);
            for (size_t i = 0; i < N; ++i)
                if (grp.gid[i] >= 0) out->count[grp.gid[i]] += cnt[i];
        }
        return SMM_OK;
    });
}

// --- highest-density intervals, half-sample modes and kernel densities of groups of chains (smm_density.hpp) -------------------------------

int smm_get_density(void* ctx, int32_t t0, int32_t t1, int32_t select, const int32_t* group, int32_t n_groups, const double* mass,
                    int32_t n_mass, int32_t n_grid, const double* range, const double* bw, smm_density_t* out) {
    return api_call(ctx, out != nullptr, [&](Ctx* c) -> int {
        const size_t N = c->P.N, np = c->P.np;
        if (const int rc = check_select(c, select)) return rc;
        if (const int rc = check_groups(c, group, n_groups, GROUPS_DEFAULT_ONE)) return rc;
        if (n_mass < 0 || (n_mass > 0 && !mass)) return fail(c, SMM_ERR_INVALID_ARG, "n_mass < 0, or mass NULL with n_mass > 0");
        for (int p = 0; p < n_mass; ++p)
            if (!(mass[p] > 0.0 && mass[p] <= 1.0)) return fail(c, SMM_ERR_INVALID_ARG, "a mass must lie in (0, 1]");
        if (n_mass == 0 && (out->hdi_lo || out->hdi_hi)) return fail(c, SMM_ERR_INVALID_ARG, "hdi_lo or hdi_hi requested with n_mass == 0");
        if (n_grid != 0 && (n_grid < 2 || n_grid > 4096)) return fail(c, SMM_ERR_INVALID_ARG, "n_grid must be 0 or lie in [2, 4096]");
        if (n_grid == 0 && (out->grid || out->density || out->kde_mode))
            return fail(c, SMM_ERR_INVALID_ARG, "grid, density or kde_mode requested with n_grid == 0");
        if (range)
            for (size_t k = 0; k < np; ++k)
                if (!(std::isfinite(range[2 * k]) && std::isfinite(range[2 * k + 1]) && range[2 * k] <= range[2 * k + 1]))
                    return fail(c, SMM_ERR_INVALID_ARG, "a range row must be finite with lo <= hi");
        if (bw)
            for (size_t k = 0; k < np; ++k)
                if (!(std::isfinite(bw[k]) && bw[k] > 0.0)) return fail(c, SMM_ERR_INVALID_ARG, "a bw entry must be finite and > 0");
        if (const int rc = settled_window(c, t0, t1)) return rc;
        const KParams& P = c->P;
        const size_t G = n_groups, NM = out->hdi_lo || out->hdi_hi ? n_mass : 0, NG = out->grid || out->density || out->kde_mode ? n_grid : 0;
        const int n = t1 - t0;
        const bool kde = out->bw || out->kde_status || NG > 0, rule = kde && !bw;
        const Groups grp = group_members(group, G, N);
        if ((size_t)grp.longest * (size_t)n > (size_t)INT_MAX)
            return fail(c, SMM_ERR_INVALID_ARG, "a group whose pooled rows would number more than 2^31 - 1");
        DevBuf<int> dci(2 * N);
        const PoolPlan pp = pool_plan(grp, pool_counts(c, grp, t0, n, select, dci.p));
        if (out->count) std::copy(pp.gm.begin(), pp.gm.end(), out->count);
        if (G == 0) return SMM_OK;
        // the plan.  Short columns (below the wide minimum) are sorted in LDS, the others by the radix sort: nl of them, nbig past one
        // workgroup's sort; NB blocks per grid-wide window argmin, nlev grid-wide levels of the longest column's mode
        const long long thr = c->H.group_wide_min, Mtot = pp.Mtot;
        const int NC = pp.NC;
        std::vector<int> sgrp, wgrp, large, cgrp(NC);
        std::vector<long long> toff, tlen;
        long long wmax = 0, smax = 0;
        int nbig = 0;
        for (size_t g = 0; g < G; ++g) {
            for (int ch = pp.gch0[g]; ch < pp.gch0[g + 1]; ++ch) cgrp[ch] = (int)g;
            if (pp.gm[g] < thr) { sgrp.push_back((int)g); smax = std::max(smax, pp.gm[g]); continue; }
            wgrp.push_back((int)g); toff.push_back(pp.G0[g]); tlen.push_back(pp.gm[g]);
            large.push_back(pp.gm[g] > RANK_SMALL ? nbig++ : 0);
            wmax = std::max(wmax, pp.gm[g]);
        }
        const size_t nl = wgrp.size();
        const long long per = std::min<long long>(DENS_WG * 16, std::max<long long>(1, thr - 1));
        const int NB = (int)std::min<long long>(DENS_NB_MAX, std::max<long long>(1, (wmax + per - 1) / per));
        int nlev = 0;
        for (long long q = wmax; q > 3 && q >= thr; q = (q + 1) / 2) ++nlev;
        // a parameter of every group takes its packed column and its sorted keys of the scratch, with long columns also the sort's second
        // key buffer, both index buffers and the digit tables; as many parameters at a time as fit
        const size_t one = std::max<size_t>(16, (size_t)Mtot * (nl ? 32 : 16) + (size_t)nbig * RANK_TABLE * 4);
        reducer_scratch(c, one);
        const size_t hook = c->H.stats_scratch;
        const size_t budget = hook ? std::min(c->st_scr_bytes, std::max(hook, one)) : c->st_scr_bytes;
        const size_t kb = std::max<size_t>(1, std::min(np, budget / one));
        // the curves go out in batches of groups: a group takes its grid, its density and its chunks' sums of every parameter of the batch
        struct GB { size_t g0, gn; int c0, nc; };
        std::vector<GB> plan;
        size_t gnx = 0, ncx = 0;
        for (size_t g0 = 0; g0 < G && NG > 0;) {
            GB b{g0, 0, pp.gch0[g0], 0};
            size_t bytes = 0;
            while (b.g0 + b.gn < G) {
                const int nc = pp.gch0[b.g0 + b.gn + 1] - pp.gch0[b.g0 + b.gn];
                const size_t add = kb * NG * 8 * (2 + (size_t)nc);
                if (b.gn > 0 && bytes + add > reducer_batch_cap(c)) break;
                bytes += add; ++b.gn; b.nc += nc;
            }
            gnx = std::max(gnx, b.gn); ncx = std::max(ncx, (size_t)b.nc);
            plan.push_back(b);
            g0 += b.gn;
        }
        Carve Rv;   // 8-byte slices first
        const auto dmass = Rv.take<double>(NM), drng = Rv.take<double>(range ? 2 * np : 0), dbw = Rv.take<double>(bw ? np : 0),
                   mean = Rv.take<double>(G * np), csum = Rv.take<double>(rule ? kb * NC : 0), cdev = Rv.take<double>(rule ? kb * NC : 0),
                   obw = Rv.take<double>(G * np), glo = Rv.take<double>(G * np), ghi = Rv.take<double>(G * np), omode = Rv.take<double>(G * np),
                   okmode = Rv.take<double>(G * np), hlo = Rv.take<double>(NM * G * np), hhi = Rv.take<double>(NM * G * np),
                   partw = Rv.take<double>(nl * kb * NB), csk = Rv.take<double>(kb * ncx * NG), gridb = Rv.take<double>(gnx * kb * NG),
                   densb = Rv.take<double>(gnx * kb * NG);
        const auto off = Rv.take<long long>(N), dG0 = Rv.take<long long>(G + 1), dgm = Rv.take<long long>(G), cst = Rv.take<long long>(NC),
                   dtoff = Rv.take<long long>(nl), dtlen = Rv.take<long long>(nl), mlo = Rv.take<long long>(nl * kb),
                   mn = Rv.take<long long>(nl * kb), parti = Rv.take<long long>(nl * kb * NB);
        const auto gch0 = Rv.take<int>(G + 1), clen = Rv.take<int>(NC), dcgrp = Rv.take<int>(NC), dsgrp = Rv.take<int>(sgrp.size()),
                   dwgrp = Rv.take<int>(nl), dlarge = Rv.take<int>(nl), gnan = Rv.take<int>(G * np), cnan = Rv.take<int>(rule ? kb * NC : 0),
                   status = Rv.take<int>(G * np), kst = Rv.take<int>(G * np);
        void* d = reducer_result(c, Rv.bytes);
        up(c, d, dmass, mass, NM); up(c, d, drng, range, 2 * np); up(c, d, dbw, bw, np);
        up(c, d, off, pp.off); up(c, d, dG0, pp.G0); up(c, d, dgm, pp.gm); up(c, d, cst, pp.cst); up(c, d, dtoff, toff); up(c, d, dtlen, tlen);
        up(c, d, gch0, pp.gch0); up(c, d, clen, pp.clen); up(c, d, dcgrp, cgrp); up(c, d, dsgrp, sgrp); up(c, d, dwgrp, wgrp);
        up(c, d, dlarge, large);
        HIPCHK(hipMemsetAsync(status.in(d), 0, G * np * 4, c->stream));   // (k_dens_keys only raises it)
        double* col = (double*)c->st_scr;
        unsigned long long* KA = (unsigned long long*)(col + kb * (size_t)Mtot);
        unsigned long long* KB = KA + kb * (size_t)Mtot;
        unsigned* IA = (unsigned*)(KB + kb * (size_t)Mtot);
        unsigned* IB = IA + kb * (size_t)Mtot;
        int* table = (int*)(IB + kb * (size_t)Mtot);
        const double *pmass = dmass.in(d), *prng = range ? drng.in(d) : nullptr, *pbw = bw ? dbw.in(d) : nullptr;
        const long long *pG0 = dG0.in(d), *pgm = dgm.in(d), *pcst = cst.in(d), *ptoff = dtoff.in(d), *ptlen = dtlen.in(d);
        const int *pgch0 = gch0.in(d), *pclen = clen.in(d), *pcgrp = dcgrp.in(d), *pwgrp = dwgrp.in(d), *pst = status.in(d), *pkst = kst.in(d);
        double *phlo = NM ? hlo.in(d) : nullptr, *phhi = NM ? hhi.in(d) : nullptr, *pmode = out->mode ? omode.in(d) : nullptr;
        for (size_t k0 = 0; k0 < np; k0 += kb) {   // batches of parameters: the packed columns [kbb][Mtot]
            const int kbb = (int)std::min(kb, np - k0);
            launch_checked(c, k_group_gather, dim3(N), dim3(STATS_WG), 0, (const double*)P.hrec, (int)N, P.HW, t0, n, (int)select,
                           (const int*)dci.p, (const long long*)off.in(d), (const int*)nullptr, (int)k0, kbb, Mtot, 0, 0, (const double*)nullptr,
                           (int)np, col, dci.p + N, 0, (int*)nullptr);
            if (rule && NC > 0) {   // the variance's two sums, chunk by chunk
                launch_checked(c, k_group_chunk_sum, dim3(NC, kbb), dim3(STATS_WG), (size_t)STATS_LDS_N * 8, (const double*)col, Mtot, pcst, pclen,
                               NC, csum.in(d), cnan.in(d));
                launch_checked(c, k_group_mean, dim3((unsigned)((G * kbb + 255) / 256)), dim3(256), 0, (const double*)csum.in(d),
                               (const int*)cnan.in(d), NC, pgch0, pgm, (int)G, (int)k0, kbb, (int)np, mean.in(d), gnan.in(d));
                launch_checked(c, k_dens_chunk_dev, dim3(NC, kbb), dim3(DENS_WG), (size_t)STATS_LDS_N * 8, (const double*)col, Mtot, pcst, pclen,
                               pcgrp, NC, (int)k0, (int)np, (const double*)mean.in(d), cdev.in(d));
            }
            if (!sgrp.empty())
                launch_checked(c, k_dens_small, dim3((unsigned)sgrp.size(), kbb), dim3(DENS_WG), (size_t)sort_lds_n((int)smax) * 8,
                               (const double*)col, Mtot, (const int*)dsgrp.in(d), pG0, pgm, (int)G, (int)k0, (int)np, pmass, (int)NM, KA,
                               status.in(d), phlo, phhi, pmode);
            if (nl > 0) {
                const unsigned nbz = (unsigned)std::min<long long>(RANK_NBLK, std::max<long long>(1, (wmax + RANK_SMALL - 1) / RANK_SMALL));
                launch_checked(c, k_dens_keys, dim3((unsigned)nl, kbb, nbz), dim3(DENS_WG), 0, (const double*)col, Mtot, pwgrp, ptoff, ptlen,
                               (int)k0, (int)np, KA, IA, status.in(d), mlo.in(d), mn.in(d));
                const RankBatch b{nullptr, nullptr, nullptr, dlarge.in(d), 0, (int)nl, 0, kbb, 0, 0, 0, 0, 0, Mtot, ptoff, ptlen};
                rank_sort_columns(c, b, nbig > 0, KA, IA, KB, IB, table);
                auto window = [&](int what) {   // one grid-wide argmin of every long column: the blocks' minima, then the finish
                    launch_checked(c, k_dens_win, dim3((unsigned)nl, kbb, NB), dim3(DENS_WG), 0, (const unsigned long long*)KA, Mtot, pwgrp,
                                   ptoff, ptlen, (int)k0, (int)np, pst, what, pmass, thr, (const long long*)mlo.in(d),
                                   (const long long*)mn.in(d), partw.in(d), parti.in(d));
                    launch_checked(c, k_dens_win_fin, dim3((unsigned)nl, kbb), dim3(64), 0, (const unsigned long long*)KA, Mtot, pwgrp, ptoff,
                                   ptlen, (int)G, (int)k0, (int)np, pst, what, pmass, thr, NB, (const double*)partw.in(d),
                                   (const long long*)parti.in(d), mlo.in(d), mn.in(d), phlo, phhi);
                };
                for (int p = 0; p < (int)NM; ++p) window(p);
                if (pmode) {
                    for (int lev = 0; lev < nlev; ++lev) window(-1);
                    launch_checked(c, k_dens_mode_fin, dim3((unsigned)nl, kbb), dim3(DENS_WG), (size_t)STATS_LDS_N * 8,
                                   (const unsigned long long*)KA, Mtot, pwgrp, ptoff, (int)k0, (int)np, pst, (const long long*)mlo.in(d),
                                   (const long long*)mn.in(d), pmode);
                }
            }
            if (kde)
                launch_checked(c, k_dens_bw, dim3((unsigned)((G * kbb + 255) / 256)), dim3(256), 0, (const double*)col,
                               (const unsigned long long*)KA, Mtot, pG0, pgm, pgch0, NC, (int)G, (int)k0, kbb, (int)np, pst,
                               (const double*)cdev.in(d), pbw, prng, obw.in(d), glo.in(d), ghi.in(d), kst.in(d));
            for (const GB& b : plan) {   // (none without a curve asked for)
                if (b.nc > 0)
                    launch_checked(c, k_dens_kde, dim3(b.nc, (unsigned)((NG + DENS_TILE - 1) / DENS_TILE), kbb), dim3(DENS_WG),
                                   (size_t)STATS_LDS_N * 8, (const double*)col, Mtot, pcst, pclen, pcgrp, b.c0, (int)k0, (int)np, (int)NG, pkst,
                                   (const double*)obw.in(d), (const double*)glo.in(d), (const double*)ghi.in(d), csk.in(d));
                launch_checked(c, k_dens_finish, dim3((unsigned)b.gn, kbb), dim3(64), 0, (const double*)csk.in(d), pgm, pgch0, (int)b.g0, b.c0,
                               b.nc, (int)k0, (int)np, (int)NG, pkst, (const double*)obw.in(d), (const double*)glo.in(d),
                               (const double*)ghi.in(d), out->grid ? gridb.in(d) : (double*)nullptr,
                               out->density ? densb.in(d) : (double*)nullptr, out->kde_mode ? okmode.in(d) : (double*)nullptr);
                // the batch's [gn][kbb][n_grid] block to its place in the caller's [G][np][n_grid]
                // (contiguous there when the batch holds every parameter)
                const size_t rows = (size_t)kbb == np ? 1 : b.gn, per = (size_t)kbb * NG * (b.gn / rows);
                for (size_t gl = 0; gl < rows; ++gl) {
                    const size_t at = ((b.g0 + gl) * np + k0) * NG;
                    down(c, d, gridb.at(gl * per), out->grid ? out->grid + at : nullptr, per);
                    down(c, d, densb.at(gl * per), out->density ? out->density + at : nullptr, per);
                }
                HIPCHK(hipStreamSynchronize(c->stream));   // (the next batch reuses the tables)
            }
        }
        down(c, d, status, out->status, G * np); down(c, d, kst, out->kde_status, G * np);
        down(c, d, hlo, out->hdi_lo, NM * G * np); down(c, d, hhi, out->hdi_hi, NM * G * np);
        down(c, d, omode, out->mode, G * np); down(c, d, obw, out->bw, G * np);
        if (NG > 0) down(c, d, okmode, out->kde_mode, G * np);
        HIPCHK(hipStreamSynchronize(c->stream));
        return SMM_OK;
    });
}

}  // extern "C"

// --- the posterior of user functions of each draw (smm_derived.hpp; the kernel around the user's function: smm_user_host.hpp) -----------

namespace {

// the kernel of a registered transform in this context: its module is loaded when the context first asks for it
hipFunction_t derived_kernel(Ctx* c, int32_t transform_id) {
    hipModule_t mod = nullptr;
    for (const auto& tm : c->tmods)
        if (tm.first == transform_id) mod = tm.second;
    if (!mod) {
        int n_out = 0;
        std::vector<char> code;
        user_transform_get(transform_id, &n_out, &code);
        HIPCHK(hipModuleLoadData(&mod, code.data()));
        c->tmods.emplace_back(transform_id, mod);
    }
    hipFunction_t fn = nullptr;
    HIPCHK(hipModuleGetFunction(&fn, mod, "smm_user_transform_kernel"));
    return fn;
}

// rows a workgroup of the transform's kernel stages: 256, or what 64 KiB of LDS hold at HW + 1 doubles and an index per row (whole
// waves where that is 64 or more)
constexpr size_t DERIVED_LDS_BYTES = (size_t)64 << 10;
int derived_rows_per_wg(int HW) {
    const int fit = (int)(DERIVED_LDS_BYTES / ((size_t)(HW + 2) * 8));
    return fit >= 256 ? 256 : fit >= 64 ? fit & ~63 : fit;
}

}  // namespace

extern "C" {

int smm_get_derived(void* ctx, int32_t transform_id, int32_t t0, int32_t t1, int32_t select, const int32_t* group, int32_t n_groups,
                    const double* tdata, int32_t n_tdata, const double* probs, int32_t n_probs, smm_derived_t* out) {
    return api_call(ctx, out != nullptr, [&](Ctx* c) -> int {
        int n_out = 0;
        if (!user_transform_get(transform_id, &n_out, nullptr))
            return fail(c, SMM_ERR_INVALID_ARG, "transform_id is no handle of smm_register_user_transform");
        if (const int rc = check_select(c, select)) return rc;
        if (const int rc = check_groups(c, group, n_groups, GROUPS_DEFAULT_ONE)) return rc;
        if (const int rc = check_probs(c, probs, n_probs, out->quantile != nullptr)) return rc;
        if (n_tdata < 0 || n_tdata > 4096 || (n_tdata > 0 && !tdata))
            return fail(c, SMM_ERR_INVALID_ARG, "n_tdata outside [0, 4096], or tdata NULL with n_tdata > 0");
        if (const int rc = settled_window(c, t0, t1)) return rc;
        const KParams& P = c->P;
        const size_t N = P.N, Q = n_out, G = n_groups, nq = out->quantile ? n_probs : 0, L = STATS_LDS_N;
        const int n = t1 - t0;
        const bool med = out->median != nullptr, ord = med || nq > 0, cov = out->cov != nullptr,
                   cols = out->mean || ord || cov || out->n_nonfinite;
        const Groups grp = group_members(group, G, N);
        DevBuf<int> dci(2 * N);
        const PoolPlan pp = pool_plan(grp, pool_counts(c, grp, t0, n, select, dci.p));
        const OrderPlan op = order_plan(c, pp, med, probs, nq);
        const long long Mtot = pp.Mtot;
        const int NC = pp.NC;
        std::vector<int> cgrp(NC);
        for (size_t g = 0; g < G; ++g)
            for (int ch = pp.gch0[g]; ch < pp.gch0[g + 1]; ++ch) cgrp[ch] = (int)g;
        // the plan.  The scratch holds the packed columns of a batch of outputs, [qb][Mtot], and behind them the row indexes of a batch
        // of chunks (rcap rows: at least one chunk); for the covariance, every output of a batch of chunks centred, [Q][Nbc][8192], and
        // behind them the batch's row indexes.  A batch of either kind runs the transform again, so the scratch is grown to every
        // output and the row indexes of the context's whole capacity where the cap allows that.
        size_t qb = 0, rcap = 0, Nbc = 0;
        if (Mtot > 0 && cols) {
            const size_t cap_rows = N * (size_t)P.T;
            reducer_scratch(c, std::max({(cap_rows + L) * 8, cov ? (Q + 1) * L * 8 : 0, std::min(reducer_batch_cap(c), (Q + 1) * cap_rows * 8)}));
            const size_t least = std::max(((size_t)Mtot + L) * 8, cov ? (Q + 1) * L * 8 : 0), hook = c->H.stats_scratch;
            const size_t budget = hook ? std::min(c->st_scr_bytes, std::max(hook, least)) : c->st_scr_bytes;
            qb = std::min(Q, (budget - L * 8) / ((size_t)Mtot * 8));
            rcap = (budget - qb * (size_t)Mtot * 8) / 8;
            Nbc = std::min<size_t>(NC, budget / ((Q + 1) * L * 8));
        }
        Carve Rv;   // 8-byte slices first
        const auto mean = Rv.take<double>(G * Q), median = Rv.take<double>(G * Q), quant = Rv.take<double>(nq * G * Q),
                   covo = Rv.take<double>(cov ? G * Q * Q : 0), csum = Rv.take<double>(qb * NC),
                   csum2 = Rv.take<double>(cov ? Q * Q * NC : 0), dtd = Rv.take<double>(n_tdata);
        const auto nnf = Rv.take<unsigned long long>(G * Q);
        const PoolDev pd(Rv, pp, op, op.wgrp.size() * qb);   // (the long columns of a batch of outputs)
        const auto cnan = Rv.take<int>(qb * NC), gnan = Rv.take<int>(G * Q), dcgrp = Rv.take<int>(NC);
        void* d = reducer_result(c, Rv.bytes);
        pd.upload(c, d, pp, op);
        up(c, d, dtd, tdata, n_tdata); up(c, d, dcgrp, cgrp);
        HIPCHK(hipMemsetAsync(nnf.in(d), 0, G * Q * 8, c->stream));
        const int *dgid = dci.p, *dcnt = dci.p + N, *dgch0 = pd.gch0.in(d), *dclen = pd.clen.in(d);
        const long long* dgm = pd.gm.in(d);
        if (qb > 0) {
            const hipFunction_t fn = derived_kernel(c, transform_id);
            const int R = derived_rows_per_wg(P.HW);
            const size_t smem = (size_t)R * (P.HW + 2) * 8;
            double* col = (double*)c->st_scr;
            // the chunks [cb0, cb0 + nb) through the transform: their rows' indexes (k_derived_rows), then the user's kernel, which
            // stores the outputs [q0, q0 + qn) packed (chunked == 0: col [qn][Mtot]) or all of them centred and chunked ([Q][nb][8192])
            auto transform = [&](int cb0, int nb, int q0, int qn, int chunked, long long* ridx) {
                long long p0 = pp.cst[cb0], p1 = pp.cst[cb0 + nb - 1] + pp.clen[cb0 + nb - 1], cstride = chunked ? (long long)L : Mtot;
                launch_checked(c, k_derived_rows, dim3(N), dim3(WINDOW_WG), 0, (const double*)P.hrec, (int)N, P.HW, t0, n, (int)select, dgid,
                               (const long long*)pd.off.in(d), dcnt, p0, p1, ridx);
                int longest = 0;
                for (int ch = cb0; ch < cb0 + nb; ++ch) longest = std::max(longest, pp.clen[ch]);
                // (tdata is never NULL on the device: a function that reads past n_tdata == 0 reads the result buffer, not address 0)
                const double *hrec = P.hrec, *mom = P.mom, *w = P.w, *ud = P.objp, *td = dtd.in(d), *gmean = mean.in(d);
                const long long *cridx = ridx, *cst = pd.cst.in(d);
                const int* pcgrp = dcgrp.in(d);
                int HW = P.HW, np = P.np, nm = P.nm, nud = c->n_objp, ntd = n_tdata, rows = R;
                unsigned long long* pnnf = nnf.in(d);
                void* args[] = {(void*)&hrec, (void*)&HW, (void*)&np, (void*)&nm, (void*)&cridx, (void*)&p0, (void*)&cst, (void*)&dclen,
                                (void*)&pcgrp, (void*)&cb0, (void*)&rows, (void*)&mom, (void*)&w, (void*)&ud, (void*)&nud, (void*)&td,
                                (void*)&ntd, (void*)&q0, (void*)&qn, (void*)&cstride, (void*)&chunked, (void*)&nb, (void*)&gmean,
                                (void*)&col, (void*)&pnnf};
                HIPCHK(hipModuleLaunchKernel(fn, (unsigned)((longest + R - 1) / R), (unsigned)nb, 1, 256, 1, 1, (unsigned)smem, c->stream, args,
                                             nullptr));
            };
            for (size_t q0 = 0; q0 < Q; q0 += qb) {   // batches of outputs: the packed columns [qn][Mtot], filled in batches of chunks
                const int qn = (int)std::min(qb, Q - q0);
                long long* ridx = (long long*)(col + (size_t)qn * Mtot);
                for (int cb0 = 0, nb; cb0 < NC; cb0 += nb) {
                    size_t rows = pp.clen[cb0];
                    for (nb = 1; cb0 + nb < NC && rows + pp.clen[cb0 + nb] <= rcap; ++nb) rows += pp.clen[cb0 + nb];
                    transform(cb0, nb, (int)q0, qn, 0, ridx);
                }
                launch_checked(c, k_group_chunk_sum, dim3(NC, qn), dim3(STATS_WG), (size_t)STATS_LDS_N * 8, (const double*)col, Mtot,
                               (const long long*)pd.cst.in(d), dclen, NC, csum.in(d), cnan.in(d));
                launch_checked(c, k_group_mean, dim3((unsigned)((G * qn + 255) / 256)), dim3(256), 0, (const double*)csum.in(d),
                               (const int*)cnan.in(d), NC, dgch0, dgm, (int)G, (int)q0, qn, (int)Q, mean.in(d), gnan.in(d));
                if (ord)
                    pool_order(c, d, pd, pp, op, col, qn, (int)q0, (int)Q, gnan.in(d), med ? median.in(d) : nullptr, quant.in(d));
            }
            if (cov) {   // batches of chunks: every output recomputed and centred; each chunk's pair sums, then the groups'
                const int nt = ((int)Q + COV_T - 1) / COV_T, ntiles = nt * (nt + 1) / 2;
                for (int cb0 = 0; cb0 < NC; cb0 += (int)Nbc) {
                    const int nb = std::min((int)Nbc, NC - cb0);
                    transform(cb0, nb, 0, (int)Q, 1, (long long*)(col + Q * (size_t)nb * L));
                    launch_checked(c, k_cov_pairs, dim3(nb, ntiles), dim3(COV_WG), 0, (const double*)col, STATS_LDS_N, NC, cb0, nb, (int)Q,
                                   dclen, csum2.in(d), 1);
                }
            }
        }
        if (cov && G > 0)
            launch_checked(c, k_group_cov, dim3((unsigned)((G * Q * (Q + 1) / 2 + 255) / 256)), dim3(256), 0, (const double*)csum2.in(d),
                           NC, dgch0, dgm, (int)G, (int)Q, covo.in(d));
        if (qb > 0) {   // (no row in any group: every summary NaN, filled below)
            down(c, d, mean, out->mean, G * Q);
            down(c, d, median, out->median, G * Q);
            down(c, d, quant, out->quantile, nq * G * Q);
        }
        down(c, d, covo, out->cov, G * Q * Q);
        down(c, d, nnf, out->n_nonfinite, G * Q);
        HIPCHK(hipStreamSynchronize(c->stream));
        if (qb == 0) {
            if (out->mean) std::fill(out->mean, out->mean + G * Q, NAN);
            if (out->median) std::fill(out->median, out->median + G * Q, NAN);
            if (out->quantile) std::fill(out->quantile, out->quantile + nq * G * Q, NAN);
        }
        if (out->count) std::copy(pp.gm.begin(), pp.gm.end(), out->count);
        if (out->n_chains) std::copy(grp.n_chains.begin(), grp.n_chains.end(), out->n_chains);
        return SMM_OK;
    });
}

}  // extern "C"
