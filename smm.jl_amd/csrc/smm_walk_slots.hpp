// the exchange walk on 16-byte chain slots and the unpadded level plan (exchangeMoves!, AlgoBGP.jl:647-716; any thresholds, the
// dist_fun menu): its staging, its level loop, and the two inline forms built of them, exchange_walk_tile (k_chain_iter) and
// exchange_walk_fast (k_chain_iter_norm) — part of libsmmhip (included by smm_chain.hpp inside smmhip.hip's anonymous namespace;
// gfx950 device code).  The stand-alone kernels k_exch_resolve_lvl and k_exch_resolve_lvl_soa (smm_exchange.hpp) run the same loop.
#pragma once
// ------------------------------------------------------------------------------------------
// exchangeMoves! inside the chain kernel (single shard, N_global <= XLVL_MAX).
// The level walk of k_exch_resolve_lvl costs ~7 us as a kernel of one workgroup plus a ~2.5 us
// kernel boundary.  Executed redundantly by EVERY tile in the prologue of the next k_chain_iter it costs
// the walk's ~4 us inside a kernel that is latency-structured anyway, and the boundary and the xres round
// trip disappear.  Same plan (k_exch_plan: pairs grouped by dependency level), same arithmetic, same result;
// the working set is 16 bytes per chain + 4 bytes per pair of LDS, the pair list overlaid by the tile's own
// blocks once the walk is over: 80 KB at N = 4096, so two tiles still share a CU.  Thresholds: one scalar when min_improve is uniform, else read from the plan (L2).
// ------------------------------------------------------------------------------------------
constexpr int XLVL_MAX = 4096;
struct __attribute__((aligned(16))) XSlot {  // one chain during the walk: 16 bytes, moved with one ds_read/write_b128
    double val;
    uint32_t src, partner;
};
// LDS of a tile with the inline walk: [XSlot slot[Ng]] [pairs[K] u32, later overlaid by the tile's own blocks]
__host__ __device__ inline size_t walk_slot_bytes(int Ng) { return (size_t)Ng * sizeof(XSlot); }

// ------------------------------------------------------------------------------------------
// The level loop, once.  A level's pairs touch pairwise disjoint chains: one parallel step and a barrier.  This thread's first
// pair of the next level is fetched while this level runs.  STORE says where a slot lives (pair(i, j, dk, m): the test and the
// swap of one pair); WalkThr where a pair's threshold comes from; DBG what a kernel with debug switches adds.
// TAIL: the level sizes fall off geometrically, and the narrow tail (levels ltail .. nlev - 1, each at most 64 pairs) is walked
// by wave 0 alone — LDS operations of one wave complete in order, so its levels need no workgroup barrier and cost one LDS round
// trip each (a barrier level of a tile costs ~0.45 us next to a second walking tile).
// ------------------------------------------------------------------------------------------
struct SlotsAoS {   // XSlot slot[Ng]
    XSlot* slot;
    __device__ __forceinline__ void pair(const uint32_t i, const uint32_t j, const int dk, const double m) const {
        const XSlot si = slot[i], sj = slot[j];
        if (dist_fun_eval(dk, si.val, sj.val) > m) {   // dist_fun (default -), AlgoBGP.jl:688
            XSlot ni, nj;                           // swap_ev_ij!, :739-744; set_exchanged!, :747-748
            ni.val = sj.val; ni.src = sj.src; ni.partner = j + 1;
            nj.val = si.val; nj.src = si.src; nj.partner = i + 1;
            slot[i] = ni;
            slot[j] = nj;
        }
    }
};
struct SlotsSoA {   // double val[Ng]; uint32_t sp[Ng]: src | partner << 16
    double* val;
    uint32_t* sp;
    __device__ __forceinline__ void pair(const uint32_t i, const uint32_t j, const int dk, const double m) const {
        const double vi = val[i], vj = val[j];
        const uint32_t si = sp[i], sj = sp[j];
        if (dist_fun_eval(dk, vi, vj) > m) {    // dist_fun (default -), AlgoBGP.jl:688
            val[i] = vj; val[j] = vi;               // swap_ev_ij!, :739-744; set_exchanged!, :747-748
            sp[i] = (sj & 0xffffu) | ((j + 1) << 16);
            sp[j] = (si & 0xffffu) | ((i + 1) << 16);
        }
    }
};
struct WalkThr {   // the threshold of the pair at position pos: the one scalar, or mi[pos] (the plan's in global memory, or a copy in LDS)
    const double* mi;
    bool uniform;
    double value;
    __device__ __forceinline__ double at(const uint32_t pos) const { return uniform ? value : mi[pos]; }
    __device__ __forceinline__ double first(const uint32_t pos, const bool has) const { return uniform ? value : (has ? mi[pos] : 0.0); }
};
struct WalkNoDebug {
    __device__ __forceinline__ bool skip_pairs() const { return false; }
    __device__ __forceinline__ bool skip_barrier() const { return false; }
    __device__ __forceinline__ void level_done() {}
};
// what the staging leaves: the pair list in LDS, the plan's level ends (lane l of ev: end of level l; g_off beyond 64 levels)
struct SlotWalkPlan {
    const uint32_t* pairs;
    const uint32_t* g_off;
    const double* g_mi;
    uint32_t ev;
    int nlev, ltail;
    __device__ __forceinline__ uint32_t level_end(const int l) const {
        const int lc = min(l, nlev - 1);
        return lc < 64 ? (uint32_t)__builtin_amdgcn_readlane((int)ev, lc) : g_off[lc];
    }
};
template <int NT, bool TAIL, class STORE, class DBG = WalkNoDebug>
__device__ __forceinline__ void slot_walk_levels(const int dist_fun, const SlotWalkPlan& W, const STORE& store, const WalkThr& thr, const int tid, DBG&& dbg = DBG()) {
    const uint32_t* pairs = W.pairs;
    const int nlev = W.nlev, ltail = TAIL ? W.ltail : W.nlev;
    uint32_t b = 0;
    uint32_t e = nlev > 0 ? W.level_end(0) : 0u;
    uint32_t e2 = nlev > 0 ? W.level_end(1) : 0u;
    uint32_t pw = (b + tid < e) ? pairs[b + tid] : 0u;
    double m = thr.first(b + tid, b + tid < e);
    // (the loops twice: the default dist_fun `-` pays nothing for the menu)
    auto levels = [&](auto gen) {
        const int dk = decltype(gen)::value ? dist_fun : 0;
#pragma clang loop unroll(disable)
        for (int l = 0; l < ltail; ++l) {
            const uint32_t e3 = W.level_end(l + 2);
            const uint32_t pw2 = (e + tid < e2) ? pairs[e + tid] : 0u;
            const double m2 = thr.first(e + tid, e + tid < e2);
            for (uint32_t pos = b + tid; pos < e && !dbg.skip_pairs(); pos += NT) {
                if (pos != b + tid) { pw = pairs[pos]; m = thr.at(pos); }
                store.pair(pw & 0xffffu, pw >> 16, dk, m);
            }
            b = e; e = e2; e2 = e3; pw = pw2; m = m2;
            if (!dbg.skip_barrier()) __syncthreads();
            dbg.level_done();
        }
        if constexpr (TAIL) {
            if (ltail < nlev) {
                if (tid < 64) {   // (pw, m) already hold this lane's pair of level ltail, e its end, e2 the next end
                    constexpr uint32_t NOPAIR = 0xffffffffu;   // i == j == 0xffff never occurs (chain ids < XLVL_MAX)
                    uint32_t cpw = (b + tid < e) ? pw : NOPAIR;
#pragma clang loop unroll(disable)
                    for (int l = ltail; l < nlev; ++l) {
                        const uint32_t e3 = W.level_end(l + 2);
                        const uint32_t npw = (e + tid < e2) ? pairs[e + tid] : NOPAIR;
                        const double m2 = thr.first(e + tid, e + tid < e2);
                        if (cpw != NOPAIR) store.pair(cpw & 0xffffu, cpw >> 16, dk, m);
                        __builtin_amdgcn_wave_barrier();
                        cpw = npw; m = m2; e = e2; e2 = e3;
                    }
                }
                __syncthreads();
            }
        }
    };
    if (dist_fun != 0) levels(std::true_type{}); else levels(std::false_type{});
}

// ------------------------------------------------------------------------------------------
// The staging of the inline forms, once: ONE round trip of global loads (the chains' values, the pair words, the level ends), then
// slots {value, src, partner = 0} and pair list into LDS, the first level of the narrow tail, the barrier, the "staged" stamp.
// while_loading: work of the caller that needs no memory (it runs between the request of the walk's inputs and their arrival)
// ------------------------------------------------------------------------------------------
struct WalkNoWork { __device__ inline void operator()() const {} };
template <int NT, class F = WalkNoWork>
__device__ __forceinline__ SlotWalkPlan slot_walk_stage(const KParams& P, const int tx, unsigned char* lds, const int tid, const int ts_tile,
                                                        const bool narrow_tail, F while_loading = F()) {
    const int Ng = P.Ng, K = P.plan_K;
    const int w = tx - P.plan_t0;
    uint4* slot = (uint4*)lds;                                  // [Ng] {value lo, value hi, src, partner}
    uint32_t* pairs = (uint32_t*)(lds + walk_slot_bytes(Ng));   // [K]
    const uint32_t* __restrict__ g_off = P.lv_off + (size_t)w * (K + 2);
    const uint32_t* __restrict__ g_pairs = P.lv_pairs + (size_t)w * K;
    constexpr int PT = XLVL_MAX / NT;
    const int lane = tid & 63;
    double v_[PT];
    uint32_t pq_[PT];
#pragma unroll
    for (int r = 0; r < PT; ++r) {
        const int g = tid + r * NT;
        v_[r] = g < Ng ? P.vals[g] : 0.0;
    }
#pragma unroll
    for (int r = 0; r < PT; ++r) {
        const int q = tid + r * NT;
        pq_[r] = q < K ? g_pairs[q] : 0u;
    }
    const uint32_t ev = g_off[min(lane, K)];   // lane l: end of level l
    const int nlev = (int)g_off[K + 1];
    while_loading();
#pragma unroll
    for (int r = 0; r < PT; ++r) {
        const int g = tid + r * NT;
        const unsigned long long uv = __builtin_bit_cast(unsigned long long, v_[r]);
        if (g < Ng) slot[g] = make_uint4((uint32_t)uv, (uint32_t)(uv >> 32), (uint32_t)g, 0u);
    }
#pragma unroll
    for (int r = 0; r < PT; ++r) {
        const int q = tid + r * NT;
        if (q < K) pairs[q] = pq_[r];
    }
    for (int q = tid + PT * NT; q < K; q += NT) pairs[q] = g_pairs[q];   // injected pair lists longer than XLVL_MAX
    int ltail = nlev;
    if (nlev > 0 && nlev <= 64 && narrow_tail) {
        const uint32_t lo = (uint32_t)__shfl_up((int)ev, 1, 64);
        const unsigned long long wide = __ballot(lane < nlev && ev - (lane > 0 ? lo : 0u) > 64u);
        ltail = wide ? 64 - __builtin_clzll(wide) : 0;
    }
    __syncthreads();
    if (P.ts && tid == 0) P.ts[(size_t)ts_tile * 8 + 5] = wall_clock64();   // staged
    return {pairs, g_off, P.lv_mi + (size_t)w * K, ev, nlev, ltail};
}

// k_chain_iter's form: any thresholds, the dist_fun menu
template <int NT>
__device__ inline void exchange_walk_tile(const KParams& P, const int tx, unsigned char* lds, const int tid, const int ts_tile = 0) {
    const SlotWalkPlan W = slot_walk_stage<NT>(P, tx, lds, tid, ts_tile, !(P.dbg & 128));
    slot_walk_levels<NT, true>(P.dist_fun, W, SlotsAoS{(XSlot*)lds}, WalkThr{W.g_mi, P.mi_uniform != 0, P.mi_value}, tid);
}

// The same walk with the level loop written for latency: a level is ONE LDS round trip (both 16-byte slots of a pair with a
// ds_read_b128 each), the compare, the two 16-byte writes of a swap and the barrier; the next level's pair word is fetched
// ahead; nothing else is in the loop (thresholds: a scalar when min_improve is uniform — the loop is instantiated twice).
// The level walk is latency, not bandwidth: a level with a handful of pairs costs almost what a level with a thousand does
// (measured per level of the first form: 1784 cycles for 1000 pairs, ~850 for 50), so what counts is the dependent chain
// per level.  It exists for its instruction count and is not the generic loop above.
// FINAL_BARRIER = false: only the walking wave 0 reads the result (its own LDS operations complete in order).
constexpr uint32_t XNOPAIR = 0xffffffffu;   // i == j == 0xffff never occurs (chain ids < XLVL_MAX)
// (inline asm: left to itself the compiler reads only the 8 value bytes first and fetches src with a second, dependent LDS
// read inside the swap branch — two round trips per level instead of one.  The asm's own LDS operations are invisible to the
// compiler's counters, hence the explicit waits: after the reads, and walk_wait_lds() before every barrier.)
__device__ inline void walk_pair(const uint32_t slot_base, const uint32_t pw, const double m) {
    const uint32_t i = pw & 0xffffu, j = pw >> 16;
    const uint32_t ai = slot_base + i * 16u, aj = slot_base + j * 16u;
    u32x4_t si, sj;
    asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %3\n\ts_waitcnt lgkmcnt(0)" : "=&v"(si), "=&v"(sj) : "v"(ai), "v"(aj) : "memory");
    const double vi = __builtin_bit_cast(double, ((unsigned long long)si.y << 32) | si.x);
    const double vj = __builtin_bit_cast(double, ((unsigned long long)sj.y << 32) | sj.x);
    if (vi - vj > m) {                                   // dist_fun = -, AlgoBGP.jl:688
        u32x4_t ni = sj, nj = si;                        // swap_ev_ij!, :739-744; set_exchanged!, :747-748
        ni.w = j + 1; nj.w = i + 1;
        asm volatile("ds_write_b128 %0, %2\n\tds_write_b128 %1, %3" :: "v"(ai), "v"(aj), "v"(ni), "v"(nj) : "memory");
    }
}
__device__ inline void walk_wait_lds() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
template <int NT, bool MI_U, bool FINAL_BARRIER>
__device__ inline void walk_levels(const KParams& P, const uint32_t slot, const SlotWalkPlan& W, const int tid) {
    const uint32_t* pairs = W.pairs;
    const double* __restrict__ g_mi = W.g_mi;
    const int nlev = W.nlev, ltail = W.ltail;
    const double mi_v = P.mi_value;
    // (level ends and this wave's first position are scalars: a wave without a pair in a level runs no vector instruction for it)
    uint32_t b = 0;
    uint32_t e = nlev > 0 ? W.level_end(0) : 0u;
    uint32_t e2 = nlev > 0 ? W.level_end(1) : 0u;
    uint32_t pw = (b + tid < e) ? pairs[b + tid] : XNOPAIR;
    double m = MI_U ? mi_v : ((b + tid < e) ? g_mi[b + tid] : 0.0);
#pragma clang loop unroll(disable)
    for (int l = 0; l < ltail; ++l) {
        const uint32_t e3 = W.level_end(l + 2);
        uint32_t pw2 = XNOPAIR;
        double m2 = mi_v;
        {   // this thread's first pair of the next level
            pw2 = (e + tid < e2) ? pairs[e + tid] : XNOPAIR;
            if constexpr (!MI_U) m2 = (e + tid < e2) ? g_mi[e + tid] : 0.0;
        }
        {
            if (pw != XNOPAIR) walk_pair(slot, pw, m);
            for (uint32_t pos = b + tid + NT; pos < e; pos += NT) walk_pair(slot, pairs[pos], MI_U ? mi_v : g_mi[pos]);   // levels wider than the workgroup
        }
        b = e; e = e2; e2 = e3; pw = pw2; m = m2;
        walk_wait_lds();
        __syncthreads();
        if (P.ts_levels && tid == 0 && blockIdx.x == 0 && l < 30) P.ts[(size_t)8 * 60000 + 16 + l] = clock64();
    }
    if (P.ts && tid == 0 && blockIdx.x == 0) { P.ts[(size_t)8 * 60000 + 14] = (unsigned long long)ltail; P.ts[(size_t)8 * 60000 + 7] = (unsigned long long)nlev; }
    if (ltail < nlev) {
        if (tid < 64) {   // the narrow tail: wave 0 alone, no barriers (pw, m hold this lane's pair of level ltail, e its end, e2 the next end)
#pragma clang loop unroll(disable)
            for (int l = ltail; l < nlev; ++l) {
                const uint32_t e3 = W.level_end(l + 2);
                const uint32_t pw2 = (e + tid < e2) ? pairs[e + tid] : XNOPAIR;
                double m2 = mi_v;
                if constexpr (!MI_U) m2 = (e + tid < e2) ? g_mi[e + tid] : 0.0;
                if (pw != XNOPAIR) walk_pair(slot, pw, m);
                __builtin_amdgcn_wave_barrier();
                pw = pw2; m = m2; e = e2; e2 = e3;
                if (P.ts_levels && tid == 0 && blockIdx.x == 0 && l < 30) { walk_wait_lds(); P.ts[(size_t)8 * 60000 + 16 + l] = clock64(); }
            }
            walk_wait_lds();
        }
        if constexpr (FINAL_BARRIER) __syncthreads();
    }
}

template <int NT, bool FINAL_BARRIER, class F = WalkNoWork>
__device__ inline void exchange_walk_fast(const KParams& P, const int tx, unsigned char* lds, const int tid, const int ts_tile,
                                          F while_loading = F()) {
    const SlotWalkPlan W = slot_walk_stage<NT>(P, tx, lds, tid, ts_tile, true, while_loading);
    const uint32_t slot_base = (uint32_t)(size_t)lds;   // LDS byte address of the chain slots
    // (dist_fun = - only: k_chain_iter_norm does not walk inline for the other entries of the menu — the host sees to it)
    if (P.mi_uniform) walk_levels<NT, true, FINAL_BARRIER>(P, slot_base, W, tid);
    else walk_levels<NT, false, FINAL_BARRIER>(P, slot_base, W, tid);
}
