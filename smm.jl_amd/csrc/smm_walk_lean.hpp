// the lean exchange walk (exchangeMoves!, AlgoBGP.jl:647-716, for one min_improve >= 0 shared by all chains): shared by
// k_chain_iter_norm (in its prologue, N_global <= 4096) and k_exch_resolve_lean (stand-alone, N_global <= 8192) — part of
// libsmmhip (included by smmhip.hip inside its anonymous namespace; gfx950 device code).
#pragma once
// ------------------------------------------------------------------------------------------
// The level walk written for the number of INSTRUCTIONS per level.
// Measured (SMMHIP_TS=2, s_memtime per level, k_chain_iter_norm at 4096 chains): a level costs what one wave needs from
// barrier to barrier, and that is not the LDS round trip (71 cycles for a dependent ds_read_b32 in that kernel) but the wave's
// own instruction stream — ~8 cycles per instruction and ~25 per taken branch for a lone wave: 556 cycles for the ~65
// instructions of a level in the straightforward loop (fetch the pair word, test for "no pair", take it apart, address
// arithmetic, test for undecided keys, carry the partner), whatever the slot size.  So the plan and the slot format take the
// work out of the loop:
//   * the plan (k_exch_plan) pads every level to whole waves with dummy pairs that never swap: no lane asks whether it has a
//     pair; a wave without pairs skips the level on a scalar compare;
//   * a pair word holds the LDS byte offsets of its two slots (halved when 16 bits would not reach the last slot);
//   * a slot is 8 bytes: {32-bit order key of the value (order_key32), src | stamp << 16}.  `value_i - value_j > 0` is ONE
//     unsigned compare of the keys; equal keys (same high word of the doubles: rare) read the exact values from memory;
//   * set_exchanged! (:747-748) costs one add per trip: a swap stamps 1 + the position of its pair word into both slots, and
//     whoever needs the partner afterwards reads that pair word (lean_partner);
//   * the lane's next pair word is requested together with the slots: one LDS round trip per level.
// LDS: slots uint2[Ng4 + 4] (Ng4 = N_global rounded up to 4; the two slots behind the chains' are the dummy pair's) | pair
// words u32[plan_Kp].  The slots must start at LDS address 0 (the callers check).
// min_improve > 0 (the reference's default is 0.5, AlgoBGP.jl:522) — the WIDE form: a key cannot decide `v_i - v_j > m`, so a
// slot is 16 bytes {value, src | stamp << 16, -} and the test is the subtraction and the compare themselves (NaN values and a
// NaN threshold need nothing special: the compare is false).  The dummy pair is (d, d) with d one slot behind the chains',
// value 0: `0 - 0 > m` is false for m >= 0 or NaN (a chain's own slot would not do: another wave's swap could change it between
// the two reads).  LDS: slots uint4[Ng4 + 1] | pair words u32[plan_Kp]; up to ~7400 chains fit the 160 KB.
// ------------------------------------------------------------------------------------------
__host__ __device__ inline int lean_walk_Kp(int K) { return (K + 64 * LV_MAXLEV + 3) & ~3; }
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
// ------------------------------------------------------------------------------------------
// The three slot layouts, each number once.  LDS from address 0: slots[Ng4 + PAD] | pair words u32[plan_Kp].
//   LEAN_KEYS    8-byte slots {order key, src | stamp << 16}; the dummy pair is the two slots behind the chains', keys 1 < 2;
//                a spare slot behind those (votes of the waves: a NaN value among the chains'); 4 slots of padding in all
//   LEAN_WIDE    16-byte slots {value, src | stamp << 16, -}; the dummy pair is (d, d), d the one zero slot behind the chains'
//   LEAN_TILE16  k_chain_iter's inline walk: 16-byte slots whatever the threshold, TWO zero slots behind the chains' — the plan
//                may be the key form's, whose dummy pair names two slots and whose offsets are read doubled
// ------------------------------------------------------------------------------------------
enum { LEAN_KEYS = 0, LEAN_WIDE = 1, LEAN_TILE16 = 2 };
__host__ __device__ constexpr uint32_t lean_Ng4(int Ng) { return (uint32_t)((Ng + 3) & ~3); }
template <int LAY>
struct LeanLayout {
    static constexpr bool WIDE = LAY != LEAN_KEYS;                     // lean_walk_levels' slot form
    static constexpr int SL = WIDE ? 4 : 3;                            // log2 of the slot size
    static constexpr uint32_t SLOT = 1u << SL;
    static constexpr uint32_t PAD = LAY == LEAN_KEYS ? 4u : LAY == LEAN_WIDE ? 1u : 2u;   // slots between the chains' and the pair words
    static constexpr uint32_t DUMMIES = LAY == LEAN_WIDE ? 1u : 2u;
    __host__ __device__ static constexpr uint32_t pbase(uint32_t Ng4) { return SLOT * (Ng4 + PAD); }   // LDS offset of the pair words
    __host__ __device__ static constexpr uint32_t spare(uint32_t Ng4) {   // 16 bytes nobody walks
        static_assert(LAY == LEAN_KEYS, "only the key layout has a spare slot: behind the dummies of the other two the pair words begin");
        return SLOT * (Ng4 + DUMMIES);
    }
    __host__ __device__ static constexpr size_t slot_bytes(int Ng) { return (size_t)pbase(lean_Ng4(Ng)); }
    __host__ __device__ static constexpr size_t bytes(int Ng, int K) { return slot_bytes(Ng) + (size_t)lean_walk_Kp(K) * 4; }
    // KParams::lean_unit of a plan made for this layout: what a pair word counts its two 16-bit offsets in — bytes where they reach
    // the last dummy slot, else halves (keys: up to 8190 chains in bytes; wide: 4092, and 8188 halved)
    __host__ __device__ static constexpr int unit4(uint32_t Ng4) { return SLOT * (Ng4 + DUMMIES) <= 65536u ? (int)SLOT : (int)SLOT / 2; }
    __host__ __device__ static constexpr int unit(int Ng) { return unit4(lean_Ng4(Ng)); }
    // the pair word of the dummy pair in a plan of that unit
    __host__ __device__ static constexpr uint32_t dummy_word(uint32_t unit, uint32_t Ng4) {
        return DUMMIES == 1u ? (unit * Ng4) * 0x10001u : (unit * Ng4) | ((unit * (Ng4 + 1u)) << 16);
    }
    // the dummy slots' contents (no swap ever: keys 1 < 2; 0 - 0 > min_improve is false for min_improve >= 0 or NaN)
    __device__ static inline void put_dummies(unsigned char* lds, const uint32_t Ng4) {
        if constexpr (LAY == LEAN_KEYS) ((uint4*)lds)[Ng4 / 2] = make_uint4(1u, 0u, 2u, 0u);
        else {
            ((uint4*)lds)[Ng4] = make_uint4(0u, 0u, 0u, 0u);
            if constexpr (DUMMIES == 2u) ((uint4*)lds)[Ng4 + 1u] = make_uint4(0u, 0u, 0u, 0u);
        }
    }
};

// LDS byte offsets of the two slots of a pair word (US = 1: the word holds them halved, KParams::lean_unit == 4)
template <int US>
__device__ inline void lean_decode(const uint32_t pw, uint32_t& ai, uint32_t& aj) {
    if constexpr (US == 0) { ai = pw & 0xffffu; aj = pw >> 16; }
    else { ai = (pw & 0xffffu) << US; aj = (pw >> 16) << US; }
}
// 1 + the chain's last exchange partner (0: none) from its slot's second word after the walk
// (SL: log2 of the slot size, 3 or 4 for the wide form)
template <int US, int SL = 3>
__device__ inline uint32_t lean_partner(const unsigned char* lds, const uint32_t pbase, const uint32_t meta, const uint32_t g) {
    const uint32_t stamp = meta >> 16;
    if (stamp == 0u) return 0u;
    const uint32_t pw = *(const uint32_t*)(lds + pbase + 4u * (stamp - 1u));
    const uint32_t i = (pw & 0xffffu) >> (SL - US), j = (pw >> 16) >> (SL - US);
    return (i == g ? j : i) + 1u;
}

// (GUARD: where the exact value of chain s comes from on a key tie — vsrc[s * vstride] by default; the p2p form reads a
// self-validating copy out of its window, GUARD::value)
struct WalkNoGuard {};
template <class GUARD>
__device__ inline double walk_value(const GUARD& g, const double* __restrict__ vsrc, const int vstride, const uint32_t s) {
    if constexpr (std::is_same<GUARD, WalkNoGuard>::value) return vsrc[(size_t)s * vstride];
    else return g.value(s);
}
// PCT (the persistent forms' wide walk, round 6): the threshold is the COLDER chain's own (min_improve[i], AlgoBGP.jl:522, :688) — a double per slot
// POSITION at LDS offset thr_base + 8 * position, read in the same LDS round trip as the slots (positions do not travel with the records a swap exchanges)
// one pair, on its own (further words of a level wider than the workgroup)
template <int US, bool WIDE = false, class GUARD = WalkNoGuard, bool PCT = false>
__device__ inline void lean_pair(const double* __restrict__ vsrc, const int vstride, const uint32_t pw, const uint32_t stamp, const double thr = 0.0,
                                 const GUARD& guard = GUARD(), const uint32_t thr_base = 0u) {
    uint32_t ai, aj;
    lean_decode<US>(pw, ai, aj);
    if constexpr (WIDE) {
        u32x4_t si, sj;
        double thr_l = thr;
        if constexpr (PCT) asm volatile("ds_read_b128 %0, %3\n\tds_read_b128 %1, %4\n\tds_read_b64 %2, %5\n\ts_waitcnt lgkmcnt(0)" : "=&v"(si), "=&v"(sj), "=&v"(thr_l) : "v"(ai), "v"(aj), "v"(thr_base + (ai >> 1)) : "memory");
        else asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %3\n\ts_waitcnt lgkmcnt(0)" : "=&v"(si), "=&v"(sj) : "v"(ai), "v"(aj) : "memory");
        const double vi = __hiloint2double((int)si.y, (int)si.x), vj = __hiloint2double((int)sj.y, (int)sj.x);
        if (vi - vj > thr_l) {   // dist_fun = -, AlgoBGP.jl:688
            const u32x4_t ni = {sj.x, sj.y, (sj.z & 0xffffu) | stamp, 0u}, nj = {si.x, si.y, (si.z & 0xffffu) | stamp, 0u};
            asm volatile("ds_write_b128 %0, %2\n\tds_write_b128 %1, %3" :: "v"(ai), "v"(aj), "v"(ni), "v"(nj) : "memory");
        }
        return;
    }
    u32x2_t si, sj;
    asm volatile("ds_read_b64 %0, %2\n\tds_read_b64 %1, %3\n\ts_waitcnt lgkmcnt(0)" : "=&v"(si), "=&v"(sj) : "v"(ai), "v"(aj) : "memory");
    bool swap = si.x > sj.x;
    if (si.x == sj.x) swap = walk_value(guard, vsrc, vstride, si.y & 0xffffu) - walk_value(guard, vsrc, vstride, sj.y & 0xffffu) > 0.0;
    if (swap) {
        const u32x2_t ni = {sj.x, (sj.y & 0xffffu) | stamp}, nj = {si.x, (si.y & 0xffffu) | stamp};
        asm volatile("ds_write_b64 %0, %2\n\tds_write_b64 %1, %3" :: "v"(ai), "v"(aj), "v"(ni), "v"(nj) : "memory");
    }
}
// the levels: `ov` holds in lane l the first word of level l (lane nlev: the padded length); pair words at LDS offset pbase;
// exact values of chain s at vsrc[s * vstride].  Every level ends with a workgroup barrier, except the narrow tail (every
// remaining level at most one wave wide), which wave 0 walks alone: only wave 0 may read the result without a barrier.
// the first level of the narrow tail (call it before the barrier that ends the staging: it needs no LDS data)
__device__ inline int lean_walk_tail(const uint32_t ov, const int nlev, const int lane) {
    const uint32_t nx = (uint32_t)__shfl_down((int)ov, 1, 64);
    const unsigned long long wide = __ballot(lane < nlev && nx - ov > 64u);
    return wide ? 64 - __builtin_clzll(wide) : 0;
}
template <int NT, int US, bool WIDE = false, class GUARD = WalkNoGuard, bool PCT = false>
__device__ inline void lean_walk_levels(const double* __restrict__ vsrc, const int vstride, const uint32_t pbase, const uint32_t ov,
                                        const int nlev, const int tid, const int ltail, const double thr = 0.0, const GUARD& guard = GUARD(),
                                        const uint32_t thr_base = 0u) {
    const uint32_t wbase = (uint32_t)__builtin_amdgcn_readfirstlane(tid & ~63);   // this wave's first word within a trip
    const uint32_t tid4p = pbase + 4u * (uint32_t)tid;
    const uint32_t tidst = ((uint32_t)tid + 1u) << 16;                           // this lane's stamp at position 0
    uint32_t st = 0u, st1 = (uint32_t)__builtin_amdgcn_readlane((int)ov, 1);     // first words of the levels l, l+1
    uint32_t pw = 0u;
    if (nlev > 0) asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(pw) : "v"(tid4p) : "memory");   // (garbage past the level: not used)
    // (written for the common case to fall through: every taken branch costs a lone wave ~25 cycles)
    auto level = [&](const int l, const bool lone) {
        const uint32_t st2 = (uint32_t)__builtin_amdgcn_readlane((int)ov, l + 2);   // (l + 2 <= 33; past the last level: anything)
        const uint32_t width = st1 - st;
        if (__builtin_expect(wbase < width, 1)) {
            uint32_t nptr;                                // this lane's word of the next level (garbage past it: not used)
            asm volatile("v_add_u32 %0, %1, %2" : "=v"(nptr) : "s"(st1 << 2), "v"(tid4p));
            uint32_t stamp;                               // in a vector register: v_and_or_b32 takes one scalar operand, the mask
            asm volatile("v_add_u32 %0, %1, %2" : "=v"(stamp) : "s"(st << 16), "v"(tidst));
            uint32_t ai, aj;
            lean_decode<US>(pw, ai, aj);
            uint32_t pwn;
            if constexpr (WIDE) {
                u32x4_t si, sj;
                double thr_l = thr;
                if constexpr (PCT)   // (the threshold of position i rides in the same LDS round trip; a compile-time form: as a run-time branch it cost the one-threshold walk 0.2 us)
                    asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %5\n\tds_read_b32 %2, %6\n\tds_read_b64 %3, %7\n\ts_waitcnt lgkmcnt(0)"
                                 : "=&v"(si), "=&v"(sj), "=&v"(pwn), "=&v"(thr_l) : "v"(ai), "v"(aj), "v"(nptr), "v"(thr_base + (ai >> 1)) : "memory");
                else
                    asm volatile("ds_read_b128 %0, %3\n\tds_read_b128 %1, %4\n\tds_read_b32 %2, %5\n\ts_waitcnt lgkmcnt(0)"
                                 : "=&v"(si), "=&v"(sj), "=&v"(pwn) : "v"(ai), "v"(aj), "v"(nptr) : "memory");
                const double vi = __hiloint2double((int)si.y, (int)si.x), vj = __hiloint2double((int)sj.y, (int)sj.x);
                if (vi - vj > thr_l) {   // dist_fun = -, AlgoBGP.jl:688; swap_ev_ij!, :739-744; the stamp stands for set_exchanged!, :747-748
                    const u32x4_t ni = {sj.x, sj.y, (sj.z & 0xffffu) | stamp, 0u}, nj = {si.x, si.y, (si.z & 0xffffu) | stamp, 0u};
                    asm volatile("ds_write_b128 %0, %2\n\tds_write_b128 %1, %3" :: "v"(ai), "v"(aj), "v"(ni), "v"(nj) : "memory");
                }
            } else {
                u32x2_t si, sj;
                asm volatile("ds_read_b64 %0, %3\n\tds_read_b64 %1, %4\n\tds_read_b32 %2, %5\n\ts_waitcnt lgkmcnt(0)"
                             : "=&v"(si), "=&v"(sj), "=&v"(pwn) : "v"(ai), "v"(aj), "v"(nptr) : "memory");
                bool swap = si.x > sj.x;
                const bool tie = si.x == sj.x;
                if (__builtin_expect(__ballot(tie) != 0ull, 0)) {   // the keys do not decide: the exact values (dist_fun = -, AlgoBGP.jl:688)
                    if (tie) swap = walk_value(guard, vsrc, vstride, si.y & 0xffffu) - walk_value(guard, vsrc, vstride, sj.y & 0xffffu) > 0.0;
                }
                if (swap) {   // swap_ev_ij!, :739-744; the stamp stands for set_exchanged!, :747-748
                    const u32x2_t ni = {sj.x, (sj.y & 0xffffu) | stamp}, nj = {si.x, (si.y & 0xffffu) | stamp};
                    asm volatile("ds_write_b64 %0, %2\n\tds_write_b64 %1, %3" :: "v"(ai), "v"(aj), "v"(ni), "v"(nj) : "memory");
                }
            }
            pw = pwn;
            if (__builtin_expect(width > (uint32_t)NT, 0)) {   // a level wider than the workgroup: its further words, one by one
                for (uint32_t o = (uint32_t)NT; wbase + o < width; o += (uint32_t)NT) {
                    uint32_t pwx;
                    asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(pwx) : "v"(tid4p + 4u * (st + o)) : "memory");
                    lean_pair<US, WIDE, GUARD, PCT>(vsrc, vstride, pwx, ((st + o) << 16) + tidst, thr, guard, thr_base);
                }
            }
        } else if (wbase < st2 - st1) {   // idle in this level, not in the next: its word
            asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(pw) : "v"(tid4p + 4u * st1) : "memory");
        }
        st = st1; st1 = st2;
        if (!lone) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __syncthreads(); }
    };
    {   // (two levels per trip of the loop, by hand: the compiler does not unroll across the barrier)
        int l = 0;
#pragma clang loop unroll(disable)
        for (; l + 2 <= ltail; l += 2) { level(l, false); level(l + 1, false); }
        if (l < ltail) level(l, false);
    }
    if (ltail < nlev && tid < 64) {   // the narrow tail: wave 0 alone, no barriers (its own LDS operations complete in order)
        int l = ltail;
#pragma clang loop unroll(disable)
        for (; l + 2 <= nlev; l += 2) { level(l, true); level(l + 1, true); }
        if (l < nlev) level(l, true);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
}

// ------------------------------------------------------------------------------------------
// Staging and read-out of a walk of the WHOLE list, in the phases every site goes through in this order:
//   request  the plan's header word and pair words, and what the slots are made of, into registers — everything before anything is
//            looked at (a load issued behind the first wait is a round trip of its own)
//   decide   lean_plan_head: the number of levels, and whether the plan has the padded form at all; the site adds its own conditions
//   commit   the slots, the pair words behind them, the dummy slots; the first level of the narrow tail.  The barrier is the site's.
//   walk     lean_walk: lean_walk_levels for the layout and the plan's unit
//   read out lean_result: src | (1 + last partner) << 32, as k_exch_resolve_* write it
// NT lanes; NMAX: the largest population the loops serve (their trip counts are compile-time).
// Callers: exchange_walk_lean_wide, exchange_walk_lean_p2p (smm_chain_norm.hpp), both branches of k_exch_resolve_lean (smm_exchange.hpp).  Three sites
// keep their request and commit written out, on this file's layout numbers and lean_plan_head: exchange_walk_lean (smm_chain_norm.hpp),
// exchange_walk_tile_lean and exchange_walk_tile_keys (smm_chain.hpp) — on these pieces their kernels, which spill scalar registers in the
// prologue, were allocated differently (MEASUREMENTS.md).
// ------------------------------------------------------------------------------------------
template <int NT, int NMAX>
struct LeanPlanRegs {
    static constexpr int PR = (NMAX + 64 * LV_MAXLEV + 4 * NT - 1) / (4 * NT);   // rounds of 16-byte loads for the pair words
    uint32_t ov;     // lane l: first word of level l; lane 33: levels; lane 34: the plan fits
    uint4 p_[PR];
    __device__ static inline const uint4* pairs(const KParams& P, const int w) { return (const uint4*)(P.lv_pairs_p + (size_t)w * P.plan_Kp); }
    __device__ __forceinline__ void request_ov(const KParams& P, const int w, const int tid) {
        ov = (P.lv_offp + (size_t)w * LV_OFFP)[min(tid & 63, LV_OFFP - 1)];
    }
    __device__ __forceinline__ void request_pairs(const KParams& P, const int w, const int tid) {
        const uint4* __restrict__ g_pairs = pairs(P, w);
#pragma unroll
        for (int r = 0; r < PR; ++r) {
            const int q4 = tid + r * NT;
            p_[r] = 4 * q4 < P.plan_Kp ? g_pairs[q4] : make_uint4(0u, 0u, 0u, 0u);
        }
    }
    // pair words and dummy slots into LDS; returns the first level of the narrow tail
    template <int LAY>
    __device__ __forceinline__ int commit(const KParams& P, unsigned char* lds, const uint32_t Ng4, const int tid, const int nlev) const {
#pragma unroll
        for (int r = 0; r < PR; ++r) {
            const int q4 = tid + r * NT;
            if (4 * q4 < P.plan_Kp) ((uint4*)(lds + LeanLayout<LAY>::pbase(Ng4)))[q4] = p_[r];
        }
        if (tid == 0) LeanLayout<LAY>::put_dummies(lds, Ng4);
        return lean_walk_tail(ov, nlev, tid & 63);
    }
};
struct LeanPlanHead { int nlev; bool fits; };
__device__ inline LeanPlanHead lean_plan_head(const uint32_t ov) {
    return {__builtin_amdgcn_readlane((int)ov, 33), __builtin_amdgcn_readlane((int)ov, 34) != 0};
}
// slot source: the chains' values at vsrc[g * vstride], chains tid, tid + NT, ...
template <int NT, int NMAX>
struct LeanValueRegs {
    static constexpr int PT = NMAX / NT;   // chains per lane
    double v_[PT];
    __device__ __forceinline__ void request(const double* __restrict__ vsrc, const int vstride, const int Ng, const int tid) {
#pragma unroll
        for (int r = 0; r < PT; ++r) {
            const int g = tid + r * NT;
            v_[r] = g < Ng ? vsrc[(size_t)g * vstride] : 0.0;
        }
    }
    __device__ __forceinline__ bool any_nan() const {
        bool nan = false;
#pragma unroll
        for (int r = 0; r < PT; ++r) nan = nan || v_[r] != v_[r];
        return nan;
    }
    template <int LAY>
    __device__ __forceinline__ void commit(unsigned char* lds, const int Ng, const int tid) const {
#pragma unroll
        for (int r = 0; r < PT; ++r) {
            const int g = tid + r * NT;
            if (g < Ng) {
                if constexpr (LAY == LEAN_KEYS) ((uint2*)lds)[g] = make_uint2(order_key32(v_[r]), (uint32_t)g);
                else ((uint4*)lds)[g] = make_uint4((uint32_t)__double2loint(v_[r]), (uint32_t)__double2hiint(v_[r]), (uint32_t)g, 0u);
            }
        }
    }
};
// the levels, for the layout and the plan's unit (KParams::lean_unit).  BYTES: the site serves no population whose plan halves its offsets
template <int NT, int LAY, class GUARD = WalkNoGuard, bool BYTES = false>
__device__ __forceinline__ void lean_walk(const int unit, const double* __restrict__ vsrc, const int vstride, const uint32_t Ng4, const uint32_t ov,
                                          const int nlev, const int tid, const int ltail, const double thr = 0.0, const GUARD& guard = GUARD()) {
    using L = LeanLayout<LAY>;
    if (BYTES || unit == (int)L::SLOT) lean_walk_levels<NT, 0, L::WIDE, GUARD>(vsrc, vstride, L::pbase(Ng4), ov, nlev, tid, ltail, thr, guard);
    else lean_walk_levels<NT, 1, L::WIDE, GUARD>(vsrc, vstride, L::pbase(Ng4), ov, nlev, tid, ltail, thr, guard);
}
// chain g's record source and 1 + its last exchange partner (0: none) after the walk: src | partner << 32
template <int LAY>
__device__ inline unsigned long long lean_result(const unsigned char* lds, const uint32_t Ng4, const int unit, const uint32_t g) {
    using L = LeanLayout<LAY>;
    const uint32_t meta = *(const uint32_t*)(lds + L::SLOT * g + (L::WIDE ? 8u : 4u));
    const uint32_t partner = unit == (int)L::SLOT ? lean_partner<0, L::SL>(lds, L::pbase(Ng4), meta, g) : lean_partner<1, L::SL>(lds, L::pbase(Ng4), meta, g);
    return (unsigned long long)(meta & 0xffffu) | ((unsigned long long)partner << 32);
}

// ------------------------------------------------------------------------------------------
// The walk of k_chain_persist_loc and k_chain_persist_tile: a LONE wave over `nsub` sub-levels of exactly 64 padded pair words at LDS offset pbase — the same
// semantics as lean_walk_levels<64, US, WIDE, GUARD, PCT>(vsrc, vstride, pbase, 64 * lane, nsub, lane, 0, thr, guard, thr_base), without
// what a lone wave on whole sub-levels never needs: no table of level starts and no readlane of it, no width test, no loop over a
// level wider than the workgroup, no idle level, no barrier.  The word address and the stamp advance by constants per sub-level
// (256 bytes, 64 << 16): the address as the DS offset immediate of a trip unrolled by four, the stamp as one add.
// The lane's FIRST pair word comes from the caller, who requests it in the LDS round trip that tells it nsub (lean_sub64_head: the
// word's address does not depend on nsub; past the list it is garbage that is not used).
// ------------------------------------------------------------------------------------------
// the word at LDS offset hoff (the same for all lanes) and this lane's first pair word, in one LDS round trip
__device__ inline void lean_sub64_head(const uint32_t hoff, const uint32_t pbase, const int lane, uint32_t& hdr, uint32_t& pw) {
    asm volatile("ds_read_b32 %0, %2\n\tds_read_b32 %1, %3\n\ts_waitcnt lgkmcnt(0)" : "=&v"(hdr), "=&v"(pw) : "v"(hoff), "v"(pbase + 4u * (uint32_t)lane) : "memory");
}
#define LEAN_SUB64_OFF(o) " offset:" #o "\n\t"
// one sub-level: `pw` is the lane's pair word of it and becomes the next sub-level's, read at ptr + OFF together with the slots
template <int US, bool WIDE, class GUARD, bool PCT, int OFF>
__device__ __forceinline__ void lean_sub64_level(const uint32_t ptr, const uint32_t stamp, uint32_t& pw, const double thr, const GUARD& guard, const uint32_t thr_base) {
    static_assert(OFF == 256 || OFF == 512 || OFF == 768 || OFF == 1024, "the word of the next sub-level within a trip of four");
    uint32_t ai, aj;
    lean_decode<US>(pw, ai, aj);
    uint32_t pwn;
    if constexpr (WIDE) {
        u32x4_t si, sj;
        double thr_l = thr;
#define LEAN_SUB64_WIDE(o) \
        if constexpr (PCT) /* (the threshold of position i rides in the same LDS round trip) */ \
            asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %5\n\tds_read_b32 %2, %6" LEAN_SUB64_OFF(o) "ds_read_b64 %3, %7\n\ts_waitcnt lgkmcnt(0)" \
                         : "=&v"(si), "=&v"(sj), "=&v"(pwn), "=&v"(thr_l) : "v"(ai), "v"(aj), "v"(ptr), "v"(thr_base + (ai >> 1)) : "memory"); \
        else \
            asm volatile("ds_read_b128 %0, %3\n\tds_read_b128 %1, %4\n\tds_read_b32 %2, %5" LEAN_SUB64_OFF(o) "s_waitcnt lgkmcnt(0)" \
                         : "=&v"(si), "=&v"(sj), "=&v"(pwn) : "v"(ai), "v"(aj), "v"(ptr) : "memory")
        if constexpr (OFF == 256) { LEAN_SUB64_WIDE(256); } else if constexpr (OFF == 512) { LEAN_SUB64_WIDE(512); }
        else if constexpr (OFF == 768) { LEAN_SUB64_WIDE(768); } else { LEAN_SUB64_WIDE(1024); }
#undef LEAN_SUB64_WIDE
        const double vi = __hiloint2double((int)si.y, (int)si.x), vj = __hiloint2double((int)sj.y, (int)sj.x);
        if (vi - vj > thr_l) {   // dist_fun = -, AlgoBGP.jl:688; swap_ev_ij!, :739-744; the stamp stands for set_exchanged!, :747-748
            const u32x4_t ni = {sj.x, sj.y, (sj.z & 0xffffu) | stamp, 0u}, nj = {si.x, si.y, (si.z & 0xffffu) | stamp, 0u};
            asm volatile("ds_write_b128 %0, %2\n\tds_write_b128 %1, %3" :: "v"(ai), "v"(aj), "v"(ni), "v"(nj) : "memory");
        }
    } else {
        u32x2_t si, sj;
#define LEAN_SUB64_KEY(o) \
        asm volatile("ds_read_b64 %0, %3\n\tds_read_b64 %1, %4\n\tds_read_b32 %2, %5" LEAN_SUB64_OFF(o) "s_waitcnt lgkmcnt(0)" \
                     : "=&v"(si), "=&v"(sj), "=&v"(pwn) : "v"(ai), "v"(aj), "v"(ptr) : "memory")
        if constexpr (OFF == 256) { LEAN_SUB64_KEY(256); } else if constexpr (OFF == 512) { LEAN_SUB64_KEY(512); }
        else if constexpr (OFF == 768) { LEAN_SUB64_KEY(768); } else { LEAN_SUB64_KEY(1024); }
#undef LEAN_SUB64_KEY
        bool swap = si.x > sj.x;
        const bool tie = si.x == sj.x;
        if (__builtin_expect(__ballot(tie) != 0ull, 0)) {   // the keys do not decide: the exact values (dist_fun = -, AlgoBGP.jl:688)
            if (tie) swap = walk_value(guard, nullptr, 1, si.y & 0xffffu) - walk_value(guard, nullptr, 1, sj.y & 0xffffu) > 0.0;
        }
        if (swap) {   // swap_ev_ij!, :739-744; the stamp stands for set_exchanged!, :747-748
            const u32x2_t ni = {sj.x, (sj.y & 0xffffu) | stamp}, nj = {si.x, (si.y & 0xffffu) | stamp};
            asm volatile("ds_write_b64 %0, %2\n\tds_write_b64 %1, %3" :: "v"(ai), "v"(aj), "v"(ni), "v"(nj) : "memory");
        }
    }
    pw = pwn;
}
#undef LEAN_SUB64_OFF
template <int US, bool WIDE = false, class GUARD = WalkNoGuard, bool PCT = false>
__device__ inline void lean_walk_sub64(const uint32_t pbase, const int nsub, const int lane, uint32_t pw, const double thr = 0.0, const GUARD& guard = GUARD(),
                                       const uint32_t thr_base = 0u) {
    static_assert(!std::is_same<GUARD, WalkNoGuard>::value || WIDE, "a key tie reads the exact values through the guard: there is no plain array here");
    constexpr uint32_t SUBST = 64u << 16;                     // the stamp's advance per sub-level: 64 words
    uint32_t ptr = pbase + 4u * (uint32_t)lane;               // this lane's word of the trip's first sub-level
    uint32_t stamp = ((uint32_t)lane + 1u) << 16;             // 1 + the position of that word
    int left = nsub;
    // (the common case falls through; a taken branch per FOUR sub-levels)
#pragma clang loop unroll(disable)
    for (; left >= 4; left -= 4) {
        lean_sub64_level<US, WIDE, GUARD, PCT, 256>(ptr, stamp, pw, thr, guard, thr_base);
        lean_sub64_level<US, WIDE, GUARD, PCT, 512>(ptr, stamp + SUBST, pw, thr, guard, thr_base);
        lean_sub64_level<US, WIDE, GUARD, PCT, 768>(ptr, stamp + 2u * SUBST, pw, thr, guard, thr_base);
        lean_sub64_level<US, WIDE, GUARD, PCT, 1024>(ptr, stamp + 3u * SUBST, pw, thr, guard, thr_base);
        ptr += 1024u; stamp += 4u * SUBST;
    }
    if (left & 2) {
        lean_sub64_level<US, WIDE, GUARD, PCT, 256>(ptr, stamp, pw, thr, guard, thr_base);
        lean_sub64_level<US, WIDE, GUARD, PCT, 512>(ptr, stamp + SUBST, pw, thr, guard, thr_base);
        ptr += 512u; stamp += 2u * SUBST;
    }
    if (left & 1) lean_sub64_level<US, WIDE, GUARD, PCT, 256>(ptr, stamp, pw, thr, guard, thr_base);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}
