// the chain kernel: tile reduction, simulation, objectives, block moves, the lean inline exchange walks (the 16-byte-slot ones: smm_walk_slots.hpp), k_chain_iter, k_flush, k_eval_batch — part of libsmmhip (included by smmhip.hip inside its anonymous namespace; gfx950 device code).
#pragma once
// ------------------------------------------------------------------------------------------
// Transposed wave reduction: every lane holds CT partial sums a[0..CT); on return lane l holds the
// 64-lane total of accumulator acc_index<CT>(l), combined by the canonical halving tree (offsets
// 32,16,8,4,2,1; IEEE addition is commutative so both partners compute the same bits).
// ------------------------------------------------------------------------------------------
// One step of the tree for two accumulators at once with gfx950's lane swaps: v_permlane32_swap exchanges the upper half of
// its first operand with the lower half of its second, v_permlane16_swap the odd rows of the first with the even rows of the
// second.  Afterwards, in the lanes whose bit OFF is clear, x = own x and y = the partner lane's x; in the other lanes
// x = the partner lane's y and y = own y: x + y is "mine + received" for the accumulator the lane keeps (3 instructions per
// pair of 64-bit accumulators instead of 4 selects, 2 LDS permutes and the add).  The offsets 8, 4, 2, 1 move by DPP inside
// a row of 16 lanes (xor_lane below): the same partner lanes, the same additions, no LDS latency between two steps of the tree.
template <int OFF>
__device__ inline double swap_add(double x, double y) {
    static_assert(OFF == 32 || OFF == 16, "lane swaps exist for offsets 32 and 16");
    const unsigned long long ux = __builtin_bit_cast(unsigned long long, x), uy = __builtin_bit_cast(unsigned long long, y);
    unsigned xl, xh, yl, yh;
    if constexpr (OFF == 32) {
        const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)ux, (unsigned)uy, false, false);
        const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)(ux >> 32), (unsigned)(uy >> 32), false, false);
        xl = lo[0]; yl = lo[1]; xh = hi[0]; yh = hi[1];
    } else {
        const auto lo = __builtin_amdgcn_permlane16_swap((unsigned)ux, (unsigned)uy, false, false);
        const auto hi = __builtin_amdgcn_permlane16_swap((unsigned)(ux >> 32), (unsigned)(uy >> 32), false, false);
        xl = lo[0]; yl = lo[1]; xh = hi[0]; yh = hi[1];
    }
    const double x2 = __builtin_bit_cast(double, ((unsigned long long)xh << 32) | xl);
    const double y2 = __builtin_bit_cast(double, ((unsigned long long)yh << 32) | yl);
    return x2 + y2;
}
// The value of lane (this lane ^ OFF) for the offsets inside a row of 16 lanes, by DPP (no LDS round trip, no ds_bpermute):
// xor 8 = row_ror:8, xor 2 / xor 1 = quad_perm [2,3,0,1] / [1,0,3,2], xor 4 = quad_perm [3,2,1,0] (xor 3) then row_half_mirror (xor 7).
template <int CTRL>
__device__ inline unsigned dpp32(unsigned v) { return (unsigned)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xf, 0xf, false); }
template <int OFF>
__device__ inline unsigned xor_lane32(unsigned v) {
    static_assert(OFF == 8 || OFF == 4 || OFF == 2 || OFF == 1, "offsets inside a row");
    if constexpr (OFF == 8) return dpp32<0x128>(v);
    else if constexpr (OFF == 4) return dpp32<0x141>(dpp32<0x1b>(v));
    else if constexpr (OFF == 2) return dpp32<0x4e>(v);
    else return dpp32<0xb1>(v);
}
template <int OFF>
__device__ inline double xor_lane(double v) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = xor_lane32<OFF>((unsigned)u), hi = xor_lane32<OFF>((unsigned)(u >> 32));
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
template <int CT, int NN, int OFF>
__device__ inline void wave_reduce_step(double (&a)[CT], int lane) {
    if constexpr (NN > 1) {
        if constexpr (OFF >= 16) {
#pragma unroll
            for (int i = 0; i < NN / 2; ++i) a[i] = swap_add<OFF>(a[i], a[i + NN / 2]);
        } else {
            const bool upper = (lane & OFF) != 0;
#pragma unroll
            for (int i = 0; i < NN / 2; ++i) {
                const double mine = upper ? a[i + NN / 2] : a[i];
                const double send = upper ? a[i] : a[i + NN / 2];
                const double recv = xor_lane<OFF>(send);
                a[i] = mine + recv;
            }
        }
        wave_reduce_step<CT, NN / 2, OFF / 2>(a, lane);
    } else if constexpr (OFF >= 16) {
        a[0] = a[0] + __shfl_xor(a[0], OFF, 64);
        wave_reduce_step<CT, 1, OFF / 2>(a, lane);
    } else if constexpr (OFF >= 1) {
        a[0] = a[0] + xor_lane<OFF>(a[0]);
        wave_reduce_step<CT, 1, OFF / 2>(a, lane);
    }
}
template <int CT>
__device__ inline double wave_reduce_transposed(double (&a)[CT], int lane) {
    wave_reduce_step<CT, CT, 32>(a, lane);
    return a[0];
}
template <int CT>
__device__ inline int acc_index(int lane) {  // the log2(CT) top lane bits
    constexpr int LG = (CT == 1) ? 0 : (CT == 2) ? 1 : (CT == 4) ? 2 : (CT == 8) ? 3 : (CT == 16) ? 4 : (CT == 32) ? 5 : 6;
    return LG == 0 ? 0 : (lane >> (6 - LG));
}
template <int CT>
__device__ inline bool acc_writer(int lane) {
    return (lane & ((64 / CT) - 1)) == 0;
}

// The simulation of objfunc_norm (ObjExamples.jl:76-79) for a tile of CT chains:
// X[k,s] = theta_c[k] + z[k,s]; lane `tid` of the 512 sums its draws tid, tid+512, ... of moment k
// in that order (numerical contract).  Rows are processed in chunks of ZU; the shocks of the next
// chunk (of this or of the next moment) are loaded from the L2-resident matrix while the current
// chunk is added up.  Chunk 0 of moment 0 is loaded by the caller before its serial prologue.
constexpr int ZU = 8;
constexpr int SMM_SCOUT_AFTER = 2;   // rounds of one try per lane segment before the remaining tries of mysample are scouted (k_chain_iter)

// The shock matrix is read through a buffer descriptor: row = scalar byte offset (SALU), lane = one constant
// 32-bit vector offset, so a chunk load is ZU buffer_load instructions and no vector address arithmetic.
typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
struct ZBuf {
    __amdgpu_buffer_rsrc_t rsrc;
    int lane_off;  // tid * 8
    __device__ inline void init_v(const double* Z, int nm, int zstride, int tid) {
        rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)Z, 0, (int)((size_t)nm * zstride * sizeof(double)), 0x00020000);
        lane_off = tid * (int)sizeof(double);
    }
    __device__ inline void init(const KParams& P, int tid) { init_v(P.Z, P.nm, P.zstride, tid); }
};
// chunk ch of moment k
__device__ inline void sim_load_chunk_v(const ZBuf& zb, const int zstride, const bool dbg8, int k, int ch, double (&z)[ZU]) {
    const int row0 = (k * zstride + (dbg8 ? 0 : ch) * (ZU * WG)) * (int)sizeof(double);  // dbg 8: timing experiment
#pragma unroll
    for (int u = 0; u < ZU; ++u)
        z[u] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(zb.rsrc, zb.lane_off, row0 + u * WG * (int)sizeof(double), 0));
}
__device__ inline void sim_load_chunk(const ZBuf& zb, const KParams& P, int k, int ch, double (&z)[ZU]) { sim_load_chunk_v(zb, P.zstride, (P.dbg & 8) != 0, k, ch, z); }

// zc: chunk 0 of moment 0 (already loaded).  s_theta [CT][np], s_part [WG/64][CT][nm] in LDS.
// Moments are reduced in groups of G = 16/CT: one transposed reduction of G*CT accumulators has the
// same number of dependent shuffle steps as one of CT, so grouping halves that latency for CT = 8.
// A moment is nch chunks; the last one may be ragged (rows masked per lane).  Two chunks per trip, the
// two register buffers trade places; the chunk after a moment's last is chunk 0 of the next moment.
// (the problem's sizes by value: the persistent tile kernel has no KParams)
template <int CT>
__device__ inline void simulate_tile_v(const int ns, const int nm, const int np, const int zstride, const bool dbg8, const ZBuf& zb, const double* s_theta, double* s_part,
                                       int tid, double (&zc)[ZU]) {
    constexpr int G = (CT >= 16) ? 1 : 16 / CT;
    const int lane = tid & 63, wave = tid >> 6;
    const int nch = (ns + ZU * WG - 1) / (ZU * WG);
    const int last_draws = ns - (nch - 1) * (ZU * WG);   // draws of the last chunk, 1 .. ZU*WG
    const bool ragged = last_draws < ZU * WG;
    for (int k0 = 0; k0 < nm; k0 += G) {
        double acc[G * CT];
#pragma unroll
        for (int i = 0; i < G * CT; ++i) acc[i] = 0.0;
#pragma unroll
        for (int kk = 0; kk < G; ++kk) {
            const int k = k0 + kk;
            if (k < nm) {
                double mu[CT];
#pragma unroll
                for (int c = 0; c < CT; ++c) mu[c] = s_theta[c * np + k];
                auto add_full = [&](const double (&z)[ZU]) {
#pragma unroll
                    for (int u = 0; u < ZU; ++u) {
#pragma unroll
                        for (int c = 0; c < CT; ++c) {
                            const double x = z[u] + mu[c];
                            acc[kk * CT + c] = acc[kk * CT + c] + x;
                        }
                    }
                };
                auto add_last = [&](const double (&z)[ZU]) {
                    if (!ragged) { add_full(z); return; }
#pragma unroll
                    for (int u = 0; u < ZU; ++u) {
                        if (tid + u * WG < last_draws) {
#pragma unroll
                            for (int c = 0; c < CT; ++c) {
                                const double x = z[u] + mu[c];
                                acc[kk * CT + c] = acc[kk * CT + c] + x;
                            }
                        }
                    }
                };
                const int knext = (k + 1 < nm) ? k + 1 : k;   // last moment: a harmless reload
                double zn[ZU];
                int ch = 0;
                for (; ch + 2 <= nch; ch += 2) {
                    sim_load_chunk_v(zb, zstride, dbg8, k, ch + 1, zn);
                    add_full(zc);
                    const bool last = (ch + 2 == nch);
                    sim_load_chunk_v(zb, zstride, dbg8, last ? knext : k, last ? 0 : ch + 2, zc);
                    if (last) add_last(zn); else add_full(zn);
                }
                if (ch < nch) {  // odd count: the last chunk is in zc; afterwards the buffers are swapped by copy
                    sim_load_chunk_v(zb, zstride, dbg8, knext, 0, zn);
                    add_last(zc);
#pragma unroll
                    for (int u = 0; u < ZU; ++u) zc[u] = zn[u];
                }
            }
        }
        const double tot = wave_reduce_transposed<G * CT>(acc, lane);
        if (acc_writer<G * CT>(lane)) {
            const int a = acc_index<G * CT>(lane);
            const int kk = a / CT, c = a - kk * CT;
            if (k0 + kk < nm) s_part[(wave * CT + c) * nm + k0 + kk] = tot;
        }
    }
}

template <int CT>
__device__ inline void simulate_tile(const KParams& P, const ZBuf& zb, const double* s_theta, double* s_part, int tid, double (&zc)[ZU]) {
    simulate_tile_v<CT>(P.ns, P.nm, P.np, P.zstride, (P.dbg & 8) != 0, zb, s_theta, s_part, tid, zc);
}

// ------------------------------------------------------------------------------------------
// Dense objective (SMM_OBJ_DENSE, BASELINE config 5): the simulation is a dense contraction, so it
// runs on the FP64 matrix cores.  A tile is 16 chains = the N dimension of v_mfma_f64_16x16x4; wave w
// of the 8 owns the hidden units d in [32w, 32w+32):
//   x tile [16 d x 16 chains]  = B[16 d x np] * theta[np x 16]        (ceil(np/4) MFMAs)
//   h = tanh(x) (smm_tanh below): the accumulator layout (row = (lane>>4) + 4r, col = lane&15) IS the B-operand layout
//   of the next product (k = 4s + (lane>>4)), so h feeds the second GEMM from registers;
//   y tile [16 k x 16 chains] += A[16 k x 16 d] * h[16 d x 16]        (4 MFMAs per output tile)
// B and A are stored in fragment order (one coalesced 8-byte load per lane per MFMA).  The wave's
// partial y goes to LDS [w][k][chain]; the 8 partials are added left to right by the chain lane.
// ------------------------------------------------------------------------------------------
typedef double d4_t __attribute__((ext_vector_type(4)));
constexpr int DENSE_D = SMM_DENSE_D;

// the hidden layer's tanh (include/smmhip.h, SMM_OBJ_DENSE): ONE exponential and ONE division — E = exp(2|x|) = 2^n (1 + p) with p = expm1(r)
// on |r| <= ln2 / 2 (Taylor to r^13: 4e-18), tanh = (E - 1) / (E + 1) with E -+ 1 = fma(2^n, p, 2^n -+ 1) (2^n -+ 1 is exact) — about 45
// instructions against ocml's ~165 (tools/dense_bench.hip: 4.4 -> 1.4 us of a tile's evaluation); at most 3 ulp from the true value.  Only
// correctly rounded operations (fma, rint, ldexp, IEEE division), so a plain C restatement of the same expression is BIT-IDENTICAL (the tests hold one).
__device__ __forceinline__ double smm_tanh(const double x) {
    const double ax = __builtin_fabs(x);
    const double z = ax + ax;
    const double zc = z > 40.0 ? 40.0 : z;   // (tanh is 1 from 19.0625 on; a NaN stays one)
    const double n = __builtin_rint(zc * 1.44269504088896338700e+00);
    double r = __builtin_fma(-n, 6.93147180369123816490e-01, zc);
    r = __builtin_fma(-n, 1.90821492927058770002e-10, r);
    double q = 1.0 / 6227020800.0;
    q = __builtin_fma(q, r, 1.0 / 479001600.0);
    q = __builtin_fma(q, r, 1.0 / 39916800.0);
    q = __builtin_fma(q, r, 1.0 / 3628800.0);
    q = __builtin_fma(q, r, 1.0 / 362880.0);
    q = __builtin_fma(q, r, 1.0 / 40320.0);
    q = __builtin_fma(q, r, 1.0 / 5040.0);
    q = __builtin_fma(q, r, 1.0 / 720.0);
    q = __builtin_fma(q, r, 1.0 / 120.0);
    q = __builtin_fma(q, r, 1.0 / 24.0);
    q = __builtin_fma(q, r, 1.0 / 6.0);
    q = __builtin_fma(q, r, 0.5);
    const double p = __builtin_fma(r * r, q, r);
    const int ni = (n == n) ? (int)n : 0;
    const double s = __builtin_ldexp(1.0, ni);
    const double em1 = __builtin_fma(s, p, s - 1.0), ep1 = __builtin_fma(s, p, s + 1.0);
    // (1 from 19.0625 on: the select sits on the NUMERATOR — ep1 / ep1 is exactly 1 — so that the division stays unconditional: selecting between
    // 1.0 and the quotient made the compiler branch around the division: four branches per lane and tile in the middle of the matrix instructions)
    const double t = (ax >= 19.0625 ? ep1 : em1) / ep1;
    return __builtin_copysign(t, x);
}

// (inlined into its kernels — out of line the operands came through generic pointers, one dependent load per MFMA —; the operand
// fragments of a product are requested TOGETHER, ahead of the MFMAs that consume them: the B fragments of both hidden-unit tiles of the
// wave before the first product, the A fragments of a tile before its tanh — an MFMA never waits for a load of its own)
// OUT OF LINE, one copy for every kernel (its ~170 live registers — operand fragments of a whole tile, accumulators, tanh — are then
// its own, not the callers'); the tile's proposals and partial sums are named by their byte offsets in the dynamic LDS (a generic pointer
// would make every access a flat one).  NPS4: the products of the first GEMM in groups of four (np <= 16 NPS4) — straight-line code:
// fragments past the last parameter are read again from the last one (any finite value) and meet a zero of the proposal's side.
template <int CT, int NPS4>
__device__ __attribute__((noinline)) void dense_tile_n(const int np_, const int nOt_, const double* dense_Bf_, const double* dense_Af_,
                                                       const uint32_t theta_off_, const uint32_t part_off_, const int tid) {
    static_assert(CT == 16, "the dense objective tiles 16 chains (MFMA N dimension)");
    extern __shared__ __attribute__((aligned(16))) unsigned char dense_lds[];
    // (the arguments of an out-of-line function arrive in vector registers: what is uniform goes back into scalar ones, and the
    // matrices are GLOBAL memory, not "somewhere")
    typedef const __attribute__((address_space(1))) double* gptr_t;
    const int np = __builtin_amdgcn_readfirstlane(np_), nOt = __builtin_amdgcn_readfirstlane(nOt_);
    const uint32_t theta_off = (uint32_t)__builtin_amdgcn_readfirstlane((int)theta_off_), part_off = (uint32_t)__builtin_amdgcn_readfirstlane((int)part_off_);
    auto uniform_ptr = [](const double* p) {
        const unsigned long long u = (unsigned long long)p;
        return (gptr_t)(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(u >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)u));
    };
    const gptr_t dense_Bf = uniform_ptr(dense_Bf_), dense_Af = uniform_ptr(dense_Af_);
    const double* s_theta = (const double*)(dense_lds + theta_off);
    double* s_part = (double*)(dense_lds + part_off);
    constexpr int PS = 4 * NPS4;
    const int lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int nPs = (np + 3) / 4, nmp = nOt * 16;
    d4_t yacc[4];
#pragma unroll
    for (int o = 0; o < 4; ++o) yacc[o] = d4_t{0.0, 0.0, 0.0, 0.0};
    double bfr[2][PS];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
        const gptr_t bf = dense_Bf + (size_t)(2 * wave + tt) * nPs * 64 + lane;
#pragma unroll
        for (int s = 0; s < PS; ++s) bfr[tt][s] = bf[(size_t)min(s, nPs - 1) * 64];
    }
    double th[PS];   // the proposal's components k = 4 s + lk of chain li (zero past the last parameter)
#pragma unroll
    for (int s = 0; s < PS; ++s) {
        const int p = 4 * s + lk;
        const double v = s_theta[li * np + min(p, np - 1)];
        th[s] = p < np ? v : 0.0;
    }
    // both first products ahead of the first tanh: the matrix pipe works on the second tile's product (and later on the first tile's second
    // product) while the wave's vector instructions evaluate the tanh; the A fragments of a tile are requested a product ahead of their use
    double afr[2][4][4];
    auto load_a = [&](const int tt) {
        const int T = 2 * wave + tt;
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const gptr_t af = dense_Af + ((size_t)(min(o, nOt - 1) * (DENSE_D / 16) + T) * 4) * 64 + lane;
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) afr[tt][o][s4] = af[s4 * 64];
        }
    };
    load_a(0);
    d4_t xacc[2];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
        xacc[tt] = d4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < PS; ++s) xacc[tt] = __builtin_amdgcn_mfma_f64_16x16x4f64(bfr[tt][s], th[s], xacc[tt], 0, 0, 0);
        if (tt == 0) load_a(1);
    }
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
        double h[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) h[r] = smm_tanh(xacc[tt][r]);
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            if (o < nOt) {
#pragma unroll
                for (int s4 = 0; s4 < 4; ++s4) yacc[o] = __builtin_amdgcn_mfma_f64_16x16x4f64(afr[tt][o][s4], h[s4], yacc[o], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        if (o < nOt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) s_part[((size_t)wave * nmp + 16 * o + lk + 4 * r) * 16 + li] = yacc[o][r];
        }
    }
}
// ------------------------------------------------------------------------------------------
// SMM_OBJ_DENSE2 (spec v2, BASELINE config 5 AS WORDED: a 256 x 256 matvec per evaluation): x = B theta, h1 = tanh x, g = A2 h1, h2 = tanh g,
// y = A h2.  The first and the last product are spec v1's; between them wave w owns the rows [32w, 32w + 32) of g — two row tiles, each ONE
// accumulator through 64 v_mfma_f64_16x16x4 (the contract's single fma chain over d = 0..255):
//   * h1 crosses the waves through LDS: [d][16 chains] = 32 KB in the region of the partial sums (free until the last product is done) —
//     the accumulator layout (row lk + 4r of tile T, chain li) lands at 256 T + 64 r + lane, and the B operand of k-step s (d = 4s + lk) is
//     read back at 64 s + lane: both conflict-free, one 8-byte LDS access per lane;
//   * A2 (512 KB, L2-resident; every tile streams all of it per evaluation: 134 MB of L2 reads per iteration at 256 tiles) lies in fragment
//     order [wave][k-step][lane][the wave's two row tiles]: ONE global_load_dwordx4 per lane feeds both MFMAs of a k-step; the loads run
//     D2_DEPTH k-steps ahead of the MFMAs that consume them (a register ring; the loop is straight-line code);
//   * two workgroup barriers: h1 complete before the first k-step; every wave done reading h1 before the partial sums overwrite it.
// 192 MFMAs per wave (32 + 128 + 32), 1536 per tile of 16 chains: 10.2 us of the matrix pipe at two waves per SIMD.
// ------------------------------------------------------------------------------------------
typedef double d2v_t __attribute__((ext_vector_type(2)));
constexpr int D2_DEPTH = 12;
template <int CT, int NPS4>
__device__ __attribute__((noinline)) void dense2_tile_n(const int np_, const int nOt_, const double* dense_Bf_, const double* dense_A2f_, const double* dense_Af_,
                                                        const uint32_t theta_off_, const uint32_t part_off_, const int tid) {
    static_assert(CT == 16, "the dense objective tiles 16 chains (MFMA N dimension)");
    extern __shared__ __attribute__((aligned(16))) unsigned char dense_lds[];
    typedef const __attribute__((address_space(1))) double* gptr_t;
    typedef const __attribute__((address_space(1))) d2v_t* g2ptr_t;
    const int np = __builtin_amdgcn_readfirstlane(np_), nOt = __builtin_amdgcn_readfirstlane(nOt_);
    const uint32_t theta_off = (uint32_t)__builtin_amdgcn_readfirstlane((int)theta_off_), part_off = (uint32_t)__builtin_amdgcn_readfirstlane((int)part_off_);
    auto uniform_ptr = [](const double* p) {
        const unsigned long long u = (unsigned long long)p;
        return (gptr_t)(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(u >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)u));
    };
    const gptr_t dense_Bf = uniform_ptr(dense_Bf_), dense_Af = uniform_ptr(dense_Af_);
    const double* s_theta = (const double*)(dense_lds + theta_off);
    double* s_part = (double*)(dense_lds + part_off);
    double* s_h1 = s_part;   // [256 hidden units][16 chains]
    constexpr int PS = 4 * NPS4;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, lk = lane >> 4;
    const int nPs = (np + 3) / 4, nmp = nOt * 16;
    const g2ptr_t a2 = (g2ptr_t)uniform_ptr(dense_A2f_) + (size_t)wave * 64 * 64 + lane;
    // (the first product's operands are asked for first: the second product's ring is not looked at before the first barrier)
    double bfr[2][PS];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
        const gptr_t bf = dense_Bf + (size_t)(2 * wave + tt) * nPs * 64 + lane;
#pragma unroll
        for (int s = 0; s < PS; ++s) bfr[tt][s] = bf[(size_t)min(s, nPs - 1) * 64];
    }
    d2v_t ring[D2_DEPTH];
#pragma unroll
    for (int s = 0; s < D2_DEPTH; ++s) ring[s] = a2[s * 64];
    double th[PS];
#pragma unroll
    for (int s = 0; s < PS; ++s) {
        const int p = 4 * s + lk;
        const double v = s_theta[li * np + min(p, np - 1)];
        th[s] = p < np ? v : 0.0;
    }
    d4_t xacc[2];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
        xacc[tt] = d4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < PS; ++s) xacc[tt] = __builtin_amdgcn_mfma_f64_16x16x4f64(bfr[tt][s], th[s], xacc[tt], 0, 0, 0);
    }
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) s_h1[256 * (2 * wave + tt) + 64 * r + lane] = smm_tanh(xacc[tt][r]);
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // h1 stands
    d4_t gacc[2] = {d4_t{0.0, 0.0, 0.0, 0.0}, d4_t{0.0, 0.0, 0.0, 0.0}};
    // the last product's operands (A's fragments of this wave's two column tiles, out of L2) are requested UNDER the second product, as its ring drains:
    // asked for where they are used, every group of four matrix instructions waited a round trip to the L2 of its own (eight per evaluation)
    double afr[2][4][4];
    auto load_afr = [&](const int tt) {
        const int T = 2 * wave + tt;
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const gptr_t af = dense_Af + ((size_t)(min(o, nOt - 1) * (DENSE_D / 16) + T) * 4) * 64 + lane;
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) afr[tt][o][s4] = af[s4 * 64];
        }
    };
#pragma unroll
    for (int s = 0; s < 64; ++s) {
        const d2v_t a = ring[s % D2_DEPTH];
        if (s + D2_DEPTH < 64) ring[s % D2_DEPTH] = a2[(s + D2_DEPTH) * 64];
        if (s == 64 - D2_DEPTH) load_afr(0);
        if (s == 64 - D2_DEPTH / 2) load_afr(1);
        const double hb = s_h1[64 * s + lane];
        gacc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, hb, gacc[0], 0, 0, 0);
        gacc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a.y, hb, gacc[1], 0, 0, 0);
    }
    d4_t yacc[4];
#pragma unroll
    for (int o = 0; o < 4; ++o) yacc[o] = d4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
        double h[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) h[r] = smm_tanh(gacc[tt][r]);
        // (an accumulator's chain in the contract's order — column tile by column tile, k-step by k-step —, the four moments' chains side by side)
        if (nOt == 4) {   // (uniform; straight-line code for the full four tiles of moments)
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
#pragma unroll
                for (int o = 0; o < 4; ++o) yacc[o] = __builtin_amdgcn_mfma_f64_16x16x4f64(afr[tt][o][s4], h[s4], yacc[o], 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int o = 0; o < 3; ++o) {
                if (o < nOt) {
#pragma unroll
                    for (int s4 = 0; s4 < 4; ++s4) yacc[o] = __builtin_amdgcn_mfma_f64_16x16x4f64(afr[tt][o][s4], h[s4], yacc[o], 0, 0, 0);
                }
            }
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        if (o < nOt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) s_part[((size_t)wave * nmp + 16 * o + lk + 4 * r) * 16 + li] = yacc[o][r];
        }
    }
}

template <int CT>
__device__ __forceinline__ void dense_tile_v(const int np, const int nOt, const double* dense_Bf, const double* dense_Af, const double* dense_A2f, const uint32_t theta_off, const uint32_t part_off, const int tid) {
    const int g = (np + 15) / 16;   // (uniform)
    if (dense_A2f) {   // (uniform: spec v2)
        if (g <= 1) dense2_tile_n<CT, 1>(np, nOt, dense_Bf, dense_A2f, dense_Af, theta_off, part_off, tid);
        else if (g == 2) dense2_tile_n<CT, 2>(np, nOt, dense_Bf, dense_A2f, dense_Af, theta_off, part_off, tid);
        else if (g == 3) dense2_tile_n<CT, 3>(np, nOt, dense_Bf, dense_A2f, dense_Af, theta_off, part_off, tid);
        else dense2_tile_n<CT, 4>(np, nOt, dense_Bf, dense_A2f, dense_Af, theta_off, part_off, tid);
        return;
    }
    if (g <= 1) dense_tile_n<CT, 1>(np, nOt, dense_Bf, dense_Af, theta_off, part_off, tid);
    else if (g == 2) dense_tile_n<CT, 2>(np, nOt, dense_Bf, dense_Af, theta_off, part_off, tid);
    else if (g == 3) dense_tile_n<CT, 3>(np, nOt, dense_Bf, dense_Af, theta_off, part_off, tid);
    else dense_tile_n<CT, 4>(np, nOt, dense_Bf, dense_Af, theta_off, part_off, tid);
}

template <int CT>
__device__ __forceinline__ void dense_tile(const KParams& P, const double* s_theta, double* s_part, int tid) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dense_lds_base[];
    dense_tile_v<CT>(P.np, P.dense_nOt, P.dense_Bf, P.dense_Af, P.dense_A2f, (uint32_t)((const unsigned char*)s_theta - dense_lds_base), (uint32_t)((const unsigned char*)s_part - dense_lds_base), tid);
}

// value / simulated moments / status for one chain from its reduced sums
// (ObjExamples.jl:79-110; banana :251-265; "exception" -> status -2, mprob.jl:183-186).
// s_mom / s_w: data moments and weights staged in LDS.
// moment k of chain ci from the reduced sums: the 8 wave totals left to right, mean, deviation over the weight, square
// (ObjExamples.jl:79-100).  Independent across k: the lanes that serve a chain share the moments.
template <int CT>
__device__ inline void moment_term(const KParams& P, const double* s_part, const double* s_mom, const double* s_w, const int ci,
                                   const int k, double& m_out, double& v_out) {
    const bool dense = P.obj == SMM_OBJ_DENSE;
    const int nmp = P.dense_nOt * 16;
    double tot = dense ? s_part[((size_t)0 * nmp + k) * 16 + ci] : s_part[(0 * CT + ci) * P.nm + k];
#pragma unroll
    for (int wv = 1; wv < WG / 64; ++wv)
        tot = tot + (dense ? s_part[((size_t)wv * nmp + k) * 16 + ci] : s_part[(wv * CT + ci) * P.nm + k]);
    const double m = dense ? tot : tot / (double)P.ns;
    m_out = m;
    v_out = moment_sq(m, s_mom[k], s_w[k]);
}

template <int CT>
__device__ inline void finish_objective(const KParams& P, const double* theta /*LDS [np]*/, const double* s_part,
                                        const double* s_mom, const double* s_w, int ci, double* simM /*[nm] out, LDS*/,
                                        double& value, int& status, int c_local = 0, const double* vk = nullptr) {
    if (P.obj == SMM_OBJ_USER) {  // evaluated by the user's kernel between the proposal and the accept launch
        for (int k = 0; k < P.nm; ++k) simM[k] = P.u_simM[(size_t)c_local * P.nm + k];
        value = P.u_value[c_local];
        status = P.u_status[c_local];
        return;
    }
    if (P.obj == SMM_OBJ_BANANA) {
        const double v = banana_value(theta, P.np);
        for (int k = 0; k < P.nm; ++k) simM[k] = s_mom[k] + 2.2;
        value = v;
        status = 1;
        return;
    }
    if (P.obj == SMM_OBJ_NORM_FAILBOX && P.objp && in_failbox(theta[0], P.objp)) {
        for (int k = 0; k < P.nm; ++k) simM[k] = NAN;
        value = -1.0;  // Eval() default, Eval.jl:84
        status = -2;
        return;
    }
    double vsum = 0.0;
    if (vk) {   // mean and squared deviation already there (moment_term by the chain's lanes): from LDS, added in order
        vsum = sum_in_order(vk, P.nm);
    } else {
        for (int k = 0; k < P.nm; ++k) {
            double v;
            moment_term<CT>(P, s_part, s_mom, s_w, ci, k, simM[k], v);
            vsum = (k == 0) ? v : vsum + v;
        }
    }
    value = vsum / (double)P.nm;
    status = 1;
}

// ------------------------------------------------------------------------------------------
// Tile shared memory and wave-cooperative block moves
// ------------------------------------------------------------------------------------------
struct TileSmem {
    double *cs, *rb, *rec, *rout, *h, *hp, *theta, *lb, *ub, *init, *mom, *w, *part;
    unsigned* arrived;
    __device__ inline void carve(double* base, int CT, int np, int nm, int RW, int HW, int RBW, bool sim) {
        cs = base;                  // [CT][CSW]
        rb = cs + CT * CSW;         // [CT][RBW]
        rec = rb + CT * RBW;        // [CT][RW]   record the chain continues from
        rout = rec + CT * RW;       // [CT][RW]   record after this iteration's accept step
        h = rout + CT * RW;         // [CT][HW]   history record of iteration t
        hp = h + CT * HW;           // [CT][HW]   rewritten history record of iteration t-1 (exchanged chains)
        theta = hp + CT * HW;       // [CT][np]
        lb = theta + CT * np;       // [np] ...
        ub = lb + np;
        init = ub + np;
        mom = init + np;            // [nm]
        w = mom + nm;
        part = w + nm;              // [WG/64][CT][nm]
        arrived = (unsigned*)(part + (size_t)(WG / 64) * CT * nm);   // simulation kind: waves whose partial sums are in LDS
        (void)sim;
    }
};
__host__ __device__ inline size_t tile_smem_doubles(int CT, int np, int nm, int RW, int HW, int RBW, int kind) {
    // (kind 3: the dense objective's spec v2 — its partial sums' region also stages the first hidden layer, [256][16])
    size_t part = kind == 1 ? (size_t)(WG / 64) * CT * nm : kind >= 2 ? (size_t)(WG / 64) * (((nm + 15) / 16) * 16) * 16 : 0;
    if (kind == 3 && part < (size_t)DENSE_D * 16) part = (size_t)DENSE_D * 16;
    return (size_t)CT * (CSW + RBW + 2 * RW + 2 * HW + np) + 3 * np + 2 * nm + part + 2;
}

// lanes (cl, r) of the control wave move chain cl's block of W doubles (W even) in 16-byte pieces
template <int CT>
__device__ inline void coop_load(double* lds_blk, const double* __restrict__ g, int W, int r) {
    constexpr int NR = 64 / CT;
    const double2* __restrict__ gs = (const double2*)g;
    double2* ld = (double2*)lds_blk;
#pragma unroll 2
    for (int i = r; i < W / 2; i += NR) ld[i] = gs[i];
}
// the same in two halves, so that the loads of several blocks are in flight together: coop_fetch requests
// the first NI pieces per lane into registers, coop_put writes them to LDS (and moves what is left of a long block)
template <int CT, int NI>
__device__ inline void coop_fetch(double2 (&v)[NI], const double* __restrict__ g, int W, int r) {
    constexpr int NR = 64 / CT;
    const double2* __restrict__ gs = (const double2*)g;
#pragma unroll
    for (int k = 0; k < NI; ++k) {
        const int i = r + k * NR;
        v[k] = i < W / 2 ? gs[i] : make_double2(0.0, 0.0);
    }
}
template <int CT, int NI>
__device__ inline void coop_put(double* lds_blk, const double2 (&v)[NI], const double* __restrict__ g, int W, int r) {
    constexpr int NR = 64 / CT;
    const double2* __restrict__ gs = (const double2*)g;
    double2* ld = (double2*)lds_blk;
#pragma unroll
    for (int k = 0; k < NI; ++k) {
        const int i = r + k * NR;
        if (i < W / 2) ld[i] = v[k];
    }
    for (int i = r + NI * NR; i < W / 2; i += NR) ld[i] = gs[i];
}
// ... with nr lanes per block
template <int NI>
__device__ inline void coop_fetch_n(double2 (&v)[NI], const double* __restrict__ g, const int W, const int r, const int nr) {
    const double2* __restrict__ gs = (const double2*)g;
#pragma unroll
    for (int k = 0; k < NI; ++k) {
        const int i = r + k * nr;
        v[k] = i < W / 2 ? gs[i] : make_double2(0.0, 0.0);
    }
}
template <int NI>
__device__ inline void coop_put_n(double* lds_blk, const double2 (&v)[NI], const double* __restrict__ g, const int W, const int r, const int nr) {
    const double2* __restrict__ gs = (const double2*)g;
    double2* ld = (double2*)lds_blk;
#pragma unroll
    for (int k = 0; k < NI; ++k) {
        const int i = r + k * nr;
        if (i < W / 2) ld[i] = v[k];
    }
    for (int i = r + NI * nr; i < W / 2; i += nr) ld[i] = gs[i];
}
template <int CT>
__device__ inline void coop_store(double* __restrict__ g, const double* lds_blk, int W, int r) {
    constexpr int NR = 64 / CT;
    double2* __restrict__ gd = (double2*)g;
    const double2* ld = (const double2*)lds_blk;
#pragma unroll 2
    for (int i = r; i < W / 2; i += NR) gd[i] = ld[i];
}

// the same with nr lanes per block
__device__ inline void coop_store_n(double* __restrict__ g, const double* lds_blk, const int W, const int r, const int nr) {
    double2* __restrict__ gd = (double2*)g;
    const double2* ld = (const double2*)lds_blk;
    for (int i = r; i < W / 2; i += nr) gd[i] = ld[i];
}

// dst[k] = src[k] for k = r, r + nr, ... < n: a copy shared by the nr lanes that serve one chain
__device__ inline void copy_strided(double* dst, const double* src, const int n, const int r, const int nr) {
    for (int k = r; k < n; k += nr) dst[k] = src[k];
}

// (the exchange walk on 16-byte slots — XLVL_MAX, XSlot, exchange_walk_tile, exchange_walk_fast: smm_walk_slots.hpp)
#include "smm_walk_slots.hpp"

// The lean walk of smm_walk_lean.hpp in k_chain_iter (one min_improve >= 0 for all chains, dist_fun = -; the plan in its padded
// form): 16-byte slots {value, src | stamp << 16} built from the chains' values — with min_improve == 0 too, whose plan (made for
// the 8-byte key slots: offsets in units of 8, a dummy pair of two slots) is read with doubled offsets and finds two zero-valued
// slots behind the chains'.  The control wave of every tile of the workgroup takes its chains' result (src | partner << 32, as
// k_exch_resolve_* write it) into xr before the tile's blocks may overwrite the pair list.  false (nothing done, no barrier
// passed): this iteration's plan has more than 31 levels — the caller walks with exchange_walk_tile.
// (written out in full, like exchange_walk_tile_keys below and exchange_walk_lean in smm_chain_norm.hpp: on the shared staging pieces of
// smm_walk_lean.hpp the register allocation of k_chain_iter / k_chain_iter_norm moved, and k_chain_iter<0, 8, 1, true> ran 0.25 us longer — MEASUREMENTS.md.
// The layout's numbers and the reading of the plan's header word are the shared ones)
template <int NT>
__device__ inline bool exchange_walk_tile_lean(const KParams& P, const int tx, unsigned char* lds, const int tid, const bool valid, const int gc,
                                               unsigned long long& xr, const int ts_tile) {
    const int Ng = P.Ng;
    const int w = tx - P.plan_t0;
    const uint32_t* __restrict__ g_offp = P.lv_offp + (size_t)w * LV_OFFP;
    const uint4* __restrict__ g_pairs = (const uint4*)(P.lv_pairs_p + (size_t)w * P.plan_Kp);
    const int lane = tid & 63;
    const uint32_t Ng4 = lean_Ng4(Ng);
    const uint32_t pbase = LeanLayout<LEAN_TILE16>::pbase(Ng4);              // LDS offset of the pair words
    constexpr int PT = XLVL_MAX / NT;                     // chains per lane
    constexpr int PR = (XLVL_MAX + 64 * LV_MAXLEV + 4 * NT - 1) / (4 * NT);   // rounds of 16-byte loads for the pair words
    const uint32_t ov = g_offp[min(lane, LV_OFFP - 1)];   // lane l: first word of level l; lane 33: levels; lane 34: the plan fits
    double v_[PT];
#pragma unroll
    for (int r = 0; r < PT; ++r) {
        const int g = tid + r * NT;
        v_[r] = g < Ng ? P.vals[g] : 0.0;
    }
    uint4 p_[PR];
#pragma unroll
    for (int r = 0; r < PR; ++r) {
        const int q4 = tid + r * NT;
        p_[r] = 4 * q4 < P.plan_Kp ? g_pairs[q4] : make_uint4(0u, 0u, 0u, 0u);
    }
    const LeanPlanHead head = lean_plan_head(ov);
    const int nlev = head.nlev;
    if (!head.fits || (uint32_t)(size_t)lds != 0u) return false;
#pragma unroll
    for (int r = 0; r < PT; ++r) {
        const int g = tid + r * NT;
        if (g < Ng) ((uint4*)lds)[g] = make_uint4((uint32_t)__double2loint(v_[r]), (uint32_t)__double2hiint(v_[r]), (uint32_t)g, 0u);
    }
#pragma unroll
    for (int r = 0; r < PR; ++r) {
        const int q4 = tid + r * NT;
        if (4 * q4 < P.plan_Kp) ((uint4*)(lds + pbase))[q4] = p_[r];
    }
    if (tid < 2) ((uint4*)lds)[Ng4 + tid] = make_uint4(0u, 0u, 0u, 0u);   // the dummy pair's slots: 0 - 0 > min_improve is false
    const int ltail = lean_walk_tail(ov, nlev, lane);
    __syncthreads();
    if (P.ts && tid == 0) P.ts[(size_t)ts_tile * 8 + 5] = wall_clock64();   // staged
    const bool bytes16 = P.lean_wide && P.lean_unit == 16;   // the pair words hold byte offsets of 16-byte slots; else halves of them
    if (bytes16) lean_walk_levels<NT, 0, true>(nullptr, 0, pbase, ov, nlev, tid, ltail, P.mi_value);
    else lean_walk_levels<NT, 1, true>(nullptr, 0, pbase, ov, nlev, tid, ltail, P.mi_value);
    __syncthreads();   // (the narrow tail was wave 0's alone; the control waves of other tiles read now)
    if (valid) {
        const uint32_t meta = ((const uint4*)lds)[gc].z;
        const uint32_t partner = bytes16 ? lean_partner<0, 4>(lds, pbase, meta, (uint32_t)gc) : lean_partner<1, 4>(lds, pbase, meta, (uint32_t)gc);
        xr = (unsigned long long)(meta & 0xffffu) | ((unsigned long long)partner << 32);
    }
    __syncthreads();   // (from here on the tile's blocks may overwrite the pair list)
    return true;
}

#include "smm_cone.hpp"

// The lean KEY walk in k_chain_iter, for single shards of 4096 < N <= 8192 chains (BASELINE config 4: banana, 8192 chains — one
// launch per iteration instead of chain kernel + stand-alone resolution): 8-byte slots {order_key32(value), src | stamp << 16}
// built from the chains' values exactly as k_exch_resolve_lean builds them, min_improve == 0, dist_fun = -.  The control wave of
// every tile takes its chains' result (src | partner << 32) into xr.  false (uniform; nothing done): the plan has more than 31
// levels or a value is NaN — the host does not launch this form where it knows of either; loud where it happens anyway.
template <int NT>
__device__ inline bool exchange_walk_tile_keys(const KParams& P, const int tx, unsigned char* lds, const int tid, const bool valid, const int gc,
                                               unsigned long long& xr, const int ts_tile, const int gc2 = -1, uint32_t* src2 = nullptr) {
    const int Ng = P.Ng;
    const int w = tx - P.plan_t0;
    const uint32_t* __restrict__ g_offp = P.lv_offp + (size_t)w * LV_OFFP;
    const uint4* __restrict__ g_pairs = (const uint4*)(P.lv_pairs_p + (size_t)w * P.plan_Kp);
    const int lane = tid & 63;
    const uint32_t Ng4 = lean_Ng4(Ng);
    const uint32_t pbase = LeanLayout<LEAN_KEYS>::pbase(Ng4);               // LDS offset of the pair words
    constexpr int PR = (XLDS_MAX + 64 * LV_MAXLEV + 4 * NT - 1) / (4 * NT);   // rounds of 16-byte loads for the pair words
    const uint32_t ov = g_offp[min(lane, LV_OFFP - 1)];   // lane l: first word of level l; lane 33: levels; lane 34: the plan fits
    // the chains' slots as the accept step wrote them ({order_key32(value), chain}; a NaN value set the sticky flag): two per 16 bytes
    constexpr int SR = XLDS_MAX / (2 * NT);               // 16-byte pieces per lane
    const uint32_t wflags = P.walk_flags[tid & 3];        // (word 0 is looked at; a per-lane address keeps it a vector load among the others)
    uint4 s_[SR];
#pragma unroll
    for (int r = 0; r < SR; ++r) {
        const int q = tid + r * NT;
        s_[r] = 2 * q < Ng ? ((const uint4*)P.slot8)[q] : make_uint4(0u, 0u, 0u, 0u);
    }
    uint4 p_[PR];
#pragma unroll
    for (int r = 0; r < PR; ++r) {
        const int q4 = tid + r * NT;
        p_[r] = 4 * q4 < P.plan_Kp ? g_pairs[q4] : make_uint4(0u, 0u, 0u, 0u);
    }
    const LeanPlanHead head = lean_plan_head(ov);
    const int nlev = head.nlev;
    if (!head.fits || __builtin_amdgcn_readlane((int)wflags, 0) != 0 || (uint32_t)(size_t)lds != 0u) return false;
    uint2* slot = (uint2*)lds;
#pragma unroll
    for (int r = 0; r < SR; ++r) {
        const int q = tid + r * NT;
        if (2 * q < Ng) ((uint4*)lds)[q] = s_[r];
    }
#pragma unroll
    for (int r = 0; r < PR; ++r) {
        const int q4 = tid + r * NT;
        if (4 * q4 < P.plan_Kp) ((uint4*)(lds + pbase))[q4] = p_[r];
    }
    if (tid == 0) { slot[Ng4] = make_uint2(1u, 0u); slot[Ng4 + 1] = make_uint2(2u, 0u); }   // the dummy pair's slots: keys 1 < 2, "no swap"
    const int ltail = lean_walk_tail(ov, nlev, lane);
    __syncthreads();
    if (P.ts && tid == 0) P.ts[(size_t)ts_tile * 8 + 5] = wall_clock64();   // staged
    if (P.lean_unit == 8) lean_walk_levels<NT, 0>(P.vals, 1, pbase, ov, nlev, tid, ltail);
    else lean_walk_levels<NT, 1>(P.vals, 1, pbase, ov, nlev, tid, ltail);
    __syncthreads();   // (the narrow tail was wave 0's alone; the control waves of other tiles read now)
    if (valid) {
        const uint32_t meta = slot[gc].y;
        const uint32_t partner = P.lean_unit == 8 ? lean_partner<0>(lds, pbase, meta, (uint32_t)gc) : lean_partner<1>(lds, pbase, meta, (uint32_t)gc);
        xr = (unsigned long long)(meta & 0xffffu) | ((unsigned long long)partner << 32);
    }
    if (gc2 >= 0) *src2 = slot[gc2].y & 0xffffu;   // (the dense kind: the record source of the chain this lane loads)
    __syncthreads();   // (from here on the tile's blocks may overwrite the pair list)
    return true;
}

// ------------------------------------------------------------------------------------------
// k_chain_iter: one next_eval (AlgoBGP.jl:272-294) for every local chain, iteration t (1-based).
// rec_in : last accepted records after iteration t-1's accept step   [N][RW]
// rec_out: the same after iteration t's accept step (input of exchangeMoves!)
// Wave 0 is the tile's control wave: lane = r*CT + cl works for chain cl.  It moves the per-chain
// blocks with 16-byte pieces (two dependent levels: state/randomness/exchange result, then the
// record the chain continues from), evaluates the proposal tries side by side, and after the
// simulation lanes r == 0 run the accept step and the wave stores the result blocks.
// ------------------------------------------------------------------------------------------
// TPW tiles per workgroup (TPW = 2 with the inline exchange walk: the two tiles that would share a CU anyway
// become one workgroup of 1024 lanes, so the CU runs ONE walk with twice the lanes instead of two copies
// contending for its LDS; everything else is per tile, on the tile-local lane id).
// proposal batches of at least this many components are drawn a lane per component pair (below: a lane per try walks them)
#ifndef SMM_COOP_MIN_BATCH
#define SMM_COOP_MIN_BATCH 6
#endif
// (IW: the inline exchange walk is compiled in — contexts that never walk inline, larger populations and shards, run the kernel
// without it: the walk's code costs the latency-bound prologue registers and scalar spills even when it is never entered)
template <int KIND, int CT, int TPW = 1, bool IW = true>
__global__ __launch_bounds__(WG * TPW, 4) void k_chain_iter(const KParams P, const int t, const double* __restrict__ rec_in,
                                                            double* __restrict__ rec_out, const int flags) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    constexpr int NR = 64 / CT;
    const int np = P.np, nm = P.nm, N = P.N, RW = P.RW, HW = P.HW, RBW = P.RBW;
    const int st = (TPW > 1) ? __builtin_amdgcn_readfirstlane((int)threadIdx.x / WG) : 0;   // tile of this workgroup (wave-uniform: scalar)
    const int tid = (int)threadIdx.x - st * WG;             // lane of the tile
    const int tile = (int)blockIdx.x * TPW + st;
    TileSmem S;
    S.carve(smem + P.tile_off + (size_t)st * ((tile_smem_doubles(CT, np, nm, RW, HW, RBW, KIND) + 1) & ~(size_t)1), CT, np, nm, RW, HW,
            RBW, KIND != 0);
    const int cl = tid % CT, r = (tid % 64) / CT;
    const int c = tile * CT + cl;             // chain served by this lane (control wave only)
    const bool ctl = tid < 64;
    const bool valid = ctl && (c < N);
    const bool chain_lane = valid && r == 0;
    const int gc = P.offset + c;
    TS_MARK(0);

    // ---- global reads, all issued before anything waits ----
    double za[ZU];
    ZBuf zb;
    if constexpr (KIND == 1) { zb.init(P, tid); sim_load_chunk(zb, P, 0, 0, za); }
    int partner = 0;
    // a hard error raised by an earlier iteration (AlgoBGP.jl:341,409 abort the run): later launches store nothing
    unsigned long long err_word = ERR_NONE;
    if (ctl || KIND == 2 || (KIND == 0 && blockDim.x != 64)) err_word = *(const volatile unsigned long long*)P.err;   // (every wave that takes part in the shared epilogue: they meet at barriers behind the exit below)
    // wave 1: problem constants, requested now and written to LDS after the walk
    // (objectives without a simulation are launched with the control wave only, 64 lanes per tile: it loads the constants itself)
    const bool slim = KIND == 0 && blockDim.x == 64;
    const bool wave1 = slim ? ctl : (tid >= 64 && tid < 128);
    const int k1 = slim ? tid : tid - 64;
    double c_lb = 0.0, c_ub = 0.0, c_init = 0.0, c_mom = 0.0, c_w = 0.0;
    if (wave1) {
        if (k1 < np) { c_lb = P.lb[k1]; c_ub = P.ub[k1]; c_init = P.init[k1]; }
        if (k1 < nm) { c_mom = P.mom[k1]; c_w = P.w[k1]; }
    }
    {
        // level 1: exchange result, chain state block, this iteration's randomness block
        constexpr int NI_MAX = 4;   // pieces per lane held in registers; longer blocks finish with a load-store loop
        constexpr int NI_CS = (CSW / 2 + NR - 1) / NR < NI_MAX ? (CSW / 2 + NR - 1) / NR : NI_MAX;
        constexpr int NI_RB = (12 + NR - 1) / NR < NI_MAX ? (12 + NR - 1) / NR : NI_MAX;
        constexpr int NI_REC = (8 + NR - 1) / NR < NI_MAX ? (8 + NR - 1) / NR : NI_MAX;
        double2 v_cs[NI_CS], v_rb[NI_RB], v_rec[NI_REC];
        // the dense kind (long blocks: 832-byte records, 808 bytes of randomness per chain at 50 parameters) without an inline walk:
        // every wave of the tile moves the blocks, 32 lanes per chain — two round trips of two or three 16-byte loads per lane
        // (the control wave alone, 4 lanes per chain: 13 + 13 pieces per lane, most of them load-store round trips: 6 us)
        // (with the key walk in the prologue — P.gen_lean == 2, N_global <= 4096 — as well: its slots and lists lie UNDER the tile's blocks)
        const bool wide_load = KIND == 2 && (!(flags & F_WALK_INLINE) || P.gen_lean == 2);
        if (wide_load) {
            constexpr int L2 = WG / CT;
            const int ccw = tid / L2, rw = tid % L2;
            const int cw = tile * CT + ccw;
            const bool vw = cw < N;
            const int cwc = vw ? cw : 0;
            const int gcw = P.offset + cwc;
            double2 w_cs[1], w_rb[2], w_rec[2];
            const double* g_csw = P.cs + (size_t)cwc * CSW;
            const double* g_rbw = P.rb + ((size_t)(t > 1 ? t - P.rb_t0 : 0) * N + cwc) * RBW;
            const int rbww = t > 1 ? RBW : 0;
            unsigned long long xrw = (unsigned long long)(unsigned)gcw;
            const bool walk_here = IW && (flags & F_WALK_INLINE);
            if (vw) {
                if ((flags & F_HAS_PENDING) && !walk_here) xrw = P.xres[gcw];
                coop_fetch_n<1>(w_cs, g_csw, CSW, rw, L2);
                coop_fetch_n<2>(w_rb, g_rbw, rbww, rw, L2);
            }
            unsigned long long xr_ctl = (unsigned long long)(unsigned)gc;
            if constexpr (IW && KIND == 2 && TPW == 1) {
                if (walk_here) {
                    // exchangeMoves! of iteration t-1 by the tile's own walk over its cone (smm_cone.hpp; where the plan kernel made none: over
                    // the whole list), while the blocks above are in flight; nothing of the tile has been written to LDS yet
                    uint32_t srcw = (uint32_t)gcw;
                    bool done = false;
                    if (P.cone_ok) done = exchange_walk_tile_cone<WG, 0>(P, t - 1, (unsigned char*)smem, (int)threadIdx.x, valid, gc, xr_ctl, (int)blockIdx.x, tile, vw ? gcw : -1, &srcw);
                    if (!done && !exchange_walk_tile_keys<WG>(P, t - 1, (unsigned char*)smem, (int)threadIdx.x, valid, gc, xr_ctl, tile, vw ? gcw : -1, &srcw) && threadIdx.x == 0)
                        report_error(P, 3, t, gc);
                    xrw = (unsigned long long)srcw;
                }
            }
            if (wave1) {  // problem constants into the tile's LDS
                if (k1 < np) { S.lb[k1] = c_lb; S.ub[k1] = c_ub; S.init[k1] = c_init; }
                if (k1 < nm) { S.mom[k1] = c_mom; S.w[k1] = c_w; }
                for (int k = k1 + 64; k < np; k += 64) { S.lb[k] = P.lb[k]; S.ub[k] = P.ub[k]; S.init[k] = P.init[k]; }
                for (int k = k1 + 64; k < nm; k += 64) { S.mom[k] = P.mom[k]; S.w[k] = P.w[k]; }
            }
            if (vw) {
                const int sw = (int)(unsigned)(xrw & 0xffffffffu) - ((flags & F_GLOBAL_REC) ? 0 : P.offset);
                const double* g_recw = rec_in + (size_t)sw * RW;
                coop_fetch_n<2>(w_rec, g_recw, RW, rw, L2);
                coop_put_n<1>(S.cs + ccw * CSW, w_cs, g_csw, CSW, rw, L2);
                coop_put_n<2>(S.rb + ccw * RBW, w_rb, g_rbw, rbww, rw, L2);
                coop_put_n<2>(S.rec + ccw * RW, w_rec, g_recw, RW, rw, L2);
            }
            if (walk_here) { if (valid) partner = (int)(xr_ctl >> 32); }
            else if (valid && (flags & F_HAS_PENDING)) partner = (int)(P.xres[gc] >> 32);   // (the control wave's lanes serve other chains than they loaded)
        } else {
        const int cc = valid ? c : 0;
        const double* g_cs = P.cs + (size_t)cc * CSW;
        const double* g_rb = P.rb + ((size_t)(t > 1 ? t - P.rb_t0 : 0) * N + cc) * RBW;
        const int rbw = t > 1 ? RBW : 0;
        unsigned long long xr = (unsigned long long)(unsigned)gc;
        if (valid) {
            if ((flags & F_HAS_PENDING) && !(flags & F_WALK_INLINE)) xr = P.xres[gc];
            coop_fetch<CT, NI_CS>(v_cs, g_cs, CSW, r);
            coop_fetch<CT, NI_RB>(v_rb, g_rb, rbw, r);
        }
        if (IW && (flags & F_WALK_INLINE)) {
            // exchangeMoves! of iteration t-1, by all lanes of the tile, while the level-1 blocks are in flight
            // (the tile's own LDS blocks overlay the walk's pair list: nothing of the tile is written before this returns)
            if (P.gen_lean == 2) {   // 4096 < N <= 8192: the key walk (no other form fits the LDS at this size)
                bool done = false;
                if constexpr (WG * TPW == 1024) {   // the workgroup's cone, where the plan kernel made one (smm_cone.hpp)
                    if (P.cone_ok)
                        done = P.lean_unit == 8 ? exchange_walk_tile_cone<1024, 0>(P, t - 1, (unsigned char*)smem, (int)threadIdx.x, valid, gc, xr, (int)blockIdx.x, tile)
                                                : exchange_walk_tile_cone<1024, 1>(P, t - 1, (unsigned char*)smem, (int)threadIdx.x, valid, gc, xr, (int)blockIdx.x, tile);
                }
                if (!done && !exchange_walk_tile_keys<WG * TPW>(P, t - 1, (unsigned char*)smem, (int)threadIdx.x, valid, gc, xr, tile) && threadIdx.x == 0)
                    report_error(P, 3, t, gc);
            } else if (!(P.gen_lean && exchange_walk_tile_lean<WG * TPW>(P, t - 1, (unsigned char*)smem, (int)threadIdx.x, valid, gc, xr, tile))) {
                exchange_walk_tile<WG * TPW>(P, t - 1, (unsigned char*)smem, (int)threadIdx.x, tile);
                if (valid) {
                    const XSlot sv = ((const XSlot*)smem)[gc];
                    xr = (unsigned long long)sv.src | ((unsigned long long)sv.partner << 32);
                }
            }
        }
        if (KIND == 1 && tid == 64) *S.arrived = 0u;
        if (wave1) {  // problem constants into the tile's LDS (which the walk's pair list occupied until now)
            if (k1 < np) { S.lb[k1] = c_lb; S.ub[k1] = c_ub; S.init[k1] = c_init; }
            if (k1 < nm) { S.mom[k1] = c_mom; S.w[k1] = c_w; }
            for (int k = k1 + 64; k < np; k += 64) { S.lb[k] = P.lb[k]; S.ub[k] = P.ub[k]; S.init[k] = P.init[k]; }
            for (int k = k1 + 64; k < nm; k += 64) { S.mom[k] = P.mom[k]; S.w[k] = P.w[k]; }
        }
        if (valid) {
            // level 2: the record the chain continues from (its own, or the donor's)
            const int s = (int)(unsigned)(xr & 0xffffffffu) - ((flags & F_GLOBAL_REC) ? 0 : P.offset);
            partner = (int)(xr >> 32);
            const double* g_rec = rec_in + (size_t)s * RW;
            coop_fetch<CT, NI_REC>(v_rec, g_rec, RW, r);
            coop_put<CT, NI_CS>(S.cs + cl * CSW, v_cs, g_cs, CSW, r);
            coop_put<CT, NI_RB>(S.rb + cl * RBW, v_rb, g_rb, rbw, r);
            coop_put<CT, NI_REC>(S.rec + cl * RW, v_rec, g_rec, RW, r);
        }
        }
    }
    TS_MARK(1);
    __syncthreads();

    // ---- settle iteration t-1 (chain lanes; registers + LDS only) ----
    // (its results go back to the LDS block and are read again after the simulation: nothing of the serial
    // bookkeeping stays in registers across the register-hungry simulation loop)
    if (chain_lane) {
        double* csb = S.cs + cl * CSW;
        int nn = (int)csb[CS_NNOEX], na = (int)csb[CS_NACC];
        double bp = csb[CS_BEST], bpid = csb[CS_BESTID];
        if (t > 1) {
            bool exch_prev = false;
            if (partner != 0) {  // swap_ev_ij!, :734-749: iteration t-1's record becomes the donor's
                exch_prev = true;
                // (the parameters and moments of the donor's record are copied by all lanes of the chain: copy_strided below)
                const Best b = swapped_head(S.hp + cl * HW, S.rec + cl * RW, partner, t - 1, csb + CS_BESTP);
                bp = b.best; bpid = b.best_id;
            } else if (csb[CS_WASX] != 0.0) {  // sharded path: k_exch_apply already rewrote record and history
                exch_prev = true;
            }
            if ((flags & F_CLOSE_PREV) && !exch_prev) { nn += 1; na += (int)csb[CS_LACC]; }  // set_acceptRate!, :253-257
        }
        csb[CS_NNOEX] = (double)nn; csb[CS_NACC] = (double)na; csb[CS_BEST] = bp; csb[CS_BESTID] = bpid;
        csb[CS_PARTNER] = (double)partner;
    }
    if (valid && t > 1 && partner != 0)   // parameters and moments of the donor's record into the rewritten history row, NR lanes per chain
        copy_strided(S.hp + cl * HW + H_PARAMS, S.rec + cl * RW + 3, np + nm, r, NR);
    TS_MARK(5);
    // ---- proposal(c), AlgoBGP.jl:424-471: lane (cl, r) evaluates try r of chain cl ----
    {
        double* th = S.theta + cl * np;
        const double* rc = S.rec + cl * RW;
        const bool draws = (t > 1) && !(P.dbg & 1);   // uniform: iteration 1 proposes the initial value (:426-427)
        if (ctl && (!draws || !valid)) {
            if (r == 0)
                for (int k = 0; k < np; ++k) th[k] = !valid ? 0.0 : (t == 1 ? S.init[k] : rc[3 + k]);
        }
        if (draws) {   // the control wave's 64 lanes walk the batches together; lanes of absent chains take no part in the tries
            const int bs = P.batch_size;
            const int max_tries = P.user_n ? min(P.rb_tries, P.smpl_iters) : P.smpl_iters;
            const int npar = min(min(NR, P.rb_tries), max_tries);  // tries evaluated side by side
            const double sg = S.cs[cl * CSW + CS_SIGMA];
            const double* zz = S.rb + cl * RBW + 1;  // [tries][np]
            // mapto_01 (mprob.jl:248) once per chain and parameter — one division each, shared by all tries —, computed by the
            // NR lanes of the chain and kept in the (still unused) output record block
            double* m01 = S.rout + cl * RW;
            // Many components (the whole proposal was 10.5 us per iteration at 50 parameters: one lane per chain and try walking
            // all the components, then the redraw loop of mysample): every wave of the tile works, a chain is served by
            // 64 * waves / CT lanes of ONE wave, a lane by the component pairs q = sl, sl + LPC, ... (one generator call per pair
            // and try).  The tries are taken in order, each one tested by all the chain's lanes at once (a segment of the
            // wave's ballot); the first one inside the unit box wins: same tries, same order, same winner as the serial form.
            // With a Cholesky factor (bs == np) a lane segment keeps the np normals of the try it evaluates in the moments' part of its
            // (still unused) history row, behind the candidate: nm doubles.  Contexts with FEWER MOMENTS THAN PARAMETERS (nm < np: a
            // dense objective like 33 x 17, a user objective with a few moments) have no room there and keep the serial form below.
            const bool coop = bs >= SMM_COOP_MIN_BATCH && (!P.chol_L || nm >= np);   // (uniform)
            if (coop) {
                __syncthreads();   // the blocks the control wave staged (records, state, randomness) are every wave's now
                // (smm_propose.hpp: every wave of the tile works, 64 * waves / CT lanes per chain)
                const CoopProp X{S.rec, RW, S.rout, RW, S.theta, np, S.h, HW, S.rb, RBW, S.cs, CSW, S.lb, S.ub,
                                 (unsigned long long*)(S.h - (size_t)st * ((tile_smem_doubles(CT, np, nm, RW, HW, RBW, KIND) + 1) & ~(size_t)1)) + 2, P.err,
                                 P.seed, P.offset, N, bs, P.rb_tries, P.user_n, P.smpl_iters, P.scout_after, P.scout_gl,
                                 P.chol_L, P.chol_per_chain, S.h + H_PARAMS + np, HW};
                if (P.chol_L) coop_mysample<CT, true>(X, t, tile, tid, (int)blockDim.x / (64 * TPW), threadIdx.x == 0, CoopSyncThreads());
                else coop_mysample<CT, false>(X, t, tile, tid, (int)blockDim.x / (64 * TPW), threadIdx.x == 0, CoopSyncThreads());
            } else if (ctl) {
            if (valid)
                for (int k = r; k < np; k += NR) {
                    const double lbk = S.lb[k];
                    m01[k] = (rc[3 + k] - lbk) / (S.ub[k] - lbk);
                }
            __builtin_amdgcn_wave_barrier();
            for (int b0 = 0; b0 < np; b0 += bs) {
                bool ok = valid && r < npar;
                if (ok) {
                    for (int k = b0; k < b0 + bs; ++k) {  // mysample, :400-410, try r
                        const double mu01 = m01[k];
                        const double step = sg * prop_direction(P, zz + r * np, k, gc);  // MvNormal(mu01, sigma): x = mu + sigma*z
                        const double x = mu01 + step;
                        if (!(x >= 0.0 && x <= 1.0)) ok = false;  // inclusive bounds, :405
                    }
                }
                const unsigned long long m = __ballot(ok);  // first successful try of every chain
                unsigned long long pat = 0;
#pragma unroll
                for (int rr = 0; rr < NR; ++rr) pat |= ((m >> (rr * CT + cl)) & 1ull) << rr;
                const int rwin = pat ? (__ffsll((long long)pat) - 1) : -1;
                if (valid && rwin == r) {
                    for (int k = b0; k < b0 + bs; ++k) {
                        const double lbk = S.lb[k];
                        const double span = S.ub[k] - lbk;
                        const double mu01 = m01[k];
                        const double step = sg * prop_direction(P, zz + r * np, k, gc);
                        const double x = mu01 + step;
                        const double sc = x * span;
                        th[k] = sc + lbk;  // mapto_ab, mprob.jl:271
                    }
                }
                if (valid && r == 0 && rwin < 0) {   // every failing chain's own lane redraws one try at a time (chains in parallel)
                    bool ok2 = false;
                    for (int rr = npar; rr < max_tries && !ok2; ++rr) {
                        ok2 = true;
                        double zc0 = 0.0, zc1 = 0.0;
                        int zq = -1;
                        const double* zv = zz + rr * np;   // Cholesky kernel: the whole try's normals
                        if (P.chol_L && rr >= P.rb_tries) {   // ... generated into the (still unused) history row of the chain
                            double* sc = S.h + cl * HW;
                            for (int q = 0; 2 * q < np; ++q) {
                                const double2 zz2 = rng_prop_normal2_outofline(P.seed, (uint32_t)gc, (uint32_t)t, (uint32_t)rr, (uint32_t)q);
                                sc[2 * q] = zz2.x;
                                if (2 * q + 1 < np) sc[2 * q + 1] = zz2.y;
                            }
                            zv = sc;
                        }
                        for (int k = b0; k < b0 + bs; ++k) {
                            const double lbk = S.lb[k];
                            const double span = S.ub[k] - lbk;
                            const double mu01 = m01[k];
                            double z;
                            if (P.chol_L) {
                                z = prop_direction(P, zv, k, gc);
                            } else if (rr < P.rb_tries) {
                                z = zz[rr * np + k];
                            } else {
                                if ((k >> 1) != zq) {
                                    zq = k >> 1;
                                    const double2 zz2 = rng_prop_normal2_outofline(P.seed, (uint32_t)gc, (uint32_t)t, (uint32_t)rr, (uint32_t)zq);
                                    zc0 = zz2.x; zc1 = zz2.y;
                                }
                                z = (k & 1) ? zc1 : zc0;
                            }
                            const double step = sg * z;
                            const double x = mu01 + step;
                            if (!(x >= 0.0 && x <= 1.0)) ok2 = false;
                            const double sc = x * span;
                            th[k] = sc + lbk;
                        }
                    }
                    if (!ok2) report_error(P, ERRK_NO_DRAW, t, gc);  // :409
                }
            }
            }
        }
    }
    TS_MARK(6);
    __syncthreads();
    TS_MARK(2);
    if (flags & F_PROPOSE_ONLY) {  // user objective: hand the proposals to the user's kernel; nothing has been stored yet, the
        if (valid && !error_before(err_word, t))   // accept launch repeats this (deterministic) prologue
            for (int k = r; k < np; k += NR) P.u_theta[(size_t)c * np + k] = S.theta[cl * np + k];
        return;
    }

    // ---- simulation: all 512 lanes, ns draws x nm moments x CT chains ----
    if constexpr (KIND == 1) {
        if (!(P.dbg & 2)) simulate_tile<CT>(P, zb, S.theta, S.part, tid, za);
        // No workgroup barrier here: only the tile's control wave consumes the partial sums.  Every wave announces
        // its partials with one LDS add and is done; the control wave waits for the tile's 8 announcements.  (With
        // two tiles per workgroup a barrier would also make the faster tile wait for the slower one.)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        if ((tid & 63) == 0) __hip_atomic_fetch_add(S.arrived, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (!ctl) return;
        while (__hip_atomic_load(S.arrived, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < (unsigned)(WG / 64))
            __builtin_amdgcn_s_sleep(1);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    } else if constexpr (KIND == 2) {
        dense_tile<CT>(P, S.theta, S.part, tid);
        __syncthreads();
    }
    TS_MARK(3);
    if (P.dbg & 4) return;
    if (error_before(err_word, t)) return;

    // ---- objective value, doAcceptReject! (:324-392), set_eval! (:220-245) ----
    // the moments of a chain (wave totals -> mean -> squared weighted deviation) are independent: its NR lanes share them
    const bool sumsq = KIND != 0 && P.obj != SMM_OBJ_USER && P.obj != SMM_OBJ_BANANA;
    // (the dense kind has all its waves here: the terms, and below the copies and the stores of the long blocks, are shared by the
    // tile's 512 lanes, 32 per chain — the control wave alone: 7.3 + 3.5 us per iteration at 50 parameters and 50 moments)
    // (so do objectives without a simulation wherever the tile was launched with all its waves — the key form of C4: its other waves
    // have nothing to do after the walk: 403 -> 410 M chain-evals/s)
    constexpr int LPC2 = WG / CT;   // lanes per chain when every wave of the tile takes part
    const int cc2 = tid / LPC2, r2 = tid % LPC2;
    const bool coop_epi = KIND == 2 || (KIND == 0 && !slim);
    const bool valid2 = coop_epi && tile * CT + cc2 < N;
    if (coop_epi) {
        if (valid2 && sumsq) {
            double* smk = S.h + cc2 * HW + H_PARAMS + np;
            double* vkk = S.rout + cc2 * RW;          // (the proposal's scratch: free again)
            for (int k = r2; k < nm; k += LPC2) moment_term<CT>(P, S.part, S.mom, S.w, cc2, k, smk[k], vkk[k]);
        }
        __syncthreads();
    } else if (valid && sumsq) {
        double* smk = S.h + cl * HW + H_PARAMS + np;
        double* vkk = S.rout + cl * RW;          // (the proposal's scratch: free again)
        for (int k = r; k < nm; k += NR) moment_term<CT>(P, S.part, S.mom, S.w, cl, k, smk[k], vkk[k]);
    }
    __builtin_amdgcn_wave_barrier();
    if (chain_lane) {
        const double* th = S.theta + cl * np;
        const double* rc = S.rec + cl * RW;
        double* hr = S.h + cl * HW;
        double* ro = S.rout + cl * RW;
        double* csb = S.cs + cl * CSW;
        double* sm = hr + H_PARAMS + np;
        double value;
        int status;
        finish_objective<CT>(P, th, S.part, S.mom, S.w, cl, sm, value, status, c, sumsq ? S.rout + cl * RW : nullptr);
        const double sig = csb[CS_SIGMA], bp = csb[CS_BEST], bpid = csb[CS_BESTID], atun = csb[CS_ATUN];
        const int nn = (int)csb[CS_NNOEX], na = (int)csb[CS_NACC];
        const double u = t > 1 ? S.rb[cl * RBW] : 0.0;  // probs_acc[iter], :85

        const double old = rc[0];
        const AcceptDecision d = accept_decide(t == 1, status, value, old, atun, u, smm_exp);
        if (d.negative) report_error(P, ERRK_NEGATIVE, t, gc);
        const double prob = d.prob;
        const bool acc = d.acc;
        status = d.status;
        TS_MARK(7);
        const double rate = accept_rate(na, nn, acc);   // (iteration t has exchanged==0 at this point)
        double nsig = sig;
        if (t > 1 && (t % P.sigma_update_steps) == 0) nsig = sigma_next(sig, rate, P.sigma_adjust_by);
        // set_eval!: curr_val[t-1] == value of the last accepted record
        const double currv = acc ? value : old;
        const Best b = t == 1 ? Best{value, 1.0} : best_of(value, t, bp, bpid);
        const double bestv = b.best, bestid = b.best_id;
        csb[CS_SIGMA] = nsig; csb[CS_RATE] = rate; csb[CS_NNOEX] = (double)nn; csb[CS_NACC] = (double)na;
        csb[CS_LACC] = acc ? 1.0 : 0.0; csb[CS_WASX] = 0.0; csb[CS_BEST] = bestv; csb[CS_BESTID] = bestid;
        csb[CS_BESTP] = bp; csb[CS_BESTPID] = bpid;  // best after t-1: needed if iteration t gets exchanged
        history_head(hr, value, prob, currv, bestv, bestid, 0.0, acc ? 1.0 : 0.0, (double)status);
        // the chain's last accepted record = input of the exchange step: its head here, the
        // parameter and moment arrays (and the history row's parameters) by all lanes of the chain below
        record_head(ro, rc, acc, value, prob, status);
        const double vnew = acc ? value : old;
        P.vals_out[c] = vnew;
        if (P.slots17_out) {   // the chain's initial slots of k_exch_resolve_rows / _key (what k_exch_keys would make of vals[c])
            P.slots17_out[c] = (uint32_t)gc | (order_key17(vnew) << 15);
            if (vnew != vnew) atomicOr(P.nan_flags_out, 1u);
        }
        if (P.slot8_out) {   // the chain's slot at the start of the next inline key walk (exchange_walk_tile_keys)
            P.slot8_out[c] = make_uint2(order_key32(vnew), (uint32_t)gc);
            if (vnew != vnew) atomicOr(P.walk_flags, 1u);
        }
    }
    __builtin_amdgcn_wave_barrier();
    if (coop_epi) {
        __syncthreads();   // the accept step's results (history head, record head, state block) are every wave's now
        if (valid2) {      // (a chain's 32 lanes sit in one wave: its copies are in place before its stores read them)
            const int c2 = tile * CT + cc2;
            const bool acc = S.h[cc2 * HW + H_ACC] != 0.0;
            copy_strided(S.h + cc2 * HW + H_PARAMS, S.theta + cc2 * np, np, r2, LPC2);
            if (acc) {
                copy_strided(S.rout + cc2 * RW + 3, S.theta + cc2 * np, np, r2, LPC2);
                copy_strided(S.rout + cc2 * RW + 3 + np, S.h + cc2 * HW + H_PARAMS + np, nm, r2, LPC2);
            } else {
                copy_strided(S.rout + cc2 * RW + 3, S.rec + cc2 * RW + 3, RW - 3, r2, LPC2);
            }
            __builtin_amdgcn_wave_barrier();
            coop_store_n(P.cs + (size_t)c2 * CSW, S.cs + cc2 * CSW, CSW, r2, LPC2);
            coop_store_n(rec_out + (size_t)c2 * RW, S.rout + cc2 * RW, RW, r2, LPC2);
            coop_store_n(P.hrec + ((size_t)(t - 1) * N + c2) * HW, S.h + cc2 * HW, HW, r2, LPC2);
            if (t > 1 && S.cs[cc2 * CSW + CS_PARTNER] != 0.0)
                coop_store_n(P.hrec + ((size_t)(t - 2) * N + c2) * HW, S.hp + cc2 * HW, HW, r2, LPC2);
        }
        TS_MARK(4);
        return;
    }
    if (valid) {
        const bool acc = S.h[cl * HW + H_ACC] != 0.0;
        copy_strided(S.h + cl * HW + H_PARAMS, S.theta + cl * np, np, r, NR);
        if (acc) {
            copy_strided(S.rout + cl * RW + 3, S.theta + cl * np, np, r, NR);
            copy_strided(S.rout + cl * RW + 3 + np, S.h + cl * HW + H_PARAMS + np, nm, r, NR);
        } else {
            copy_strided(S.rout + cl * RW + 3, S.rec + cl * RW + 3, RW - 3, r, NR);
        }
    }
    // ---- the control wave stores the tile's result blocks ----
    if (valid) {
        __builtin_amdgcn_wave_barrier();
        coop_store<CT>(P.cs + (size_t)c * CSW, S.cs + cl * CSW, CSW, r);
        coop_store<CT>(rec_out + (size_t)c * RW, S.rout + cl * RW, RW, r);
        coop_store<CT>(P.hrec + ((size_t)(t - 1) * N + c) * HW, S.h + cl * HW, HW, r);
        if (t > 1 && S.cs[cl * CSW + CS_PARTNER] != 0.0)
            coop_store<CT>(P.hrec + ((size_t)(t - 2) * N + c) * HW, S.hp + cl * HW, HW, r);
    }
    TS_MARK(4);
}

// k_flush: settle the last iteration (pending exchange + accept-rate counters) without starting a
// new one, so that state/history can be read back or saved (save/readMalgo, AlgoAbstract.jl:83-102).
__global__ void k_flush(const KParams P, const int t_next, const double* __restrict__ rec_in, double* __restrict__ rec_out,
                        const int flags) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= P.N) return;
    if (*(const volatile unsigned long long*)P.err != ERR_NONE) return;   // the run stopped at the failing iteration
    const int RW = P.RW, HW = P.HW, N = P.N;
    double* csb = P.cs + (size_t)c * CSW;
    const int goff = (flags & F_GLOBAL_REC) ? 0 : P.offset;   // rec_in indexed by global chain id (all-gathered buffer)?
    int s = P.offset + c - goff;
    bool exch = false;
    if (flags & F_HAS_PENDING) {
        const unsigned long long xr = P.xres[P.offset + c];
        const int partner = (int)(xr >> 32);
        if (partner != 0) {
            exch = true;
            s = (int)(unsigned)(xr & 0xffffffffu) - goff;
            const int tp = t_next - 1;
            const double* donor = rec_in + (size_t)s * RW;
            double* hrec = P.hrec + ((size_t)(tp - 1) * N + c) * HW;
            const Best b = swapped_head(hrec, donor, partner, tp, csb + CS_BESTP);
            for (int k = 0; k < P.np + P.nm; ++k) hrec[H_PARAMS + k] = donor[3 + k];
            csb[CS_BEST] = b.best; csb[CS_BESTID] = b.best_id;
        }
    } else if (csb[CS_WASX] != 0.0) {
        exch = true;
        csb[CS_WASX] = 0.0;
    }
    if ((flags & F_CLOSE_PREV) && !exch) {
        csb[CS_NNOEX] += 1.0;
        csb[CS_NACC] += csb[CS_LACC];
    }
    for (int f = 0; f < RW; ++f) rec_out[(size_t)c * RW + f] = rec_in[(size_t)s * RW + f];
}

// One tile of CT evaluations out of n, evaluation i = blockIdx.x * CT + lane: what every batched evaluation kernel of the built-in
// objectives runs (k_eval_batch here; the estimators' k_eval_slice and k_eval_lm, smm_evalscratch.hpp) -> value [n], simM [nm][n], status
// [n].  The kernels differ in where a tile's parameters come from: fill(S, tid) writes S.theta [CT][np] — 0.0 for the evaluations past
// n — before the first barrier.
template <int KIND, int CT, class Fill>
__device__ __forceinline__ void eval_tile(const KParams& P, const int n, Fill fill, double* __restrict__ out_value, double* __restrict__ out_simM,
                                          int8_t* __restrict__ out_status) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    TileSmem S;
    S.carve(smem, CT, P.np, P.nm, P.RW, P.HW, P.RBW, KIND != 0);
    const int tid = threadIdx.x;
    const int i = blockIdx.x * CT + tid;
    const bool chain_lane = (tid < CT) && (i < n);
    double za[ZU];
    ZBuf zb;
    if constexpr (KIND == 1) { zb.init(P, tid); sim_load_chunk(zb, P, 0, 0, za); }
    if (tid >= 64 && tid < 128)
        for (int k = tid - 64; k < P.nm; k += 64) { S.mom[k] = P.mom[k]; S.w[k] = P.w[k]; }
    fill(S, tid);
    __syncthreads();
    if constexpr (KIND == 1) {
        simulate_tile<CT>(P, zb, S.theta, S.part, tid, za);
        __syncthreads();
    } else if constexpr (KIND == 2) {
        dense_tile<CT>(P, S.theta, S.part, tid);
        __syncthreads();
    }
    if (chain_lane) {
        double v;
        int st;
        double* sm = S.h + tid * P.HW;
        finish_objective<CT>(P, S.theta + tid * P.np, S.part, S.mom, S.w, tid, sm, v, st);
        out_value[i] = v;
        out_status[i] = (int8_t)st;
        for (int k = 0; k < P.nm; ++k) out_simM[(size_t)k * n + i] = sm[k];
    }
}

// batched evaluateObjective(m,p), mprob.jl:175-188: params [np][M] -> value, simM [nm][M], status
template <int KIND, int CT>
__global__ __launch_bounds__(WG, 4) void k_eval_batch(const KParams P, const double* __restrict__ params, const int M,
                                                      double* __restrict__ value, double* __restrict__ simM,
                                                      int8_t* __restrict__ status) {
    eval_tile<KIND, CT>(P, M, [&](const TileSmem& S, const int tid) {   // (lanes tid < CT: np loads each)
        const int i = blockIdx.x * CT + tid;
        if (tid < CT)
            for (int k = 0; k < P.np; ++k) S.theta[tid * P.np + k] = i < M ? params[(size_t)k * M + i] : 0.0;
    }, value, simM, status);
}

// objfunc_norm with options[:noseed] = true (ObjExamples.jl:71-75): every evaluation draws its own shock matrix (the
// counter generator keyed by base_seed + i) — getSigma's repetitions (econometrics.jl:125-145).  One workgroup per
// evaluation; lane l generates and sums its draws l, l + 512, ... (the numerical contract of the seeded form).
__global__ __launch_bounds__(WG) void k_eval_batch_noseed(const KParams P, const double* __restrict__ params, const int M,
                                                          const uint64_t base_seed, double* __restrict__ value,
                                                          double* __restrict__ simM, int8_t* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) double smem[];   // [WG/64][nm] wave totals
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nm = P.nm, ns = P.ns;
    const uint64_t seed = base_seed + (uint64_t)i;
    for (int q = 0; 2 * q < nm; ++q) {   // one Philox block serves moments 2q and 2q+1
        const int k0 = 2 * q, k1 = 2 * q + 1;
        const double mu0 = params[(size_t)k0 * M + i], mu1 = k1 < nm ? params[(size_t)k1 * M + i] : 0.0;
        double a0 = 0.0, a1 = 0.0;
        for (int s = tid; s < ns; s += WG) {
            double z0, z1;
            box_muller(philox_stream(seed, STREAM_Z, (uint32_t)s, (uint32_t)q, 0, 0), z0, z1);
            const double x0 = z0 + mu0, x1 = z1 + mu1;
            a0 = a0 + x0;
            a1 = a1 + x1;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) { a0 = a0 + __shfl_xor(a0, off, 64); a1 = a1 + __shfl_xor(a1, off, 64); }
        if (lane == 0) { smem[wave * nm + k0] = a0; if (k1 < nm) smem[wave * nm + k1] = a1; }
    }
    __syncthreads();
    if (tid == 0) {
        double vsum = 0.0;
        for (int k = 0; k < nm; ++k) {
            double tot = smem[k];
            for (int wv = 1; wv < WG / 64; ++wv) tot = tot + smem[wv * nm + k];
            const double m = tot / (double)ns;
            simM[(size_t)k * M + i] = m;
            const double v = moment_sq(m, P.mom[k], P.w[k]);
            vsum = (k == 0) ? v : vsum + v;
        }
        value[i] = vsum / (double)nm;
        status[i] = 1;
    }
}
