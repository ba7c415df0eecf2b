// pooled summaries of groups of chains on the device (smm_get_group_stats, include/smmhip.h) — part of libsmmhip (included by smmhip.hip
// inside its anonymous namespace after smm_cov.hpp; gfx950 device code).  Reads the history records hrec [T][N][HW] (smm_params.hpp: H_*)
// and nothing else; writes only the scratch and result buffers of the call.  A group's pooled column is the concatenation of its member
// chains' selected draws, members in ascending local index; the groups' pooled columns lie one after another in the pooled index space
// (group g from G0[g]), and each group's column is cut into chunks of STATS_LDS_N draws starting at its own first draw.
//
//   k_group_gather    : one workgroup per chain streams the chain's records of the window, 256 iterations at a time (lane = iteration):
//                       the rows of select 0 / 1 at their rank among the selected ones (block_rank), the state rows of select 2 at their
//                       iteration (state_walk; both smm_window.hpp).  kb = 0: the count only.  Packed form: columns [k0, k0 + kb) to col
//                       [kb][Mtot] at off[c] + rank.  Chunked form: every column, centred by its group's mean, to col [D][Nbc]
//                       [STATS_LDS_N] at (chunk, position in chunk) for the chunks [cb0, cb0 + Nbc) only.  The columns are the np
//                       parameters (smm_get_group_stats) or the D = np + nm joint columns (smm_get_moment_stats, smm_moments.hpp).
//   k_group_chunk_sum : one workgroup per (chunk, parameter) of the packed columns: the chunk's pairwise sum (stats_pw through pw_sum,
//                       smm_stats.hpp) and whether it holds a NaN.
//   k_group_mean      : one lane per (group, parameter): the chunk sums added in order, S = S + s_c, then S / m (the chain-stats mean).
//   k_group_small     : one workgroup per short column (m <= STATS_LDS_N): its keys sorted in LDS (stats_sort), median and quantiles.
//   k_group_hist      : one digit of the grid-wide radix select of the longer columns (the contract's 6 digits of 11/11/11/11/11/9 bits of
//                       stats_key): many workgroups per column, each with an LDS histogram per rank of the keys that match the rank's
//                       prefix so far, added into the global per-(column, rank) histogram by device-scope integer atomics.
//   k_group_pick      : one workgroup per (column, rank): the digit holding the rank and the count below it; zeroes the histogram.
//   k_group_finish    : one lane per long column: median and quantiles from the selected keys (stats_quantile over 64-bit ranks).
//   k_cov_pairs       : (smm_cov.hpp, raw) the chunk sums of every pair's centred products, the chunked columns taken as its chains.
//   k_group_cov       : one lane per (group, pair j >= k): the chunk sums added in order, / (m - 1), both triangles.
#pragma once

constexpr int GROUP_RB = 4;          // ranks one k_group_hist workgroup counts (4 LDS histograms of 2048 bins: 32 KB)
constexpr int GROUP_BINS = 2048;     // bins of a digit (11 bits; the last digit uses 512)
constexpr size_t GROUP_HIST_CAP = (size_t)32 << 20;   // bytes of global histograms: the long columns are selected this many at a time

// One workgroup per chain.  sel: 0 every row of the window, 1 the accepted rows, 2 row a(t) of every iteration (a row without one reads
// NaN).  Columns [k0, k0 + kb) of the D pooled ones, which lie behind H_PARAMS in the record (the parameters, then the simulated moments).
// counting != 0 (sel 0 / 1, kb = 0): count[c] = the chain's selected rows.  Otherwise count[c] is read: a chain outside every group, or
// with no row in the chunks [cb0, cb0 + Nbc) of the chunked form (cch0 != NULL), reads nothing.  gbad (NULL: not tested): gbad[g] = 1
// for a value that is not finite among the columns written (the chunked form: of the rows of its chunks, before they are centred).
__global__ __launch_bounds__(STATS_WG) void k_group_gather(const double* __restrict__ hrec, int N, int HW, int t0, int n, int sel,
                                                           const int* __restrict__ gid, const long long* __restrict__ off,
                                                           const int* __restrict__ cch0, int k0, int kb, long long Mtot, int cb0, int Nbc,
                                                           const double* __restrict__ gmean, int D, double* __restrict__ col,
                                                           int* __restrict__ count, int counting, int* __restrict__ gbad) {
    __shared__ int wtot[STATS_WG / 64];
    const int c = xcd_chain(blockIdx.x, gridDim.x), tid = threadIdx.x;
    const int g = gid[c];
    const bool chunked = cch0 != nullptr;
    long long o = 0;
    if (!counting) {
        if (g < 0 || count[c] == 0) return;
        o = off[c];
        if (chunked && (cch0[c] + o / STATS_LDS_N >= cb0 + Nbc || cch0[c] + (o + count[c] - 1) / STATS_LDS_N < cb0)) return;
    }
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    // pooled position pos takes the columns of record h (NULL: no state row yet)
    auto put = [&](long long pos, const double* __restrict__ h) {
        if (!chunked) {
            bool bad = false;
            for (int kk = 0; kk < kb; ++kk) {
                const double v = h ? h[H_PARAMS + k0 + kk] : qnan;
                if (gbad) bad |= !isfinite(v);
                col[(size_t)kk * Mtot + pos] = v;
            }
            if (bad) gbad[g] = 1;
        } else {
            const long long ch = cch0[c] + pos / STATS_LDS_N - cb0;
            if (ch < 0 || ch >= Nbc) return;
            const size_t at = (size_t)ch * STATS_LDS_N + (size_t)(pos % STATS_LDS_N);
            bool bad = false;
            for (int kk = 0; kk < kb; ++kk) {
                const double v = h ? h[H_PARAMS + k0 + kk] : qnan;
                if (gbad) bad |= !isfinite(v);
                col[(size_t)kk * Nbc * STATS_LDS_N + at] = v - gmean[(size_t)g * D + k0 + kk];
            }
            if (bad) gbad[g] = 1;
        }
    };
    if (sel == 2) {
        state_walk(hrec, N, HW, c, t0, n, wtot, [&](int r, int a, bool) { put(o + r, a < 0 ? nullptr : hrec + ((size_t)a * N + c) * HW); });
        return;
    }
    long long base = 0;
    for (int r0 = 0; r0 < n; r0 += STATS_WG) {
        const int r = r0 + tid;
        const bool valid = r < n;
        const double* h = hrec + ((size_t)(t0 + (valid ? r : 0)) * N + c) * HW;
        const bool take = valid && (sel == 0 || h[H_ACC] != 0.0);
        const long long pos = o + block_rank(take, wtot, base);
        if (take && kb > 0) put(pos, h);
    }
    if (counting && tid == 0) count[c] = (int)base;
}

__global__ __launch_bounds__(STATS_WG) void k_group_chunk_sum(const double* __restrict__ col, long long Mtot, const long long* __restrict__ cst,
                                                              const int* __restrict__ clen, int NC, double* __restrict__ csum,
                                                              int* __restrict__ cnan) {
    extern __shared__ __align__(16) double sx[];   // STATS_LDS_N
    __shared__ PwTree pt;   // (pt.flag: a NaN among the draws)
    const int ch = blockIdx.x, kk = blockIdx.y, tid = threadIdx.x;
    const double* x = col + (size_t)kk * Mtot + cst[ch];
    if (tid == 0) pt.flag = 0;
    __syncthreads();
    const double s = pw_sum(clen[ch], [&](int i) { const double v = x[i]; if (v != v) pt.flag = 1; return v; }, sx, pt);
    if (tid == 0) {
        csum[(size_t)kk * NC + ch] = s;
        cnan[(size_t)kk * NC + ch] = pt.flag;
    }
}

__global__ void k_group_mean(const double* __restrict__ csum, const int* __restrict__ cnan, int NC, const int* __restrict__ gch0,
                             const long long* __restrict__ gm, int G, int k0, int kb, int np, double* __restrict__ o_mean,
                             int* __restrict__ o_nan) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= G * kb) return;
    const int g = e / kb, kk = e - g * kb, k = k0 + kk;
    double S = 0.0;
    int bad = 0;
    for (int ch = gch0[g]; ch < gch0[g + 1]; ++ch) { S = S + csum[(size_t)kk * NC + ch]; bad |= cnan[(size_t)kk * NC + ch]; }
    const long long m = gm[g];
    o_mean[(size_t)g * np + k] = m == 0 ? __longlong_as_double(0x7ff8000000000000ll) : S / (double)m;
    o_nan[(size_t)g * np + k] = bad;
}

// median and quantiles of group g, parameter k from at(i) = its i-th smallest draw; NaN for a NaN among the draws or no draw
template <class At>
__device__ void group_order_out(long long m, bool bad, At at, int g, int k, int G, int np, const double* __restrict__ probs, int nq,
                                double* __restrict__ o_median, double* __restrict__ o_quant) {
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    if (o_median)
        o_median[(size_t)g * np + k] = bad || m == 0 ? qnan : (m & 1) ? (0.0 + at(m / 2)) / 1.0 : ((0.0 + at(m / 2 - 1)) + at(m / 2)) / 2.0;
    for (int p = 0; p < nq; ++p) o_quant[((size_t)p * G + g) * np + k] = bad || m == 0 ? qnan : stats_quantile(m, probs[p], at);
}

__global__ __launch_bounds__(STATS_WG) void k_group_small(const double* __restrict__ col, long long Mtot, const int* __restrict__ sgrp,
                                                          const long long* __restrict__ G0, const long long* __restrict__ gm, int G, int k0,
                                                          int np, const int* __restrict__ gnan, const double* __restrict__ probs, int nq,
                                                          double* __restrict__ o_median, double* __restrict__ o_quant) {
    extern __shared__ __align__(16) double sx[];   // STATS_LDS_N keys
    unsigned long long* sk = (unsigned long long*)sx;
    const int g = sgrp[blockIdx.x], kk = blockIdx.y, k = k0 + kk;
    const int m = (int)gm[g];
    const bool bad = gnan[(size_t)g * np + k] != 0;
    if (!bad && m > 0) {
        const double* x = col + (size_t)kk * Mtot + G0[g];
        stats_sort(sk, m, [&](int i) { return x[i]; });
    }
    if (threadIdx.x == 0)
        group_order_out((long long)m, bad, [&](long long i) { return stats_unkey(sk[i]); }, g, k, G, np, probs, nq, o_median, o_quant);
}

// digit d of the radix select: its shift and width in the key, and the mask of the digits above it
__device__ __forceinline__ void group_digit(int d, int& shift, int& width, unsigned long long& known) {
    shift = d < 5 ? 53 - 11 * d : 0;
    width = d < 5 ? 11 : 9;
    known = d == 0 ? 0ull : ~0ull << (shift + width);
}

// columns w = wi x kb + kk: wide group wgrp[wi], parameter k0 + kk; ranks r < R of each (rem < 0: an unused slot).  A launch counts the
// columns w0 + blockIdx.x into ghist [gridDim.x][R][GROUP_BINS].
__global__ __launch_bounds__(STATS_WG) void k_group_hist(const double* __restrict__ col, long long Mtot, const int* __restrict__ wgrp,
                                                         const long long* __restrict__ G0, const long long* __restrict__ gm, int kb, int R,
                                                         int d, int w0, const long long* __restrict__ rem,
                                                         const unsigned long long* __restrict__ pre, unsigned long long* __restrict__ ghist) {
    __shared__ int hist[GROUP_RB][GROUP_BINS];
    const int w = w0 + blockIdx.x, wi = w / kb, kk = w - wi * kb, g = wgrp[wi], tid = threadIdx.x;
    const int r0 = blockIdx.z * GROUP_RB, nr = min(GROUP_RB, R - r0);
    const double* x = col + (size_t)kk * Mtot + G0[g];
    const long long m = gm[g];
    int shift, width;
    unsigned long long known;
    group_digit(d, shift, width, known);
    const unsigned dmask = (1u << width) - 1u;
    unsigned long long p[GROUP_RB];
    bool on[GROUP_RB];
    for (int r = 0; r < GROUP_RB; ++r) {
        on[r] = r < nr && rem[(size_t)w * R + r0 + r] >= 0;
        p[r] = on[r] ? pre[(size_t)w * R + r0 + r] : 0ull;
    }
    for (int i = tid; i < GROUP_RB * GROUP_BINS; i += STATS_WG) (&hist[0][0])[i] = 0;
    __syncthreads();
    for (long long i = (long long)blockIdx.y * STATS_WG + tid; i < m; i += (long long)gridDim.y * STATS_WG) {
        const unsigned long long key = stats_key(x[i]);
        const int bin = (int)((key >> shift) & dmask);
        for (int r = 0; r < GROUP_RB; ++r)
            if (on[r] && (key & known) == p[r]) atomicAdd(&hist[r][bin], 1);
    }
    __syncthreads();
    for (int r = 0; r < nr; ++r) {
        unsigned long long* gh = ghist + ((size_t)blockIdx.x * R + r0 + r) * GROUP_BINS;
        for (int b = tid; b < GROUP_BINS; b += STATS_WG)
            if (hist[r][b]) atomicAdd(&gh[b], (unsigned long long)hist[r][b]);
    }
}

// (column, rank) e0 + blockIdx.x, its histogram at ghist [blockIdx.x]
__global__ __launch_bounds__(STATS_WG) void k_group_pick(int d, int e0, unsigned long long* __restrict__ ghist, long long* __restrict__ rem,
                                                         unsigned long long* __restrict__ pre) {
    __shared__ unsigned long long part[STATS_WG];
    __shared__ long long res[2];
    const int e = e0 + blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const long long rank = rem[e];
    if (rank < 0) return;
    int shift, width;
    unsigned long long known;
    group_digit(d, shift, width, known);
    unsigned long long* hist = ghist + (size_t)blockIdx.x * GROUP_BINS;
    unsigned long long s8 = 0;
    for (int j = 0; j < 8; ++j) s8 += hist[tid * 8 + j];
    part[tid] = s8;
    if (tid == 0) { res[0] = 0; res[1] = 0; }
    __syncthreads();
    if (tid < 64) {   // wave 0: inclusive scan of the 256 partial sums, 4 per lane (stats_select's search, 64-bit counts)
        const unsigned long long a0 = part[4 * lane], a1 = part[4 * lane + 1], a2 = part[4 * lane + 2], a3 = part[4 * lane + 3];
        const unsigned long long own = a0 + a1 + a2 + a3;
        unsigned long long inc = own;
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long y = __shfl_up(inc, o, 64);
            if (lane >= o) inc += y;
        }
        unsigned long long before = inc - own;
        const unsigned long long ur = (unsigned long long)rank;
        if (ur >= before && ur < inc) {   // exactly one lane
            int q = 4 * lane;
            if (ur >= before + a0) {
                before += a0; ++q;
                if (ur >= before + a1) {
                    before += a1; ++q;
                    if (ur >= before + a2) { before += a2; ++q; }
                }
            }
            int bin = q * 8;
            while (ur >= before + hist[bin]) { before += hist[bin]; ++bin; }
            res[0] = bin;
            res[1] = (long long)(ur - before);
        }
    }
    __syncthreads();
    for (int j = 0; j < 8; ++j) hist[tid * 8 + j] = 0;   // zero again for the next digit (every read of it is done)
    if (tid == 0) {
        pre[e] |= (unsigned long long)res[0] << shift;
        rem[e] = res[1];
    }
}

// one lane per long column w < nw: the outputs from the selected keys pre[w][r] of the ranks rk[wi][r]
__global__ void k_group_finish(int nw, const int* __restrict__ wgrp, const long long* __restrict__ gm, int G, int k0, int kb, int np, int R,
                               const long long* __restrict__ rk, const unsigned long long* __restrict__ pre, const int* __restrict__ gnan,
                               const double* __restrict__ probs, int nq, double* __restrict__ o_median, double* __restrict__ o_quant) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nw) return;
    const int wi = w / kb, kk = w - wi * kb, g = wgrp[wi], k = k0 + kk;
    auto at = [&](long long i) {
        for (int r = 0; r < R; ++r)
            if (rk[(size_t)wi * R + r] == i) return stats_unkey(pre[(size_t)w * R + r]);
        return __longlong_as_double(0x7ff8000000000000ll);   // (every rank the outputs read was selected)
    };
    group_order_out(gm[g], gnan[(size_t)g * np + k] != 0, at, g, k, G, np, probs, nq, o_median, o_quant);
}

// one lane per (group, pair j >= k): cov[g][j][k] = cov[g][k][j] = (sum of the group's chunk sums in order) / (m - 1); m < 2: NaN
__global__ void k_group_cov(const double* __restrict__ csum2, int NC, const int* __restrict__ gch0, const long long* __restrict__ gm, int G,
                            int np, double* __restrict__ o_cov) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x, npp = np * (np + 1) / 2;
    if (e >= G * npp) return;
    const int g = e / npp;
    int q = e - g * npp, j = 0;
    while (q > j) { q -= j + 1; ++j; }
    const int k = q;
    double S = 0.0;
    for (int ch = gch0[g]; ch < gch0[g + 1]; ++ch) S = S + csum2[((size_t)j * np + k) * NC + ch];
    const long long m = gm[g];
    const double v = m < 2 ? __longlong_as_double(0x7ff8000000000000ll) : S / (double)(m - 1);
    o_cov[((size_t)g * np + j) * np + k] = v;
    o_cov[((size_t)g * np + k) * np + j] = v;
}
