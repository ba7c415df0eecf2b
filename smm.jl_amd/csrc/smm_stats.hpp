// chain summaries on the device (smm_get_chain_stats, include/smmhip.h) — part of libsmmhip (included by smmhip.hip inside its anonymous
// namespace; gfx950 device code).  Reads the history records hrec [T][N][HW] (smm_params.hpp: H_*) and nothing else; writes only the
// scratch and result buffers of the call.
//
//   k_stats_gather : one workgroup per chain streams the chain's records of the window, 256 iterations at a time (lane = iteration), and
//                    compacts the selected draws of parameters [k0, k0 + kb) into column-major scratch col [kb][Nb][n] (position = rank
//                    of the iteration among the selected ones: block_rank, smm_window.hpp, for the draws and the exchanges at once).  In the first
//                    parameter batch also: count, findmin of value, the exchanges and the compacted non-zero partner ids pcol [Nb][n].
//   k_stats_column : one workgroup per compacted column: the mean by the pairwise contract (chunks of 8192 staged in LDS: 8 lanes per
//                    leaf of <= 128 draws, the combining tree replayed by one lane), then the order statistics — a bitonic sort of the
//                    order-preserving keys in LDS when the column has <= 8192 draws, an exact radix select (6 digits of 11/11/11/11/11/9
//                    bits, one pass over the column in L2 per digit) of every rank needed above that.  Both give the same values.
//   k_stats_mode   : one workgroup per chain: the most frequent partner (ties to the smallest id) by an LDS histogram of the partner ids,
//                    STATS_MODE_BINS ids per pass over the column.
// Shared with smm_cov.hpp and smm_diag.hpp: the pairwise-sum core (pw_leaves walks numpy's tree of a chunk once, stats_pw sums the leaves
// and replays the walk's combines, pw_sum stages the chunks through LDS; PwTree is its LDS) and the XCD chain swizzle (xcd_chain).
#pragma once

constexpr int STATS_WG = 256;
constexpr int STATS_LDS_N = 8192;       // longest column sorted in LDS (64 KB of keys); also the mean's chunk (numpy's buffer)
constexpr int STATS_LEAF_MAX = 192;     // leaves of one 8192-chunk: each has > 56 draws, so <= 146
constexpr int STATS_MODE_BINS = 16384;  // partner ids counted per pass (64 KB)

__device__ __forceinline__ unsigned long long stats_key(double x) {   // IEEE total order: -0 before +0
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return b ^ ((unsigned long long)((long long)b >> 63) | 0x8000000000000000ull);
}
__device__ __forceinline__ double stats_unkey(unsigned long long k) {
    return __longlong_as_double((long long)((k & 0x8000000000000000ull) ? (k ^ 0x8000000000000000ull) : ~k));
}

// numpy's argmin order: the first NaN, else the first minimum (index = iteration)
__device__ __forceinline__ bool stats_better(double v, int i, double bv, int bi) {
    if (bi < 0) return i >= 0;
    if (i < 0) return false;
    const bool vn = v != v, bn = bv != bv;
    if (vn || bn) return vn && (!bn || i < bi);
    return v < bv || (v == bv && i < bi);
}

// the local chain of block b of a grid of G chains: neighbouring chains on one XCD, where their records share lines
__device__ __forceinline__ int xcd_chain(int b, int G) { return (G & 7) ? b : (b & 7) * (G >> 3) + (b >> 3); }

__global__ __launch_bounds__(STATS_WG) void k_stats_gather(const double* __restrict__ hrec, int N, int HW, int t0, int n, int acc_only,
                                                           int c0, int Nb, int k0, int kb, int first, double* __restrict__ col,
                                                           int* __restrict__ pcol, int* __restrict__ o_count, int* __restrict__ o_nex,
                                                           double* __restrict__ o_bestv, int* __restrict__ o_besti) {
    __shared__ int wtot[2][STATS_WG / 64];
    __shared__ double wbv[STATS_WG / 64];
    __shared__ int wbi[STATS_WG / 64];
    const int cl = xcd_chain(blockIdx.x, gridDim.x), c = c0 + cl;
    const int tid = threadIdx.x;
    int base[2] = {0, 0};   // the selected draws and the exchanges so far
    double bv = 0.0;
    int bi = -1;
    for (int r0 = 0; r0 < n; r0 += STATS_WG) {
        const int r = r0 + tid;
        const bool valid = r < n;
        const double* h = hrec + ((size_t)(t0 + (valid ? r : 0)) * N + c) * HW;
        double v = 0.0, ex = 0.0, acc = 0.0;
        if (valid) { v = h[H_VALUE]; ex = h[H_EXCH]; acc = h[H_ACC]; }
        const bool take[2] = {valid && (!acc_only || acc != 0.0), valid && ex != 0.0};
        if (valid && stats_better(v, t0 + r, bv, bi)) { bv = v; bi = t0 + r; }
        int pos[2];
        block_rank(take, wtot, base, pos);
        if (take[0])
            for (int kk = 0; kk < kb; ++kk) col[((size_t)kk * Nb + cl) * n + (size_t)pos[0]] = h[H_PARAMS + k0 + kk];
        if (first && take[1]) pcol[(size_t)cl * n + pos[1]] = (int)ex;
    }
    if (!first) return;
    block_best(bv, bi, wbv, wbi, stats_better);
    if (tid == 0) {
        o_count[c] = base[0];
        o_nex[c] = base[1];
        o_bestv[c] = bi < 0 ? __longlong_as_double(0x7ff8000000000000ll) : bv;
        o_besti[c] = bi + 1;   // 1-based iteration; 0 for an empty window
    }
}

// The pairwise tree of numpy over one chunk of L draws (include/smmhip.h), walked depth first, left before right, by ONE lane: the leaves
// in order (offset, size), and after each leaf the number of (left + right) combines the post-order walk makes before the next leaf.
// Stack in LDS (depth <= 2 x 8 + 1).
__device__ int pw_leaves(int L, int* __restrict__ loff, int* __restrict__ lnum, int* __restrict__ lcomb, int* __restrict__ tstk) {
    int sp = 0, nl = 0, lo = 0;
    tstk[sp++] = L;
    while (sp > 0) {
        const int t = tstk[--sp];
        if (t < 0) ++lcomb[nl - 1];
        else if (t <= 128) { loff[nl] = lo; lnum[nl] = t; lcomb[nl] = 0; lo += t; ++nl; }
        else {
            int n2 = t / 2;
            n2 -= n2 % 8;
            tstk[sp++] = -1;
            tstk[sp++] = t - n2;
            tstk[sp++] = n2;
        }
    }
    return nl;
}

// the LDS of stats_pw: the tree of a chunk (leaves, their combine counts and sums, the two stacks, the leaf count) and a flag the
// caller's staging may raise
struct PwTree {
    int loff[STATS_LEAF_MAX], lnum[STATS_LEAF_MAX], lcomb[STATS_LEAF_MAX];
    double lsum[STATS_LEAF_MAX];
    int tstk[64];
    double vstk[64];
    int nl, flag;
};

// pairwise sum of x[0..L) (L <= STATS_LDS_N, in LDS); every thread of the block calls it and gets the sum (left at the bottom of the
// value stack)
__device__ double stats_pw(const double* __restrict__ x, int L, PwTree& t) {
    const int tid = threadIdx.x;
    if (tid == 0) t.nl = pw_leaves(L, t.loff, t.lnum, t.lcomb, t.tstk);
    __syncthreads();
    const int nl = t.nl;
    const int g = tid >> 3, k = tid & 7;
    for (int b0 = 0; b0 < nl; b0 += STATS_WG / 8) {   // 8 lanes per leaf: lane k holds numpy's accumulator r[k]
        const int leaf = b0 + g;
        const bool has = leaf < nl;
        const int lo = has ? t.loff[leaf] : 0, m = has ? t.lnum[leaf] : 0;
        double r = 0.0;
        if (m >= 8) {
            r = x[lo + k];
            const int m8 = m - m % 8;
            for (int i = 8; i < m8; i += 8) r = r + x[lo + i + k];
        }
        r = r + __shfl_xor(r, 1, 64);   // ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)): a butterfly (IEEE addition commutes)
        r = r + __shfl_xor(r, 2, 64);
        r = r + __shfl_xor(r, 4, 64);
        if (has && k == 0) {
            double s;
            if (m < 8) {
                s = 0.0;
                for (int i = 0; i < m; ++i) s = s + x[lo + i];
            } else {
                s = r;
                for (int i = m - m % 8; i < m; ++i) s = s + x[lo + i];
            }
            t.lsum[leaf] = s;
        }
    }
    __syncthreads();
    if (tid == 0) {   // the walk's post-order: push each leaf sum, then make its combines (pop right, pop left, push left + right)
        int sp = 0;
        for (int l = 0; l < nl; ++l) {
            t.vstk[sp++] = t.lsum[l];
            for (int q = t.lcomb[l]; q > 0; --q) {
                --sp;
                t.vstk[sp - 1] = t.vstk[sp - 1] + t.vstk[sp];
            }
        }
    }
    __syncthreads();
    return t.vstk[0];
}

// the chain-stats sum of f(0 .. L) (numpy's pairwise sum over chunks of STATS_LDS_N, include/smmhip.h): each chunk's terms staged
// through sx (LDS), then stats_pw.  Every thread of the block calls it and gets the sum.
template <class F>
__device__ double pw_sum(int L, F f, double* __restrict__ sx, PwTree& t) {
    double S = 0.0;
    for (int c8 = 0; c8 < L; c8 += STATS_LDS_N) {
        const int Lc = min(STATS_LDS_N, L - c8);
        for (int i = threadIdx.x; i < Lc; i += STATS_WG) sx[i] = f(c8 + i);
        __syncthreads();
        const double s = stats_pw(sx, Lc, t);
        S = S + s;
    }
    return S;
}

// the rank-th smallest key (0-based) of the column x[0..m) in global memory: radix select, block-wide
__device__ unsigned long long stats_select(const double* __restrict__ x, int m, int rank, int* __restrict__ hist, int* __restrict__ part,
                                           int* __restrict__ res) {
    const int tid = threadIdx.x, lane = tid & 63;
    unsigned long long prefix = 0, known = 0;
    for (int d = 0; d < 6; ++d) {
        const int shift = d < 5 ? 53 - 11 * d : 0, width = d < 5 ? 11 : 9;
        const unsigned dmask = (1u << width) - 1u;
        for (int i = tid; i < 2048; i += STATS_WG) hist[i] = 0;
        __syncthreads();
        for (int i = tid; i < m; i += STATS_WG) {
            const unsigned long long k = stats_key(x[i]);
            if ((k & known) == prefix) atomicAdd(&hist[(int)((k >> shift) & dmask)], 1);
        }
        __syncthreads();
        int s8 = 0;
        for (int j = 0; j < 8; ++j) s8 += hist[tid * 8 + j];
        part[tid] = s8;
        __syncthreads();
        if (tid < 64) {   // wave 0: inclusive scan of the 256 partial sums, 4 per lane
            const int a0 = part[4 * lane], a1 = part[4 * lane + 1], a2 = part[4 * lane + 2], a3 = part[4 * lane + 3];
            const int own = a0 + a1 + a2 + a3;
            int inc = own;
            for (int o = 1; o < 64; o <<= 1) {
                const int y = __shfl_up(inc, o, 64);
                if (lane >= o) inc += y;
            }
            int before = inc - own;
            if (rank >= before && rank < inc) {   // exactly one lane
                int q = 4 * lane;
                if (rank >= before + a0) {
                    before += a0; ++q;
                    if (rank >= before + a1) {
                        before += a1; ++q;
                        if (rank >= before + a2) { before += a2; ++q; }
                    }
                }
                int bin = q * 8;
                while (rank >= before + hist[bin]) { before += hist[bin]; ++bin; }
                res[0] = bin;
                res[1] = rank - before;
            }
        }
        __syncthreads();
        const int bin = res[0];
        rank = res[1];
        prefix |= (unsigned long long)bin << shift;
        known |= (unsigned long long)dmask << shift;
        __syncthreads();
    }
    return prefix;
}

// quantile of the sorted column by numpy's linear method (include/smmhip.h); at(i) = i-th smallest draw (I: int for a chain's
// column, long long for a pooled one)
template <class At, class I = int>
__device__ double stats_quantile(I m, double p, At at) {
    const double h = (double)(m - 1) * p;
    double a, b, g;
    if (h >= (double)(m - 1)) { a = b = at(m - 1); g = h + 1.0; }   // numpy: both indexes clipped to -1, gamma = h - (-1)
    else {
        const I j = (I)floor(h);
        a = at(j); b = at(j + 1); g = h - (double)j;
    }
    const double d = b - a;
    return g >= 0.5 ? b - d * (1.0 - g) : a + d * g;
}

// the keys of x(0 .. m) (m <= STATS_LDS_N) sorted into sk[0 .. m) in LDS by a bitonic sort (padded with ~0 to a power of two); x(i) may
// read sk[i] itself.  Every thread of the block calls it.
template <class X>
__device__ void stats_sort(unsigned long long* __restrict__ sk, int m, X x) {
    const int tid = threadIdx.x;
    int P = 2;
    while (P < m) P <<= 1;
    for (int i = tid; i < P; i += STATS_WG) sk[i] = i < m ? stats_key(x(i)) : ~0ull;
    __syncthreads();
    for (int kb = 2; kb <= P; kb <<= 1)
        for (int j = kb >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += STATS_WG) {
                const int ij = i ^ j;
                if (ij > i) {
                    const unsigned long long a = sk[i], b = sk[ij];
                    if ((a > b) == ((i & kb) == 0)) { sk[i] = b; sk[ij] = a; }
                }
            }
            __syncthreads();
        }
}

__global__ __launch_bounds__(STATS_WG) void k_stats_column(const double* __restrict__ col, int n, int N, int c0, int Nb, int k0,
                                                           const int* __restrict__ o_count, const double* __restrict__ probs, int n_probs,
                                                           int np, double* __restrict__ o_mean, double* __restrict__ o_median,
                                                           double* __restrict__ o_quant) {
    extern __shared__ __align__(16) double sx[];   // min(n, STATS_LDS_N) rounded up to a power of two
    __shared__ PwTree pt;   // (pt.flag: a NaN among the draws)
    __shared__ int part[STATS_WG], res[2];
    const int cl = blockIdx.x, kk = blockIdx.y, c = c0 + cl, k = k0 + kk, tid = threadIdx.x;
    const double* x = col + ((size_t)kk * Nb + cl) * n;
    const int m = o_count[c];
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    if (tid == 0) pt.flag = 0;
    __syncthreads();
    const double S = pw_sum(m, [&](int i) { const double v = x[i]; if (v != v) pt.flag = 1; return v; }, sx, pt);
    const bool bad = pt.flag != 0 || m == 0;
    if (bad) {
        if (tid == 0) {
            o_mean[(size_t)k * N + c] = m == 0 ? qnan : S / (double)m;
            o_median[(size_t)k * N + c] = qnan;
            for (int p = 0; p < n_probs; ++p) o_quant[((size_t)p * np + k) * N + c] = qnan;
        }
        return;
    }
    if (m <= STATS_LDS_N) {   // the column is in LDS: sort its keys there
        unsigned long long* sk = (unsigned long long*)sx;
        stats_sort(sk, m, [&](int i) { return sx[i]; });
        if (tid == 0) {
            auto at = [&](int i) { return stats_unkey(sk[i]); };
            o_mean[(size_t)k * N + c] = S / (double)m;
            o_median[(size_t)k * N + c] = (m & 1) ? (0.0 + at(m / 2)) / 1.0 : ((0.0 + at(m / 2 - 1)) + at(m / 2)) / 2.0;
            for (int p = 0; p < n_probs; ++p) o_quant[((size_t)p * np + k) * N + c] = stats_quantile(m, probs[p], at);
        }
        return;
    }
    // longer than the LDS: select each rank the outputs need from the column in global memory (the block walks the same ranks)
    int* hist = (int*)sx;
    int r0 = -1, r1 = -1;
    unsigned long long v0 = 0, v1 = 0;
    auto at = [&](int i) {
        if (i == r0) return stats_unkey(v0);
        if (i == r1) return stats_unkey(v1);
        const unsigned long long v = stats_select(x, m, i, hist, part, res);
        r1 = r0; v1 = v0; r0 = i; v0 = v;
        return stats_unkey(v);
    };
    const double med = (m & 1) ? (0.0 + at(m / 2)) / 1.0 : ((0.0 + at(m / 2 - 1)) + at(m / 2)) / 2.0;
    if (tid == 0) { o_mean[(size_t)k * N + c] = S / (double)m; o_median[(size_t)k * N + c] = med; }
    for (int p = 0; p < n_probs; ++p) {
        const double q = stats_quantile(m, probs[p], at);
        if (tid == 0) o_quant[((size_t)p * np + k) * N + c] = q;
    }
}

__global__ __launch_bounds__(STATS_WG) void k_stats_mode(const int* __restrict__ pcol, int n, int c0, int bins,
                                                         const int* __restrict__ o_nex, int* __restrict__ o_most) {
    extern __shared__ __align__(16) double smode[];
    int* hist = (int*)smode;   // bins (<= STATS_MODE_BINS) ids per pass
    __shared__ int wc[STATS_WG / 64], wid[STATS_WG / 64], wmax[STATS_WG / 64];
    const int cl = blockIdx.x, c = c0 + cl, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int* x = pcol + (size_t)cl * n;
    const int m = o_nex[c];
    int mx = 0;
    for (int i = tid; i < m; i += STATS_WG) mx = max(mx, x[i]);
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o, 64));
    if (lane == 0) wmax[w] = mx;
    __syncthreads();
    for (int q = 0; q < STATS_WG / 64; ++q) mx = max(mx, wmax[q]);
    int bc = 0, bid = 0;   // count, id: the most frequent id >= 1, ties to the smallest (np.bincount(...).argmax())
    for (int lo = 1; lo <= mx; lo += bins) {
        const int nb = min(bins, mx - lo + 1);
        for (int i = tid; i < nb; i += STATS_WG) hist[i] = 0;
        __syncthreads();
        for (int i = tid; i < m; i += STATS_WG) {
            const int id = x[i] - lo;
            if (id >= 0 && id < nb) atomicAdd(&hist[id], 1);
        }
        __syncthreads();
        for (int i = tid; i < nb; i += STATS_WG)
            if (hist[i] > bc) { bc = hist[i]; bid = lo + i; }   // a thread's ids increase: strict > keeps the smallest
        __syncthreads();
    }
    for (int o = 32; o > 0; o >>= 1) {
        const int oc = __shfl_xor(bc, o, 64), oi = __shfl_xor(bid, o, 64);
        if (oc > bc || (oc == bc && oc > 0 && oi < bid)) { bc = oc; bid = oi; }
    }
    if (lane == 0) { wc[w] = bc; wid[w] = bid; }
    __syncthreads();
    if (tid == 0) {
        for (int q = 1; q < STATS_WG / 64; ++q)
            if (wc[q] > bc || (wc[q] == bc && wc[q] > 0 && wid[q] < bid)) { bc = wc[q]; bid = wid[q]; }
        o_most[c] = bc > 0 ? bid : 0;
    }
}
