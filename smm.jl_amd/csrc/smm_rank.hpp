// rank-normalised split R-hat, bulk / tail / mean ESS and rank histograms of groups of chains (smm_get_rank_diag, include/smmhip.h) —
// part of libsmmhip (included by smmhip.hip inside its anonymous namespace after smm_trace.hpp; gfx950 device code).  Reads the history
// records hrec [T][N][HW] (smm_params.hpp: H_*) and nothing else; writes only the scratch and result buffers of the call.
//
// A batch is the groups [g0, g0 + gn) and the series [s0, s0 + sb).  Member i of group g gives the split chains 2 i (x[0:h]) and 2 i + 1
// (x[n-h:n]); the batch's split chains are numbered qb = 0 .. mtot - 1 in group, member, half order (q0 + qb over the whole call), so
// that chain qb of series sl lies at [sl][qb h .. qb h + h) of every value array [sb][Mtot], Mtot = mtot h, and group g's pooled column
// (M = 2 k h values) starts at (2 gm0[g] - q0) h.  Cells are numbered g S + s over the whole call.
//
//   k_rank_gather     : one workgroup per member chain: the state series (state_walk, smm_window.hpp) into split-chain layout X.
//   k_rank_keys       : the order keys (stats_key, -0 taken as +0) of x, or of |x - med| (fold), with the pooled index; a non-finite x
//                       raises the cell's flag.
//   k_rank_sort_small : one workgroup per column of <= RANK_SMALL values: the 8 passes of an LSD radix sort, 8 bits each, between the two
//                       key / index buffers.  A pass: each wave counts the digits of its own segment into its LDS histogram (integer
//                       atomics), the 4 x 256 counts are scanned digit-major, then each wave scatters its segment 64 values at a time
//                       in order — a value's place among its wave's equal digits by ballots —, which keeps every pass stable.
//   k_rank_count / k_rank_scan / k_rank_scatter : the same pass for a longer column spread over up to RANK_NBLK workgroups: the
//                       segments' counts to a global table [256][segments], one workgroup's digit-major scan of it, the scatter.
//                       The three sort kernels and k_rank_sort_small also sort the columns of a plain (offset, length) table
//                       (RankBatch::tab_off / tab_len: smm_get_density's long columns); rank_sort_columns launches them for both.
//   k_rank_ties       : rank2 = 2 L + E + 1 of every sorted position from the ends of its tie run (its neighbours where the run is the
//                       value alone, else a binary search of the sorted keys), written back by pooled index.
//   k_rank_order      : one lane per column: median, q05 and q95 read from the sorted keys (the chain-stats order statistics).
//   k_rank_scores     : one workgroup per split chain: z = ndtri((rank2 / 2 - 0.375) / (M + 0.25)) (AS 241 PPND16 over smm_log) and, in
//                       the same pass of the unfolded ranks, the two tail indicators and the chain's binned ranks (LDS counters when
//                       n_bins <= RANK_HIST_LDS, then 64-bit global integer atomics).
//   k_rank_chain_mom  : one workgroup per (split chain, series, kind): mean and variance (pw_sum, smm_stats.hpp), then y - mean in place.
//   k_rank_cell_mom   : one lane per (cell, kind): W, var_plus, the R-hats; Geyer's state of the cell reset.
//   k_rank_acov       : a block of 256 lags of every split chain of the cells still open (diag_pw, smm_diag.hpp; lane = lag).
//   k_rank_geyer      : one workgroup per (cell, kind): lane = lag: the chains' autocovariances averaged in order by that lane, rho_t;
//                       lane 0 extends Geyer's sequence over the block's pairs and closes the cell once it is truncated.
//   k_rank_finish     : one lane per cell: tau, the ESS values, rhat_rank and the statuses.
// The kinds of series: 0 z (bulk), 1 x (mean), 2 and 3 the indicators x <= q05, x <= q95 (tail), 4 z of |x - med| (folded: moments only).
#pragma once

constexpr int RANK_WG = 256;
constexpr int RANK_SMALL = STATS_LDS_N;   // the longest column one workgroup sorts
constexpr int RANK_NBLK = 64;             // workgroups of a longer column's pass (4 segments each)
constexpr int RANK_TABLE = 256 * RANK_NBLK * 4;   // ints of a longer column's digit table
constexpr int RANK_HIST_LDS = 4096;       // bins of a chain's rank histogram counted in LDS
constexpr int RANK_KINDS = 5, RANK_ESS_KINDS = 4;

struct RankBatch {
    const int* gm0;      // [G + 1] the groups' first members
    const int* mem;      // the members' local chains
    const int* qgrp;     // the group of every split chain of the call
    const int* large;    // [G] the ordinal of a group among its batch's long columns
    int g0, gn, s0, sb, S, q0, mtot, h, n;
    long long Mtot;
    // a plain column table instead (the sort alone, for smm_get_density): column g has tab_len[g] values from tab_off[g] of its series
    const long long* tab_off = nullptr;
    const long long* tab_len = nullptr;
};
__device__ __forceinline__ long long rank_col_len(const RankBatch& b, int g) {
    return b.tab_len ? b.tab_len[g] : 2ll * (b.gm0[g + 1] - b.gm0[g]) * b.h;
}
__device__ __forceinline__ long long rank_col_off(const RankBatch& b, int g, int sl) {
    return (long long)sl * b.Mtot + (b.tab_off ? b.tab_off[g] : (long long)(2 * b.gm0[g] - b.q0) * b.h);
}

__global__ __launch_bounds__(RANK_WG) void k_rank_gather(const double* __restrict__ hrec, int N, int HW, int np, int t0, RankBatch b,
                                                         double* __restrict__ X) {
    __shared__ int wred[RANK_WG / 64];
    const int bi = blockIdx.x, c = b.mem[b.gm0[b.g0] + bi];
    state_walk(hrec, N, HW, c, t0, b.n, wred, [&](int r, int a, bool) {
        long long pos;
        if (r < b.h) pos = (long long)(2 * bi) * b.h + r;
        else if (r >= b.n - b.h) pos = (long long)(2 * bi + 1) * b.h + (r - (b.n - b.h));
        else return;   // (the middle iteration of an odd window)
        const double* hr = hrec + ((size_t)(a < 0 ? 0 : a) * N + c) * HW;
        for (int sl = 0; sl < b.sb; ++sl) {
            const int s = b.s0 + sl;
            X[(size_t)sl * b.Mtot + pos] = a < 0 ? __longlong_as_double(0x7ff8000000000000ll) : s < np ? hr[H_PARAMS + s] : hr[H_VALUE];
        }
    });
}

__global__ __launch_bounds__(RANK_WG) void k_rank_keys(RankBatch b, int fold, const double* __restrict__ X, const double* __restrict__ ord,
                                                       unsigned long long* __restrict__ K, unsigned* __restrict__ I, int* __restrict__ flag) {
    const int g = b.g0 + blockIdx.x, sl = blockIdx.y, cell = g * b.S + b.s0 + sl;
    const long long M = rank_col_len(b, g), off = rank_col_off(b, g, sl);
    const double med = fold ? ord[3 * cell] : 0.0;
    for (long long i = (long long)blockIdx.z * RANK_WG + threadIdx.x; i < M; i += (long long)gridDim.z * RANK_WG) {
        double v = X[off + i];
        if (fold) v = fabs(v - med);
        else if (!isfinite(v)) flag[cell] = 1;
        K[off + i] = stats_key(v == 0.0 ? 0.0 : v);
        I[off + i] = (unsigned)i;
    }
}

// the segment sg of nseg of a column of M values: [lo, hi), walked in `trips` tiles of 64 (the same count for every segment)
__device__ __forceinline__ void rank_segment(long long M, int nseg, int sg, long long& lo, long long& hi, int& trips) {
    const long long seg = ((M + nseg - 1) / nseg + 63) / 64 * 64;
    lo = min(M, (long long)sg * seg);
    hi = min(M, lo + seg);
    trips = (int)(seg / 64);
}

__device__ __forceinline__ void rank_count_segment(const unsigned long long* K, long long off, long long lo, long long hi, int trips,
                                                   int shift, int* hist) {
    const int lane = threadIdx.x & 63;
    for (int it = 0; it < trips; ++it) {
        const long long p = lo + (long long)it * 64 + lane;
        if (p < hi) atomicAdd(&hist[(int)((K[off + p] >> shift) & 255ull)], 1);
    }
}

// the wave's segment to its places: base [256] (LDS) holds the next place of each digit for this wave.  Every thread of the block
// calls it with its wave's segment; the tiles go in order, a value behind its wave's earlier equal digits.
__device__ __forceinline__ void rank_scatter_segment(const unsigned long long* Kin, const unsigned* Iin, unsigned long long* Kout,
                                                     unsigned* Iout, long long off, long long M, long long lo, long long hi, int trips,
                                                     int shift, int* base) {
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int it = 0; it < trips; ++it) {
        const long long p = lo + (long long)it * 64 + lane;
        const bool valid = p < hi;
        const unsigned long long key = valid ? Kin[off + p] : 0ull;
        const unsigned idx = valid ? Iin[off + p] : 0u;
        const int d = (int)((key >> shift) & 255ull);
        unsigned long long peers = __ballot(valid);
        for (int bit = 0; bit < 8; ++bit) {
            const bool on = (d >> bit) & 1;
            const unsigned long long mb = __ballot(on);
            peers &= on ? mb : ~mb;
        }
        const int rank = __popcll(peers & below), cnt = __popcll(peers);
        const int b0 = valid ? base[d] : 0;
        __syncthreads();
        const long long pos = (long long)b0 + rank;
        if (valid && pos < M) {
            Kout[off + pos] = key;
            Iout[off + pos] = idx;
            if (rank == cnt - 1) base[d] = b0 + cnt;
        }
        __syncthreads();
    }
}

// exclusive scan of tot [256] (LDS) in place, by one lane
__device__ __forceinline__ void rank_scan256(int* tot) {
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int d = 0; d < 256; ++d) { const int t = tot[d]; tot[d] = run; run += t; }
    }
    __syncthreads();
}

__global__ __launch_bounds__(RANK_WG) void k_rank_sort_small(RankBatch b, unsigned long long* KA, unsigned* IA, unsigned long long* KB,
                                                             unsigned* IB) {
    __shared__ int hist[RANK_WG / 64][256];
    __shared__ int tot[256];
    const int g = b.g0 + blockIdx.x, sl = blockIdx.y, tid = threadIdx.x, w = tid >> 6;
    const long long M = rank_col_len(b, g), off = rank_col_off(b, g, sl);
    if (M == 0 || M > RANK_SMALL) return;
    long long lo, hi;
    int trips;
    rank_segment(M, RANK_WG / 64, w, lo, hi, trips);
    for (int pass = 0; pass < 8; ++pass) {
        const unsigned long long* Kin = (pass & 1) ? KB : KA;
        const unsigned* Iin = (pass & 1) ? IB : IA;
        unsigned long long* Kout = (pass & 1) ? KA : KB;
        unsigned* Iout = (pass & 1) ? IA : IB;
        for (int q = 0; q < RANK_WG / 64; ++q) hist[q][tid] = 0;
        __syncthreads();
        rank_count_segment(Kin, off, lo, hi, trips, 8 * pass, hist[w]);
        __syncthreads();
        int cq[RANK_WG / 64], t = 0;
        for (int q = 0; q < RANK_WG / 64; ++q) { cq[q] = hist[q][tid]; t += cq[q]; }
        tot[tid] = t;
        rank_scan256(tot);
        int run = tot[tid];
        for (int q = 0; q < RANK_WG / 64; ++q) { hist[q][tid] = run; run += cq[q]; }
        __syncthreads();
        rank_scatter_segment(Kin, Iin, Kout, Iout, off, M, lo, hi, trips, 8 * pass, hist[w]);
        __syncthreads();   // (the pass's stores, before the next pass reads them)
    }
}

// a longer column: its workgroups and the table [256][nseg] of its segments' digit counts, then places
__device__ __forceinline__ int rank_nblk(long long M) { return (int)min((long long)RANK_NBLK, (M + RANK_SMALL - 1) / RANK_SMALL); }

__global__ __launch_bounds__(RANK_WG) void k_rank_count(RankBatch b, int pass, const unsigned long long* K, int* __restrict__ table) {
    __shared__ int hist[RANK_WG / 64][256];
    const int g = b.g0 + blockIdx.x, sl = blockIdx.y, tid = threadIdx.x, w = tid >> 6;
    const long long M = rank_col_len(b, g), off = rank_col_off(b, g, sl);
    if (M <= RANK_SMALL) return;
    const int nblk = rank_nblk(M), nseg = nblk * (RANK_WG / 64);
    if ((int)blockIdx.z >= nblk) return;
    int* tab = table + ((size_t)b.large[g] * b.sb + sl) * RANK_TABLE;
    long long lo, hi;
    int trips;
    const int sg0 = blockIdx.z * (RANK_WG / 64);
    rank_segment(M, nseg, sg0 + w, lo, hi, trips);
    for (int q = 0; q < RANK_WG / 64; ++q) hist[q][tid] = 0;
    __syncthreads();
    rank_count_segment(K, off, lo, hi, trips, 8 * pass, hist[w]);
    __syncthreads();
    for (int q = 0; q < RANK_WG / 64; ++q) tab[(size_t)tid * nseg + sg0 + q] = hist[q][tid];
}

__global__ __launch_bounds__(RANK_WG) void k_rank_scan(RankBatch b, int* __restrict__ table) {
    __shared__ int tot[256];
    const int g = b.g0 + blockIdx.x, sl = blockIdx.y, tid = threadIdx.x;
    const long long M = rank_col_len(b, g);
    if (M <= RANK_SMALL) return;
    const int nseg = rank_nblk(M) * (RANK_WG / 64);
    int* row = table + ((size_t)b.large[g] * b.sb + sl) * RANK_TABLE + (size_t)tid * nseg;
    int t = 0;
    for (int q = 0; q < nseg; ++q) t += row[q];
    tot[tid] = t;
    rank_scan256(tot);
    int run = tot[tid];
    for (int q = 0; q < nseg; ++q) { const int cq = row[q]; row[q] = run; run += cq; }
}

__global__ __launch_bounds__(RANK_WG) void k_rank_scatter(RankBatch b, int pass, const unsigned long long* Kin, const unsigned* Iin,
                                                          unsigned long long* Kout, unsigned* Iout, const int* __restrict__ table) {
    __shared__ int base[RANK_WG / 64][256];
    const int g = b.g0 + blockIdx.x, sl = blockIdx.y, tid = threadIdx.x, w = tid >> 6;
    const long long M = rank_col_len(b, g), off = rank_col_off(b, g, sl);
    if (M <= RANK_SMALL) return;
    const int nblk = rank_nblk(M), nseg = nblk * (RANK_WG / 64);
    if ((int)blockIdx.z >= nblk) return;
    const int* tab = table + ((size_t)b.large[g] * b.sb + sl) * RANK_TABLE;
    long long lo, hi;
    int trips;
    const int sg0 = blockIdx.z * (RANK_WG / 64);
    rank_segment(M, nseg, sg0 + w, lo, hi, trips);
    for (int q = 0; q < RANK_WG / 64; ++q) base[q][tid] = tab[(size_t)tid * nseg + sg0 + q];
    __syncthreads();
    rank_scatter_segment(Kin, Iin, Kout, Iout, off, M, lo, hi, trips, 8 * pass, base[w]);
}

__global__ __launch_bounds__(RANK_WG) void k_rank_ties(RankBatch b, const unsigned long long* __restrict__ K, const unsigned* __restrict__ I,
                                                       long long* __restrict__ R2) {
    const int g = b.g0 + blockIdx.x, sl = blockIdx.y;
    const long long M = rank_col_len(b, g), off = rank_col_off(b, g, sl);
    const unsigned long long* k = K + off;
    for (long long p = (long long)blockIdx.z * RANK_WG + threadIdx.x; p < M; p += (long long)gridDim.z * RANK_WG) {
        const unsigned long long key = k[p];
        long long L = p, U = p + 1;
        if (p > 0 && k[p - 1] == key) {   // the first position holding key in [0, p)
            long long a = 0, e = p - 1;
            while (a < e) { const long long m = (a + e) / 2; if (k[m] < key) a = m + 1; else e = m; }
            L = a;
        }
        if (p + 1 < M && k[p + 1] == key) {   // the first position past key in (p + 1, M]
            long long a = p + 2, e = M;
            while (a < e) { const long long m = (a + e) / 2; if (k[m] <= key) a = m + 1; else e = m; }
            U = a;
        }
        const long long i = I[off + p];
        if (i < M) R2[off + i] = 2 * L + (U - L) + 1;
    }
}

__global__ void k_rank_order(RankBatch b, const unsigned long long* __restrict__ K, double* __restrict__ ord) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= b.gn * b.sb) return;
    const int g = b.g0 + e / b.sb, sl = e % b.sb, cell = g * b.S + b.s0 + sl;
    const long long M = rank_col_len(b, g);
    if (M == 0) return;
    const unsigned long long* k = K + rank_col_off(b, g, sl);
    auto at = [&](long long i) { return stats_unkey(k[i]); };
    ord[3 * cell] = (M & 1) ? (0.0 + at(M / 2)) / 1.0 : ((0.0 + at(M / 2 - 1)) + at(M / 2)) / 2.0;
    ord[3 * cell + 1] = stats_quantile<decltype(at), long long>(M, 0.05, at);
    ord[3 * cell + 2] = stats_quantile<decltype(at), long long>(M, 0.95, at);
}

// Wichura's AS 241 PPND16, every operation in its order; the logarithm is the contract's smm_log (smm_rng.hpp), the root IEEE's
__device__ double rank_ndtri(const double p) {
    const double q = p - 0.5;
    if (fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        const double num = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r +
                                4.5921953931549871457e+4) * r + 1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r +
                             1.3314166789178437745e+2) * r + 3.3871328727963666080e+0) * q;
        const double den = (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r +
                                2.1213794301586595867e+4) * r + 5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r +
                             4.2313330701600911252e+1) * r + 1.0);
        return num / den;
    }
    double r = q <= 0.0 ? p : 1.0 - p;
    r = __builtin_sqrt(-smm_log(r));
    double num, den;
    if (r <= 5.0) {
        r = r - 1.6;
        num = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r +
                   1.27045825245236838258e+0) * r + 3.64784832476320460504e+0) * r + 5.76949722146069140550e+0) * r +
                4.63033784615654529590e+0) * r + 1.42343711074968357734e+0);
        den = (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r +
                   1.48103976427480074590e-1) * r + 6.89767334985100004550e-1) * r + 1.67638483018380384940e+0) * r +
                2.05319162663775882187e+0) * r + 1.0);
    } else {
        r = r - 5.0;
        num = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r +
                   2.65321895265761230930e-2) * r + 2.96560571828504891230e-1) * r + 1.78482653991729133580e+0) * r +
                5.46378491116411436990e+0) * r + 6.65790464350110377720e+0);
        den = (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r +
                   7.86869131145613259100e-4) * r + 1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r +
                5.99832206555887937690e-1) * r + 1.0);
    }
    const double x = num / den;
    return q < 0.0 ? -x : x;
}

// Y = the kinds' value arrays [RANK_KINDS][sb][Mtot] (0 z, 1 x, 2 and 3 the indicators, 4 the folded z); hist [n_bins][S][N] or NULL
__global__ __launch_bounds__(RANK_WG) void k_rank_scores(RankBatch b, int fold, const long long* __restrict__ R2, const double* __restrict__ ord,
                                                         const int* __restrict__ flag, double* __restrict__ Y, int n_bins, int N,
                                                         unsigned long long* __restrict__ hist) {
    __shared__ int lh[RANK_HIST_LDS];
    const int qb = blockIdx.x, sl = blockIdx.y, tid = threadIdx.x;
    const int qg = b.q0 + qb, g = b.qgrp[qg], s = b.s0 + sl, cell = g * b.S + s, c = b.mem[qg >> 1];
    const long long M = rank_col_len(b, g);
    const size_t E = (size_t)b.sb * b.Mtot, at0 = (size_t)sl * b.Mtot + (size_t)qb * b.h;
    const double dm = (double)M + 0.25;
    if (fold) {
        for (int i = tid; i < b.h; i += RANK_WG) Y[4 * E + at0 + i] = rank_ndtri(((double)R2[at0 + i] * 0.5 - 0.375) / dm);
        return;
    }
    const bool count = hist != nullptr && flag[cell] == 0, lds = n_bins <= RANK_HIST_LDS;
    if (count && lds)
        for (int i = tid; i < n_bins; i += RANK_WG) lh[i] = 0;
    __syncthreads();
    const double q05 = ord[3 * cell + 1], q95 = ord[3 * cell + 2];
    for (int i = tid; i < b.h; i += RANK_WG) {
        const long long r2 = R2[at0 + i];
        const double x = Y[E + at0 + i];
        Y[at0 + i] = rank_ndtri(((double)r2 * 0.5 - 0.375) / dm);
        Y[2 * E + at0 + i] = x <= q05 ? 1.0 : 0.0;
        Y[3 * E + at0 + i] = x <= q95 ? 1.0 : 0.0;
        if (count) {
            const long long bin = ((r2 - 1) * n_bins) / (2 * M);
            if (bin >= 0 && bin < n_bins) {
                if (lds) atomicAdd(&lh[(int)bin], 1);
                else atomicAdd(&hist[((size_t)bin * b.S + s) * N + c], 1ull);
            }
        }
    }
    __syncthreads();
    if (count && lds)
        for (int i = tid; i < n_bins; i += RANK_WG)
            if (lh[i]) atomicAdd(&hist[((size_t)i * b.S + s) * N + c], (unsigned long long)lh[i]);
}

// cmu, cvar [RANK_KINDS][sb][mtot]
__global__ __launch_bounds__(RANK_WG) void k_rank_chain_mom(RankBatch b, double* __restrict__ Y, double* __restrict__ cmu,
                                                            double* __restrict__ cvar) {
    extern __shared__ __align__(16) double sx[];   // min(h, STATS_LDS_N)
    __shared__ PwTree pt;
    const int qb = blockIdx.x, sl = blockIdx.y, kind = blockIdx.z, tid = threadIdx.x;
    double* y = Y + ((size_t)kind * b.sb + sl) * b.Mtot + (size_t)qb * b.h;
    const int h = b.h;
    const double mu = pw_sum(h, [&](int i) { return y[i]; }, sx, pt) / (double)h;
    const double ss = pw_sum(h, [&](int i) { const double e = y[i] - mu; return e * e; }, sx, pt);
    if (tid == 0) {
        const size_t o = ((size_t)kind * b.sb + sl) * b.mtot + qb;
        cmu[o] = mu;
        cvar[o] = ss / (double)(h - 1);
    }
    for (int i = tid; i < h; i += RANK_WG) y[i] = y[i] - mu;
}

// one leaf of numpy's pairwise tree over f(lo .. lo + m - 1) (m <= 128), and the tree over [lo, lo + len) (len <= 8192), by one lane
template <class F>
__device__ double rank_leaf(F f, int lo, int m) {
    if (m < 8) {
        double s = 0.0;
        for (int i = lo; i < lo + m; ++i) s = s + f(i);
        return s;
    }
    double r[8];
    for (int k = 0; k < 8; ++k) r[k] = f(lo + k);
    const int m8 = lo + m - m % 8;
    for (int i = lo + 8; i < m8; i += 8)
        for (int k = 0; k < 8; ++k) r[k] = r[k] + f(i + k);
    double s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (int i = m8; i < lo + m; ++i) s = s + f(i);
    return s;
}
template <int D, class F>
__device__ double rank_pw(F f, int lo, int len) {
    if constexpr (D == 0) {
        return rank_leaf(f, lo, len);
    } else {
        if (len <= 128) return rank_leaf(f, lo, len);
        int n2 = len / 2;
        n2 -= n2 % 8;
        const double lf = rank_pw<D - 1>(f, lo, n2);
        const double rt = rank_pw<D - 1>(f, lo + n2, len - n2);
        return lf + rt;
    }
}
// the chain-stats sum S of f(0 .. m), by one lane
template <class F>
__device__ double rank_S(F f, int m) {
    double S = 0.0;
    for (int c8 = 0; c8 < m; c8 += STATS_LDS_N) {
        const double p = rank_pw<7>(f, c8, min(STATS_LDS_N, m - c8));
        S = S + p;
    }
    return S;
}

// cW, cvp [RANK_KINDS][G S]; gQ, gT, gst [RANK_ESS_KINDS][G S] (gst: 1 truncated, 2 undefined)
__global__ void k_rank_cell_mom(RankBatch b, int GS, const double* __restrict__ cmu, const double* __restrict__ cvar, double* __restrict__ cW,
                                double* __restrict__ cvp, double* __restrict__ gQ, double* __restrict__ gT, int* __restrict__ gst,
                                double* __restrict__ o_rb, double* __restrict__ o_rf) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= b.gn * b.sb * RANK_KINDS) return;
    const int kind = e % RANK_KINDS, sl = (e / RANK_KINDS) % b.sb, g = b.g0 + e / (RANK_KINDS * b.sb), cell = g * b.S + b.s0 + sl;
    const int m = 2 * (b.gm0[g + 1] - b.gm0[g]);
    double W = 0.0, vp = 0.0;
    if (m > 0) {
        const size_t o = ((size_t)kind * b.sb + sl) * b.mtot + (2 * b.gm0[g] - b.q0);
        const double dm = (double)m;
        W = rank_S([&](int j) { return cvar[o + j]; }, m) / dm;
        const double mm = rank_S([&](int j) { return cmu[o + j]; }, m) / dm;
        const double v = rank_S([&](int j) { const double dv = cmu[o + j] - mm; return dv * dv; }, m) / (dm - 1.0);
        vp = (((double)b.h - 1.0) / (double)b.h) * W + v;
        if (kind == 0) o_rb[cell] = __builtin_sqrt(vp / W);
        if (kind == 4) o_rf[cell] = __builtin_sqrt(vp / W);
    }
    cW[(size_t)kind * GS + cell] = W;
    cvp[(size_t)kind * GS + cell] = vp;
    if (kind < RANK_ESS_KINDS) {
        gQ[(size_t)kind * GS + cell] = 0.0;
        gT[(size_t)kind * GS + cell] = 0.0;
        gst[(size_t)kind * GS + cell] = (m == 0 || W == 0.0 || vp == 0.0) ? 2 : 0;
    }
}

// acov [RANK_ESS_KINDS][sb][mtot][LB]: the lags kb .. kb + 255 (<= max_lag) of every split chain of a cell still open
__global__ __launch_bounds__(RANK_WG) void k_rank_acov(RankBatch b, int GS, int kb, int max_lag, int LB, const double* __restrict__ Y,
                                                       const int* __restrict__ gst, double* __restrict__ acov) {
    extern __shared__ __align__(16) double sx[];   // min(h, STATS_LDS_N)
    const int qb = blockIdx.x, sl = blockIdx.y, kind = blockIdx.z, tid = threadIdx.x;
    const int g = b.qgrp[b.q0 + qb], cell = g * b.S + b.s0 + sl, h = b.h;
    if (gst[(size_t)kind * GS + cell] != 0) return;
    const double* y = Y + ((size_t)kind * b.sb + sl) * b.Mtot + (size_t)qb * h;
    const double* d = y;
    if (h <= STATS_LDS_N) {
        for (int i = tid; i < h; i += RANK_WG) sx[i] = y[i];
        d = sx;
    }
    __syncthreads();
    const int k = kb + tid;
    if (k > max_lag || tid >= LB) return;
    const int L = h - k;
    double Sk = 0.0;
    for (int c8 = 0; c8 < L; c8 += STATS_LDS_N) {
        const double p = diag_pw<7>(d, c8, min(STATS_LDS_N, L - c8), k);
        Sk = Sk + p;
    }
    acov[(((size_t)kind * b.sb + sl) * b.mtot + qb) * LB + tid] = Sk / (double)h;
}

__global__ __launch_bounds__(RANK_WG) void k_rank_geyer(RankBatch b, int GS, int kb, int max_lag, int LB, const double* __restrict__ acov,
                                                        const double* __restrict__ cW, const double* __restrict__ cvp, double* __restrict__ gQ,
                                                        double* __restrict__ gT, int* __restrict__ gst) {
    __shared__ double srho[RANK_WG];
    const int gl = blockIdx.x / b.sb, sl = blockIdx.x % b.sb, kind = blockIdx.y, tid = threadIdx.x;
    const int g = b.g0 + gl, cell = g * b.S + b.s0 + sl;
    const size_t ci = (size_t)kind * GS + cell;
    if (gst[ci] != 0) return;
    const int m = 2 * (b.gm0[g + 1] - b.gm0[g]);
    const double W = cW[ci], vp = cvp[ci];
    const int k = kb + tid;
    double rho = 0.0;
    if (k <= max_lag && tid < LB) {
        const double* a = acov + (((size_t)kind * b.sb + sl) * b.mtot + (2 * b.gm0[g] - b.q0)) * LB + tid;
        const double A = rank_S([&](int j) { return a[(size_t)j * LB]; }, m) / (double)m;
        rho = k == 0 ? 1.0 : 1.0 - (W - A) / vp;
    }
    srho[tid] = rho;
    __syncthreads();
    if (tid == 0) {
        double Q = gQ[ci], T = gT[ci];
        bool trunc = false;
        for (int k2 = kb; !trunc && k2 + 1 <= max_lag && k2 + 1 < kb + RANK_WG; k2 += 2) {   // pair j = k2 / 2
            const double P = srho[k2 - kb] + srho[k2 - kb + 1];
            if (k2 == 0) { Q = P; T = 0.0 + Q; }
            else if (!(P > 0.0)) trunc = true;
            else { Q = P < Q ? P : Q; T = T + Q; }
        }
        gQ[ci] = Q;
        gT[ci] = T;
        if (trunc) gst[ci] = 1;
    }
}

// o_* [G][S]; o_status [4][G][S]: bulk, folded, tail, mean
__global__ void k_rank_finish(RankBatch b, int GS, const int* __restrict__ flag, const double* __restrict__ cW, const double* __restrict__ cvp,
                              const double* __restrict__ gT, const int* __restrict__ gst, double* __restrict__ o_rr, double* __restrict__ o_rb,
                              double* __restrict__ o_rf, double* __restrict__ o_eb, double* __restrict__ o_et, double* __restrict__ o_em,
                              int* __restrict__ o_status) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= b.gn * b.sb) return;
    const int g = b.g0 + e / b.sb, sl = e % b.sb, cell = g * b.S + b.s0 + sl;
    const long long M = rank_col_len(b, g);
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    if (M == 0 || flag[cell]) {
        o_rr[cell] = o_rb[cell] = o_rf[cell] = o_eb[cell] = o_et[cell] = o_em[cell] = qnan;
        for (int q = 0; q < 4; ++q) o_status[(size_t)q * GS + cell] = M == 0 ? 2 : 3;
        return;
    }
    double ess[RANK_ESS_KINDS];
    int st[RANK_ESS_KINDS];
    for (int kind = 0; kind < RANK_ESS_KINDS; ++kind) {
        const size_t ci = (size_t)kind * GS + cell;
        const double tau = -1.0 + 2.0 * gT[ci];
        const bool undef = (gst[ci] & 2) || !(tau > 0.0);
        ess[kind] = undef ? qnan : (double)M / tau;
        st[kind] = undef ? 2 : (gst[ci] & 1) ? 0 : 1;
    }
    const double rb = o_rb[cell], rf = o_rf[cell];
    o_rr[cell] = (rb != rb || rf != rf) ? qnan : rb > rf ? rb : rf;
    o_eb[cell] = ess[0];
    o_em[cell] = ess[1];
    o_et[cell] = (ess[2] != ess[2] || ess[3] != ess[3]) ? qnan : ess[2] < ess[3] ? ess[2] : ess[3];
    o_status[cell] = st[0];
    o_status[(size_t)GS + cell] = (cW[(size_t)4 * GS + cell] == 0.0 || cvp[(size_t)4 * GS + cell] == 0.0) ? 2 : 0;
    o_status[(size_t)2 * GS + cell] = max(st[2], st[3]);
    o_status[(size_t)3 * GS + cell] = st[1];
}
