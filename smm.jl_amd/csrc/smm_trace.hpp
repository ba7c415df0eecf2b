// the population per iteration on the device (smm_get_trace, include/smmhip.h) — part of libsmmhip (included by smmhip.hip inside its
// anonymous namespace after smm_hist.hpp; gfx950 device code).  Reads the history records hrec [T][N][HW] (smm_params.hpp: H_*) and nothing
// else; writes only the scratch and result buffers of the call.  The other reducers collapse the iterations of a window per chain or
// group; these collapse the member chains of a group per kept iteration.  mem [M]: the members of every group, group by group in
// ascending local index (gmem0: the CSR offsets), as smm_get_histogram lists them.
//
//   k_trace_state  : (select 2) one workgroup per member walks the member's state rows from the batch's first kept iteration to its
//                    last (state_walk, smm_window.hpp); the kept rows' a(t) (-1: none) go to tab [kept iteration][member].
//   k_trace_gather : one workgroup per (kept iteration, group), TRACE_KMAX series of the series batch per blockIdx.y, walks the group's
//                    members 256 at a time (lane = member): the row each member contributes and its rank among the selected ones (block_rank,
//                    smm_window.hpp, as k_stats_gather ranks along time); then the threads read the
//                    block's (member, series) pairs, the series consecutive across lanes (a record's fields are contiguous), into the
//                    contiguous column col [kept iteration][series][M] at the group's offset + rank.  The first workgroup of a (kept
//                    iteration, group) in the first series batch also counts the members selected, accepted, exchanged and failed
//                    at row t and finds the best value among them (stats_better keyed by the position in the member list).
//   k_trace_column : one workgroup per column: mean and variance by the pairwise contract (pw_sum, smm_stats.hpp: the second sum is of
//                    (x - mu) (x - mu)), then the order statistics as k_stats_column finds them — a bitonic sort of the keys in LDS
//                    when the column has <= 8192 members, the exact radix select from global memory above that.
#pragma once

constexpr int TRACE_WG = STATS_WG;   // lanes of every kernel; also the members (rows) of one block
constexpr int TRACE_KMAX = 64;       // series of one k_trace_gather workgroup

// the field of a history record that series s reads: parameter s, the objective value at s == np, simulated moment s - np - 1 behind it
__device__ __forceinline__ int trace_field(int s, int np) { return s < np ? H_PARAMS + s : s == np ? H_VALUE : H_PARAMS + s - 1; }

// grid (M).  Rows tb .. tb + (nk - 1) stride; tab [nk][Me]
__global__ __launch_bounds__(TRACE_WG) void k_trace_state(const double* __restrict__ hrec, int N, int HW, const int* __restrict__ mem, int Me,
                                                          int tb, int nk, int stride, int* __restrict__ tab) {
    __shared__ int wred[TRACE_WG / 64];
    const int p = xcd_chain(blockIdx.x, gridDim.x), c = mem[p];
    state_walk(hrec, N, HW, c, tb, (nk - 1) * stride + 1, wred, [&](int r, int a, bool) {
        if (r % stride == 0) tab[(size_t)(r / stride) * Me + p] = a;
    });
}

// grid (nk G, max(1, ceil(sb / TRACE_KMAX))).  Kept iteration il of the batch is row tb + il stride; series [s0, s0 + sb) to col
// [nk][sb][M]; first != 0: the counts and the best of the rows go to o_* [nk][G]
__global__ __launch_bounds__(TRACE_WG) void k_trace_gather(const double* __restrict__ hrec, int N, int HW, int np, const int* __restrict__ mem,
                                                           const int* __restrict__ gmem0, int G, int M, int Me, int chain0, int tb, int stride,
                                                           int sel, const int* __restrict__ tab, int s0, int sb, int first,
                                                           double* __restrict__ col, int* __restrict__ o_count, int* __restrict__ o_nacc,
                                                           int* __restrict__ o_nex, int* __restrict__ o_nfail, double* __restrict__ o_bestv,
                                                           int* __restrict__ o_bestc) {
    __shared__ int rows[TRACE_WG], posn[TRACE_WG], cidx[TRACE_WG];
    __shared__ int wtot[TRACE_WG / 64], wbi[TRACE_WG / 64];
    __shared__ double wbv[TRACE_WG / 64];
    const int b = xcd_chain(blockIdx.x, gridDim.x), il = b / G, g = b - il * G;
    const int tid = threadIdx.x;
    const int t = tb + il * stride;
    const int m0 = gmem0[g], mg = gmem0[g + 1] - m0;
    const int k0 = blockIdx.y * TRACE_KMAX, kn = min(TRACE_KMAX, sb - k0);
    const int P = max(kn, 1), R = TRACE_WG / P, rr0 = tid / P, kk = tid - rr0 * P;
    const int field = trace_field(s0 + k0 + kk, np);
    const bool head = first != 0 && blockIdx.y == 0;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    int base = 0, nacc = 0, nex = 0, nfail = 0, bi = -1;
    double bv = 0.0;
    for (int j0 = 0; j0 < mg; j0 += TRACE_WG) {
        const int j = j0 + tid;
        const bool valid = j < mg;
        const int c = valid ? mem[m0 + j] : 0;
        const double* h = hrec + ((size_t)t * N + c) * HW;
        const double acc = valid && (sel == 1 || head) ? h[H_ACC] : 0.0;
        const bool take = valid && (sel != 1 || acc != 0.0);
        if (head && valid) {
            const double ex = h[H_EXCH], v = h[H_VALUE];
            if (ex != 0.0) ++nex;
            else if (acc != 0.0) ++nacc;
            if (h[H_STATUS] < 0.0) ++nfail;
            if (stats_better(v, j, bv, bi)) { bv = v; bi = j; }
        }
        posn[tid] = block_rank<int, false>(take, wtot, base);   // (the barrier behind rows[] closes it)
        rows[tid] = !take ? -2 : sel == 2 ? tab[(size_t)il * Me + m0 + j] : t;   // (-1: no state, a NaN; -2: not selected)
        cidx[tid] = c;
        __syncthreads();
        if (kn > 0 && rr0 < R) {
            const int nb = min(TRACE_WG, mg - j0);
            double* o = col + ((size_t)il * sb + k0 + kk) * M + m0;
            for (int r = rr0; r < nb; r += R) {
                const int src = rows[r];
                if (src == -2) continue;
                o[posn[r]] = src < 0 ? qnan : hrec[((size_t)src * N + cidx[r]) * HW + field];
            }
        }
        __syncthreads();
    }
    if (!head) return;
    nacc = block_sum(nacc, wtot);
    nex = block_sum(nex, wtot);
    nfail = block_sum(nfail, wtot);
    block_best(bv, bi, wbv, wbi, stats_better);
    if (tid == 0) {
        o_count[b] = base;
        o_nacc[b] = nacc;
        o_nex[b] = nex;
        o_nfail[b] = nfail;
        o_bestv[b] = bi < 0 ? qnan : bv;
        o_bestc[b] = bi < 0 ? 0 : chain0 + mem[m0 + bi] + 1;   // 1-based global id; 0 for an empty group
    }
}

// grid (nk G, sb): column (kept iteration, group) blockIdx.x, series s0 + blockIdx.y, to o_* [nk][G][S] (o_quant [n_probs][..] qs apart);
// o_var, o_median may be NULL (not computed), n_probs 0
__global__ __launch_bounds__(TRACE_WG) void k_trace_column(const double* __restrict__ col, int M, const int* __restrict__ gmem0, int G, int s0,
                                                           int sb, int S, const int* __restrict__ count, const double* __restrict__ probs,
                                                           int n_probs, size_t qs, double* __restrict__ o_mean, double* __restrict__ o_var,
                                                           double* __restrict__ o_median, double* __restrict__ o_quant) {
    extern __shared__ __align__(16) double sx[];   // min(longest column, STATS_LDS_N) rounded up to a power of two
    __shared__ PwTree pt;   // (pt.flag: a NaN in the column)
    __shared__ int part[TRACE_WG], res[2];
    const int b = blockIdx.x, sl = blockIdx.y, il = b / G, g = b - il * G, tid = threadIdx.x;
    const double* x = col + ((size_t)il * sb + sl) * M + gmem0[g];
    const int m = count[b];
    const size_t at = (size_t)b * S + s0 + sl;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    if (tid == 0) pt.flag = 0;
    __syncthreads();
    const double S1 = pw_sum(m, [&](int i) { const double v = x[i]; if (v != v) pt.flag = 1; return v; }, sx, pt);
    const bool bad = pt.flag != 0 || m == 0;
    const double mu = m == 0 ? qnan : S1 / (double)m;
    double var = qnan;
    if (o_var && m >= 2) {
        const double S2 = pw_sum(m, [&](int i) { const double d = x[i] - mu; return d * d; }, sx, pt);
        var = S2 / (double)(m - 1);
    }
    if (tid == 0) {
        o_mean[at] = mu;
        if (o_var) o_var[at] = var;
    }
    if (!o_median && n_probs == 0) return;
    if (bad) {
        if (tid == 0) {
            if (o_median) o_median[at] = qnan;
            for (int p = 0; p < n_probs; ++p) o_quant[(size_t)p * qs + at] = qnan;
        }
        return;
    }
    if (m <= STATS_LDS_N) {   // sort the column's keys in LDS
        unsigned long long* sk = (unsigned long long*)sx;
        stats_sort(sk, m, [&](int i) { return x[i]; });
        if (tid == 0) {
            auto at_ = [&](int i) { return stats_unkey(sk[i]); };
            if (o_median) o_median[at] = (m & 1) ? (0.0 + at_(m / 2)) / 1.0 : ((0.0 + at_(m / 2 - 1)) + at_(m / 2)) / 2.0;
            for (int p = 0; p < n_probs; ++p) o_quant[(size_t)p * qs + at] = stats_quantile(m, probs[p], at_);
        }
        return;
    }
    // longer than the LDS: select each rank the outputs need from the column in global memory (the block walks the same ranks)
    int* hist = (int*)sx;
    int r0 = -1, r1 = -1;
    unsigned long long v0 = 0, v1 = 0;
    auto at_ = [&](int i) {
        if (i == r0) return stats_unkey(v0);
        if (i == r1) return stats_unkey(v1);
        const unsigned long long v = stats_select(x, m, i, hist, part, res);
        r1 = r0; v1 = v0; r0 = i; v0 = v;
        return stats_unkey(v);
    };
    if (o_median) {
        const double med = (m & 1) ? (0.0 + at_(m / 2)) / 1.0 : ((0.0 + at_(m / 2 - 1)) + at_(m / 2)) / 2.0;
        if (tid == 0) o_median[at] = med;
    }
    for (int p = 0; p < n_probs; ++p) {
        const double q = stats_quantile(m, probs[p], at_);
        if (tid == 0) o_quant[(size_t)p * qs + at] = q;
    }
}
