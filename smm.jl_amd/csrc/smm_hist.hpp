// histograms of the draws of groups of chains on the device (smm_get_histogram, include/smmhip.h) — part of libsmmhip (included by
// smmhip.hip inside its anonymous namespace after smm_diag.hpp; gfx950 device code).  Reads the history records hrec [T][N][HW]
// (smm_params.hpp: H_*) and nothing else; writes only the result buffer of the call.  Every count is an integer: LDS counters are u32,
// global ones u64, added with integer atomics only, so the counts do not depend on the order of additions.
//
// Every kernel takes one member chain per workgroup (mem[m0 + xcd_chain(blockIdx.x)]: the members of a batch of groups, group by group)
// and walks the chain's window HIST_WG rows at a time through hist_rows: lane = iteration picks the row it selects into LDS (select 2:
// a(t) by state_before and state_scan, smm_window.hpp); then the workgroup's threads read the block's rows as (row, column)
// pairs, the columns consecutive across lanes (a row's parameters are contiguous).
//
//   k_hist_range  : the chain's selected rows and, per parameter (64 per workgroup), the min, the max and whether a draw is not finite.
//   k_hist_edges  : one workgroup per (group, parameter): the members' ranges combined, the outer edges, the status and both edge tables
//                   (numpy's _get_outer_edges and linspace), then status 3 where the 1-D edges are not strictly increasing.
//   k_hist_count  : one workgroup per (chain, batch of kb parameters): u32 counters [kb][bins] in LDS with the edges of the +-1 corrections
//                   staged beside them; a group of one chain stores its rows, pooled groups add each non-zero bin into the group's u64
//                   counts with one atomic per bin and workgroup.  Where they do not fit (large bins), lanes add into the global
//                   counts directly and read the edges from L2.
//   k_hist_pairs  : one workgroup per (chain, batch of kp pairs): each draw's two axis indexes (an exact binary search of the edges),
//                   then the pair's cell, in LDS [kp][bins2][bins2] when it fits, else added into the global counts directly.
#pragma once

constexpr int HIST_WG = STATS_WG;            // lanes of every kernel; also the rows of one block
constexpr int HIST_KMAX = 64;                // parameters (pairs) of one workgroup
constexpr size_t HIST_LDS_BYTES = 62 << 10;  // dynamic LDS of k_hist_count / k_hist_pairs: with the static part <= 64 KiB, two per CU

__device__ __forceinline__ bool hist_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }

// the window's rows of chain c, HIST_WG at a time: rows[r] = the history row that row r of the block reads (-1: a NaN row of the state
// series, -2: not selected), then body(nb) for the nb rows of the block.  Returns this lane's count of selected rows.
template <class Body>
__device__ int hist_rows(const double* __restrict__ hrec, int N, int HW, int c, int t0, int n, int sel, int* __restrict__ rows,
                         int* __restrict__ wred, Body body) {
    const int tid = threadIdx.x;
    int carry = sel == 2 ? state_before(hrec, N, HW, c, t0, wred) : -1;
    int cnt = 0;
    for (int r0 = 0; r0 < n; r0 += HIST_WG) {
        const int r = r0 + tid, t = t0 + r;
        const bool valid = r < n;
        const bool acc = valid && sel != 0 && hrec[((size_t)t * N + c) * HW + H_ACC] != 0.0;
        int src;
        if (sel == 2) {
            const int a = state_scan(acc ? t : -1, carry, wred);
            src = valid ? a : -2;
        } else {
            src = valid && (sel == 0 || acc) ? t : -2;
        }
        rows[tid] = src;
        cnt += src != -2;
        __syncthreads();
        body(min(HIST_WG, n - r0));
        __syncthreads();
    }
    return cnt;
}

// numpy's uniform-bins index of x (include/smmhip.h, 1-D), -1 when x is dropped; e: the bins + 1 edges
__device__ __forceinline__ int hist_bin(double x, double lo, double delta, int bins, const double* e) {
    if (!(x >= lo && x <= e[bins])) return -1;
    const double f = ((x - lo) / delta) * (double)bins;
    int i = (int)f;
    if (i == bins) i = bins - 1;
    if (x < e[i]) i = i - 1;
    if (i < 0) return -1;   // (x >= lo = e[0]: not reached; keeps the reads in bounds)
    if (x >= e[i + 1] && i != bins - 1) i = i + 1;
    return i;
}

// numpy's histogramdd index of x on one axis of B cells, -1 outside: searchsorted(e, x, 'right'), minus one on the last edge
__device__ __forceinline__ int hist_axis(double x, const double* e, int B) {
    if (x != x) return -1;
    int a = 0, b = B + 1;   // the first i with e[i] > x
    while (a < b) {
        const int m = (a + b) >> 1;
        if (e[m] <= x) a = m + 1;
        else b = m;
    }
    if (x == e[B]) a = a - 1;
    return a >= 1 && a <= B ? a - 1 : -1;
}

// grid (members, ceil(np / HIST_KMAX)), or (members, 1) with cmin == NULL: the count only
__global__ __launch_bounds__(HIST_WG) void k_hist_range(const double* __restrict__ hrec, int N, int HW, int t0, int n, int sel,
                                                        const int* __restrict__ mem, int m0, int np, int* __restrict__ o_cnt,
                                                        double* __restrict__ cmin, double* __restrict__ cmax, int* __restrict__ cbad) {
    __shared__ int rows[HIST_WG];
    __shared__ int wred[HIST_WG / 64];
    __shared__ double smn[HIST_WG], smx[HIST_WG];
    __shared__ int sbad[HIST_WG];
    const int c = mem[m0 + xcd_chain(blockIdx.x, gridDim.x)], tid = threadIdx.x;
    const int k0 = blockIdx.y * HIST_KMAX, kb = cmin ? min(HIST_KMAX, np - k0) : 1;
    const int P = kb, R = HIST_WG / P, rr0 = tid / P, kk = tid - rr0 * P;
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    double mn = inf, mx = -inf;
    int bad = 0;
    const int cnt = hist_rows(hrec, N, HW, c, t0, n, sel, rows, wred, [&](int nb) {
        if (!cmin || rr0 >= R) return;
        for (int r = rr0; r < nb; r += R) {
            const int src = rows[r];
            if (src == -2) continue;
            if (src == -1) { bad = 1; continue; }
            const double x = hrec[((size_t)src * N + c) * HW + H_PARAMS + k0 + kk];
            if (!hist_finite(x)) { bad = 1; continue; }
            if (x < mn) mn = x;
            if (x > mx) mx = x;
        }
    });
    const int total = block_sum(cnt, wred);
    if (blockIdx.y == 0 && tid == 0) o_cnt[c] = total;
    if (!cmin) return;
    smn[tid] = mn; smx[tid] = mx; sbad[tid] = bad;
    __syncthreads();
    if (tid < P) {
        for (int r = 1; r < R; ++r) {
            const int q = r * P + tid;
            if (smn[q] < mn) mn = smn[q];
            if (smx[q] > mx) mx = smx[q];
            bad |= sbad[q];
        }
        const size_t at = (size_t)c * np + k0 + tid;
        cmin[at] = mn; cmax[at] = mx; cbad[at] = bad;
    }
}

// grid (groups of the batch, np).  rng [np][2] given, or the members' ranges (cmin, cmax, cbad of chains with o_cnt > 0).  Writes lo, hi,
// status [G][np] at group g0 + blockIdx.x, and the batch's edges [gb][np][bins + 1], edges2 [gb][np][bins2 + 1] (NULL: none)
__global__ __launch_bounds__(HIST_WG) void k_hist_edges(const int* __restrict__ gmem0, const int* __restrict__ mem, int g0, int np,
                                                        const int* __restrict__ cnt, const double* __restrict__ cmin,
                                                        const double* __restrict__ cmax, const int* __restrict__ cbad,
                                                        const double* __restrict__ rng, int bins, int bins2, double* __restrict__ o_lo,
                                                        double* __restrict__ o_hi, int* __restrict__ o_st, double* __restrict__ edges,
                                                        double* __restrict__ edges2) {
    __shared__ double smn[HIST_WG], smx[HIST_WG];
    __shared__ int sany[HIST_WG], sbad[HIST_WG];
    __shared__ double slo, shi;
    __shared__ int sst;
    const int gl = blockIdx.x, g = g0 + gl, k = blockIdx.y, tid = threadIdx.x;
    const double inf = __longlong_as_double(0x7ff0000000000000ll), qnan = __longlong_as_double(0x7ff8000000000000ll);
    double mn = inf, mx = -inf;
    int any = 0, bad = 0;
    if (!rng)
        for (int i = gmem0[g] + tid; i < gmem0[g + 1]; i += HIST_WG) {
            const int c = mem[i];
            if (cnt[c] == 0) continue;
            const size_t at = (size_t)c * np + k;
            any = 1;
            bad |= cbad[at];
            if (cmin[at] < mn) mn = cmin[at];
            if (cmax[at] > mx) mx = cmax[at];
        }
    smn[tid] = mn; smx[tid] = mx; sany[tid] = any; sbad[tid] = bad;
    __syncthreads();
    if (tid == 0) {
        for (int q = 1; q < HIST_WG; ++q) {
            if (smn[q] < mn) mn = smn[q];
            if (smx[q] > mx) mx = smx[q];
            any |= sany[q]; bad |= sbad[q];
        }
        double lo, hi;
        int st = 0;
        if (rng) { lo = rng[2 * k]; hi = rng[2 * k + 1]; }
        else if (!any) { lo = 0.0; hi = 1.0; }
        else if (bad) { lo = qnan; hi = qnan; st = 1; }
        else { lo = mn; hi = mx; }
        if (st == 0) {
            if (lo == hi) { lo = lo - 0.5; hi = hi + 0.5; }
            if (!hist_finite(hi - lo)) st = 2;
        }
        slo = lo; shi = hi; sst = st;
    }
    __syncthreads();
    const double lo = slo, hi = shi, delta = hi - lo;
    const int st = sst;
    auto table = [&](double* e, int b) {
        const double step = delta / (double)b;
        for (int i = tid; i <= b; i += HIST_WG)
            e[i] = st != 0 ? qnan : i == b ? hi : step != 0.0 ? (double)i * step + lo : ((double)i / (double)b) * delta + lo;
    };
    double* e = edges + ((size_t)gl * np + k) * (bins + 1);
    table(e, bins);
    if (edges2) table(edges2 + ((size_t)gl * np + k) * (bins2 + 1), bins2);
    __syncthreads();
    int rep = 0;   // the 1-D edges not strictly increasing (numpy: "Too many bins for data range")
    if (st == 0)
        for (int i = tid; i < bins; i += HIST_WG) rep |= !(e[i] < e[i + 1]);
    sany[tid] = rep;
    __syncthreads();
    if (tid == 0) {
        for (int q = 1; q < HIST_WG; ++q) rep |= sany[q];
        const size_t at = (size_t)g * np + k;
        o_lo[at] = lo; o_hi[at] = hi; o_st[at] = st == 0 && rep ? 3 : st;
    }
}

// grid (members of the batch, ceil(np / kb)); lds != 0: counters and edges in the dynamic LDS (kb (12 bins + 8) bytes), else the
// global counts and edges.  single[gl]: the group has one member (its counts are stored, not added); hist [gb][np][bins] zeroed
__global__ __launch_bounds__(HIST_WG) void k_hist_count(const double* __restrict__ hrec, int N, int HW, int t0, int n, int sel,
                                                        const int* __restrict__ mem, const int* __restrict__ gid, const int* __restrict__ gmem0,
                                                        int m0, int g0, int np, int kb, int bins, int lds, const double* __restrict__ lo,
                                                        const double* __restrict__ hi, const int* __restrict__ st, const double* __restrict__ edges,
                                                        unsigned long long* __restrict__ hist) {
    extern __shared__ __align__(16) double lds_e[];   // [kb][bins + 1] edges, then [kb][bins] u32 counters
    __shared__ int rows[HIST_WG];
    __shared__ int wred[HIST_WG / 64];
    __shared__ double slo[HIST_KMAX], sdel[HIST_KMAX];
    __shared__ int sok[HIST_KMAX];
    const int c = mem[m0 + xcd_chain(blockIdx.x, gridDim.x)], tid = threadIdx.x;
    const int gl = gid[c] - g0, k0 = blockIdx.y * kb, kn = min(kb, np - k0);
    const bool single = gmem0[gl + g0 + 1] - gmem0[gl + g0] == 1;
    const double* ge = edges + ((size_t)gl * np + k0) * (bins + 1);
    unsigned long long* gh = hist + ((size_t)gl * np + k0) * bins;
    unsigned* cntr = (unsigned*)(lds_e + (size_t)kn * (bins + 1));
    if (tid < kn) {
        const size_t at = (size_t)(gl + g0) * np + k0 + tid;
        slo[tid] = lo[at];
        sdel[tid] = hi[at] - lo[at];
        sok[tid] = st[at] == 0;
    }
    if (lds) {
        for (int i = tid; i < kn * (bins + 1); i += HIST_WG) lds_e[i] = ge[i];
        for (int i = tid; i < kn * bins; i += HIST_WG) cntr[i] = 0u;
    }
    __syncthreads();
    const double* e = lds ? lds_e : ge;
    const int P = kn, R = HIST_WG / P, rr0 = tid / P, kk0 = tid - rr0 * P;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    hist_rows(hrec, N, HW, c, t0, n, sel, rows, wred, [&](int nb) {
        if (rr0 >= R) return;
        for (int r = rr0; r < nb; r += R) {
            const int src = rows[r];
            if (src == -2) continue;
            const double* h = src >= 0 ? hrec + ((size_t)src * N + c) * HW + H_PARAMS + k0 : nullptr;
            for (int kk = kk0; kk < kn; kk += P) {
                if (!sok[kk]) continue;
                const double x = h ? h[kk] : qnan;
                const int b = hist_bin(x, slo[kk], sdel[kk], bins, e + (size_t)kk * (bins + 1));
                if (b < 0) continue;
                if (lds) atomicAdd(&cntr[(size_t)kk * bins + b], 1u);
                else atomicAdd(&gh[(size_t)kk * bins + b], 1ull);
            }
        }
    });
    if (!lds) return;
    for (int i = tid; i < kn * bins; i += HIST_WG) {
        const unsigned v = cntr[i];
        if (single) gh[i] = v;
        else if (v) atomicAdd(&gh[i], (unsigned long long)v);
    }
}

// grid (members of the batch, ceil(n_pairs / kp)); lds != 0: the pairs' edges and cells in the dynamic LDS (kp (16 (bins2 + 1) +
// 4 bins2 bins2) bytes), else the global ones.  hist2 [gb][n_pairs][bins2][bins2] zeroed
__global__ __launch_bounds__(HIST_WG) void k_hist_pairs(const double* __restrict__ hrec, int N, int HW, int t0, int n, int sel,
                                                        const int* __restrict__ mem, const int* __restrict__ gid, const int* __restrict__ gmem0,
                                                        int m0, int g0, int np, const int* __restrict__ pairs, int n_pairs, int kp, int B,
                                                        int lds, const int* __restrict__ st, const double* __restrict__ edges2,
                                                        unsigned long long* __restrict__ hist2) {
    extern __shared__ __align__(16) double lds_e[];   // [kp][2][B + 1] edges, then [kp][B][B] u32 cells
    __shared__ int rows[HIST_WG];
    __shared__ int wred[HIST_WG / 64];
    __shared__ int spa[HIST_KMAX], spb[HIST_KMAX], sok[HIST_KMAX];
    const int c = mem[m0 + xcd_chain(blockIdx.x, gridDim.x)], tid = threadIdx.x;
    const int gl = gid[c] - g0, p0 = blockIdx.y * kp, pn = min(kp, n_pairs - p0);
    const bool single = gmem0[gl + g0 + 1] - gmem0[gl + g0] == 1;
    const size_t BB = (size_t)B * B;
    const double* ge = edges2 + (size_t)gl * np * (B + 1);
    unsigned long long* gh = hist2 + ((size_t)gl * n_pairs + p0) * BB;
    unsigned* cells = (unsigned*)(lds_e + (size_t)pn * 2 * (B + 1));
    if (tid < pn) {
        const int a = pairs[2 * (p0 + tid)], b = pairs[2 * (p0 + tid) + 1];
        const size_t at = (size_t)(gl + g0) * np;
        spa[tid] = a; spb[tid] = b;
        sok[tid] = (st[at + a] == 0 || st[at + a] == 3) && (st[at + b] == 0 || st[at + b] == 3);
    }
    __syncthreads();
    if (lds) {
        for (int i = tid; i < pn * 2 * (B + 1); i += HIST_WG) {
            const int p = i / (2 * (B + 1)), s = i - p * 2 * (B + 1), ax = s / (B + 1), j = s - ax * (B + 1);
            lds_e[i] = ge[(size_t)(ax ? spb[p] : spa[p]) * (B + 1) + j];
        }
        for (size_t i = tid; i < (size_t)pn * BB; i += HIST_WG) cells[i] = 0u;
    }
    __syncthreads();
    const int P = min(pn, HIST_KMAX), R = HIST_WG / P, rr0 = tid / P, pp0 = tid - rr0 * P;
    hist_rows(hrec, N, HW, c, t0, n, sel, rows, wred, [&](int nb) {
        if (rr0 >= R) return;
        for (int r = rr0; r < nb; r += R) {
            const int src = rows[r];
            if (src < 0) continue;   // (-1: a NaN row, in no cell)
            const double* h = hrec + ((size_t)src * N + c) * HW + H_PARAMS;
            for (int p = pp0; p < pn; p += P) {
                if (!sok[p]) continue;
                const double* ea = lds ? lds_e + (size_t)p * 2 * (B + 1) : ge + (size_t)spa[p] * (B + 1);
                const double* eb = lds ? ea + (B + 1) : ge + (size_t)spb[p] * (B + 1);
                const int i = hist_axis(h[spa[p]], ea, B);
                if (i < 0) continue;
                const int j = hist_axis(h[spb[p]], eb, B);
                if (j < 0) continue;
                if (lds) atomicAdd(&cells[(size_t)p * BB + (size_t)i * B + j], 1u);
                else atomicAdd(&gh[(size_t)p * BB + (size_t)i * B + j], 1ull);
            }
        }
    });
    if (!lds) return;
    for (size_t i = tid; i < (size_t)pn * BB; i += HIST_WG) {
        const unsigned v = cells[i];
        if (single) gh[i] = v;
        else if (v) atomicAdd(&gh[i], (unsigned long long)v);
    }
}
