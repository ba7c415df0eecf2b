// highest-density intervals, half-sample modes and Gaussian kernel densities of groups of chains on the device (smm_get_density,
// include/smmhip.h) — part of libsmmhip (included by smmhip.hip inside its anonymous namespace after smm_rank.hpp; gfx950 device code).
// Reads the packed pooled columns col [kb][Mtot] that k_group_gather wrote (smm_group.hpp: group g's column from G0[g], gm[g] rows, cut
// into chunks of STATS_LDS_N rows from its own first row) and nothing else; writes only the scratch and result buffers of the call.
// Column (g, k) of a batch of kb parameters from k0 is (g, kk), k = k0 + kk; the per-column results lie at [g][k] of [G][np] arrays.
// A long column w = wi kb + kk is column kk of the wi-th long group (wgrp[wi], its rows at off[wi], len[wi] of them).
//
//   k_dens_small     : one workgroup per short column (m < the wide minimum, so m <= STATS_LDS_N): the status, the keys sorted in LDS
//                      (stats_sort, smm_stats.hpp) and stored, then in place the window argmin of every mass (dens_argmin: lanes stride
//                      the windows, the minimum taken on (width, index), so the earliest tie wins whatever order waves finish in) and the
//                      levels and the ending of the half-sample mode (dens_mode).
//   k_dens_keys      : the order keys of the long columns with their pooled index, for the segmented radix sort of smm_rank.hpp
//                      (k_rank_sort_small, k_rank_count / _scan / _scatter over a plain (offset, length) table); status 1 for a draw
//                      that is not finite; the mode's range set to the whole column.
//   k_dens_win       : one grid-wide window argmin of every long column over its sorted keys: the windows of a mass (what = its index), or
//                      of the mode's next level (what < 0) while the range is not yet below the wide minimum.  Block z takes the z-th
//                      slice of the windows' first rows — a window's far end may lie in a later block's slice — and stores its minimum.
//   k_dens_win_fin   : one wave per long column: the blocks' minima combined on (width, index); the interval of the mass, or the mode's
//                      range moved to the window found.
//   k_dens_mode_fin  : one workgroup per long column: the rest of the mode's range in LDS, its remaining levels and ending (dens_mode).
//   k_dens_chunk_dev : one workgroup per (chunk, parameter): the chunk's pairwise sum (pw_sum) of (x - mean)^2, for the variance.
//   k_dens_bw        : one lane per column: the bandwidth (given, or R's bw.nrd0 from the variance and the quartiles of the sorted keys),
//                      the ends of the grid and kde_status.
//   k_dens_kde       : one workgroup per (chunk, tile of DENS_TILE grid points, parameter): each lane keeps its 32 draws of the chunk in
//                      registers across the tile's grid points; per grid point the terms e_ij go to LDS at the places pw_sum stages them
//                      and stats_pw (smm_stats.hpp) adds them: the chunk sums [kb][chunks of the batch][n_grid].
//   k_dens_finish    : one wave per column of a batch of groups: lane = grid point: the chunk sums added left to right, the density, the
//                      grid; then the first maximum (np.argmax's order).
#pragma once

constexpr int DENS_WG = STATS_WG;
constexpr int DENS_TILE = 16;                    // grid points of one k_dens_kde workgroup
constexpr int DENS_REG = STATS_LDS_N / DENS_WG;  // draws of a chunk one lane holds
constexpr int DENS_NB_MAX = 1024;                // blocks of a grid-wide window argmin

struct DensRed {   // the LDS of dens_argmin: the waves' minima
    double w[DENS_WG / 64];
    long long i[DENS_WG / 64];
};

__device__ __forceinline__ double dens_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// (w, i) before (bw, bi) in the argmin's order: the smaller width, then the smaller index; bi < 0: nothing yet
__device__ __forceinline__ bool dens_before(double w, long long i, double bw, long long bi) {
    if (i < 0) return false;
    return bi < 0 || w < bw || (w == bw && i < bi);
}

// the windows [base + i, base + i + span] of the sorted column at(.), i in [i0, i1): this thread's, then this wave's first minimum
template <class At>
__device__ __forceinline__ void dens_wave_argmin(At at, long long base, long long i0, long long i1, long long span, double& bw, long long& bi) {
    bw = 0.0; bi = -1;
    for (long long i = i0 + threadIdx.x; i < i1; i += DENS_WG) {
        const double w = at(base + i + span) - at(base + i);
        if (dens_before(w, i, bw, bi)) { bw = w; bi = i; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double ow = __shfl_xor(bw, o, 64);
        const long long oi = __shfl_xor(bi, o, 64);
        if (dens_before(ow, oi, bw, bi)) { bw = ow; bi = oi; }
    }
}

// the same over the block: every thread calls it and gets (bw, bi); bi < 0: no window in [i0, i1)
template <class At>
__device__ void dens_argmin(At at, long long base, long long i0, long long i1, long long span, DensRed& r, double& bw, long long& bi) {
    dens_wave_argmin(at, base, i0, i1, span, bw, bi);
    if ((threadIdx.x & 63) == 0) { r.w[threadIdx.x >> 6] = bw; r.i[threadIdx.x >> 6] = bi; }
    __syncthreads();
    bw = r.w[0]; bi = r.i[0];
    for (int q = 1; q < DENS_WG / 64; ++q)
        if (dens_before(r.w[q], r.i[q], bw, bi)) { bw = r.w[q]; bi = r.i[q]; }
    __syncthreads();   // (r is free again)
}

// the HDI's window span of mass p over m >= 1 sorted draws
__device__ __forceinline__ long long dens_hdi_span(double p, long long m) {
    const long long k = (long long)floor(p * (double)m);
    return k < m - 1 ? k : m - 1;
}

// the half-sample mode of the n >= 1 sorted draws at(lo .. lo + n): the levels left, then the ending; every thread of the block calls it
template <class At>
__device__ double dens_mode(At at, long long lo, long long n, DensRed& r) {
    while (n > 3) {
        const long long h = (n + 1) / 2;
        double bw;
        long long bi;
        dens_argmin(at, lo, 0, n - h + 1, h - 1, r, bw, bi);
        lo += bi;
        n = h;
    }
    if (n == 1) return at(lo);
    if (n == 2) return (at(lo) + at(lo + 1)) / 2.0;
    const double a = at(lo + 1) - at(lo), b = at(lo + 2) - at(lo + 1);
    return a < b ? (at(lo) + at(lo + 1)) / 2.0 : b < a ? (at(lo + 1) + at(lo + 2)) / 2.0 : at(lo + 1);
}

// grid (short groups, kb); SK [kb][Mtot] gets the sorted keys; o_hlo, o_hhi [n_mass][G][np] (NULL: no interval), o_mode [G][np] or NULL
__global__ __launch_bounds__(DENS_WG) void k_dens_small(const double* __restrict__ col, long long Mtot, const int* __restrict__ sgrp,
                                                        const long long* __restrict__ G0, const long long* __restrict__ gm, int G, int k0,
                                                        int np, const double* __restrict__ mass, int n_mass,
                                                        unsigned long long* __restrict__ SK, int* __restrict__ o_status,
                                                        double* __restrict__ o_hlo, double* __restrict__ o_hhi, double* __restrict__ o_mode) {
    extern __shared__ __align__(16) double sx[];   // the keys: the power of two at or above the longest short column
    __shared__ DensRed red;
    unsigned long long* sk = (unsigned long long*)sx;
    const int g = sgrp[blockIdx.x], kk = blockIdx.y, k = k0 + kk, tid = threadIdx.x;
    const int m = (int)gm[g];
    const double* x = col + (size_t)kk * Mtot + G0[g];
    int bad = 0;
    for (int i = tid; i < m; i += DENS_WG) bad |= !isfinite(x[i]);
    bad = __syncthreads_or(bad);
    const int st = m == 0 ? 2 : bad ? 1 : 0;
    const size_t at_gk = (size_t)g * np + k;
    if (tid == 0) o_status[at_gk] = st;
    if (st != 0) {
        if (tid == 0) {
            for (int p = 0; p < n_mass && o_hlo; ++p) o_hlo[(size_t)p * G * np + at_gk] = o_hhi[(size_t)p * G * np + at_gk] = dens_nan();
            if (o_mode) o_mode[at_gk] = dens_nan();
        }
        return;
    }
    stats_sort(sk, m, [&](int i) { return x[i]; });
    unsigned long long* so = SK + (size_t)kk * Mtot + G0[g];
    for (int i = tid; i < m; i += DENS_WG) so[i] = sk[i];
    auto at = [&](long long i) { return stats_unkey(sk[i]); };
    for (int p = 0; p < n_mass && o_hlo; ++p) {
        const long long span = dens_hdi_span(mass[p], m);
        double bw;
        long long bi;
        dens_argmin(at, 0, 0, m - span, span, red, bw, bi);
        if (tid == 0) { o_hlo[(size_t)p * G * np + at_gk] = at(bi); o_hhi[(size_t)p * G * np + at_gk] = at(bi + span); }
    }
    if (o_mode) {
        const double md = dens_mode(at, 0, m, red);
        if (tid == 0) o_mode[at_gk] = md;
    }
}

// grid (long groups, kb, blocks); K, I [kb][Mtot]; o_status zeroed; mlo, mn [long groups][kb]
__global__ __launch_bounds__(DENS_WG) void k_dens_keys(const double* __restrict__ col, long long Mtot, const int* __restrict__ wgrp,
                                                       const long long* __restrict__ off, const long long* __restrict__ len, int k0, int np,
                                                       unsigned long long* __restrict__ K, unsigned* __restrict__ I,
                                                       int* __restrict__ o_status, long long* __restrict__ mlo, long long* __restrict__ mn) {
    const int wi = blockIdx.x, kk = blockIdx.y, g = wgrp[wi];
    const long long m = len[wi];
    const size_t o = (size_t)kk * Mtot + off[wi];
    bool bad = false;
    for (long long i = (long long)blockIdx.z * DENS_WG + threadIdx.x; i < m; i += (long long)gridDim.z * DENS_WG) {
        const double v = col[o + i];
        bad |= !isfinite(v);
        K[o + i] = stats_key(v);
        I[o + i] = (unsigned)i;
    }
    if (bad) o_status[(size_t)g * np + k0 + kk] = 1;
    if (blockIdx.z == 0 && threadIdx.x == 0) { mlo[(size_t)wi * gridDim.y + kk] = 0; mn[(size_t)wi * gridDim.y + kk] = m; }
}

// the windows of long column (wi, kk) that a pass looks at: what >= 0 the mass's, else the mode's next level (false: none is due)
__device__ __forceinline__ bool dens_pass(int what, const double* __restrict__ mass, long long m, long long lo, long long n, long long wide_min,
                                          long long& base, long long& cnt, long long& span) {
    if (what >= 0) {
        span = dens_hdi_span(mass[what], m);
        base = 0;
        cnt = m - span;
        return true;
    }
    if (n <= 3 || n < wide_min) return false;
    const long long h = (n + 1) / 2;
    base = lo; cnt = n - h + 1; span = h - 1;
    return true;
}

// grid (long groups, kb, NB); part_w, part_i [long groups][kb][NB]
__global__ __launch_bounds__(DENS_WG) void k_dens_win(const unsigned long long* __restrict__ K, long long Mtot, const int* __restrict__ wgrp,
                                                      const long long* __restrict__ off, const long long* __restrict__ len, int k0, int np,
                                                      const int* __restrict__ status, int what, const double* __restrict__ mass,
                                                      long long wide_min, const long long* __restrict__ mlo, const long long* __restrict__ mn,
                                                      double* __restrict__ part_w, long long* __restrict__ part_i) {
    __shared__ DensRed red;
    const int wi = blockIdx.x, kk = blockIdx.y, g = wgrp[wi];
    const size_t w = (size_t)wi * gridDim.y + kk;
    if (status[(size_t)g * np + k0 + kk] != 0) return;
    long long base, cnt, span;
    if (!dens_pass(what, mass, len[wi], mlo[w], mn[w], wide_min, base, cnt, span)) return;
    const unsigned long long* s = K + (size_t)kk * Mtot + off[wi];
    const long long per = (cnt + gridDim.z - 1) / gridDim.z;
    const long long i0 = min(cnt, (long long)blockIdx.z * per), i1 = min(cnt, i0 + per);
    double bw;
    long long bi;
    dens_argmin([&](long long i) { return stats_unkey(s[i]); }, base, i0, i1, span, red, bw, bi);
    if (threadIdx.x == 0) { part_w[w * gridDim.z + blockIdx.z] = bw; part_i[w * gridDim.z + blockIdx.z] = bi; }
}

// grid (long groups, kb), 64 lanes; NB: the blocks of the pass
__global__ __launch_bounds__(64) void k_dens_win_fin(const unsigned long long* __restrict__ K, long long Mtot, const int* __restrict__ wgrp,
                                                     const long long* __restrict__ off, const long long* __restrict__ len, int G, int k0,
                                                     int np, const int* __restrict__ status, int what, const double* __restrict__ mass,
                                                     long long wide_min, int NB, const double* __restrict__ part_w,
                                                     const long long* __restrict__ part_i, long long* __restrict__ mlo,
                                                     long long* __restrict__ mn, double* __restrict__ o_hlo, double* __restrict__ o_hhi) {
    const int wi = blockIdx.x, kk = blockIdx.y, g = wgrp[wi], lane = threadIdx.x;
    const size_t w = (size_t)wi * gridDim.y + kk, at_gk = (size_t)g * np + k0 + kk;
    if (status[at_gk] != 0) {
        if (what >= 0 && lane == 0) o_hlo[(size_t)what * G * np + at_gk] = o_hhi[(size_t)what * G * np + at_gk] = dens_nan();
        return;
    }
    long long base, cnt, span;
    if (!dens_pass(what, mass, len[wi], mlo[w], mn[w], wide_min, base, cnt, span)) return;
    double bw = 0.0;
    long long bi = -1;
    for (int z = lane; z < NB; z += 64)
        if (dens_before(part_w[w * NB + z], part_i[w * NB + z], bw, bi)) { bw = part_w[w * NB + z]; bi = part_i[w * NB + z]; }
    for (int o = 32; o > 0; o >>= 1) {
        const double ow = __shfl_xor(bw, o, 64);
        const long long oi = __shfl_xor(bi, o, 64);
        if (dens_before(ow, oi, bw, bi)) { bw = ow; bi = oi; }
    }
    if (lane != 0) return;
    const unsigned long long* s = K + (size_t)kk * Mtot + off[wi];
    if (what >= 0) {
        o_hlo[(size_t)what * G * np + at_gk] = stats_unkey(s[bi]);
        o_hhi[(size_t)what * G * np + at_gk] = stats_unkey(s[bi + span]);
    } else {
        mlo[w] = base + bi;
        mn[w] = span + 1;
    }
}

// grid (long groups, kb): the mode's range is below the wide minimum (or at most 3 rows) by now
__global__ __launch_bounds__(DENS_WG) void k_dens_mode_fin(const unsigned long long* __restrict__ K, long long Mtot, const int* __restrict__ wgrp,
                                                           const long long* __restrict__ off, int k0, int np, const int* __restrict__ status,
                                                           const long long* __restrict__ mlo, const long long* __restrict__ mn,
                                                           double* __restrict__ o_mode) {
    extern __shared__ __align__(16) double sx[];   // STATS_LDS_N keys
    __shared__ DensRed red;
    unsigned long long* sk = (unsigned long long*)sx;
    const int wi = blockIdx.x, kk = blockIdx.y, g = wgrp[wi], tid = threadIdx.x;
    const size_t w = (size_t)wi * gridDim.y + kk, at_gk = (size_t)g * np + k0 + kk;
    if (status[at_gk] != 0) {
        if (tid == 0) o_mode[at_gk] = dens_nan();
        return;
    }
    const long long lo = mlo[w];
    const int n = (int)min(mn[w], (long long)STATS_LDS_N);
    const unsigned long long* s = K + (size_t)kk * Mtot + off[wi] + lo;
    for (int i = tid; i < n; i += DENS_WG) sk[i] = s[i];
    __syncthreads();
    const double md = dens_mode([&](long long i) { return stats_unkey(sk[i]); }, 0, n, red);
    if (tid == 0) o_mode[at_gk] = md;
}

// grid (chunks, kb); mean [G][np]; cdev [kb][NC]
__global__ __launch_bounds__(DENS_WG) void k_dens_chunk_dev(const double* __restrict__ col, long long Mtot, const long long* __restrict__ cst,
                                                            const int* __restrict__ clen, const int* __restrict__ cgrp, int NC, int k0,
                                                            int np, const double* __restrict__ mean, double* __restrict__ cdev) {
    extern __shared__ __align__(16) double sx[];   // STATS_LDS_N
    __shared__ PwTree pt;
    const int ch = blockIdx.x, kk = blockIdx.y;
    const double* x = col + (size_t)kk * Mtot + cst[ch];
    const double mu = mean[(size_t)cgrp[ch] * np + k0 + kk];
    const double s = pw_sum(clen[ch], [&](int i) { const double e = x[i] - mu; return e * e; }, sx, pt);
    if (threadIdx.x == 0) cdev[(size_t)kk * NC + ch] = s;
}

// one lane per (group, parameter of the batch).  bw_in [np] or NULL (bw.nrd0), rng [np][2] or NULL (3 bandwidths past the extremes)
__global__ void k_dens_bw(const double* __restrict__ col, const unsigned long long* __restrict__ SK, long long Mtot,
                          const long long* __restrict__ G0, const long long* __restrict__ gm, const int* __restrict__ gch0, int NC, int G,
                          int k0, int kb, int np, const int* __restrict__ status, const double* __restrict__ cdev,
                          const double* __restrict__ bw_in, const double* __restrict__ rng, double* __restrict__ o_bw,
                          double* __restrict__ o_lo, double* __restrict__ o_hi, int* __restrict__ o_kst) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= G * kb) return;
    const int g = e / kb, kk = e - g * kb, k = k0 + kk;
    const size_t at_gk = (size_t)g * np + k;
    const long long m = gm[g];
    double h = dens_nan(), lo = dens_nan(), hi = dens_nan();
    int kst = 1;
    if (status[at_gk] == 0) {
        const unsigned long long* s = SK + (size_t)kk * Mtot + G0[g];
        auto at = [&](long long i) { return stats_unkey(s[i]); };
        if (bw_in) h = bw_in[k];
        else {
            double S = 0.0;
            for (int ch = gch0[g]; ch < gch0[g + 1]; ++ch) S = S + cdev[(size_t)kk * NC + ch];
            const double sd = __builtin_sqrt(m < 2 ? dens_nan() : S / (double)(m - 1));
            const double q75 = stats_quantile<decltype(at), long long>(m, 0.75, at), q25 = stats_quantile<decltype(at), long long>(m, 0.25, at);
            const double a = (q75 - q25) / 1.34;
            double l = sd < a ? sd : a;
            if (l == 0.0) l = sd;
            if (l == 0.0) l = fabs(col[(size_t)kk * Mtot + G0[g]]);
            if (l == 0.0) l = 1.0;
            h = (0.9 * l) * smm_exp(-0.2 * smm_log((double)m));
        }
        if (hist_finite(h) && h > 0.0) {
            if (rng) { lo = rng[2 * k]; hi = rng[2 * k + 1]; }
            else { lo = at(0) - 3.0 * h; hi = at(m - 1) + 3.0 * h; }
            kst = hist_finite(hi - lo) ? 0 : 2;
        }
    }
    o_bw[at_gk] = h; o_lo[at_gk] = lo; o_hi[at_gk] = hi; o_kst[at_gk] = kst;
}

// grid point j of numpy's linspace(lo, hi, b + 1) (smm_get_histogram's edges)
__device__ __forceinline__ double dens_grid(int j, double lo, double hi, int b) {
    const double delta = hi - lo, step = delta / (double)b;
    return j == b ? hi : step != 0.0 ? (double)j * step + lo : ((double)j / (double)b) * delta + lo;
}

// grid (chunks [c0, c0 + gridDim.x) of the batch's groups, tiles, kb); csk [kb][gridDim.x][n_grid]
__global__ __launch_bounds__(DENS_WG) void k_dens_kde(const double* __restrict__ col, long long Mtot, const long long* __restrict__ cst,
                                                      const int* __restrict__ clen, const int* __restrict__ cgrp, int c0, int k0, int np,
                                                      int n_grid, const int* __restrict__ kst, const double* __restrict__ bw,
                                                      const double* __restrict__ glo, const double* __restrict__ ghi,
                                                      double* __restrict__ csk) {
    extern __shared__ __align__(16) double sx[];   // STATS_LDS_N terms
    __shared__ PwTree pt;
    const int ch = c0 + blockIdx.x, kk = blockIdx.z, tid = threadIdx.x;
    const size_t at_gk = (size_t)cgrp[ch] * np + k0 + kk;
    if (kst[at_gk] != 0) return;
    const int Lc = clen[ch];
    const double* x = col + (size_t)kk * Mtot + cst[ch];
    double xr[DENS_REG];
#pragma unroll
    for (int q = 0; q < DENS_REG; ++q) xr[q] = tid + q * DENS_WG < Lc ? x[tid + q * DENS_WG] : 0.0;
    const double h = bw[at_gk], rh = 1.0 / h, lo = glo[at_gk], hi = ghi[at_gk];
    double* o = csk + ((size_t)kk * gridDim.x + blockIdx.x) * n_grid;
    const int j1 = min(n_grid, ((int)blockIdx.y + 1) * DENS_TILE);
    for (int j = blockIdx.y * DENS_TILE; j < j1; ++j) {
        const double gj = dens_grid(j, lo, hi, n_grid - 1);
#pragma unroll
        for (int q = 0; q < DENS_REG; ++q)
            if (tid + q * DENS_WG < Lc) {
                const double u = (gj - xr[q]) * rh;
                sx[tid + q * DENS_WG] = smm_exp(-0.5 * (u * u));
            }
        __syncthreads();
        const double s = stats_pw(sx, Lc, pt);
        if (tid == 0) o[j] = s;
    }
}

// grid (groups [g0, g0 + gridDim.x), kb), 64 lanes; c0 = gch0[g0], NCb the batch's chunks; o_grid, o_dens [gridDim.x][kb][n_grid] (either
// may be NULL); o_kmode [G][np] or NULL
__global__ __launch_bounds__(64) void k_dens_finish(const double* __restrict__ csk, const long long* __restrict__ gm, const int* __restrict__ gch0,
                                                    int g0, int c0, int NCb, int k0, int np, int n_grid, const int* __restrict__ kst,
                                                    const double* __restrict__ bw, const double* __restrict__ glo,
                                                    const double* __restrict__ ghi, double* __restrict__ o_grid, double* __restrict__ o_dens,
                                                    double* __restrict__ o_kmode) {
    const int gl = blockIdx.x, g = g0 + gl, kk = blockIdx.y, kb = gridDim.y, lane = threadIdx.x;
    const size_t at_gk = (size_t)g * np + k0 + kk, row = ((size_t)gl * kb + kk) * n_grid;
    if (kst[at_gk] != 0) {
        for (int j = lane; j < n_grid; j += 64) {
            if (o_grid) o_grid[row + j] = dens_nan();
            if (o_dens) o_dens[row + j] = dens_nan();
        }
        if (o_kmode && lane == 0) o_kmode[at_gk] = dens_nan();
        return;
    }
    const double h = bw[at_gk], lo = glo[at_gk], hi = ghi[at_gk], dm = (double)gm[g];
    double bv = 0.0;
    int bj = -1;   // np.argmax: the first NaN, else the first maximum
    auto better = [](double v, int j, double w, int i) {
        if (j < 0) return false;
        if (i < 0) return true;
        const bool vn = v != v, wn = w != w;
        if (vn || wn) return vn && (!wn || j < i);
        return v > w || (v == w && j < i);
    };
    for (int j = lane; j < n_grid; j += 64) {
        double D = 0.0;
        for (int ch = gch0[g]; ch < gch0[g + 1]; ++ch) D = D + csk[((size_t)kk * NCb + (ch - c0)) * n_grid + j];
        const double dj = (D / dm) / (h * 2.5066282746310002);
        if (o_grid) o_grid[row + j] = dens_grid(j, lo, hi, n_grid - 1);
        if (o_dens) o_dens[row + j] = dj;
        if (better(dj, j, bv, bj)) { bv = dj; bj = j; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(bv, o, 64);
        const int oj = __shfl_xor(bj, o, 64);
        if (better(ov, oj, bv, bj)) { bv = ov; bj = oj; }
    }
    if (o_kmode && lane == 0) o_kmode[at_gk] = dens_grid(bj, lo, hi, n_grid - 1);
}
