// chains' autocorrelation, effective sample size and split R-hat halves (smm_get_chain_diag, include/smmhip.h) — part of libsmmhip
// (included by smmhip.hip inside its anonymous namespace after smm_stats.hpp; gfx950 device code).  Reads the history records hrec
// [T][N][HW] (smm_params.hpp: H_*) and nothing else; writes only the scratch and result buffers of the call.
//
//   k_diag_gather : one workgroup per chain walks the window's state rows (state_walk, smm_window.hpp: lane = iteration, a(t) = the last
//                   accepted row at or before t) and writes the S = np + 1 carry-forward columns col [S][Nb][n] (params[a(t)][s], then
//                   value[a(t)]; NaN while no row is accepted); counts the window's non-exchanged iterations E and the accepted ones
//                   among them A.
//   k_diag_acov   : one workgroup per (chain, series) column: a non-finite entry ends it (status 3).  Otherwise the two halves' mean and
//                   variance for R-hat (pw_sum, smm_stats.hpp), the column's mean, then d = x - mean (in LDS when n <= 8192,
//                   else in place in the scratch column, read from L2).  The lags then go in blocks of 256, lane = lag: each lane sums
//                   its products d[i] d[i + k] by the pairwise tree of numpy over chunks of 8192, walked in registers (the tree of a
//                   chunk is at most 7 levels deep; a leaf of <= 128 products keeps numpy's 8 strided accumulators).  After a block
//                   lane 0 extends Geyer's initial monotone sequence over its pairs; the loop stops once the sequence is truncated and
//                   every requested acf lag is written.
// R-hat itself (a few doubles per group) is reduced by the host from the halves (smmhip.hip: smm_get_chain_diag).
#pragma once

constexpr int DIAG_WG = 256;   // lanes of both kernels; also the lags of one block of k_diag_acov

__global__ __launch_bounds__(DIAG_WG) void k_diag_gather(const double* __restrict__ hrec, int N, int HW, int np, int t0, int n, int c0,
                                                         int Nb, double* __restrict__ col, int* __restrict__ o_nacc,
                                                         int* __restrict__ o_noex) {
    __shared__ int wred[DIAG_WG / 64];
    __shared__ int wtot[DIAG_WG / 64];
    const int cl = xcd_chain(blockIdx.x, gridDim.x), c = c0 + cl;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int S = np + 1;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    int nacc = 0, noex = 0;
    state_walk<H_EXCH>(hrec, N, HW, c, t0, n, wred, [&](int r, int a, bool acc, double ex) {
        if (ex == 0.0) { ++noex; if (acc) ++nacc; }
        double* o = col + (size_t)cl * n + r;
        const size_t cs = (size_t)Nb * n;
        if (a < 0) {
            for (int s = 0; s < S; ++s) o[s * cs] = qnan;
        } else {
            const double* h = hrec + ((size_t)a * N + c) * HW;
            for (int s = 0; s < np; ++s) o[s * cs] = h[H_PARAMS + s];
            o[np * cs] = h[H_VALUE];
        }
    });
    for (int o = 32; o > 0; o >>= 1) { nacc += __shfl_xor(nacc, o, 64); noex += __shfl_xor(noex, o, 64); }
    if (lane == 0) { wred[w] = nacc; wtot[w] = noex; }
    __syncthreads();
    if (tid == 0) {
        for (int q = 1; q < DIAG_WG / 64; ++q) { nacc += wred[q]; noex += wtot[q]; }
        o_nacc[c] = nacc;
        o_noex[c] = noex;
    }
}

// one leaf of the pairwise tree over the products d[i] d[i + k], i = lo .. lo + m - 1 (m <= 128): numpy's 8 strided accumulators
__device__ __noinline__ double diag_leaf(const double* __restrict__ d, int lo, int m, int k) {
    if (m < 8) {
        double s = 0.0;
        for (int i = lo; i < lo + m; ++i) { const double p = d[i] * d[i + k]; s = s + p; }
        return s;
    }
    double r0 = d[lo] * d[lo + k], r1 = d[lo + 1] * d[lo + 1 + k], r2 = d[lo + 2] * d[lo + 2 + k], r3 = d[lo + 3] * d[lo + 3 + k];
    double r4 = d[lo + 4] * d[lo + 4 + k], r5 = d[lo + 5] * d[lo + 5 + k], r6 = d[lo + 6] * d[lo + 6 + k], r7 = d[lo + 7] * d[lo + 7 + k];
    const int m8 = lo + m - m % 8;
    for (int i = lo + 8; i < m8; i += 8) {
        const double* x = d + i;
        const double* y = d + i + k;
        const double p0 = x[0] * y[0], p1 = x[1] * y[1], p2 = x[2] * y[2], p3 = x[3] * y[3];
        const double p4 = x[4] * y[4], p5 = x[5] * y[5], p6 = x[6] * y[6], p7 = x[7] * y[7];
        r0 = r0 + p0; r1 = r1 + p1; r2 = r2 + p2; r3 = r3 + p3;
        r4 = r4 + p4; r5 = r5 + p5; r6 = r6 + p6; r7 = r7 + p7;
    }
    double s = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (int i = m8; i < lo + m; ++i) { const double p = d[i] * d[i + k]; s = s + p; }
    return s;
}

// numpy's pairwise tree over the products of [lo, lo + len) (len <= 8192: at most 7 levels above the leaves), left + right at each node
template <int D>
__device__ __forceinline__ double diag_pw(const double* __restrict__ d, int lo, int len, int k) {
    if constexpr (D == 0) {
        return diag_leaf(d, lo, len, k);
    } else {
        if (len <= 128) return diag_leaf(d, lo, len, k);
        int n2 = len / 2;
        n2 -= n2 % 8;
        const double lf = diag_pw<D - 1>(d, lo, n2, k);
        const double rt = diag_pw<D - 1>(d, lo + n2, len - n2, k);
        return lf + rt;
    }
}

__global__ __launch_bounds__(DIAG_WG) void k_diag_acov(double* __restrict__ col, int n, int N, int c0, int Nb, int S, int max_lag,
                                                       int n_acf, int halves, double* __restrict__ o_ess, int* __restrict__ o_status,
                                                       double* __restrict__ o_acf, double* __restrict__ o_hmu, double* __restrict__ o_hvar) {
    extern __shared__ __align__(16) double sx[];   // min(n, STATS_LDS_N)
    __shared__ PwTree pt;   // (pt.flag: a non-finite entry)
    __shared__ int sdone;
    __shared__ double sac[DIAG_WG];
    const int cl = blockIdx.x, s = blockIdx.y, c = c0 + cl, tid = threadIdx.x;
    double* x = col + ((size_t)s * Nb + cl) * n;
    const size_t o1 = (size_t)s * N + c;   // [S][N]
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    if (tid == 0) { pt.flag = 0; sdone = 0; }
    __syncthreads();
    bool bad = false;
    for (int i = tid; i < n; i += DIAG_WG) bad |= !isfinite(x[i]);
    if (bad) pt.flag = 1;
    __syncthreads();
    if (pt.flag) {
        if (tid == 0) { o_ess[o1] = qnan; o_status[o1] = 3; }
        if (o_acf)
            for (int k = tid; k < n_acf; k += DIAG_WG) o_acf[(size_t)k * S * N + o1] = qnan;
        return;
    }
    const double dn = (double)n;
    if (halves) {   // split R-hat: x[0:h] and x[n-h:n], mean and np.var(ddof=1) each
        const int h = n / 2;
        for (int hf = 0; hf < 2; ++hf) {
            const double* y = x + (hf ? n - h : 0);
            const double mu = pw_sum(h, [&](int i) { return y[i]; }, sx, pt) / (double)h;
            const double ss = pw_sum(h, [&](int i) { const double e = y[i] - mu; return e * e; }, sx, pt);
            if (tid == 0) {
                o_hmu[(size_t)hf * S * N + o1] = mu;
                o_hvar[(size_t)hf * S * N + o1] = ss / (double)(h - 1);
            }
        }
    }
    const double m = pw_sum(n, [&](int i) { return x[i]; }, sx, pt) / dn;
    const double* d;
    if (n <= STATS_LDS_N) {
        for (int i = tid; i < n; i += DIAG_WG) sx[i] = x[i] - m;
        d = sx;
    } else {   // the column's own scratch, overwritten in place: read back through L2
        for (int i = tid; i < n; i += DIAG_WG) x[i] = x[i] - m;
        d = x;
    }
    __syncthreads();
    double a0 = 0.0;       // acov_0 (every lane, from the first block)
    double Q = 0.0, T = 0.0;   // lane 0: the monotone sequence so far and its sum
    bool trunc = false;
    for (int kb = 0; kb <= max_lag; kb += DIAG_WG) {
        const int k = kb + tid;
        double ac = 0.0;
        if (k <= max_lag) {
            const int L = n - k;
            double Sk = 0.0;
            for (int c8 = 0; c8 < L; c8 += STATS_LDS_N) {
                const double p = diag_pw<7>(d, c8, min(STATS_LDS_N, L - c8), k);
                Sk = Sk + p;
            }
            ac = Sk / dn;
        }
        sac[tid] = ac;
        __syncthreads();
        if (kb == 0) a0 = sac[0];
        if (o_acf && k <= max_lag && k < n_acf) o_acf[(size_t)k * S * N + o1] = ac / a0;
        if (tid == 0) {
            for (int k2 = kb; !trunc && k2 + 1 <= max_lag && k2 + 1 < kb + DIAG_WG; k2 += 2) {   // pair j = k2 / 2
                const double r0 = sac[k2 - kb] / a0, r1 = sac[k2 - kb + 1] / a0;
                const double P = r0 + r1;
                if (k2 == 0) { Q = P; T = 0.0 + Q; }
                else if (!(P > 0.0)) trunc = true;
                else { Q = P < Q ? P : Q; T = T + Q; }
            }
            sdone = trunc && kb + DIAG_WG >= n_acf;
        }
        __syncthreads();
        if (sdone) break;
    }
    if (tid == 0) {
        const double tau = -1.0 + 2.0 * T;
        const bool undef = a0 == 0.0 || !(tau > 0.0);
        o_ess[o1] = undef ? qnan : dn / tau;
        o_status[o1] = undef ? 2 : (trunc ? 0 : 1);
    }
}
