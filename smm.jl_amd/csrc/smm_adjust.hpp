// the regression-adjusted posterior of groups of chains (smm_get_adjustment, include/smmhip.h) — part of libsmmhip (included by
// smmhip.hip inside its anonymous namespace after smm_moments.hpp; gfx950 device code).  Reads the history records through
// k_group_gather (smm_group.hpp) and nothing else; writes only the scratch and result buffers of the call.  The D = np + nm joint columns
// of a batch of chunks lie in the scratch as k_group_gather's chunked form leaves them, [column][chunk][STATS_LDS_N] in the record's
// order (the np parameters, then the nm simulated moments; gathered against a mean of zeros, so untouched), with two more columns behind
// them for the weight and its square.  The single sums are k_group_chunk_sum's, the pair sums k_cov_pairs' (raw) added by
// k_moment_cov_acc, the bandwidth pool_order's quantile of the distance column, the factor and the substitutions moment_chol's and
// moment_subst's (smm_moments.hpp).  What is the adjustment's own:
//
//   k_adjust_rows    : the row pass.  One lane per row of a batch of chunks (lane = row: every column is read and written coalesced),
//                      every sum over the moments inside the lane.  mode 0: the distance d2 of the row to the packed column the bandwidth is
//                      selected from (the gather of this sweep raises k_group_gather's gbad).  mode 1: the weight w; the joint columns
//                      overwritten by w v, the two extra columns by w and w w; the kept rows and their integer weights q counted per
//                      workgroup in LDS, then by one 64-bit atomic each.  mode 2: the joint columns overwritten by e = sqrt(w) (v - mu).
//   k_adjust_sum_acc : one lane per (group, column): the batch's chunk sums added in chunk order onto the group's running sum.
//   k_adjust_means   : one lane per (group, joint column): mu = S(w v) / S(w).
//   k_adjust_solve   : one workgroup of one wave per group, lane = row.  A = C_xx with the ridge in LDS [nm][nm + 1] and its factor; then
//                      lane = parameter: the parameter's column of C_x,theta in LDS solved in place into beta, the intercept and the
//                      residual standard deviation; the status.  (nm + np) (nm + 1) doubles: 65 KB at the caps.
//   k_adjust_apply   : the adjust pass.  One lane per row of a batch of chunks, a batch of parameters: x in place, then theta* = theta -
//                      x' beta with the group's beta in LDS, to the packed columns the weighted select reads; q to its packed column;
//                      the rows that leave [lb, ub] counted per wave by a ballot, per workgroup in LDS, then by 64-bit atomics.
//   k_adjust_targets : one lane per (column, prob): the weight the select looks for, ceil(p Q) - 1 as k_group_pick's rank.
//   k_adjust_hist    : one digit of the weighted radix select on k_group_hist's digit layout: the histograms add q instead of 1, 64-bit
//                      in LDS per workgroup and then in global memory; rows with q = 0 are skipped where they lie.  A workgroup counts
//                      blocks of `per` consecutive rows of its column, so a short column crosses workgroups when per is small.  Integer
//                      weights: the sums, and so the selected keys, do not depend on the order the workgroups arrive in.  k_group_pick
//                      (smm_group.hpp) finds the digit: the smallest key whose weights below and at it reach the target is the key of
//                      weighted rank target - 1.
//   k_adjust_finish  : one lane per (column, prob): the selected key as a double.
#pragma once

constexpr int ADJ_WG = 256;   // lanes of the row passes
constexpr int ADJ_RB = 3;     // probs one k_adjust_hist workgroup counts (3 LDS histograms of 2048 64-bit bins: 48 KB)
static_assert(STATS_LDS_N % ADJ_WG == 0, "k_adjust_rows: a workgroup lies inside one chunk");

// sc_k: the caller's scale, else smm_get_moment_stats' s_k
__device__ __forceinline__ double adjust_scale(const double* __restrict__ scale, const double* __restrict__ w, int k) {
    if (scale) return scale[k];
    const double wk = w[k];
    return (isfinite(wk) && wk != 0.0) ? wk : 1.0;
}

__device__ __forceinline__ double adjust_weight(double d2, double del, int kernel) {
    if (kernel == 0) return d2 <= del ? 1.0 : 0.0;
    if (!(d2 < del)) return 0.0;
    const double q = d2 / del;
    return 1.0 - q;
}

struct AdjRows {   // what the row passes share: the batch of chunks in the scratch and where its rows belong
    double* buf;                 // [D + 2][nb][STATS_LDS_N]
    int nb, cb0, np, nm;
    const int* clen;             // [NC] rows of a chunk
    const int* cgrp;             // [NC] its group
    const long long* cst;        // [NC] its first row in the pooled index space
    const double *mom, *w, *scale;
    const double* delta;         // [G] the bandwidth (modes 1, 2 and the adjust pass)
    int kernel;
};

// the row's x_k = (s_k - mom_k) / sc_k for k ascending, handed to f(k, x_k), and its distance
template <class F>
__device__ __forceinline__ double adjust_distance(const AdjRows& a, size_t at, size_t cs, F f) {
    double d2 = 0.0;
    for (int k = 0; k < a.nm; ++k) {
        const double d = a.buf[(size_t)(a.np + k) * cs + at] - a.mom[k];
        const double x = d / adjust_scale(a.scale, a.w, k);
        const double p = x * x;
        d2 = d2 + p;
        f(k, x);
    }
    return d2;
}

// grid (STATS_LDS_N / ADJ_WG, nb)
__global__ __launch_bounds__(ADJ_WG) void k_adjust_rows(AdjRows a, int mode, double* __restrict__ d2col,
                                                        const double* __restrict__ mu, unsigned long long* __restrict__ nkept,
                                                        unsigned long long* __restrict__ qsum) {
    __shared__ unsigned long long skept, sq;
    const int cl = blockIdx.y, ch = a.cb0 + cl, pos = blockIdx.x * ADJ_WG + threadIdx.x, D = a.np + a.nm;
    if (blockIdx.x * ADJ_WG >= a.clen[ch]) return;   // (the whole workgroup)
    const bool row = pos < a.clen[ch];
    const int g = a.cgrp[ch];
    const size_t cs = (size_t)a.nb * STATS_LDS_N, at = (size_t)cl * STATS_LDS_N + pos;
    if (mode == 1 && threadIdx.x == 0) { skept = 0; sq = 0; }
    if (mode == 1) __syncthreads();
    if (row) {
        if (mode == 0) {
            d2col[a.cst[ch] + pos] = adjust_distance(a, at, cs, [](int, double) {});
        } else {
            const double d2 = adjust_distance(a, at, cs, [](int, double) {});
            const double om = adjust_weight(d2, a.delta[g], a.kernel);
            if (mode == 1) {
                for (int j = 0; j < a.np; ++j) a.buf[(size_t)j * cs + at] = om * a.buf[(size_t)j * cs + at];
                adjust_distance(a, at, cs, [&](int k, double x) { a.buf[(size_t)(a.np + k) * cs + at] = om * x; });
                a.buf[(size_t)D * cs + at] = om;
                a.buf[(size_t)(D + 1) * cs + at] = om * om;
                if (om > 0.0) {
                    atomicAdd(&skept, 1ull);
                    atomicAdd(&sq, (unsigned long long)(long long)ceil(om * 1048576.0));
                }
            } else {
                const double r = sqrt(om);
                const double* m = mu + (size_t)g * D;
                for (int j = 0; j < a.np; ++j) {
                    const double d = a.buf[(size_t)j * cs + at] - m[j];
                    a.buf[(size_t)j * cs + at] = r * d;
                }
                adjust_distance(a, at, cs, [&](int k, double x) {
                    const double d = x - m[a.np + k];
                    a.buf[(size_t)(a.np + k) * cs + at] = r * d;
                });
            }
        }
    }
    if (mode == 1) {
        __syncthreads();
        if (threadIdx.x == 0 && skept) { atomicAdd(&nkept[g], skept); atomicAdd(&qsum[g], sq); }
    }
}

// csum [DC][nb]: k_group_chunk_sum's sums of the chunks [cb0, cb0 + nb); sums [G][DC]
__global__ void k_adjust_sum_acc(const double* __restrict__ csum, int nb, int cb0, const int* __restrict__ gch0, int G, int DC,
                                 double* __restrict__ sums) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= G * DC) return;
    const int g = e / DC, q = e - g * DC;
    const int lo = max(gch0[g], cb0), hi = min(gch0[g + 1], cb0 + nb);
    if (lo >= hi) return;
    double S = sums[e];
    for (int ch = lo; ch < hi; ++ch) S = S + csum[(size_t)q * nb + (ch - cb0)];
    sums[e] = S;
}

// mu [G][D] in the record's order from sums [G][D + 2] (column D: the sum of the weights)
__global__ void k_adjust_means(const double* __restrict__ sums, int G, int D, double* __restrict__ mu) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= G * D) return;
    const int g = e / D, q = e - g * D;
    mu[e] = sums[(size_t)g * (D + 2) + q] / sums[(size_t)g * (D + 2) + D];
}

struct AdjustOut {   // the call's result slices on the device (NULL: not asked for)
    long long* n_kept;
    double *bandwidth, *sum_w, *ess, *x_mean, *raw_mean, *beta, *adj_mean, *adj_sd;
};

// acc [G][D][D] (a >= b, the record's order: parameter j is column j, discrepancy k column np + k); st [G] and betai [G][nm][np] are
// the call's own copies for the adjust pass and the select
__global__ __launch_bounds__(MOMENT_WG) void k_adjust_solve(const double* __restrict__ acc, const double* __restrict__ sums,
                                                            const double* __restrict__ mu, const double* __restrict__ delta,
                                                            const long long* __restrict__ gm, const int* __restrict__ gbad,
                                                            const unsigned long long* __restrict__ nkept, int np, int nm, int kernel,
                                                            double ridge, int* __restrict__ st, double* __restrict__ betai, AdjustOut o) {
    extern __shared__ __align__(16) double sm[];   // A [nm][nm + 1], X [np][nm + 1]
    __shared__ int bad;
    const int g = blockIdx.x, tid = threadIdx.x, D = np + nm, ld = nm + 1;
    double* A = sm;
    double* X = A + (size_t)nm * ld;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    const long long m = gm[g], kept = (long long)nkept[g];
    const double del = delta[g], sw = sums[(size_t)g * (D + 2) + D], sw2 = sums[(size_t)g * (D + 2) + D + 1];
    int status = m < 2 ? 1 : gbad[g] != 0 ? 2 : ((kernel == 1 && !(del > 0.0)) || kept < nm + 2) ? 3 : 0;
    const bool none = status == 1 || status == 2;
    auto C = [&](int a, int b) {   // the pair sum of the record's columns a, b
        const int hi = a >= b ? a : b, lo = a >= b ? b : a;
        return acc[((size_t)g * D + hi) * D + lo];
    };
    if (tid == 0) {
        bad = 0;
        if (o.n_kept) o.n_kept[g] = none ? 0 : kept;
        if (o.bandwidth) o.bandwidth[g] = none ? qnan : del;
        if (o.sum_w) o.sum_w[g] = none ? qnan : sw;
        if (o.ess) o.ess[g] = none ? qnan : (sw * sw) / sw2;
    }
    for (int k = tid; k < nm; k += MOMENT_WG)
        if (o.x_mean) o.x_mean[(size_t)g * nm + k] = none ? qnan : mu[(size_t)g * D + np + k];
    for (int j = tid; j < np; j += MOMENT_WG)
        if (o.raw_mean) o.raw_mean[(size_t)g * np + j] = none ? qnan : mu[(size_t)g * D + j];
    auto finish = [&](int s) {
        if (s != 0) {
            for (int e = tid; e < nm * np; e += MOMENT_WG) {
                betai[(size_t)g * nm * np + e] = qnan;
                if (o.beta) o.beta[(size_t)g * nm * np + e] = qnan;
            }
            for (int j = tid; j < np; j += MOMENT_WG) {
                if (o.adj_mean) o.adj_mean[(size_t)g * np + j] = qnan;
                if (o.adj_sd) o.adj_sd[(size_t)g * np + j] = qnan;
            }
        }
        if (tid == 0) st[g] = s;
    };
    if (status != 0) { finish(status); return; }
    const int k = tid;
    if (k < nm)
        for (int l = 0; l <= k; ++l) {
            double v = C(np + k, np + l);
            if (l == k) {
                const double p = ridge * v;
                v = v + p;
            }
            A[k * ld + l] = v;
        }
    __syncthreads();
    moment_chol(A, nm, ld, k, &bad);
    if (bad) { finish(4); return; }
    if (k < np) {   // parameter k: A beta = C_x,theta's column k
        const int j = k;
        double* x = X + (size_t)j * ld;
        for (int i = 0; i < nm; ++i) x[i] = C(np + i, j);
        moment_subst(A, nm, ld, x);
        double t = 0.0, u = 0.0;
        for (int i = 0; i < nm; ++i) {
            const double b = x[i];
            betai[((size_t)g * nm + i) * np + j] = b;
            if (o.beta) o.beta[((size_t)g * nm + i) * np + j] = b;
            const double p = mu[(size_t)g * D + np + i] * b;
            t = t + p;
            const double q = b * C(np + i, j);
            u = u + q;
        }
        if (o.adj_mean) o.adj_mean[(size_t)g * np + j] = mu[(size_t)g * D + j] - t;
        if (o.adj_sd) {
            const double rad = C(j, j) - u;
            o.adj_sd[(size_t)g * np + j] = sqrt(rad / sw);
        }
    }
    finish(0);
}

// grid (STATS_LDS_N / ADJ_WG, nb); the parameters [j0, j0 + jb): ts [jb][Mtot], qcol [Mtot] (written with the first batch), nout [G][np]
__global__ __launch_bounds__(ADJ_WG) void k_adjust_apply(AdjRows a, int j0, int jb, long long Mtot, const int* __restrict__ st,
                                                         const double* __restrict__ betai, const double* __restrict__ lb,
                                                         const double* __restrict__ ub, double* __restrict__ ts,
                                                         long long* __restrict__ qcol, unsigned long long* __restrict__ nout) {
    extern __shared__ __align__(16) double sb[];   // beta [nm][jb], then the counters [jb]
    const int cl = blockIdx.y, ch = a.cb0 + cl, pos = blockIdx.x * ADJ_WG + threadIdx.x;
    if (blockIdx.x * ADJ_WG >= a.clen[ch]) return;
    int* sout = (int*)(sb + (size_t)a.nm * jb);
    const int g = a.cgrp[ch];
    const bool ok = st[g] == 0;
    const size_t cs = (size_t)a.nb * STATS_LDS_N, at = (size_t)cl * STATS_LDS_N + pos;
    for (int e = threadIdx.x; e < a.nm * jb; e += ADJ_WG) {
        const int k = e / jb, jj = e - k * jb;
        sb[e] = betai[((size_t)g * a.nm + k) * a.np + j0 + jj];
    }
    for (int jj = threadIdx.x; jj < jb; jj += ADJ_WG) sout[jj] = 0;
    __syncthreads();
    const bool row = pos < a.clen[ch];
    const long long prow = a.cst[ch] + pos;
    long long q = 0;
    if (row) {
        if (ok) {
            const double d2 = adjust_distance(a, at, cs, [&](int k, double x) { a.buf[(size_t)(a.np + k) * cs + at] = x; });
            const double om = adjust_weight(d2, a.delta[g], a.kernel);
            if (om > 0.0) q = (long long)ceil(om * 1048576.0);
        }
        if (j0 == 0) qcol[prow] = q;
    }
    for (int jj = 0; jj < jb; ++jj) {   // (every lane of the workgroup: the ballot counts a wave's rows in one LDS add)
        bool outside = false;
        if (q > 0) {
            double t = 0.0;
            for (int k = 0; k < a.nm; ++k) {
                const double p = a.buf[(size_t)(a.np + k) * cs + at] * sb[k * jb + jj];
                t = t + p;
            }
            const double v = a.buf[(size_t)(j0 + jj) * cs + at] - t;
            ts[(size_t)jj * Mtot + prow] = v;
            outside = v < lb[j0 + jj] || v > ub[j0 + jj];
        }
        const unsigned long long b = __ballot(outside);
        if ((threadIdx.x & 63) == 0 && b) atomicAdd(&sout[jj], __popcll(b));
    }
    __syncthreads();
    for (int jj = threadIdx.x; jj < jb; jj += ADJ_WG)
        if (sout[jj]) atomicAdd(&nout[(size_t)g * a.np + j0 + jj], (unsigned long long)sout[jj]);
}

// columns w = g x jb + jj, ranks r < R: rem = ceil(p Q) - 1 (at least 0), -1 for a group without a select; pre = 0
__global__ void k_adjust_targets(const unsigned long long* __restrict__ qsum, const int* __restrict__ st, const double* __restrict__ probs,
                                 int G, int jb, int R, long long* __restrict__ rem, unsigned long long* __restrict__ pre) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= G * jb * R) return;
    const int g = e / (jb * R), r = e % R;
    long long t = -1;
    if (st[g] == 0) {
        const double h = probs[r] * (double)(long long)qsum[g];
        t = max(1ll, (long long)ceil(h)) - 1;
    }
    rem[e] = t;
    pre[e] = 0ull;
}

// a launch counts the columns w0 + blockIdx.x into ghist [gridDim.x][R][GROUP_BINS]; grid (columns, workgroups of a column, R / ADJ_RB);
// workgroup y of a column counts its rows [y per, (y + 1) per), then those gridDim.y per further on
__global__ __launch_bounds__(STATS_WG) void k_adjust_hist(const double* __restrict__ ts, const long long* __restrict__ qcol, long long Mtot,
                                                          const long long* __restrict__ G0, const long long* __restrict__ gm, int jb, int R,
                                                          int d, int w0, long long per, const long long* __restrict__ rem,
                                                          const unsigned long long* __restrict__ pre, unsigned long long* __restrict__ ghist) {
    __shared__ unsigned long long hist[ADJ_RB][GROUP_BINS];
    const int w = w0 + blockIdx.x, g = w / jb, jj = w - g * jb, tid = threadIdx.x;
    const int r0 = blockIdx.z * ADJ_RB, nr = min(ADJ_RB, R - r0);
    int shift, width;
    unsigned long long known;
    group_digit(d, shift, width, known);
    const unsigned dmask = (1u << width) - 1u;
    unsigned long long p[ADJ_RB];
    bool on[ADJ_RB], any = false;
    for (int r = 0; r < ADJ_RB; ++r) {
        on[r] = r < nr && rem[(size_t)w * R + r0 + r] >= 0;
        p[r] = on[r] ? pre[(size_t)w * R + r0 + r] : 0ull;
        any |= on[r];
    }
    if (!any) return;
    const double* x = ts + (size_t)jj * Mtot + G0[g];
    const long long* q = qcol + G0[g];
    const long long m = gm[g];
    for (int i = tid; i < ADJ_RB * GROUP_BINS; i += STATS_WG) (&hist[0][0])[i] = 0ull;
    __syncthreads();
    for (long long b0 = (long long)blockIdx.y * per; b0 < m; b0 += (long long)gridDim.y * per)   // the workgroup's blocks of per rows
        for (long long i = b0 + tid; i < min(b0 + per, m); i += STATS_WG) {
            const long long qi = q[i];
            if (qi == 0) continue;
            const unsigned long long key = stats_key(x[i]);
            const int bin = (int)((key >> shift) & dmask);
            for (int r = 0; r < ADJ_RB; ++r)
                if (on[r] && (key & known) == p[r]) atomicAdd(&hist[r][bin], (unsigned long long)qi);
        }
    __syncthreads();
    for (int r = 0; r < nr; ++r) {
        unsigned long long* gh = ghist + ((size_t)blockIdx.x * R + r0 + r) * GROUP_BINS;
        for (int b = tid; b < GROUP_BINS; b += STATS_WG)
            if (hist[r][b]) atomicAdd(&gh[b], hist[r][b]);
    }
}

// quant [R][G][np]: the selected keys of the parameters [j0, j0 + jb)
__global__ void k_adjust_finish(const unsigned long long* __restrict__ pre, const int* __restrict__ st, int G, int np, int j0, int jb, int R,
                                double* __restrict__ quant) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= G * jb * R) return;
    const int g = e / (jb * R), jj = (e / R) % jb, r = e % R;
    quant[((size_t)r * G + g) * np + j0 + jj] = st[g] == 0 ? stats_unkey(pre[e]) : __longlong_as_double(0x7ff8000000000000ll);
}
