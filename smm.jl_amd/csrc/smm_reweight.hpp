// the target posterior from every temperature (smm_get_reweighted, include/smmhip.h) — part of libsmmhip (included by smmhip.hip inside
// its anonymous namespace after smm_adjust.hpp; gfx950 device code).  Reads the history records, the chains' acc_tuner in the chain state
// blocks (cs [N][CSW], CS_ATUN) and nothing else; writes only the scratch and result buffers of the call.  A chain's scored rows (selected
// by the walk of smm_window.hpp, value finite) are packed behind one another in the pooled index space exactly as k_group_gather packs the
// selected ones: member i from off[i], its group's column cut into chunks of STATS_LDS_N rows from the group's first scored row.  The single
// sums are k_group_chunk_sum's added by k_adjust_sum_acc, the means k_adjust_means', the pair sums k_cov_pairs' (raw) added by
// k_moment_cov_acc, the weighted select k_adjust_targets / k_adjust_hist / k_group_pick / k_adjust_finish.  What is the call's own:
//
//   k_rw_walk   : one workgroup per chain walks the window once per form, 256 iterations at a time (lane = iteration): the rows of select
//                 0 / 1 directly, the state rows of select 2 through state_before and state_scan; both the selected and the scored rows
//                 ranked by one block_rank.  Counting form: the chain's selected and scored rows.  Index form: the history row, the chain
//                 and the value of every scored row to the packed columns src, rowc and vcol at off[c] + rank, so that no later pass
//                 walks the window again and the targets run over the same columns.
//   k_rw_chain  : the per-chain pass.  One workgroup per member chain with a scored row, one target per launch.  lw = d v; L = max lw
//                 over the lanes, the waves (shuffles) and the workgroup (LDS): a maximum does not depend on the order; w = smm_exp(lw - L)
//                 to the packed column wcol; sw and sw2 by pw_sum (the chain-stats pairwise order, chunks of STATS_LDS_N from the chain's
//                 first scored row, added in order); f_c, L, chain_ess and chain_logz.
//   k_rw_group  : one lane per group: F = the largest f_c among the members with a scored row, and whether a member's L is not finite.
//   k_rw_rows   : the row pass.  One lane per pooled row of a batch of chunks (lane = row: every column is written coalesced).  mode 1:
//                 u = w f_c; the chunk's columns [D + 3][nb][STATS_LDS_N] = u theta_j, u s_k, u v, u, u u; q to its packed column; the rows
//                 with u > 0 and their q counted per workgroup in LDS, then by one 64-bit atomic each; a parameter that is not finite
//                 raises gbad.  mode 2: the first np columns = sqrt(u) (theta_j - mean_j).  mode 3: theta_j of the parameters [j0, j0 + jb)
//                 to the packed columns ts [jb][Mtot] the weighted select reads.
//   k_rw_finish : one workgroup of one wave per group: the status of (target, group) and its results, or NaN.
#pragma once

constexpr int RW_WG = 256;
static_assert(RW_WG == WINDOW_WG && RW_WG == STATS_WG && STATS_LDS_N % RW_WG == 0,
              "k_rw_walk walks with smm_window.hpp, k_rw_chain sums with pw_sum; a workgroup of k_rw_rows lies inside one chunk");

// cnt [2][N]: the selected rows, then the scored rows of every chain (0 for a chain outside every group).  counting == 0: the chains with
// a scored row write theirs to src / rowc / vcol at off[c] + rank.
__global__ __launch_bounds__(RW_WG) void k_rw_walk(const double* __restrict__ hrec, int N, int HW, int t0, int n, int sel,
                                                   const int* __restrict__ gid, const long long* __restrict__ off, int counting,
                                                   int* __restrict__ cnt, int* __restrict__ src, int* __restrict__ rowc,
                                                   double* __restrict__ vcol) {
    __shared__ int wtot[2][RW_WG / 64];
    __shared__ int wred[RW_WG / 64];
    const int c = xcd_chain(blockIdx.x, gridDim.x), tid = threadIdx.x;
    if (gid[c] < 0) {
        if (counting && tid == 0) { cnt[c] = 0; cnt[N + c] = 0; }
        return;
    }
    if (!counting && cnt[N + c] == 0) return;
    const long long o = counting ? 0 : off[c];
    int carry = sel == 2 ? state_before(hrec, N, HW, c, t0, wred) : -1;
    int base[2] = {0, 0};
    for (int r0 = 0; r0 < n; r0 += RW_WG) {
        const int r = r0 + tid, t = t0 + r;
        const bool valid = r < n;
        const bool acc = valid && hrec[((size_t)t * N + c) * HW + H_ACC] != 0.0;
        int a = (valid && (sel == 0 || acc)) ? t : -1;   // the history row this lane contributes (-1: none)
        if (sel == 2) a = state_scan(acc ? t : -1, carry, wred);
        double v = 0.0;
        if (valid && a >= 0) v = hrec[((size_t)a * N + c) * HW + H_VALUE];
        const bool flag[2] = {valid && (sel == 2 || a >= 0), valid && a >= 0 && isfinite(v)};   // (|v| <= DBL_MAX)
        int pos[2];
        block_rank(flag, wtot, base, pos);
        if (!counting && flag[1]) {
            src[o + pos[1]] = a;
            rowc[o + pos[1]] = c;
            vcol[o + pos[1]] = v;
        }
    }
    if (counting && tid == 0) { cnt[c] = base[0]; cnt[N + c] = base[1]; }
}

// grid: the member chains with a scored row (act); fc, Lc [N]; o_ess, o_logz: the target's rows [N] of the results (NULL: not asked for)
__global__ __launch_bounds__(RW_WG) void k_rw_chain(const int* __restrict__ act, const long long* __restrict__ off,
                                                    const int* __restrict__ nsc, const double* __restrict__ cs,
                                                    const double* __restrict__ vcol, double target, double* __restrict__ wcol,
                                                    double* __restrict__ fc, double* __restrict__ Lc, double* __restrict__ o_ess,
                                                    double* __restrict__ o_logz) {
    extern __shared__ __align__(16) double sx[];   // STATS_LDS_N
    __shared__ PwTree pt;
    __shared__ double wmax[RW_WG / 64];
    const int c = act[blockIdx.x], tid = threadIdx.x, m = nsc[c];
    const double d = cs[(size_t)c * CSW + CS_ATUN] - target;
    const double* v = vcol + off[c];
    double* w = wcol + off[c];
    double L = -__builtin_huge_val();
    for (int i = tid; i < m; i += RW_WG) {
        const double lw = d * v[i];
        L = lw > L ? lw : L;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double y = __shfl_xor(L, o, 64);
        L = y > L ? y : L;
    }
    if ((tid & 63) == 0) wmax[tid >> 6] = L;
    __syncthreads();
    L = wmax[0];
    for (int q = 1; q < RW_WG / 64; ++q) L = wmax[q] > L ? wmax[q] : L;
    const double sw = pw_sum(m, [&](int i) {
        const double lw = d * v[i];
        const double x = lw - L;
        const double wi = smm_exp(x);   // (1.0 at 0.0, 0.0 at -inf, NaN at NaN)
        w[i] = wi;
        return wi;
    }, sx, pt);
    const double sw2 = pw_sum(m, [&](int i) { const double wi = w[i]; return wi * wi; }, sx, pt);   // (a lane reads what it wrote)
    if (tid == 0) {
        fc[c] = sw / sw2;
        Lc[c] = L;
        if (o_ess) o_ess[c] = (sw * sw) / sw2;
        if (o_logz) o_logz[c] = L + smm_log(sw / (double)m);
    }
}

// mem, gmem0: the groups' members; F [G], bad3 [G]
__global__ void k_rw_group(const int* __restrict__ mem, const int* __restrict__ gmem0, const int* __restrict__ nsc,
                           const double* __restrict__ fc, const double* __restrict__ Lc, int G, double* __restrict__ F,
                           int* __restrict__ bad3) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    double f = 0.0;
    int bad = 0;
    for (int i = gmem0[g]; i < gmem0[g + 1]; ++i) {
        const int c = mem[i];
        if (nsc[c] == 0) continue;
        if (fc[c] > f) f = fc[c];
        if (!isfinite(Lc[c])) bad = 1;
    }
    F[g] = f;
    bad3[g] = bad;
}

struct RwRows {   // what the row passes share: the batch of chunks in the scratch and where its rows come from
    double* buf;                 // [D + 3][nb][STATS_LDS_N]
    int nb, cb0, np, nm, N, HW;
    const int* clen;             // [NC] rows of a chunk
    const int* cgrp;             // [NC] its group
    const long long* cst;        // [NC] its first row in the pooled index space
    const double* hrec;
    const int *src, *rowc;       // [Mtot] the history row and the chain of a pooled row
    const double *vcol, *wcol;   // [Mtot] its value and its weight w
    const double* fc;            // [N]
    const double* F;             // [G]
};

// grid (STATS_LDS_N / RW_WG, nb).  mode 3: ts [jb][Mtot] (buf unused)
__global__ __launch_bounds__(RW_WG) void k_rw_rows(RwRows a, int mode, const double* __restrict__ mu, long long* __restrict__ qcol,
                                                   unsigned long long* __restrict__ nkept, unsigned long long* __restrict__ qsum,
                                                   int* __restrict__ gbad, int j0, int jb, long long Mtot, double* __restrict__ ts) {
    __shared__ unsigned long long skept, sq;
    const int cl = blockIdx.y, ch = a.cb0 + cl, pos = blockIdx.x * RW_WG + threadIdx.x, D = a.np + a.nm;
    if (blockIdx.x * RW_WG >= a.clen[ch]) return;   // (the whole workgroup)
    const bool row = pos < a.clen[ch];
    const int g = a.cgrp[ch];
    const size_t cs = (size_t)a.nb * STATS_LDS_N, at = (size_t)cl * STATS_LDS_N + pos;
    if (mode == 1 && threadIdx.x == 0) { skept = 0; sq = 0; }
    if (mode == 1) __syncthreads();
    if (row) {
        const long long prow = a.cst[ch] + pos;
        const int c = a.rowc[prow];
        const double* h = a.hrec + ((size_t)a.src[prow] * a.N + c) * a.HW + H_PARAMS;
        if (mode == 3) {
            for (int jj = 0; jj < jb; ++jj) ts[(size_t)jj * Mtot + prow] = h[j0 + jj];
        } else {
            const double u = a.wcol[prow] * a.fc[c];
            if (mode == 1) {
                bool bad = false;
                for (int j = 0; j < D; ++j) {
                    const double x = h[j];
                    if (j < a.np) bad |= !isfinite(x);
                    a.buf[(size_t)j * cs + at] = u * x;
                }
                if (bad) gbad[g] = 1;
                a.buf[(size_t)D * cs + at] = u * a.vcol[prow];
                a.buf[(size_t)(D + 1) * cs + at] = u;
                a.buf[(size_t)(D + 2) * cs + at] = u * u;
                long long q = 0;
                if (u > 0.0) {
                    const double s = u / a.F[g];
                    q = (long long)ceil(s * 1048576.0);
                    atomicAdd(&skept, 1ull);
                    atomicAdd(&sq, (unsigned long long)q);
                }
                qcol[prow] = q;
            } else {
                const double r = sqrt(u);
                const double* m = mu + (size_t)g * (D + 1);
                for (int j = 0; j < a.np; ++j) {
                    const double e = h[j] - m[j];
                    a.buf[(size_t)j * cs + at] = r * e;
                }
            }
        }
    }
    if (mode == 1) {
        __syncthreads();
        if (threadIdx.x == 0 && skept) { atomicAdd(&nkept[g], skept); atomicAdd(&qsum[g], sq); }
    }
}

struct RwOut {   // the target's rows of the call's results on the device (NULL: not asked for)
    int* status;
    long long* n_kept;
    double *sum_u, *ess, *mean, *cov, *value_mean, *m_mean;
};

// sums [G][D + 3] (columns D + 1, D + 2: the sums of u and of u u), mu [G][D + 1], acc [G][np][np] (a >= b); st [G]: the call's own copy
// of the status for the select
__global__ __launch_bounds__(64) void k_rw_finish(const double* __restrict__ sums, const double* __restrict__ mu,
                                                  const double* __restrict__ acc, const long long* __restrict__ gm,
                                                  const int* __restrict__ gbad, const int* __restrict__ bad3,
                                                  const unsigned long long* __restrict__ nkept, int np, int nm, int* __restrict__ st,
                                                  RwOut o) {
    const int g = blockIdx.x, tid = threadIdx.x, D = np + nm;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    const double su = sums[(size_t)g * (D + 3) + D + 1], su2 = sums[(size_t)g * (D + 3) + D + 2];
    const int status = gm[g] < 2 ? 1 : gbad[g] != 0 ? 2 : (bad3[g] != 0 || !isfinite(su)) ? 3 : 0;
    const bool ok = status == 0;
    const double* m = mu + (size_t)g * (D + 1);
    if (tid == 0) {
        st[g] = status;
        if (o.status) o.status[g] = status;
        if (o.n_kept) o.n_kept[g] = ok ? (long long)nkept[g] : 0;
        if (o.sum_u) o.sum_u[g] = ok ? su : qnan;
        if (o.ess) o.ess[g] = ok ? (su * su) / su2 : qnan;
        if (o.value_mean) o.value_mean[g] = ok ? m[D] : qnan;
    }
    if (o.mean)
        for (int j = tid; j < np; j += 64) o.mean[(size_t)g * np + j] = ok ? m[j] : qnan;
    if (o.m_mean)
        for (int k = tid; k < nm; k += 64) o.m_mean[(size_t)g * nm + k] = ok ? m[np + k] : qnan;
    if (o.cov)
        for (int e = tid; e < np * np; e += 64) {
            const int j = e / np, k = e - j * np, hi = j >= k ? j : k, lo = j >= k ? k : j;
            o.cov[(size_t)g * np * np + e] = ok ? acc[((size_t)g * np + hi) * np + lo] / su : qnan;
        }
}
