// chain covariances and the batched Cholesky of adapted proposals (smm_get_chain_cov, smm_adapt_proposal, include/smmhip.h) — part of
// libsmmhip (included by smmhip.hip inside its anonymous namespace after smm_stats.hpp; gfx950 device code).  The draws come from
// k_stats_gather (smm_stats.hpp) run with every parameter in one batch, so the selection and compaction are smm_get_chain_stats' own.
//
//   k_cov_center : one workgroup per (chain, parameter) column of the compacted scratch col [np][Nb][n]: the draws mapped to [0, 1]
//                  (unit_space; mapto_01, the kernels' arithmetic, in pw_sum's staging), their mean by the chain-stats contract
//                  (pw_sum, smm_stats.hpp), then the column overwritten in place by the centered draws d = u - mean.
//   k_cov_pairs  : one workgroup of COV_WG = 128 lanes per (chain, tile of COV_T x COV_T pairs (j, k), tile row >= tile column).  The
//                  leaves of the pairwise tree of a chunk depend only on the chain's count m: lane 0 lists them once per chunk, with
//                  the number of combines the post-order walk of the tree makes after each leaf (pw_leaves, smm_stats.hpp).  The
//                  tile's centered columns are staged in LDS (rows padded against bank conflicts), COV_G draws at a time, in runs of
//                  whole leaves.  Lane = (2 x 2
//                  block of pairs, accumulator r[a] of the leaf, a = lane & 7): 4 products from 4 LDS reads per step (ds_read_b64 at
//                  32 doubles per clock per CU against
//                  about 64 FP64 adds: the blocked product keeps both busy).  After a leaf the 8 accumulators meet by a butterfly, lane
//                  a = 0 adds the tail, pushes the 4 leaf sums on the pairs' stacks in LDS and makes the leaf's combines there.
//                  raw != 0 writes the sum S instead of S / (m - 1): smm_group.hpp runs it over 8192-draw chunks of pooled columns.
//   k_cov_chol   : one wave per chain, lane = row k (np <= MAX_DIM = 64): A = C / tau (+ ridge on the diagonal) in LDS (32 KB at
//                  np = 64); column j: lane j finishes the pivot, then lanes k > j their entry, each subtracting in i order — the
//                  restatement's order.  The factor goes straight into the chain's rows of P.chol_L, and only where status is 0.
#pragma once

constexpr int COV_WG = 128;           // lanes of k_cov_pairs: 16 blocks of 2 x 2 pairs x 8 accumulators
constexpr int COV_T = 8;              // a tile of pairs: 8 rows j x 8 columns k
constexpr int COV_G = 256;            // draws of the tile's 16 columns staged in LDS at a time (32 KB)
constexpr int COV_STK = 16;           // per-pair combine stack (the tree of 8192 draws is at most 8 levels deep)
// row padding of the staged tile: a wave's 8 blocks read rows {0, 2} (j) and {8, 10, 12, 14} (k) at the same offset, 8 doubles each;
// rows 2 KB apart would share the same 16 of the 64 four-byte banks, rows 2 KB + 32 B apart start 64 B apart: no two collide
constexpr int COV_PAD = 4;

__global__ __launch_bounds__(STATS_WG) void k_cov_center(double* __restrict__ col, int n, int N, int c0, int Nb, int unit,
                                                         const double* __restrict__ lb, const double* __restrict__ ub,
                                                         const int* __restrict__ o_count, double* __restrict__ o_mean) {
    extern __shared__ __align__(16) double sx[];   // min(n, STATS_LDS_N)
    __shared__ PwTree pt;
    const int cl = blockIdx.x, k = blockIdx.y, c = c0 + cl, tid = threadIdx.x;
    double* x = col + ((size_t)k * Nb + cl) * n;
    const int m = o_count[c];
    const double lbk = lb[k], span = ub[k] - lbk;
    const double S = pw_sum(m, [&](int i) {
        double v = x[i];
        if (unit) v = (v - lbk) / span;   // mapto_01, mprob.jl:248
        return v;
    }, sx, pt);
    const double mu = S / (double)m;
    if (tid == 0) o_mean[(size_t)k * N + c] = mu;
    for (int i = tid; i < m; i += STATS_WG) {
        double v = x[i];
        if (unit) v = (v - lbk) / span;
        x[i] = v - mu;
    }
}

__global__ __launch_bounds__(COV_WG) void k_cov_pairs(const double* __restrict__ col, int n, int N, int c0, int Nb, int np,
                                                      const int* __restrict__ o_count, double* __restrict__ o_cov, int raw) {
    __shared__ double sd[2 * COV_T][COV_G + COV_PAD];          // the tile's columns: rows j0.., then columns k0..
    __shared__ double stk[COV_T * COV_T][COV_STK];
    __shared__ int loff[STATS_LEAF_MAX], lnum[STATS_LEAF_MAX], lcomb[STATS_LEAF_MAX];
    __shared__ int tstk[64];
    __shared__ int snl;
    const int cl = blockIdx.x, c = c0 + cl, tid = threadIdx.x;
    // tile (tj, tk), tk <= tj, from the linear index: tj (tj + 1) / 2 + tk
    int tj = 0;
    while ((tj + 1) * (tj + 2) / 2 <= (int)blockIdx.y) ++tj;
    const int tk = blockIdx.y - tj * (tj + 1) / 2;
    const int j0 = tj * COV_T, k0 = tk * COV_T;
    const int a = tid & 7, blk = tid >> 3;                    // accumulator; block of pairs (rows 2 bj, 2 bj + 1) x (columns 2 bk, 2 bk + 1)
    const int bj = blk >> 2, bk = blk & 3;
    const int m = o_count[c];
    const double* xc = col + (size_t)cl * n;                   // column q of the chain: xc + q * Nb * n
    const size_t cstride = (size_t)Nb * n;
    int sp = 0;                                                // stack depth (the same for the 4 pairs, kept by lane a = 0)
    double S[4] = {0.0, 0.0, 0.0, 0.0};
    for (int c8 = 0; c8 < m; c8 += STATS_LDS_N) {
        const int L = min(STATS_LDS_N, m - c8);
        if (tid == 0) snl = pw_leaves(L, loff, lnum, lcomb, tstk);
        __syncthreads();
        const int nl = snl;
        sp = 0;
        int leaf = 0;
        while (leaf < nl) {
            // a run of whole leaves, at most COV_G draws
            const int g0 = loff[leaf];
            int le = leaf;
            while (le < nl && loff[le] + lnum[le] - g0 <= COV_G) ++le;
            const int gn = loff[le - 1] + lnum[le - 1] - g0;
            for (int e = tid; e < 2 * COV_T * gn; e += COV_WG) {
                const int q = e / gn, i = e - q * gn;
                const int qc = min((q < COV_T ? j0 + q : k0 + q - COV_T), np - 1);
                sd[q][i] = xc[qc * cstride + c8 + g0 + i];
            }
            __syncthreads();
            const double* dj0 = sd[2 * bj];
            const double* dj1 = sd[2 * bj + 1];
            const double* dk0 = sd[COV_T + 2 * bk];
            const double* dk1 = sd[COV_T + 2 * bk + 1];
            for (int lf = leaf; lf < le; ++lf) {
                const int lo = loff[lf] - g0, cnt = lnum[lf];
                double r0 = 0.0, r1 = 0.0, r2 = 0.0, r3 = 0.0;
                if (cnt >= 8) {
                    const int m8 = cnt - cnt % 8;
                    {
                        const double x0 = dj0[lo + a], x1 = dj1[lo + a], y0 = dk0[lo + a], y1 = dk1[lo + a];
                        r0 = x0 * y0; r1 = x0 * y1; r2 = x1 * y0; r3 = x1 * y1;
                    }
                    for (int i = 8; i < m8; i += 8) {
                        const double x0 = dj0[lo + i + a], x1 = dj1[lo + i + a], y0 = dk0[lo + i + a], y1 = dk1[lo + i + a];
                        const double p0 = x0 * y0, p1 = x0 * y1, p2 = x1 * y0, p3 = x1 * y1;
                        r0 = r0 + p0; r1 = r1 + p1; r2 = r2 + p2; r3 = r3 + p3;
                    }
                }
                // ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)) over the 8 accumulator lanes (IEEE addition commutes)
                for (int o = 1; o < 8; o <<= 1) {
                    r0 = r0 + __shfl_xor(r0, o, 64); r1 = r1 + __shfl_xor(r1, o, 64);
                    r2 = r2 + __shfl_xor(r2, o, 64); r3 = r3 + __shfl_xor(r3, o, 64);
                }
                if (a == 0) {
                    double s0, s1, s2, s3;
                    int i = 0;
                    if (cnt < 8) { s0 = s1 = s2 = s3 = 0.0; }
                    else { s0 = r0; s1 = r1; s2 = r2; s3 = r3; i = cnt - cnt % 8; }
                    for (; i < cnt; ++i) {
                        const double x0 = dj0[lo + i], x1 = dj1[lo + i], y0 = dk0[lo + i], y1 = dk1[lo + i];
                        const double p0 = x0 * y0, p1 = x0 * y1, p2 = x1 * y0, p3 = x1 * y1;
                        s0 = s0 + p0; s1 = s1 + p1; s2 = s2 + p2; s3 = s3 + p3;
                    }
                    double* st0 = stk[4 * blk];
                    double* st1 = stk[4 * blk + 1];
                    double* st2 = stk[4 * blk + 2];
                    double* st3 = stk[4 * blk + 3];
                    st0[sp] = s0; st1[sp] = s1; st2[sp] = s2; st3[sp] = s3;
                    ++sp;
                    for (int q = lcomb[lf]; q > 0; --q) {   // left + right
                        --sp;
                        st0[sp - 1] = st0[sp - 1] + st0[sp]; st1[sp - 1] = st1[sp - 1] + st1[sp];
                        st2[sp - 1] = st2[sp - 1] + st2[sp]; st3[sp - 1] = st3[sp - 1] + st3[sp];
                    }
                }
            }
            __syncthreads();
            leaf = le;
        }
        if (a == 0)
            for (int q = 0; q < 4; ++q) S[q] = S[q] + stk[4 * blk + q][0];
        __syncthreads();
    }
    if (a != 0) return;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    const double den = (double)(m - 1);
    for (int q = 0; q < 4; ++q) {
        const int j = j0 + 2 * bj + (q >> 1), k = k0 + 2 * bk + (q & 1);
        if (j >= np || k >= np || k > j) continue;             // (the pairs above the diagonal of a diagonal tile: their mirror writes both)
        const double v = raw ? S[q] : m < 2 ? qnan : S[q] / den;   // (raw: the sum itself, for smm_group.hpp's chunks)
        o_cov[((size_t)j * np + k) * N + c] = v;
        o_cov[((size_t)k * np + j) * N + c] = v;
    }
}

// adapt: status 1 (count < min_draws), 2 (a non-finite entry of C), 3 (a pivot !(s > 0)), else 0 and the factor installed into
// chol_L's rows of global chain gchain = chain_offset + c
__global__ __launch_bounds__(64) void k_cov_chol(const double* __restrict__ cov, const int* __restrict__ o_count, int N, int np,
                                                 int min_draws, int normalize, double ridge, int chain_offset,
                                                 double* __restrict__ chol_L, int* __restrict__ o_status) {
    __shared__ double A[MAX_DIM][MAX_DIM + 1];
    __shared__ int bad;
    const int c = blockIdx.x, k = threadIdx.x;
    if (k == 0) bad = 0;
    __syncthreads();
    if (o_count[c] < min_draws) {
        if (k == 0) o_status[c] = 1;
        return;
    }
    bool nonfinite = false;
    if (k < np)
        for (int j = 0; j < np; ++j) {
            const double v = cov[((size_t)k * np + j) * N + c];
            nonfinite |= !isfinite(v);
            A[k][j] = v;
        }
    if (nonfinite) bad = 1;
    __syncthreads();
    if (bad) {
        if (k == 0) o_status[c] = 2;
        return;
    }
    double tau = 0.0;
    for (int j = 0; j < np; ++j) tau = tau + A[j][j];   // (every lane: the same sum)
    tau = tau / (double)np;
    __syncthreads();
    if (k < np)
        for (int j = 0; j <= k; ++j) {
            double v = normalize ? A[k][j] / tau : A[k][j];
            if (j == k) v = v + ridge;
            A[k][j] = v;
        }
    __syncthreads();
    for (int j = 0; j < np; ++j) {
        if (k == j) {
            double s = A[j][j];
            for (int i = 0; i < j; ++i) {
                const double p = A[j][i] * A[j][i];
                s = s - p;
            }
            if (!(s > 0.0)) bad = 1;
            A[j][j] = sqrt(s);
        }
        __syncthreads();
        if (k > j && k < np) {
            double s = A[k][j];
            for (int i = 0; i < j; ++i) {
                const double p = A[k][i] * A[j][i];
                s = s - p;
            }
            A[k][j] = s / A[j][j];
        }
        __syncthreads();
    }
    if (bad) {
        if (k == 0) o_status[c] = 3;
        return;
    }
    if (k < np) {
        double* Lk = chol_L + ((size_t)(chain_offset + c) * np + k) * np;
        for (int j = 0; j < np; ++j) Lk[j] = j <= k ? A[k][j] : 0.0;
    }
    if (k == 0) o_status[c] = 0;
}
