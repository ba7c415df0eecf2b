// smm_sens_sobol: variance-based global sensitivity — Sobol' first-order (Saltelli 2010) and total-order (Jansen 1999) indices of the
// objective value and of every simulated moment with respect to every parameter, over a box — part of libsmmhip (included by smmhip.hip
// inside its anonymous namespace; gfx950 device code; hiprtc never sees it).  Host side: smm_sobol_host.hpp; contract: include/smmhip.h
// (smm_sens_sobol).  N base points need N (np + 2) independent evaluations: matrix m = 0 is A, 1 is B, 2 + i is A with coordinate i from B.
// Base points go in batches of nb; evaluation m * nb + jj of a launch is matrix m at base point j0 + jj, so that one matrix's outputs are
// contiguous.  Output f of F = nm + 1: 0 is the value, 1 + f' is moment f'.
//   k_eval_sobol      : eval_tile_of on points that are never written: every parameter is u53 of its own Philox block.
//   k_sobol_candidates: the same points as rows, for a user objective's compiled kernel.
//   k_sobol_centre    : one workgroup: the pilot's valid evaluations, a lane per output walking them in j order.
//   k_sobol_valid     : a lane per evaluation of a launch: invalid ones counted and their base point flagged; matrix A's outputs out to the
//                       resident yA.
//   k_sobol_terms     : THE HOT PATH, O(N x np x F).  A workgroup owns one block of T (256 consecutive base points, the part of it the launch
//                       holds) and 16 pairs (i, f).  The order of T binds only the additions: everything before them is done by all 256
//                       lanes at once, a lane per base point — the base point is the fastest index of every column of the built-in
//                       layout, so every load of yA, yB and yABi is a run of 128 consecutive doubles — and the terms p and q go to LDS,
//                       half a block at a time.  Then one wave walks them in j order, a lane per (pair, sum): 16 pairs x the sums of p,
//                       p^2, q and (q / 2)^2, one dependent addition a step.  A block that began in an earlier launch goes on from the
//                       sums it left.
//   k_sobol_ysum      : a workgroup per block of T over the resident yA, sixteen outputs at a time through LDS: the block sums of yA, then
//                       of (yA - mean)^2.
//   k_sobol_fold      : a lane per output: block sums left to right, divided by n.
//   k_sobol_finish    : a lane per pair: its block sums left to right, the divisions and the square roots.
// Every operation is rounded on its own (-ffp-contract=off).
#pragma once

constexpr int SOBOL_TB = 256;      // T's block: base points whose terms are added left to right into one block sum
constexpr int SOBOL_WG = 256;      // the workgroup of k_sobol_centre and k_sobol_fold
constexpr int SOBOL_PG = 16;      // pairs (i, f) a workgroup of the term kernel owns: with the four sums of each, one wave walks them
constexpr int SOBOL_HB = 128;      // base points it stages at a time: half a block of T
constexpr int SOBOL_LD = SOBOL_PG + 1;
constexpr int SOBOL_PILOT = 256;   // the pilot: base points whose A evaluations give the centre
constexpr int SOBOL_YF = 16;       // outputs k_sobol_ysum stages at a time
constexpr int SOBOL_SUMS = 4;      // p, p^2, q, (q / 2)^2
static_assert(2 * SOBOL_HB == SOBOL_TB && SOBOL_SUMS * SOBOL_PG == 64, "k_sobol_terms: two halves of its lanes stage half the pairs each; one wave walks");
static_assert(SOBOL_PILOT <= SOBOL_WG && MAX_DIM + 1 <= SOBOL_WG, "k_sobol_centre takes a lane per evaluation, then per output");

struct SobolArgs {
    int N, np, F;
    const double* lo;                 // [np] the box
    const double* hi;
    EvalScratch E;                    // one launch's scratch (smm_evalscratch.hpp)
    double* yA;                       // [F][N]  matrix A's outputs
    int32_t* bad;                     // [N]     not 0: an evaluation of this base point is invalid
    double* centre;                   // [F]
    double* bs;                       // [blocks of T][SOBOL_SUMS][pairs] the pairs' block sums
    double* ys;                       // [blocks of T][F] the block sums of yA, then of its squared deviations
    double* mean;                     // [F]
    double* var;                      // [F]
    double* res;                      // [6][F][np] first, total, v_first, v_total, se_first, se_total
    long long* counts;                // n_complete, n_invalid
};

// parameter k of base point j in matrix m
__device__ inline double sobol_point(const KParams& P, const SobolArgs& A, const int j, const int m, const int k) {
    const uint32_t from_b = (m == 1 || m == k + 2) ? 1u : 0u;
    const smm::U4 x = smm::philox_stream(P.seed, smm::STREAM_GSA, (uint32_t)j, from_b, (uint32_t)(k >> 1), 0u);
    const double u = (k & 1) ? smm::u53(x.z, x.w) : smm::u53(x.x, x.y);
    const double lok = A.lo[k], span = A.hi[k] - lok;
    const double sc = u * span;
    return sc + lok;   // mapto_ab
}
// output f of evaluation i of n
__device__ inline double sobol_y(const EvalScratch& E, const size_t n, const size_t i, const int f) { return f == 0 ? E.value_of(i) : E.mom(n, i, f - 1); }
__device__ inline bool sobol_finite(const double y) { return __builtin_fabs(y) <= 1.7976931348623157e308; }
// (pair p of F x np is output f = p / np and parameter i = p % np, as in the results)

template <int KIND, int CT>
__global__ __launch_bounds__(WG, 4) void k_eval_sobol(const KParams P, const SobolArgs A, const int j0, const int nb, const int n, int8_t* __restrict__ status) {
    eval_tile_of<KIND, CT>(P, n, [&](const int ie, const int k) {
        const int m = ie / nb;
        return sobol_point(P, A, j0 + (ie - m * nb), m, k);
    }, A.E, status);
}

// one thread per (evaluation, parameter)
__global__ __launch_bounds__(256) void k_sobol_candidates(const KParams P, const SobolArgs A, const int j0, const int nb, const int n) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int np = A.np;
    if (t >= (size_t)n * (size_t)np) return;
    const int i = (int)(t / (size_t)np), k = (int)(t % (size_t)np);
    const int m = i / nb;
    A.E.put_cand((size_t)n, (size_t)i, k, sobol_point(P, A, j0 + (i - m * nb), m, k));
}

__device__ inline bool sobol_valid(const SobolArgs& A, const size_t n, const size_t i) {
    bool ok = A.E.status_of(i) >= 1;
    for (int f = 0; f < A.F; ++f) ok = ok && sobol_finite(sobol_y(A.E, n, i, f));
    return ok;
}

// the pilot's n <= SOBOL_PILOT evaluations of matrix A: centre_f = T(y_f over the valid ones) / their number, 0.0 without one
__global__ __launch_bounds__(SOBOL_WG) void k_sobol_centre(const SobolArgs A, const int n) {
    __shared__ int ok[SOBOL_PILOT];
    const int tid = (int)threadIdx.x;
    if (tid < n) ok[tid] = sobol_valid(A, (size_t)n, (size_t)tid) ? 1 : 0;
    __syncthreads();
    if (tid >= A.F) return;
    double blk = 0.0;
    int cnt = 0;
    for (int j = 0; j < n; ++j)
        if (ok[j]) { blk = blk + sobol_y(A.E, (size_t)n, (size_t)j, tid); ++cnt; }
    const double t = 0.0 + blk;   // (T: one block)
    A.centre[tid] = cnt ? t / (double)cnt : 0.0;
}

__global__ __launch_bounds__(256) void k_sobol_valid(const SobolArgs A, const int j0, const int nb, const int n) {
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    bool invalid = false;
    if (i < n) {
        const int m = i / nb, j = j0 + (i - m * nb);
        bool ok = A.E.status_of((size_t)i) >= 1;
        for (int f = 0; f < A.F; ++f) {
            const double y = sobol_y(A.E, (size_t)n, (size_t)i, f);
            ok = ok && sobol_finite(y);
            if (m == 0) A.yA[(size_t)f * A.N + j] = y;
        }
        invalid = !ok;
        if (invalid) atomicOr(&A.bad[j], 1);
    }
    const unsigned long long b = __ballot(invalid);   // (integer counts: no order to keep)
    if (b && ((int)threadIdx.x & 63) == 0) atomicAdd((unsigned long long*)&A.counts[1], (unsigned long long)__popcll(b));
}

// The launch's part of block b of T for the SOBOL_PG pairs of blockIdx.y.  Staging, every lane: base point j of the half block, eight of
// the pairs: p and q of (pair, j) into LDS, 0.0 for an incomplete point — a sum that starts from +0.0 never is -0.0, so adding +0.0 to it
// changes no bit: the same as skipping.  Walk, one wave: lane = (sum, pair) adds its 128 terms in j order.
__global__ __launch_bounds__(SOBOL_TB) void k_sobol_terms(const SobolArgs A, const int j0, const int nb, const int n) {
    __shared__ double tpq[2 * SOBOL_HB * SOBOL_LD];   // [p, q][base point of the half block][pair]
    const int tid = (int)threadIdx.x, np = A.np, NP = A.F * np;
    const int b = j0 / SOBOL_TB + (int)blockIdx.x;
    const int jb = max(j0, b * SOBOL_TB), je = min(j0 + nb, (b + 1) * SOBOL_TB);
    const int p0 = (int)blockIdx.y * SOBOL_PG;
    const size_t ns = (size_t)n, nbs = (size_t)nb;
    const int sjj = tid & (SOBOL_HB - 1), slp = (tid / SOBOL_HB) * (SOBOL_PG / 2);   // staging: this lane's base point and its first pair
    const int wlp = tid & (SOBOL_PG - 1), which = tid / SOBOL_PG;                     // walk (tid < 4 SOBOL_PG): this lane's pair and sum
    const bool walker = tid < SOBOL_SUMS * SOBOL_PG && p0 + wlp < NP;
    double* const out = A.bs + ((size_t)b * SOBOL_SUMS + (size_t)(which & 3)) * NP + p0 + wlp;
    double s = 0.0;
    if (walker && jb > b * SOBOL_TB) s = *out;   // (the block began in an earlier launch)
    const double* const tab = tpq + (which >> 1 & 1) * (SOBOL_HB * SOBOL_LD) + wlp;
    const double scale = which == 3 ? 0.5 : 1.0;
    const bool squared = (which & 1) != 0;
    for (int js = jb; js < je; js += SOBOL_HB) {
        const int j = js + sjj;
        if (j < je) {
            const size_t e = (size_t)(j - j0);
            const bool skip = A.bad[j] != 0;
#pragma unroll 4
            for (int k = 0; k < SOBOL_PG / 2; ++k) {
                const int p = p0 + slp + k;
                double pt = 0.0, qt = 0.0;
                if (p < NP && !skip) {
                    const int f = p / np, i = p - f * np;   // (the same in every lane)
                    const double ya = sobol_y(A.E, ns, e, f), yb = sobol_y(A.E, ns, nbs + e, f), yab = sobol_y(A.E, ns, (size_t)(2 + i) * nbs + e, f);
                    const double d = yab - ya, g = yb - A.centre[f];
                    pt = g * d;
                    const double dq = ya - yab;
                    qt = dq * dq;
                }
                tpq[sjj * SOBOL_LD + slp + k] = pt;
                tpq[(SOBOL_HB + sjj) * SOBOL_LD + slp + k] = qt;
            }
        }
        __syncthreads();
        if (walker) {
            const int cnt = min(SOBOL_HB, je - js);
            for (int jj = 0; jj < cnt; ++jj) {
                const double y = tab[jj * SOBOL_LD] * scale;   // p, p, q, q / 2
                s = s + (squared ? y * y : y);
            }
        }
        __syncthreads();
    }
    if (walker) *out = s;
}

// the base points without an invalid evaluation: n_complete
__global__ __launch_bounds__(COMPACT_WG) void k_sobol_count(const SobolArgs A) {
    __shared__ int tot;
    if (threadIdx.x == 0) tot = 0;
    __syncthreads();
    int mine = 0;
    for (int j = (int)threadIdx.x; j < A.N; j += COMPACT_WG) mine += A.bad[j] ? 0 : 1;
    atomicAdd(&tot, mine);
    __syncthreads();
    if (threadIdx.x == 0) A.counts[0] = (long long)tot;
}

// block b of T over the resident yA: mode 0 the block sum of y, mode 1 of (y - mean)^2; incomplete base points skipped
__global__ __launch_bounds__(SOBOL_TB) void k_sobol_ysum(const SobolArgs A, const int mode) {
    __shared__ double tile[SOBOL_TB * (SOBOL_YF + 1)];
    const int tid = (int)threadIdx.x, b = (int)blockIdx.x;
    const int jb = b * SOBOL_TB, cnt = min(SOBOL_TB, A.N - jb);
    for (int f0 = 0; f0 < A.F; f0 += SOBOL_YF) {
        const int nf = min(SOBOL_YF, A.F - f0);
        if (tid < cnt)
            for (int fl = 0; fl < nf; ++fl) tile[tid * (SOBOL_YF + 1) + fl] = A.yA[(size_t)(f0 + fl) * A.N + jb + tid];
        __syncthreads();
        if (tid < nf) {
            const double mu = mode ? A.mean[f0 + tid] : 0.0;
            double blk = 0.0;
            for (int jj = 0; jj < cnt; ++jj) {
                if (A.bad[jb + jj]) continue;
                const double y = tile[jj * (SOBOL_YF + 1) + tid];
                if (mode) { const double dv = y - mu; blk = blk + dv * dv; }
                else blk = blk + y;
            }
            A.ys[(size_t)b * A.F + f0 + tid] = blk;
        }
        __syncthreads();
    }
}

// dst_f = (ys' block sums of output f, left to right from 0.0) / n
__global__ __launch_bounds__(SOBOL_WG) void k_sobol_fold(const SobolArgs A, const int nblk, double* __restrict__ dst) {
    const int f = (int)threadIdx.x;
    if (f >= A.F) return;
    double t = 0.0;
    for (int b = 0; b < nblk; ++b) t = t + A.ys[(size_t)b * A.F + f];
    dst[f] = t / (double)A.counts[0];
}

__global__ __launch_bounds__(256) void k_sobol_finish(const SobolArgs A, const int nblk) {
    const int p = (int)blockIdx.x * 256 + (int)threadIdx.x, NP = A.F * A.np;
    if (p >= NP) return;
    const int f = p / A.np;
    double tp = 0.0, tpp = 0.0, tq = 0.0, thh = 0.0;
    for (int b = 0; b < nblk; ++b) {
        const double* s = A.bs + (size_t)b * SOBOL_SUMS * NP + p;
        tp = tp + s[0]; tpp = tpp + s[NP]; tq = tq + s[2 * (size_t)NP]; thh = thh + s[3 * (size_t)NP];
    }
    const double nd = (double)A.counts[0], var = A.var[f];
    const double vf = tp / nd, vt = tq / (2.0 * nd);
    double rf = tpp / nd - vf * vf, rt = thh / nd - vt * vt;
    if (rf < 0.0) rf = 0.0;
    if (rt < 0.0) rt = 0.0;
    const size_t at = (size_t)p, R = (size_t)NP;
    A.res[at] = vf / var;
    A.res[R + at] = vt / var;
    A.res[2 * R + at] = vf;
    A.res[3 * R + at] = vt;
    A.res[4 * R + at] = __builtin_sqrt(rf / nd) / var;   // (IEEE square root: correctly rounded)
    A.res[5 * R + at] = __builtin_sqrt(rt / nd) / var;
}
