// smm_abc_pmc: the adaptive population Monte Carlo ABC sampler of Lenormand, Jabot & Deffuant (2013) — part of libsmmhip (included by
// smmhip.hip inside its anonymous namespace; gfx950 device code; hiprtc never sees it).  Host side: smm_pmc_host.hpp; contract:
// include/smmhip.h (smm_abc_pmc).  A generation is one batched evaluation plus reductions; nothing of it depends on a chain.
//   k_pmc_generate : generation 0, a lane per (particle, Philox block): two uniforms of the box.
//   k_pmc_weights  : one workgroup: the kept particles' sampling weights — max lw, q, their exclusive integer prefix, Q, the sum of q^2, wn, ess.
//   k_pmc_mean, k_pmc_pairs : a workgroup per column / per pair: the weighted mean and the pair sums by pw_sum (smm_stats.hpp), in unit space for
//                    the kernel covariance, in parameter space for the summary.
//   k_pmc_chol     : one wave, lane = row: Sigma = scale C + ridge I, moment_chol (k_cov_chol's order), logc.
//   k_pmc_whiten   : a lane per particle: z = L^-1 u by forward substitution, the factor in LDS, every lane reading the same entry; the kept
//                    particles' z once more by particle (kzT [i][NPC]) for the weight kernel.
//   k_pmc_propose  : a lane per new particle: the parent by a binary search of the integer prefix, the normals of its Philox blocks through
//                    LDS, the Cholesky step of smm_propose.hpp, the inside test.
//   k_pmc_gather, k_pmc_scatter : the compacted list of inside particles into a launch's scratch (smm_evalscratch.hpp), and its values back
//                    as distances.
//   k_pmc_kernel   : THE HOT PATH, O(kept x new x np).  One lane owns a new particle with a finite distance, its z in registers (NPC, np rounded up to
//                    a multiple of 4 and padded with zeros, is a template parameter so that they are); blockIdx.y owns one block of PMC_TB consecutive kept
//                    particles.  A kept particle is the same for every lane of a wave, so its row of kzT and its wn come through the scalar
//                    cache into scalar registers and enter the FP64 instructions as scalar operands: nothing goes through LDS and no barrier
//                    stands in the loop.  A lane walks the block in stored order, so that its sum is T's block sum.  The block sums of a pass lie in
//                    part [pass blocks][lanes]; k_pmc_combine adds them to D in block order: grid and scheduling never touch the order.
//   k_pmc_logw     : lw = -(log D + logc), the underflow rule, and the count behind p_acc.
//   k_pmc_select   : one workgroup: A' and the A'-th smallest distance by the radix select of smm_stats.hpp, then the stable compaction of
//                    the candidates (ballots and prefix counts, no atomics), eps, and whether the run goes on.
//   k_pmc_move     : the selected candidates' rows into the other kept set.
//   k_pmc_quantile : a workgroup per (prob, parameter): the inverted integer-weight CDF by a radix select over weighted histograms.
// Every operation is rounded on its own (-ffp-contract=off); smm_exp's own fma are the contract's.
#pragma once

constexpr int PMC_TB = 256;      // T's block: kept particles whose terms are added left to right into one block sum
constexpr int PMC_WG = 256;      // particles per workgroup of k_pmc_kernel
constexpr int PMC_PASS = 64;     // blocks of T per pass: part holds PMC_PASS x lanes doubles
constexpr int PMC_W_WG = 1024;   // k_pmc_weights' workgroup
static_assert(PMC_WG == STATS_WG, "k_pmc_select and the sums run on smm_stats.hpp's workgroup");

// what the kernels of a call share beside the particles: counts the host reads, and the generation's scalars
struct PmcCtl {
    int32_t stop;        // -1 the run goes on, else the final status
    int32_t nk;          // A': the kept particles
    int32_t n_inside;    // new particles inside the box
    int32_t n_w;         // new particles with a finite distance
    int32_t n_acc;       // new particles with a distance below the previous eps
    int32_t pad;
    long long Q;         // the sum of q
    double eps, ess, logc;
};

// the per-generation outputs kept on the device, [max_gen + 1] each
struct PmcGen {
    double *eps, *p_acc, *ess;
    int32_t *n_invalid, *n_underflow, *n_new_kept;
};

__device__ inline double pmc_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// generation 0: particle j, parameters 2q and 2q + 1 from the block at counter {j, 0, q, 0}
__global__ __launch_bounds__(256) void k_pmc_generate(const KParams P, const int n, const size_t stride, double* __restrict__ u, double* __restrict__ theta) {
    const int np = P.np, nq = (np + 1) / 2;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)n * nq) return;
    const int q = (int)(e / (size_t)n), j = (int)(e - (size_t)q * n);
    const smm::U4 x = smm::philox_stream(P.seed, smm::STREAM_PMC, (uint32_t)j, 0u, (uint32_t)q, 0u);
    const double uu[2] = {smm::u53(x.x, x.y), smm::u53(x.z, x.w)};
    for (int h = 0; h < 2; ++h) {
        const int k = 2 * q + h;
        if (k >= np) break;
        const double lbk = P.lb[k], span = P.ub[k] - lbk;
        const double sc = uu[h] * span;
        u[(size_t)k * stride + j] = uu[h];
        theta[(size_t)k * stride + j] = sc + lbk;   // mapto_ab
    }
}

// evaluations [off, off + n) of the list (nullptr: the particles themselves) into the launch's scratch (smm_evalscratch.hpp)
__global__ __launch_bounds__(256) void k_pmc_gather(const EvalScratch E, const int32_t* __restrict__ list, const int off, const int n,
                                                    const double* __restrict__ theta, const size_t stride) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)n * E.np) return;
    const int k = (int)(e / (size_t)n), i = (int)(e - (size_t)k * n);
    const int j = list ? list[off + i] : off + i;
    E.put_cand((size_t)n, (size_t)i, k, theta[(size_t)k * stride + j]);
}

// ... and back: the distance is the value where the status is >= 1 and |value| <= DBL_MAX, else +inf and the particle counts as invalid
__global__ __launch_bounds__(256) void k_pmc_scatter(const EvalScratch E, const int32_t* __restrict__ list, const int off, const int n,
                                                     double* __restrict__ rho, double* __restrict__ mom, const size_t stride, int32_t* __restrict__ flagw,
                                                     int32_t* __restrict__ n_invalid) {
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= n) return;
    const int j = list ? list[off + i] : off + i;
    const int st = E.status_of((size_t)i);
    const double v = E.value_of((size_t)i);
    const bool ok = st >= 1 && __builtin_fabs(v) <= 1.7976931348623157e308;
    rho[j] = ok ? v : __builtin_huge_val();
    flagw[j] = ok ? 1 : 0;
    if (!ok) atomicAdd(n_invalid, 1);
    for (int f = 0; f < E.nm; ++f) mom[(size_t)f * stride + j] = E.mom((size_t)n, (size_t)i, f);
}

// the sampling weights of the kept set (nk = ctl->nk particles, lw): M = max lw, w = smm_exp(lw - M), q = (int64) ceil(w 2^20) >= 1, pre their
// exclusive prefix, Q, wn = q / Q, ess = (Q Q) / sum q^2.  Integer sums: no order.  nk == 0: ess NaN
__global__ __launch_bounds__(PMC_W_WG) void k_pmc_weights(PmcCtl* __restrict__ ctl, const double* __restrict__ lw, long long* __restrict__ q,
                                                          long long* __restrict__ pre, double* __restrict__ wn, double* __restrict__ gen_ess) {
    __shared__ double wmax[PMC_W_WG / 64];
    __shared__ long long wsum[PMC_W_WG / 64];
    __shared__ long long base;
    __shared__ unsigned long long sq2;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, nk = ctl->nk;
    if (nk == 0) {
        if (tid == 0) { ctl->Q = 0; ctl->ess = pmc_nan(); *gen_ess = pmc_nan(); }
        return;
    }
    double m = -__builtin_huge_val();
    for (int i = tid; i < nk; i += PMC_W_WG) { const double x = lw[i]; m = x > m ? x : m; }
    for (int off = 32; off >= 1; off >>= 1) { const double o = __shfl_xor(m, off); m = o > m ? o : m; }
    if (lane == 0) wmax[wave] = m;
    if (tid == 0) { base = 0; sq2 = 0ull; }
    __syncthreads();
    for (int w = 0; w < PMC_W_WG / 64; ++w) m = wmax[w] > m ? wmax[w] : m;
    unsigned long long my2 = 0ull;
    for (int i0 = 0; i0 < nk; i0 += PMC_W_WG) {
        const int i = i0 + tid;
        long long qi = 0;
        if (i < nk) {
            const double x = lw[i] - m;
            const double w = smm::smm_exp(x);
            qi = (long long)ceil(w * 1048576.0);
            if (qi < 1) qi = 1;
            q[i] = qi;
            my2 += (unsigned long long)qi * (unsigned long long)qi;
        }
        long long inc = qi;
        for (int o = 1; o < 64; o <<= 1) { const long long y = __shfl_up(inc, o, 64); if (lane >= o) inc += y; }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        long long before = base;
        for (int w = 0; w < wave; ++w) before += wsum[w];
        if (i < nk) pre[i] = before + inc - qi;
        __syncthreads();
        if (tid == 0) { long long t = base; for (int w = 0; w < PMC_W_WG / 64; ++w) t += wsum[w]; base = t; }
        __syncthreads();
    }
    for (int off = 32; off >= 1; off >>= 1) my2 += __shfl_xor(my2, off);
    if (lane == 0) atomicAdd(&sq2, my2);
    __syncthreads();
    const long long Q = base;
    const double Qd = (double)Q;
    for (int i = tid; i < nk; i += PMC_W_WG) wn[i] = (double)q[i] / Qd;   // (a lane reads the q it wrote)
    if (tid == 0) {
        const double ess = (Qd * Qd) / (double)(long long)sq2;
        ctl->Q = Q; ctl->ess = ess; *gen_ess = ess;
    }
}

// column k = blockIdx.x of x [.][stride]: mean_k = S(wn_i x_ik) over the nk kept, S the chunked pairwise sum.  Nothing runs once the run has stopped
// unless `always` (the summary)
__global__ __launch_bounds__(STATS_WG) void k_pmc_mean(const PmcCtl* __restrict__ ctl, const int always, const double* __restrict__ wn,
                                                       const double* __restrict__ x, const size_t stride, double* __restrict__ mean) {
    extern __shared__ __align__(16) double sx[];   // STATS_LDS_N
    __shared__ PwTree pt;
    if (!always && ctl->stop >= 0) return;
    const int k = (int)blockIdx.x, nk = ctl->nk;
    const double* __restrict__ xk = x + (size_t)k * stride;
    const double s = pw_sum(nk, [&](int i) { return wn[i] * xk[i]; }, sx, pt);
    if (threadIdx.x == 0) mean[k] = nk > 0 ? s : pmc_nan();
}

// pair blockIdx.x = a (a + 1) / 2 + b, b <= a: C_ab = C_ba = S(e_ia e_ib), e_ik = sqrt(wn_i) (x_ik - mean_k)
__global__ __launch_bounds__(STATS_WG) void k_pmc_pairs(const PmcCtl* __restrict__ ctl, const int always, const int np, const double* __restrict__ wn,
                                                        const double* __restrict__ x, const size_t stride, const double* __restrict__ mean,
                                                        double* __restrict__ C) {
    extern __shared__ __align__(16) double sx[];   // STATS_LDS_N
    __shared__ PwTree pt;
    if (!always && ctl->stop >= 0) return;
    int a = 0;
    const int pr = (int)blockIdx.x, nk = ctl->nk;
    while ((a + 1) * (a + 2) / 2 <= pr) ++a;
    const int b = pr - a * (a + 1) / 2;
    const double* __restrict__ xa = x + (size_t)a * stride;
    const double* __restrict__ xb = x + (size_t)b * stride;
    const double ma = mean[a], mb = mean[b];
    const double s = pw_sum(nk, [&](int i) {
        const double r = sqrt(wn[i]);
        const double da = xa[i] - ma, db = xb[i] - mb;
        const double ea = r * da, eb = r * db;
        return ea * eb;
    }, sx, pt);
    if (threadIdx.x == 0) {
        const double v = nk > 0 ? s : pmc_nan();
        C[(size_t)a * np + b] = v;
        C[(size_t)b * np + a] = v;
    }
}

// Sigma = scale C with ridge added on the diagonal; L = chol(Sigma) in k_cov_chol's order (moment_chol); a pivot that is not > 0 stops the run
// with status 3; logc = -(np 0.9189385332046727) - (((0.0 + log L_00) + log L_11) + ..).  L [np][np] by row, zero above the diagonal
__global__ __launch_bounds__(64) void k_pmc_chol(PmcCtl* __restrict__ ctl, const int np, const double scale, const double ridge,
                                                 const double* __restrict__ C, double* __restrict__ L) {
    __shared__ double M[MAX_DIM * (MAX_DIM + 1)];
    __shared__ int bad;
    if (ctl->stop >= 0) return;   // (uniform)
    const int k = (int)threadIdx.x, ld = MAX_DIM + 1;
    if (k == 0) bad = 0;
    if (k < np)
        for (int l = 0; l < np; ++l) {
            double v = scale * C[(size_t)k * np + l];
            if (l == k) v = v + ridge;
            M[k * ld + l] = v;
        }
    __syncthreads();
    moment_chol(M, np, ld, k, &bad);
    __syncthreads();
    if (k < np)
        for (int l = 0; l < np; ++l) L[(size_t)k * np + l] = l <= k ? M[k * ld + l] : 0.0;
    if (k == 0) {
        if (bad) ctl->stop = 3;
        else {
            double t = 0.0;
            for (int j = 0; j < np; ++j) t = t + smm::smm_log(M[j * ld + j]);
            const double a = (double)np * 0.9189385332046727;
            ctl->logc = -a - t;
        }
    }
}

// z = L^-1 u of particles [0, n): s = u_k, s = s - L_km z_m for m < k in order, z_k = s / L_kk.  A lane reads back the z_m it wrote.  zT (the
// kept particles'): the same values once more by particle, [n][ldt], which is how k_pmc_kernel reads them
__global__ __launch_bounds__(256) void k_pmc_whiten(const int n, const int np, const double* __restrict__ L, const double* __restrict__ u,
                                                    double* __restrict__ z, const size_t stride, double* __restrict__ zT, const int ldt) {
    __shared__ double sL[MAX_DIM * MAX_DIM];
    for (int e = (int)threadIdx.x; e < np * np; e += 256) sL[e] = L[e];
    __syncthreads();
    const int j = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (j >= n) return;
    for (int k = 0; k < np; ++k) {
        double s = u[(size_t)k * stride + j];
        for (int m = 0; m < k; ++m) {
            const double p = sL[k * np + m] * z[(size_t)m * stride + j];
            s = s - p;
        }
        const double zk = s / sL[k * np + k];
        z[(size_t)k * stride + j] = zk;
        if (zT) zT[(size_t)j * ldt + k] = zk;
    }
    if (zT)
        for (int k = np; k < ldt; ++k) zT[(size_t)j * ldt + k] = 0.0;
}

// new particle j < n of generation g: the parent from the block at counter {j, g, 0, 1}, the normals 2m, 2m + 1 from {j, g, m, 2}; y = L n as the
// Cholesky step of smm_propose.hpp adds it, u = u_parent + y, inside when 0 <= u_k <= 1 for every k.  Every new particle starts with the
// distance +inf and the log-weight 0
__global__ __launch_bounds__(64) void k_pmc_propose(const KParams P, const PmcCtl* __restrict__ ctl, const int g, const int n, const double* __restrict__ L,
                                                    const long long* __restrict__ pre, const double* __restrict__ ku, const size_t kstride,
                                                    double* __restrict__ nu, double* __restrict__ nth, double* __restrict__ nrho, double* __restrict__ nlw,
                                                    const size_t stride, int32_t* __restrict__ inside, int32_t* __restrict__ flagw) {
    __shared__ double nb[MAX_DIM][64];
    const int lane = (int)threadIdx.x, j = (int)blockIdx.x * 64 + lane, np = P.np;
    if (j >= n) return;   // (no barrier below: a lane reads only its own column of nb)
    const int nk = ctl->nk;
    const long long Q = ctl->Q;
    const smm::U4 xp = smm::philox_stream(P.seed, smm::STREAM_PMC, (uint32_t)j, (uint32_t)g, 0u, 1u);
    const double v = smm::u53(xp.x, xp.y);
    long long r = (long long)(v * (double)Q);
    if (r > Q - 1) r = Q - 1;
    int lo = 0, hi = nk - 1;   // the largest i with pre_i <= r (q >= 1: the prefix is strictly increasing)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (pre[mid] <= r) lo = mid; else hi = mid - 1;
    }
    const int parent = lo;
    for (int m = 0; 2 * m < np; ++m) {
        double z0, z1;
        smm::box_muller(smm::philox_stream(P.seed, smm::STREAM_PMC, (uint32_t)j, (uint32_t)g, (uint32_t)m, 2u), z0, z1);
        nb[2 * m][lane] = z0;
        if (2 * m + 1 < np) nb[2 * m + 1][lane] = z1;
    }
    bool ok = true;
    for (int k = 0; k < np; ++k) {
        const double* __restrict__ Lk = L + (size_t)k * np;
        double y = Lk[0] * nb[0][lane];
        for (int m = 1; m <= k; ++m) {
            const double pr = Lk[m] * nb[m][lane];
            y = y + pr;
        }
        const double x = ku[(size_t)k * kstride + parent] + y;
        if (!(x >= 0.0 && x <= 1.0)) ok = false;
        const double lbk = P.lb[k], span = P.ub[k] - lbk;
        const double sc = x * span;
        nu[(size_t)k * stride + j] = x;
        nth[(size_t)k * stride + j] = sc + lbk;   // mapto_ab
    }
    nrho[j] = __builtin_huge_val();
    nlw[j] = 0.0;
    inside[j] = ok ? 1 : 0;
    flagw[j] = 0;
}

// block b = b0 + blockIdx.y of T over the kept particles; lane w of the list owns new particle wlist[w]: part[blockIdx.y][w] = the block's
// terms t_i = wn_i smm_exp(-0.5 d2_i) added left to right from 0.0, d2 = (z_0 - z_i0)^2, then + (z_k - z_ik)^2 left to right.  The kept
// particle i is the same for every lane: its row kzT [i][NPC] and wn_i are read through the scalar cache into scalar registers.  NPC is np
// rounded up to a multiple of 4; the padding is 0.0 on both sides and adds 0.0 to d2
template <int NPC>
__global__ __launch_bounds__(PMC_WG) void k_pmc_kernel(const PmcCtl* __restrict__ ctl, const int np, const int b0, const int32_t* __restrict__ wlist,
                                                       const double* __restrict__ nz, const size_t stride, const double* __restrict__ kzT,
                                                       const double* __restrict__ wn, double* __restrict__ part, const size_t pstride) {
    const int w = (int)blockIdx.x * PMC_WG + (int)threadIdx.x, nk = ctl->nk, n_w = ctl->n_w;
    if (w >= n_w) return;
    const int j = wlist[w];
    double z[NPC];
#pragma unroll
    for (int k = 0; k < NPC; ++k) z[k] = k < np ? nz[(size_t)k * stride + j] : 0.0;
    const int i0 = (b0 + (int)blockIdx.y) * PMC_TB, i1 = min(i0 + PMC_TB, nk);
    double bsum = 0.0;
    for (int i = i0; i < i1; ++i) {
        const double* __restrict__ zi = kzT + (size_t)i * NPC;
        const double d0 = z[0] - zi[0];
        double d2 = d0 * d0;
#pragma unroll
        for (int k = 1; k < NPC; ++k) {   // (k >= np: z and the row are 0.0, and d2 + 0.0 is d2: no guard, so that the row's loads go out together)
            const double d = z[k] - zi[k];
            const double p = d * d;
            d2 = d2 + p;
        }
        const double h = -0.5 * d2;
        const double t = wn[i] * smm::smm_exp(h);
        bsum = bsum + t;
    }
    part[(size_t)blockIdx.y * pstride + w] = bsum;
}

// D_w = D_w + the block sums of a pass, in block order (first: from 0.0)
__global__ __launch_bounds__(256) void k_pmc_combine(const PmcCtl* __restrict__ ctl, const int first, const int nblk, const double* __restrict__ part,
                                                     const size_t pstride, double* __restrict__ D) {
    const int w = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (w >= ctl->n_w) return;
    double d = first ? 0.0 : D[w];
    for (int b = 0; b < nblk; ++b) d = d + part[(size_t)b * pstride + w];
    D[w] = d;
}

// lw = -(smm_log(D) + logc); D < DBL_MIN: the distance becomes +inf and the particle counts as underflow; then the particles below the previous eps
__global__ __launch_bounds__(256) void k_pmc_logw(PmcCtl* __restrict__ ctl, const int32_t* __restrict__ wlist, const double* __restrict__ D,
                                                  double* __restrict__ nrho, double* __restrict__ nlw, int32_t* __restrict__ n_underflow) {
    const int w = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (w >= ctl->n_w) return;
    const int j = wlist[w];
    const double d = D[w];
    if (d < 2.2250738585072014e-308) {
        nrho[j] = __builtin_huge_val();
        atomicAdd(n_underflow, 1);
        return;
    }
    const double s = smm::smm_log(d) + ctl->logc;
    nlw[j] = -s;
    if (nrho[j] < ctl->eps) atomicAdd(&ctl->n_acc, 1);
}

// The select over the n candidates rho (the kept in stored order, then the new in j order): A' = min(A, finite ones); the A' smallest by the
// IEEE total order of smm_stats.hpp's keys, ties to the earlier candidate, compacted in candidate order into src [A'] (the candidate each
// kept row comes from); eps = the largest kept distance; then whether the run goes on.  nk_old: the candidates before the new ones
__global__ __launch_bounds__(STATS_WG) void k_pmc_select(PmcCtl* __restrict__ ctl, const PmcGen G, const int g, const int max_gen, const double p_acc_min,
                                                         const int A, const int n, const int nk_old, const double* __restrict__ rho,
                                                         int32_t* __restrict__ src) {
    __shared__ int hist[2048], part[STATS_WG], res[2];
    __shared__ int wtot[2][STATS_WG / 64];
    __shared__ int sh_cnt[2], sh_nnk;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double inf = __builtin_huge_val();
    if (tid < 2) sh_cnt[tid] = 0;
    if (tid == 2) sh_nnk = 0;
    __syncthreads();
    int c = 0;
    for (int i = tid; i < n; i += STATS_WG) c += rho[i] < inf ? 1 : 0;
    for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off);
    if (lane == 0) atomicAdd(&sh_cnt[0], c);
    __syncthreads();
    const int nfin = sh_cnt[0], Ap = min(A, nfin);
    double eps = pmc_nan();
    int n_new_kept = 0;
    if (Ap >= 1) {
        const unsigned long long thr = stats_select(rho, n, Ap - 1, hist, part, res);
        c = 0;
        for (int i = tid; i < n; i += STATS_WG) c += stats_key(rho[i]) < thr ? 1 : 0;
        for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off);
        if (lane == 0) atomicAdd(&sh_cnt[1], c);
        __syncthreads();
        const int need = Ap - sh_cnt[1];   // the candidates equal to the threshold that are kept: the first `need` of them
        int base_eq = 0, base_take = 0;
        for (int i0 = 0; i0 < n; i0 += STATS_WG) {
            const int i = i0 + tid;
            const unsigned long long key = i < n ? stats_key(rho[i]) : ~0ull;
            const bool eq = i < n && key == thr;
            const unsigned long long me = __ballot(eq);
            if (lane == 0) wtot[0][wave] = __popcll(me);
            __syncthreads();
            int eq_before = base_eq, eq_all = base_eq;
            for (int w = 0; w < STATS_WG / 64; ++w) { if (w < wave) eq_before += wtot[0][w]; eq_all += wtot[0][w]; }
            eq_before += __popcll(me & ((1ull << lane) - 1ull));
            const bool take = i < n && (key < thr || (eq && eq_before < need));
            const unsigned long long mt = __ballot(take);
            if (lane == 0) wtot[1][wave] = __popcll(mt);
            __syncthreads();
            int t_before = base_take, t_all = base_take;
            for (int w = 0; w < STATS_WG / 64; ++w) { if (w < wave) t_before += wtot[1][w]; t_all += wtot[1][w]; }
            if (take) {
                src[t_before + __popcll(mt & ((1ull << lane) - 1ull))] = i;
                if (i >= nk_old) ++n_new_kept;
            }
            base_eq = eq_all; base_take = t_all;
            __syncthreads();
        }
        eps = stats_unkey(thr);
    }
    for (int off = 32; off >= 1; off >>= 1) n_new_kept += __shfl_xor(n_new_kept, off);
    if (lane == 0) atomicAdd(&sh_nnk, n_new_kept);
    __syncthreads();
    if (tid == 0) {
        double p_acc = pmc_nan();
        if (g >= 1) p_acc = (double)ctl->n_acc / (double)(n - nk_old);
        int stop = -1;
        if (Ap < 2) stop = 2;
        else if (g >= 1 && p_acc <= p_acc_min) stop = 1;
        else if (g == max_gen) stop = 0;
        G.eps[g] = eps; G.p_acc[g] = p_acc; G.n_new_kept[g] = sh_nnk;
        ctl->nk = Ap; ctl->eps = eps; ctl->stop = stop; ctl->n_acc = 0;
    }
}

// kept row d < ctl->nk from candidate src[d]: an old kept row, or new particle src[d] - nk_old, born in generation g.  Rows: u, theta (np each),
// the moments (nm), then the distance, the log-weight and the generation.  One lane per (row, d)
struct PmcSet { double *u, *th, *mom, *rho, *lw; int32_t* born; };
__global__ __launch_bounds__(256) void k_pmc_move(const PmcCtl* __restrict__ ctl, const int np, const int nm, const int g, const int nk_old,
                                                  const int32_t* __restrict__ src, const PmcSet from, const size_t kstride, const PmcSet fresh,
                                                  const size_t stride, const PmcSet to) {
    const int d = (int)blockIdx.x * 256 + (int)threadIdx.x, row = (int)blockIdx.y;
    if (d >= ctl->nk) return;
    const int s = src[d];
    const bool old = s < nk_old;
    const int j = old ? s : s - nk_old;
    const PmcSet& f = old ? from : fresh;
    const size_t st = old ? kstride : stride;
    if (row < np) to.u[(size_t)row * kstride + d] = f.u[(size_t)row * st + j];
    else if (row < 2 * np) { const int k = row - np; to.th[(size_t)k * kstride + d] = f.th[(size_t)k * st + j]; }
    else if (row < 2 * np + nm) { const int m = row - 2 * np; to.mom[(size_t)m * kstride + d] = f.mom[(size_t)m * st + j]; }
    else {
        to.rho[d] = f.rho[j];
        to.lw[d] = f.lw[j];
        to.born[d] = old ? f.born[j] : g;
    }
}

// quantile [n_probs][np]: blockIdx.x the parameter, blockIdx.y the prob: target = max(1, (int64) ceil(p (double) Q)); the smallest kept theta
// at which the q of the rows with theta <= it reach the target, over the IEEE total order: a radix select over histograms of q
__global__ __launch_bounds__(STATS_WG) void k_pmc_quantile(const PmcCtl* __restrict__ ctl, const int np, const double* __restrict__ probs,
                                                           const double* __restrict__ th, const size_t kstride, const long long* __restrict__ q,
                                                           double* __restrict__ quant) {
    __shared__ unsigned long long hist[2048];
    __shared__ unsigned long long s_rem;
    __shared__ int s_bin;
    const int tid = (int)threadIdx.x, k = (int)blockIdx.x, r = (int)blockIdx.y, nk = ctl->nk;
    if (nk == 0) { if (tid == 0) quant[(size_t)r * np + k] = pmc_nan(); return; }
    const double* __restrict__ x = th + (size_t)k * kstride;
    if (tid == 0) {
        const double h = probs[r] * (double)ctl->Q;
        const long long t = (long long)ceil(h);
        s_rem = (unsigned long long)(t < 1 ? 1 : t);
    }
    unsigned long long prefix = 0ull, known = 0ull;
    for (int d = 0; d < 6; ++d) {
        const int shift = d < 5 ? 53 - 11 * d : 0, width = d < 5 ? 11 : 9;
        const unsigned dmask = (1u << width) - 1u;
        for (int i = tid; i < 2048; i += STATS_WG) hist[i] = 0ull;
        __syncthreads();
        for (int i = tid; i < nk; i += STATS_WG) {
            const unsigned long long key = stats_key(x[i]);
            if ((key & known) == prefix) atomicAdd(&hist[(int)((key >> shift) & dmask)], (unsigned long long)q[i]);
        }
        __syncthreads();
        if (tid == 0) {
            unsigned long long rem = s_rem, run = 0ull;
            int bin = 0;
            const int last = (1 << width) - 1;
            while (bin < last && run + hist[bin] < rem) { run += hist[bin]; ++bin; }
            s_rem = rem - run;
            s_bin = bin;
        }
        __syncthreads();
        prefix |= (unsigned long long)s_bin << shift;
        known |= (unsigned long long)dmask << shift;
        __syncthreads();
    }
    if (tid == 0) quant[(size_t)r * np + k] = stats_unkey(prefix);
}
