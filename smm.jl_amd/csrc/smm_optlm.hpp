// smm_opt_lm: K Levenberg–Marquardt searches inside the parameter box advancing together, on the moments' residuals r_j = (sim_j - mom_j) /
// s_j with forward-difference Jacobians — part of libsmmhip (included by smmhip.hip inside its anonymous namespace behind smm_optsimplex.hpp,
// whose clip it uses; scratch view, evaluation tile and list compaction: smm_evalscratch.hpp; gfx950 device code; hiprtc never sees it).  Host side: smm_optlm_host.hpp;
// contract: include/smmhip.h (smm_opt_lm).  Every state kernel takes one wave (a workgroup of 64) per search, a lane per parameter
// (np <= 64); every sum of the contract runs in ascending index inside one lane, nothing is reduced across lanes but maxima and ballots.
// The factorisation and the substitutions are moment_chol's and moment_subst's (smm_moments.hpp).  Every operation is rounded on its own
// (-ffp-contract=off).
//
// LDS: k_lm_normal stages J [nm][np] and r [nm], (nm np + nm) x 8 bytes — 32.5 KiB at np = nm = 64 —, and writes A's rows straight to the
// batch's state, so A takes no LDS; k_lm_step holds B [np][np + 1], the right-hand side and its pivot flag, 33 KiB at np = 64.  Both run ONE
// wave per workgroup: at the interface's maximum four such workgroups share a compute unit's 160 KiB (one per SIMD), at C5 (np = nm = 50:
// 19.9 KiB) eight do, and a workgroup of several waves would only tie searches that need different numbers of tries to one barrier.
#pragma once

// the results, [.][K] with the search the fastest index (search s = s0 + b) — x, F, lambda and the counters of a running search live in
// them —, the state of one batch of nb searches that is no result, and one launch's scratch (smm_evalscratch.hpp)
struct LmArgs {
    int K, nb, s0, max_iter, max_tries;
    double fd_step, lambda0, lambda_up, lambda_down, xtol, ftol, gtol;
    double* r;               // [nb][nm]     the residuals at x
    double* A;               // [nb][np][np] J'J with the active set applied, the lower triangle
    double* xnew;            // [nb][np]     the trial point of the current try
    int32_t* itry;           // [nb] tries of the current iteration
    int32_t* piv;            // [nb] the current try failed at a pivot: its evaluation pads the launch
    int32_t* f_try;          // [nb] the search makes (another) try
    int32_t* f_go;           // [nb] the search goes on into the next iteration
    EvalScratch E;           // the candidates: one trial point per search, or a user objective's Jacobian points [n x np][np]
    double* best;            // [np][K]
    double* value;           // [K]
    double* sim_moments;     // [nm][K]
    double* ssr;             // [K]
    double* grad;            // [np][K]
    double* jac;             // [nm][np][K], or nullptr: not asked for
    double* lambda;          // [K]
    double* step;            // [K]
    double* dF;              // [K]
    int32_t* active;         // [np][K]
    int32_t* iterations;     // [K]
    int32_t* tries;          // [K]
    int32_t* n_eval;         // [K]
    int32_t* status;         // [K]
};

__device__ inline bool lm_finite(const double x) { return x - x == 0.0; }
// s_j: smm_get_moment_stats' rule
__device__ inline double lm_scale(const double w) { return (lm_finite(w) && w != 0.0) ? w : 1.0; }
// the shifted coordinate of the Jacobian's point k: forward, backward where forward leaves the box
__device__ inline double lm_shift(const double x, const double lb, const double ub, const double fd_step) {
    const double w = ub - lb;
    const double h = fd_step * w;
    const double y = x + h;
    return y > ub ? x - h : y;
}
__device__ inline double lm_residual(const double sim, const double mom, const double w) {
    const double d = sim - mom;
    return d / lm_scale(w);
}

// every search of the batch at its start: evaluation b of nb
__global__ __launch_bounds__(64) void k_lm_init(const KParams P, const LmArgs A, const double* __restrict__ starts) {
    const int lane = (int)threadIdx.x, b = (int)blockIdx.x, N = P.np, nm = P.nm;
    const size_t s = (size_t)A.s0 + b, K = (size_t)A.K;
    const double nan = __builtin_nan("");
    if (lane < N) {
        const double x = starts[(size_t)lane * K + s];
        A.best[(size_t)lane * K + s] = x;
        A.grad[(size_t)lane * K + s] = nan;
        A.active[(size_t)lane * K + s] = 0;
        A.E.put_cand((size_t)A.nb, (size_t)b, lane, x);
        if (A.jac)
            for (int j = 0; j < nm; ++j) A.jac[((size_t)j * N + lane) * K + s] = nan;
    }
    if (lane == 0) {
        A.lambda[s] = A.lambda0; A.step[s] = nan; A.dF[s] = nan;
        A.iterations[s] = 0; A.tries[s] = 0; A.n_eval[s] = 0; A.status[s] = 0;
        A.itry[b] = 0; A.piv[b] = 0; A.f_try[b] = 0; A.f_go[b] = 0;
    }
}

// evaluation i of n as residuals into LDS (res [nm]) by the wave's lanes; all finite?  F = 0.0 + r_0^2 + ... by every lane alike
__device__ inline bool lm_take_residuals(const KParams& P, const LmArgs& A, const int lane, const size_t n, const size_t i, double* res, double& F) {
    const int nm = P.nm;
    bool fin = true;
    for (int j = lane; j < nm; j += 64) {
        const double rj = lm_residual(A.E.mom(n, i, j), P.mom[j], P.w[j]);
        res[j] = rj;
        fin = fin && lm_finite(rj);
    }
    __syncthreads();
    double acc = 0.0;
    for (int j = 0; j < nm; ++j) {
        const double sq = res[j] * res[j];
        acc = acc + sq;
    }
    F = acc;
    return __ballot(!fin) == 0ull;
}
// ... and x's new value, moments, residuals and F filed as evaluated
__device__ inline void lm_file(const KParams& P, const LmArgs& A, const int lane, const int b, const size_t n, const size_t i, const double* res, const double F) {
    const int nm = P.nm;
    const size_t s = (size_t)A.s0 + b, K = (size_t)A.K;
    for (int j = lane; j < nm; j += 64) {
        A.r[(size_t)b * nm + j] = res[j];
        A.sim_moments[(size_t)j * K + s] = A.E.mom(n, i, j);
    }
    if (lane == 0) { A.value[s] = A.E.value_of(i); A.ssr[s] = F; }
}

// the start's evaluation: a residual that is not finite stops the search with status 2
__global__ __launch_bounds__(64) void k_lm_start(const KParams P, const LmArgs A) {
    __shared__ double res[MAX_DIM];
    const int lane = (int)threadIdx.x, b = (int)blockIdx.x;
    const size_t s = (size_t)A.s0 + b;
    double F;
    const bool fin = lm_take_residuals(P, A, lane, (size_t)A.nb, (size_t)b, res, F);
    lm_file(P, A, lane, b, (size_t)A.nb, (size_t)b, res, F);
    if (lane == 0) {
        A.n_eval[s] = 1;
        A.status[s] = fin ? 0 : 2;
        A.f_go[b] = fin ? 1 : 0;
    }
}

// a user objective's Jacobian points as rows: evaluation i = a * np + k of n is the a-th running search's x with coordinate k shifted
__global__ __launch_bounds__(256) void k_lm_candidates(const KParams P, const LmArgs A, const int32_t* __restrict__ list, const size_t n) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int np = P.np;
    if (t >= n * (size_t)np) return;
    const size_t i = t / (size_t)np;
    const int j = (int)(t % (size_t)np), k = (int)(i % (size_t)np);
    const size_t at = (size_t)j * A.K + (size_t)A.s0 + list[i / (size_t)np];
    const double x = A.best[at];
    A.E.put_cand(n, i, j, j == k ? lm_shift(x, P.lb[j], P.ub[j], A.fd_step) : x);
}

// eval_tile on the Jacobian's points, which are never written: the tile's theta comes from the search's x and the one shifted coordinate.
// Evaluation i = a * np + k of n -> value [n], simM [nm][n], status [n]
template <int KIND, int CT>
__global__ __launch_bounds__(WG, 4) void k_eval_lm(const KParams P, const LmArgs A, const int32_t* __restrict__ list, const int n, int8_t* __restrict__ status) {
    eval_tile_of<KIND, CT>(P, n, [&](const int ie, const int j) {
        const double x = A.best[(size_t)j * A.K + (size_t)A.s0 + list[ie / P.np]];
        return j == ie % P.np ? lm_shift(x, P.lb[j], P.ub[j], A.fd_step) : x;
    }, A.E, status);
}

// The normal equations of running search a from its np Jacobian evaluations a * np + k of n: J, g, A, the active set and the stops that
// need no try (status 2: a J_jk that is not finite; 4: a parameter that moves no moment; 1: the free gradient within gtol).  Lane k: column k
// of J, g_k and row k of A.  f_try: the search makes its first try.  Dynamic LDS: J [nm][np], r [nm]
__global__ __launch_bounds__(64) void k_lm_normal(const KParams P, const LmArgs A, const int32_t* __restrict__ list, const size_t n) {
    extern __shared__ __attribute__((aligned(16))) double lm_smem[];
    const int lane = (int)threadIdx.x, a = (int)blockIdx.x, N = P.np, nm = P.nm, k = lane;
    const int b = list[a];
    const size_t s = (size_t)A.s0 + b, K = (size_t)A.K;
    double* J = lm_smem;
    double* r = J + (size_t)nm * N;
    for (int j = lane; j < nm; j += 64) r[j] = A.r[(size_t)b * nm + j];
    __syncthreads();
    double x = 0.0, lb = 0.0, ub = 0.0;
    bool fin = true;
    if (k < N) {
        lb = P.lb[k]; ub = P.ub[k];
        x = A.best[(size_t)k * K + s];
        const double y = lm_shift(x, lb, ub, A.fd_step);
        const double d = y - x;
        const size_t i = (size_t)a * N + k;
        for (int j = 0; j < nm; ++j) {
            const double rk = lm_residual(A.E.mom(n, i, j), P.mom[j], P.w[j]);
            const double diff = rk - r[j];
            const double Jjk = diff / d;
            J[(size_t)j * N + k] = Jjk;
            fin = fin && lm_finite(Jjk);
            if (A.jac) A.jac[((size_t)j * N + k) * K + s] = Jjk;
        }
    }
    __syncthreads();
    int status = 0, go_try = 0;
    if (__ballot(!fin) != 0ull) status = 2;
    else {
        double g = 0.0, Akk = 1.0;
        if (k < N) {
            for (int j = 0; j < nm; ++j) {
                const double p = J[(size_t)j * N + k] * r[j];
                g = g + p;
            }
            A.grad[(size_t)k * K + s] = g;
        }
        const bool act = k < N && ((x == lb && g > 0.0) || (x == ub && g < 0.0));
        const unsigned long long am = __ballot(act);
        if (k < N) {
            A.active[(size_t)k * K + s] = act ? 1 : 0;
            double* row = A.A + ((size_t)b * N + k) * N;
            for (int l = 0; l <= k; ++l) {
                double v = 0.0;
                for (int j = 0; j < nm; ++j) {
                    const double p = J[(size_t)j * N + k] * J[(size_t)j * N + l];
                    v = v + p;
                }
                if (l == k) Akk = v;
                if (act || ((am >> l) & 1ull)) v = l == k ? 1.0 : 0.0;
                row[l] = v;
            }
        }
        const bool fre = k < N && !act;
        const double ag = __builtin_fabs(g);
        if (__ballot(fre && Akk == 0.0) != 0ull) status = 4;
        else if (__ballot(fre && !(ag <= A.gtol)) == 0ull) status = 1;
        else go_try = 1;
    }
    if (lane == 0) {
        A.iterations[s] += 1;
        A.n_eval[s] += N;
        A.status[s] = status;
        A.itry[b] = 0; A.piv[b] = 0;
        A.f_try[b] = go_try;
        A.f_go[b] = 0;
    }
}

// One try of the a-th listed search: B = A with lambda A_kk added on the diagonal, its factor, delta = solve(L, -g), the clipped trial
// point as evaluation a of n.  A pivot that is not > 0 (piv) and a search that stopped at its normal equations (first round only) put x
// there: the evaluation pads the launch and is never looked at.  Dynamic LDS: B [np][np + 1], delta [np], the pivot flag (no static LDS:
// it would sit in front of the dynamic region and take the doubles off their alignment)
__global__ __launch_bounds__(64) void k_lm_step(const KParams P, const LmArgs A, const int32_t* __restrict__ list, const size_t n) {
    extern __shared__ __attribute__((aligned(16))) double lm_smem[];
    const int lane = (int)threadIdx.x, a = (int)blockIdx.x, N = P.np, k = lane, ld = N + 1;
    const int b = list[a];
    const size_t s = (size_t)A.s0 + b, K = (size_t)A.K;
    double* B = lm_smem;
    double* delta = B + (size_t)N * ld;
    int& bad = *(int*)(delta + N);
    const double x = k < N ? A.best[(size_t)k * K + s] : 0.0;
    const bool trying = A.f_try[b] != 0;   // (uniform)
    if (lane == 0) bad = 0;
    if (trying && k < N) {
        const double lambda = A.lambda[s];
        const double* row = A.A + ((size_t)b * N + k) * N;
        for (int l = 0; l < k; ++l) B[k * ld + l] = row[l];
        const double p = lambda * row[k];
        B[k * ld + k] = row[k] + p;
        const double g = A.active[(size_t)k * K + s] ? 0.0 : A.grad[(size_t)k * K + s];
        delta[k] = -g;
    }
    __syncthreads();
    if (trying) {
        moment_chol(B, N, ld, k, &bad);
        if (!bad && lane == 0) moment_subst(B, N, ld, delta);
        __syncthreads();
    }
    const bool padded = !trying || bad != 0;
    if (k < N) {
        const double xn = padded ? x : sx_clip(x + delta[k], P.lb[k], P.ub[k]);
        A.xnew[(size_t)b * N + k] = xn;
        A.E.put_cand(n, (size_t)a, k, xn);
    }
    if (lane == 0) A.piv[b] = trying && bad != 0 ? 1 : 0;
}

// The try's verdict: r_new all finite and F_new < F -> accepted (x, r, F, value and moments replaced as evaluated; step, dF; lambda down;
// the search converged, ran out of iterations, or goes on: f_go); else lambda up, and another try (f_try) unless lambda is no longer finite
// or the iteration's tries are used up (status 3)
__global__ __launch_bounds__(64) void k_lm_judge(const KParams P, const LmArgs A, const int32_t* __restrict__ list, const size_t n) {
    __shared__ double res[MAX_DIM];
    const int lane = (int)threadIdx.x, a = (int)blockIdx.x, N = P.np, k = lane;
    const int b = list[a];
    const size_t s = (size_t)A.s0 + b, K = (size_t)A.K;
    if (A.f_try[b] == 0) return;   // (uniform: stopped at its normal equations)
    const bool piv = A.piv[b] != 0;
    double Fn = 0.0;
    bool accept = false;
    const double F = A.ssr[s];
    if (!piv) {
        const bool fin = lm_take_residuals(P, A, lane, n, (size_t)a, res, Fn);
        accept = fin && Fn < F;
    }
    int status = 0, again = 0, go = 0;
    double lambda = A.lambda[s];
    if (accept) {
        double mx = 0.0;
        if (k < N) {
            const double xn = A.xnew[(size_t)b * N + k];
            const double d = xn - A.best[(size_t)k * K + s];
            mx = __builtin_fabs(d);
            A.best[(size_t)k * K + s] = xn;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double o = __shfl_xor(mx, off);
            mx = o > mx ? o : mx;
        }
        lm_file(P, A, lane, b, n, (size_t)a, res, Fn);
        const double dF = F - Fn;
        const double t = lambda / A.lambda_down;
        lambda = t > 1e-300 ? t : 1e-300;
        const double bound = A.ftol * Fn;
        if (mx <= A.xtol || dF <= bound) status = 1;
        else if (A.iterations[s] >= A.max_iter) status = 0;
        else go = 1;
        if (lane == 0) { A.step[s] = mx; A.dF[s] = dF; }
    } else {
        lambda = lambda * A.lambda_up;
        if (!lm_finite(lambda) || A.itry[b] + 1 >= A.max_tries) status = 3;
        else again = 1;
    }
    if (lane == 0) {
        A.lambda[s] = lambda;
        A.tries[s] += 1;
        A.itry[b] += 1;
        if (!piv) A.n_eval[s] += 1;
        A.status[s] = status;
        A.f_try[b] = again;
        A.f_go[b] = go;
    }
}
