// smm_opt_simplex: K Nelder–Mead searches inside the parameter box advancing together (scipy's _minimize_neldermead with bounds and a given
// initial_simplex, made exact) — part of libsmmhip (included by smmhip.hip inside its anonymous namespace; gfx950 device code; hiprtc never
// sees it).  Host side: smm_optsimplex_host.hpp; contract: include/smmhip.h (smm_opt_simplex).  Every state kernel takes one wave (a
// workgroup of 64) per search, a lane per coordinate (np <= 64), so the centroid's left-to-right sum is in-lane.  A simplex is never moved:
// the N + 1 <= 65 values are ranked by counting and the permutation position -> row is what the sort rewrites.  Lists of searches (running,
// second point, shrinking) are compacted in ascending order by one workgroup (k_compact, smm_evalscratch.hpp).  Every operation is rounded
// on its own (-ffp-contract=off).
#pragma once

// the state of one batch of nb searches, the search b of the batch the slowest index, one launch's scratch (smm_evalscratch.hpp), and the
// results, [.][K] with the search the fastest index (search s = s0 + b)
struct SxArgs {
    int K, nb, s0, max_iter;
    double xatol, fatol;
    double step;
    double c_r, rho;         // (1 + rho), rho
    double c_e, rhochi;      // (1 + rho chi), rho chi
    double c_c, psirho;      // (1 + psi rho), psi rho
    double c_i, psi;         // (1 - psi), psi
    double sigma;
    double* sim;             // [nb][N + 1][np] the vertices, by row
    double* mom;             // [nb][N + 1][nm] their moments, by row
    double* fsim;            // [nb][N + 1]     their values, by position (sorted order)
    int32_t* perm;           // [nb][N + 1]     position -> row
    double* xbar;            // [nb][np] the centroid of the current iteration
    double* xr;              // [nb][np] the reflected point, its value and moments
    double* mr;              // [nb][nm]
    double* fxr;             // [nb]
    int32_t* kind;           // [nb] the second point this iteration needs: 0 none, 1 expansion, 2 outside, 3 inside contraction
    int32_t* flag;           // [nb] what the next compaction keeps
    EvalScratch E;
    double* best;            // [np][K]
    double* value;           // [K]
    double* sim_moments;     // [nm][K]
    double* simplex;         // [N + 1][np][K]
    double* simplex_value;   // [N + 1][K]
    double* size_x;          // [K]
    double* size_f;          // [K]
    int32_t* iterations;     // [K]
    int32_t* status;         // [K]
    int32_t* moves;          // [5][K]
    int32_t* n_eval;         // [K]
};

__device__ inline double sx_clip(const double x, const double lb, const double ub) {
    const double y = x < lb ? lb : x;   // (np.clip: minimum(maximum(x, lb), ub))
    return y > ub ? ub : y;
}
// ascending, NaN last, +inf just before NaN
__device__ inline bool sx_less(const double a, const double b) {
    if (a != a) return false;
    if (b != b) return true;
    return a < b;
}
// "take": x (lane k), its value and the moments of evaluation i of n replace the worst vertex of search b (lanes of one wave)
__device__ inline void sx_take_scratch(const KParams& P, const SxArgs& A, const int b, const int lane, const double x, const double f, const size_t n, const size_t i) {
    const int N = P.np, nm = P.nm;
    const int row = A.perm[(size_t)b * (N + 1) + N];
    if (lane < N) A.sim[((size_t)b * (N + 1) + row) * N + lane] = x;
    for (int m = lane; m < nm; m += 64) A.mom[((size_t)b * (N + 1) + row) * nm + m] = A.E.mom(n, i, m);
    if (lane == 0) A.fsim[(size_t)b * (N + 1) + N] = f;
}

// the initial simplex of every search of the batch: vertex 0 the start, vertex k + 1 the start with coordinate k at y = x_k + step * (ub_k -
// lb_k), reflected at ub_k and clipped
__global__ __launch_bounds__(64) void k_sx_init(const KParams P, const SxArgs A, const double* __restrict__ starts) {
    const int lane = (int)threadIdx.x, b = (int)blockIdx.x, N = P.np;
    const size_t s = (size_t)A.s0 + b, K = (size_t)A.K;
    double x = 0.0, y = 0.0;
    if (lane < N) {
        const double lb = P.lb[lane], ub = P.ub[lane];
        x = starts[(size_t)lane * K + s];
        const double w = ub - lb;
        const double d = A.step * w;
        y = x + d;
        if (y > ub) { const double t = 2.0 * ub; y = t - y; }
        y = sx_clip(y, lb, ub);
    }
    for (int j = 0; j <= N; ++j) {
        const double v = (j >= 1 && lane == j - 1) ? y : x;
        if (lane < N) A.sim[((size_t)b * (N + 1) + j) * N + lane] = v;
    }
    for (int p = lane; p <= N; p += 64) A.perm[(size_t)b * (N + 1) + p] = p;
    if (lane < 5) A.moves[(size_t)lane * K + s] = 0;
    if (lane == 0) {
        const double nan = __builtin_nan("");
        A.size_x[s] = nan; A.size_f[s] = nan;
        A.iterations[s] = 0; A.status[s] = 0; A.n_eval[s] = 0;
        A.kind[b] = 0; A.flag[b] = 0;
    }
}

// The initial evaluation and a shrink go vertex by vertex, so that a launch's scratch is one evaluation per search: the vertex at position
// pos of the a-th listed search as evaluation a of n (list == nullptr: the batch itself) ...
__global__ __launch_bounds__(64) void k_sx_vertex(const KParams P, const SxArgs A, const int32_t* __restrict__ list, const int pos, const size_t n) {
    const int lane = (int)threadIdx.x, a = (int)blockIdx.x, N = P.np;
    const int b = list ? list[a] : a;
    const size_t at = (size_t)b * (N + 1);
    if (lane < N) A.E.put_cand(n, (size_t)a, lane, A.sim[(at + A.perm[at + pos]) * N + lane]);
}
// ... and its value and moments, as evaluated, into the state
__global__ __launch_bounds__(64) void k_sx_store(const KParams P, const SxArgs A, const int32_t* __restrict__ list, const int pos, const size_t n) {
    const int lane = (int)threadIdx.x, a = (int)blockIdx.x, N = P.np, nm = P.nm;
    const int b = list ? list[a] : a;
    const size_t at = (size_t)b * (N + 1);
    const int row = A.perm[at + pos];
    for (int m = lane; m < nm; m += 64) A.mom[(at + row) * nm + m] = A.E.mom(n, (size_t)a, m);
    if (lane == 0) {
        A.fsim[at + pos] = A.E.value_of(a);
        A.n_eval[(size_t)A.s0 + b] += 1;
    }
}

// The stable ascending sort of a listed search's values by counting (NaN last, +inf just before NaN, equal values keep their order), then
// what follows every sort: no finite value -> status 2; max_iter iterations run -> status 0; the convergence test, size_x <= xatol &&
// size_f <= fatol -> status 1 (a NaN in either maximum makes it false).  flag = the search goes on.  count_iter: the sort ends an iteration
__global__ __launch_bounds__(64) void k_sx_sort(const KParams P, const SxArgs A, const int32_t* __restrict__ list, const int count_iter) {
    __shared__ double f_in[65], f_out[65];
    __shared__ int32_t row_out[65];
    const int lane = (int)threadIdx.x, a = (int)blockIdx.x, N = P.np;
    const int b = list ? list[a] : a;
    const size_t s = (size_t)A.s0 + b, at = (size_t)b * (N + 1);
    for (int p = lane; p <= N; p += 64) f_in[p] = A.fsim[at + p];
    __syncthreads();
    for (int p = lane; p <= N; p += 64) {
        const double f = f_in[p];
        int rank = 0;
        for (int q = 0; q <= N; ++q) {
            const double g = f_in[q];
            if (sx_less(g, f) || (q < p && !sx_less(f, g))) ++rank;
        }
        f_out[rank] = f;
        row_out[rank] = A.perm[at + p];
    }
    __syncthreads();
    for (int p = lane; p <= N; p += 64) { A.fsim[at + p] = f_out[p]; A.perm[at + p] = row_out[p]; }
    int it = A.iterations[s];
    if (count_iter) ++it;
    const double f0 = f_out[0];
    int keep = 0, status = 0;
    if (!(f0 - f0 == 0.0)) status = 2;               // (not finite)
    else if (it >= A.max_iter) status = 0;
    else {
        // size_x = max |sim[j][k] - sim[0][k]|, j >= 1: the lane's coordinate over the vertices, then over the lanes (no NaN: the box is finite)
        double mx = 0.0;
        if (lane < N) {
            const double x0 = A.sim[(at + row_out[0]) * N + lane];
            for (int j = 1; j <= N; ++j) {
                const double d = A.sim[(at + row_out[j]) * N + lane] - x0;
                const double ad = __builtin_fabs(d);
                mx = ad > mx ? ad : mx;
            }
        }
        // size_f = max |fsim[0] - fsim[j]|, j >= 1: NaN if any difference is NaN, as np.max gives it
        double mf = 0.0;
        int nanf = 0;
        for (int j = 1 + lane; j <= N; j += 64) {
            const double d = f0 - f_out[j];
            const double ad = __builtin_fabs(d);
            if (ad != ad) nanf = 1;
            else mf = ad > mf ? ad : mf;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double ox = __shfl_xor(mx, off), of = __shfl_xor(mf, off);
            const int on = __shfl_xor(nanf, off);
            mx = ox > mx ? ox : mx;
            mf = of > mf ? of : mf;
            nanf |= on;
        }
        if (nanf) mf = __builtin_nan("");
        if (lane == 0) { A.size_x[s] = mx; A.size_f[s] = mf; }
        if (mx <= A.xatol && mf <= A.fatol) status = 1;
        else keep = 1;
    }
    if (lane == 0) {
        A.iterations[s] = it;
        A.status[s] = status;
        A.flag[b] = keep;
    }
}

// centroid of the N best vertices, added left to right, and the reflected point of running search a: evaluation a of n
__global__ __launch_bounds__(64) void k_sx_reflect(const KParams P, const SxArgs A, const int32_t* __restrict__ list, const size_t n) {
    const int lane = (int)threadIdx.x, a = (int)blockIdx.x, N = P.np;
    const int b = list[a];
    const size_t at = (size_t)b * (N + 1);
    if (lane >= N) return;
    double acc = A.sim[(at + A.perm[at]) * N + lane];
    for (int j = 1; j < N; ++j) acc = acc + A.sim[(at + A.perm[at + j]) * N + lane];
    const double xbar = acc / (double)N;
    const double xn = A.sim[(at + A.perm[at + N]) * N + lane];
    const double t1 = A.c_r * xbar, t2 = A.rho * xn;
    const double xr = sx_clip(t1 - t2, P.lb[lane], P.ub[lane]);
    A.xbar[(size_t)b * N + lane] = xbar;
    A.xr[(size_t)b * N + lane] = xr;
    A.E.put_cand(n, (size_t)a, lane, xr);
}

// scipy's comparisons on fxr, literally (a NaN fails every <): the reflected point is taken, or the search needs a second point (kind, flag)
__global__ __launch_bounds__(64) void k_sx_decide(const KParams P, const SxArgs A, const int32_t* __restrict__ list, const size_t n) {
    const int lane = (int)threadIdx.x, a = (int)blockIdx.x, N = P.np, nm = P.nm;
    const int b = list[a];
    const size_t s = (size_t)A.s0 + b, at = (size_t)b * (N + 1);
    const double fxr = A.E.value_of(a), f0 = A.fsim[at], fn1 = A.fsim[at + N - 1], fN = A.fsim[at + N];
    int kind;
    if (fxr < f0) kind = 1;
    else if (fxr < fn1) kind = 0;
    else if (fxr < fN) kind = 2;
    else kind = 3;
    for (int m = lane; m < nm; m += 64) A.mr[(size_t)b * nm + m] = A.E.mom(n, (size_t)a, m);
    if (kind == 0) sx_take_scratch(P, A, b, lane, lane < N ? A.xr[(size_t)b * N + lane] : 0.0, fxr, n, (size_t)a);
    if (lane == 0) {
        A.fxr[b] = fxr;
        A.kind[b] = kind;
        A.flag[b] = kind != 0;
        A.n_eval[s] += 1;
        if (kind == 0) A.moves[s] += 1;
    }
}

// the second point of the a-th search that needs one: expansion, outside or inside contraction; evaluation a of n
__global__ __launch_bounds__(64) void k_sx_second(const KParams P, const SxArgs A, const int32_t* __restrict__ list, const size_t n) {
    const int lane = (int)threadIdx.x, a = (int)blockIdx.x, N = P.np;
    const int b = list[a];
    const size_t at = (size_t)b * (N + 1);
    if (lane >= N) return;
    const int kind = A.kind[b];
    const double xbar = A.xbar[(size_t)b * N + lane], xn = A.sim[(at + A.perm[at + N]) * N + lane];
    double t1, t2, x;
    if (kind == 1) { t1 = A.c_e * xbar; t2 = A.rhochi * xn; x = t1 - t2; }
    else if (kind == 2) { t1 = A.c_c * xbar; t2 = A.psirho * xn; x = t1 - t2; }
    else { t1 = A.c_i * xbar; t2 = A.psi * xn; x = t1 + t2; }
    x = sx_clip(x, P.lb[lane], P.ub[lane]);
    A.xbar[(size_t)b * N + lane] = x;   // (the centroid has served: the second point takes its place until k_sx_accept)
    A.E.put_cand(n, (size_t)a, lane, x);
}

// the second point's value against fxr (expansion: fxe < fxr; outside contraction: fxc <= fxr) or the worst vertex's (inside: fxcc < fsim[N]):
// it is taken, or the reflected point is (a failed expansion), or the search shrinks (flag)
__global__ __launch_bounds__(64) void k_sx_accept(const KParams P, const SxArgs A, const int32_t* __restrict__ list, const size_t n) {
    const int lane = (int)threadIdx.x, a = (int)blockIdx.x, N = P.np, nm = P.nm;
    const int b = list[a];
    const size_t s = (size_t)A.s0 + b, at = (size_t)b * (N + 1), K = (size_t)A.K;
    const int kind = A.kind[b];
    const double f2 = A.E.value_of(a), fxr = A.fxr[b], fN = A.fsim[at + N];
    const bool take2 = kind == 1 ? f2 < fxr : kind == 2 ? f2 <= fxr : f2 < fN;
    const bool shrink = !take2 && kind != 1;
    int move;
    if (take2) {
        move = kind;   // (1 expansion, 2 outside, 3 inside contraction)
        sx_take_scratch(P, A, b, lane, lane < N ? A.xbar[(size_t)b * N + lane] : 0.0, f2, n, (size_t)a);
    } else if (kind == 1) {
        move = 0;
        const int row = A.perm[at + N];
        if (lane < N) A.sim[(at + row) * N + lane] = A.xr[(size_t)b * N + lane];
        for (int m = lane; m < nm; m += 64) A.mom[(at + row) * nm + m] = A.mr[(size_t)b * nm + m];
        if (lane == 0) A.fsim[at + N] = fxr;
    } else move = 4;
    if (lane == 0) {
        A.flag[b] = shrink;
        A.n_eval[s] += 1;
        A.moves[(size_t)move * K + s] += 1;
    }
}

// shrink: vertex j = 1 .. N of the a-th shrinking search towards vertex 0 (evaluated behind it, vertex by vertex).  blockIdx.y = j - 1
__global__ __launch_bounds__(64) void k_sx_shrink(const KParams P, const SxArgs A, const int32_t* __restrict__ list) {
    const int lane = (int)threadIdx.x, a = (int)blockIdx.x, jj = (int)blockIdx.y, N = P.np;
    const int b = list[a];
    const size_t at = (size_t)b * (N + 1);
    if (lane >= N) return;
    const int row = A.perm[at + 1 + jj];
    const double x0 = A.sim[(at + A.perm[at]) * N + lane], xj = A.sim[(at + row) * N + lane];
    const double d = xj - x0;
    const double sd = A.sigma * d;
    const double x = sx_clip(x0 + sd, P.lb[lane], P.ub[lane]);
    A.sim[(at + row) * N + lane] = x;
}

// the batch's results: the final simplex in sorted order, vertex 0 as best with its value and moments
__global__ __launch_bounds__(64) void k_sx_finish(const KParams P, const SxArgs A) {
    const int lane = (int)threadIdx.x, b = (int)blockIdx.x, N = P.np, nm = P.nm;
    const size_t s = (size_t)A.s0 + b, at = (size_t)b * (N + 1), K = (size_t)A.K;
    for (int j = 0; j <= N; ++j) {
        const int row = A.perm[at + j];
        if (lane < N) {
            const double x = A.sim[(at + row) * N + lane];
            A.simplex[((size_t)j * N + lane) * K + s] = x;
            if (j == 0) A.best[(size_t)lane * K + s] = x;
        }
        if (j == 0)
            for (int m = lane; m < nm; m += 64) A.sim_moments[(size_t)m * K + s] = A.mom[(at + row) * nm + m];
    }
    for (int j = lane; j <= N; j += 64) A.simplex_value[(size_t)j * K + s] = A.fsim[at + j];
    if (lane == 0) A.value[s] = A.fsim[at];
}
