// smm_opt_slices: K cyclic coordinate searches on grids advancing together (optSlices, slices.jl:114-242) — part of libsmmhip (included by
// smmhip.hip inside its anonymous namespace; gfx950 device code; hiprtc never sees it).  Host side: smm_optslices_host.hpp; contract:
// include/smmhip.h (smm_opt_slices).  One coordinate step of all running searches is one evaluation launch over n = (active searches of
// the batch) x G grid points, evaluation i = a * G + g (a: the search's rank among the active ones of the batch), then k_os_select; a cycle
// ends in k_os_cycle_end, which drops the searches that stopped.  Every operation is rounded on its own (-ffp-contract=off).
#pragma once

// the searches' state, [.][K] with the search the fastest index, and one step's scratch (smm_evalscratch.hpp)
struct OsArgs {
    int K, G, max_cycles;
    double tol, update;      // update NaN: the ranges never shrink
    double* bestp;           // [np][K] the point each search stands at
    double* lo;              // [np][K] the search ranges
    double* hi;
    double* dvec;            // [np][K] the moves of the current cycle
    double* value;           // [K]     value and moments of the last winner (+inf / NaN before the first)
    double* simM;            // [nm][K]
    double* delta;           // [K]
    double* cycle_value;     // [max_cycles][K]
    int32_t* cycles;         // [K]
    int32_t* converged;      // [K]
    EvalScratch E;           // (the step's candidates only where they are materialised)
};

// numpy's linspace(lo, hi, G)[g], G >= 2: step = (hi - lo) / (G - 1), x_g = g * step + lo, the last point hi itself; a step that rounds to
// zero: x_g = (g / (G - 1)) * (hi - lo) + lo
__device__ inline double os_grid(const double lo, const double hi, const int G, const int g) {
    if (g == G - 1) return hi;
    const double d = hi - lo, div = (double)(G - 1);
    const double step = d / div;
    if (step == 0.0) {
        const double f = (double)g / div;
        const double y = f * d;
        return y + lo;
    }
    const double y = (double)g * step;
    return y + lo;
}

__global__ __launch_bounds__(256) void k_os_init(const KParams P, const OsArgs A, int32_t* __restrict__ act) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t K = (size_t)A.K;
    const double nan = __builtin_nan("");
    if (i < K) {
        act[i] = (int32_t)i;
        A.value[i] = INFINITY; A.delta[i] = INFINITY;
        A.cycles[i] = 0; A.converged[i] = 0;
    }
    if (i < K * (size_t)P.np) { const int k = (int)(i / K); A.lo[i] = P.lb[k]; A.hi[i] = P.ub[k]; A.dvec[i] = 0.0; }
    if (i < K * (size_t)P.nm) A.simM[i] = nan;
    if (i < K * (size_t)A.max_cycles) A.cycle_value[i] = nan;
}

// the step's candidates as rows, for the kernels that read a matrix (a user objective's compiled kernel; the built-in objectives'
// k_eval_batch in the timing experiment): one thread per (evaluation, parameter)
__global__ __launch_bounds__(256) void k_os_candidates(const KParams P, const OsArgs A, const int32_t* __restrict__ act, const int k, const int a0, const int n) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int np = P.np;
    if (t >= (size_t)n * (size_t)np) return;
    const int i = (int)(t / (size_t)np), j = (int)(t % (size_t)np);
    const int s = act[a0 + i / A.G], g = i % A.G;
    const size_t at = (size_t)j * A.K + s;
    const double x = j == k ? os_grid(A.lo[at], A.hi[at], A.G, g) : A.bestp[at];
    A.E.put_cand((size_t)n, (size_t)i, j, x);
}

// eval_tile on candidates that are never written: the tile's theta comes from the search's bestp column and the one replaced coordinate.
// Evaluation i of n -> value [n], simM [nm][n], status [n]
template <int KIND, int CT>
__global__ __launch_bounds__(WG, 4) void k_eval_slice(const KParams P, const OsArgs A, const int32_t* __restrict__ act, const int k, const int a0, const int n,
                                                      int8_t* __restrict__ status) {
    eval_tile_of<KIND, CT>(P, n, [&](const int ie, const int j) {
        const size_t at = (size_t)j * A.K + act[a0 + ie / A.G];
        return j == k ? os_grid(A.lo[at], A.hi[at], A.G, ie % A.G) : A.bestp[at];
    }, A.E, status);
}

// One wave per active search of the batch: the grid point with the smallest finite value, ties to the lowest g, by a butterfly over the
// lanes' (value, g); the status is not consulted (slices.jl:181).  The winner becomes bestp_k, its value and moments the search's, as
// evaluated; without a finite value bestp stays.  dvec_k = old_k - new_k.
constexpr int OS_WPB = 4;   // searches (waves) per workgroup
__global__ __launch_bounds__(64 * OS_WPB) void k_os_select(const KParams P, const OsArgs A, const int32_t* __restrict__ act, const int k, const int a0, const int nb) {
    const int lane = (int)threadIdx.x & 63;
    const int b = (int)blockIdx.x * OS_WPB + ((int)threadIdx.x >> 6);
    if (b >= nb) return;   // (the whole wave)
    const int s = act[a0 + b], G = A.G, nm = P.nm;
    const size_t j0 = (size_t)b * (size_t)G, n = (size_t)nb * (size_t)G;
    constexpr int NONE = 0x7fffffff;
    double bv = INFINITY;
    int bg = NONE;
    for (int g = lane; g < G; g += 64) {
        const double v = A.E.value_of(j0 + g);
        if (v < bv && v > -INFINITY) { bv = v; bg = g; }   // (finite and strictly lower; ascending g: an equal value keeps the lower one)
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double ov = __shfl_xor(bv, off);
        const int og = __shfl_xor(bg, off);
        if (ov < bv || (ov == bv && og < bg)) { bv = ov; bg = og; }
    }
    const size_t at = (size_t)k * A.K + s;
    if (bg == NONE) {
        if (lane == 0) A.dvec[at] = 0.0;   // (old - old)
        return;
    }
    const size_t jw = j0 + (size_t)bg;
    for (int f = lane; f < nm; f += 64) A.simM[(size_t)f * A.K + s] = A.E.mom(n, jw, f);
    if (lane == 0) {
        const double old = A.bestp[at], x = os_grid(A.lo[at], A.hi[at], G, bg);
        A.bestp[at] = x;
        A.dvec[at] = old - x;
        A.value[s] = bv;
    }
}

// The end of cycle `cyc` (0-based) for the n_act searches of act_in, by one workgroup: the ranges shrink around bestp (update not NaN), delta =
// sqrt(sum of the squared moves, left to right), the search stops converged at delta <= tol or unconverged after max_cycles cycles; then the
// searches that go on into act_out in ascending order (compact_push, smm_evalscratch.hpp) and their number into n_out.
__global__ __launch_bounds__(COMPACT_WG) void k_os_cycle_end(const KParams P, const OsArgs A, const int32_t* __restrict__ act_in, const int n_act, const int cyc,
                                                           int32_t* __restrict__ act_out, int32_t* __restrict__ n_out) {
    __shared__ CompactLds L;
    const int tid = (int)threadIdx.x, np = P.np;
    const size_t K = (size_t)A.K;
    compact_begin(L);
    for (int a_first = 0; a_first < n_act; a_first += COMPACT_WG) {
        const int a = a_first + tid;
        bool keep = false;
        int s = 0;
        if (a < n_act) {
            s = act_in[a];
            double acc = 0.0;
            for (int k = 0; k < np; ++k) {
                const size_t at = (size_t)k * K + s;
                if (A.update == A.update) {
                    const double l = A.lo[at], h = A.hi[at], x = A.bestp[at];
                    const double r = (h - l) / 2.0;
                    const double ur = A.update * r;
                    const double nl = x - ur, nh = x + ur;
                    A.lo[at] = l > nl ? l : nl;
                    A.hi[at] = h < nh ? h : nh;
                }
                const double d = A.dvec[at];
                const double sq = d * d;
                acc = k == 0 ? sq : acc + sq;
            }
            const double delta = __builtin_sqrt(acc);   // (IEEE square root: correctly rounded)
            A.delta[s] = delta;
            A.cycle_value[(size_t)cyc * K + s] = A.value[s];
            A.cycles[s] = cyc + 1;
            A.converged[s] = delta <= A.tol ? 1 : 0;
            keep = delta > A.tol && cyc + 1 < A.max_cycles;
        }
        compact_push(L, keep, s, act_out);
    }
    if (tid == 0) *n_out = L.base;
}
