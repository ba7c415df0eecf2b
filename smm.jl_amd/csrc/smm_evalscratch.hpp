// what the estimators that evaluate many points off the chains share on the device — the starting population, smm_opt_slices,
// smm_opt_simplex, smm_opt_lm, smm_abc_pmc, smm_sens_sobol: the view of one evaluation launch's scratch, the evaluation tile on points that are never
// written, and the compaction of a list — part of libsmmhip (included by smmhip.hip inside its anonymous namespace, in front of
// smm_population.hpp; gfx950 device code; hiprtc never sees it).  Host side: smm_estimate_host.hpp.
#pragma once

// One launch's scratch of n evaluations, in the layouts the evaluation kernels fix (launch_eval_dev): the built-in objectives read the
// candidates [np][n] and write simM [nm][n] and status as int8; a user objective's kernel reads [n][np] and writes [n][nm] and status as int.
// Evaluation i of n, parameter k, moment f.
struct EvalScratch {
    double* cand;
    double* value;           // [n]
    double* simM;
    void* status;            // [n]
    int user;                // 1: a user objective's layouts
    int np, nm;
    __device__ size_t at(const int width, const size_t n, const size_t i, const int k) const {
        return user ? i * (size_t)width + (size_t)k : (size_t)k * n + i;
    }
    __device__ void put_cand(const size_t n, const size_t i, const int k, const double x) const { cand[at(np, n, i, k)] = x; }
    __device__ double mom(const size_t n, const size_t i, const int f) const { return simM[at(nm, n, i, f)]; }
    __device__ double value_of(const size_t i) const { return value[i]; }
    __device__ int status_of(const size_t i) const { return user ? ((const int*)status)[i] : (int)((const int8_t*)status)[i]; }
    // evaluation 0's status from the first four bytes of `status`, read back
    __host__ __device__ int status_of_word(const int32_t w) const { return user ? (int)w : (int)(int8_t)(w & 0xff); }
};

// eval_tile (smm_chain.hpp) on points that are never written: every lane takes part in the fill, np loads per evaluation, the evaluations
// of a tile side by side in every column; theta_of(ie, j) is parameter j of evaluation ie < n
template <int KIND, int CT, class ThetaOf>
__device__ __forceinline__ void eval_tile_of(const KParams& P, const int n, ThetaOf theta_of, const EvalScratch& E, int8_t* __restrict__ status) {
    eval_tile<KIND, CT>(P, n, [&](const TileSmem& S, const int tid) {
        for (int e = tid; e < CT * P.np; e += WG) {
            const int cl = e / P.np, j = e - cl * P.np, ie = blockIdx.x * CT + cl;
            S.theta[e] = ie < n ? theta_of(ie, j) : 0.0;
        }
    }, E.value, E.simM, status);
}

// The compaction of a list by ONE workgroup of COMPACT_WG: the items whose lane says `keep` into `out` in ascending order of the passes and
// of the lanes within a pass — ballots and prefix counts, no atomics.  Every lane of the workgroup calls compact_begin once, compact_push
// once per pass, and reads the number kept so far from L.base behind it.
constexpr int COMPACT_WG = 1024;
struct CompactLds { int wtot[COMPACT_WG / 64]; int base; };
__device__ inline void compact_begin(CompactLds& L) {
    if (threadIdx.x == 0) L.base = 0;
    __syncthreads();
}
__device__ inline void compact_push(CompactLds& L, const bool keep, const int32_t item, int32_t* __restrict__ out) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long m = __ballot(keep);
    if (lane == 0) L.wtot[wave] = __popcll(m);
    __syncthreads();
    int before = L.base;
    for (int w = 0; w < wave; ++w) before += L.wtot[w];
    if (keep) out[before + __popcll(m & ((1ull << lane) - 1ull))] = item;
    __syncthreads();
    if (tid == 0) {
        int tot = L.base;
        for (int w = 0; w < COMPACT_WG / 64; ++w) tot += L.wtot[w];
        L.base = tot;
    }
    __syncthreads();
}

// the entries of list_in (nullptr: 0 .. n_in - 1) whose flag is set into list_out, their number into n_out
__global__ __launch_bounds__(COMPACT_WG) void k_compact(const int32_t* __restrict__ list_in, const int n_in, const int32_t* __restrict__ flag,
                                                        int32_t* __restrict__ list_out, int32_t* __restrict__ n_out) {
    __shared__ CompactLds L;
    compact_begin(L);
    for (int a_first = 0; a_first < n_in; a_first += COMPACT_WG) {
        const int a = a_first + (int)threadIdx.x;
        bool keep = false;
        int b = 0;
        if (a < n_in) {
            b = list_in ? list_in[a] : a;
            keep = flag[b] != 0;
        }
        compact_push(L, keep, b, list_out);
    }
    if (threadIdx.x == 0) *n_out = L.base;
}
