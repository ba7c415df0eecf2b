// the starting population: candidates in the box and the install of every chain's start as its completed iteration 1 — part of libsmmhip
// (included by smmhip.hip inside its anonymous namespace; gfx950 device code).  Host side: smm_population_host.hpp; contract: include/smmhip.h
// (smm_set_population, smm_scatter_population).  Both kernels move a few hundred bytes per chain next to the evaluations between them.
#pragma once

// one batch of chains [c0, c0 + nb) of the context and their M candidates each, j = b * M + m the candidate's index in the batch (n = nb * M)
struct PopArgs {
    EvalScratch E;           // the candidates and their evaluations (smm_evalscratch.hpp)
    int c0, nb, M, n;
    double spread;
    int keep_init, force;    // force: candidate 0 is the start whatever it evaluates to (smm_set_population)
    double init_value;       // initial_value's evaluation
    int init_status;
    const double* init_simM; // [nm]
    double* rec_out;         // [N][RW] the last-accepted records
    double* o_start;         // [np][N]
    double* o_value;         // [N]
    int32_t* o_pick;         // [N]
    uint32_t* nan_flag;      // set when a NaN value is installed
};

// candidate m of global chain g, parameters 2q and 2q + 1 (include/smmhip.h: STREAM_POP): one thread per (candidate, parameter pair)
__global__ __launch_bounds__(256) void k_pop_candidates(const KParams P, const PopArgs A) {
    const int nq = (P.np + 1) >> 1;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)A.n * (size_t)nq) return;
    const size_t j = i / (size_t)nq;
    const int q = (int)(i % (size_t)nq);
    const uint32_t g = (uint32_t)(P.offset + A.c0 + (int)(j / (size_t)A.M)), m = (uint32_t)(j % (size_t)A.M);
    const U4 x = philox_stream(P.seed, STREAM_POP, g, m, (uint32_t)q, 0u);
    const double half = A.spread * 0.5;
    for (int h = 0; h < 2; ++h) {
        const int k = 2 * q + h;
        if (k >= P.np) break;
        const double u = h ? u53(x.z, x.w) : u53(x.x, x.y);
        const double lbk = P.lb[k], span = P.ub[k] - lbk;
        const double c01 = (P.init[k] - lbk) / span;            // mapto_01, mprob.jl:248
        const double lo = fmax(0.0, c01 - half), hi = fmin(1.0, c01 + half);
        const double step = u * (hi - lo);
        const double x01 = lo + step;
        const double sc = x01 * span;
        A.E.put_cand((size_t)A.n, j, k, sc + lbk);                // mapto_ab, mprob.jl:271
    }
}

// One wave per chain: the valid candidate with the lowest value, ties to the lowest m, by a butterfly over the lanes' (value, m); then the
// chain's completed iteration 1 from the winner's evaluation — exactly the fields iteration 1 of k_chain_iter leaves behind once settled
// (k_flush) and smm_set_state uploads for iter == 1: history row 0, the last-accepted record, the chain-state block.
constexpr int POP_WPB = 4;   // chains (waves) per workgroup
__global__ __launch_bounds__(64 * POP_WPB) void k_pop_select(const KParams P, const PopArgs A) {
    const int lane = (int)threadIdx.x & 63;
    const int b = (int)blockIdx.x * POP_WPB + ((int)threadIdx.x >> 6);
    if (b >= A.nb) return;   // (the whole wave)
    const int c = A.c0 + b, N = P.N, np = P.np, nm = P.nm;
    const size_t j0 = (size_t)b * (size_t)A.M;
    constexpr int NONE = 0x7fffffff;
    double bv = INFINITY;
    int bm = NONE;
    if (A.force) {
        bm = 0;
    } else {
        for (int m = lane; m < A.M; m += 64) {
            const double v = A.E.value_of(j0 + m);
            const int st = A.E.status_of(j0 + m);
            if (st >= 1 && v >= 0.0 && v < INFINITY && v < bv) { bv = v; bm = m; }   // (ascending m: an equal value keeps the lower one)
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {   // (value, m) in lexicographic order: every lane ends with the same winner
            const double ov = __shfl_xor(bv, off);
            const int om = __shfl_xor(bm, off);
            if (ov < bv || (ov == bv && om < bm)) { bv = ov; bm = om; }
        }
        const bool init_ok = A.init_status >= 1 && A.init_value >= 0.0 && A.init_value < INFINITY;
        if (bm == NONE || (A.keep_init && init_ok && A.init_value <= bv)) bm = -1;   // initial_value: candidate -1, wins ties
    }
    const int pick = bm;
    const size_t jw = j0 + (size_t)(pick < 0 ? 0 : pick);
    const double value = pick < 0 ? A.init_value : A.E.value_of(jw);
    double* hr = P.hrec + (size_t)c * P.HW;          // row 0
    double* ro = A.rec_out + (size_t)c * P.RW;
    for (int f = lane; f < np + nm; f += 64) {
        const double x = f < np ? (pick < 0 ? P.init[f] : A.E.cand[A.E.at(np, (size_t)A.n, jw, f)])
                                : (pick < 0 ? A.init_simM[f - np] : A.E.mom((size_t)A.n, jw, f - np));
        hr[H_PARAMS + f] = x;
        ro[3 + f] = x;
        if (f < np) A.o_start[(size_t)f * N + c] = x;
    }
    for (int f = H_PARAMS + np + nm + lane; f < P.HW; f += 64) hr[f] = 0.0;
    for (int f = 3 + np + nm + lane; f < P.RW; f += 64) ro[f] = 0.0;
    if (lane == 0) {
        // doAcceptReject! at iteration 1 (AlgoBGP.jl:326-332): accepted with prob 1 and status 1, whatever the evaluation said
        history_head(hr, value, 1.0, value, value, 1.0, 0.0, 1.0, 1.0);
        ro[0] = value; ro[1] = 1.0; ro[2] = 1.0;
        double* csb = P.cs + (size_t)c * CSW;        // (sigma and acc_tuner stay: iteration 1 updates neither)
        csb[CS_RATE] = 1.0; csb[CS_NNOEX] = 1.0; csb[CS_NACC] = 1.0; csb[CS_LACC] = 0.0; csb[CS_WASX] = 0.0;
        csb[CS_BEST] = value; csb[CS_BESTID] = 1.0; csb[CS_BESTP] = value; csb[CS_BESTPID] = 1.0;
        A.o_value[c] = value;
        A.o_pick[c] = pick;
        if (value != value) atomicOr(A.nan_flag, 1u);
    }
}
