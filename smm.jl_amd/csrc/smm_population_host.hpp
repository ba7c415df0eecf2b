// the host side of the starting population (smm_set_population, smm_scatter_population; kernels: smm_population.hpp) — part of libsmmhip
// (included once by smmhip.hip, behind the estimators' frame, smm_estimate_host.hpp; hiprtc never sees it).  Both calls share one frame:
// settle and refuse (pop_enter), evaluate initial_value or nothing, then per batch of chains candidates -> the context's evaluation kernel
// on device pointers (launch_eval_dev) -> k_pop_select, which writes the chains' completed iteration 1; then the bookkeeping of
// smm_set_state for iter == 1.
#pragma once

namespace {

// bytes of candidate and result scratch a batch of chains may take (the test seam SMMHIP_POP_SCRATCH replaces the cap)
constexpr size_t POP_SCRATCH_CAP = (size_t)64 << 20;
size_t pop_scratch_cap(const Ctx* c) { return c->H.pop_scratch ? c->H.pop_scratch : POP_SCRATCH_CAP; }

// the device buffers of one call
struct PopBufs {
    DevBuf<double> cand, value, simM, i_value, i_simM, o_start, o_value;
    DevBuf<int32_t> status, i_status, o_pick;
    DevBuf<uint32_t> flag;
    PopBufs(const KParams& P, size_t n)
        : cand(n * P.np), value(n), simM(n * P.nm), i_value(1), i_simM(P.nm), o_start((size_t)P.np * P.N), o_value(P.N), status(n), i_status(1),
          o_pick(P.N), flag(1) {}
};

// what both calls do before they look at their arguments: the estimators' prologue, then refuse a failed context and one that has stepped
int pop_enter(Ctx* c) {
    if (const int rc = estimate_enter(c)) return rc;
    if (c->failed) return told(c);
    if (c->run.iter != 0) return fail(c, SMM_ERR_STATE, "the starting population is installed before the first iteration only (completed iterations: " + std::to_string(c->run.iter) + ")");
    if (c->P.T < 1) return fail(c, SMM_ERR_MAXITER, "maxiter == 0: no room for the chains' first iteration");
    return SMM_OK;
}

void pop_launch_select(Ctx* c, const PopArgs& A) {
    hipLaunchKernelGGL(k_pop_select, dim3((unsigned)((A.nb + POP_WPB - 1) / POP_WPB)), dim3(64 * POP_WPB), 0, c->stream, c->P, A);
    HIPCHK(hipGetLastError());
}

// behind the last k_pop_select: results out, then the context stands at iteration 1 as after smm_set_state with iter == 1
void pop_finish(Ctx* c, PopBufs& B, smm_population_t* out, int64_t evaluated, int kind, int M, double spread) {
    const KParams& P = c->P;
    uint32_t flag = 0;
    HIPCHK(hipMemcpyAsync(&flag, B.flag.p, 4, hipMemcpyDeviceToHost, c->stream));
    if (out) {
        const Download down{c};
        down(out->start, B.o_start.p, (size_t)P.np * P.N); down(out->value, B.o_value.p, (size_t)P.N); down(out->pick, B.o_pick.p, (size_t)P.N);
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    if (out) out->evaluated = evaluated;
    c->nan_values = flag != 0u;
    c->run.iter = 1;
    c->rec_external = false; c->pending_ext = false; c->run.unresolved = false;
    c->run.pending = false;
    c->run.prev_open = false;
    c->a2a_open = false;
    c->p2p_current = false;
    c->run.exch_done = false;
    c->run.slots_iter = -1;
    if (P.walk_flags) HIPCHK(hipMemset(P.walk_flags, 0, 16));
    c->pop_kind = kind; c->pop_M = M; c->pop_spread = spread;
}

PopArgs pop_args(Ctx* c, PopBufs& B) {
    PopArgs A{};
    A.E = eval_scratch(c, B.cand.p, B.value.p, B.simM.p, B.status.p);
    A.init_simM = B.i_simM.p;
    A.rec_out = c->rec[c->run.cur];
    A.o_start = B.o_start.p; A.o_value = B.o_value.p; A.o_pick = B.o_pick.p; A.nan_flag = B.flag.p;
    return A;
}

}  // namespace

extern "C" {

int smm_set_population(void* ctx, const double* starts, smm_population_t* out) {
    return api_call(ctx, true, [&](Ctx* c) -> int {
        if (const int rc = pop_enter(c)) return rc;
        if (!starts) return fail(c, SMM_ERR_INVALID_ARG, "smm_set_population: starts is NULL");
        const KParams& P = c->P;
        const size_t N = P.N, np = P.np;
        if (const int rc = starts_in_box(c, "smm_set_population", "chain", P.offset + 1, starts, N)) return rc;
        PopBufs B(P, N);
        PopArgs A = pop_args(c, B);
        std::vector<double> tp;   // (alive until pop_finish has synchronised)
        if (A.E.user) {   // a user objective's kernel reads [N][np]
            tp.resize(N * np);
            for (size_t i = 0; i < N; ++i)
                for (size_t k = 0; k < np; ++k) tp[i * np + k] = starts[k * N + i];
        }
        HIPCHK(hipMemcpyAsync(B.cand.p, A.E.user ? tp.data() : starts, N * np * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemsetAsync(B.flag.p, 0, 4, c->stream));
        launch_eval_dev(c, A.E, (int)N);
        A.c0 = 0; A.nb = (int)N; A.M = 1; A.n = (int)N; A.force = 1;
        pop_launch_select(c, A);
        pop_finish(c, B, out, (int64_t)N, 1, 0, 0.0);
        return SMM_OK;
    });
}

int smm_scatter_population(void* ctx, int32_t M, double spread, int32_t keep_init, smm_population_t* out) {
    return api_call(ctx, true, [&](Ctx* c) -> int {
        if (const int rc = pop_enter(c)) return rc;
        const KParams& P = c->P;
        if (M < 1) return fail(c, SMM_ERR_INVALID_ARG, "smm_scatter_population: M < 1");
        if (!(spread > 0.0 && spread <= 1.0)) return fail(c, SMM_ERR_INVALID_ARG, "smm_scatter_population: spread must lie in (0, 1]");
        if ((int64_t)M * (int64_t)P.Ng >= ((int64_t)1 << 31)) return fail(c, SMM_ERR_INVALID_ARG, "smm_scatter_population: M x N_global must stay below 2^31");
        const size_t per_chain = (size_t)M * ((size_t)(P.np + P.nm + 1) * 8 + 4);
        const int nb_max = batch_size(pop_scratch_cap(c), (size_t)P.N, per_chain);
        PopBufs B(P, (size_t)nb_max * (size_t)M);
        PopArgs A = pop_args(c, B);
        HIPCHK(hipMemsetAsync(B.flag.p, 0, 4, c->stream));
        // initial_value, once: every chain's candidate -1 (the evaluation is the same for all of them, a stream objective's draws included)
        launch_eval_dev(c, P.init, 1, B.i_value.p, B.i_simM.p, B.i_status.p);
        int32_t ist = 0;
        HIPCHK(hipMemcpyAsync(&A.init_value, B.i_value.p, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(&ist, B.i_status.p, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        A.init_status = A.E.status_of_word(ist);
        A.M = M; A.spread = spread; A.keep_init = keep_init != 0; A.force = 0;
        for (int c0 = 0; c0 < P.N; c0 += nb_max) {
            A.c0 = c0; A.nb = std::min(nb_max, P.N - c0); A.n = A.nb * M;
            const size_t work = (size_t)A.n * (size_t)((P.np + 1) / 2);
            hipLaunchKernelGGL(k_pop_candidates, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, c->stream, P, A);
            HIPCHK(hipGetLastError());
            launch_eval_dev(c, A.E, A.n);
            pop_launch_select(c, A);
        }
        pop_finish(c, B, out, (int64_t)M * P.N + 1, 2, M, spread);
        return SMM_OK;
    });
}

}  // extern "C"
