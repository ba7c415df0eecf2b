// the host side of smm_opt_lm (kernels: smm_optlm.hpp; the estimators' frame: smm_estimate_host.hpp) — part of libsmmhip (included once by
// smmhip.hip, behind smm_opt_simplex' host side; hiprtc never sees it).  The searches go in batches whose state and launch scratch stay under
// the cap; a batch runs to its end before the next starts.  One lock-step iteration of a batch: the Jacobian's np points of every running
// search in ONE evaluation launch (the built-in objectives: k_eval_lm, the points never written; a user objective: k_lm_candidates and its
// own kernel) -> k_lm_normal -> rounds of tries, the first over all running searches (those that stopped at their normal equations pad it),
// the later ones over the compacted list of the searches that try again: k_lm_step -> evaluation of one point per listed search ->
// k_lm_judge -> compaction -> and the searches that go on compacted.  The host reads one 4-byte count per round of tries and one per
// iteration, which size the next launches; nothing else of the searches' state visits the host before the results are copied out.
#pragma once

namespace {

// bytes of state and launch scratch a search takes: the Jacobian launch's np evaluations (moments, value, status; a user objective's points
// too, else one trial point), its residuals, A, trial point, four flags and counts and four list entries
size_t lm_bytes_per_search(const KParams& P, bool user) {
    const size_t np = P.np, nm = P.nm;
    return np * ((nm + 1) * 8 + 4) + (user ? np * np : np) * 8 + (nm + np * np + np) * 8 + 32;
}

struct LmBufs {
    DevBuf<double> starts, r, A, xnew, s_cand, s_value, s_simM;
    DevBuf<int32_t> itry, piv, f_try, f_go, run0, run1, trying0, trying1, count, s_status;
    DevBuf<double> best, value, sim_moments, ssr, grad, jac, lambda, step, dF;
    DevBuf<int32_t> active, iterations, tries, n_eval, status;
    LmBufs(const KParams& P, size_t K, size_t nb, bool user, bool jac_wanted)
        : starts(K * P.np), r(nb * P.nm), A(nb * P.np * P.np), xnew(nb * P.np), s_cand(nb * P.np * (user ? P.np : 1)), s_value(nb * P.np),
          s_simM(nb * P.np * P.nm), itry(nb), piv(nb), f_try(nb), f_go(nb), run0(nb), run1(nb), trying0(nb), trying1(nb), count(1),
          s_status(nb * P.np), best(K * P.np), value(K), sim_moments(K * P.nm), ssr(K), grad(K * P.np),
          jac(jac_wanted ? K * P.nm * P.np : 1), lambda(K), step(K), dF(K), active(K * P.np), iterations(K), tries(K), n_eval(K), status(K) {}
};

}  // namespace

extern "C" {

int smm_opt_lm(void* ctx, const double* starts, int32_t K, double fd_step, double lambda0, double lambda_up, double lambda_down, double xtol,
               double ftol, double gtol, int32_t max_iter, int32_t max_tries, smm_opt_lm_t* out) {
    return api_call(ctx, true, [&](Ctx* c) -> int {
        if (const int rc = estimate_enter(c)) return rc;
        const KParams& P = c->P;
        if (!starts) return fail(c, SMM_ERR_INVALID_ARG, "smm_opt_lm: starts is NULL");
        if (K < 1) return fail(c, SMM_ERR_INVALID_ARG, "smm_opt_lm: K < 1");
        if ((int64_t)K * (int64_t)P.np >= ((int64_t)1 << 31)) return fail(c, SMM_ERR_INVALID_ARG, "smm_opt_lm: K x np must stay below 2^31");
        if (!(fd_step > 0.0 && fd_step <= 0.5)) return fail(c, SMM_ERR_INVALID_ARG, "smm_opt_lm: fd_step must be in (0, 0.5]");
        if (!(lambda0 > 0.0 && lambda0 - lambda0 == 0.0)) return fail(c, SMM_ERR_INVALID_ARG, "smm_opt_lm: lambda0 must be > 0 and finite");
        if (!(lambda_up > 1.0)) return fail(c, SMM_ERR_INVALID_ARG, "smm_opt_lm: lambda_up must be > 1");
        if (!(lambda_down >= 1.0)) return fail(c, SMM_ERR_INVALID_ARG, "smm_opt_lm: lambda_down must be >= 1");
        if (!(xtol >= 0.0)) return fail(c, SMM_ERR_INVALID_ARG, "smm_opt_lm: xtol must be >= 0");
        if (!(ftol >= 0.0)) return fail(c, SMM_ERR_INVALID_ARG, "smm_opt_lm: ftol must be >= 0");
        if (!(gtol >= 0.0)) return fail(c, SMM_ERR_INVALID_ARG, "smm_opt_lm: gtol must be >= 0");
        if (max_iter < 1) return fail(c, SMM_ERR_INVALID_ARG, "smm_opt_lm: max_iter < 1");
        if (max_tries < 1) return fail(c, SMM_ERR_INVALID_ARG, "smm_opt_lm: max_tries < 1");
        static_assert(MAX_DIM <= 64, "the state kernels take a lane per parameter");
        const size_t Ks = (size_t)K, np = P.np, nm = P.nm;
        const int N = P.np;
        if (const int rc = starts_in_box(c, "smm_opt_lm", "search", 1, starts, Ks)) return rc;
        const bool user = c->obj == SMM_OBJ_USER;
        const int nb_max = batch_size(c, Ks, lm_bytes_per_search(P, user));
        LmBufs B(P, Ks, (size_t)nb_max, user, out && out->jac);
        LmArgs A{};
        A.K = K; A.max_iter = max_iter; A.max_tries = max_tries;
        A.fd_step = fd_step; A.lambda0 = lambda0; A.lambda_up = lambda_up; A.lambda_down = lambda_down; A.xtol = xtol; A.ftol = ftol; A.gtol = gtol;
        A.r = B.r.p; A.A = B.A.p; A.xnew = B.xnew.p; A.itry = B.itry.p; A.piv = B.piv.p; A.f_try = B.f_try.p; A.f_go = B.f_go.p;
        A.E = eval_scratch(c, B.s_cand.p, B.s_value.p, B.s_simM.p, B.s_status.p);
        A.best = B.best.p; A.value = B.value.p; A.sim_moments = B.sim_moments.p; A.ssr = B.ssr.p; A.grad = B.grad.p;
        A.jac = out && out->jac ? B.jac.p : nullptr;
        A.lambda = B.lambda.p; A.step = B.step.p; A.dF = B.dF.p; A.active = B.active.p; A.iterations = B.iterations.p; A.tries = B.tries.p;
        A.n_eval = B.n_eval.p; A.status = B.status.p;
        HIPCHK(hipMemcpyAsync(B.starts.p, starts, Ks * np * 8, hipMemcpyHostToDevice, c->stream));
        const size_t lds_normal = (nm * np + nm) * 8, lds_step = (np * (np + 1) + np + 1) * 8;
        int32_t* run[2] = {B.run0.p, B.run1.p};
        int32_t* trying[2] = {B.trying0.p, B.trying1.p};
        const dim3 wave(64);
        // the entries of `list` (nullptr: the batch) whose flag is set into `to`; their number comes back: the one read of a phase
        auto compact = [&](const int32_t* list, int n_in, const int32_t* flag, int32_t* to) { return compact_count(c, list, n_in, flag, to, B.count.p); };
        // the np Jacobian points of each of the n_run searches of `list`
        auto eval_jacobian = [&](const int32_t* list, int n_run) {
            const int n = n_run * N;
            if (user) {
                const size_t work = (size_t)n * np;
                hipLaunchKernelGGL(k_lm_candidates, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, c->stream, P, A, list, (size_t)n);
                HIPCHK(hipGetLastError());
                launch_eval_dev(c, A.E, n);
                return;
            }
            int8_t* st = (int8_t*)A.E.status;
            void* args[] = {(void*)&P, (void*)&A, (void*)&list, (void*)&n, (void*)&st};
            launch_eval_tiles(c, EF_LM, n, args);
        };
        for (int s0 = 0; s0 < K; s0 += nb_max) {
            const int nb = std::min(nb_max, K - s0);
            A.s0 = s0; A.nb = nb;
            hipLaunchKernelGGL(k_lm_init, dim3((unsigned)nb), wave, 0, c->stream, P, A, (const double*)B.starts.p);
            HIPCHK(hipGetLastError());
            launch_eval_dev(c, A.E, nb);
            hipLaunchKernelGGL(k_lm_start, dim3((unsigned)nb), wave, 0, c->stream, P, A);
            HIPCHK(hipGetLastError());
            int n_run = compact(nullptr, nb, A.f_go, run[0]);
            for (int it = 0; n_run > 0; ++it) {
                const int32_t* cur = run[it & 1];
                eval_jacobian(cur, n_run);
                hipLaunchKernelGGL(k_lm_normal, dim3((unsigned)n_run), wave, lds_normal, c->stream, P, A, cur, (size_t)n_run * np);
                HIPCHK(hipGetLastError());
                const int32_t* tl = cur;
                int n_try = n_run;
                for (int round = 0; n_try > 0; ++round) {
                    const size_t n = (size_t)n_try;
                    hipLaunchKernelGGL(k_lm_step, dim3((unsigned)n_try), wave, lds_step, c->stream, P, A, tl, n);
                    HIPCHK(hipGetLastError());
                    launch_eval_dev(c, A.E, n_try);
                    hipLaunchKernelGGL(k_lm_judge, dim3((unsigned)n_try), wave, 0, c->stream, P, A, tl, n);
                    HIPCHK(hipGetLastError());
                    int32_t* to = trying[round & 1];
                    n_try = compact(tl, n_try, A.f_try, to);
                    tl = to;
                }
                n_run = compact(cur, n_run, A.f_go, run[(it & 1) ^ 1]);
            }
        }
        HIPCHK(hipStreamSynchronize(c->stream));
        if (out) {
            const Download down{c};
            down(out->best, B.best.p, Ks * np); down(out->value, B.value.p, Ks); down(out->sim_moments, B.sim_moments.p, Ks * nm);
            down(out->ssr, B.ssr.p, Ks); down(out->grad, B.grad.p, Ks * np); down(out->jac, B.jac.p, Ks * nm * np);
            down(out->lambda, B.lambda.p, Ks); down(out->step, B.step.p, Ks); down(out->dF, B.dF.p, Ks);
            down(out->active, B.active.p, Ks * np); down(out->iterations, B.iterations.p, Ks); down(out->tries, B.tries.p, Ks);
            down(out->n_eval, B.n_eval.p, Ks); down(out->status, B.status.p, Ks);
            std::vector<int32_t> ne(Ks);
            HIPCHK(hipMemcpyAsync(ne.data(), B.n_eval.p, Ks * 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            int64_t evaluated = 0;
            for (size_t s = 0; s < Ks; ++s) evaluated += ne[s];
            out->evaluated = evaluated;
        }
        return SMM_OK;
    });
}

}  // extern "C"
