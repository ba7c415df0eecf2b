// the host side of smm_opt_simplex (kernels: smm_optsimplex.hpp; the estimators' frame: smm_estimate_host.hpp) — part of libsmmhip (included
// once by smmhip.hip, behind smm_opt_slices' host side; hiprtc never sees it).  The searches go in batches whose state and launch scratch stay under the
// cap; a batch runs to its end before the next starts.  One lock-step iteration of a batch: k_sx_reflect -> evaluation of the running
// searches' xr -> k_sx_decide -> the searches that need a second point compacted -> k_sx_second -> evaluation -> k_sx_accept -> the searches
// that shrink compacted -> k_sx_shrink -> their vertices 1 .. N evaluated, one launch a vertex -> k_sx_sort -> the searches that go on
// compacted.  No launch evaluates more than one point per search, so the scratch of a launch is one evaluation per search.  The host reads
// three 4-byte counts per iteration — second-point, shrinking and running searches — which size the next launches; nothing else of the
// searches' state visits the host before the results are copied out.
#pragma once

namespace {

// bytes of state and launch scratch a search takes: per vertex its coordinates, moments, value and permutation entry; once more for a launch's
// candidate, moments, value and status; centroid, reflected point with moments and value, kind, flag, 3 list entries
size_t simplex_bytes_per_search(const KParams& P) {
    const size_t np = P.np, nm = P.nm;
    return (np + 2) * ((np + nm + 1) * 8 + 4) + (2 * np + nm + 1) * 8 + 20;
}

struct SimplexBufs {
    DevBuf<double> starts, sim, mom, fsim, xbar, xr, mr, fxr, s_cand, s_value, s_simM;
    DevBuf<int32_t> perm, kind, flag, run0, run1, second, shrink, count, s_status;
    DevBuf<double> best, value, sim_moments, simplex, simplex_value, size_x, size_f;
    DevBuf<int32_t> iterations, status, moves, n_eval;
    SimplexBufs(const KParams& P, size_t K, size_t nb)
        : starts(K * P.np), sim(nb * (P.np + 1) * P.np), mom(nb * (P.np + 1) * P.nm), fsim(nb * (P.np + 1)), xbar(nb * P.np), xr(nb * P.np),
          mr(nb * P.nm), fxr(nb), s_cand(nb * P.np), s_value(nb), s_simM(nb * P.nm),
          perm(nb * (P.np + 1)), kind(nb), flag(nb), run0(nb), run1(nb), second(nb), shrink(nb), count(1), s_status(nb),
          best(K * P.np), value(K), sim_moments(K * P.nm), simplex(K * (P.np + 1) * P.np), simplex_value(K * (P.np + 1)), size_x(K), size_f(K),
          iterations(K), status(K), moves(K * 5), n_eval(K) {}
};

}  // namespace

extern "C" {

int smm_opt_simplex(void* ctx, const double* starts, int32_t K, double step, int32_t adaptive, double xatol, double fatol, int32_t max_iter,
                    smm_opt_simplex_t* out) {
    return api_call(ctx, true, [&](Ctx* c) -> int {
        if (const int rc = estimate_enter(c)) return rc;
        const KParams& P = c->P;
        if (!starts) return fail(c, SMM_ERR_INVALID_ARG, "smm_opt_simplex: starts is NULL");
        if (K < 1) return fail(c, SMM_ERR_INVALID_ARG, "smm_opt_simplex: K < 1");
        if ((int64_t)K * (int64_t)(P.np + 1) >= ((int64_t)1 << 31)) return fail(c, SMM_ERR_INVALID_ARG, "smm_opt_simplex: K x (np + 1) must stay below 2^31");
        if (!(step > 0.0 && step <= 1.0)) return fail(c, SMM_ERR_INVALID_ARG, "smm_opt_simplex: step must be in (0, 1]");
        if (!(xatol >= 0.0)) return fail(c, SMM_ERR_INVALID_ARG, "smm_opt_simplex: xatol must be >= 0");
        if (!(fatol >= 0.0)) return fail(c, SMM_ERR_INVALID_ARG, "smm_opt_simplex: fatol must be >= 0");
        if (max_iter < 1) return fail(c, SMM_ERR_INVALID_ARG, "smm_opt_simplex: max_iter < 1");
        static_assert(MAX_DIM <= 64, "the state kernels take a lane per coordinate");
        const size_t Ks = (size_t)K, np = P.np, nm = P.nm, V = np + 1;
        const int N = P.np;
        if (const int rc = starts_in_box(c, "smm_opt_simplex", "search", 1, starts, Ks)) return rc;
        const int nb_max = batch_size(c, Ks, simplex_bytes_per_search(P));
        SimplexBufs B(P, Ks, (size_t)nb_max);
        SxArgs A{};
        A.K = K; A.max_iter = max_iter; A.xatol = xatol; A.fatol = fatol; A.step = step;
        // the coefficients and their products, once, in double, as Python computes them
        const double dim = (double)N;
        const double rho = 1.0, chi = adaptive ? 1.0 + 2.0 / dim : 2.0, psi = adaptive ? 0.75 - 1.0 / (2.0 * dim) : 0.5, sigma = adaptive ? 1.0 - 1.0 / dim : 0.5;
        A.rho = rho; A.c_r = 1.0 + rho;
        A.rhochi = rho * chi; A.c_e = 1.0 + A.rhochi;
        A.psirho = psi * rho; A.c_c = 1.0 + A.psirho;
        A.psi = psi; A.c_i = 1.0 - psi;
        A.sigma = sigma;
        A.sim = B.sim.p; A.mom = B.mom.p; A.fsim = B.fsim.p; A.perm = B.perm.p; A.xbar = B.xbar.p; A.xr = B.xr.p; A.mr = B.mr.p; A.fxr = B.fxr.p;
        A.kind = B.kind.p; A.flag = B.flag.p; A.E = eval_scratch(c, B.s_cand.p, B.s_value.p, B.s_simM.p, B.s_status.p);
        A.best = B.best.p; A.value = B.value.p; A.sim_moments = B.sim_moments.p; A.simplex = B.simplex.p; A.simplex_value = B.simplex_value.p;
        A.size_x = B.size_x.p; A.size_f = B.size_f.p; A.iterations = B.iterations.p; A.status = B.status.p; A.moves = B.moves.p; A.n_eval = B.n_eval.p;
        HIPCHK(hipMemcpyAsync(B.starts.p, starts, Ks * np * 8, hipMemcpyHostToDevice, c->stream));
        int32_t* run[2] = {B.run0.p, B.run1.p};
        const dim3 wave(64);
        // the flagged entries of `list` (nullptr: the batch) into `to`; their number comes back: the one read of a phase
        auto compact = [&](const int32_t* list, int n_in, int32_t* to) { return compact_count(c, list, n_in, A.flag, to, B.count.p); };
        auto eval = [&](size_t n) { launch_eval_dev(c, A.E, (int)n); };
        int64_t evaluated = 0;
        // the vertices at positions p0 .. p1 of the listed searches (nullptr: the batch), a launch of n evaluations per position, filed as evaluated
        auto evaluate_vertices = [&](const int32_t* list, int n, int p0, int p1) {
            for (int pos = p0; pos <= p1; ++pos) {
                hipLaunchKernelGGL(k_sx_vertex, dim3((unsigned)n), wave, 0, c->stream, P, A, list, pos, (size_t)n);
                HIPCHK(hipGetLastError());
                eval((size_t)n);
                hipLaunchKernelGGL(k_sx_store, dim3((unsigned)n), wave, 0, c->stream, P, A, list, pos, (size_t)n);
                HIPCHK(hipGetLastError());
            }
            evaluated += (int64_t)n * (int64_t)(p1 - p0 + 1);
        };
        for (int s0 = 0; s0 < K; s0 += nb_max) {
            const int nb = std::min(nb_max, K - s0);
            A.s0 = s0; A.nb = nb;
            hipLaunchKernelGGL(k_sx_init, dim3((unsigned)nb), wave, 0, c->stream, P, A, (const double*)B.starts.p);
            HIPCHK(hipGetLastError());
            evaluate_vertices(nullptr, nb, 0, N);
            hipLaunchKernelGGL(k_sx_sort, dim3((unsigned)nb), wave, 0, c->stream, P, A, (const int32_t*)nullptr, 0);
            HIPCHK(hipGetLastError());
            int n_run = compact(nullptr, nb, run[0]);
            for (int it = 0; n_run > 0; ++it) {
                const int32_t* cur = run[it & 1];
                const size_t n1 = (size_t)n_run;
                hipLaunchKernelGGL(k_sx_reflect, dim3((unsigned)n_run), wave, 0, c->stream, P, A, cur, n1);
                HIPCHK(hipGetLastError());
                eval(n1);
                hipLaunchKernelGGL(k_sx_decide, dim3((unsigned)n_run), wave, 0, c->stream, P, A, cur, n1);
                HIPCHK(hipGetLastError());
                evaluated += (int64_t)n1;
                const int n_second = compact(cur, n_run, B.second.p);
                if (n_second > 0) {
                    const size_t n2 = (size_t)n_second;
                    hipLaunchKernelGGL(k_sx_second, dim3((unsigned)n_second), wave, 0, c->stream, P, A, (const int32_t*)B.second.p, n2);
                    HIPCHK(hipGetLastError());
                    eval(n2);
                    hipLaunchKernelGGL(k_sx_accept, dim3((unsigned)n_second), wave, 0, c->stream, P, A, (const int32_t*)B.second.p, n2);
                    HIPCHK(hipGetLastError());
                    evaluated += (int64_t)n2;
                    const int n_shrink = compact(B.second.p, n_second, B.shrink.p);
                    if (n_shrink > 0) {
                        hipLaunchKernelGGL(k_sx_shrink, dim3((unsigned)n_shrink, (unsigned)N), wave, 0, c->stream, P, A, (const int32_t*)B.shrink.p);
                        HIPCHK(hipGetLastError());
                        evaluate_vertices(B.shrink.p, n_shrink, 1, N);
                    }
                }
                hipLaunchKernelGGL(k_sx_sort, dim3((unsigned)n_run), wave, 0, c->stream, P, A, cur, 1);
                HIPCHK(hipGetLastError());
                n_run = compact(cur, n_run, run[(it & 1) ^ 1]);
            }
            hipLaunchKernelGGL(k_sx_finish, dim3((unsigned)nb), wave, 0, c->stream, P, A);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipStreamSynchronize(c->stream));
        if (out) {
            const Download down{c};
            down(out->best, B.best.p, Ks * np); down(out->value, B.value.p, Ks); down(out->sim_moments, B.sim_moments.p, Ks * nm);
            down(out->simplex, B.simplex.p, Ks * V * np); down(out->simplex_value, B.simplex_value.p, Ks * V);
            down(out->size_x, B.size_x.p, Ks); down(out->size_f, B.size_f.p, Ks);
            down(out->iterations, B.iterations.p, Ks); down(out->status, B.status.p, Ks); down(out->moves, B.moves.p, Ks * 5);
            down(out->n_eval, B.n_eval.p, Ks);
            HIPCHK(hipStreamSynchronize(c->stream));
            out->evaluated = evaluated;
        }
        return SMM_OK;
    });
}

}  // extern "C"
