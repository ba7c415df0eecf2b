// the host side of smm_opt_slices (kernels: smm_optslices.hpp; the estimators' frame: smm_estimate_host.hpp) — part of libsmmhip (included once
// by smmhip.hip, behind the starting population's host side; hiprtc never sees it).  The loop: per cycle and parameter one evaluation
// launch over the running searches' grid points and k_os_select, per cycle k_os_cycle_end and ONE 4-byte read-back — the number of searches
// that go on — which sizes the next cycle's launches and ends the loop.  Nothing else of the searches' state visits the host before the
// results are copied out.
#pragma once

namespace {

// the device buffers of one call
struct OptBufs {
    DevBuf<double> bestp, lo, hi, dvec, value, simM, delta, cycle_value, s_cand, s_value, s_simM;
    DevBuf<int32_t> cycles, converged, act0, act1, n_act, s_status;
    OptBufs(const KParams& P, size_t K, size_t max_cycles, size_t n, bool cand)
        : bestp(K * P.np), lo(K * P.np), hi(K * P.np), dvec(K * P.np), value(K), simM(K * P.nm), delta(K), cycle_value(K * max_cycles),
          s_cand(cand ? n * P.np : 1), s_value(n), s_simM(n * P.nm), cycles(K), converged(K), act0(K), act1(K), n_act(1), s_status(n) {}
};

// coordinate k of the running searches [a0, a0 + nb) of `act`: their n = nb x G grid points evaluated into the step scratch
void opt_launch_eval(Ctx* c, const OsArgs& A, const int32_t* act, int k, int a0, int nb, bool materialise) {
    const KParams& P = c->P;
    const int n = nb * A.G;
    if (materialise) {
        const size_t work = (size_t)n * (size_t)P.np;
        hipLaunchKernelGGL(k_os_candidates, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, c->stream, P, A, act, k, a0, n);
        HIPCHK(hipGetLastError());
        launch_eval_dev(c, A.E, n);
        return;
    }
    int8_t* st = (int8_t*)A.E.status;
    void* args[] = {(void*)&P, (void*)&A, (void*)&act, (void*)&k, (void*)&a0, (void*)&n, (void*)&st};
    launch_eval_tiles(c, EF_SLICE, n, args);
}

}  // namespace

extern "C" {

int smm_opt_slices(void* ctx, const double* starts, int32_t K, int32_t npoints, double tol, double update, int32_t max_cycles, smm_opt_slices_t* out) {
    return api_call(ctx, true, [&](Ctx* c) -> int {
        if (const int rc = estimate_enter(c)) return rc;
        if (!starts) return fail(c, SMM_ERR_INVALID_ARG, "smm_opt_slices: starts is NULL");
        if (K < 1) return fail(c, SMM_ERR_INVALID_ARG, "smm_opt_slices: K < 1");
        if (npoints < 2) return fail(c, SMM_ERR_INVALID_ARG, "smm_opt_slices: npoints < 2");
        if ((int64_t)K * (int64_t)npoints >= ((int64_t)1 << 31)) return fail(c, SMM_ERR_INVALID_ARG, "smm_opt_slices: K x npoints must stay below 2^31");
        if (!(tol >= 0.0)) return fail(c, SMM_ERR_INVALID_ARG, "smm_opt_slices: tol must be >= 0");
        if (update == update && !(update > 0.0)) return fail(c, SMM_ERR_INVALID_ARG, "smm_opt_slices: update must be > 0 (NaN: the ranges never shrink)");
        if (max_cycles < 1) return fail(c, SMM_ERR_INVALID_ARG, "smm_opt_slices: max_cycles < 1");
        const KParams& P = c->P;
        const size_t Ks = (size_t)K, np = P.np, nm = P.nm, G = (size_t)npoints;
        if (const int rc = starts_in_box(c, "smm_opt_slices", "search", 1, starts, Ks)) return rc;
        const bool user = c->obj == SMM_OBJ_USER;
        const bool materialise = user || c->H.opt_materialise;   // (a user objective's kernel reads a matrix; the hook: the timing experiment)
        // a step's values, moments and status (and candidates, where they are materialised) per search; the running searches go in batches
        const size_t per_search = G * ((nm + 1) * 8 + 4 + (materialise ? np * 8 : 0));
        const int nb_max = batch_size(c, Ks, per_search);
        OptBufs B(P, Ks, (size_t)max_cycles, (size_t)nb_max * G, materialise);
        OsArgs A{};
        A.K = K; A.G = npoints; A.max_cycles = max_cycles; A.tol = tol; A.update = update;
        A.bestp = B.bestp.p; A.lo = B.lo.p; A.hi = B.hi.p; A.dvec = B.dvec.p; A.value = B.value.p; A.simM = B.simM.p; A.delta = B.delta.p;
        A.cycle_value = B.cycle_value.p; A.cycles = B.cycles.p; A.converged = B.converged.p;
        A.E = eval_scratch(c, B.s_cand.p, B.s_value.p, B.s_simM.p, B.s_status.p);
        int32_t* act[2] = {B.act0.p, B.act1.p};
        HIPCHK(hipMemcpyAsync(B.bestp.p, starts, Ks * np * 8, hipMemcpyHostToDevice, c->stream));
        const size_t cells = Ks * std::max<size_t>(std::max<size_t>(np, nm), (size_t)max_cycles);
        hipLaunchKernelGGL(k_os_init, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, c->stream, P, A, act[0]);
        HIPCHK(hipGetLastError());
        int32_t n_act = K;
        int64_t evaluated = 0;
        for (int cyc = 0; n_act > 0; ++cyc) {
            const int32_t* cur = act[cyc & 1];
            for (int k = 0; k < P.np; ++k)
                for (int a0 = 0; a0 < n_act; a0 += nb_max) {
                    const int nb = std::min(nb_max, n_act - a0);
                    opt_launch_eval(c, A, cur, k, a0, nb, materialise);
                    hipLaunchKernelGGL(k_os_select, dim3((unsigned)((nb + OS_WPB - 1) / OS_WPB)), dim3(64 * OS_WPB), 0, c->stream, P, A, cur, k, a0, nb);
                    HIPCHK(hipGetLastError());
                }
            evaluated += (int64_t)n_act * (int64_t)npoints * (int64_t)P.np;
            hipLaunchKernelGGL(k_os_cycle_end, dim3(1), dim3(COMPACT_WG), 0, c->stream, P, A, cur, (int)n_act, cyc, act[(cyc & 1) ^ 1], B.n_act.p);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(&n_act, B.n_act.p, 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
        }
        if (out) {
            const Download down{c};
            down(out->best, B.bestp.p, Ks * np); down(out->value, B.value.p, Ks); down(out->sim_moments, B.simM.p, Ks * nm);
            down(out->lo, B.lo.p, Ks * np); down(out->hi, B.hi.p, Ks * np); down(out->delta, B.delta.p, Ks);
            down(out->cycle_value, B.cycle_value.p, Ks * (size_t)max_cycles);
            down(out->cycles, B.cycles.p, Ks); down(out->converged, B.converged.p, Ks);
            HIPCHK(hipStreamSynchronize(c->stream));
            out->evaluated = evaluated;
        }
        return SMM_OK;
    });
}

}  // extern "C"
