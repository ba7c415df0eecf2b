// the host side of smm_opt_slices (kernels: smm_optslices.hpp) — part of libsmmhip (included once by smmhip.hip, behind the starting
// population's host side; hiprtc never sees it).  The loop: per cycle and parameter one evaluation launch over the running searches' grid
// points and k_os_select, per cycle k_os_cycle_end and ONE 4-byte read-back — the number of searches that go on — which sizes the next
// cycle's launches and ends the loop.  Nothing else of the searches' state visits the host before the results are copied out.
#pragma once

namespace {

// bytes of step scratch a batch of running searches may take (the test seam SMMHIP_OPT_SCRATCH replaces the cap)
constexpr size_t OPT_SCRATCH_CAP = (size_t)64 << 20;
size_t opt_scratch_cap(const Ctx* c) { return c->H.opt_scratch ? c->H.opt_scratch : OPT_SCRATCH_CAP; }

// the built-in objectives' slice evaluation: the instances k_eval_batch has (launch_eval_dev), and the tile each takes
struct SliceKernel { const void* fn; int ct; };
SliceKernel slice_kernel(const Ctx* c) {
    if (is_sim(c->obj)) return {(const void*)k_eval_slice<1, 8>, 8};
    if (c->obj == SMM_OBJ_DENSE) return {(const void*)k_eval_slice<2, 16>, 16};
    return {(const void*)k_eval_slice<0, 8>, 8};
}
// (lds_limits: their dynamic LDS beyond the default, next to k_eval_batch's)
void slice_lds_limits() {
    for (const void* fn : {(const void*)k_eval_slice<1, 8>, (const void*)k_eval_slice<2, 16>, (const void*)k_eval_slice<0, 8>})
        HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_CU));
}

// the device buffers of one call
struct OptBufs {
    DevBuf<double> bestp, lo, hi, dvec, value, simM, delta, cycle_value, s_cand, s_value, s_simM;
    DevBuf<int32_t> cycles, converged, act0, act1, n_act, s_status;
    OptBufs(const KParams& P, size_t K, size_t max_cycles, size_t n, bool cand)
        : bestp(K * P.np), lo(K * P.np), hi(K * P.np), dvec(K * P.np), value(K), simM(K * P.nm), delta(K), cycle_value(K * max_cycles),
          s_cand(cand ? n * P.np : 1), s_value(n), s_simM(n * P.nm), cycles(K), converged(K), act0(K), act1(K), n_act(1), s_status(n) {}
};

// coordinate k of the running searches [a0, a0 + nb) of `act`: their n = nb x G grid points evaluated into the step scratch
void opt_launch_eval(Ctx* c, const OsArgs& A, const int32_t* act, int k, int a0, int nb, void* status, bool materialise) {
    const KParams& P = c->P;
    const int n = nb * A.G;
    if (materialise) {
        const size_t work = (size_t)n * (size_t)P.np;
        hipLaunchKernelGGL(k_os_candidates, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, c->stream, P, A, act, k, a0, n);
        HIPCHK(hipGetLastError());
        launch_eval_dev(c, A.s_cand, n, A.s_value, A.s_simM, status);
        return;
    }
    const SliceKernel S = slice_kernel(c);
    int8_t* st = (int8_t*)status;
    void* args[] = {(void*)&P, (void*)&A, (void*)&act, (void*)&k, (void*)&a0, (void*)&n, (void*)&st};
    HIPCHK(hipLaunchKernel(S.fn, dim3((unsigned)((n + S.ct - 1) / S.ct)), dim3(WG), args, tile_smem_base(c, S.ct), c->stream));
}

}  // namespace

extern "C" {

int smm_opt_slices(void* ctx, const double* starts, int32_t K, int32_t npoints, double tol, double update, int32_t max_cycles, smm_opt_slices_t* out) {
    return api_call(ctx, true, [&](Ctx* c) -> int {
        // settled and finished, and a hard error nobody has been told of reported once, as the starting population does (nothing runs then)
        HIPCHK(hipSetDevice(c->device));
        settle_persist(c);
        HIPCHK(hipStreamSynchronize(c->stream));
        (void)check_device_error(c);
        if (c->failed && !c->failed_told) { c->failed_told = true; return c->failed; }
        if (!starts) return fail(c, SMM_ERR_INVALID_ARG, "smm_opt_slices: starts is NULL");
        if (K < 1) return fail(c, SMM_ERR_INVALID_ARG, "smm_opt_slices: K < 1");
        if (npoints < 2) return fail(c, SMM_ERR_INVALID_ARG, "smm_opt_slices: npoints < 2");
        if ((int64_t)K * (int64_t)npoints >= ((int64_t)1 << 31)) return fail(c, SMM_ERR_INVALID_ARG, "smm_opt_slices: K x npoints must stay below 2^31");
        if (!(tol >= 0.0)) return fail(c, SMM_ERR_INVALID_ARG, "smm_opt_slices: tol must be >= 0");
        if (update == update && !(update > 0.0)) return fail(c, SMM_ERR_INVALID_ARG, "smm_opt_slices: update must be > 0 (NaN: the ranges never shrink)");
        if (max_cycles < 1) return fail(c, SMM_ERR_INVALID_ARG, "smm_opt_slices: max_cycles < 1");
        const KParams& P = c->P;
        const size_t Ks = (size_t)K, np = P.np, nm = P.nm, G = (size_t)npoints;
        std::vector<double> lb(np), ub(np);
        HIPCHK(hipMemcpy(lb.data(), P.lb, np * 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(ub.data(), P.ub, np * 8, hipMemcpyDeviceToHost));
        for (size_t s = 0; s < Ks; ++s)
            for (size_t k = 0; k < np; ++k) {
                const double x = starts[k * Ks + s];
                if (!(x >= lb[k] && x <= ub[k])) {
                    char b[192];
                    snprintf(b, sizeof b, "smm_opt_slices: the start of search %d, parameter %d is %g: outside [%g, %g]", (int)s + 1, (int)k + 1, x, lb[k], ub[k]);
                    return fail(c, SMM_ERR_INVALID_ARG, b);
                }
            }
        const bool user = c->obj == SMM_OBJ_USER;
        const bool materialise = user || c->H.opt_materialise;   // (a user objective's kernel reads a matrix; the hook: the timing experiment)
        // a step's values, moments and status (and candidates, where they are materialised) per search; the running searches go in batches
        const size_t per_search = G * ((nm + 1) * 8 + 4 + (materialise ? np * 8 : 0));
        const int nb_max = (int)std::min<size_t>(Ks, std::max<size_t>(1, opt_scratch_cap(c) / per_search));
        OptBufs B(P, Ks, (size_t)max_cycles, (size_t)nb_max * G, materialise);
        OsArgs A{};
        A.K = K; A.G = npoints; A.user = user ? 1 : 0; A.max_cycles = max_cycles; A.tol = tol; A.update = update;
        A.bestp = B.bestp.p; A.lo = B.lo.p; A.hi = B.hi.p; A.dvec = B.dvec.p; A.value = B.value.p; A.simM = B.simM.p; A.delta = B.delta.p;
        A.cycle_value = B.cycle_value.p; A.cycles = B.cycles.p; A.converged = B.converged.p;
        A.s_cand = B.s_cand.p; A.s_value = B.s_value.p; A.s_simM = B.s_simM.p;
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
                    opt_launch_eval(c, A, cur, k, a0, nb, B.s_status.p, materialise);
                    hipLaunchKernelGGL(k_os_select, dim3((unsigned)((nb + OS_WPB - 1) / OS_WPB)), dim3(64 * OS_WPB), 0, c->stream, P, A, cur, k, a0, nb);
                    HIPCHK(hipGetLastError());
                }
            evaluated += (int64_t)n_act * (int64_t)npoints * (int64_t)P.np;
            hipLaunchKernelGGL(k_os_cycle_end, dim3(1), dim3(OS_CE_WG), 0, c->stream, P, A, cur, (int)n_act, cyc, act[(cyc & 1) ^ 1], B.n_act.p);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(&n_act, B.n_act.p, 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
        }
        if (out) {
            auto down = [&](void* dst, const void* src, size_t bytes) { if (dst) HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream)); };
            down(out->best, B.bestp.p, Ks * np * 8); down(out->value, B.value.p, Ks * 8); down(out->sim_moments, B.simM.p, Ks * nm * 8);
            down(out->lo, B.lo.p, Ks * np * 8); down(out->hi, B.hi.p, Ks * np * 8); down(out->delta, B.delta.p, Ks * 8);
            down(out->cycle_value, B.cycle_value.p, Ks * (size_t)max_cycles * 8);
            down(out->cycles, B.cycles.p, Ks * 4); down(out->converged, B.converged.p, Ks * 4);
            HIPCHK(hipStreamSynchronize(c->stream));
            out->evaluated = evaluated;
        }
        return SMM_OK;
    });
}

}  // extern "C"
