// the host side of smm_sens_sobol (kernels: smm_sobol.hpp; the estimators' frame: smm_estimate_host.hpp) — part of libsmmhip (included once by
// smmhip.hip, behind the sampler's host side; hiprtc never sees it).  The pilot's launch and k_sobol_centre; then per batch of base points
// one evaluation launch over its np + 2 matrices, k_sobol_valid and k_sobol_terms; then k_sobol_count, the two passes of k_sobol_ysum and
// k_sobol_fold for mean and var, and k_sobol_finish.  The host reads nothing per batch: one download at the end.
#pragma once

namespace {

// the device buffers of one call: the resident arrays, and a launch's scratch of n evaluations
struct SobolBufs {
    DevBuf<double> box, yA, centre, bs, ys, mean, var, res, s_cand, s_value, s_simM;
    DevBuf<int32_t> bad, s_status;
    DevBuf<long long> counts;
    SobolBufs(size_t np, size_t nm, size_t N, size_t nblk, size_t n, bool cand)
        : box(2 * np), yA((nm + 1) * N), centre(nm + 1), bs(nblk * SOBOL_SUMS * (nm + 1) * np), ys(nblk * (nm + 1)), mean(nm + 1), var(nm + 1),
          res(6 * (nm + 1) * np), s_cand(cand ? n * np : 1), s_value(n), s_simM(n * nm), bad(N), s_status(n), counts(2) {}
};

// base points [j0, j0 + nb) in their first n / nb matrices evaluated into the launch's scratch
void sobol_launch_eval(Ctx* c, const SobolArgs& A, int j0, int nb, int n, bool materialise) {
    const KParams& P = c->P;
    if (materialise) {
        const size_t work = (size_t)n * (size_t)P.np;
        hipLaunchKernelGGL(k_sobol_candidates, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, c->stream, P, A, j0, nb, n);
        HIPCHK(hipGetLastError());
        launch_eval_dev(c, A.E, n);
        return;
    }
    int8_t* st = (int8_t*)A.E.status;
    void* args[] = {(void*)&P, (void*)&A, (void*)&j0, (void*)&nb, (void*)&n, (void*)&st};
    launch_eval_tiles(c, EF_SOBOL, n, args);
}

}  // namespace

extern "C" {

int smm_sens_sobol(void* ctx, int32_t n_base, const double* lo, const double* hi, smm_sens_sobol_t* out) {
    return api_call(ctx, true, [&](Ctx* c) -> int {
        if (const int rc = estimate_enter(c)) return rc;
        if (n_base < 1 || n_base > (1 << 20)) return fail(c, SMM_ERR_INVALID_ARG, "smm_sens_sobol: n_base must be in [1, 2^20]");
        if ((lo == nullptr) != (hi == nullptr)) return fail(c, SMM_ERR_INVALID_ARG, "smm_sens_sobol: lo and hi are given together or not at all");
        const KParams& P = c->P;
        const size_t np = P.np, nm = P.nm, F = nm + 1, N = (size_t)n_base, NP = F * np;
        std::vector<double> box(2 * np);
        HIPCHK(hipMemcpy(box.data(), P.lb, np * 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(box.data() + np, P.ub, np * 8, hipMemcpyDeviceToHost));
        if (lo) {
            for (size_t k = 0; k < np; ++k)
                if (!(box[k] <= lo[k] && lo[k] <= hi[k] && hi[k] <= box[np + k])) {
                    char b[192];
                    snprintf(b, sizeof b, "smm_sens_sobol: parameter %d: [%g, %g] is not a box inside [%g, %g]", (int)k + 1, lo[k], hi[k], box[k], box[np + k]);
                    return fail(c, SMM_ERR_INVALID_ARG, b);
                }
            std::copy(lo, lo + np, box.begin());
            std::copy(hi, hi + np, box.begin() + np);
        }
        const bool materialise = c->obj == SMM_OBJ_USER || c->H.opt_materialise;   // (a user objective's kernel reads a matrix; the hook: the timing experiment)
        // a launch's scratch: per evaluation its parameters, moments, value and status; a base point is np + 2 evaluations
        const size_t per_eval = (np + nm + 1) * 8 + 4;
        const int nb_max = batch_size(c, N, (np + 2) * per_eval);
        const int n_pilot = (int)std::min<size_t>(N, SOBOL_PILOT);
        const int nblk = (int)((N + SOBOL_TB - 1) / SOBOL_TB);
        SobolBufs B(np, nm, N, (size_t)nblk, std::max((size_t)nb_max * (np + 2), (size_t)n_pilot), materialise);
        const hipStream_t s = c->stream;
        HIPCHK(hipMemcpyAsync(B.box.p, box.data(), 2 * np * 8, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemsetAsync(B.bad.p, 0, N * 4, s));
        HIPCHK(hipMemsetAsync(B.counts.p, 0, 2 * sizeof(long long), s));
        SobolArgs A{};
        A.N = n_base; A.np = (int)np; A.F = (int)F;
        A.lo = B.box.p; A.hi = B.box.p + np;
        A.E = eval_scratch(c, B.s_cand.p, B.s_value.p, B.s_simM.p, B.s_status.p);
        A.yA = B.yA.p; A.bad = B.bad.p; A.centre = B.centre.p; A.bs = B.bs.p; A.ys = B.ys.p; A.mean = B.mean.p; A.var = B.var.p; A.res = B.res.p;
        A.counts = B.counts.p;
        // the pilot: matrix A of the first base points
        sobol_launch_eval(c, A, 0, n_pilot, n_pilot, materialise);
        hipLaunchKernelGGL(k_sobol_centre, dim3(1), dim3(SOBOL_WG), 0, s, A, n_pilot);
        HIPCHK(hipGetLastError());
        const unsigned pair_groups = (unsigned)((NP + SOBOL_PG - 1) / SOBOL_PG);
        for (int j0 = 0; j0 < n_base; j0 += nb_max) {
            const int nb = std::min(nb_max, n_base - j0), n = nb * (int)(np + 2);
            sobol_launch_eval(c, A, j0, nb, n, materialise);
            hipLaunchKernelGGL(k_sobol_valid, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, A, j0, nb, n);
            HIPCHK(hipGetLastError());
            const unsigned blocks = (unsigned)((j0 + nb - 1) / SOBOL_TB - j0 / SOBOL_TB + 1);
            hipLaunchKernelGGL(k_sobol_terms, dim3(blocks, pair_groups), dim3(SOBOL_TB), 0, s, A, j0, nb, n);
            HIPCHK(hipGetLastError());
        }
        hipLaunchKernelGGL(k_sobol_count, dim3(1), dim3(COMPACT_WG), 0, s, A);
        HIPCHK(hipGetLastError());
        for (int mode = 0; mode < 2; ++mode) {
            hipLaunchKernelGGL(k_sobol_ysum, dim3((unsigned)nblk), dim3(SOBOL_TB), 0, s, A, mode);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(k_sobol_fold, dim3(1), dim3(SOBOL_WG), 0, s, A, nblk, mode ? A.var : A.mean);
            HIPCHK(hipGetLastError());
        }
        hipLaunchKernelGGL(k_sobol_finish, dim3((unsigned)((NP + 255) / 256)), dim3(256), 0, s, A, nblk);
        HIPCHK(hipGetLastError());
        long long counts[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(counts, B.counts.p, sizeof counts, hipMemcpyDeviceToHost, s));
        if (out) {
            const Download down{c};
            down(out->mean, (const double*)B.mean.p, F); down(out->var, (const double*)B.var.p, F); down(out->centre, (const double*)B.centre.p, F);
            double* const fields[6] = {out->first, out->total, out->v_first, out->v_total, out->se_first, out->se_total};
            for (int r = 0; r < 6; ++r) down(fields[r], (const double*)B.res.p + (size_t)r * NP, NP);
        }
        HIPCHK(hipStreamSynchronize(s));
        if (out) {
            out->n_complete = (int64_t)counts[0];
            out->n_invalid = (int64_t)counts[1];
            out->evaluated = (int64_t)N * (int64_t)(np + 2) + (int64_t)n_pilot;
        }
        return SMM_OK;
    });
}

}  // extern "C"
