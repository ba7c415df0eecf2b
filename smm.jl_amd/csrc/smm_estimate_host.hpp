// the host frame of the estimators that evaluate many points off the chains (device side: smm_evalscratch.hpp) — part of libsmmhip (included
// once by smmhip.hip, in front of smm_population_host.hpp; hiprtc never sees it).  What the starting population, smm_opt_slices,
// smm_opt_simplex, smm_opt_lm, smm_abc_pmc and smm_sens_sobol share, each rule once: the prologue (estimate_enter, smm_set_state's too), the starts inside
// the box, the batch a scratch cap allows, a launch's scratch as a view, the compacted list's count read back, the results' way out.  An
// estimator's own file keeps its argument checks, its buffers, its argument block and its loop.
#pragma once

namespace {

// What every estimator does before it looks at its arguments: the iterations enqueued so far settled and finished, and a hard error nobody
// has been TOLD of yet (raised on the device by steps this caller enqueued and never synchronised; the state readers do not raise) reported,
// once; nothing runs then.  smm_set_state enters the same way: it is the recovery from a failure, it must not be the place where one
// disappears — it reports it, once, and uploads nothing; the caller's next smm_set_state goes through
// (tests/test_gpu_error_enumeration.py: every `... step ss` sequence lost its error here)
int estimate_enter(Ctx* c) {
    HIPCHK(hipSetDevice(c->device));
    settle_persist(c);
    HIPCHK(hipStreamSynchronize(c->stream));
    (void)check_device_error(c);
    if (c->failed && !c->failed_told) return told(c);
    return SMM_OK;
}

// starts [np][n], item the fastest index: every coordinate inside the box, or the first that is not named (`noun` `first`, `first` + 1, ..)
int starts_in_box(Ctx* c, const char* fn, const char* noun, int first, const double* starts, size_t n) {
    const KParams& P = c->P;
    const size_t np = P.np;
    std::vector<double> lb(np), ub(np);
    HIPCHK(hipMemcpy(lb.data(), P.lb, np * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ub.data(), P.ub, np * 8, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i)
        for (size_t k = 0; k < np; ++k) {
            const double x = starts[k * n + i];
            if (!(x >= lb[k] && x <= ub[k])) {
                char b[192];
                snprintf(b, sizeof b, "%s: the start of %s %d, parameter %d is %g: outside [%g, %g]", fn, noun, first + (int)i, (int)k + 1, x, lb[k], ub[k]);
                return fail(c, SMM_ERR_INVALID_ARG, b);
            }
        }
    return SMM_OK;
}

// bytes of state and launch scratch a batch of an optimiser's searches or of the sampler's particles may take (the test seam
// SMMHIP_OPT_SCRATCH replaces the cap) ...
constexpr size_t OPT_SCRATCH_CAP = (size_t)64 << 20;
size_t opt_scratch_cap(const Ctx* c) { return c->H.opt_scratch ? c->H.opt_scratch : OPT_SCRATCH_CAP; }
// ... and the items of bytes_each, out of n, that go in one batch under a cap: at least one
int batch_size(size_t cap, size_t n, size_t bytes_each) { return (int)std::min<size_t>(n, std::max<size_t>(1, cap / bytes_each)); }
int batch_size(const Ctx* c, size_t n, size_t bytes_each) { return batch_size(opt_scratch_cap(c), n, bytes_each); }

// one launch's scratch as the kernels see it (EvalScratch: the layouts), and n evaluations of its candidates into it
EvalScratch eval_scratch(const Ctx* c, double* cand, double* value, double* simM, void* status) {
    return EvalScratch{cand, value, simM, status, c->obj == SMM_OBJ_USER ? 1 : 0, c->P.np, c->P.nm};
}
void launch_eval_dev(Ctx* c, const EvalScratch& E, int n) { launch_eval_dev(c, E.cand, n, E.value, E.simM, E.status); }

// the entries of `list` (nullptr: 0 .. n_in - 1) whose flag is set into `to` (k_compact); their number comes back through `count`: the one
// 4-byte read of a phase, which sizes the next launches
int compact_count(Ctx* c, const int32_t* list, int n_in, const int32_t* flag, int32_t* to, int32_t* count) {
    int32_t n_to = 0;
    hipLaunchKernelGGL(k_compact, dim3(1), dim3(COMPACT_WG), 0, c->stream, list, n_in, flag, to, count);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&n_to, count, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return (int)n_to;
}

// results on their way out: n elements of a device array into the caller's, where the caller gave one; onto the context's stream
struct Download {
    Ctx* c;
    template <class T>
    void operator()(T* dst, const T* src, size_t n) const {
        if (dst) HIPCHK(hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyDeviceToHost, c->stream));
    }
};

}  // namespace
