// the host side of smm_abc_pmc (kernels: smm_pmc.hpp; the estimators' frame: smm_estimate_host.hpp) — part of libsmmhip (included once by
// smmhip.hip, behind the optimisers' host sides; hiprtc never sees it).  One generation g >= 1: k_pmc_whiten of the kept -> k_pmc_propose ->
// the inside particles compacted (the first read: their number) -> their evaluation in batches under the cap (k_pmc_gather, launch_eval_dev,
// k_pmc_scatter) -> the particles with a finite distance compacted -> k_pmc_whiten of the new -> k_pmc_kernel and k_pmc_combine, a pass of
// PMC_PASS blocks of T at a time -> k_pmc_logw -> k_pmc_select -> k_pmc_move -> k_pmc_weights -> k_pmc_mean, k_pmc_pairs, k_pmc_chol for the next
// generation (the second read: A' and whether the run goes on).  Generation 0 is k_pmc_generate, the evaluation of all P and the same tail.
// Nothing else of the particles visits the host before the results are copied out.
#pragma once

namespace {

// the particles of one call: two kept sets of A rows (the select moves from one to the other), the new particles of a generation (P rows),
// the candidates' distances — the kept in front, the new behind them, so that the select reads one column — and a launch's scratch
struct PmcBufs {
    DevBuf<double> ku0, ku1, kth0, kth1, kmom0, kmom1, klw0, klw1, crho0, crho1, kz, kzT, kwn;
    DevBuf<int32_t> kborn0, kborn1;
    DevBuf<long long> kq, kpre;
    DevBuf<double> nu, nth, nmom, nlw, nz, D, part;
    DevBuf<int32_t> inside_flag, flagw, inside, wlist, src;
    DevBuf<double> s_cand, s_value, s_simM;
    DevBuf<int32_t> s_status;
    DevBuf<double> L, C, mean, g_eps, g_pacc, g_ess, probs, quant;
    DevBuf<int32_t> g_ninv, g_nund, g_nnk;
    DevBuf<PmcCtl> ctl;
    PmcBufs(const KParams& K, size_t P, size_t A, size_t nb, size_t G1, size_t nq)
        : ku0(A * K.np), ku1(A * K.np), kth0(A * K.np), kth1(A * K.np), kmom0(A * K.nm), kmom1(A * K.nm), klw0(A), klw1(A), crho0(P), crho1(P),
          kz(A * K.np), kzT(A * MAX_DIM), kwn(A), kborn0(A), kborn1(A), kq(A), kpre(A),
          nu(P * K.np), nth(P * K.np), nmom(P * K.nm), nlw(P), nz(P * K.np), D(P), part((size_t)PMC_PASS * P),
          inside_flag(P), flagw(P), inside(P), wlist(P), src(A),
          s_cand(nb * K.np), s_value(nb), s_simM(nb * K.nm), s_status(nb),
          L((size_t)K.np * K.np), C((size_t)K.np * K.np), mean(K.np), g_eps(G1), g_pacc(G1), g_ess(G1), probs(nq), quant(nq * K.np),
          g_ninv(G1), g_nund(G1), g_nnk(G1), ctl(1) {}
};

template <int NPC>
void pmc_launch_kernel(Ctx* c, dim3 grid, const PmcCtl* ctl, int np, int b0, const int32_t* wlist, const double* nz, size_t stride, const double* kzT,
                       const double* wn, double* part, size_t pstride) {
    hipLaunchKernelGGL((k_pmc_kernel<NPC>), grid, dim3(PMC_WG), 0, c->stream, ctl, np, b0, wlist, nz, stride, kzT, wn, part, pstride);
    HIPCHK(hipGetLastError());
}

// k_pmc_kernel<NPC> for NPC = 4, 8, .. 64: entry NPC / 4 - 1
using PmcLaunch = void (*)(Ctx*, dim3, const PmcCtl*, int, int, const int32_t*, const double*, size_t, const double*, const double*, double*, size_t);
const PmcLaunch pmc_kernels[MAX_DIM / 4] = {pmc_launch_kernel<4>,  pmc_launch_kernel<8>,  pmc_launch_kernel<12>, pmc_launch_kernel<16>,
                                            pmc_launch_kernel<20>, pmc_launch_kernel<24>, pmc_launch_kernel<28>, pmc_launch_kernel<32>,
                                            pmc_launch_kernel<36>, pmc_launch_kernel<40>, pmc_launch_kernel<44>, pmc_launch_kernel<48>,
                                            pmc_launch_kernel<52>, pmc_launch_kernel<56>, pmc_launch_kernel<60>, pmc_launch_kernel<64>};
static_assert(MAX_DIM == 64, "pmc_kernels names every NPC up to MAX_DIM; k_pmc_chol takes a lane per row");

}  // namespace

extern "C" {

int smm_abc_pmc(void* ctx, int32_t n_particles, int32_t n_keep, int32_t max_gen, double p_acc_min, double scale, double ridge, const double* probs,
                int32_t n_probs, smm_abc_pmc_t* out) {
    return api_call(ctx, true, [&](Ctx* c) -> int {
        if (const int rc = estimate_enter(c)) return rc;
        if (n_particles > (1 << 22)) return fail(c, SMM_ERR_INVALID_ARG, "smm_abc_pmc: n_particles must not exceed 2^22");
        if (n_keep < 2 || n_keep >= n_particles) return fail(c, SMM_ERR_INVALID_ARG, "smm_abc_pmc: n_keep must be in [2, n_particles)");
        if (max_gen < 0) return fail(c, SMM_ERR_INVALID_ARG, "smm_abc_pmc: max_gen < 0");
        if (!(p_acc_min >= 0.0 && p_acc_min < 1.0)) return fail(c, SMM_ERR_INVALID_ARG, "smm_abc_pmc: p_acc_min must be in [0, 1)");
        if (!(scale > 0.0)) return fail(c, SMM_ERR_INVALID_ARG, "smm_abc_pmc: scale must be > 0");
        if (!(ridge >= 0.0 && ridge <= 1.7976931348623157e308)) return fail(c, SMM_ERR_INVALID_ARG, "smm_abc_pmc: ridge must be finite and >= 0");
        if (n_probs < 0 || (n_probs > 0 && !probs)) return fail(c, SMM_ERR_INVALID_ARG, "smm_abc_pmc: probs is NULL or n_probs < 0");
        for (int r = 0; r < n_probs; ++r)
            if (!(probs[r] >= 0.0 && probs[r] <= 1.0)) return fail(c, SMM_ERR_INVALID_ARG, "smm_abc_pmc: a prob outside [0, 1]");
        const KParams& K = c->P;
        const int np = K.np, nm = K.nm, P = n_particles, A = n_keep;
        const size_t Ps = (size_t)P, As = (size_t)A, G1 = (size_t)max_gen + 1, nq = (size_t)n_probs;
        // a launch's scratch: per evaluation its parameters, moments, value and status
        const size_t per_eval = (size_t)(np + nm + 1) * 8 + 4;
        const int nb_max = batch_size(c, Ps, per_eval);
        PmcBufs B(K, Ps, As, (size_t)nb_max, G1, nq);
        const EvalScratch E = eval_scratch(c, B.s_cand.p, B.s_value.p, B.s_simM.p, B.s_status.p);
        HIPCHK(hipFuncSetAttribute((const void*)k_pmc_mean, hipFuncAttributeMaxDynamicSharedMemorySize, STATS_LDS_N * 8));
        HIPCHK(hipFuncSetAttribute((const void*)k_pmc_pairs, hipFuncAttributeMaxDynamicSharedMemorySize, STATS_LDS_N * 8));
        const hipStream_t s = c->stream;
        // generations that never run report NaN and -1
        std::vector<double> gd(G1, std::numeric_limits<double>::quiet_NaN());
        std::vector<int32_t> gi(G1, -1), n_outside(G1, -1);
        for (double* p : {B.g_eps.p, B.g_pacc.p, B.g_ess.p}) HIPCHK(hipMemcpyAsync(p, gd.data(), G1 * 8, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(B.g_nnk.p, gi.data(), G1 * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemsetAsync(B.g_ninv.p, 0, G1 * 4, s));
        HIPCHK(hipMemsetAsync(B.g_nund.p, 0, G1 * 4, s));
        PmcCtl h_ctl{};
        h_ctl.stop = -1;
        h_ctl.eps = h_ctl.ess = h_ctl.logc = std::numeric_limits<double>::quiet_NaN();
        HIPCHK(hipMemcpyAsync(B.ctl.p, &h_ctl, sizeof h_ctl, hipMemcpyHostToDevice, s));
        if (nq) HIPCHK(hipMemcpyAsync(B.probs.p, probs, nq * 8, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemsetAsync(B.nlw.p, 0, Ps * 8, s));   // (generation 0: lw = 0.0)
        PmcCtl* ctl = B.ctl.p;
        const PmcGen G{B.g_eps.p, B.g_pacc.p, B.g_ess.p, B.g_ninv.p, B.g_nund.p, B.g_nnk.p};
        PmcSet kept[2] = {{B.ku0.p, B.kth0.p, B.kmom0.p, B.crho0.p, B.klw0.p, B.kborn0.p}, {B.ku1.p, B.kth1.p, B.kmom1.p, B.crho1.p, B.klw1.p, B.kborn1.p}};
        const int npc = (np + 3) / 4 * 4;   // k_pmc_kernel's NPC: the row length of kzT
        int cur = 0, nk = 0, stop = -1, g = 0;
        int64_t evaluated = 0;
        auto blocks = [](size_t n, size_t wg) { return dim3((unsigned)((n + wg - 1) / wg)); };
        // the n listed new particles (nullptr: all of them) evaluated in batches under the cap; their distances behind the kept ones'
        auto evaluate = [&](const int32_t* list, int n, double* nrho) {
            for (int off = 0; off < n; off += nb_max) {
                const int nb = std::min(nb_max, n - off);
                hipLaunchKernelGGL(k_pmc_gather, blocks((size_t)nb * np, 256), dim3(256), 0, s, E, list, off, nb, (const double*)B.nth.p, Ps);
                HIPCHK(hipGetLastError());
                launch_eval_dev(c, E, nb);
                hipLaunchKernelGGL(k_pmc_scatter, blocks((size_t)nb, 256), dim3(256), 0, s, E, list, off, nb, nrho, B.nmom.p, Ps, B.flagw.p, B.g_ninv.p + g);
                HIPCHK(hipGetLastError());
            }
            evaluated += (int64_t)n;
        };
        // what follows every generation's evaluation: the select over the candidates, the kept rows moved, their sampling weights, and the next
        // generation's kernel covariance and factor; then the second read of the generation
        auto select_and_prepare = [&](int n_new) {
            const PmcSet fresh{B.nu.p, B.nth.p, B.nmom.p, kept[cur].rho + nk, B.nlw.p, nullptr};
            hipLaunchKernelGGL(k_pmc_select, dim3(1), dim3(STATS_WG), 0, s, ctl, G, g, (int)max_gen, p_acc_min, A, nk + n_new, nk, (const double*)kept[cur].rho, B.src.p);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(k_pmc_move, dim3((unsigned)((A + 255) / 256), (unsigned)(2 * np + nm + 1)), dim3(256), 0, s, (const PmcCtl*)ctl, np, nm, g, nk,
                               (const int32_t*)B.src.p, kept[cur], As, fresh, Ps, kept[cur ^ 1]);
            HIPCHK(hipGetLastError());
            cur ^= 1;
            hipLaunchKernelGGL(k_pmc_weights, dim3(1), dim3(PMC_W_WG), 0, s, ctl, (const double*)kept[cur].lw, B.kq.p, B.kpre.p, B.kwn.p, B.g_ess.p + g);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(k_pmc_mean, dim3((unsigned)np), dim3(STATS_WG), (size_t)STATS_LDS_N * 8, s, (const PmcCtl*)ctl, 0, (const double*)B.kwn.p,
                               (const double*)kept[cur].u, As, B.mean.p);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(k_pmc_pairs, dim3((unsigned)(np * (np + 1) / 2)), dim3(STATS_WG), (size_t)STATS_LDS_N * 8, s, (const PmcCtl*)ctl, 0, np,
                               (const double*)B.kwn.p, (const double*)kept[cur].u, As, (const double*)B.mean.p, B.C.p);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(k_pmc_chol, dim3(1), dim3(64), 0, s, ctl, np, scale, ridge, (const double*)B.C.p, B.L.p);
            HIPCHK(hipGetLastError());
            int32_t two[2];
            HIPCHK(hipMemcpyAsync(two, ctl, 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            stop = two[0]; nk = two[1];
        };
        hipLaunchKernelGGL(k_pmc_generate, blocks(Ps * (size_t)((np + 1) / 2), 256), dim3(256), 0, s, K, P, Ps, B.nu.p, B.nth.p);
        HIPCHK(hipGetLastError());
        n_outside[0] = 0;
        evaluate(nullptr, P, kept[cur].rho);
        select_and_prepare(P);
        while (stop < 0) {
            ++g;
            const int n_new = P - nk;
            double* nrho = kept[cur].rho + nk;
            hipLaunchKernelGGL(k_pmc_whiten, blocks((size_t)nk, 256), dim3(256), 0, s, nk, np, (const double*)B.L.p, (const double*)kept[cur].u, B.kz.p, As, B.kzT.p, npc);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(k_pmc_propose, blocks((size_t)n_new, 64), dim3(64), 0, s, K, (const PmcCtl*)ctl, g, n_new, (const double*)B.L.p, (const long long*)B.kpre.p,
                               (const double*)kept[cur].u, As, B.nu.p, B.nth.p, nrho, B.nlw.p, Ps, B.inside_flag.p, B.flagw.p);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(k_compact, dim3(1), dim3(COMPACT_WG), 0, s, (const int32_t*)nullptr, n_new, (const int32_t*)B.inside_flag.p, B.inside.p, &ctl->n_inside);
            HIPCHK(hipGetLastError());
            int32_t n_inside = 0;
            HIPCHK(hipMemcpyAsync(&n_inside, &ctl->n_inside, 4, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            n_outside[g] = n_new - n_inside;
            if (n_inside > 0) {
                evaluate(B.inside.p, n_inside, nrho);
                hipLaunchKernelGGL(k_compact, dim3(1), dim3(COMPACT_WG), 0, s, (const int32_t*)nullptr, n_new, (const int32_t*)B.flagw.p, B.wlist.p, &ctl->n_w);
                HIPCHK(hipGetLastError());
                hipLaunchKernelGGL(k_pmc_whiten, blocks((size_t)n_new, 256), dim3(256), 0, s, n_new, np, (const double*)B.L.p, (const double*)B.nu.p, B.nz.p, Ps, (double*)nullptr, 0);
                HIPCHK(hipGetLastError());
                // the lanes are sized by the inside particles, an upper bound of the list the device holds
                const int nblk = (nk + PMC_TB - 1) / PMC_TB;
                const unsigned gx = (unsigned)((n_inside + PMC_WG - 1) / PMC_WG);
                for (int b0 = 0; b0 < nblk; b0 += PMC_PASS) {
                    const int nbk = std::min(PMC_PASS, nblk - b0);
                    const dim3 grid(gx, (unsigned)nbk);
                    const PmcCtl* cc = ctl;
                    const int32_t* wl = B.wlist.p;
                    const double *nz = B.nz.p, *kz = B.kzT.p, *wn = B.kwn.p;
                    pmc_kernels[npc / 4 - 1](c, grid, cc, np, b0, wl, nz, Ps, kz, wn, B.part.p, Ps);
                    hipLaunchKernelGGL(k_pmc_combine, blocks((size_t)n_inside, 256), dim3(256), 0, s, cc, b0 == 0 ? 1 : 0, nbk, (const double*)B.part.p, Ps, B.D.p);
                    HIPCHK(hipGetLastError());
                }
                hipLaunchKernelGGL(k_pmc_logw, blocks((size_t)n_inside, 256), dim3(256), 0, s, ctl, (const int32_t*)B.wlist.p, (const double*)B.D.p, nrho, B.nlw.p, B.g_nund.p + g);
                HIPCHK(hipGetLastError());
            }
            select_and_prepare(n_new);
        }
        // the summary of the final kept set, in parameter space
        const PmcSet& fin = kept[cur];
        hipLaunchKernelGGL(k_pmc_mean, dim3((unsigned)np), dim3(STATS_WG), (size_t)STATS_LDS_N * 8, s, (const PmcCtl*)ctl, 1, (const double*)B.kwn.p, (const double*)fin.th, As, B.mean.p);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_pmc_pairs, dim3((unsigned)(np * (np + 1) / 2)), dim3(STATS_WG), (size_t)STATS_LDS_N * 8, s, (const PmcCtl*)ctl, 1, np, (const double*)B.kwn.p,
                           (const double*)fin.th, As, (const double*)B.mean.p, B.C.p);
        HIPCHK(hipGetLastError());
        if (nq) {
            hipLaunchKernelGGL(k_pmc_quantile, dim3((unsigned)np, (unsigned)nq), dim3(STATS_WG), 0, s, (const PmcCtl*)ctl, np, (const double*)B.probs.p, (const double*)fin.th, As,
                               (const long long*)B.kq.p, B.quant.p);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipMemcpyAsync(&h_ctl, ctl, sizeof h_ctl, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (out) {
            const Download down{c};
            down(out->theta, fin.th, As * np); down(out->value, fin.rho, As); down(out->sim_moments, fin.mom, As * nm);
            down(out->weight, B.kwn.p, As); down(out->logw, fin.lw, As); down(out->born, fin.born, As);
            down(out->eps, B.g_eps.p, G1); down(out->p_acc, B.g_pacc.p, G1); down(out->gen_ess, B.g_ess.p, G1);
            down(out->n_invalid, B.g_ninv.p, G1); down(out->n_underflow, B.g_nund.p, G1); down(out->n_new_kept, B.g_nnk.p, G1);
            down(out->mean, B.mean.p, (size_t)np); down(out->cov, B.C.p, (size_t)np * np); down(out->quantile, B.quant.p, nq * np);
            HIPCHK(hipStreamSynchronize(s));
            // rows past n_kept, and the counts of generations that never ran
            const double nan = std::numeric_limits<double>::quiet_NaN();
            const size_t nks = (size_t)nk;
            for (size_t i = nks; i < As; ++i) {
                if (out->theta) for (int k = 0; k < np; ++k) out->theta[(size_t)k * As + i] = nan;
                if (out->sim_moments) for (int m = 0; m < nm; ++m) out->sim_moments[(size_t)m * As + i] = nan;
                if (out->value) out->value[i] = nan;
                if (out->weight) out->weight[i] = nan;
                if (out->logw) out->logw[i] = nan;
                if (out->born) out->born[i] = -1;
            }
            for (size_t t = (size_t)g + 1; t < G1; ++t) {
                if (out->n_invalid) out->n_invalid[t] = -1;
                if (out->n_underflow) out->n_underflow[t] = -1;
            }
            if (out->n_outside) std::copy(n_outside.begin(), n_outside.end(), out->n_outside);
            out->ess = h_ctl.ess;
            out->n_kept = nk;
            out->generations = g;
            out->status = stop;
            out->evaluated = evaluated;
        }
        return SMM_OK;
    });
}

}  // extern "C"
