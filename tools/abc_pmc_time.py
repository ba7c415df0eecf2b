"""Population Monte Carlo ABC on the device (smm_abc_pmc) timed at P = 65536 particles, A = 32768 kept, on C4 (banana, np = 10) and C5
(SMM_OBJ_DENSE2, np = nm = 50): one call of `--gens` generations, `--reps` repetitions after a warm call, the median; the time per generation
is the difference to a call of 0 generations (the prior's evaluation and one select) divided by the generations run.  Against it:
  - the same loop on the host — the contract's restatement (tests/pmc_ref.py) over BGPContext.eval_batch, the arithmetic in numpy — whole and
    as the part inside eval_batch alone (`--host-gens`, default 1 generation, one repetition: its weight sums are O(A x P x np) numpy work;
    the results are compared with the device's bit for bit);
  - BGP steps of 4096 chains over the same number of objective evaluations (evaluated / 4096 iterations of a fresh context).
It prints the FP64 instructions of the weight kernel (k_pmc_kernel) as the contract counts them — per (new particle with a finite distance,
kept particle): np subtractions, np products, np - 1 additions, the product by -0.5, smm_exp's 21, the product by wn and the addition to
the block sum = 3 np + 24.  The kernel's own time is not visible to a host timer: --device-only runs the device calls alone, the run to put
under a kernel trace for the time per kernel, and --kernel-ms-c4 / --kernel-ms-c5 take k_pmc_kernel's time PER CALL from such a trace (its
total over the run divided by the calls of `--gens` generations: 1 + reps under --device-only) and print the achieved FP64 rate against
the FP64-add roof of BENCH_r06.json (39.3216e12 / s).  Without them only the count and its time at the roof are printed.
  python tools/abc_pmc_time.py [c4|c5 ...] [--reps 3] [--gens 3] [--scale-c4 0.25] [--scale-c5 0.02] [--host-gens 1] [--no-host] [--device-only]
                               [--kernel-ms-c4 MS] [--kernel-ms-c5 MS]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import smm_jl_amd as S   # noqa: E402
from smm_jl_amd.workloads import build_problem   # noqa: E402
from oracle import oracle as O   # noqa: E402
import pmc_ref as R   # noqa: E402

P, A, N_BGP = 65536, 32768, 4096
RIDGE = 1e-6
ADD_ROOF = 39.3216e12


def arg(name, default, kind):
    return kind(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def kernel_instructions(r, np_):
    """FP64 instructions of k_pmc_kernel over the call, by the contract's count"""
    total = 0
    for g in range(1, r["generations"] + 1):
        kept = int(r["n_new_kept"][0]) if g == 1 else int(r["n_kept"])      # (A' of the generation before: A wherever A particles are finite)
        n_w = (P - kept) - int(r["n_outside"][g]) - int(r["n_invalid"][g])
        total += n_w * kept * (3 * np_ + 24)
    return total


def main():
    shapes = [a for a in sys.argv[1:] if a in ("c4", "c5")] or ["c4", "c5"]
    reps, gens, host_gens = arg("--reps", 3, int), arg("--gens", 3, int), arg("--host-gens", 1, int)
    scale = {"c4": arg("--scale-c4", 0.25, float), "c5": arg("--scale-c5", 0.02, float)}
    device_only, no_host = "--device-only" in sys.argv, "--no-host" in sys.argv
    for w in shapes:
        prob, opts = build_problem(w, N_BGP, N_BGP, 0, 64, 0)
        h = S.hip_context(prob, opts)
        sc = scale[w]
        call = lambda G: h.abc_pmc(P, A, G, 0.0, sc, RIDGE, (0.5,))   # noqa: E731
        call(gens)      # warm: the first launches of every kernel and shape
        t_g, t_0 = [], []
        for _ in range(reps):
            t = time.perf_counter(); r = call(gens); t_g.append(time.perf_counter() - t)
            t = time.perf_counter(); call(0); t_0.append(time.perf_counter() - t)
        d, d0 = np.median(t_g), np.median(t_0)
        ms = lambda x: ", ".join("%.1f" % (y * 1e3) for y in x)   # noqa: E731
        G = max(1, r["generations"])
        print("%s: P = %d, A = %d, np %d, nm %d, scale %g, ridge %g; %d repetitions, medians, host perf_counter around synchronised calls"
              % (w, P, A, prob.np, prob.nm, sc, RIDGE, reps))
        print("  device (smm_abc_pmc): %d generations %.1f ms (%s); generation 0 alone %.1f ms (%s); %.2f ms per generation; status %d, evaluated %d "
              "= %.1f ns per evaluation; eps %s; p_acc %s; outside %s; ess %.0f"
              % (r["generations"], d * 1e3, ms(t_g), d0 * 1e3, ms(t_0), (d - d0) * 1e3 / G, r["status"], r["evaluated"], d * 1e9 / r["evaluated"],
                 ["%.4g" % x for x in r["eps"]], ["%.3f" % x for x in r["p_acc"]], list(r["n_outside"]), r["ess"]))
        ki = kernel_instructions(r, prob.np)
        print("  k_pmc_kernel: %.4g FP64 instructions per call (3 np + 24 per pair); at the add roof of %.4g / s that is %.2f ms" % (ki, ADD_ROOF, ki / ADD_ROOF * 1e3))
        kms = arg("--kernel-ms-" + w, None, float)
        if kms is not None:
            print("  k_pmc_kernel: %.3f ms per call in the trace = %.4g FP64 instructions / s = %.2f of the add roof" % (kms, ki / (kms * 1e-3), ki / (kms * 1e-3) / ADD_ROOF))
        if device_only:
            h.close()
            continue
        if not no_host:
            in_eval = [0.0]

            def evaluator(Pm):
                t = time.perf_counter()
                out = h.eval_batch(Pm)
                in_eval[0] += time.perf_counter() - t
                return out
            t = time.perf_counter()
            rh = R.abc_pmc(O, evaluator, int(opts.seed), prob.lb, prob.ub, prob.nm, P, A, host_gens, 0.0, sc, RIDGE, (0.5,))
            th = time.perf_counter() - t
            t = time.perf_counter(); rd = call(host_gens); td = time.perf_counter() - t
            R.assert_equal(rd, rh)
            print("  host loop over eval_batch, %d generation(s), once: %.1f s, of which inside eval_batch %.1f ms; the device call of the same: %.1f ms; "
                  "host loop / device = %.0f, eval_batch alone / device = %.2f; results equal bit for bit"
                  % (host_gens, th, in_eval[0] * 1e3, td * 1e3, th / td, in_eval[0] / td))
        iters = max(2, int(round(r["evaluated"] / N_BGP)))
        t_b = []
        for _ in range(reps):
            b = S.hip_context(*build_problem(w, N_BGP, N_BGP, 0, iters, 0))
            t = time.perf_counter(); b.step(iters); b.state(); t_b.append(time.perf_counter() - t)
            b.close()
        tb = np.median(t_b)
        print("  BGP, %d chains x %d iterations = %d evaluations: %.1f ms (%s) = %.1f ns per evaluation; BGP / smm_abc_pmc = %.2f"
              % (N_BGP, iters, N_BGP * iters, tb * 1e3, ms(t_b), tb * 1e9 / (N_BGP * iters), tb / d), flush=True)
        h.close()


if __name__ == "__main__":
    main()
