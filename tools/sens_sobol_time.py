"""Global sensitivity on the device (smm_sens_sobol) timed at N = 65536 base points on C4 (banana, np = 10: 786432 + 256 evaluations) and C5
(SMM_OBJ_DENSE2, np = nm = 50: 3407872 + 256 evaluations): one call, `--reps` repetitions after a warm call, the median.  Against it the same
loop on the host — the contract's restatement (tests/sobol_ref.py) over BGPContext.eval_batch in the device's batches, the points built and
the terms summed in numpy — at `--host-n` base points (default 2048: the restatement keeps every output of every matrix), whole and as the
part inside eval_batch alone, once; the device call of the same size is timed next to it and the results are compared bit for bit.
The kernels' own times are not visible to a host timer: --device-only runs the device calls alone, the run to put under a kernel trace for
the time per kernel (k_eval_sobol, k_sobol_valid, k_sobol_terms, the finishing kernels); the term kernel's share is its time next to the
evaluation kernel's in such a trace.
  python tools/sens_sobol_time.py [c4|c5 ...] [--reps 3] [--n 65536] [--host-n 2048] [--no-host] [--device-only]"""
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
import sobol_ref as R   # noqa: E402

N_BGP = 4096
CAP = 64 << 20


def arg(name, default, kind):
    return kind(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    shapes = [a for a in sys.argv[1:] if a in ("c4", "c5")] or ["c4", "c5"]
    reps, N, host_n = arg("--reps", 3, int), arg("--n", 65536, int), arg("--host-n", 2048, int)
    device_only, no_host = "--device-only" in sys.argv, "--no-host" in sys.argv
    ms = lambda x: ", ".join("%.1f" % (y * 1e3) for y in x)   # noqa: E731
    for w in shapes:
        prob, opts = build_problem(w, N_BGP, N_BGP, 0, 64, 0)
        h = S.hip_context(prob, opts)
        nb = max(1, min(N, CAP // ((prob.np + 2) * ((prob.np + prob.nm + 1) * 8 + 4))))
        h.sens_sobol(N)      # warm: the first launches of every kernel and shape
        t_d = []
        for _ in range(reps):
            t = time.perf_counter(); r = h.sens_sobol(N); t_d.append(time.perf_counter() - t)
        d = np.median(t_d)
        pairs = (prob.nm + 1) * prob.np
        print("%s: N = %d, np %d, nm %d: %d evaluations in batches of %d base points, %d pairs (i, f); %d repetitions, medians, host perf_counter "
              "around synchronised calls" % (w, N, prob.np, prob.nm, r["evaluated"], nb, pairs, reps))
        print("  device (smm_sens_sobol): %.1f ms (%s) = %.1f ns per evaluation; n_complete %d, n_invalid %d; the value's largest total index %.3f, "
              "largest interaction %.3f" % (d * 1e3, ms(t_d), d * 1e9 / r["evaluated"], r["n_complete"], r["n_invalid"], np.nanmax(r["total"][0]),
                                            np.nanmax(r["total"][0] - r["first"][0])), flush=True)
        if device_only or no_host:
            h.close()
            continue
        in_eval = [0.0]

        def evaluator(Pm):
            t = time.perf_counter()
            out = h.eval_batch(Pm)
            in_eval[0] += time.perf_counter() - t
            return out
        t = time.perf_counter()
        rh = R.sens_sobol(O, evaluator, int(opts.seed), prob.lb, prob.ub, prob.nm, host_n, batch=nb)
        th = time.perf_counter() - t
        h.sens_sobol(host_n)
        t = time.perf_counter(); rd = h.sens_sobol(host_n); td = time.perf_counter() - t
        R.assert_equal(rd, rh)
        print("  host loop over eval_batch at N = %d, once: %.2f s, of which inside eval_batch %.1f ms; the device call of the same: %.2f ms; host loop / "
              "device = %.0f, eval_batch alone / device = %.2f; results equal bit for bit"
              % (host_n, th, in_eval[0] * 1e3, td * 1e3, th / td, in_eval[0] / td), flush=True)
        h.close()


if __name__ == "__main__":
    main()
