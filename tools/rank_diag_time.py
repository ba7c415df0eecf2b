"""Rank-normalised diagnostics on the device (smm_get_rank_diag: rank-normalised split R-hat, bulk / tail / mean ESS, rank histograms)
against the host path they replace: smm_get_history of the window + the contract's restatement in numpy (tests/rank_diag_ref.py: a
stable argsort and its tie runs per pooled column, AS 241 normal scores, lag by lag until Geyer's sequence is truncated).  The outputs
without a logarithm behind them must be equal, the others within rank_diag_ref.RANK_RTOL (checked here).  Shapes: C2 (objfunc_norm,
4096 chains x 1400 iterations, np = 2) and C5 (SMM_OBJ_DENSE2, 4096 chains x 2000 iterations, np = nm = 50); groups of 8 neighbouring
chains.  Kernel times come from a separate rocprofv3 --kernel-trace --stats run of this script (--no-host).
  python tools/rank_diag_time.py [c2|c5 ...] [--no-host]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import smm_jl_amd as S   # noqa: E402
from smm_jl_amd.workloads import build_problem   # noqa: E402
import rank_diag_ref as R   # noqa: E402

SHAPES = {"c2": (4096, 1400), "c5": (4096, 2000)}


def main():
    shapes = [a for a in sys.argv[1:] if a in SHAPES] or list(SHAPES)
    host = "--no-host" not in sys.argv
    for w in shapes:
        N, T = SHAPES[w]
        prob, opts = build_problem(w, N, N, 0, T, 0)
        h = S.hip_context(prob, opts)
        t = time.time()
        h.step(T)
        print("%s: %d chains x %d iterations, np %d: stepped in %.1f s" % (w, N, T, prob.np, time.time() - t), flush=True)
        groups = np.arange(N) // 8
        h.rank_diag(0, T, groups=groups)   # (first call: allocates the scratch)
        reps = []
        for _ in range(3):
            t = time.perf_counter()
            dev = h.rank_diag(0, T, groups=groups)
            reps.append(time.perf_counter() - t)
        print("  device: %.2f ms (best of 3: %s); bulk status counts 0/1/2/3: %s"
              % (min(reps) * 1e3, ", ".join("%.2f" % (r * 1e3) for r in reps), np.bincount(dev["status"][0].ravel(), minlength=4).tolist()),
              flush=True)
        if host:
            t = time.perf_counter()
            hist = h.history(0, T)
            td = time.perf_counter() - t
            with np.errstate(invalid="ignore", divide="ignore"):
                ref = R.rank_diag_from_history(hist, 0, T, None, 20, groups)
            th = time.perf_counter() - t
            HW = (8 + prob.np + prob.nm + 1) // 2 * 2
            print("  host (smm_get_history of %.2f GB in %.2f s + restatement): %.2f s; device / host = 1 / %.0f"
                  % (N * T * HW * 8 / 1e9, td, th, th / min(reps)), flush=True)
            R.assert_rank_diag_close(dev, ref)
            print("  same results (the outputs behind ndtri within %.1e)" % R.RANK_RTOL, flush=True)
        h.close()


if __name__ == "__main__":
    main()
