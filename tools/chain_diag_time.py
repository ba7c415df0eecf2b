"""Chain diagnostics on the device (smm_get_chain_diag: accept rate, ESS, split R-hat) against the host path they replace:
smm_get_history of the window + the contract's restatement vectorised over chains (tests/chain_diag_ref.py: row-wise np.sum on
C-contiguous [chains][n] arrays, lag by lag until Geyer's sequence is truncated).  Both give the same numbers (checked here, NaN equal
to NaN).  Shapes: C2 (objfunc_norm, 4096 chains x 1400 iterations, np = 2) and C5 (SMM_OBJ_DENSE2, 4096 chains x 2000 iterations,
np = nm = 50); R-hat over groups of 8 neighbouring chains.  Prints the distribution of the truncation lags (2 J) and the product
count of the work model; kernel times come from a separate rocprofv3 --kernel-trace --stats run of this script (--no-host).
  python tools/chain_diag_time.py [c2|c5 ...] [--no-host]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import smm_jl_amd as S   # noqa: E402
from smm_jl_amd.workloads import build_problem   # noqa: E402
import chain_diag_ref as R   # noqa: E402

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
        h.chain_diag(0, T, groups=groups)   # (first call: allocates the scratch)
        reps = []
        for _ in range(3):
            t = time.perf_counter()
            dev = h.chain_diag(0, T, groups=groups)
            reps.append(time.perf_counter() - t)
        st = dev["status"]
        print("  device: %.2f ms (best of 3: %s); status counts 0/1/2/3: %s"
              % (min(reps) * 1e3, ", ".join("%.2f" % (r * 1e3) for r in reps), np.bincount(st.ravel(), minlength=4).tolist()), flush=True)
        if host:
            t = time.perf_counter()
            hist = h.history(0, T)
            td = time.perf_counter() - t
            pairs = np.zeros(st.size, int)
            with np.errstate(invalid="ignore", divide="ignore"):
                ref = R.diag_from_history(hist, 0, T, None, 0, groups, pairs=pairs)
            th = time.perf_counter() - t
            same = all(np.array_equal(dev[f], ref[f], equal_nan=True) for f in ref)
            lag = 2 * pairs[st.ravel() <= 1]
            q = np.percentile(lag, [0, 50, 90, 99, 100]) if len(lag) else [np.nan] * 5
            HW = (8 + prob.np + prob.nm + 1) // 2 * 2
            print("  host (smm_get_history of %.2f GB in %.2f s + restatement): %.2f s; device / host = 1 / %.0f; same results: %s"
                  % (N * T * HW * 8 / 1e9, td, th, th / min(reps), same), flush=True)
            print("  truncation lag 2J: min %d, median %d, p90 %d, p99 %d, max %d; work model (N S n lags, lags rounded up to the"
                  " device's blocks of 256): %.3g products" % (*q, float(np.sum(T * 256 * np.ceil((lag + 2) / 256.0)))), flush=True)
            if not same:
                raise SystemExit("device and host results differ")
        h.close()


if __name__ == "__main__":
    main()
