"""Chain summaries on the device (smm_get_chain_stats) against the host path they replace: smm_get_history of the whole window + numpy's
mean / median / quantile / argmin / bincount per chain (what host.mean, median, CI, best and summary did).  Both give the same numbers
(checked here, NaN equal to NaN).  Shapes: C2 (objfunc_norm, 4096 chains x 1400 iterations, np = 2) and C5 (SMM_OBJ_DENSE2, 4096 chains
x 2000 iterations, np = nm = 50).  Prints the bytes the device path reads (model from the shapes) and the time they would take at the
6.0 TB/s streaming rate; kernel times come from a separate rocprofv3 --kernel-trace --stats run of this script.
  python tools/chain_stats_time.py [c2|c5 ...] [--no-host]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import smm_jl_amd as S   # noqa: E402
from smm_jl_amd.workloads import build_problem   # noqa: E402

SHAPES = {"c2": (4096, 1400), "c5": (4096, 2000)}
PROBS = (0.025, 0.975)


def host_path(h, T, probs):
    hist = h.history(0, T)
    N, npar = hist.value.shape[1], hist.params.shape[1]
    out = dict(count=np.empty(N, np.int32), mean=np.empty((npar, N)), median=np.empty((npar, N)), quantile=np.empty((len(probs), npar, N)),
               best_value=np.empty(N), best_iter=np.empty(N, np.int32), n_exchanged=np.empty(N, np.int32),
               most_exchanged_with=np.empty(N, np.int32))
    for j in range(N):
        sel = hist.accepted[:, j].astype(bool)
        out["count"][j] = sel.sum()
        for k in range(npar):
            v = hist.params[sel, k, j]
            out["mean"][k, j], out["median"][k, j] = np.mean(v), np.median(v)
            out["quantile"][:, k, j] = np.quantile(v, list(probs))
        i = int(np.argmin(hist.value[:, j]))
        out["best_value"][j], out["best_iter"][j] = hist.value[i, j], i + 1
        ex = hist.exchanged[:, j]
        ew = ex[ex != 0]
        out["n_exchanged"][j] = len(ew)
        out["most_exchanged_with"][j] = int(np.bincount(ew).argmax()) if len(ew) else 0
    return out


def bytes_model(N, T, npar, HW, count_total):
    """HBM bytes of the device path: the gather reads value / exchanged / accepted and the np parameters of every record (whole 64-B
    sectors of them), writes the compacted columns and partner ids; the column kernel reads each column once (the sort is in LDS)"""
    rec_read = N * T * min(HW * 8, 64 * -(-(8 + npar) * 8 // 64))
    cols = count_total * npar * 8
    return rec_read + 2 * cols + 2 * N * T * 4


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
        h.chain_stats(0, T, True, PROBS)   # (first call: allocates the scratch)
        reps = []
        for _ in range(3):
            t = time.perf_counter()
            dev = h.chain_stats(0, T, True, PROBS)
            reps.append(time.perf_counter() - t)
        HW = (8 + prob.np + prob.nm + 1) // 2 * 2
        B = bytes_model(N, T, prob.np, HW, int(dev["count"].sum()))
        print("  device: %.2f ms (best of 3: %s); bytes model %.3f GB -> %.2f ms at 6.0 TB/s"
              % (min(reps) * 1e3, ", ".join("%.2f" % (r * 1e3) for r in reps), B / 1e9, B / 6.0e12 * 1e3), flush=True)
        if host:
            t = time.perf_counter()
            ref = host_path(h, T, PROBS)
            th = time.perf_counter() - t
            same = all(np.array_equal(dev[f], ref[f], equal_nan=True) for f in ref)
            print("  host (smm_get_history of %.2f GB + numpy): %.2f s; device / host = 1 / %.0f; same results: %s"
                  % (N * T * HW * 8 / 1e9, th, th / min(reps), same), flush=True)
            if not same:
                raise SystemExit("device and host results differ")
        h.close()


if __name__ == "__main__":
    main()
