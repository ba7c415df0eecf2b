"""The population per iteration on the device (smm_get_trace) against the host path it replaces: smm_get_history of the whole window +
numpy (mean, var, median, quantile along the members) on contiguous columns.  Both give the same numbers (checked here).  Shapes: C2
(objfunc_norm, np = 2) and C5 (SMM_OBJ_DENSE2, np = 50, with and without the simulated moments), 4096 chains x 2000 iterations each, 8
groups of 512 chains (the levels of a tempered population), probs (0.025, 0.5, 0.975), every iteration kept.  Device times are the
median of 5 synchronised calls after a warm-up call, for the rows themselves (select "all", what the host path computes) and for the
state series; the history bytes per second are the window's records (N x T x HW x 8) over the device time, beside the 6.29 TB/s a
copy kernel reaches on this part.  Kernel times come from a separate rocprofv3 --kernel-trace --stats run of this script (--no-host).
  python tools/trace_time.py [c2|c5 ...] [--no-host]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import smm_jl_amd as S   # noqa: E402
from smm_jl_amd.workloads import build_problem   # noqa: E402

SHAPES = {"c2": (4096, 2000), "c5": (4096, 2000)}
PROBS = (0.025, 0.5, 0.975)
HBM = 6.29e12


def host_path(hist, groups, G, moments):
    f = [hist.params[:, k, :] for k in range(hist.params.shape[1])] + [hist.value]
    if moments:
        f += [hist.sim_moments[:, k, :] for k in range(hist.sim_moments.shape[1])]
    T, Sn = hist.value.shape[0], len(f)
    out = dict(mean=np.empty((T, G, Sn)), var=np.empty((T, G, Sn)), median=np.empty((T, G, Sn)), quantile=np.empty((len(PROBS), T, G, Sn)))
    for g in range(G):
        mem = np.flatnonzero(groups == g)
        for s in range(Sn):
            x = np.ascontiguousarray(f[s][:, mem])   # [T][m]: a contiguous column per iteration
            out["mean"][:, g, s] = np.mean(x, axis=-1)
            out["var"][:, g, s] = np.var(x, axis=-1, ddof=1)
            out["median"][:, g, s] = np.median(x, axis=-1)
            out["quantile"][:, :, g, s] = np.quantile(x, PROBS, axis=-1, method="linear")
    return out


def main():
    shapes = [a for a in sys.argv[1:] if a in SHAPES] or list(SHAPES)
    host = "--no-host" not in sys.argv
    for w in shapes:
        N, T = SHAPES[w]
        prob, opts = build_problem(w, N, N, 0, T, 0)
        h = S.hip_context(prob, opts)
        t = time.time()
        h.step(T)
        HW = (8 + prob.np + prob.nm + 1) // 2 * 2
        gb = N * T * HW * 8 / 1e9
        G = 8
        groups = (np.arange(N) // (N // G)).astype(np.int32)   # 8 levels of N / 8 replicas, the C3 layout's groups
        print("%s: %d chains x %d iterations, np %d, nm %d, %d groups: stepped in %.1f s; the window's records %.3f GB" %
              (w, N, T, prob.np, prob.nm, G, time.time() - t, gb), flush=True)
        hist, td = None, 0.0
        for moments in ((False,) if w == "c2" else (False, True)):
            for sel in ("all", "state"):
                h.trace(0, T, 1, sel, moments, groups, PROBS)   # (first call: allocates the scratch and the result buffer)
                reps = []
                for _ in range(5):
                    t = time.perf_counter()
                    dev = h.trace(0, T, 1, sel, moments, groups, PROBS)
                    reps.append(time.perf_counter() - t)
                med = float(np.median(reps))
                print("  moments %s, select %s: device %.2f ms (median of 5: %s); %.3f TB/s of history = %.1f%% of %.2f TB/s" %
                      ("on" if moments else "off", sel, med * 1e3, ", ".join("%.2f" % (r * 1e3) for r in reps), gb / 1e3 / med,
                       100 * gb * 1e9 / med / HBM, HBM / 1e12), flush=True)
                if host and sel == "all":
                    if hist is None:   # (downloaded once; its time counts in every host row)
                        t = time.perf_counter()
                        hist = h.history(0, T)
                        td = time.perf_counter() - t
                    t = time.perf_counter()
                    ref = host_path(hist, groups, G, moments)
                    th = td + time.perf_counter() - t
                    same = all(np.array_equal(dev[f], ref[f], equal_nan=True) for f in ref)
                    print("    host (smm_get_history of %.2f GB in %.2f s + numpy): %.2f s; device / host = 1 / %.0f; same results: %s"
                          % (gb, td, th, th / med, same), flush=True)
                    if not same:
                        raise SystemExit("device and host results differ")


if __name__ == "__main__":
    main()
