"""Histograms of chains and groups of chains on the device (smm_get_histogram) against the host path they replace: smm_get_history of
the whole window + np.histogram / np.histogram2d of each column.  Both give the same counts and edges (checked here).  Shapes: C2
(objfunc_norm, np = 2) and C5 (SMM_OBJ_DENSE2, np = 50), 4096 chains x 2000 iterations each; per-chain histograms and the default
groups (equal acc_tuners), 1-D only and with 2-D pairs.  Device times are the median of 5 synchronised calls after a warm-up call;
kernel times come from a separate rocprofv3 --kernel-trace --stats run of this script (--no-host).
  python tools/histogram_time.py [c2|c5 ...] [--no-host]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import smm_jl_amd as S   # noqa: E402
from smm_jl_amd.workloads import build_problem   # noqa: E402

SHAPES = {"c2": (4096, 2000), "c5": (4096, 2000)}
BINS, BINS2 = 32, 16


def host_path(hist, groups, G, bins, pairs, bins2):
    npar = hist.params.shape[1]
    out = dict(hist=np.zeros((G, npar, bins), np.int64), edges=np.zeros((G, npar, bins + 1)))
    if pairs:
        out["hist2"] = np.zeros((G, len(pairs), bins2, bins2), np.int64)
    for g in range(G):
        mem = np.flatnonzero(groups == g)
        x = np.concatenate([hist.params[hist.accepted[:, c].astype(bool), :, c] for c in mem])
        for k in range(npar):
            out["hist"][g, k], out["edges"][g, k] = np.histogram(x[:, k], bins)
        for p, (a, b) in enumerate(pairs):
            out["hist2"][g, p] = np.histogram2d(x[:, a], x[:, b], bins2)[0]
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
        print("%s: %d chains x %d iterations, np %d: stepped in %.1f s; the window's parameter words %.3f GB" %
              (w, N, T, prob.np, time.time() - t, N * T * prob.np * 8 / 1e9), flush=True)
        ids = {}
        dflt = np.array([ids.setdefault(float(a), len(ids)) for a in opts.acc_tuner], np.int32)
        pairs = [(0, 1)] if prob.np == 2 else [(j, j + 1) for j in range(0, 20, 2)]
        hist, td = None, 0.0
        for name, groups in (("per chain", np.arange(N, dtype=np.int32)), ("default groups (%d)" % (dflt.max() + 1), dflt)):
            G = int(groups.max()) + 1
            for pp in ((), pairs):
                h.histogram(0, T, "accepted", groups, BINS, None, pp, BINS2)   # (first call: allocates the result buffer)
                reps = []
                for _ in range(5):
                    t = time.perf_counter()
                    dev = h.histogram(0, T, "accepted", groups, BINS, None, pp, BINS2)
                    reps.append(time.perf_counter() - t)
                print("  %s, %s: device %.2f ms (median of 5: %s)" % (name, "1-D + %d pairs" % len(pp) if pp else "1-D", np.median(reps) * 1e3,
                                                                      ", ".join("%.2f" % (r * 1e3) for r in reps)), flush=True)
                if host:
                    if hist is None:   # (downloaded once; its time counts in every host row)
                        t = time.perf_counter()
                        hist = h.history(0, T)
                        td = time.perf_counter() - t
                    t = time.perf_counter()
                    ref = host_path(hist, groups, G, BINS, list(pp), BINS2)
                    th = td + time.perf_counter() - t
                    same = all(np.array_equal(dev[f], ref[f]) for f in ref) and (dev["status"] == 0).all()
                    print("    host (smm_get_history of %.2f GB in %.2f s + numpy): %.2f s; device / host = 1 / %.0f; same results: %s"
                          % (N * T * HW * 8 / 1e9, td, th, th / np.median(reps), same), flush=True)
                    if not same:
                        raise SystemExit("device and host results differ")


if __name__ == "__main__":
    main()
