"""Nelder–Mead from many starts on the device (smm_opt_simplex) against the best host loop the library offered before it, on the same
problem: the contract's K-wide loop (tests/simplex_ref.py) driven over BGPContext.eval_batch — one upload and three downloads per evaluation
launch (reflected points, second points, shrunk vertices) for ALL running starts, the simplex arithmetic in numpy on the host.  The host
loop's time is reported whole and as the part spent inside eval_batch alone: the first includes this restatement's per-search Python, which
a compiled host loop would not pay; the second is what no host loop can avoid.  On the same starts also smm_opt_slices (G = 16, update =
0.5, tol = 1e-3, 6 cycles: tools/opt_slices_time.py's setting): the median final value and the evaluations each optimiser spent.
Shapes: C4 (banana, np = 10) and C5 (SMM_OBJ_DENSE2, np = nm = 50) after 200 iterations of 4096 chains, K = 4096 starts = every chain's
best point.  Times are host perf_counter around calls that end in a device synchronisation, medians of the repetitions; the two paths give
the same results (checked here).  --device-only runs the device call alone, `reps` times after one warm call: the run to put under a
kernel trace, whose per-kernel sums say how the call's time divides between the state kernels (k_sx_*) and the evaluation.
  python tools/opt_simplex_time.py [c4|c5 ...] [--reps 3] [--max-iter-c4 100] [--max-iter-c5 30] [--device-only]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import smm_jl_amd as S   # noqa: E402
from smm_jl_amd.workloads import build_problem   # noqa: E402
import simplex_ref as R   # noqa: E402

N, ITERS = 4096, 200
STEP, ADAPTIVE, XATOL, FATOL = 0.05, True, 1e-4, 1e-4
SL_G, SL_UPDATE, SL_TOL, SL_CYCLES = 16, 0.5, 1e-3, 6


def arg(name, default, kind):
    return kind(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def best_points(h, np_):
    """every chain's best point as chain_stats reports it (best_iter over the accepted draws), row by row of the history"""
    bi = h.chain_stats(0, ITERS, True, ())["best_iter"]
    starts = np.empty((np_, N))
    for t in np.unique(bi):
        row = h.history(int(t) - 1, int(t)).params[0]
        starts[:, bi == t] = row[:, bi == t]
    return starts


def main():
    shapes = [a for a in sys.argv[1:] if a in ("c4", "c5")] or ["c4", "c5"]
    reps = arg("--reps", 3, int)
    max_iter = {"c4": arg("--max-iter-c4", 100, int), "c5": arg("--max-iter-c5", 30, int)}
    device_only = "--device-only" in sys.argv
    for w in shapes:
        prob, opts = build_problem(w, N, N, 0, ITERS, 0)
        h = S.hip_context(prob, opts)
        h.step(ITERS)
        starts = best_points(h, prob.np)
        mi = max_iter[w]
        dev_call = lambda: h.opt_simplex(starts, STEP, ADAPTIVE, XATOL, FATOL, mi)   # noqa: E731
        dev_call()      # warm: the first launches of every kernel and shape
        if device_only:
            t_dev = []
            for _ in range(reps):
                t = time.perf_counter(); rd = dev_call(); t_dev.append(time.perf_counter() - t)
            print("%s: device only, K = %d, np %d, max_iter %d: %s ms; evaluations %d; iterations median %d, max %d; status 1 / 0 / 2: %d / %d / %d; "
                  "value median %.6g -> %.6g, best -> %.6g" % (w, N, prob.np, mi, ", ".join("%.1f" % (x * 1e3) for x in t_dev), rd["evaluated"],
                                                              int(np.median(rd["iterations"])), rd["iterations"].max(), (rd["status"] == 1).sum(),
                                                              (rd["status"] == 0).sum(), (rd["status"] == 2).sum(), np.median(h.eval_batch(starts)[0]),
                                                              np.median(rd["value"]), np.nanmin(rd["value"])), flush=True)
            h.close()
            continue
        in_eval = [0.0]

        def evaluator(P):
            t = time.perf_counter()
            out = h.eval_batch(P)
            in_eval[0] += time.perf_counter() - t
            return out
        h.eval_batch(np.repeat(starts, prob.np + 1, axis=1))
        t_dev, t_host, t_eval, t_sl = [], [], [], []
        for _ in range(reps):      # (alternating: the paths share the host and the device with whatever else runs)
            t = time.perf_counter(); rd = dev_call(); t_dev.append(time.perf_counter() - t)
            in_eval[0] = 0.0
            t = time.perf_counter(); rh = R.opt_simplex(evaluator, starts, prob.lb, prob.ub, prob.nm, STEP, ADAPTIVE, XATOL, FATOL, mi)
            t_host.append(time.perf_counter() - t); t_eval.append(in_eval[0])
            R.assert_equal(rd, rh)
            t = time.perf_counter(); rs = h.opt_slices(starts, SL_G, SL_TOL, SL_UPDATE, SL_CYCLES); t_sl.append(time.perf_counter() - t)
        d, hs, he, sl = (np.median(x) for x in (t_dev, t_host, t_eval, t_sl))
        ms = lambda x: ", ".join("%.1f" % (y * 1e3) for y in x)   # noqa: E731
        it = rd["iterations"]
        start_value = h.eval_batch(starts)[0]
        print("%s: K = %d starts (every chain's best point after %d iterations), np %d, nm %d; step %g, adaptive %s, xatol %g, fatol %g, max_iter %d; "
              "%d repetitions, medians, host perf_counter around synchronised calls" % (w, N, ITERS, prob.np, prob.nm, STEP, ADAPTIVE, XATOL, FATOL, mi, reps))
        print("  iterations run: min %d, median %d, max %d; status 1 / 0 / 2: %d / %d / %d; moves (reflection, expansion, outside, inside, shrink): %s; "
              "evaluation launches of the host loop: %d" % (it.min(), int(np.median(it)), it.max(), (rd["status"] == 1).sum(), (rd["status"] == 0).sum(),
                                                           (rd["status"] == 2).sum(), [int(x) for x in rd["moves"].sum(1)], rh["launches"]))
        print("  device (smm_opt_simplex): %.1f ms (%s) = %.1f ns per evaluation, %.3f ms per lock-step iteration"
              % (d * 1e3, ms(t_dev), d * 1e9 / rd["evaluated"], d * 1e3 / max(1, it.max())))
        print("  K-wide host loop over eval_batch: %.1f ms (%s), of which inside eval_batch %.1f ms (%s); host loop / device = %.1f, eval_batch alone / "
              "device = %.2f" % (hs * 1e3, ms(t_host), he * 1e3, ms(t_eval), hs / d, he / d))
        print("  from the same starts, median value %.6g: smm_opt_simplex -> median %.6g, best %.6g with %d evaluations; smm_opt_slices (G %d, update %g, "
              "tol %g, %d cycles) -> median %.6g, best %.6g with %d evaluations in %.1f ms (%s); searches where the simplex ends lower: %d of %d"
              % (np.median(start_value), np.median(rd["value"]), np.nanmin(rd["value"]), rd["evaluated"], SL_G, SL_UPDATE, SL_TOL, SL_CYCLES,
                 np.median(rs["value"]), np.nanmin(rs["value"]), rs["evaluated"], sl * 1e3, ms(t_sl), int((rd["value"] < rs["value"]).sum()), N), flush=True)
        h.close()


if __name__ == "__main__":
    main()
