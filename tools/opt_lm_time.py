"""Levenberg–Marquardt from many starts on the device (smm_opt_lm) beside the two optimisers that use the objective value alone, from the same
starts: smm_opt_simplex (step 0.05, adaptive, xatol = fatol = 1e-4, max_iter 100 at C4 and 30 at C5: tools/opt_simplex_time.py's setting)
and smm_opt_slices (G = 16, update = 0.5, tol = 1e-3, 6 cycles: tools/opt_slices_time.py's).  Per optimiser the time of the call, the
evaluations it spent and the median and lowest value it reached; for smm_opt_lm also the statuses, iterations and tries, and the median
sum of squared residuals.  Shapes: C4 (banana, np = 10 — its moments are constant, so every Levenberg–Marquardt search must end with
status 4 at its first Jacobian: the timing there is the call's floor) and C5 (SMM_OBJ_DENSE2, np = nm = 50) after 200 iterations of 4096
chains, K = 4096 starts = every chain's best point.  Times are host perf_counter around calls that end in a device synchronisation, medians
of the repetitions after one warm call.
Time per kernel: --device-only runs smm_opt_lm alone, `reps` times after one warm call — the run to put under a kernel trace
(rocprofv3 --kernel-trace --stats --output-format csv -- python tools/opt_lm_time.py c5 --device-only --reps 1); --kernel-stats FILE reads
that trace's kernel_stats.csv and prints, per kernel of the call, launches, total and mean time, and the sums for the evaluation
(k_eval_lm, k_eval_batch), the state kernels (k_lm_*) and the list compaction (k_compact).
  python tools/opt_lm_time.py [c4|c5 ...] [--reps 3] [--max-iter 100] [--fd-step 1e-4] [--device-only] [--kernel-stats FILE]"""
import csv
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, ITERS = 4096, 200
SX = dict(step=0.05, adaptive=True, xatol=1e-4, fatol=1e-4)
SX_MAX_ITER = {"c4": 100, "c5": 30}
SL_G, SL_UPDATE, SL_TOL, SL_CYCLES = 16, 0.5, 1e-3, 6


def arg(name, default, kind):
    return kind(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def kernel_stats(path):
    """the rows of a kernel_stats.csv (Name, Calls, TotalDurationNs, ...) that belong to the call, and the sums by family"""
    fam = {"evaluation": r"\bk_eval_(?:lm|batch)\b", "state": r"\bk_lm_\w+", "compaction": r"\bk_compact\b"}
    tot = dict.fromkeys(fam, 0.0)
    for row in csv.DictReader(open(path)):
        name = row["Name"]
        hit = [f for f, p in fam.items() if re.search(p, name)]
        if not hit and "user_objective" not in name:
            continue
        ns, calls = float(row["TotalDurationNs"]), int(row["Calls"])
        short = re.search(r"\b(k_\w+(?:<[^>]*>)?|\w*user_objective\w*)", name)
        print("  %-28s %6d launches  %10.3f ms  %8.2f us each" % (short.group(1) if short else name[:28], calls, ns / 1e6, ns / 1e3 / calls))
        for f in hit:
            tot[f] += ns
    print("  sums: " + "; ".join("%s %.3f ms" % (f, v / 1e6) for f, v in tot.items()))


def best_points(h, np_):
    """every chain's best point as chain_stats reports it (best_iter over the accepted draws), row by row of the history"""
    bi = h.chain_stats(0, ITERS, True, ())["best_iter"]
    starts = np.empty((np_, N))
    for t in np.unique(bi):
        row = h.history(int(t) - 1, int(t)).params[0]
        starts[:, bi == t] = row[:, bi == t]
    return starts


def main():
    if "--kernel-stats" in sys.argv:
        return kernel_stats(arg("--kernel-stats", None, str))
    import smm_jl_amd as S
    from smm_jl_amd.workloads import build_problem
    shapes = [a for a in sys.argv[1:] if a in ("c4", "c5")] or ["c4", "c5"]
    reps, max_iter, fd_step = arg("--reps", 3, int), arg("--max-iter", 100, int), arg("--fd-step", 1e-4, float)
    device_only = "--device-only" in sys.argv
    ms = lambda x: ", ".join("%.1f" % (y * 1e3) for y in x)   # noqa: E731

    def timed(call):
        call()      # warm: the first launches of every kernel and shape
        ts = []
        for _ in range(reps):
            t = time.perf_counter(); r = call(); ts.append(time.perf_counter() - t)
        return r, ts

    for w in shapes:
        prob, opts = build_problem(w, N, N, 0, ITERS, 0)
        h = S.hip_context(prob, opts)
        h.step(ITERS)
        starts = best_points(h, prob.np)
        start_value = h.eval_batch(starts)[0]
        rl, t_lm = timed(lambda: h.opt_lm(starts, fd_step=fd_step, max_iter=max_iter))
        st, it = rl["status"], rl["iterations"]
        print("%s: K = %d starts (every chain's best point after %d iterations), np %d, nm %d; %d repetitions after a warm call, host perf_counter "
              "around synchronised calls; median value of the starts %.6g" % (w, N, ITERS, prob.np, prob.nm, reps, np.median(start_value)))
        print("  smm_opt_lm (fd_step %g, max_iter %d, the other arguments at their defaults): %.1f ms (%s); %d evaluations = %.1f ns each; status 0 / 1 / "
              "2 / 3 / 4: %s; iterations min %d, median %d, max %d; tries median %d, max %d; value median %.6g, lowest %.6g; ssr median %.6g"
              % (fd_step, max_iter, np.median(t_lm) * 1e3, ms(t_lm), rl["evaluated"], np.median(t_lm) * 1e9 / rl["evaluated"],
                 " / ".join(str(int((st == s).sum())) for s in range(5)), it.min(), int(np.median(it)), it.max(), int(np.median(rl["tries"])),
                 rl["tries"].max(), np.median(rl["value"]), np.nanmin(rl["value"]), np.median(rl["ssr"])), flush=True)
        if not device_only:
            rs, t_sx = timed(lambda: h.opt_simplex(starts, max_iter=SX_MAX_ITER[w], **SX))
            ro, t_sl = timed(lambda: h.opt_slices(starts, SL_G, SL_TOL, SL_UPDATE, SL_CYCLES))
            print("  smm_opt_simplex (step %g, adaptive, xatol = fatol = %g, max_iter %d): %.1f ms (%s); %d evaluations; value median %.6g, lowest %.6g"
                  % (SX["step"], SX["xatol"], SX_MAX_ITER[w], np.median(t_sx) * 1e3, ms(t_sx), rs["evaluated"], np.median(rs["value"]), np.nanmin(rs["value"])))
            print("  smm_opt_slices (G %d, update %g, tol %g, %d cycles): %.1f ms (%s); %d evaluations; value median %.6g, lowest %.6g"
                  % (SL_G, SL_UPDATE, SL_TOL, SL_CYCLES, np.median(t_sl) * 1e3, ms(t_sl), ro["evaluated"], np.median(ro["value"]), np.nanmin(ro["value"])))
            print("  searches where smm_opt_lm ends lower than the simplex: %d of %d; than the slices: %d of %d"
                  % (int((rl["value"] < rs["value"]).sum()), N, int((rl["value"] < ro["value"]).sum()), N), flush=True)
        h.close()


if __name__ == "__main__":
    main()
