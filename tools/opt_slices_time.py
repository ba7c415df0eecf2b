"""Coordinate search from many starts on the device (smm_opt_slices) against the best the library offered before it, on the same problem:
the contract's K-wide loop (tests/opt_slices_ref.py) driven over BGPContext.eval_batch — one round trip per coordinate step for ALL starts:
candidates made in numpy, uploaded, evaluated, three downloads, the argmin on the host.  For scale also callers.optSlices (one start, one
round trip per parameter and cycle) on 8 of the starts: EIGHT, not K.  And the device call once more with the built-in objectives'
candidates written out and evaluated by k_eval_batch instead of the slice kernel (the test build's seam SMMHIP_OPT_MATERIALISE).
Shapes: C2 (objfunc_norm, np = 2, ns = 10000) and C5 (SMM_OBJ_DENSE2, np = nm = 50) after 200 iterations of 4096 chains, K = 4096 starts =
every chain's best point, G = 16, update = 0.5.  Times are host perf_counter around calls that end in a device synchronisation, medians of
the repetitions; the three paths give the same results (checked here).
  python tools/opt_slices_time.py [c2|c5 ...] [--reps 3] [--tol 1e-3] [--max-cycles 6]"""
import os
import sys
import time
from collections import OrderedDict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import smm_jl_amd as S   # noqa: E402
from smm_jl_amd import _abi as A   # noqa: E402
from smm_jl_amd.workloads import build_problem   # noqa: E402
import opt_slices_ref as R   # noqa: E402

N, G, UPDATE, ITERS = 4096, 16, 0.5, 200


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


def one_start_loop(h, prob, starts, tol, max_cycles):
    """callers.optSlices over the device evaluation, start by start"""
    m = S.MProb()
    names = ["p%d" % k for k in range(prob.np)]
    S.addMoment(m, {"name": ["m%d" % k for k in range(prob.nm)], "value": list(prob.mom), "weight": list(prob.w)})
    out = []
    for s in range(starts.shape[1]):
        m.initial_value, m.params_to_sample = OrderedDict(), OrderedDict()
        S.addSampledParam(m, OrderedDict((n, [float(starts[k, s]), float(prob.lb[k]), float(prob.ub[k])]) for k, n in enumerate(names)))
        out.append(S.optSlices(m, G, tol=tol, update=UPDATE, maxiter=max_cycles, evaluator=lambda mm, P, nb=None: h.eval_batch(P)))
    return out


def main():
    shapes = [a for a in sys.argv[1:] if a in ("c2", "c5")] or ["c2", "c5"]
    reps, tol, mc = arg("--reps", 3, int), arg("--tol", 1e-3, float), arg("--max-cycles", 6, int)
    A.use_test_hooks(True)      # (the same kernels; the build with the seam for the written-out candidates)
    for w in shapes:
        prob, opts = build_problem(w, N, N, 0, ITERS, 0)
        h = S.hip_context(prob, opts)
        h.step(ITERS)
        starts = best_points(h, prob.np)
        os.environ["SMMHIP_OPT_MATERIALISE"] = "1"
        hm = S.hip_context(prob, opts)      # (the seam is read at creation)
        del os.environ["SMMHIP_OPT_MATERIALISE"]
        dev_call = lambda c: c.opt_slices(starts, G, tol, UPDATE, mc)   # noqa: E731
        host_call = lambda: R.opt_slices(h.eval_batch, starts, prob.lb, prob.ub, prob.nm, G, tol, UPDATE, mc)   # noqa: E731
        dev_call(h); dev_call(hm); h.eval_batch(np.repeat(starts, G, axis=1))      # warm: the first launches of every kernel and shape
        t_dev, t_mat, t_host = [], [], []
        for _ in range(reps):      # (alternating: the paths share the host and the device with whatever else runs)
            t = time.perf_counter(); rd = dev_call(h); t_dev.append(time.perf_counter() - t)
            t = time.perf_counter(); rm = dev_call(hm); t_mat.append(time.perf_counter() - t)
            t = time.perf_counter(); rh = host_call(); t_host.append(time.perf_counter() - t)
            R.assert_equal(rd, rh)
            R.assert_equal(rm, rh)
        t = time.perf_counter()
        one = one_start_loop(h, prob, starts[:, :8], tol, mc)
        t_one = time.perf_counter() - t
        same8 = all(o["iterations"] == rd["cycles"][s] and [o["best"]["p"]["p%d" % k] for k in range(prob.np)] == list(rd["best"][:, s])
                    for s, o in enumerate(one))
        d, mt, hs = (np.median(x) for x in (t_dev, t_mat, t_host))
        cyc = rd["cycles"]
        print("%s: K = %d starts (every chain's best point after %d iterations), np %d, nm %d, G = %d, update = %g, tol = %g, max_cycles = %d; %d "
              "repetitions, medians, host perf_counter around synchronised calls" % (w, N, ITERS, prob.np, prob.nm, G, UPDATE, tol, mc, reps))
        print("  cycles run: min %d, median %d, max %d; converged %d of %d; evaluations %d; best value %.6g -> %.6g"
              % (cyc.min(), int(np.median(cyc)), cyc.max(), int(rd["converged"].sum()), N, rd["evaluated"],
                 h.chain_stats(0, ITERS, True, ())["best_value"].min(), rd["value"].min()))
        print("  device (smm_opt_slices, slice kernel): %.1f ms (%s) = %.1f ns per evaluation"
              % (d * 1e3, ", ".join("%.1f" % (x * 1e3) for x in t_dev), d * 1e9 / rd["evaluated"]))
        print("  device, candidates written out + k_eval_batch: %.1f ms (%s); written out / slice = %.3f"
              % (mt * 1e3, ", ".join("%.1f" % (x * 1e3) for x in t_mat), mt / d))
        print("  K-wide host loop over eval_batch: %.1f ms (%s); host loop / device = %.1f" % (hs * 1e3, ", ".join("%.1f" % (x * 1e3) for x in t_host), hs / d))
        print("  callers.optSlices on 8 of the starts (EIGHT, one at a time): %.1f ms, %.1f ms a start; same results as the device for them: %s"
              % (t_one * 1e3, t_one * 1e3 / 8, same8), flush=True)
        h.close(); hm.close()


if __name__ == "__main__":
    main()
