"""Simulated moments per group from the device (BGPContext.moment_stats = smm_get_moment_stats, every output) against the host path it
replaces on the same context: smm_get_history of the window, then numpy on the downloaded arrays — the pooled state series, np.mean,
np.quantile, np.cov of the joint columns, np.linalg.solve for the Jacobian, the sensitivity and the standard errors.  The host's
numbers are numpy's own (BLAS summation order), so they are compared to rounding, not bit for bit (tests/ hold the device bit for bit
against tests/moment_stats_ref.py at small shapes).  Shape: C5 (SMM_OBJ_DENSE2, 4096 chains x 2000 iterations, np = nm = 50); one group
of every chain and the default temperature groups (the chains with equal acc_tuner); select 2; probs 0.025 / 0.5 / 0.975.
  python tools/moment_stats_time.py [--chains N] [--iters T] [--no-host]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import smm_jl_amd as S   # noqa: E402
from smm_jl_amd.workloads import build_problem   # noqa: E402
import moment_stats_ref as MR   # noqa: E402

PROBS = (0.025, 0.5, 0.975)


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def host_path(hist, T, g, ng, prob):
    """numpy on the downloaded history: per group the mean and quantiles of the moments and se by np.linalg"""
    npar = prob.np
    out = []
    for x in MR.joint_columns(hist, 0, T, 2, g, ng):
        C = np.cov(x)
        J = np.linalg.solve(C[:npar, :npar], C[:npar, npar:]).T
        s, W = MR.weights(prob.w)
        JW = J.T * W
        L = -np.linalg.solve(JW @ J, JW)
        out.append((x[npar:].mean(axis=1), np.quantile(x[npar:], PROBS, axis=1), np.sqrt(np.diag((L * (s * s)) @ L.T))))
    return out


def main():
    N, T = arg("--chains", 4096), arg("--iters", 2000)
    host = "--no-host" not in sys.argv
    prob, opts = build_problem("c5", N, N, 0, T, 0)
    h = S.hip_context(prob, opts)
    t = time.time()
    h.step(T)
    print("c5: %d chains x %d iterations, np %d nm %d: stepped in %.1f s" % (N, T, prob.np, prob.nm, time.time() - t), flush=True)
    ids = {}
    temp = np.array([ids.setdefault(float(a), len(ids)) for a in opts.acc_tuner], np.int32)
    cases = [("one group", np.zeros(N, np.int32)), ("%d temperature groups" % len(ids), temp)]
    hist, td = None, 0.0
    if host:
        t = time.perf_counter()
        hist = h.history(0, T)
        td = time.perf_counter() - t
        print("  smm_get_history: %.2f s" % td, flush=True)
    for name, g in cases:
        ng = int(g.max()) + 1
        h.moment_stats(0, T, 2, g, PROBS)   # (first call: allocates the scratch and the result buffer)
        reps = []
        for _ in range(3):
            t = time.perf_counter()
            dev = h.moment_stats(0, T, 2, g, PROBS)
            reps.append(time.perf_counter() - t)
        md = np.median(reps)
        line = "  %s: status %s; device %.1f ms (median of 3)" % (name, np.bincount(dev["status"], minlength=5).tolist(), md * 1e3)
        if host:
            t = time.perf_counter()
            ref = host_path(hist, T, g, ng, prob)
            ti = time.perf_counter() - t
            dm = max(float(np.max(np.abs(dev["m_mean"][k] - r[0]) / np.abs(r[0]))) for k, r in enumerate(ref))
            ok = [k for k in range(ng) if dev["status"][k] == 0]
            ds = max([float(np.max(np.abs(dev["se"][k] - ref[k][2]) / ref[k][2])) for k in ok] or [float("nan")])
            line += "; host: download %.2f s + numpy %.2f s = %.0f x the device; m_mean within %.1e, se within %.1e (relative)" % (
                td, ti, (td + ti) / md, dm, ds)
        print(line, flush=True)
    h.close()


if __name__ == "__main__":
    main()
