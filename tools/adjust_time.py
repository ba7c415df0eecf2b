"""The regression-adjusted posterior from the device (BGPContext.adjustment = smm_get_adjustment, every output) against the host path it
replaces on the same context: smm_get_history of the window, then numpy on the downloaded arrays — the pooled state series, the
distances, np.quantile for the bandwidth, the weights, np.linalg.lstsq of the weighted centred parameters on the weighted centred
discrepancies, the adjusted draws and their weighted quantiles by a sort.  The host's numbers are numpy's own (BLAS summation order),
so adj_mean is compared to rounding, not bit for bit (tests/ hold the device bit for bit against tests/adjust_ref.py at small shapes).
Shapes: C2 (serialNormal, np = nm = 2), then C5 (SMM_OBJ_DENSE2, np = nm = 50), each 4096 chains x 2000 iterations; one group of every
chain; select 2; tol 0.2; Epanechnikov's kernel; probs 0.025 / 0.5 / 0.975.
  python tools/adjust_time.py [--chains N] [--iters T] [--no-host] [--only c2|c5]"""
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
TOL = 0.2


def arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def host_path(hist, T, prob):
    """numpy on the downloaded history, one group of every chain: (adj_mean, quantiles [3][np])"""
    npar = prob.np
    x = MR.joint_columns(hist, 0, T, 2, np.zeros(hist.value.shape[1], np.int32), 1)[0]
    theta, d = x[:npar], (x[npar:] - np.asarray(prob.mom)[:, None]) / MR.weights(prob.w)[0][:, None]
    d2 = (d * d).sum(axis=0)
    delta2 = np.quantile(d2, TOL)
    keep = d2 < delta2
    om = 1.0 - d2[keep] / delta2
    r = np.sqrt(om)
    d, theta = d[:, keep], theta[:, keep]
    mx, mt = (d * om).sum(axis=1) / om.sum(), (theta * om).sum(axis=1) / om.sum()
    beta = np.linalg.lstsq((r * (d - mx[:, None])).T, (r * (theta - mt[:, None])).T, rcond=None)[0]
    star = theta - beta.T @ d
    q = np.empty((len(PROBS), npar))
    for j in range(npar):
        o = np.argsort(star[j])
        cw = np.cumsum(om[o])
        q[:, j] = star[j][o][np.searchsorted(cw, np.asarray(PROBS) * cw[-1])]
    return mt - mx @ beta, q


def run(workload, N, T, host):
    prob, opts = build_problem(workload, N, N, 0, T, 0)
    h = S.hip_context(prob, opts)
    t = time.time()
    h.step(T)
    print("%s: %d chains x %d iterations, np %d nm %d: stepped in %.1f s" % (workload, N, T, prob.np, prob.nm, time.time() - t), flush=True)
    hist, td = None, 0.0
    if host:
        t = time.perf_counter()
        hist = h.history(0, T)
        td = time.perf_counter() - t
        print("  smm_get_history: %.2f s" % td, flush=True)
    h.adjustment(0, T, 2, None, TOL, 1, None, 0.0, PROBS)   # (first call: allocates the scratch and the result buffer)
    reps = []
    for _ in range(3):
        t = time.perf_counter()
        dev = h.adjustment(0, T, 2, None, TOL, 1, None, 0.0, PROBS)
        reps.append(time.perf_counter() - t)
    md = np.median(reps)
    line = "  one group: status %s, n_kept %d of %d, ess %.0f, n_outside %d; device %.1f ms (median of 3)" % (
        dev["status"].tolist(), dev["n_kept"][0], dev["count"][0], dev["ess"][0], dev["n_outside"].sum(), md * 1e3)
    if host:
        t = time.perf_counter()
        am, q = host_path(hist, T, prob)
        ti = time.perf_counter() - t
        span = np.asarray(prob.ub) - np.asarray(prob.lb)
        line += "; host: download %.2f s + numpy %.2f s = %.0f x the device; adj_mean within %.1e, quantiles within %.1e (of ub - lb)" % (
            td, ti, (td + ti) / md, float(np.max(np.abs(dev["adj_mean"][0] - am) / span)),
            float(np.max(np.abs(dev["adj_quantile"][:, 0] - q) / span)))
    print(line, flush=True)
    h.close()


def main():
    N, T = arg("--chains", 4096), arg("--iters", 2000)
    only = arg("--only", None, str)
    for workload in ("c2", "c5"):
        if only in (None, workload):
            run(workload, N, T, "--no-host" not in sys.argv)


if __name__ == "__main__":
    main()
