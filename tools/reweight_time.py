"""The target posterior from every temperature from the device (BGPContext.reweighted = smm_get_reweighted, every output) against the
host path it replaces on the same context: smm_get_history of the window, then numpy on the downloaded arrays — every chain's state
series, its weights exp((acc_tuner - target) v) normalised per chain, the pooled weighted mean and covariance and the weighted quantiles
by a sort.  The host's numbers are numpy's own (its exp and its summation order), so the mean is compared to rounding, not bit for bit
(tests/ hold the device bit for bit against tests/reweight_ref.py at small shapes).  Shapes: C2 (serialNormal, np = nm = 2), then C5
(SMM_OBJ_DENSE2, np = nm = 50), each 4096 chains x 2000 iterations; one group of every chain; select 2; the target is the largest
acc_tuner; probs 0.025 / 0.5 / 0.975.
  python tools/reweight_time.py [--chains N] [--iters T] [--no-host] [--only c2|c5]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import smm_jl_amd as S   # noqa: E402
from smm_jl_amd.workloads import build_problem   # noqa: E402

PROBS = (0.025, 0.5, 0.975)


def arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def host_path(hist, T, acc, target):
    """numpy on the downloaded history, one group of every chain: (mean [np], quantiles [3][np], ess)"""
    N, npar = hist.value.shape[1], hist.params.shape[1]
    rows = np.where(hist.accepted[:T] != 0, np.arange(T)[:, None], -1)
    a = np.maximum.accumulate(rows, axis=0)                  # a(t) per chain
    th, us = [], []
    for c in range(N):
        src = a[:, c][a[:, c] >= 0]
        v = hist.value[src, c]
        ok = np.isfinite(v)
        src, v = src[ok], v[ok]
        if not len(v):
            continue
        lw = (acc[c] - target) * v
        w = np.exp(lw - lw.max())
        th.append(hist.params[src, :, c])
        us.append(w * (w.sum() / (w * w).sum()))
    th, u = np.concatenate(th), np.concatenate(us)
    q = np.empty((len(PROBS), npar))
    for j in range(npar):
        o = np.argsort(th[:, j])
        cw = np.cumsum(u[o])
        q[:, j] = th[o, j][np.minimum(np.searchsorted(cw, np.asarray(PROBS) * cw[-1]), len(cw) - 1)]
    return (u[:, None] * th).sum(axis=0) / u.sum(), q, u.sum() ** 2 / (u * u).sum()


def run(workload, N, T, host):
    prob, opts = build_problem(workload, N, N, 0, T, 0)
    acc = np.asarray(opts.acc_tuner, float)
    target = float(acc.max())
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
    h.reweighted(0, T, 2, None, (target,), PROBS)   # (first call: allocates the scratch and the result buffer)
    reps = []
    for _ in range(3):
        t = time.perf_counter()
        dev = h.reweighted(0, T, 2, None, (target,), PROBS)
        reps.append(time.perf_counter() - t)
    md = np.median(reps)
    line = "  one group, target %.3g: status %s, n_kept %d of %d scored, ess %.0f; device %.1f ms (median of 3)" % (
        target, dev["status"].tolist(), dev["n_kept"][0, 0], dev["n_scored"][0], dev["ess"][0, 0], md * 1e3)
    if host:
        t = time.perf_counter()
        mean, q, ess = host_path(hist, T, acc, target)
        ti = time.perf_counter() - t
        span = np.asarray(prob.ub) - np.asarray(prob.lb)
        line += "; host: download %.2f s + numpy %.2f s = %.0f x the device; mean within %.1e, quantiles within %.1e (of ub - lb), ess within %.1e" % (
            td, ti, (td + ti) / md, float(np.max(np.abs(dev["mean"][0, 0] - mean) / span)),
            float(np.max(np.abs(dev["quantile"][:, 0, 0] - q) / span)), abs(dev["ess"][0, 0] - ess) / ess)
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
