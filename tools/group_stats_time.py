"""Pooled summaries of groups of chains on the device (smm_get_group_stats) against the host path they replace: smm_get_history of the
whole window + np.concatenate of the members' accepted draws + numpy's mean / median / quantile and the np.sum covariance per group.
Both give the same numbers (checked here, NaN equal to NaN).  Shapes: C3 (objfunc_norm, 4096 chains x 2000 iterations, np = 2, 8 levels
of 512 replicas) and C5 (SMM_OBJ_DENSE2, 4096 chains x 2000 iterations, np = nm = 50: one group of every chain, and groups of 64).
Prints the device call's plan and a bytes model of it (the time those bytes take at the 6.0 TB/s streaming rate); kernel times come
from a separate rocprofv3 --kernel-trace --stats run of this script.
  python tools/group_stats_time.py [c3|c5 ...] [--no-host]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import smm_jl_amd as S   # noqa: E402
from smm_jl_amd.workloads import build_problem   # noqa: E402

SHAPES = {"c3": (4096, 2000), "c5": (4096, 2000)}
PROBS = (0.025, 0.975)
CAP = 256 << 20       # smm_reducers_host.hpp: REDUCER_BATCH_CAP
LDS_N = 8192          # smm_stats.hpp: STATS_LDS_N


def host_path(hist, groups, G, probs):
    npar = hist.params.shape[1]
    out = dict(count=np.zeros(G, np.int64), mean=np.full((G, npar), np.nan), median=np.full((G, npar), np.nan),
               quantile=np.full((len(probs), G, npar), np.nan), cov=np.full((G, npar, npar), np.nan))
    for g in range(G):
        mem = np.flatnonzero(groups == g)
        cols = [np.ascontiguousarray(hist.params[hist.accepted[:, c].astype(bool), :, c].T) for c in mem]
        x = np.concatenate(cols, axis=1)
        m = x.shape[1]
        out["count"][g] = m
        if m == 0:
            continue
        for k in range(npar):
            v = np.ascontiguousarray(x[k])
            out["mean"][g, k], out["median"][g, k] = np.mean(v), np.median(v)
            out["quantile"][:, g, k] = np.quantile(v, list(probs))
        if m >= 2:
            d = x - out["mean"][g][:, None]
            for j in range(npar):
                for k in range(j + 1):
                    out["cov"][g, j, k] = out["cov"][g, k, j] = np.sum(d[j] * d[k]) / (m - 1)
    return out


def plan_and_bytes(N, T, npar, HW, counts, R):
    """(kb, Nbc, bytes): the host's plan of a call with cov (smm_reducers_host.hpp: smm_get_group_stats) and the HBM bytes it moves: the counting
    pass reads one 64-B sector of every record; each parameter batch re-reads the records' sectors holding its kb parameters, writes and
    re-reads the packed columns (chunk sums), and reads each long column 6 x ceil(R / 4) times (the select's digits); the cov pass reads
    every record's np parameters, writes the centred chunks and reads 16 columns per tile of 8 x 8 pairs"""
    Mtot = int(np.sum(counts))
    scr = max(min(N * T * (8 * npar + 4), CAP), N * T * 8, npar * LDS_N * 8)
    kb = min(npar, scr // (Mtot * 8))
    Nbc = scr // (npar * LDS_N * 8)
    sect = lambda nbytes: 64 * -(-nbytes // 64)
    nt = -(-npar // 8)
    B = N * T * 64
    for k0 in range(0, npar, kb):
        kbb = min(kb, npar - k0)
        B += N * T * sect(kbb * 8) + 2 * Mtot * kbb * 8 + 6 * -(-R // 4) * Mtot * kbb * 8
    B += N * T * sect(npar * 8) + Mtot * npar * 8 + nt * (nt + 1) // 2 * 16 * Mtot * 8
    return kb, Nbc, B


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
        cases = [("8 groups of 512", np.arange(N) // 512)] if w == "c3" else [("one group", np.zeros(N)), ("groups of 64", np.arange(N) // 64)]
        hist = None
        for name, groups in cases:
            groups = groups.astype(np.int32)
            G = int(groups.max()) + 1
            h.group_stats(0, T, True, groups, PROBS)   # (first call: allocates the scratch)
            reps = []
            for _ in range(3):
                t = time.perf_counter()
                dev = h.group_stats(0, T, True, groups, PROBS)
                reps.append(time.perf_counter() - t)
            HW = (8 + prob.np + prob.nm + 1) // 2 * 2
            kb, Nbc, B = plan_and_bytes(N, T, prob.np, HW, dev["count"], 2 + 2 * len(PROBS))
            print("  %s: pooled draws %d .. %d; kb %d, %d chunks per cov batch; device %.2f ms (best of 3: %s); bytes model %.3f GB -> "
                  "%.2f ms at 6.0 TB/s" % (name, dev["count"].min(), dev["count"].max(), kb, Nbc, min(reps) * 1e3,
                                           ", ".join("%.2f" % (r * 1e3) for r in reps), B / 1e9, B / 6.0e12 * 1e3), flush=True)
            if host:
                t = time.perf_counter()
                if hist is None:
                    hist = h.history(0, T)
                ref = host_path(hist, groups, G, PROBS)
                th = time.perf_counter() - t
                same = all(np.array_equal(dev[f], ref[f], equal_nan=True) for f in ref)
                print("  host (smm_get_history of %.2f GB + concatenate + numpy): %.2f s; device / host = 1 / %.0f; same results: %s"
                      % (N * T * HW * 8 / 1e9, th, th / min(reps), same), flush=True)
                if not same:
                    raise SystemExit("device and host results differ")


if __name__ == "__main__":
    main()
