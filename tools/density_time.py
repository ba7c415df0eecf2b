"""Highest-density intervals, half-sample modes and kernel densities on the device (smm_get_density: BGPContext.density, accepted
draws, mass 0.94, 128 grid points, bw.nrd0) against the host path they replace: smm_get_history of the whole window + numpy per column
(sort, the shortest window, the half-sample mode, bw.nrd0, the Gaussian sum on the same grid).  Shapes: C2-like (objfunc_norm, np = 2)
and C5-like (SMM_OBJ_DENSE2, np = 50), 4096 chains x 2000 iterations each; per chain, per temperature group (equal acc_tuners) and in 8 pooled groups of 512 chains
(long columns: the radix sort and the grid-wide window argmin).
The device times are the median of 3 synchronised calls after a warm-up call, for the intervals and modes alone (n_grid = 0) and with
the curves.  The host path is timed on the first HOST_PARAMS parameters of the first HOST_GROUPS groups and scaled to all columns (it is linear
in them); on those columns the intervals and modes must equal the device's, the densities agree to 1e-12 (numpy's exp is not the contract's).
  python tools/density_time.py [c2|c5 ...] [--no-host]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import smm_jl_amd as S   # noqa: E402
from smm_jl_amd.workloads import build_problem   # noqa: E402

SHAPES = {"c2": (4096, 2000), "c5": (4096, 2000)}
MASS, N_GRID, HOST_GROUPS, HOST_PARAMS = 0.94, 128, 8, 4


def host_column(x, n_grid):
    """(hdi_lo, hdi_hi, mode, bw, density on the device's grid rule) of one column, in plain numpy"""
    s = np.sort(x)
    m = len(s)
    k = min(int(np.floor(MASS * m)), m - 1)
    i = int(np.argmin(s[k:] - s[: m - k]))
    lo, n = 0, m
    while n > 3:
        h = (n + 1) // 2
        lo, n = lo + int(np.argmin(s[lo + h - 1: lo + n] - s[lo: lo + n - h + 1])), h
    if n == 1:
        md = s[lo]
    elif n == 2:
        md = (s[lo] + s[lo + 1]) / 2
    else:
        a, b = s[lo + 1] - s[lo], s[lo + 2] - s[lo + 1]
        md = (s[lo] + s[lo + 1]) / 2 if a < b else (s[lo + 1] + s[lo + 2]) / 2 if b < a else s[lo + 1]
    q = np.quantile(s, [0.25, 0.75])
    bw = 0.9 * (min(np.std(x, ddof=1), (q[1] - q[0]) / 1.34) or np.std(x, ddof=1) or abs(x[0]) or 1.0) * m ** -0.2
    d = None
    if n_grid:
        g = np.linspace(s[0] - 3 * bw, s[-1] + 3 * bw, n_grid)
        d = np.empty(n_grid)
        for j0 in range(0, n_grid, 16):   # (tiles: the [grid][m] terms of a long column do not fit memory at once)
            d[j0: j0 + 16] = np.exp(-0.5 * ((g[j0: j0 + 16, None] - x[None, :]) / bw) ** 2).sum(axis=1)
        d = d / m / (bw * np.sqrt(2 * np.pi))
    return s[i], s[i + k], md, bw, d


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
        print("%s: %d chains x %d iterations, np %d: stepped in %.1f s" % (w, N, T, prob.np, time.time() - t), flush=True)
        ids = {}
        dflt = np.array([ids.setdefault(float(a), len(ids)) for a in opts.acc_tuner], np.int32)
        hist, td = None, 0.0
        for name, groups in (("per chain", np.arange(N, dtype=np.int32)), ("temperature groups (%d)" % (dflt.max() + 1), dflt),
                             ("8 pooled groups of %d chains" % (N // 8), (np.arange(N) // (N // 8)).astype(np.int32))):
            G = int(groups.max()) + 1
            for n_grid in (0, N_GRID):
                h.density(0, T, "accepted", groups, (MASS,), n_grid)   # (first call: allocates the buffers)
                reps = []
                for _ in range(3):
                    t = time.perf_counter()
                    dev = h.density(0, T, "accepted", groups, (MASS,), n_grid)
                    reps.append(time.perf_counter() - t)
                what = "intervals and modes" if n_grid == 0 else "with %d-point curves" % n_grid
                print("  %s, %s: device %.1f ms (median of 3: %s); rows %d, statuses 0: %s" %
                      (name, what, np.median(reps) * 1e3, ", ".join("%.1f" % (r * 1e3) for r in reps), dev["count"].sum(),
                       bool((dev["status"] == 0).all())), flush=True)
                if not host:
                    continue
                if hist is None:   # (downloaded once; its time counts in every host row)
                    t = time.perf_counter()
                    hist = h.history(0, T)
                    td = time.perf_counter() - t
                gs, ks = min(G, HOST_GROUPS), min(prob.np, HOST_PARAMS)
                t = time.perf_counter()
                same, worst = True, 0.0
                for g in range(gs):
                    x = np.concatenate([hist.params[hist.accepted[:, c].astype(bool), :, c] for c in np.flatnonzero(groups == g)])
                    for k in range(ks):
                        lo, hi, md, bw, d = host_column(np.ascontiguousarray(x[:, k]), n_grid)
                        same &= (lo, hi, md) == (dev["hdi_lo"][0, g, k], dev["hdi_hi"][0, g, k], dev["mode"][g, k])
                        if n_grid:
                            worst = max(worst, float(np.max(np.abs(d - dev["density"][g, k]) / d.max())))
                th = td + (time.perf_counter() - t) * (G / gs) * (prob.np / ks)
                print("    host (smm_get_history of %.2f GB in %.2f s + numpy on %d of %d groups x %d of %d parameters, scaled): %.1f s; device / host = 1 / %.0f;"
                      " same intervals and modes: %s; densities within %.1e" % (N * T * HW * 8 / 1e9, td, gs, G, ks, prob.np, th, th / np.median(reps), same, worst),
                      flush=True)
                if not same or worst > 1e-12:
                    raise SystemExit("device and host results differ")


if __name__ == "__main__":
    main()
