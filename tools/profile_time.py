"""The objective and the moments binned along parameters from the device (BGPContext.profile = smm_get_profile: 50 bins per parameter,
one pair at 64 x 64 cells, moments on, accepted rows, one group of every chain) against the host path it replaces on the same context:
smm_get_history of the window, then numpy — np.digitize per parameter, np.bincount / np.minimum.at per bin for the counts, the mean
value, the minimum and the mean moments.  The host's means are bincount sums (another order of additions), so they are compared to
rounding; counts and minima are compared exactly (tests/ hold the device bit for bit against tests/profile_ref.py at small shapes).
Beside it smm_get_histogram with the same arguments on the same context, and both calls' history bytes per second (the window's
records once: N x T x HW x 8 bytes).  Shapes: C2's population (4096 chains x 2000 iterations, np = 2) and C5 (np = nm = 50).
  python tools/profile_time.py [--chains N] [--iters T] [--no-host] [--only c2|c5]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import smm_jl_amd as S   # noqa: E402
from smm_jl_amd.workloads import build_problem   # noqa: E402

BINS, BINS2, REPS = 50, 64, 5


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def host_path(hist, edges, nm):
    """numpy on the downloaded history: per parameter the accepted rows' bins, then counts, mean value, minimum and mean moments"""
    acc = hist.accepted.T != 0                            # [N][T]: the pooled order
    v = hist.value.T[acc]
    sc = np.abs(v) <= np.finfo(float).max
    out = []
    for k in range(hist.params.shape[1]):
        x = hist.params[:, k, :].T[acc]
        e = edges[k]
        b = np.clip(np.searchsorted(e, x, "right") - 1, 0, BINS - 1)
        ok = (x >= e[0]) & (x <= e[-1])
        n = np.bincount(b[ok], minlength=BINS)
        ok &= sc
        m = np.bincount(b[ok], minlength=BINS)
        vmin = np.full(BINS, np.inf)
        np.minimum.at(vmin, b[ok], v[ok])
        with np.errstate(invalid="ignore"):
            vmean = np.bincount(b[ok], v[ok], BINS) / m
            mm = np.stack([np.bincount(b[ok], hist.sim_moments[:, j, :].T[acc][ok], BINS) / m for j in range(nm)], axis=1)
        out.append((n, m, np.where(m > 0, vmin, np.nan), vmean, mm))
    return out


def main():
    N, T = arg("--chains", 4096), arg("--iters", 2000)
    host = "--no-host" not in sys.argv
    for name in ("c2", "c5"):
        if arg("--only", name) != name:
            continue
        prob, opts = build_problem(name, N, N, 0, T, 0)
        h = S.hip_context(prob, opts)
        t = time.time()
        h.step(T)
        rec = 8 * (8 + prob.np + prob.nm)                 # bytes of a history record (smm_params.hpp: H_PARAMS + np + nm doubles)
        gb = N * T * rec / 1e9
        print("%s: %d chains x %d iterations, np %d nm %d, %.2f GB of records: stepped in %.1f s" % (name, N, T, prob.np, prob.nm, gb, time.time() - t),
              flush=True)
        pairs = [(0, 1)]
        kw = dict(select="accepted", groups=None, bins=BINS, pairs=pairs, bins2=BINS2)
        times = {}
        for what, call in (("profile", lambda: h.profile(0, T, moments=True, **kw)), ("histogram", lambda: h.histogram(0, T, **kw))):
            call()                                        # (first call: allocates the scratch and the result buffer)
            reps = []
            for _ in range(REPS):
                t = time.perf_counter()
                r = call()
                reps.append(time.perf_counter() - t)
            times[what] = (float(np.median(reps)), r)
            print("  %-9s: %.1f ms (median of %d, min %.1f, max %.1f): %.1f GB/s of records" % (
                what, times[what][0] * 1e3, REPS, min(reps) * 1e3, max(reps) * 1e3, gb / times[what][0]), flush=True)
        dev, hs = times["profile"][1], times["histogram"][1]
        assert np.array_equal(dev["n"], hs["hist"]) and np.array_equal(dev["n2"], hs["hist2"])
        if host:
            t = time.perf_counter()
            hist = h.history(0, T)
            td = time.perf_counter() - t
            t = time.perf_counter()
            ref = host_path(hist, dev["edges"][0], prob.nm)
            ti = time.perf_counter() - t
            dv = dm = 0.0
            for k, (n, m, vmin, vmean, mm) in enumerate(ref):
                assert np.array_equal(dev["n"][0, k], n) and np.array_equal(dev["n_scored"][0, k], m)
                assert np.array_equal(dev["v_min"][0, k], vmin, equal_nan=True)
                with np.errstate(invalid="ignore", divide="ignore"):
                    dv = max(dv, float(np.nanmax(np.abs(dev["v_mean"][0, k] - vmean) / np.abs(vmean))))
                    dm = max(dm, float(np.nanmax(np.abs(dev["m_mean"][0, k] - mm) / np.maximum(np.abs(mm), 1e-300))))
            print("  host: download %.2f s + numpy (1-D only) %.2f s = %.0f x the device call; counts and minima equal, v_mean within %.1e, m_mean "
                  "within %.1e (relative)" % (td, ti, (td + ti) / times["profile"][0], dv, dm), flush=True)
        h.close()


if __name__ == "__main__":
    main()
