"""The posterior sample from the device (BGPContext.draws = smm_get_draws: a sizing call, then the row call) against the host path it
replaces on the same context: smm_get_history of the window, then the rows indexed out of the downloaded arrays with numpy as
tests/draws_ref.py indexes them.  Same rows checked bit for bit.  Shape: C5 (SMM_OBJ_DENSE2, 4096 chains x 2000 iterations,
np = nm = 50); one group of every chain and the default temperature groups (the chains with equal acc_tuner); max_rows = 10000;
select 1 (accepted) and 2 (state).  The sizing call is timed on its own as well: its share of the pair is printed.
  python tools/draws_time.py [--chains N] [--iters T] [--no-host]"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import smm_jl_amd as S   # noqa: E402
from smm_jl_amd import _abi as A   # noqa: E402
from smm_jl_amd.workloads import build_problem   # noqa: E402
import draws_ref as DR   # noqa: E402


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def sizing_call(h, T, sel, g, ng, K):
    r = dict(count=np.zeros(ng, np.int64), n_chains=np.zeros(ng, np.int32), row0=np.zeros(ng + 1, np.int64))
    s = h._out(A.smm_draws_t, r)
    h._check(h._fn("get_draws")(h._ctx, 0, T, sel, g.ctypes.data_as(A.c_int32_p), ng, 1, K, 0, C.byref(s)))
    return r


def main():
    N, T, K = arg("--chains", 4096), arg("--iters", 2000), 10000
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
        HW = (8 + prob.np + prob.nm + 1) // 2 * 2
        print("  smm_get_history of %.2f GB: %.2f s" % (N * T * HW * 8 / 1e9, td), flush=True)
    for name, g in cases:
        ng = int(g.max()) + 1
        for sel in (1, 2):
            h.draws(0, T, sel, g, 1, K)   # (first call: allocates the scratch and the result buffer)
            reps, sizing = [], []
            for _ in range(5):
                t = time.perf_counter()
                dev = h.draws(0, T, sel, g, 1, K)
                reps.append(time.perf_counter() - t)
                t = time.perf_counter()
                sizing_call(h, T, sel, g, ng, K)
                sizing.append(time.perf_counter() - t)
            md, ms = np.median(reps), np.median(sizing)
            line = "  %s, select %d: %d rows of %d kept; device %.2f ms (median of 5; the sizing call alone %.2f ms = %.0f %%)" % (
                name, sel, len(dev["value"]), int(dev["count"].sum()), md * 1e3, ms * 1e3, 100 * ms / md)
            if host:
                t = time.perf_counter()
                ref = DR.draws_from_history(hist, 0, T, sel, g, 1, K)
                ti = time.perf_counter() - t
                DR.assert_draws_equal(dev, ref)
                line += "; host: download %.2f s + indexing %.2f s = %.0f x the device; same rows" % (td, ti, (td + ti) / md)
            print(line, flush=True)
    h.close()


if __name__ == "__main__":
    main()
