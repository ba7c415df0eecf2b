"""Scatter search on the device (smm_scatter_population) against the hand path it replaces, on the same problem: candidates made in numpy
by the same contract (include/smmhip.h; a vectorised Philox4x32-10 here), smm_eval_batch (upload, evaluate, download), the argmin on the
host with the contract's validity and tie rules (tests/population_ref.py: select), a one-row history and a full state, smm_set_state.  Both
install the same starts (checked here).  Shapes: C2 (objfunc_norm, 4096 chains, ns = 10000) and C5 (SMM_OBJ_DENSE2, np = nm = 50, 4096
chains), M = 64 candidates per chain.  A context takes a starting population once, so every repetition runs on a fresh context (created
outside the timed region); the median of the repetitions is reported, and the hand path also without its candidate generation.
  python tools/population_time.py [c2|c5 ...] [--reps 5]"""
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
import population_ref as R   # noqa: E402

N, M = 4096, 64
MASK = np.uint64(0xffffffff)


def philox4x32_10(c, k0, k1):
    """c: four uint64 arrays holding 32-bit words; returns the block's four words"""
    c0, c1, c2, c3 = c
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & MASK, (k1 + np.uint64(0xBB67AE85)) & MASK
    return c0, c1, c2, c3


def candidates(prob, opts, M, spread):
    """theta [np][N * M] by the contract (the vectorised form of tests/population_ref.py: candidates)"""
    nq = (prob.np + 1) // 2
    g, m, q = np.meshgrid(np.arange(opts.N, dtype=np.uint64) + np.uint64(opts.chain_offset), np.arange(M, dtype=np.uint64),
                          np.arange(nq, dtype=np.uint64), indexing="ij")
    x = philox4x32_10((g.ravel(), m.ravel(), q.ravel(), np.zeros(g.size, np.uint64)), opts.seed & 0xffffffff,
                      ((opts.seed >> 32) ^ (R.STREAM_POP * 0x9E3779B9)) & 0xffffffff)
    u = np.empty((opts.N * M, 2 * nq))
    u[:, 0::2] = ((((x[0] << np.uint64(32)) | x[1]) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53).reshape(-1, nq)
    u[:, 1::2] = ((((x[2] << np.uint64(32)) | x[3]) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53).reshape(-1, nq)
    u = u[:, :prob.np].T
    lb, span = prob.lb[:, None], (prob.ub - prob.lb)[:, None]
    c = (prob.init[:, None] - lb) / span
    lo, hi = np.maximum(0.0, c - spread * 0.5), np.minimum(1.0, c + spread * 0.5)
    step = u * (hi - lo)
    x01 = lo + step
    sc = x01 * span
    return np.ascontiguousarray(sc + lb)


def hand_path(h, prob, opts, M, spread, keep_init):
    t = [time.perf_counter()]
    th = candidates(prob, opts, M, spread)
    t.append(time.perf_counter())
    v, sm, st = h.eval_batch(th)
    iv, ism, ist = h.eval_batch(prob.init[:, None])
    t.append(time.perf_counter())
    n = opts.N
    pick = R.select(v.reshape(n, M), st.reshape(n, M), iv[0], ist[0], keep_init)
    j = np.arange(n) * M + np.maximum(pick, 0)
    start = np.where(pick < 0, prob.init[:, None], th[:, j])
    value = np.where(pick < 0, iv[0], v[j])
    simM = np.where(pick < 0, ism[:, :1], sm[:, j])
    t.append(time.perf_counter())
    R.install(h, opts, start, value, simM)
    t.append(time.perf_counter())
    return dict(start=start, value=value, pick=pick), np.diff(t)


def main():
    shapes = [a for a in sys.argv[1:] if a in ("c2", "c5")] or ["c2", "c5"]
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
    for w in shapes:
        prob, opts = build_problem(w, N, N, 0, 8, 0)
        warm = S.hip_context(prob, opts)      # (the first launches of every kernel involved)
        warm.scatter_population(M)
        warm.close()
        dev, hand, parts = [], [], []
        for _ in range(reps):
            a, b = S.hip_context(prob, opts), S.hip_context(prob, opts)
            t = time.perf_counter()
            ra = a.scatter_population(M, 1.0, True)
            dev.append(time.perf_counter() - t)
            t = time.perf_counter()
            rb, p = hand_path(b, prob, opts, M, 1.0, True)
            hand.append(time.perf_counter() - t)
            parts.append(p)
            same = all(np.array_equal(ra[f], rb[f]) for f in ("start", "value", "pick"))
            a.step(7); b.step(7)
            same = same and all(np.array_equal(getattr(a.history(), f), getattr(b.history(), f), equal_nan=True) for f in A.HistoryBuffers.FIELDS)
            a.close(); b.close()
            if not same:
                raise SystemExit("%s: the device path and the hand path differ" % w)
        p = np.median(np.array(parts), axis=0) * 1e3
        d, hd = np.median(dev) * 1e3, np.median(hand) * 1e3
        print("%s: %d chains x %d candidates, np %d, nm %d, %d repetitions, medians" % (w, N, M, prob.np, prob.nm, reps))
        print("  device (smm_scatter_population): %.2f ms (%s)" % (d, ", ".join("%.2f" % (x * 1e3) for x in dev)))
        print("  hand path: %.2f ms = candidates in numpy %.2f + smm_eval_batch %.2f + argmin and gather %.2f + smm_set_state %.2f"
              % (hd, p[0], p[1], p[2], p[3]))
        print("  hand / device = %.1f; without the numpy candidates %.1f; picked initial_value: %d of %d chains; same starts and same 7 "
              "iterations behind them: True" % (hd / d, (hd - p[0]) / d, int((ra["pick"] < 0).sum()), N), flush=True)


if __name__ == "__main__":
    main()
