"""What do the proposal's late tries cost the persistent chain kernel (k_chain_persist_loc) on the headline configuration (C2: 4096 chains,
2p/2m, ns = 10000)?  With SMMHIP_TS=1, per launch of 200 iterations: the iterations in which at least one tile entered persist_late_tries
(its first four tries all left the box), the tile events, the control wave's time inside that call per event (mean over the tiles' means,
and the slowest tile's mean), and min / mean / max over the tiles of "settle+proposal" and of the wait at the barrier (us per iteration:
the means over tiles that tools/persist_time.py prints hide the late tile).  Beside each launch the CPU estimate from the launch's own
starting state (tests/late_tries_ref.py, the form of tools/late_tries_estimate.py).
  python tools/late_tries_time.py [launches] [first launch] [chains]      (default 20 launches from iteration 201 on)"""
import ctypes as C
import os
import sys
import time

import numpy as np

os.environ.setdefault("SMMHIP_TS", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import smm_jl_amd as S, common as cm
import late_tries_ref as LT

K = int(sys.argv[1]) if len(sys.argv) > 1 else 20
K0 = int(sys.argv[2]) if len(sys.argv) > 2 else 1
N = int(sys.argv[3]) if len(sys.argv) > 3 else 4096
IT, LATE_N, NW, TSW = 200, 16384, 16, 8
if os.environ.get("LATE_TRIES_LIB"):   # another build of the library (an experiment hook that lives here, as tools/exp/bench_ab.py's)
    S._abi.LIB_PATH = os.path.join(ROOT, "smm.jl_amd", "csrc", os.environ["LATE_TRIES_LIB"])
lib = S._abi.load()
prob, opts = cm.serial_normal(N=N, T=IT * (K0 + K))
ctx = S.hip_context(prob, opts)
ctx.set_persistent(1)
ctx.step(IT * K0)
tiles = (N + 15) // 16
nt = min(tiles, 2048)


def late_counts():
    b = np.zeros(LATE_N, np.uint64)
    assert lib.smm_debug_ts(ctx._ctx, b.ctypes.data_as(C.c_void_p), -2) == 0
    return b


print("%s: %d chains, launches of %d iterations (SMMHIP_TS=1: the stamps cost time themselves)" % (os.path.basename(S._abi.LIB_PATH), N, IT))
print("| iterations | us / iteration | iterations with >= 1 late tile | tile events | L: us per event, mean / slowest tile | estimate: P(>= 1), E[chains past 4 / past 8] "
      "| settle+proposal min / mean / max | wait min / mean / max |")
print("|---|---|---|---|---|---|---|---|")
tot_it = tot_ev = tot_Lev = 0
tot_L = tot_dt = 0.0
for k in range(K):
    st = ctx.state()
    pf = LT.p_fail(st.sigma, st.la_params, prob.lb, prob.ub)
    (e4, p4), (e8, _) = LT.past_tries(pf, 4), LT.past_tries(pf, 8)
    before = late_counts()
    l0 = ctx.persistent_info()[1]
    t0 = time.perf_counter()
    ctx.step(IT)
    dt = time.perf_counter() - t0
    assert ctx.persistent_info()[1] > l0 and ctx.persistent_info()[2] == 0, "the persistent kernel ran, no repair"
    d = (late_counts() - before).astype(np.int64)
    buf = np.zeros((tiles, 8), np.uint64)
    lib.smm_debug_ts(ctx._ctx, buf.ctypes.data_as(C.c_void_p), tiles)
    nit = int(buf[0, 6])
    ph = buf[:, :6].astype(np.float64) / 100.0 / nit          # us per iteration and tile (100 MHz ticks)
    w = np.zeros((nt, NW, TSW), np.uint64)
    assert lib.smm_debug_ts_waves(ctx._ctx, w.ctypes.data_as(C.c_void_p), nt) == 0
    ev, tk = w[:, 0, 6].astype(np.int64), w[:, 0, 7].astype(np.int64).astype(np.float64)
    assert ev.sum() <= d.sum(), (ev.sum(), d.sum())   # (the per-tile stamps are the step's LAST launch's, the counts by iteration every launch's)
    per = tk[ev > 0] / ev[ev > 0] / 100.0
    first = IT * (K0 + k) + 1
    print("| %d-%d | %.2f | %d of %d | %d | %s | %.2f, %.2f / %.3f | %.2f / %.2f / %.2f | %.2f / %.2f / %.2f |"
          % (first, first + IT - 1, dt / IT * 1e6, (d > 0).sum(), IT, d.sum(), "%.2f / %.2f" % (tk.sum() / ev.sum() / 100.0, per.max()) if ev.sum() else "-",
             p4, e4, e8, ph[:, 3].min(), ph[:, 3].mean(), ph[:, 3].max(), ph[:, 0].min(), ph[:, 0].mean(), ph[:, 0].max()), flush=True)
    tot_it += int((d > 0).sum()); tot_ev += int(d.sum()); tot_Lev += int(ev.sum()); tot_L += tk.sum() / 100.0; tot_dt += dt
n_it = K * IT
print("\nall %d iterations: %.2f us per iteration (host clock around each step); some tile entered persist_late_tries in %d of them (%.1f %%), %d tile events;"
      % (n_it, tot_dt / n_it * 1e6, tot_it, 100.0 * tot_it / n_it, tot_ev))
if tot_ev:
    L = tot_L / tot_Lev
    print("L = %.2f us per event inside persist_late_tries; frequency x L = %.3f us per iteration (iterations with an event x L / iterations)" % (L, tot_it * L / n_it))
