"""The simulation phase of k_chain_persist_loc wave by wave, on the headline configuration (C2: 4096 chains, 2p/2m, ns = 10000), with
SMMHIP_TS=1: the kernel's phase stamps (as tools/persist_time.py) and, per wave of the first tiles, the mean wall clock over the last launch's
iterations at which the wave leaves barrier BB, has issued its last add, has stored its partials (s_part), and at which the control wave's
wait for all partials ends / a worker's side job of the iteration (randomness, table, pair lists, gather) ends.  Times in us after BB, mean
over tiles; the SIMD of a wave is its HW_ID's.  Per SIMD: the first and the last of its waves to issue their last add and to store their
partials, the control wave's share, and the tail in which fewer than 4 waves of the SIMD are still adding (last - first add end).
(Means of per-iteration stamps: the tail of a mean is not the mean of the tails; the wall clock ticks at 100 MHz.)
  python tools/persist_waves.py [steps] [chains]"""
import ctypes as C
import os
import sys
import time

import numpy as np

os.environ.setdefault("SMMHIP_TS", "1")
sys.path.insert(0, '.'); sys.path.insert(0, 'tests')
import smm_jl_amd as S, common as cm

K = int(sys.argv[1]) if len(sys.argv) > 1 else 5
N = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
IT = 200
NW, TSW = 16, 8
lib = S._abi.load()
prob, opts = cm.serial_normal(N=N, T=IT * (K + 1))
ctx = S.hip_context(prob, opts)
ctx.set_persistent(1)
ctx.step(IT)
t0 = time.perf_counter()
for _ in range(K):
    ctx.step_async(IT)
ctx.sync()
dt = time.perf_counter() - t0
avail, launches, repairs = ctx.persistent_info()
print("persistent: %.2f us per iteration, %.1f M chain-evals/s   (launches of the persistent kernel %d)" % (dt / (K * IT) * 1e6, N * K * IT / dt / 1e6, launches))
assert launches, "the persistent kernel did not run"
tiles = (N + 15) // 16
buf = np.zeros((tiles, 8), np.uint64)
lib.smm_debug_ts(ctx._ctx, buf.ctypes.data_as(C.c_void_p), tiles)
nit = int(buf[0, 6])
ph = buf[:, :6].astype(np.float64).mean(axis=0) / 100.0 / nit
print("phases of the last launch, %d iterations (us per iteration, mean over tiles):" % nit, " wait at the barrier (gather) %.2f | walk %.2f | record %.2f | "
      "settle+proposal %.2f | B2+simulation %.2f | accept+publish %.2f | sum %.2f" % (*ph, ph.sum()))
nt = min(tiles, 2048)
w = np.zeros((nt, NW, TSW), np.uint64)
assert lib.smm_debug_ts_waves(ctx._ctx, w.ctypes.data_as(C.c_void_p), nt) == 0
n = w[:, :, 5].astype(np.float64)
assert (n == nit).all(), "every wave stamps every iteration"
m = w[:, :, :4].astype(np.float64) / n[:, :, None]            # mean wall clock (ticks) per tile, wave, stamp
ref = m[:, :, 0].min(axis=1)                                   # the tile's release from BB
rel = (m - ref[:, None, None]) / 100.0                         # us after BB
simd = ((w[:, :, 4] >> np.uint64(4)) & np.uint64(3)).astype(int)
print("\nper wave (us after BB, mean over %d tiles): SIMD (mode) | leaves BB | last add issued | partials stored | %s" % (nt, "wait for all partials ends (wave 0) / side job ends (workers)"))
for v in range(NW):
    md = np.bincount(simd[:, v], minlength=4).argmax()
    print("  wave %2d  SIMD %d (%3.0f %%) | %5.2f | %5.2f | %5.2f | %5.2f" % (v, md, 100.0 * (simd[:, v] == md).mean(), *rel[:, v, :].mean(axis=0)))
print("\nper SIMD (us after BB, mean over tiles; 'ctl' = the SIMD that runs the control wave):")
print("  SIMD  | waves | first / last add issued | first / last partials stored | tail < 4 waves adding | control wave: adds / partials / wait ends")
for s in range(4):
    first_a, last_a, first_r, last_r, tail, cnt = [], [], [], [], [], []
    for ti in range(nt):
        on = simd[ti] == s
        if not on.any():
            continue
        a, r = rel[ti, on, 1], rel[ti, on, 2]
        first_a.append(a.min()); last_a.append(a.max()); first_r.append(r.min()); last_r.append(r.max()); tail.append(a.max() - a.min()); cnt.append(on.sum())
    ctl = simd[:, 0] == s
    cs = "%5.2f / %5.2f / %5.2f" % tuple(rel[ctl, 0, 1:4].mean(axis=0)) if ctl.any() else "-"
    print("  %d%s | %5.2f | %5.2f / %5.2f | %5.2f / %5.2f | %5.2f | %s" % (s, " ctl" if ctl.mean() > 0.5 else "    ", np.mean(cnt), np.mean(first_a), np.mean(last_a),
                                                                          np.mean(first_r), np.mean(last_r), np.mean(tail), cs))
last = rel[:, :, 2].max(axis=1)
print("\nthe phase: last partials stored %.2f (the slowest wave: control %.0f %% of the tiles) | control's wait ends %.2f | slowest worker's partials %.2f"
      % (last.mean(), 100.0 * (rel[:, :, 2].argmax(axis=1) == 0).mean(), rel[:, 0, 3].mean(), rel[:, 1:, 2].max(axis=1).mean()))
