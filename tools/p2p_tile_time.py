"""BASELINE config 5 (dense2, np = nm = 50, 4096 chains) as G shards: G processes on the ONE GPU (HIP IPC windows, all 256 tiles resident),
us per iteration and rank over 200 iterations of the free-running ranks, in the shard form of the persistent tile kernel
(k_chain_persist_tile<2, false, true>) and in the generic per-iteration p2p form (set_persistent(0)); G = 1 is the single shard
(k_chain_persist_tile<2, false, false> against the per-iteration kernels).  The in-kernel phase times of the persistent form's last
launch (SMMHIP_TS=1: lane 0 of every tile, mean over rank 0's tiles) say where a shard's iteration goes.  Ranks on one device are not
xGMI: a peer's window is this device's memory, so the figures are what the protocol costs, not what eight GPUs' links would add.
  python tools/p2p_tile_time.py [G ...]          (default 1 2 4 8; 8 is the only case past four processes)"""
import os
import pickle
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = r"""
import os, sys, pickle, time, ctypes as C
import numpy as np
os.environ["SMMHIP_TS"] = "1"
sys.path.insert(0, {root!r})
import smm_jl_amd as S
from smm_jl_amd.workloads import build_problem
rank, G, Ng, d, pers = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], int(sys.argv[5])
IT, WARM = 200, 50
N = Ng // G
prob, opts = build_problem("c5", N, Ng, rank, 1 + WARM + IT, 0)
c = S.hip_context(prob, opts)
c.set_persistent(bool(pers))
form = c.describe()["persistent"]
def put(tag, data=b""):
    open(os.path.join(d, "%s_%d.tmp" % (tag, rank)), "wb").write(data); os.rename(os.path.join(d, "%s_%d.tmp" % (tag, rank)), os.path.join(d, "%s_%d" % (tag, rank)))
def get(tag, r):
    p = os.path.join(d, "%s_%d" % (tag, r)); t0 = time.time()
    while not os.path.exists(p):
        time.sleep(0.001)
        if time.time() - t0 > 120: raise SystemExit("rank %d: no %s from rank %d" % (rank, tag, r))
    return open(p, "rb").read()
if G > 1:
    handle, _ = c.p2p_init()
    put("handle", handle)
    for r in range(G):
        if r != rank: c.p2p_attach(r, handle=get("handle", r))
    put("mapped"); [get("mapped", r) for r in range(G)]
    step, fin = c.p2p_step, c.p2p_finish
else:
    step, fin = c.step_async, (lambda: None)
step(1); step(WARM); c.sync()
put("warm"); [get("warm", r) for r in range(G)]
t0 = time.perf_counter()
step(IT)
c.sync()
dt = time.perf_counter() - t0
tiles = N // 16
buf = np.zeros((tiles, 8), np.uint64)
S._abi.load().smm_debug_ts(c._ctx, buf.ctypes.data_as(C.c_void_p), tiles)
nit = max(int(buf[0, 7]), 1)
ph = buf[:, :7].astype(np.float64).mean(axis=0) / 100.0 / nit
fin(); c.sync()
put("result", pickle.dumps((dt / IT * 1e6, ph, nit, c.persistent_info(), form)))
[get("result", r) for r in range(G)]
"""
NG = 4096
PH = ("rows+gather+wait", "walk", "donor+settle", "proposal", "objective", "moments", "accept+publish")
for G in [int(x) for x in sys.argv[1:]] or [1, 2, 4, 8]:
    for pers in (1, 0):
        with tempfile.TemporaryDirectory() as d:
            script = os.path.join(d, "w.py")
            open(script, "w").write(WORKER.format(root=ROOT))
            env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
            procs = [subprocess.Popen([sys.executable, script, str(r), str(G), str(NG), d, str(pers)], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True) for r in range(G)]
            outs = [p.communicate(timeout=600)[0] for p in procs]
            for r, p in enumerate(procs):
                if p.returncode != 0:
                    print("rank %d failed:\n%s" % (r, outs[r][-2000:]))
                    sys.exit(1)
            res = [pickle.loads(open(os.path.join(d, "result_%d" % r), "rb").read()) for r in range(G)]
        us = max(r[0] for r in res)
        ph, nit, info, form = res[0][1], res[0][2], res[0][3], res[0][4]
        print("C5, %d rank(s) x %4d chains on one GPU, %-10s form (%s): %7.2f us per iteration and rank (slowest rank); rank 0: %d launches of the persistent form, %d repairs"
              % (G, NG // G, "persistent" if pers else "generic", form if pers else "off", us, info[1], info[2]), flush=True)
        if pers:
            print("   rank 0, last launch (%d iterations), us per iteration, mean over its tiles: %s | sum %.2f"
                  % (nit, " | ".join("%s %.2f" % (n, v) for n, v in zip(PH, ph)), ph.sum()), flush=True)
