"""Cholesky proposals in the persistent tile kernel (k_chain_persist_tile's CH form, coop_mysample<CT, true>): us per iteration of
  c5     the C5 instance (SMM_OBJ_DENSE2, 50 parameters, 4096 chains)
  norm18 objfunc_norm with 18 parameters, 4096 chains
with per-chain identity factors (--mode chol), without a factor (--mode iso: the isotropic persistent form, the floor — identity factors
compute the same history) and with adapted, non-identity factors late in a run (--mode adapted: WARM iterations, smm_adapt_proposal over
them, then the windows).  Method: a warm-up, then the median of --reps windows of --iters iterations each (enqueued with step_async,
one sync per window).  --lib PATH times another build of libsmmhip.so (an earlier commit's: the per-iteration kernels a factor used to
get) — run the two alternately, in processes of their own, on one machine.  With SMMHIP_TS=1 the persistent kernel's phase stamps of the
last launch are printed (proposal is the phase this work changes).  --per-iteration switches the persistent forms off (set_persistent(False)):
with --mode iso, k_chain_iter on a context without a factor, the kernel that now holds both forms of the cooperative proposal.
  python tools/proposal_chol_time.py [c5|norm18 ...] [--mode chol|iso|adapted] [--lib PATH] [--per-iteration] [--reps R] [--iters K] [--warm W]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import smm_jl_amd as S   # noqa: E402
from smm_jl_amd.workloads import build_problem, general_normal   # noqa: E402

N = 4096


def opt(args, name, default):
    return type(default)(args[args.index(name) + 1]) if name in args else default


def problem(which, T):
    if which == "c5":
        return build_problem("c5", N, N, 0, T, 0)
    prob, opts = general_normal(18, N=N, T=T, ns=2000)
    opts.smpl_iters = 100000
    return prob, opts


def main():
    args = sys.argv[1:]
    mode, reps, iters, warm = opt(args, "--mode", "chol"), opt(args, "--reps", 7), opt(args, "--iters", 100), opt(args, "--warm", 100)
    if "--lib" in args:
        S._abi.LIB_PATH = os.path.abspath(args[args.index("--lib") + 1])
    lib = S._abi.load()
    for which in [a for a in args if a in ("c5", "norm18")] or ["c5", "norm18"]:
        T = warm + reps * iters
        prob, opts = problem(which, T)
        if mode != "iso":
            opts.chol_L = np.ascontiguousarray(np.broadcast_to(np.eye(prob.np), (N, prob.np, prob.np)))
        h = S.hip_context(prob, opts)
        if "--per-iteration" in args:
            h.set_persistent(False)
        h.step(warm)
        installed = None
        if mode == "adapted":
            installed = int((h.adapt_proposal(0, warm, accepted_only=False) == 0).sum())
            h.step(2)   # (the first launch behind the call)
        h.sync()
        us = []
        for _ in range(reps):
            n = min(iters, T - h.state().iter)
            t0 = time.perf_counter()
            h.step_async(n)
            h.sync()
            us.append((time.perf_counter() - t0) / n * 1e6)
        avail, launches, repairs = h.persistent_info()
        line = dict(shape=which, mode=mode, lib=os.path.relpath(S._abi.LIB_PATH, ROOT), form=h.describe()["persistent"], chain=h.describe()["chain"], launches=launches, repairs=repairs,
                    us_per_iter_median=round(float(np.median(us)), 2), us_per_iter_min=round(min(us), 2), us_per_iter_max=round(max(us), 2),
                    windows=reps, iters=iters)
        if installed is not None:
            line["adapted_chains"] = installed
        if os.environ.get("SMMHIP_TS") == "1" and launches:
            tiles = (N + 15) // 16
            buf = np.zeros((tiles, 8), np.uint64)
            lib.smm_debug_ts(h._ctx, buf.ctypes.data_as(C.c_void_p), tiles)
            nit = int(buf[0, 7]) or 1
            ph = buf[:, :7].astype(np.float64).mean(axis=0) / 100.0 / nit   # (100 MHz ticks -> us per iteration, mean over tiles)
            line["phases_us"] = dict(zip(("publish_to_B0", "walk", "donor_settle", "proposal", "objective", "moments", "accept_publish"),
                                         [round(float(x), 2) for x in ph]))
        print(json.dumps(line), flush=True)
        h.close()


if __name__ == "__main__":
    main()
