"""Adapted proposals on the device (smm_get_chain_cov, smm_adapt_proposal) against the host path they replace: smm_get_history of the
window, np.cov and np.linalg.cholesky per chain, then a new context created with the factors and the whole state and history uploaded
again (smm_set_state).  Shapes: C2 (objfunc_norm, 4096 chains x 1400 iterations, np = 2) and C5 (SMM_OBJ_DENSE2, 4096 chains x 2000
iterations, np = nm = 50), every chain with an identity factor.  Wall times of the calls (each synchronises); kernel times come from a
separate rocprofv3 --kernel-trace --stats run of this script, the pair kernel's counters from a counters-only --pmc run.
  python tools/proposal_adapt_time.py [c2|c5 ...] [--no-host] [--reps R]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import smm_jl_amd as S   # noqa: E402
from smm_jl_amd.workloads import build_problem   # noqa: E402

SHAPES = {"c2": (4096, 1400), "c5": (4096, 2000)}


def wall(f, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        r = f()
        ts.append(time.perf_counter() - t)
    return min(ts), r


def host_path(h, prob, opts, T):
    t = time.perf_counter()
    hist, st = h.history(0, T), h.state()
    t_dl = time.perf_counter() - t
    N, npar = hist.value.shape[1], hist.params.shape[1]
    span = (prob.ub - prob.lb)[:, None]
    L = np.empty((N, npar, npar))
    t = time.perf_counter()
    for j in range(N):
        sel = hist.accepted[:, j].astype(bool)
        u = (hist.params[sel, :, j].T - prob.lb[:, None]) / span
        C = np.cov(u, ddof=1)
        L[j] = np.linalg.cholesky(C / np.mean(np.diag(C)) + 1e-8 * np.eye(npar))
    t_cov = time.perf_counter() - t
    t = time.perf_counter()
    opts.chol_L = L
    h2 = S.hip_context(prob, opts)
    st.iter = T
    h2.set_state(st, hist)
    t_new = time.perf_counter() - t
    h2.close()
    return t_dl, t_cov, t_new


def main():
    args = sys.argv[1:]
    host = "--no-host" not in args
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 5
    which = [a for a in args if a in SHAPES] or list(SHAPES)
    for w in which:
        N, T = SHAPES[w]
        prob, opts = build_problem(w, N, N, 0, T, 0)
        opts.chol_L = np.ascontiguousarray(np.broadcast_to(np.eye(prob.np), (N, prob.np, prob.np)))
        h = S.hip_context(prob, opts)
        h.step(T)
        h.sync()
        t_cov, (count, _, _) = wall(lambda: h.chain_cov(0, T, True, True), reps)
        t_ad, st = wall(lambda: h.adapt_proposal(0, T), reps)
        line = dict(workload=w, N=N, T=T, np=prob.np, draws_mean=float(count.mean()), chain_cov_s=round(t_cov, 5),
                    adapt_s=round(t_ad, 5), installed=int((st == 0).sum()))
        if host:
            t_dl, t_np, t_new = host_path(h, prob, opts, T)
            line.update(host_download_s=round(t_dl, 3), host_cov_chol_s=round(t_np, 3), host_recreate_set_state_s=round(t_new, 3),
                        host_total_s=round(t_dl + t_np + t_new, 3))
        print(line, flush=True)
        h.close()


if __name__ == "__main__":
    main()
