"""How often does some chain of the population go past the first 4 (8) tries of its proposal?  No GPU: the oracle's own states of a bench
instance, and per chain  p_fail = 1 - prod_k [Phi((1 - mu01_k) / sigma) - Phi(-mu01_k / sigma)]  from its sigma and last accepted
parameters (tests/late_tries_ref.py); the expected number of chains past n tries in an iteration is  sum p_fail^n.  A tile of the
persistent chain kernels whose chain is past the tries drawn ahead runs the generator between two publications, and every tile of its
cone waits for it (EXPERIMENTS.md §R8.1).
  python tools/late_tries_estimate.py [c2|c3|c4] [iteration ...]     (default c2 at 200 1000 2200 4200; threads = the oracle's maximum)"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import smm_jl_amd as S
from smm_jl_amd.workloads import build_problem
from oracle import oracle as O
import late_tries_ref as LT

wl = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].isdigit() else "c2"
its = [int(a) for a in sys.argv[1:] if a.isdigit()] or [200, 1000, 2200, 4200]
N = {"c2": 4096, "c3": 32768, "c4": 8192}[wl]
O.load()
prob, opts = build_problem(wl, N, N, 0, max(its), 0)
o = O.OracleContext(prob, opts, threads=min(16, O.max_threads()))
print("%s: %d chains, np = %d, smpl_iters %d; the oracle with %d threads" % (wl, N, prob.np, opts.smpl_iters, min(16, O.max_threads())))
print("| after iteration | sigma min / max | E[chains past 4 tries] per iteration | P(>= 1 such chain) | E[chains past 8 tries] | P(>= 1 chain past 8 tries) |")
print("|---|---|---|---|---|---|")
done = 0
t0 = time.time()
for it in sorted(its):
    o.step(it - done)
    done = it
    st = o.state()
    pf = LT.p_fail(st.sigma, st.la_params, prob.lb, prob.ub)
    (e4, p4), (e8, p8) = LT.past_tries(pf, 4), LT.past_tries(pf, 8)
    print("| %d | %.3f / %.3f | %.2f | %.2f | %.3f | %.3f |" % (it, st.sigma.min(), st.sigma.max(), e4, p4, e8, p8), flush=True)
print("(%.0f s)" % (time.time() - t0))
