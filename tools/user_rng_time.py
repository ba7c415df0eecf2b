"""What the library's generator costs a user objective against a hand-rolled one: a panel of 256 agents x 40 periods as a map-reduce user
objective (256 lanes), 4096 chains, shocks either Gaussian from smm_normal2 (tests/user_rng_src.py: PANEL_RNG_SOURCE) or uniform from a 64-bit
LCG (tests/user_objective_src.py: PANEL_SOURCE); each in the persistent tile form (tile_user) and in the per-iteration form.  Prints us per
iteration of every window (a step of `iters` iterations ending in a synchronise), and the median; the first window of every context is warm-up.
  python tools/user_rng_time.py [windows] [iters] [chains]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import smm_jl_amd as S  # noqa: E402
import common as cm  # noqa: E402
from user_objective_src import PANEL_SOURCE  # noqa: E402
from user_rng_src import PANEL_RNG_SOURCE  # noqa: E402

windows = int(sys.argv[1]) if len(sys.argv) > 1 else 7
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 100
N = int(sys.argv[3]) if len(sys.argv) > 3 else 4096
AGENTS, PERIODS, LANES = 256, 40, 256

ids = {"normal2": S.register_user_objective(PANEL_RNG_SOURCE, n_sums=3, lanes=LANES, rng=True),
       "lcg": S.register_user_objective(PANEL_SOURCE, n_sums=3, lanes=LANES)}
out = {"chains": N, "agents": AGENTS, "periods": PERIODS, "lanes": LANES, "iters_per_window": iters, "windows": windows, "runs": []}
T = iters * (windows + 1)
for shocks in ("normal2", "lcg", "normal2", "lcg"):   # (alternated: both measured twice)
    for persistent in (True, False):
        prob = S.Problem(init=[0.3, 1.0], lb=[-0.95, 0.1], ub=[0.95, 3.0], mom=[0.0, 1.3, 0.6], w=[0.05, 0.1, 0.1], ns=1,
                         objective_id=ids[shocks], obj_params=[float(PERIODS), float(AGENTS)])
        opts = S.BGPOpts(N=N, maxiter=T, sigma=0.05 * cm.temps(N, 4.0), acc_tuner=np.geomspace(3.0, 0.5, N), min_improve=np.zeros(N), seed=7)
        ctx = S.hip_context(prob, opts)
        ctx.set_persistent(persistent)
        form = ctx.describe()["persistent"] if persistent else "per-iteration"
        us = []
        for w in range(windows + 1):
            t0 = time.perf_counter()
            ctx.step_async(iters); ctx.sync()
            if w:
                us.append((time.perf_counter() - t0) / iters * 1e6)
        avail, launches, repairs = ctx.persistent_info()
        r = {"shocks": shocks, "form": form, "us_per_iter": us, "median_us": float(np.median(us)), "launches": launches, "repairs": repairs,
             "accept_rate": float(ctx.history().accepted.mean())}
        out["runs"].append(r)
        print("%-8s %-14s us per iteration by window: %s | median %.1f  (persistent launches %d, repairs %d)"
              % (shocks, form, " ".join("%.1f" % x for x in us), r["median_us"], launches, repairs), flush=True)
        ctx.close()
print(json.dumps(out))
