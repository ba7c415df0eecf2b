"""The posterior of a user function of each draw on the device (smm_get_derived: BGPContext.derived, accepted rows, Q = 4 outputs, mean,
median, the 2.5 % and 97.5 % quantiles and the covariance) against the two paths beside it: the download-and-numpy path it replaces
(smm_get_history of the whole window, the same transform vectorised, np.mean / np.median / np.quantile / np.cov per group), and
smm_get_group_stats on the same window and groups (BGPContext.group_stats: the same summaries of the np parameter columns, without the
extra row read and the transform).  Shapes: C2-like (objfunc_norm, np = nm = 2) and C5-like (SMM_OBJ_DENSE2, np = 50), 4096 chains x
2000 iterations each; per chain and in 8 pooled groups of 512 chains.  The device times are the median of 3 synchronised calls after a
warm-up call.  The host's means and quantiles must agree with the device's to 1e-9 relative (numpy sums in another order).
  python tools/derived_time.py [c2|c5 ...] [--no-host]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import smm_jl_amd as S   # noqa: E402
from smm_jl_amd.workloads import build_problem   # noqa: E402

SHAPES = {"c2": (4096, 2000), "c5": (4096, 2000)}
PROBS = (0.025, 0.975)
SOURCE = """
SMM_USER_TRANSFORM(const double* theta, int np, const double* sim_moments, int nm, double value, const double* mom, const double* w,
                   const double* udata, int n_udata, const double* tdata, int n_tdata, double* out, int n_out) {
    out[0] = theta[0] / (1.0 + theta[1] * theta[1]);
    out[1] = theta[0] * theta[1];
    out[2] = sim_moments[0] - tdata[0] * sim_moments[1];
    out[3] = sqrt(value);
}
"""


def host_transform(th, sm, va, td):
    return np.stack([th[0] / (1.0 + th[1] * th[1]), th[0] * th[1], sm[0] - td[0] * sm[1], np.sqrt(va)])


def timed(call):
    call()   # (first call: allocates the buffers, loads the module)
    reps = []
    for _ in range(3):
        t = time.perf_counter()
        r = call()
        reps.append(time.perf_counter() - t)
    return r, reps


def main():
    shapes = [a for a in sys.argv[1:] if a in SHAPES] or list(SHAPES)
    host = "--no-host" not in sys.argv
    tr = S.user_transform(SOURCE, 4)
    td = [0.5]
    for w in shapes:
        N, T = SHAPES[w]
        prob, opts = build_problem(w, N, N, 0, T, 0)
        h = S.hip_context(prob, opts)
        t = time.time()
        h.step(T)
        HW = (8 + prob.np + prob.nm + 1) // 2 * 2
        print("%s: %d chains x %d iterations, np %d, nm %d: stepped in %.1f s" % (w, N, T, prob.np, prob.nm, time.time() - t), flush=True)
        hist, tdl = None, 0.0
        for name, groups in (("per chain", np.arange(N, dtype=np.int32)),
                             ("8 pooled groups of %d chains" % (N // 8), (np.arange(N) // (N // 8)).astype(np.int32))):
            G = int(groups.max()) + 1
            dev, reps = timed(lambda: h.derived(tr, 0, T, "accepted", groups, PROBS, td))
            gs, greps = timed(lambda: h.group_stats(0, T, True, groups, PROBS))
            print("  %s: smm_get_derived %.1f ms (median of 3: %s); smm_get_group_stats on the %d parameters %.1f ms (%s); rows %d, "
                  "non-finite %d" % (name, np.median(reps) * 1e3, ", ".join("%.1f" % (r * 1e3) for r in reps), prob.np,
                                      np.median(greps) * 1e3, ", ".join("%.1f" % (r * 1e3) for r in greps), dev["count"].sum(),
                                      dev["n_nonfinite"].sum()), flush=True)
            assert np.array_equal(dev["count"], gs["count"])
            if not host:
                continue
            if hist is None:   # (downloaded once; its time counts in every host row)
                t = time.perf_counter()
                hist = h.history(0, T)
                tdl = time.perf_counter() - t
            t = time.perf_counter()
            acc = hist.accepted != 0
            worst = 0.0
            for g in range(G):
                th, sm, va = [], [], []
                for c in np.flatnonzero(groups == g):
                    rows = acc[:, c]
                    th.append(hist.params[rows, :2, c].T); sm.append(hist.sim_moments[rows, :2, c].T); va.append(hist.value[rows, c])
                y = host_transform(np.concatenate(th, axis=1), np.concatenate(sm, axis=1), np.concatenate(va), td)
                if y.shape[1] < 2:
                    continue
                mean, med, q, cov = y.mean(axis=1), np.median(y, axis=1), np.quantile(y, PROBS, axis=1), np.cov(y)
                sd = np.sqrt(np.diag(cov))                 # (differences in units of each output's spread)
                for a, b, scale in ((mean, dev["mean"][g], sd), (med, dev["median"][g], sd), (q, dev["quantile"][:, g], sd[None, :]),
                                    (cov, dev["cov"][g], np.outer(sd, sd))):
                    worst = max(worst, float(np.max(np.abs(a - b) / np.maximum(scale, 1e-300))))
            th_ = tdl + time.perf_counter() - t
            print("    host (smm_get_history of %.2f GB in %.2f s + numpy on every group): %.1f s; device / host = 1 / %.0f; largest "
                  "relative difference %.1e" % (N * T * HW * 8 / 1e9, tdl, th_, th_ / np.median(reps), worst), flush=True)
            if worst > 1e-9:
                raise SystemExit("device and host results differ")


if __name__ == "__main__":
    main()
