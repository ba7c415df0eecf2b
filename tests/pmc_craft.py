"""Crafted objectives for smm_abc_pmc's edge tests (tests/test_pmc_craft.py, tests/test_gpu_abc_pmc_edges.py), each a one-thread user
objective with a numpy twin of the same few exact operations (fabs, floor, compares, one division by a power of two; the bowl's products
and sums are rounded one by one on both sides), so that the twin equals the device's evaluation to the bit by construction.  The cases'
sizes and seeds are committed here with the conditions they were chosen for: tests/test_pmc_craft.py asserts every condition on the
restatement (tests/pmc_ref.py) with the twins, without a GPU; the GPU tier asserts the same condition on the restatement run with the
context's own eval_batch before it compares the device.  A twin and a device objective that disagree then show as a failed condition.

STAIRCASE  np = 2, box [-1, 1]^2, udata = [levels L (a power of two), shift s]: r = max(|theta0|, |theta1|), v = (floor(L r) - s) / L; where
           v == 0.0 the value is -0.0 for theta0 < 0 and +0.0 otherwise.  L + 1 distinct values, some negative, both zeros: every select has ties.
CONSTANT   np = 2: the value +0.0 everywhere.
ISLANDS    np = 1, box [-1, 1], udata = [half-width hw]: the value |theta|; status 1 where |theta - 0.5| < hw or |theta + 0.5| < hw, -2 elsewhere.
           hw >= 1.5 makes every point of the box valid: a continuous objective.
BOWL       any np (10, and 64 for the floor), box [-1, 1]^np: the sum of squares, added left to right.
The moments of each are its first two parameters (ISLANDS: theta and |theta|); every status but ISLANDS' is 1.

Not covered here: the underflow rule (D < DBL_MIN).  A new particle sits n away from its parent in whitened space with |n| <= 8.6 a coordinate,
and wn >= 2^-42, so D cannot fall below DBL_MIN through the public call for np <= 64: the rule stays with the CPU tier.  Tied parameter
values in the quantile are not reachable with distinct particles either."""
import math

import numpy as np

import reweight_ref as RW

_HEAD = ("SMM_USER_OBJECTIVE(const double* theta, int np, const double* mom, const double* w, int nm,\n"
         "                   const double* udata, int n_udata, double* sim_moments, double* value, int* status)\n{\n")

STAIRCASE_SOURCE = _HEAD + r"""
    const double a0 = __builtin_fabs(theta[0]), a1 = __builtin_fabs(theta[1]);
    const double r = a0 > a1 ? a0 : a1;
    const double L = udata[0], s = udata[1];
    const double lr = L * r;
    const double f = __builtin_floor(lr) - s;
    double v = f / L;
    if (v == 0.0) v = theta[0] < 0.0 ? -0.0 : 0.0;
    sim_moments[0] = theta[0];
    sim_moments[1] = theta[1];
    *value = v;
    *status = 1;
}
"""
CONSTANT_SOURCE = _HEAD + r"""
    sim_moments[0] = theta[0];
    sim_moments[1] = theta[1];
    *value = 0.0;
    *status = 1;
}
"""
ISLANDS_SOURCE = _HEAD + r"""
    const double t = theta[0], hw = udata[0];
    const double dp = __builtin_fabs(t - 0.5), dm = __builtin_fabs(t + 0.5);
    sim_moments[0] = t;
    sim_moments[1] = __builtin_fabs(t);
    *value = __builtin_fabs(t);
    *status = (dp < hw || dm < hw) ? 1 : -2;
}
"""
BOWL_SOURCE = _HEAD + r"""
    double v = theta[0] * theta[0];
    for (int k = 1; k < np; ++k) { const double p = theta[k] * theta[k]; v = v + p; }
    sim_moments[0] = theta[0];
    sim_moments[1] = theta[1];
    *value = v;
    *status = 1;
}
"""
SOURCES = {"staircase": STAIRCASE_SOURCE, "constant": CONSTANT_SOURCE, "islands": ISLANDS_SOURCE, "bowl": BOWL_SOURCE}
NPAR = {"staircase": 2, "constant": 2, "islands": 1, "bowl": 10}
NM = 2


# ---- the numpy twins: f(P [np][n]) -> (value [n], sim_moments [2][n], status [n]) -----------------------------------------------------------
def staircase(L, s):
    L, s = np.float64(L), np.float64(s)

    def f(P):
        P = np.asarray(P, np.float64)
        a0, a1 = np.fabs(P[0]), np.fabs(P[1])
        r = np.where(a0 > a1, a0, a1)
        v = (np.floor(L * r) - s) / L
        v = np.where(v == 0.0, np.where(P[0] < 0.0, -0.0, 0.0), v)
        return v, P[:2].copy(), np.ones(P.shape[1], np.int8)
    return f


def constant(P):
    P = np.asarray(P, np.float64)
    return np.zeros(P.shape[1]), P[:2].copy(), np.ones(P.shape[1], np.int8)


def islands(hw):
    hw = np.float64(hw)

    def f(P):
        t = np.asarray(P, np.float64)[0]
        ok = (np.fabs(t - 0.5) < hw) | (np.fabs(t + 0.5) < hw)
        return np.fabs(t), np.stack([t, np.fabs(t)]), np.where(ok, 1, -2).astype(np.int8)
    return f


def bowl(P):
    P = np.asarray(P, np.float64)
    v = P[0] * P[0]
    for k in range(1, P.shape[0]):
        v = v + P[k] * P[k]
    return v, P[:2].copy(), np.ones(P.shape[1], np.int8)


def twin(name, udata=()):
    return {"staircase": lambda: staircase(*udata), "constant": lambda: constant, "islands": lambda: islands(*udata), "bowl": lambda: bowl}[name]()


def problem(S, name, oid, udata, seed, npar=None):
    """the box [-1, 1]^np with `name`'s objective under the handle oid; opts.seed is the sampler's seed"""
    n = npar or NPAR[name]
    prob = S.Problem(init=np.zeros(n), lb=-np.ones(n), ub=np.ones(n), mom=np.zeros(NM), w=np.ones(NM), ns=1, objective_id=oid,
                     obj_params=[float(x) for x in udata] or None)
    opts = S.BGPOpts(N=1, maxiter=1, sigma=[0.05], acc_tuner=[1.0], min_improve=[0.0], seed=seed)
    return prob, opts


# ---- helpers of the conditions ------------------------------------------------------------------------------------------------------------------
def key(x):
    return RW.total_order_key(np.atleast_1d(np.asarray(x, np.float64)))


def zero_classes(v):
    """which of "negative", "-0", "+0" occur among the values v"""
    v = np.asarray(v, np.float64)
    v = v[~np.isnan(v)]
    out = set()
    if (v < 0).any():
        out.add("negative")
    if ((v == 0) & np.signbit(v)).any():
        out.add("-0")
    if ((v == 0) & ~np.signbit(v)).any():
        out.add("+0")
    return out


def new_finite(want):
    """per generation g >= 1 that ran: (the kept set's size it was proposed from, its new particles with a finite distance)"""
    return [(len(t["wn"]), int(np.isfinite(t["rho_new"]).sum())) for t in want["trace"] if "rho_new" in t]


# ---- A. ties: the staircase ---------------------------------------------------------------------------------------------------------------------
TIES_UDATA = (4.0, 1.0)
TIES = dict(max_gen=3, p_acc_min=0.0, probs=(0.0, 0.5, 1.0))
# (P, A, seed) -> the classes of zero and sign among the final kept distances.  511 / 512 / 513 candidates: the end of the select's walk one
# short of, at and one past two iterations of 256; 600: the tie class over three.  Seed 1 keeps no +0.0: its last eps is -0.0 itself
_ALL = frozenset({"negative", "-0", "+0"})
TIES_CASES = {(511, 255, 5): _ALL, (512, 256, 5): _ALL, (513, 257, 5): _ALL, (600, 300, 5): _ALL, (600, 300, 1): frozenset({"negative", "-0"})}


def ties_condition(P, A, seed):
    classes = TIES_CASES[(P, A, seed)]

    def condition(want):
        assert want["generations"] == TIES["max_gen"] and want["status"] == 0 and want["n_kept"] == A
        mixed = at_eps = 0
        for g, s in enumerate(want["selects"]):
            eq = np.flatnonzero(key(s["rho"]) == key(want["eps"][g]))
            kept_eq = np.intersect1d(eq, s["keep"])
            assert len(s["rho"]) == P and 1 <= len(kept_eq) < len(eq), (g, len(kept_eq), len(eq))      # the tie rule decides
            assert len(set(eq // 256)) >= 2 and len(set(eq % 256 // 64)) >= 2, g      # ... across iterations and waves of the select
            if g >= 1:
                mixed += (eq < s["nk_old"]).any() and (eq >= s["nk_old"]).any()
                at_eps += int((s["rho"][s["nk_old"]:] == want["eps"][g - 1]).sum())
        assert mixed >= 1 and at_eps >= 1, (mixed, at_eps)      # old and new tied at eps; new particles at the previous eps exactly
        assert zero_classes(want["value"]) == classes, zero_classes(want["value"])
        last = want["eps"][-1]
        assert last == 0.0 and bool(np.signbit(last)) == ("+0" not in classes)      # eps is a zero of the sign the total order puts last
    return condition


# ---- B. everything ties: the constant -------------------------------------------------------------------------------------------------------------
CONSTANT_CASE = dict(P=600, A=300, max_gen=3, p_acc_min=0.0, seed=5)


def constant_condition(want):
    assert want["status"] == 1 and want["generations"] == 1 and list(want["n_new_kept"]) == [300, 0, -1, -1]
    assert want["p_acc"][1] == 0.0 and (want["born"] == 0).all()
    assert all(list(s["keep"]) == list(range(300)) for s in want["selects"]) and len(want["selects"]) == 2      # the first 300 of the prior, in order
    assert (want["value"] == 0.0).all() and not np.signbit(want["value"]).any()


# ---- C. skewed weights: the bowl; quantiles at the CDF's own steps ---------------------------------------------------------------------------
SKEW = dict(P=200, A=100, max_gen=5, p_acc_min=0.0, scale=0.01, ridge=1e-6, seed=5)
SKEW_STEPS = 9      # kept rows, spread over the sorted order of parameter 0, at whose cumulative q the quantile is asked


def skew_condition(want):
    assert want["generations"] == SKEW["max_gen"] and want["n_kept"] == SKEW["A"]
    qs = [t["q"] for t in want["trace"][1:]] + [want["q"]]      # after generations 1 .. 5
    assert len(qs) == 5
    for q in qs:
        assert (q == 1).sum() >= 10 and q.max() == 2 ** 20 and q.min() == 1, ((q == 1).sum(), q.max())
    # the parents of generations 2 .. 5 come from such a prefix
    assert all(len(set(t["q"])) > 1 and "parent" in t for t in want["trace"][1:])


def skew_probs(want):
    """(probs, steps): for SKEW_STEPS kept rows spread over parameter 0's sorted order, c = the cumulative q up to and including the row:
    c / Q and its two neighbours; then 0 and 1.  steps: the three positions of each row's probs"""
    th, q = want["theta"][0], want["q"]
    order = np.argsort(key(th), kind="stable")
    cum = np.cumsum(q[order])
    Q = int(cum[-1])
    rows = np.unique(np.linspace(0, len(order) - 2, SKEW_STEPS).astype(int))      # (never the last row: its c / Q is 1.0)
    probs, steps = [], []
    for i in rows:
        p = float(cum[i]) / float(Q)
        steps.append(tuple(range(len(probs), len(probs) + 3)))
        probs += [math.nextafter(p, 0.0), p, math.nextafter(p, 1.0)]
    return tuple(probs) + (0.0, 1.0), steps


def skew_quantile_condition(steps):
    def condition(want):
        skew_condition(want)
        assert len(steps) >= 8
        quant = want["quantile"][:, 0]
        assert sum(len({quant[i] for i in st}) > 1 for st in steps) >= 1      # a step at which the neighbours answer with different rows
        assert quant[-2] == want["theta"][0].min() and quant[-1] == want["theta"][0].max()
    return condition


# the floor itself.  q = 1 above comes from ceil: smm_exp(lw - M) is tiny there, not 0.0.  At 64 parameters with scale = ridge = 1e-12 the factor's
# diagonal is about 1e-6, logc about 64 x 13, and a new particle's lw about -800 beside the prior particles' 0.0: smm_exp underflows to 0.0 (the
# smallest subnormal is exp(-745.2)), ceil gives 0 and only the floor makes q = 1.  D itself stays far above DBL_MIN (n_underflow == 0)
FLOOR = dict(npar=64, P=48, A=20, max_gen=2, p_acc_min=0.0, scale=1e-12, ridge=1e-12, seed=5, probs=(0.5,))


def floor_condition(want):
    assert want["generations"] == 2 and want["status"] == 0 and want["n_kept"] == 20 and (want["n_underflow"][:3] == 0).all()
    lw = want["logw"]
    under = lw - lw.max() < -750.0
    assert under.sum() >= 5 and (want["q"][under] == 1).all() and (want["q"][~under] == 2 ** 20).all() and (~under).sum() >= 2
    assert (want["born"][under] >= 1).all() and (want["n_new_kept"][1:] >= 5).all()
    t = want["trace"][1]      # generation 2's parents come from a prefix with floored entries
    assert (t["q"] == 1).sum() == want["n_new_kept"][1] and set(t["q"]) == {1, 2 ** 20} and (t["q"][t["parent"]] == 2 ** 20).all()


# ---- D. around the weight kernel's stride (serial_normal, ns = 20) ----------------------------------------------------------------------------
STRIDE = dict(max_gen=2, p_acc_min=0.0, scale=0.01, probs=(0.1, 0.9), seed=15)      # (of seeds 1 .. 39, 8 draw parent 1024 in generation 2)
STRIDE_A = (1023, 1024, 1025)
STRIDE_NEW = 300


def stride_condition(A):
    def condition(want):
        assert want["generations"] == 2 and want["n_kept"] == A and len(want["trace"]) == 2
        t = want["trace"][1]      # the kept set and the prefix entering generation 2
        assert len(t["q"]) == A and len(set(t["q"])) > 1 and (np.diff(t["prefix"]) == t["q"][:-1]).all()
        assert A != 1025 or (t["parent"] > 1023).any()
    return condition


# ---- E. the corners of the weight kernel's grid (serial_normal) ---------------------------------------------------------------------------------
CORNER = dict(A=257, n_new=272, max_gen=2, p_acc_min=0.0, scale=0.01, ns=40)
PASS2 = dict(A=16400, P=16700, max_gen=1, p_acc_min=0.0, scale=0.01, ns=20, probs=(0.5,))


def corner_condition(want):
    """a second block of T (blockIdx.y = 1) together with a second workgroup of new particles (blockIdx.x = 1)"""
    nf = new_finite(want)
    assert want["n_kept"] == 257 and len(nf) >= 1 and any(nk == 257 and n > 256 for nk, n in nf), nf


def pass2_condition(want):
    """the second pass's one block sum added onto the D of lanes beyond 255"""
    nf = new_finite(want)
    assert want["n_kept"] == 16400 and nf == [(16400, nf[0][1])] and nf[0][1] > 256, nf


# ---- F. empty and thin generations: the islands ------------------------------------------------------------------------------------------------
THIN_A = 40
# all outside: every point valid (hw 2.0), a kernel far wider than the box
OUTSIDE = dict(hw=2.0, P=64, A=24, max_gen=3, p_acc_min=0.0, scale=1e6, seeds=(1, 2, 3, 4, 5))
# name -> (hw, P, scale, seeds)
THIN_CASES = {"invalid_nk2": (0.002, 400, 400.0, (1, 4, 16)), "invalid_nk3or4": (0.004, 300, 100.0, (1, 4, 6, 7, 10)),
              "grows": (0.004, 300, 100.0, (12,)), "one": (0.002, 400, 400.0, (2, 9, 18)), "none": (0.002, 400, 400.0, (3, 11))}
THIN = dict(max_gen=2, p_acc_min=0.0, probs=(0.0, 0.5, 1.0))


def outside_condition(want):
    assert want["n_outside"][1] == 40 and want["status"] == 1 and want["generations"] == 1 and want["evaluated"] == 64
    assert want["n_invalid"][1] == 0 and want["n_new_kept"][1] == 0 and want["p_acc"][1] == 0.0 and want["n_kept"] == 24


def thin_condition(name):
    def invalid(want, lo, hi):
        t = want["trace"][0]
        n_inside = int(t["inside"].sum())
        assert lo <= len(t["wn"]) <= hi < THIN_A and want["n_new_kept"][0] == len(t["wn"])      # the kept set the generation started from
        assert n_inside > 0 and not np.isfinite(t["rho_new"]).any()
        assert want["n_invalid"][1] == n_inside and want["status"] == 1 and want["generations"] == 1 and want["n_kept"] == len(t["wn"])

    def grows(want):
        nk0 = want["n_new_kept"][0]
        assert 2 <= nk0 < want["n_kept"] < THIN_A and want["generations"] == 2 and (want["n_new_kept"][1:] > 0).all()
        assert [len(t["wn"]) for t in want["trace"]] == [nk0, nk0 + want["n_new_kept"][1]]      # nk grows twice: n_new = P - nk shrinks

    def one(want):
        assert want["status"] == 2 and want["n_kept"] == 1 and want["generations"] == 0 and want["weight"][0] == 1.0
        assert (want["cov"] == 0).all() and (want["quantile"] == want["theta"][0, 0]).all() and want["mean"][0] == want["theta"][0, 0]

    def none(want):
        assert want["status"] == 2 and want["n_kept"] == 0 and want["generations"] == 0 and want["n_invalid"][0] == want["evaluated"]
        assert np.isnan(want["theta"]).all() and np.isnan(want["quantile"]).all()
    return {"invalid_nk2": lambda w: invalid(w, 2, 2), "invalid_nk3or4": lambda w: invalid(w, 3, 4), "grows": grows, "one": one, "none": none}[name]
