"""smm_abc_pmc (include/smmhip.h), CPU tier: the contract's restatement (tests/pmc_ref.py) held against what it restates before the device is
compared with it (tests/test_gpu_abc_pmc.py): the log-weights against a direct evaluation of the mixture through np.linalg.solve, the
blocked sum T against a scalar loop, eps, the integer CDF of the parents, the box's edges, the select's ties, every status; the ABI and the
host binding."""
import ctypes as C
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import common as cm  # noqa: E402,F401  (path set-up)
import pmc_ref as R  # noqa: E402

import smm_jl_amd as S  # noqa: E402
from smm_jl_amd import _abi as A  # noqa: E402
from oracle import oracle as O  # noqa: E402

INF, NAN = float("inf"), float("nan")


def bowl(centre, width):
    """value = sum ((theta - centre) / width)^2; moments: theta itself"""
    centre, width = np.asarray(centre, float)[:, None], np.asarray(width, float)[:, None]

    def f(P):
        P = np.asarray(P, float)
        return (((P - centre) / width) ** 2).sum(0), P.copy(), np.ones(P.shape[1], np.int8)
    return f


def holes(P):
    """tests/test_gpu_opt_simplex.py's objective with holes: +inf on a band of x, NaN on a band of y, nothing finite for x > 1.5, status -2
    left of x = -1.5"""
    x, y = np.asarray(P, float)
    ay = np.abs(y + 0.4)
    v = (x - 0.3) ** 2 + np.where(ay < 0.25, 0.0, ay - 0.25)
    v = np.where((x > -1.2) & (x < -0.9), INF, v)
    v = np.where((y > 0.9) & (y < 1.3), NAN, v)
    v = np.where(x > 1.5, np.where(y > 0.0, NAN, INF), v)
    return v, np.stack([x + y, x * y - 0.5]), np.where(x < -1.5, -2, 1).astype(np.int8)


LB2, UB2 = [-2.0, -2.0], [2.0, 2.0]


def run(f, npar=2, P=96, A=48, max_gen=4, seed=5, lb=None, ub=None, **kw):
    lb = [-2.0] * npar if lb is None else lb
    ub = [2.0] * npar if ub is None else ub
    return R.abc_pmc(O, f, seed, lb, ub, npar, P, A, max_gen, **kw)


# ---- 1. the weights are the mixture's ---------------------------------------------------------------------------------------------------------
def direct_logw(u, kept_u, wn, Sigma):
    """-log sum_i wn_i N(u; u_i, Sigma), the covariance applied through np.linalg.solve"""
    npar = len(u)
    d = u[:, None] - kept_u
    m = np.einsum("ki,ki->i", d, np.linalg.solve(Sigma, d))
    dens = np.exp(-0.5 * m) / math.sqrt((2.0 * math.pi) ** npar * np.linalg.det(Sigma))
    return -math.log(math.fsum(wn * dens))


def check_weights(r, min_checked):
    checked = 0
    for t in r["trace"]:
        if "lw_new" not in t:
            continue
        assert np.linalg.cond(t["Sigma"]) <= 1e3      # (on the restatement alone: rounding then stays orders below 1e-9)
        for j in np.flatnonzero(np.isfinite(t["rho_new"])):
            want = direct_logw(t["u_new"][:, j], t["kept_u"], t["wn"], t["Sigma"])
            assert abs(t["lw_new"][j] - want) <= 1e-9 * abs(want), (j, t["lw_new"][j], want)
            checked += 1
    assert checked >= min_checked


def test_the_log_weights_are_the_mixture_density():
    check_weights(run(bowl([0.3, -0.4], [1.0, 1.5]), max_gen=4), 60)
    # correlated: a valley along the diagonal, np = 3
    def valley(P):
        x, y, z = np.asarray(P, float)
        return (x - y) ** 2 * 4.0 + (x + y) ** 2 * 0.25 + z * z, np.stack([x, y, z]), np.ones(P.shape[1], np.int8)
    check_weights(run(valley, npar=3, P=120, A=60, max_gen=3), 60)


def test_T_adds_blocks_of_256_from_zero_left_to_right():
    rng = np.random.default_rng(1)
    zk, zn, wn = rng.normal(size=(2, 600)), rng.normal(size=(2, 3)), rng.uniform(0.5, 1.5, 600) / 600
    D = R.mixture(O, zn, zk, wn)
    exp = lambda x: float(O.contract_math("exp", np.array([x]))[0])      # noqa: E731
    for j in range(3):
        blocks = []
        for b0 in range(0, 600, 256):
            s = 0.0
            for i in range(b0, min(b0 + 256, 600)):
                d2 = (zn[0, j] - zk[0, i]) ** 2
                d2 = d2 + (zn[1, j] - zk[1, i]) ** 2
                s = s + wn[i] * exp(-0.5 * d2)
            blocks.append(s)
        want = 0.0
        for s in blocks:
            want = want + s
        assert D[j] == want and len(blocks) == 3
        assert abs(D[j] - math.fsum(wn * np.exp(-0.5 * ((zn[:, j:j + 1] - zk) ** 2).sum(0)))) <= 1e-13 * D[j]


# ---- 2. the loop -----------------------------------------------------------------------------------------------------------------------------
def test_eps_never_increases_and_the_kept_are_the_best_of_a_superset():
    r = run(bowl([0.3, -0.4], [1.0, 1.5]), max_gen=6, p_acc_min=0.0)
    g = r["generations"]
    assert g == 6 and r["status"] == 0
    assert (np.diff(r["eps"][:g + 1]) <= 0).all() and r["eps"][g] < 0.2 * r["eps"][0]
    assert r["value"].max() == r["eps"][g] and r["n_kept"] == 48 and (r["born"] <= g).all() and (r["born"] >= 0).all()
    assert np.isnan(r["p_acc"][0]) and ((r["p_acc"][1:g + 1] > 0) & (r["p_acc"][1:g + 1] <= 1)).all()
    assert r["evaluated"] == 96 + int((48 - r["n_outside"][1:g + 1]).sum())
    assert abs(r["weight"].sum() - 1.0) < 1e-12 and 1.0 < r["ess"] <= 48.0 and r["ess"] == r["gen_ess"][g]
    assert abs(r["mean"][0] - 0.3) < 0.3 and abs(r["mean"][1] + 0.4) < 0.45      # (the posterior sits on the bowl's centre)


def test_the_parents_follow_the_integer_cdf():
    r = run(bowl([0.3, -0.4], [1.0, 1.5]), max_gen=5, p_acc_min=0.0)
    seen = 0
    for t in r["trace"]:
        if "parent" not in t:
            continue
        q, prefix, Q = t["q"], t["prefix"], t["Q"]
        assert prefix[0] == 0 and (np.diff(prefix) == q[:-1]).all() and prefix[-1] + q[-1] == Q and (q >= 1).all() and q.max() == 2 ** 20
        for v, rr, p in zip(t["v"], t["r"], t["parent"]):
            assert rr == min(int(v * float(Q)), Q - 1) and prefix[p] <= rr < prefix[p] + q[p]
        seen += len(t["parent"])
    assert seen == 5 * 48
    # the ends of the CDF: r = 0 is the first kept particle, r = Q - 1 the last
    prefix = np.array([0, 3, 4, 10], np.int64)
    assert list(np.searchsorted(prefix, np.array([0, 2, 3, 4, 9, 10, 14]), side="right") - 1) == [0, 0, 1, 2, 2, 3, 3]


def test_inside_is_decided_at_exactly_zero_and_one():
    up, down = math.nextafter(1.0, 2.0), math.nextafter(0.0, -1.0)
    u = np.array([[0.0, 1.0, -0.0, up, down, NAN, 0.5, 0.5], [0.5, 0.5, 1.0, 0.5, 0.5, 0.5, up, 1.0]])
    assert list(R.inside_box(u)) == [True, True, True, False, False, False, False, True]
    # in a run: a narrow box around a wide kernel throws particles out; they are not evaluated, never kept, and counted
    calls = []
    f = bowl([0.0, 0.0], [1.0, 1.0])

    def counting(P):
        calls.append(P.shape[1])
        return f(P)
    r = run(counting, max_gen=3, scale=8.0, p_acc_min=0.0)
    assert r["n_outside"][0] == 0 and r["n_outside"][1:].sum() > 0
    assert calls == [96] + [48 - int(n) for n in r["n_outside"][1:]] and r["evaluated"] == sum(calls)
    for t in r["trace"]:
        if "inside" in t:
            assert np.isinf(t["rho_new"][~t["inside"]]).all() and (t["lw_new"][~t["inside"]] == 0).all()
    assert ((r["theta"] >= -2.0) & (r["theta"] <= 2.0)).all()


def test_the_select_keeps_the_smallest_and_the_earlier_of_equals():
    rho = np.array([3.0, 1.0, INF, 1.0, 2.0, 1.0, 0.5, INF, 2.0])
    assert list(R.select(rho, 3)) == [1, 3, 6]                  # 0.5, then the first two of the three 1.0
    assert list(R.select(rho, 4)) == [1, 3, 5, 6]
    assert list(R.select(rho, 6)) == [1, 3, 4, 5, 6, 8]          # both 2.0, in candidate order
    assert list(R.select(rho, 8)) == [0, 1, 3, 4, 5, 6, 8]       # A' = 7 < A: +inf is never kept
    assert list(R.select(np.array([INF, INF]), 2)) == []
    assert list(R.select(np.array([0.0, -0.0, 0.0]), 1)) == [1]  # the IEEE total order: -0.0 before +0.0
    assert list(R.select(np.array([-1.0, -3.0, 2.0]), 2)) == [0, 1]
    rho2, bad = R.distance([1.0, NAN, INF, -INF, 2.0, 3.0], [1, 1, 1, 1, -2, 0])
    assert list(rho2) == [1.0, INF, INF, INF, INF, INF] and list(bad) == [False, True, True, True, True, True]


def test_holes_are_never_kept():
    r0 = run(holes, max_gen=0, P=128, A=100, seed=9)
    n = r0["n_kept"]
    assert r0["n_invalid"][0] > 28 and n == 128 - r0["n_invalid"][0] == r0["n_new_kept"][0]      # A' < A: fewer than A finite candidates
    assert np.isfinite(r0["value"][:n]).all() and np.isnan(r0["value"][n:]).all() and (r0["born"][n:] == -1).all()
    assert np.isnan(r0["theta"][:, n:]).all() and np.isnan(r0["weight"][n:]).all() and np.isnan(r0["sim_moments"][:, n:]).all()
    r = run(holes, max_gen=4, p_acc_min=0.0, P=128, A=100, seed=9)
    n = r["n_kept"]
    assert r["status"] == 0 and r["n_invalid"][1:].sum() > 0 and np.isfinite(r["value"][:n]).all()
    th = r["theta"][:, :n]
    assert (th[0] >= -1.5).all() and not ((th[0] > -1.2) & (th[0] < -0.9)).any() and not ((th[1] > 0.9) & (th[1] < 1.3)).any() and (th[0] <= 1.5).all()


# ---- 3. every status ---------------------------------------------------------------------------------------------------------------------------
def test_every_status_is_reached():
    f = bowl([0.3, -0.4], [1.0, 1.5])
    r0 = run(f, max_gen=0)
    assert r0["status"] == 0 and r0["generations"] == 0 and r0["evaluated"] == 96 and (r0["born"] == 0).all() and (r0["logw"] == 0).all()
    assert (r0["weight"] == 1.0 / 48).all() and r0["ess"] == 48.0 and r0["trace"] == []      # the prior's best A, equally weighted
    assert run(f, max_gen=3, p_acc_min=0.0)["status"] == 0
    r1 = run(f, max_gen=5, p_acc_min=0.99)
    assert r1["status"] == 1 and r1["generations"] == 1 and r1["p_acc"][1] <= 0.99 and np.isnan(r1["eps"][2]) and r1["n_outside"][2] == -1
    nothing = lambda P: (np.full(P.shape[1], INF), np.zeros((2, P.shape[1])), np.ones(P.shape[1], np.int8))      # noqa: E731
    r2 = run(nothing, max_gen=3)
    assert r2["status"] == 2 and r2["n_kept"] == 0 and r2["generations"] == 0 and np.isnan(r2["mean"]).all() and np.isnan(r2["ess"])
    assert r2["n_invalid"][0] == 96 and np.isnan(r2["eps"][0])
    one = lambda P: (np.where(np.arange(P.shape[1]) == 17, 1.0, NAN), np.zeros((2, P.shape[1])), np.ones(P.shape[1], np.int8))      # noqa: E731
    r2 = run(one, max_gen=3, probs=(0.5,))
    assert r2["status"] == 2 and r2["n_kept"] == 1 and r2["weight"][0] == 1.0 and (r2["cov"] == 0).all() and r2["eps"][0] == 1.0
    assert (r2["quantile"][0] == r2["theta"][:, 0]).all() and (r2["mean"] == r2["theta"][:, 0]).all()


def test_two_particles_in_three_dimensions_are_not_positive_definite():
    """A = 2, np = 3, ridge = 0: the covariance of two points has rank one"""
    f3 = bowl([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])
    st = [run(f3, npar=3, P=24, A=2, max_gen=3, seed=s)["status"] for s in range(1, 9)]
    assert 3 in st, st
    r = run(f3, npar=3, P=24, A=2, max_gen=3, seed=1 + st.index(3))
    assert r["generations"] == 0 and r["n_kept"] == 2 and not r["trace"][-1]["ok"] and np.isfinite(r["mean"]).all()
    assert run(f3, npar=3, P=24, A=2, max_gen=3, seed=1 + st.index(3), ridge=1e-3)["status"] != 3      # (a ridge repairs it)


# ---- 4. the ABI and the host binding ----------------------------------------------------------------------------------------------------------------
def test_the_struct_and_the_prototype_are_the_headers():
    names = [f[0] for f in A.smm_abc_pmc_t._fields_]
    assert names == ["theta", "value", "sim_moments", "weight", "logw", "born", "eps", "p_acc", "gen_ess", "n_outside", "n_invalid", "n_underflow",
                     "n_new_kept", "mean", "cov", "quantile", "ess", "n_kept", "generations", "status", "reserved", "evaluated"]
    assert C.sizeof(A.smm_abc_pmc_t) == 16 * 8 + 8 + 4 * 4 + 8
    sym = dict((s[0], s) for s in A.SYMBOLS)["smm_abc_pmc"]
    assert sym[1] is C.c_int and len(sym[2]) == 10 and sym[2][4] is C.c_double and sym[2][8] is C.c_int32
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "smmhip.h")).read()
    body = header[header.index("smm_opt_simplex_t;"):header.index("} smm_abc_pmc_t;")]
    body = body[body.rindex("typedef struct"):]
    declared = [line.split(";")[0].split()[-1] for line in body.splitlines()[1:] if ";" in line]
    assert declared == names
    assert "STREAM_PMC = 8" in open(os.path.join(os.path.dirname(A.__file__), "csrc", "smm_rng.hpp")).read()
    assert hasattr(A.load(), "smm_abc_pmc") and hasattr(S.BGPContext, "abc_pmc") and callable(S.abc_pmc)


def test_the_result_object():
    raw = run(bowl([0.3, -0.4], [1.0, 1.5]), max_gen=2, probs=(0.1, 0.9))
    res = S.ABCPMCResult(["p1", "p2"], raw)
    assert list(res.mean()) == ["p1", "p2"] and res.mean()["p2"] == raw["mean"][1] and res.cov().shape == (2, 2)
    assert res.quantile()["p1"] == list(raw["quantile"][:, 0]) and len(res.eps) == 3 and res.status == 0
    th, w = res.draws()
    assert th.shape == (2, 48) and w.shape == (48,) and not np.isnan(th).any()
