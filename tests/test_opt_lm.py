"""smm_opt_lm (include/smmhip.h), CPU tier: the contract's restatement (tests/lm_ref.py) against the closed-form least-squares solution of a
linear residual and against scipy's bounded least squares on a smooth one, before the device is compared with it bit for bit
(tests/test_gpu_opt_lm.py); every status and branch of the contract on crafted inputs, asserted on the restatement's own counters; the
independence of the searches; the ABI."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import common as cm  # noqa: E402,F401  (path set-up)
import lm_ref as lmr  # noqa: E402

import smm_jl_amd as S  # noqa: E402
from smm_jl_amd import _abi as A  # noqa: E402


def model(sim, mom, w):
    """an evaluator over P [np][n] from sim(P) -> [nm][n]: value = F / nm, as objfunc_norm and the dense objectives report it"""
    s = lmr.scales(w)

    def evaluator(P):
        P = np.asarray(P, float)
        with np.errstate(all="ignore"):
            sm = sim(P)
            r = (sm - np.asarray(mom, float)[:, None]) / s[:, None]
            return (r * r).sum(0) / len(mom), sm, np.ones(P.shape[1], np.int8)
    return evaluator


# ---- 1. a linear residual: the closed form ------------------------------------------------------------------------------------------------
def linear_case(seed):
    """nm = 7 moments linear in np = 5 parameters, weights that exercise the rule s_j (0 and inf count as 1), a box far from the solution"""
    rng = np.random.default_rng(seed)
    M, c, mom = rng.normal(size=(7, 5)), rng.normal(size=7), rng.normal(size=7)
    w = np.array([1.0, 2.0, 0.5, 0.0, np.inf, 3.0, 1.5])
    return M, c, mom, w, np.full(5, -50.0), np.full(5, 50.0), np.random.default_rng(100 + seed).uniform(-5, 5, (5, 12))


LINEAR_BOUND = 4.5e-7


def test_a_linear_residual_ends_at_the_closed_form_solution():
    """Five linear problems, twelve starts each, xtol = ftol = 0: a search ends when no try descends any more (status 3), after 4 .. 9
    iterations.  Against np.linalg.lstsq on (M / s) theta = (mom - c) / s.  The largest distance of an end point from the closed form
    measured over the 60 searches was 4.5e-8 (by case: 4.5e-8, 3.3e-9, 7.6e-10, 6.0e-10, 2.5e-9).  That is what a test on F can give: the
    minimum has a residual, F = O(1) there is quadratic in the distance, and a try is accepted only while F_new < F in doubles — an ulp
    of F, 1e-16 or so, is a distance of 1e-8 or so.  The bound is ten times the largest distance seen: 4.5e-7."""
    worst = 0.0
    for seed in range(5):
        M, c, mom, w, lb, ub, st = linear_case(seed)
        s = lmr.scales(w)
        assert list(s) == [1.0, 2.0, 0.5, 1.0, 1.0, 3.0, 1.5]
        out = lmr.opt_lm(model(lambda P: M @ P + c[:, None], mom, w), st, lb, ub, mom, w, fd_step=1e-6, xtol=0.0, ftol=0.0)
        sol = np.linalg.lstsq(M / s[:, None], (mom - c) / s, rcond=None)[0]
        d = float(np.abs(out["best"] - sol[:, None]).max())
        print("linear case %d: largest distance from the closed form %.3g; status %s; iterations %d .. %d"
              % (seed, d, sorted(set(out["status"])), out["iterations"].min(), out["iterations"].max()))
        worst = max(worst, d)
        assert set(out["status"]) <= {1, 3} and (out["iterations"] < 100).all() and out["active"].sum() == 0
        r = (M @ out["best"] + c[:, None] - mom[:, None]) / s[:, None]
        assert np.allclose(out["ssr"], (r * r).sum(0), rtol=1e-13) and np.allclose(out["value"], out["ssr"] / 7, rtol=1e-13)
    print("linear: largest distance %.3g, bound %.3g" % (worst, LINEAR_BOUND))
    assert worst <= LINEAR_BOUND


# ---- 2. a smooth bounded residual: scipy's least_squares ------------------------------------------------------------------------------------
def tanh_case():
    """a dense tanh model, np = 5, nm = 7, box [-2, 2]^5; the moments come from a point whose first coordinate is 2.5: outside the box"""
    rng = np.random.default_rng(5)
    W, b = rng.normal(size=(7, 5)) * 0.5, rng.normal(size=7) * 0.3
    tstar = rng.uniform(-1.5, 1.5, 5)
    tstar[0] = 2.5
    return W, b, np.tanh(W @ tstar + b), np.ones(7), np.full(5, -2.0), np.full(5, 2.0), np.random.default_rng(6).uniform(-2, 2, (5, 40))


TANH_BOUND = 2.51e-5


@pytest.fixture(scope="module")
def tanh_run():
    W, b, mom, w, lb, ub, st = tanh_case()
    return lmr.opt_lm(model(lambda P: np.tanh(W @ P + b[:, None]), mom, w), st, lb, ub, mom, w, fd_step=1e-6, xtol=1e-14, ftol=1e-14)


def test_a_smooth_bounded_residual_ends_where_scipys_least_squares_ends(tanh_run):
    """40 random starts, fd_step = 1e-6 of a range of 4, tolerances of 1e-14 on both sides; scipy.optimize.least_squares (trf, bounds, the
    analytic Jacobian) from the same starts.  The constrained minimum has a residual (F = 0.0191), so the forward difference's bias in J
    moves the minimiser by the order of h = 4e-6: the largest distance measured between an end point and scipy's was 2.51e-6 (scipy's own
    40 end points agree to 4.2e-8), every search ending in 15 .. 22 iterations and 102 .. 150 evaluations at the upper bound of the first
    parameter, with status 3: no try descends any more.  The bound is ten times the measurement — the margin is for other starts —:
    2.51e-5."""
    so = pytest.importorskip("scipy.optimize", reason="scipy is the reference this restatement is compared with")
    W, b, mom, w, lb, ub, st = tanh_case()
    out = tanh_run
    fun = lambda t: np.tanh(W @ t + b) - mom                               # noqa: E731
    jac = lambda t: (1.0 - np.tanh(W @ t + b) ** 2)[:, None] * W           # noqa: E731
    ref = np.array([so.least_squares(fun, st[:, q], jac=jac, bounds=(lb, ub), xtol=1e-14, ftol=1e-14, gtol=1e-14).x for q in range(40)]).T
    d = np.abs(out["best"] - ref).max(0)
    print("tanh: largest distance from scipy %.3g (bound %.3g); scipy's own spread %.3g; iterations %d .. %d, evaluations %d .. %d, status %s"
          % (d.max(), TANH_BOUND, np.abs(ref - ref[:, :1]).max(), out["iterations"].min(), out["iterations"].max(), out["n_eval"].min(),
             out["n_eval"].max(), sorted(set(out["status"]))))
    assert d.max() <= TANH_BOUND
    assert (out["best"][0] == 2.0).all() and (out["active"][0] == 1).all() and out["active"][1:].sum() == 0 and (out["grad"][0] < 0).all()
    assert set(out["status"]) <= {1, 3} and (out["iterations"] <= 30).all() and (out["n_eval"] <= 200).all()
    assert np.array_equal(out["n_eval"], 1 + 5 * out["iterations"] + out["tries"] - out["pivot"]) and out["evaluated"] == out["n_eval"].sum()


# ---- 3. every status and branch -----------------------------------------------------------------------------------------------------------
def rosenbrock(P):
    return np.stack([10.0 * (P[1] - P[0] * P[0]), 1.0 - P[0]])


def test_every_status_and_branch_is_reached(tanh_run):
    W, b, mom, w, lb, ub, st = tanh_case()
    ev = model(lambda P: np.tanh(W @ P + b[:, None]), mom, w)
    # status 0: the iteration cap, after exactly max_iter Jacobians with the last try accepted
    out = lmr.opt_lm(ev, st[:, :4], lb, ub, mom, w, fd_step=1e-6, xtol=0.0, ftol=0.0, max_iter=2)
    assert (out["status"] == 0).all() and (out["iterations"] == 2).all() and (out["step"] > 0).all() and (out["dF"] > 0).all()
    # status 1 by the step's tolerances, and by the gradient's alone
    out = lmr.opt_lm(ev, st[:, :4], lb, ub, mom, w, fd_step=1e-6, xtol=1e-4, ftol=0.0)
    assert (out["status"] == 1).all() and (out["step"] <= 1e-4).all() and (out["step"] > 0).all()
    out = lmr.opt_lm(ev, st[:, :4], lb, ub, mom, w, fd_step=1e-6, xtol=0.0, ftol=1e-8)
    assert (out["status"] == 1).all() and (out["dF"] <= 1e-8 * out["ssr"]).all() and (out["step"] > 1e-6).all()
    loose = lmr.opt_lm(ev, st[:, :4], lb, ub, mom, w, fd_step=1e-6, xtol=0.0, ftol=0.0, gtol=1e-3)
    assert (loose["status"] == 1).all() and (np.abs(loose["grad"][1:]) <= 1e-3).all() and (loose["iterations"] < tanh_run["iterations"][:4]).all()
    # an active bound, met at x == ub with g < 0; a start on ub: a backward difference
    assert (tanh_run["met_active"] > 0).all() and (tanh_run["backward"] > 0).all()
    at_ub = lmr.opt_lm(ev, ub[:, None].copy(), lb, ub, mom, w, fd_step=1e-6, max_iter=1)
    assert at_ub["backward"][0] == 5 and np.isfinite(at_ub["jac"]).all()
    # status 3: no try descends (a minimum to the last bit); a rejected try was evaluated
    assert (tanh_run["status"] == 3).any() and (tanh_run["rejected"][tanh_run["status"] == 3] >= 12).all()
    # a rejected try that is no stop: from (-1.2, 1) the undamped step of the banana's residuals overshoots
    rb = lmr.opt_lm(model(rosenbrock, [0.0, 0.0], [1.0, 1.0]), [[-1.2], [1.0]], [-3.0, -3.0], [3.0, 3.0], [0.0, 0.0], [1.0, 1.0], fd_step=1e-7,
                    lambda0=1e-10)
    assert rb["rejected"][0] >= 1 and rb["status"][0] in (1, 3) and np.abs(rb["best"][:, 0] - 1.0).max() < 1e-5 and rb["ssr"][0] < 1e-10
    # status 2 at the start, and at a Jacobian point: moments that are NaN where theta_0 > 2 or theta_1 < -1
    holes = model(lambda P: np.where((P[0] > 2.0) | (P[1] < -1.0), np.nan, rosenbrock(P)), [0.0, 0.0], [1.0, 1.0])
    h2 = lmr.opt_lm(holes, [[2.5, 2.0, -1.2], [0.0, 0.0, 1.0]], [-3.0, -3.0], [3.0, 3.0], [0.0, 0.0], [1.0, 1.0], fd_step=1e-7, lambda0=1e-10)
    assert list(h2["status"][:2]) == [2, 2] and list(h2["iterations"][:2]) == [0, 1] and list(h2["n_eval"][:2]) == [1, 3]
    assert np.isnan(h2["jac"][:, :, 0]).all() and np.isnan(h2["jac"][:, 0, 1]).all() and np.isfinite(h2["jac"][:, 1, 1]).all()
    assert np.isnan(h2["grad"][:, :2]).all() and np.array_equal(h2["best"][:, :2], [[2.5, 2.0], [0.0, 0.0]])
    # ... and a NaN band met by a try is a rejected try, not a stop: the third search's undamped first step lands at theta_1 = -3
    assert h2["status"][2] in (1, 3) and h2["rejected"][2] >= 1 and np.abs(h2["best"][:, 2] - 1.0).max() < 1e-5
    # status 4: a parameter that moves no moment (here the second), at the first Jacobian — before the gradient is looked at
    flat = lmr.opt_lm(model(lambda P: np.stack([P[0], 2.0 * P[0]]), [0.5, 1.0], [1.0, 1.0]), [[0.0, 0.5], [0.3, 0.3]], [-1.0, -1.0], [1.0, 1.0],
                      [0.5, 1.0], [1.0, 1.0])
    assert (flat["status"] == 4).all() and (flat["iterations"] == 1).all() and (flat["n_eval"] == 3).all() and (flat["tries"] == 0).all()
    assert (flat["grad"][1] == 0.0).all() and (flat["jac"][:, 1] == 0.0).all() and flat["grad"][0, 1] == 0.0      # (search 1 sits at the minimum: 4, not 1)
    # a pivot that is not > 0: one moment, two parameters, J = [1, 1] exactly (h = 2^-8), so B = A = [[1, 1], [1, 1]] until 1 + lambda > 1;
    # from lambda0 = 1e-20 that takes five tries, which cost no evaluation
    one = model(lambda P: (P[0] + P[1])[None, :], [0.25], [1.0])
    pv = lmr.opt_lm(one, [[0.5], [-0.75]], [-2.0, -2.0], [2.0, 2.0], [0.25], [1.0], fd_step=2.0 ** -10, lambda0=1e-20, max_iter=1)
    assert pv["jac"].tolist() == [[[1.0], [1.0]]] and pv["pivot"][0] == 5 and pv["tries"][0] == 6 and pv["n_eval"][0] == 1 + 2 + 1
    lam = 1e-20
    for _ in range(5):
        lam = lam * 10.0
    assert pv["status"][0] in (0, 1) and pv["ssr"][0] < 1e-20 and pv["lambda"][0] == lam / 10.0
    # ... and a search whose tries all fail at the pivot stops with status 3 and has evaluated the start and the Jacobian only
    pv3 = lmr.opt_lm(one, [[0.5], [-0.75]], [-2.0, -2.0], [2.0, 2.0], [0.25], [1.0], fd_step=2.0 ** -10, lambda0=1e-20, max_tries=4)
    assert pv3["status"][0] == 3 and pv3["pivot"][0] == 4 and pv3["n_eval"][0] == 3 and np.isnan(pv3["step"][0])
    # lambda that is no longer finite: status 3 before the tries are used up
    big = lmr.opt_lm(one, [[0.5], [-0.75]], [-2.0, -2.0], [2.0, 2.0], [0.25], [1.0], fd_step=2.0 ** -10, lambda0=1e-20, lambda_up=1e200, max_tries=9)
    assert big["status"][0] in (0, 1, 3) and big["tries"][0] <= 2


def test_the_searches_are_independent(tanh_run):
    """any subset of the starts, in any order, gives the same columns"""
    W, b, mom, w, lb, ub, st = tanh_case()
    pick = [31, 2, 17]
    sub = lmr.opt_lm(model(lambda P: np.tanh(W @ P + b[:, None]), mom, w), st[:, pick], lb, ub, mom, w, fd_step=1e-6, xtol=1e-14, ftol=1e-14)
    lmr.assert_equal(sub, {f: tanh_run[f][..., pick] for f in lmr.FIELDS} | {"evaluated": int(tanh_run["n_eval"][pick].sum())})


# ---- 4. the ABI ------------------------------------------------------------------------------------------------------------------------
def test_struct_layout_and_symbol():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "smmhip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(smm_opt_lm_t), offsetof(smm_opt_lm_t, jac), offsetof(smm_opt_lm_t, lambda),
         offsetof(smm_opt_lm_t, active), offsetof(smm_opt_lm_t, status), offsetof(smm_opt_lm_t, evaluated));
  return 0; }
'''
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), os.path.join(d, "p.c"), "-o", os.path.join(d, "p")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "p")]).split()]
    T = A.smm_opt_lm_t
    assert got == [C.sizeof(T), T.jac.offset, getattr(T, "lambda").offset, T.active.offset, T.status.offset, T.evaluated.offset]
    assert [f for f, _ in T._fields_][:-1] == list(lmr.FIELDS)
    assert hasattr(A.load(), "smm_opt_lm") and hasattr(A.load_hooks(), "smm_opt_lm")
    assert callable(S.optLMDevice) and callable(S.BGPContext.opt_lm)
