"""smm_opt_lm on the device (include/smmhip.h; smm.jl_amd/csrc/smm_optlm.hpp, smm_optlm_host.hpp) against the contract's restatement
(tests/lm_ref.py, compared with the closed form and with scipy in tests/test_opt_lm.py): every output field bit for bit.  The restatement
evaluates the built-in objectives through the oracle's eval_batch and user objectives through the context's own eval_batch — neither is new
code.  Shapes are the smallest that can still go wrong: K no multiple of the evaluation tile (8 chains; 16 for the dense objective), more
moments than parameters and fewer, 50 of a wave's 64 lanes and all 64 with a 64-row factor, searches that stop at different iterations and
tries (the lists are compacted), batches of 2 searches and, once, more searches than one pass of the list compaction (1024)."""
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import common as cm  # noqa: E402
import lm_ref as lmr  # noqa: E402
from moment_stats_ref import dense_problem  # noqa: E402

from smm_jl_amd.workloads import build_problem  # noqa: E402

pytestmark = pytest.mark.gpu
_user = {}

# tests/test_gpu_opt_simplex.py's objectives with holes, both forms, in this test's own copy: the search reads the moments, not the value, so
# where the value is not finite — +inf on a band of x, NaN on a band of y, one or the other for x > 1.5 — the first moment takes it; the
# status says "failed" left of x = -1.5 although the moments are fine there: the search does not consult it
HOLES_BODY = r"""
    const double x = theta[0], y = theta[1];
    const double ay = __builtin_fabs(y + 0.4);
    double v = (x - 0.3) * (x - 0.3) + (ay < 0.25 ? 0.0 : ay - 0.25);
    if (x > -1.2 && x < -0.9) v = __builtin_inf();
    if (y > 0.9 && y < 1.3) v = __builtin_nan("");
    if (x > 1.5) v = y > 0.0 ? __builtin_nan("") : __builtin_inf();
    if (!(v - v == 0.0)) sim_moments[0] = v;
    *value = v;
    *status = x < -1.5 ? -2 : 1;
}
"""
HOLES_SOURCE = r"""
SMM_USER_OBJECTIVE(const double* theta, int np, const double* mom, const double* w, int nm,
                   const double* udata, int n_udata, double* sim_moments, double* value, int* status)
{
    sim_moments[0] = theta[0] + theta[1];
    sim_moments[1] = theta[0] * theta[1] - mom[1];
""" + HOLES_BODY
HOLES_LANES_SOURCE = r"""
SMM_USER_PARTIAL(const double* theta, int np, const double* udata, int n_udata, int lane, int n_lanes, double* partial)
{
    const int A = (int)udata[0];
    for (int a = lane; a < A; a += n_lanes) { partial[0] += theta[0] * (double)(a % 3); partial[1] += theta[1] + 0.25 * (double)(a % 5); }
}

SMM_USER_FINISH(const double* theta, int np, const double* totals, int n_sums, const double* mom, const double* w, int nm,
                const double* udata, int n_udata, double* sim_moments, double* value, int* status)
{
    sim_moments[0] = totals[0] / udata[0];
    sim_moments[1] = totals[1] / udata[0] - mom[1];
""" + HOLES_BODY


def registered(S, name, register):
    key = (name, id(S._abi.load()))      # (a handle belongs to the library that compiled it: the shipped one, or the test build under `hooks`)
    if key not in _user:
        _user[key] = register()
    return _user[key]


def holes_problem(S, form):
    oid = registered(S, "lm_" + form, lambda: S.register_user_objective(HOLES_SOURCE) if form == "one_thread"
                     else S.register_user_objective(HOLES_LANES_SOURCE, n_sums=2, lanes=128))
    # (the map-reduce form's moments are linear in theta: with the first one's target inside the +inf band of x every search walks into it)
    mom = [0.0, 0.5] if form == "one_thread" else [-1.05, 0.5]
    prob = S.Problem(init=[0.0, 0.0], lb=[-2.0, -2.0], ub=[2.0, 2.0], mom=mom, w=[1.0, 2.0], ns=1, objective_id=oid, obj_params=[700.0])
    opts = S.BGPOpts(N=5, maxiter=4, sigma=0.05 * cm.temps(5, 4.0), acc_tuner=np.geomspace(3.0, 0.5, 5), min_improve=np.zeros(5), seed=9)
    return prob, opts


def holes_starts():
    rng = np.random.default_rng(3)
    st = rng.uniform(-2, 1.4, (2, 11))
    st[:, 0] = [0.3, -0.4]
    st[:, 1] = [1.9, 1.0]       # not finite at the start: NaN
    st[:, 2] = [0.0, 1.1]       # in the NaN band of y
    st[:, 3] = [-1.9, -2.0]     # status -2 at perfectly good moments
    st[:, 4] = [-1.0, 0.0]      # in the +inf band of x: not finite at the start either
    st[:, 5] = [-0.7, 0.5]      # next to the +inf band
    st[:, 6] = [-1.4, -1.0]     # ... and on its other side
    return st


def box_starts(prob, K, seed):
    rng = np.random.default_rng(seed)
    st = rng.uniform(prob.lb[:, None], prob.ub[:, None], (prob.np, K))
    st[:, 0], st[:, K - 1] = prob.lb, prob.ub      # the bounds themselves are inside (at ub every difference is backward)
    return st


def oracle_evaluator(S, O, prob, opts, h):
    o = O.OracleContext(prob, opts, S.Tables(Z=h.Z()), threads=O.max_threads())
    return o.eval_batch


def compare(h, evaluator, prob, starts, condition=None, **kw):
    want = lmr.opt_lm(evaluator, starts, prob.lb, prob.ub, prob.mom, prob.w, **kw)
    if condition:      # (a condition on the inputs, asserted on the restatement alone before the device is compared)
        condition(want)
    got = h.opt_lm(starts, **kw)
    lmr.assert_equal(got, want)
    return got, want


# ---- 1. the built-in objectives ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p2_ub", [20.0, 5.0])
def test_objfunc_norm_equals_the_restatement(S, O, p2_ub):
    """K = 13: no multiple of the tile's 8 chains.  lb and ub are starts: at ub both differences are backward.  With the second parameter's
    range cut at 5 its moment's target, 10, lies outside: the searches end on that bound with the coordinate in the active set"""
    prob, opts = cm.serial_normal(N=3, T=4, ns=500, p2_bounds=(-20.0, p2_ub))
    h = S.hip_context(prob, opts)

    def condition(want):
        assert want["backward"][12] >= 2 and (want["iterations"] >= 2).all() and (want["status"] != 2).all()
        if p2_ub == 5.0:
            assert (want["best"][1] == 5.0).all() and (want["active"][1] == 1).all() and (want["met_active"] > 0).all()
        else:
            assert want["active"].sum() == 0 and np.abs(want["sim_moments"] - prob.mom[:, None]).max() < 1e-6
    got, _ = compare(h, oracle_evaluator(S, O, prob, opts, h), prob, box_starts(prob, 13, 1), condition, max_iter=20)
    assert got["evaluated"] == got["n_eval"].sum() and np.allclose(got["value"], got["ssr"] / 2, rtol=1e-12)


@pytest.mark.parametrize("npar,nm,K", [(5, 7, 17), (6, 3, 9)])
def test_dense_sim_equals_the_restatement(S, O, npar, nm, K):
    """nm > np, K = 17 crossing the 16-chain tile (85 Jacobian points a launch); nm < np: J'J is singular, and only lambda keeps B definite"""
    prob, opts = dense_problem(npar, nm, 4, 4)
    h = S.hip_context(prob, opts)

    def condition(want):
        assert (want["iterations"] >= 2).any() and (want["status"] != 2).all() and (want["tries"] >= want["iterations"]).all()
        if nm < npar:
            assert (np.linalg.matrix_rank(want["jac"].transpose(2, 0, 1)) <= nm).all()
    got, _ = compare(h, oracle_evaluator(S, O, prob, opts, h), prob, box_starts(prob, K, 2), condition, max_iter=8)
    assert (got["best"] != box_starts(prob, K, 2)).any() and np.allclose(got["value"], got["ssr"] / nm, rtol=1e-12)


# ---- 2. the interface's cap: 64 parameters; 50 of 64 lanes -----------------------------------------------------------------------------
def test_64_parameters_equal_the_restatement(S, O):
    """objfunc_norm with np = nm = 64: 64 lanes, a 64-row factor, 64 x 3 = 192 Jacobian points a launch"""
    prob, opts = cm.general_normal(64, N=1, T=2, ns=100)
    h = S.hip_context(prob, opts)
    st = box_starts(prob, 3, 6)
    got, _ = compare(h, oracle_evaluator(S, O, prob, opts, h), prob, st, max_iter=2)
    assert (got["iterations"] == 2).all() and got["jac"].shape == (64, 64, 3) and (got["n_eval"] >= 1 + 2 * 64 + 2).all()
    assert np.isfinite(got["ssr"]).all() and np.allclose(got["value"], got["ssr"] / 64, rtol=1e-12)


@pytest.mark.parametrize("workload", ["c5v1", "c5"])
def test_50_parameters_equal_the_restatement(S, O, workload):
    """np = nm = 50: 50 of 64 lanes; K = 17 crosses the 16-chain tile, 850 Jacobian points a launch"""
    prob, opts = build_problem(workload, 4, 4, 0, 4, 0)
    h = S.hip_context(prob, opts)
    st = box_starts(prob, 17, 2) * 0.5
    got, _ = compare(h, oracle_evaluator(S, O, prob, opts, h), prob, st, max_iter=2)
    assert (got["iterations"] == 2).all() and (got["best"] != st).any() and np.isfinite(got["value"]).all()


# ---- 3. the banana: its moments do not move ---------------------------------------------------------------------------------------------
def test_banana_ends_with_status_4_at_its_first_jacobian(S, O):
    prob, opts = build_problem("c4", 3, 3, 0, 4, 0)
    h = S.hip_context(prob, opts)
    st = box_starts(prob, 9, 4)
    got, _ = compare(h, oracle_evaluator(S, O, prob, opts, h), prob, st)
    assert (got["status"] == 4).all() and (got["iterations"] == 1).all() and (got["n_eval"] == 11).all() and (got["tries"] == 0).all()
    assert (got["jac"] == 0.0).all() and (got["grad"] == 0.0).all() and np.array_equal(got["best"], st) and got["evaluated"] == 99


# ---- 4. user objectives: +inf, NaN, a status that says no ----------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["one_thread", "map_reduce"])
def test_user_objectives_with_holes_equal_the_restatement(S, hooks, form):
    """(in the test build of the library: a registration is for the life of the process, the handles of the shipped library run on through the
    whole suite, and the oracle's table of user objectives, which later tests need for theirs, ends at 64 — these two sources take none of them)"""
    prob, opts = holes_problem(S, form)
    h = S.hip_context(prob, opts)
    st = holes_starts()

    def condition(want):
        # a try that met a hole was refused and the search went on; searches end after different numbers of iterations
        went_on = (want["not_finite"] > 0) & (want["status"] != 2) & (want["iterations"] >= 2)
        assert went_on.any() and len(set(want["iterations"])) >= 3, (want["not_finite"], want["status"], want["iterations"])
    got, want = compare(h, h.eval_batch, prob, st, condition, lambda0=1e-6, max_iter=30)
    for s in (1, 2, 4):
        assert got["status"][s] == 2 and got["n_eval"][s] == 1 and got["iterations"][s] == 0 and np.array_equal(got["best"][:, s], st[:, s])
        assert np.isnan(got["grad"][:, s]).all() and np.isnan(got["jac"][:, :, s]).all() and not np.isfinite(got["ssr"][s])
    # (status -2 at the start's evaluation is not consulted: the search runs, and where it ends with status 2 that is a Jacobian's point
    # in a hole, many iterations later)
    assert got["iterations"][3] >= 3 and np.isfinite(got["ssr"][3]) and (got["best"][:, 3] != st[:, 3]).all()
    assert got["evaluated"] == int(got["n_eval"].sum())


# ---- 5. searches that stop at different iterations and tries -----------------------------------------------------------------------------
@pytest.mark.parametrize("max_tries", [1, 2])
def test_searches_that_stop_at_different_times_equal_the_restatement(S, O, max_tries):
    """lambda0 = 1e-9 on the dense objective from the corners and the middle of the box: undamped steps, of which some fail — with one try an
    iteration such a search stops with status 3 while others go on to the cap, with two it may go on"""
    prob, opts = dense_problem(5, 7, 4, 4)
    h = S.hip_context(prob, opts)

    def condition(want):
        assert len(set(want["iterations"])) >= 2 and len(set(want["status"])) >= 2, (want["iterations"], want["status"])
        if max_tries == 2:
            assert (want["tries"] > want["iterations"]).any() and (want["tries"] == want["iterations"]).any()
    compare(h, oracle_evaluator(S, O, prob, opts, h), prob, box_starts(prob, 21, 8), condition, lambda0=1e-9, max_iter=3, max_tries=max_tries)


# ---- 6. batches -------------------------------------------------------------------------------------------------------------------
def bytes_per_search(prob):
    """include/smmhip.h (smm_opt_lm, Scratch), the built-in objectives"""
    n, m = prob.np, prob.nm
    return n * ((m + 1) * 8 + 4) + n * 8 + (m + n * n + n) * 8 + 32


def test_small_scratch_gives_the_same_results_in_batches_of_two(S, hooks, monkeypatch):
    """9 searches in batches of 2 (the last of 1): each batch runs to its end before the next starts"""
    prob, opts = dense_problem(5, 7, 4, 4)
    st = box_starts(prob, 9, 2)
    kw = dict(lambda0=1e-9, max_iter=4, max_tries=2)
    one = S.hip_context(prob, opts).opt_lm(st, **kw)
    assert len(set(one["iterations"])) >= 2 or len(set(one["tries"])) >= 2
    cap = 2 * bytes_per_search(prob) + bytes_per_search(prob) // 2
    assert cap // bytes_per_search(prob) == 2
    monkeypatch.setenv("SMMHIP_OPT_SCRATCH", str(cap))
    lmr.assert_equal(S.hip_context(prob, opts).opt_lm(st, **kw), one)
    monkeypatch.setenv("SMMHIP_OPT_SCRATCH", "1")      # less than one search's bytes: one search per batch
    lmr.assert_equal(S.hip_context(prob, opts).opt_lm(st, **kw), one)


def test_more_searches_than_one_pass_of_the_list_compaction(S, O):
    """K = 1025: k_compact's workgroup of 1024 takes each list in two passes, the second of one search"""
    prob, opts = cm.serial_normal(N=3, T=4, ns=500)
    h = S.hip_context(prob, opts)
    st = np.random.default_rng(7).uniform(prob.lb[:, None], prob.ub[:, None], (2, 1025))
    got, _ = compare(h, oracle_evaluator(S, O, prob, opts, h), prob, st, max_iter=2)
    assert got["iterations"][1024] == 2 and got["evaluated"] == got["n_eval"].sum()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_and_nothing_runs(S):
    prob, opts = cm.serial_normal(N=16, T=6, ns=500)
    h, plain = S.hip_context(prob, opts), S.hip_context(prob, opts)
    h.step(3)
    A = S._abi
    st = box_starts(prob, 6, 5)
    nan, inf = float("nan"), float("inf")
    calls = [lambda: h.opt_lm(np.empty((2, 0))),
             lambda: h.opt_lm(st, fd_step=0.0), lambda: h.opt_lm(st, fd_step=0.5000001), lambda: h.opt_lm(st, fd_step=-0.1),
             lambda: h.opt_lm(st, fd_step=nan),
             lambda: h.opt_lm(st, lambda0=0.0), lambda: h.opt_lm(st, lambda0=-1.0), lambda: h.opt_lm(st, lambda0=inf), lambda: h.opt_lm(st, lambda0=nan),
             lambda: h.opt_lm(st, lambda_up=1.0), lambda: h.opt_lm(st, lambda_up=nan),
             lambda: h.opt_lm(st, lambda_down=0.999), lambda: h.opt_lm(st, lambda_down=nan),
             lambda: h.opt_lm(st, xtol=-1e-9), lambda: h.opt_lm(st, xtol=nan),
             lambda: h.opt_lm(st, ftol=-1e-9), lambda: h.opt_lm(st, ftol=nan),
             lambda: h.opt_lm(st, gtol=-1e-9), lambda: h.opt_lm(st, gtol=nan),
             lambda: h.opt_lm(st, max_iter=0), lambda: h.opt_lm(st, max_tries=0)]
    for i, call in enumerate(calls):
        with pytest.raises(S.SMMHipError) as e:
            call()
        assert e.value.code == A.SMM_ERR_INVALID_ARG and "smm_opt_lm" in str(e.value), i
    fn = h._fn("opt_lm")
    args = (1e-4, 1e-3, 10.0, 10.0, 1e-8, 1e-12, 0.0, 10, 12, None)
    assert fn(h._ctx, None, 1, *args) == A.SMM_ERR_INVALID_ARG
    # K x np = 2^31 does not fit an int32 (refused before a start is read)
    assert fn(h._ctx, A.dptr(A.f64(st)), 2 ** 30, *args) == A.SMM_ERR_INVALID_ARG
    for bad, msg in ((3.0000001, "smm_opt_lm: the start of search 5, parameter 1 is 3: outside [-3, 3]"),
                     (nan, "smm_opt_lm: the start of search 5, parameter 1 is nan: outside [-3, 3]")):
        s2 = st.copy()
        s2[0, 4] = bad
        with pytest.raises(S.SMMHipError) as e:
            h.opt_lm(s2)
        assert e.value.code == A.SMM_ERR_INVALID_ARG and "search 5, parameter 1" in str(e.value)
        assert str(e.value).split(": ", 1)[1] == msg
    assert h.state().iter == 3
    h.opt_lm(st, fd_step=0.5, lambda_down=1.0, max_iter=3)     # ... and the context is usable afterwards (the arguments' edges are inside)
    h.step(3); plain.step(6)
    cm.assert_history_equal(h.history(0, 6), plain.history(0, 6), exact_floats=True)


# ---- 8. the context is untouched ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("persistent", [True, False])
def test_the_chains_do_not_notice(S, persistent):
    prob, opts = cm.serial_normal(N=64, T=10, ns=500)
    a, b, twin = (S.hip_context(prob, opts) for _ in range(3))
    for c in (a, b, twin):
        c.set_persistent(persistent)
    st = box_starts(prob, 13, 1)
    a.step(5)
    s0, h0, d0 = a.state(), a.history(0, 5), a.describe()
    r = a.opt_lm(st, max_iter=6)
    cm.assert_state_equal(a.state(), s0, rtol=0)
    cm.assert_history_equal(a.history(0, 5), h0, exact_floats=True)
    assert a.describe() == d0
    b.step(5)
    lmr.assert_equal(b.opt_lm(st, max_iter=6), r)      # (nor does the search notice them: a fresh context gives the same)
    lmr.assert_equal(S.hip_context(prob, opts).opt_lm(st, max_iter=6), r)
    b.step(5)
    twin.step(10)
    assert np.array_equal(b.history(0, 10).params, twin.history(0, 10).params)
    cm.assert_history_equal(b.history(0, 10), twin.history(0, 10), exact_floats=True)
    cm.assert_state_equal(b.state(), twin.state(), rtol=0)
    assert b.describe() == twin.describe()
    assert (b.persistent_info()[1] >= 1) == persistent and b.persistent_info()[1] == twin.persistent_info()[1] + (1 if persistent else 0)


# ---- 9. the host layers ---------------------------------------------------------------------------------------------------------------
def make_mprob(S):
    m = S.MProb()
    S.addSampledParam(m, OrderedDict([("p1", [0.2, -3, 3]), ("p2", [-0.2, -20, 20])]))
    S.addMoment(m, {"name": ["mu1", "mu2"], "value": [-1.0, 10.0], "weight": [1.0, 1.0]})
    S.addEvalFunc(m, S.objfunc_norm)
    return m


def test_polish_and_optLMDevice_return_what_the_raw_call_returns(S):
    opts = {"N": 6, "maxiter": 30, "maxtemp": 3, "smpl_iters": 1000, "min_improve": [0.0] * 6, "acc_tuners": [2.0, 2.0, 2.0, 1.0, 1.0, 1.0]}
    m = make_mprob(S)
    MA = S.MAlgoBGP(m, dict(opts))
    S.run(MA)
    cs = MA._ctx.chain_stats(0, 30, True, ())
    P = MA._history().params
    starts = np.array([[P[cs["best_iter"][j] - 1, k, j] for j in range(6)] for k in range(2)])
    raw = MA._ctx.opt_lm(starts, fd_step=1e-5, max_iter=20)
    res = S.polish(MA, None, per="chain", method="lm", fd_step=1e-5, max_iter=20)
    assert len(res) == 6 and sorted(r["start"]["chain"] for r in res) == list(range(6))
    assert [r["best"]["value"] for r in res] == sorted(raw["value"])
    for r in res:
        j = r["start"]["chain"]
        assert list(r["best"]["p"].items()) == [("p1", raw["best"][0, j]), ("p2", raw["best"][1, j])]
        assert r["best"]["value"] == raw["value"][j] and r["iterations"] == raw["iterations"][j] and r["converged"] == (raw["status"][j] == 1)
        assert r["status"] == raw["status"][j] and r["n_eval"] == raw["n_eval"][j] and r["tries"] == raw["tries"][j]
        assert r["ssr"] == raw["ssr"][j] and r["lambda"] == raw["lambda"][j] and r["start"]["value"] == cs["best_value"][j]
    assert all(r["best"]["value"] <= r["start"]["value"] for r in res)
    assert MA.i == 30 and MA._ctx.state().iter == 30
    with pytest.raises(TypeError):
        S.polish(MA, 9, fd_step=1e-5)
    dev = S.optLMDevice(m, starts=starts, fd_step=1e-5, maxiter=20)
    assert [d["best"]["value"] for d in dev] == list(raw["value"]) and [d["iterations"] for d in dev] == list(raw["iterations"])
    one = S.optLMDevice(m)
    assert len(one) == 1 and set(one[0]) == {"best", "iterations", "converged", "status", "n_eval", "tries", "ssr", "lambda"} and one[0]["iterations"] <= 100
