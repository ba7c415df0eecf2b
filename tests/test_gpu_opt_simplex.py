"""smm_opt_simplex on the device (include/smmhip.h; smm.jl_amd/csrc/smm_optsimplex.hpp, smm_optsimplex_host.hpp) against the contract's restatement
(tests/simplex_ref.py, pinned to scipy in tests/test_opt_simplex.py): every output field bit for bit.  The restatement evaluates the built-in
objectives through the oracle's eval_batch and user objectives through the context's own eval_batch — neither is new code.  Shapes are the
smallest that can still go wrong: K no multiple of the evaluation tile (8 chains; 16 for the dense objective), 51 vertices on 50 lanes, 65
vertices — one more than a wave — at the interface's 64 parameters, searches that stop at different iterations (the running list is
compacted), batches of 2 searches and, once, more searches than one pass of the list compaction (1024)."""
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import common as cm  # noqa: E402
import simplex_ref as sxr  # noqa: E402
from user_objective_src import GENERIC_SOURCE, generic_moments  # noqa: E402

from smm_jl_amd.workloads import build_problem  # noqa: E402

pytestmark = pytest.mark.gpu
_user = {}

# tests/test_gpu_opt_slices.py's objectives with holes, both forms.  value: a bowl around (0.3, -0.4), flat in y inside |y + 0.4| < 0.25 (ties),
# +inf on a band of x, NaN on a band of y, nothing finite for x > 1.5; the status says "failed" left of x = -1.5 although the value is fine
# there: the search does not consult it
HOLES_BODY = r"""
    const double x = theta[0], y = theta[1];
    const double ay = __builtin_fabs(y + 0.4);
    double v = (x - 0.3) * (x - 0.3) + (ay < 0.25 ? 0.0 : ay - 0.25);
    if (x > -1.2 && x < -0.9) v = __builtin_inf();
    if (y > 0.9 && y < 1.3) v = __builtin_nan("");
    if (x > 1.5) v = y > 0.0 ? __builtin_nan("") : __builtin_inf();
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
    oid = registered(S, form, lambda: S.register_user_objective(HOLES_SOURCE) if form == "one_thread"
                     else S.register_user_objective(HOLES_LANES_SOURCE, n_sums=2, lanes=128))
    prob = S.Problem(init=[0.0, 0.0], lb=[-2.0, -2.0], ub=[2.0, 2.0], mom=[0.0, 0.5], w=[1.0, 1.0], ns=1, objective_id=oid, obj_params=[700.0])
    opts = S.BGPOpts(N=5, maxiter=4, sigma=0.05 * cm.temps(5, 4.0), acc_tuner=np.geomspace(3.0, 0.5, 5), min_improve=np.zeros(5), seed=9)
    return prob, opts


def holes_starts():
    rng = np.random.default_rng(3)
    st = rng.uniform(-2, 1.4, (2, 11))
    st[:, 0] = [0.3, -0.4]      # at the optimum, in the flat band
    st[:, 1] = [1.9, 1.0]       # nothing finite at any vertex
    st[:, 2] = [0.0, 1.1]       # in the NaN band of y
    st[:, 3] = [-1.9, -2.0]     # status -2 at a perfectly good value
    return st


def box_starts(prob, K, seed):
    rng = np.random.default_rng(seed)
    st = rng.uniform(prob.lb[:, None], prob.ub[:, None], (prob.np, K))
    st[:, 0], st[:, K - 1] = prob.lb, prob.ub      # the bounds themselves are inside (at ub every new vertex is reflected)
    return st


def oracle_evaluator(S, O, prob, opts, h):
    o = O.OracleContext(prob, opts, S.Tables(Z=h.Z()), threads=O.max_threads())
    return o.eval_batch


def compare(h, evaluator, prob, starts, step, adaptive, xatol, fatol, max_iter, condition=None):
    want = sxr.opt_simplex(evaluator, starts, prob.lb, prob.ub, prob.nm, step, adaptive, xatol, fatol, max_iter)
    if condition:      # (a condition on the inputs, asserted on the restatement alone before the device is compared)
        condition(want)
    got = h.opt_simplex(starts, step, adaptive, xatol, fatol, max_iter)
    sxr.assert_equal(got, want)
    return got, want


# ---- 1. the built-in objectives ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("adaptive", [False, True])
def test_objfunc_norm_equals_the_restatement(S, O, adaptive):
    """K = 13: no multiple of the tile's 8 chains; 39 initial evaluations"""
    prob, opts = cm.serial_normal(N=3, T=4, ns=500)
    h = S.hip_context(prob, opts)
    got, _ = compare(h, oracle_evaluator(S, O, prob, opts, h), prob, box_starts(prob, 13, 1), 0.05, adaptive, 1e-3, 1e-3, 40)
    assert (got["iterations"] >= 1).all() and np.isfinite(got["value"]).all() and got["evaluated"] == got["n_eval"].sum()
    assert (got["value"] <= got["simplex_value"]).all() and np.array_equal(got["simplex"][0], got["best"])


def banana_case(S):
    prob, opts = build_problem("c4", 3, 3, 0, 4, 0)
    return prob, opts, box_starts(prob, 9, 4)


def banana_condition(want):
    # reflection, expansion and both contractions each occur, and the searches stop after at least three different numbers of iterations:
    # the running list is compacted while others go on
    assert (want["moves"][:4].sum(1) > 0).all(), want["moves"].sum(1)
    assert len(set(want["iterations"])) >= 3, sorted(set(want["iterations"]))


BANANA = dict(step=0.05, xatol=0.18, fatol=1e9, max_iter=60)      # (the initial simplex is 0.2 wide: a search converges once it has contracted a little)


@pytest.mark.parametrize("adaptive", [False, True])
def test_banana_equals_the_restatement(S, O, adaptive):
    prob, opts, st = banana_case(S)
    h = S.hip_context(prob, opts)
    compare(h, oracle_evaluator(S, O, prob, opts, h), prob, st, BANANA["step"], adaptive, BANANA["xatol"], BANANA["fatol"], BANANA["max_iter"],
            banana_condition)


@pytest.mark.parametrize("workload", ["c5v1", "c5"])
def test_dense_sim_equals_the_restatement(S, O, workload):
    """np = nm = 50: 51 vertices ranked by 50 lanes' worth of coordinates; K = 17 crosses the 16-chain tile, 17 x 51 = 867 initial evaluations"""
    prob, opts = build_problem(workload, 4, 4, 0, 4, 0)
    h = S.hip_context(prob, opts)
    st = box_starts(prob, 17, 2) * 0.5
    got, _ = compare(h, oracle_evaluator(S, O, prob, opts, h), prob, st, 0.05, True, 1e-4, 1e-4, 25)
    assert (got["best"] != st).any() and np.isfinite(got["value"]).all() and (got["iterations"] == 25).all()


# ---- 2. the interface's cap: 64 parameters, 65 vertices ------------------------------------------------------------------------------
def test_64_parameters_equal_the_restatement(S):
    """the generic user objective as tests/test_user_shapes.py builds its wide ones (np = nm = 64): the 65th value is ranked by lane 0's
    second turn, and the evaluation fails (status -2, a NaN moment) where the last parameter lies above 0.375 — which the search ignores"""
    oid = registered(S, "generic", lambda: S.register_user_objective(GENERIC_SOURCE))
    mom, w = generic_moments(64)
    prob = S.Problem(init=np.zeros(64), lb=-np.ones(64), ub=np.ones(64), mom=mom, w=w, ns=1, objective_id=oid, obj_params=[37.0, 0.375, 64.0])
    opts = S.BGPOpts(N=1, maxiter=1, sigma=[0.05], acc_tuner=[1.0], min_improve=[0.0])
    h = S.hip_context(prob, opts)
    st = np.random.default_rng(6).integers(-200, 201, (64, 3)) / 256.0
    st[:, 2] = prob.ub
    for adaptive in (False, True):
        got, _ = compare(h, h.eval_batch, prob, st, 0.125, adaptive, 1e-6, 1e-6, 8)
        assert (got["iterations"] == 8).all() and got["simplex"].shape == (65, 64, 3) and (got["n_eval"] >= 65 + 8).all()


# ---- 3. user objectives: +inf, NaN, ties, a status that says no -------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["one_thread", "map_reduce"])
@pytest.mark.parametrize("adaptive", [False, True])
def test_user_objectives_with_holes_equal_the_restatement(S, form, adaptive):
    prob, opts = holes_problem(S, form)
    h = S.hip_context(prob, opts)
    st = holes_starts()

    def condition(want):
        assert want["moves"][4].sum() > 0 and want["ties"].any() and len(set(want["iterations"])) >= 3      # shrinks, ties, drop-outs
    got, want = compare(h, h.eval_batch, prob, st, 0.05, adaptive, 1e-6, 1e-6, 80, condition)
    assert got["status"][1] == 2 and got["n_eval"][1] == 3 and got["iterations"][1] == 0 and np.isnan(got["value"][1])
    assert np.array_equal(got["best"][:, 1], st[:, 1]) and np.isnan(got["size_x"][1]) and not np.isfinite(got["simplex_value"][:, 1]).any()
    assert np.isfinite(got["value"][3]) and got["status"][3] != 2      # (status -2 at the start's evaluations: not consulted)
    assert got["evaluated"] == int(got["n_eval"].sum()) and np.array_equal(got["moves"].sum(0), got["iterations"])


# ---- 4. batches -------------------------------------------------------------------------------------------------------------------
def bytes_per_search(prob):
    """include/smmhip.h (smm_opt_simplex, Scratch)"""
    n, m = prob.np, prob.nm
    return (n + 2) * ((n + m + 1) * 8 + 4) + (2 * n + m + 1) * 8 + 20


def test_small_scratch_gives_the_same_results_in_batches_of_two(S, hooks, monkeypatch):
    """the banana case again, 9 searches in batches of 2 (the last of 1): each batch runs to its end before the next starts, and searches
    drop out of a batch's running list as they stop"""
    prob, opts, st = banana_case(S)
    args = (st, BANANA["step"], True, BANANA["xatol"], BANANA["fatol"], BANANA["max_iter"])
    one = S.hip_context(prob, opts).opt_simplex(*args)
    banana_condition(one)
    cap = 2 * bytes_per_search(prob) + bytes_per_search(prob) // 2
    assert cap // bytes_per_search(prob) == 2
    monkeypatch.setenv("SMMHIP_OPT_SCRATCH", str(cap))
    sxr.assert_equal(S.hip_context(prob, opts).opt_simplex(*args), one)
    monkeypatch.setenv("SMMHIP_OPT_SCRATCH", "1")      # less than one search's bytes: one search per batch
    sxr.assert_equal(S.hip_context(prob, opts).opt_simplex(*args), one)


def test_more_searches_than_one_pass_of_the_list_compaction(S, O):
    """K = 1100: k_compact's workgroup of 1024 takes each list in two passes, the second of at most 76; the searches that need a second
    point lie all over the list"""
    prob, opts = cm.serial_normal(N=3, T=4, ns=500)
    h = S.hip_context(prob, opts)
    st = np.random.default_rng(7).uniform(prob.lb[:, None], prob.ub[:, None], (2, 1100))

    def condition(want):
        for part in (slice(0, 1024), slice(1024, 1100)):
            m = want["moves"][:, part].sum(1)
            assert m[0] > 0 and m[1] > 0 and m[3] > 0, m      # with and without a second point on both sides of the pass seam
    compare(h, oracle_evaluator(S, O, prob, opts, h), prob, st, 0.05, False, 1e-3, 1e-3, 4, condition)


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_and_nothing_runs(S):
    prob, opts = cm.serial_normal(N=16, T=6, ns=500)
    h, plain = S.hip_context(prob, opts), S.hip_context(prob, opts)
    h.step(3)
    A = S._abi
    st = box_starts(prob, 6, 5)
    nan = float("nan")
    calls = [lambda: h.opt_simplex(np.empty((2, 0))),
             lambda: h.opt_simplex(st, step=0.0), lambda: h.opt_simplex(st, step=1.0000001), lambda: h.opt_simplex(st, step=-0.1),
             lambda: h.opt_simplex(st, step=nan),
             lambda: h.opt_simplex(st, xatol=-1e-9), lambda: h.opt_simplex(st, xatol=nan),
             lambda: h.opt_simplex(st, fatol=-1e-9), lambda: h.opt_simplex(st, fatol=nan),
             lambda: h.opt_simplex(st, max_iter=0)]
    for i, call in enumerate(calls):
        with pytest.raises(S.SMMHipError) as e:
            call()
        assert e.value.code == A.SMM_ERR_INVALID_ARG and "smm_opt_simplex" in str(e.value), i
    fn = h._fn("opt_simplex")
    assert fn(h._ctx, None, 1, 0.05, 0, 1e-4, 1e-4, 10, None) == A.SMM_ERR_INVALID_ARG
    # K x (np + 1) = 3 x 2^30 does not fit an int32 (refused before a start is read)
    assert fn(h._ctx, A.dptr(A.f64(st)), 2 ** 30, 0.05, 0, 1e-4, 1e-4, 10, None) == A.SMM_ERR_INVALID_ARG
    for bad, msg in ((3.0000001, "smm_opt_simplex: the start of search 5, parameter 1 is 3: outside [-3, 3]"),
                     (nan, "smm_opt_simplex: the start of search 5, parameter 1 is nan: outside [-3, 3]")):
        s2 = st.copy()
        s2[0, 4] = bad
        with pytest.raises(S.SMMHipError) as e:
            h.opt_simplex(s2)
        assert e.value.code == A.SMM_ERR_INVALID_ARG and "search 5, parameter 1" in str(e.value)
        assert str(e.value).split(": ", 1)[1] == msg
    assert h.state().iter == 3
    h.opt_simplex(st, step=1.0, max_iter=3)     # ... and the context is usable afterwards (step = 1: the whole range, reflected)
    h.step(3); plain.step(6)
    cm.assert_history_equal(h.history(0, 6), plain.history(0, 6), exact_floats=True)


# ---- 6. the context is untouched ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("persistent", [True, False])
def test_the_chains_do_not_notice(S, persistent):
    prob, opts = cm.serial_normal(N=64, T=10, ns=500)
    a, b, twin = (S.hip_context(prob, opts) for _ in range(3))
    for c in (a, b, twin):
        c.set_persistent(persistent)
    st = box_starts(prob, 13, 1)
    a.step(5)
    s0, h0, d0 = a.state(), a.history(0, 5), a.describe()
    r = a.opt_simplex(st, max_iter=12)
    cm.assert_state_equal(a.state(), s0, rtol=0)
    cm.assert_history_equal(a.history(0, 5), h0, exact_floats=True)
    assert a.describe() == d0
    b.step(5)
    sxr.assert_equal(b.opt_simplex(st, max_iter=12), r)      # (nor does the search notice them: a fresh context gives the same)
    sxr.assert_equal(S.hip_context(prob, opts).opt_simplex(st, max_iter=12), r)
    b.step(5)
    twin.step(10)
    assert np.array_equal(b.history(0, 10).params, twin.history(0, 10).params)
    cm.assert_history_equal(b.history(0, 10), twin.history(0, 10), exact_floats=True)
    cm.assert_state_equal(b.state(), twin.state(), rtol=0)
    assert b.describe() == twin.describe()
    assert (b.persistent_info()[1] >= 1) == persistent and b.persistent_info()[1] == twin.persistent_info()[1] + (1 if persistent else 0)


# ---- 7. the host layers ---------------------------------------------------------------------------------------------------------------
def make_mprob(S):
    m = S.MProb()
    S.addSampledParam(m, OrderedDict([("p1", [0.2, -3, 3]), ("p2", [-0.2, -20, 20])]))
    S.addMoment(m, {"name": ["mu1", "mu2"], "value": [-1.0, 10.0], "weight": [1.0, 1.0]})
    S.addEvalFunc(m, S.objfunc_norm)
    return m


def test_polish_and_optSimplexDevice_return_what_the_raw_call_returns(S):
    opts = {"N": 6, "maxiter": 30, "maxtemp": 3, "smpl_iters": 1000, "min_improve": [0.0] * 6, "acc_tuners": [2.0, 2.0, 2.0, 1.0, 1.0, 1.0]}
    m = make_mprob(S)
    MA = S.MAlgoBGP(m, dict(opts))
    S.run(MA)
    cs = MA._ctx.chain_stats(0, 30, True, ())
    P = MA._history().params
    starts = np.array([[P[cs["best_iter"][j] - 1, k, j] for j in range(6)] for k in range(2)])
    raw = MA._ctx.opt_simplex(starts, 0.02, True, 1e-3, 1e-3, 50)
    res = S.polish(MA, 9, per="chain", method="simplex", step=0.02, adaptive=True, xatol=1e-3, fatol=1e-3, max_iter=50)
    assert len(res) == 6 and sorted(r["start"]["chain"] for r in res) == list(range(6))
    assert [r["best"]["value"] for r in res] == sorted(raw["value"])
    for r in res:
        j = r["start"]["chain"]
        assert list(r["best"]["p"].items()) == [("p1", raw["best"][0, j]), ("p2", raw["best"][1, j])]
        assert r["best"]["value"] == raw["value"][j] and r["iterations"] == raw["iterations"][j] and r["converged"] == (raw["status"][j] == 1)
        assert r["status"] == raw["status"][j] and r["n_eval"] == raw["n_eval"][j] and r["moves"] == list(raw["moves"][:, j])
        assert r["start"]["value"] == cs["best_value"][j] and list(r["start"]["p"].values()) == list(starts[:, j])
    assert any(r["converged"] for r in res)
    grp = S.polish(MA, None, per="group", method="simplex", step=0.02, adaptive=True, xatol=1e-3, fatol=1e-3, max_iter=50)
    assert [g["start"]["group"] for g in sorted(grp, key=lambda g: g["start"]["group"])] == [0, 1]
    for g in grp:
        members = [0, 1, 2] if g["start"]["group"] == 0 else [3, 4, 5]
        j = members[int(np.argmin(cs["best_value"][members]))]
        assert g["best"] == [r for r in res if r["start"]["chain"] == j][0]["best"]
    assert MA.i == 30 and MA._ctx.state().iter == 30
    # the default method is the coordinate search, as before: the same records from the same positional call
    sl = MA._ctx.opt_slices(starts, 9, 1e-3, 0.5, 20)
    old = S.polish(MA, 9, "chain", 1e-3, 0.5, 20)
    assert [r["best"]["value"] for r in old] == sorted(sl["value"]) and all(set(r) == {"best", "iterations", "converged", "start"} for r in old)
    assert old == S.polish(MA, 9, per="chain", tol=1e-3, update=0.5, maxiter=20, method="slices")
    with pytest.raises(ValueError):
        S.polish(MA, 9, method="newton")
    with pytest.raises(TypeError):
        S.polish(MA, 9, step=0.1)
    # callers.optSimplexDevice: the evaluation context of the MProb
    dev = S.optSimplexDevice(m, starts=starts, step=0.02, adaptive=True, xatol=1e-3, fatol=1e-3, maxiter=50)
    assert [d["best"]["value"] for d in dev] == list(raw["value"]) and [d["iterations"] for d in dev] == list(raw["iterations"])
    one = S.optSimplexDevice(m)
    assert len(one) == 1 and set(one[0]) == {"best", "iterations", "converged", "status", "n_eval", "moves"} and one[0]["iterations"] <= 400
