"""smm_sens_sobol on the device (include/smmhip.h; smm.jl_amd/csrc/smm_sobol.hpp, smm_sobol_host.hpp) against the contract's restatement
(tests/sobol_ref.py, held against closed forms in tests/test_sens_sobol.py): every output field bit for bit.  The restatement evaluates the
built-in objectives through the oracle's eval_batch and user objectives through the context's own eval_batch — neither is new code.  Shapes
are the smallest that can still go wrong: one base point, two, one below, at and one above the block of T (256), three blocks; at np = 2 a
launch is 4 nb evaluations, multiples of the evaluation tile of 8 and off it; the dense kind's tile of 16; 1 and 64 parameters (65 outputs
x 64 parameters: 17 groups of 256 pairs); objectives with holes; batches that end inside a block of T, at its end, and of one base point."""
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import common as cm  # noqa: E402
import sobol_ref as R  # noqa: E402
from moment_stats_ref import dense_problem  # noqa: E402
from test_gpu_opt_simplex import holes_problem, oracle_evaluator, registered  # noqa: E402
from user_objective_src import GENERIC_SOURCE, generic_moments  # noqa: E402

from smm_jl_amd.workloads import build_problem  # noqa: E402

pytestmark = pytest.mark.gpu


def compare(O, h, evaluator, prob, opts, N, lo=None, hi=None, condition=None):
    want = R.sens_sobol(O, evaluator, int(opts.seed), prob.lb, prob.ub, prob.nm, N, lo, hi)
    if condition:      # (a condition on the inputs, asserted on the restatement alone before the device is compared)
        condition(want)
    got = h.sens_sobol(N, lo, hi)
    R.assert_equal(got, want)
    return got, want


def norm_case(S, O, ns=40):
    prob, opts = cm.serial_normal(N=3, T=4, ns=ns)
    h = S.hip_context(prob, opts)
    return prob, opts, h, oracle_evaluator(S, O, prob, opts, h)


def generic_case(S, npar, fail_above):
    oid = registered(S, "generic", lambda: S.register_user_objective(GENERIC_SOURCE))
    mom, w = generic_moments(npar)
    prob = S.Problem(init=np.zeros(npar), lb=-np.ones(npar), ub=np.ones(npar), mom=mom, w=w, ns=1, objective_id=oid,
                     obj_params=[37.0, fail_above, float(npar)])
    opts = S.BGPOpts(N=1, maxiter=1, sigma=[0.05], acc_tuner=[1.0], min_improve=[0.0], seed=21)
    return prob, opts, S.hip_context(prob, opts)


def per_base_point(prob):
    """bytes of a launch's scratch a base point takes (include/smmhip.h: smm_sens_sobol, Scratch)"""
    return (prob.np + 2) * ((prob.np + prob.nm + 1) * 8 + 4)


# ---- 1. the built-in objectives ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 255, 256, 257, 600])
def test_objfunc_norm_equals_the_restatement(S, O, N):
    """a launch is 4 N evaluations: half a tile of 8 at N = 1, one at N = 2, 127.5 at N = 255; one block of T, a block and a block of one,
    three blocks.  Simulated moment f is the mean of shocks shifted by parameter f alone: no other parameter moves it at all"""
    prob, opts, h, ev = norm_case(S, O)

    def condition(want):
        for f in range(2):
            assert want["v_total"][1 + f, 1 - f] == 0.0 and want["v_total"][1 + f, f] > 0.0
            if N >= 2:
                assert want["total"][1 + f, 1 - f] == 0.0 and want["total"][1 + f, f] > 0.5
        assert want["n_complete"] == N and want["n_invalid"] == 0
    got, _ = compare(O, h, ev, prob, opts, N, condition=condition)
    assert got["evaluated"] == 4 * N + min(N, 256)


def test_banana_at_ten_parameters_equals_the_restatement(S, O):
    """the banana's moments are constant: every moment's numerators are exactly 0.0, and its var is 0 or the rounding of a mean of equal
    values (measured with the restatement: 7.1e-30), so its indices are 0.0 or NaN; the value's are finite, with interactions"""
    prob, opts = build_problem("c4", 3, 3, 0, 4, 0)
    h = S.hip_context(prob, opts)

    def condition(want):
        assert (want["v_total"][1:] == 0.0).all() and (want["v_first"][1:] == 0.0).all() and (want["var"][1:] <= 1e-25).all()
        assert ((want["total"][1:] == 0.0) | np.isnan(want["total"][1:])).all() and ((want["first"][1:] == 0.0) | np.isnan(want["first"][1:])).all()
        assert np.isfinite(want["total"][0]).all() and np.isfinite(want["first"][0]).all() and want["var"][0] > 0.0
        assert (want["total"][0] > want["first"][0]).any()
    compare(O, h, oracle_evaluator(S, O, prob, opts, h), prob, opts, 300, condition=condition)


def test_dense_sim_equals_the_restatement(S, O):
    """the dense kind's tile of 16: 280 evaluations are 17.5 tiles; 8 outputs x 5 parameters"""
    prob, opts = dense_problem(5, 7, 4, 4)
    h = S.hip_context(prob, opts)

    def condition(want):
        assert want["n_complete"] == 40 and np.isfinite(want["total"]).all() and (want["total"] > 0.0).all()
    compare(O, h, oracle_evaluator(S, O, prob, opts, h), prob, opts, 40, condition=condition)


def test_the_points_written_out_give_the_same_results(S, O, hooks, monkeypatch):
    """k_sobol_candidates and k_eval_batch instead of k_eval_sobol (the seam of the timing tools)"""
    prob, opts = cm.serial_normal(N=3, T=4, ns=40)
    one = S.hip_context(prob, opts).sens_sobol(300)
    monkeypatch.setenv("SMMHIP_OPT_MATERIALISE", "1")
    R.assert_equal(S.hip_context(prob, opts).sens_sobol(300), one)


# ---- 2. user objectives: one parameter, sixty-four, holes --------------------------------------------------------------------------------
def test_one_parameter(S, O):
    prob, opts, h = generic_case(S, 1, 2.0)
    got, _ = compare(O, h, h.eval_batch, prob, opts, 40)
    assert got["n_complete"] == 40 and got["first"].shape == (prob.nm + 1, 1)


def test_64_parameters(S, O):
    """66 evaluations a base point, 32 Philox blocks a point, 65 x 64 pairs; the evaluation fails (status -2) where the last parameter lies
    above 0.375: a base point is complete where neither its A nor its B does"""
    prob, opts, h = generic_case(S, 64, 0.375)

    def condition(want):
        assert 2 <= want["n_complete"] < 40 and want["n_invalid"] > 40
    compare(O, h, h.eval_batch, prob, opts, 40, condition=condition)


@pytest.mark.parametrize("form", ["one_thread", "map_reduce"])
def test_user_objectives_with_holes_equal_the_restatement(S, O, form):
    """+inf, NaN and status -2 make an evaluation invalid, and its base point incomplete"""
    prob, opts = holes_problem(S, form)
    h = S.hip_context(prob, opts)

    def condition(want):
        assert 0 < want["n_complete"] < 300 and want["n_invalid"] > 0 and np.isfinite(want["total"]).all()
    compare(O, h, h.eval_batch, prob, opts, 300, condition=condition)
    # a box where nothing is finite
    prob2 = S.Problem(init=[1.8, 0.0], lb=[1.6, -2.0], ub=[2.0, 2.0], mom=prob.mom, w=prob.w, ns=1, objective_id=prob.objective_id, obj_params=[700.0])
    h2 = S.hip_context(prob2, opts)
    got, _ = compare(O, h2, h2.eval_batch, prob2, opts, 40)
    assert got["n_complete"] == 0 and got["n_invalid"] == 160 and (got["centre"] == 0.0).all()
    assert all(np.isnan(got[f]).all() for f in ("mean", "var") + R.TABLES)


# ---- 3. batches, sub-boxes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,nb", [(600, 100), (600, 256), (30, 0)])
def test_batches_give_the_one_batch_result(S, O, hooks, monkeypatch, N, nb):
    """batches of 100 end inside the blocks of T, which go on from their partial sums; batches of 256 are the blocks; nb = 0: a cap of one
    byte, one base point a batch"""
    prob, opts = cm.serial_normal(N=3, T=4, ns=40)
    one = S.hip_context(prob, opts).sens_sobol(N)
    monkeypatch.setenv("SMMHIP_OPT_SCRATCH", str(nb * per_base_point(prob) + 10) if nb else "1")
    R.assert_equal(S.hip_context(prob, opts).sens_sobol(N), one)


def test_a_user_objective_in_batches(S, O, hooks, monkeypatch):
    prob, opts = holes_problem(S, "one_thread")
    one = S.hip_context(prob, opts).sens_sobol(300)
    assert 0 < one["n_complete"] < 300
    monkeypatch.setenv("SMMHIP_OPT_SCRATCH", str(70 * per_base_point(prob) + 10))
    R.assert_equal(S.hip_context(prob, opts).sens_sobol(300), one)


def test_a_sub_box_and_a_frozen_parameter(S, O):
    prob, opts, h, ev = norm_case(S, O)
    span = prob.ub - prob.lb
    lo, hi = prob.lb + 0.25 * span, prob.lb + 0.5 * span
    got, _ = compare(O, h, ev, prob, opts, 300, lo, hi)
    whole = h.sens_sobol(300)
    assert (got["var"] < whole["var"]).all() and (got["mean"] != whole["mean"]).all()
    # the bounds themselves are a sub-box: the same bits as none
    R.assert_equal(h.sens_sobol(300, prob.lb, prob.ub), whole)
    # the second parameter frozen: nothing moves with it
    hi2 = np.array([hi[0], lo[1]])

    def condition(want):
        assert (want["total"][:, 1] == 0.0).all() and (want["first"][:, 1] == 0.0).all() and want["total"][1, 0] > 0.5
        assert want["var"][2] <= 1e-25 and (want["v_total"][2] == 0.0).all()      # (its own moment is constant)
    compare(O, h, ev, prob, opts, 300, lo, hi2, condition=condition)


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_and_nothing_runs(S):
    prob, opts = cm.serial_normal(N=16, T=6, ns=500)
    h, plain = S.hip_context(prob, opts), S.hip_context(prob, opts)
    h.step(3)
    A = S._abi
    lb, ub = prob.lb, prob.ub
    mid = 0.5 * (lb + ub)
    nan = np.array([float("nan"), mid[1]])
    calls = [lambda: h.sens_sobol(0), lambda: h.sens_sobol(-5), lambda: h.sens_sobol(2 ** 20 + 1), lambda: h.sens_sobol(64, lb, None),
             lambda: h.sens_sobol(64, None, ub), lambda: h.sens_sobol(64, lb - 1e-9, ub), lambda: h.sens_sobol(64, lb, ub + 1e-9),
             lambda: h.sens_sobol(64, mid + [0.0, 1e-9], mid), lambda: h.sens_sobol(64, nan, ub), lambda: h.sens_sobol(64, lb, nan)]
    for i, call in enumerate(calls):
        with pytest.raises(S.SMMHipError) as e:
            call()
        assert e.value.code == A.SMM_ERR_INVALID_ARG and "smm_sens_sobol" in str(e.value), i
    fn = h._fn("sens_sobol")
    assert fn(h._ctx, 0, None, None, None) == A.SMM_ERR_INVALID_ARG
    assert fn(h._ctx, 64, None, None, None) == 0      # (no output asked for: it runs)
    assert h.sens_sobol(64, mid, mid)["n_complete"] == 64      # (a box of one point is allowed)
    assert h.state().iter == 3
    h.step(3); plain.step(6)
    cm.assert_history_equal(h.history(0, 6), plain.history(0, 6), exact_floats=True)


# ---- 5. the context is untouched ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [0, 20])
def test_the_chains_do_not_notice(S, steps):
    prob, opts = cm.serial_normal(N=64, T=30, ns=500)
    a, twin = S.hip_context(prob, opts), S.hip_context(prob, opts)
    if steps:
        a.step(steps)
        s0, h0 = a.state(), a.history(0, steps)
    d0 = a.describe()
    r = a.sens_sobol(300)
    if steps:
        cm.assert_state_equal(a.state(), s0, rtol=0)
        cm.assert_history_equal(a.history(0, steps), h0, exact_floats=True)
    assert a.describe() == d0 and a.state().iter == steps
    R.assert_equal(S.hip_context(prob, opts).sens_sobol(300), r)      # (nor does the call notice them)
    a.step(10)
    twin.step(steps + 10)
    cm.assert_history_equal(a.history(0, steps + 10), twin.history(0, steps + 10), exact_floats=True)
    cm.assert_state_equal(a.state(), twin.state(), rtol=0)
    assert a.describe() == twin.describe()


# ---- 6. the host layer ------------------------------------------------------------------------------------------------------------------
def test_host_global_sensitivity_returns_what_the_raw_call_returns(S):
    m = S.MProb()
    S.addSampledParam(m, OrderedDict([("p1", [0.2, -3, 3]), ("p2", [-0.2, -20, 20])]))
    S.addMoment(m, {"name": ["mu1", "mu2"], "value": [-1.0, 10.0], "weight": [1.0, 1.0]})
    S.addEvalFunc(m, S.objfunc_norm)
    MA = S.MAlgoBGP(m, {"N": 6, "maxiter": 10, "maxtemp": 3, "smpl_iters": 200, "min_improve": [0.0] * 6, "acc_tuners": [2.0, 2.0, 2.0, 1.0, 1.0, 1.0]})
    raw = MA._ctx.sens_sobol(512)
    res = S.global_sensitivity(MA, 512)
    assert list(res.first().keys()) == ["value", "mu1", "mu2"] and list(res.first()["mu2"].items()) == [("p1", raw["first"][2, 0]), ("p2", raw["first"][2, 1])]
    assert res.total()["value"]["p2"] == raw["total"][0, 1] and res.interaction()["value"]["p1"] == raw["total"][0, 0] - raw["first"][0, 0]
    assert res.se()["first"]["mu1"]["p1"] == raw["se_first"][1, 0] and res.se()["total"]["value"]["p2"] == raw["se_total"][0, 1]
    assert res.ranking("mu2") == ["p2", "p1"] and res.ranking("mu1") == ["p1", "p2"] and res.unidentified(1e-12) == []
    assert res.n_complete == 512 and res.evaluated == raw["evaluated"] == 512 * 4 + 256 and MA.i == 0
    # a sub-box around an estimate, by name; and the same through the MProb alone
    sub = S.global_sensitivity(MA, 512, box={"p2": (5.0, 15.0)})
    R.assert_equal(sub.raw, MA._ctx.sens_sobol(512, [-3.0, 5.0], [3.0, 15.0]))
    R.assert_equal(S.sobolIndicesDevice(m, 512, ctx=MA._ctx).raw, raw)
    # p2 frozen: it moves no moment anywhere in the box
    assert S.global_sensitivity(MA, 512, box={"p2": (10.0, 10.0)}).unidentified(1e-12) == ["p2"]
