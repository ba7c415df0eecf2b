"""smm_opt_slices on the device (include/smmhip.h; smm.jl_amd/csrc/smm_optslices.hpp, smm_optslices_host.hpp) against the contract's restatement
(tests/opt_slices_ref.py): every output field bit for bit.  The restatement evaluates the built-in objectives through the oracle's eval_batch and
user objectives through the context's own eval_batch — neither is new code.  Shapes are the smallest that can still go wrong: K no multiple
of the evaluation tile (8 chains; 16 for the dense objective), more searches than one workgroup of the select (4) and, once, than one pass
of the cycle end (1024), G = 2 (the end points only) and small odd and even G."""
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import common as cm  # noqa: E402
import opt_slices_ref as osr  # noqa: E402

from smm_jl_amd.workloads import build_problem  # noqa: E402

pytestmark = pytest.mark.gpu
_user = {}

# value: a bowl around (0.3, -0.4), flat in y inside |y + 0.4| < 0.25 (ties), +inf on a band of x, NaN on a band of y, nothing finite for
# x > 1.5; the status says "failed" left of x = -1.5 although the value is fine there: the search does not consult it
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


def holes_problem(S, form):
    key = (form, id(S._abi.load()))      # (a handle belongs to the library that compiled it: the shipped one, or the test build under `hooks`)
    if key not in _user:
        _user[key] = (S.register_user_objective(HOLES_SOURCE) if form == "one_thread"
                      else S.register_user_objective(HOLES_LANES_SOURCE, n_sums=2, lanes=128))
    prob = S.Problem(init=[0.0, 0.0], lb=[-2.0, -2.0], ub=[2.0, 2.0], mom=[0.0, 0.5], w=[1.0, 1.0], ns=1, objective_id=_user[key], obj_params=[700.0])
    opts = S.BGPOpts(N=5, maxiter=4, sigma=0.05 * cm.temps(5, 4.0), acc_tuner=np.geomspace(3.0, 0.5, 5), min_improve=np.zeros(5), seed=9)
    return prob, opts


def holes_starts():
    rng = np.random.default_rng(3)
    st = rng.uniform(-2, 1.4, (2, 11))
    st[:, 0] = [0.3, -0.4]      # at the optimum
    st[:, 1] = [1.9, 1.0]       # nothing finite anywhere: along x the NaN band of y, along y the region x > 1.5
    st[:, 2] = [0.0, 1.1]       # the first coordinate step (along x at y = 1.1) sees no finite value, the second does
    st[:, 3] = [-1.9, -2.0]     # status -2 at a perfectly good value
    return st


def box_starts(prob, K, seed):
    rng = np.random.default_rng(seed)
    st = rng.uniform(prob.lb[:, None], prob.ub[:, None], (prob.np, K))
    st[:, 0], st[:, K - 1] = prob.lb, prob.ub      # the bounds themselves are inside
    return st


def oracle_evaluator(S, O, prob, opts, h):
    o = O.OracleContext(prob, opts, S.Tables(Z=h.Z()), threads=O.max_threads())
    return o.eval_batch


def compare(h, evaluator, prob, starts, G, tol, update, max_cycles, min_distinct_cycles=1):
    want = osr.opt_slices(evaluator, starts, prob.lb, prob.ub, prob.nm, G, tol, update, max_cycles)
    # (a condition on the inputs, asserted on the restatement alone before the device is compared)
    assert len(set(want["cycles"])) >= min_distinct_cycles, sorted(set(want["cycles"]))
    got = h.opt_slices(starts, G, tol, update, max_cycles)
    osr.assert_equal(got, want)
    return got, want


# ---- 1. the built-in objectives ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,update", [(5, 0.5), (2, 0.5), (5, None)])
def test_objfunc_norm_equals_the_restatement(S, O, G, update):
    """K = 13: no multiple of the tile's 8 chains, 13 x 5 = 65 evaluations: one past a multiple of 8 and of 64"""
    prob, opts = cm.serial_normal(N=3, T=4, ns=500)
    h = S.hip_context(prob, opts)
    got, want = compare(h, oracle_evaluator(S, O, prob, opts, h), prob, box_starts(prob, 13, 1), G, 0.02, update, 12)
    assert got["converged"].any() and (got["cycles"] >= 2).all()
    if update:
        assert (got["hi"] - got["lo"] < (prob.ub - prob.lb)[:, None]).all()
    else:
        assert np.array_equal(got["lo"], np.repeat(prob.lb[:, None], 13, 1)) and np.array_equal(got["hi"], np.repeat(prob.ub[:, None], 13, 1))


@pytest.mark.parametrize("workload,tol,update,max_cycles,distinct", [("c5v1", 0.01, None, 6, 3), ("c5", 0.01, None, 6, 3), ("c5v1", 1e-3, 0.5, 2, 1)])
def test_dense_sim_equals_the_restatement(S, O, workload, tol, update, max_cycles, distinct):
    """np = nm = 50, K = 17 crosses the 16-chain tile, G = 3: 51 evaluations a step, the last tile of four holds three.  On the fixed grids
    (update None) the searches stop after 3 to 6 cycles: the slice kernel reads the compacted list of those that go on"""
    prob, opts = build_problem(workload, 4, 4, 0, 4, 0)
    h = S.hip_context(prob, opts)
    st = box_starts(prob, 17, 2) * 0.5
    got, _ = compare(h, oracle_evaluator(S, O, prob, opts, h), prob, st, 3, tol, update, max_cycles, min_distinct_cycles=distinct)
    assert (got["best"] != st).any() and np.isfinite(got["value"]).all()


def test_banana_equals_the_restatement(S, O):
    prob, opts = build_problem("c4", 3, 3, 0, 4, 0)
    h = S.hip_context(prob, opts)
    compare(h, oracle_evaluator(S, O, prob, opts, h), prob, box_starts(prob, 9, 4), 4, 1e-2, 0.5, 6)


# ---- 2. user objectives: +inf, NaN, ties, a status that says no --------------------------------------------------------------------
@pytest.mark.parametrize("form", ["one_thread", "map_reduce"])
@pytest.mark.parametrize("G,update", [(7, 0.5), (6, None)])
def test_user_objectives_with_holes_equal_the_restatement(S, form, G, update):
    prob, opts = holes_problem(S, form)
    h = S.hip_context(prob, opts)
    st = holes_starts()
    got, want = compare(h, h.eval_batch, prob, st, G, 1e-4, update, 12, min_distinct_cycles=3)   # drop-out: compaction must not disturb the others
    assert got["value"][1] == np.inf and np.isnan(got["sim_moments"][:, 1]).all() and np.array_equal(got["best"][:, 1], st[:, 1])
    assert np.isfinite(got["value"][2]) and got["best"][1, 2] != st[1, 2]
    assert np.isfinite(got["value"][3]) and got["best"][0, 3] != st[0, 3]
    assert got["evaluated"] == G * 2 * int(got["cycles"].sum())


@pytest.mark.parametrize("G,update,max_cycles", [(6, None, 6), (7, 0.5, 10)])
def test_more_searches_than_one_pass_of_the_cycle_end(S, G, update, max_cycles):
    """K = 2100: k_os_cycle_end's workgroup of 1024 takes the list in three passes, the last of 52; searches stop after 1, 2 and 3 (7, 8
    and 10) cycles all over the list, so what goes on is compacted across waves and across passes"""
    prob, opts = holes_problem(S, "one_thread")
    h = S.hip_context(prob, opts)
    st = np.random.default_rng(7).uniform(-2, 2, (2, 2100))
    got, _ = compare(h, h.eval_batch, prob, st, G, 1e-4, update, max_cycles, min_distinct_cycles=3)
    assert len(set(got["cycles"][1000:1064])) >= 2 and len(set(got["cycles"][2048:])) >= 2 and np.isinf(got["value"]).sum() >= 10


def test_ties_go_to_the_lowest_grid_point(S):
    """the y grid of 33 points over [-2, 2] has four points in the flat band: -0.625 wins, and dvec follows (delta)"""
    prob, opts = holes_problem(S, "one_thread")
    h = S.hip_context(prob, opts)
    st = np.array([[0.3], [-2.0]])
    got, _ = compare(h, h.eval_batch, prob, st, 33, 1e-4, None, 1)
    assert got["best"][0, 0] == 0.25 and got["best"][1, 0] == -0.625
    assert got["delta"][0] == np.sqrt((0.3 - 0.25) * (0.3 - 0.25) + (-2.0 + 0.625) * (-2.0 + 0.625))
    assert got["cycles"][0] == 1 and got["converged"][0] == 0


def test_max_cycles_cuts_the_searches_that_would_go_on(S, O):
    prob, opts = cm.serial_normal(N=3, T=4, ns=500)
    h = S.hip_context(prob, opts)
    ev = oracle_evaluator(S, O, prob, opts, h)
    st = box_starts(prob, 13, 1)
    # search 5 starts at a fixed point of the first cycle's grids (the ranges shrink only behind a cycle): it does not move and stops converged
    # after one cycle; the others would take four
    st[:, 5] = osr.opt_slices(ev, st[:, 5:6], prob.lb, prob.ub, 2, 5, 0.02, None, 12)["best"][:, 0]
    assert (osr.opt_slices(ev, st, prob.lb, prob.ub, 2, 5, 0.02, 0.5, 12)["cycles"] > 2).sum() == 12
    got, want = compare(h, ev, prob, st, 5, 0.02, 0.5, 2, min_distinct_cycles=2)
    cut = got["cycles"] == 2
    assert cut.sum() == 12 and (got["converged"][cut] == 0).all() and (got["delta"][cut] > 0.02).all()
    assert got["cycles"][5] == 1 and got["converged"][5] == 1 and got["delta"][5] == 0.0
    assert np.isnan(got["cycle_value"][1, 5]) and not np.isnan(got["cycle_value"][:, cut]).any() and got["cycle_value"][0, 5] == got["value"][5]


# ---- 3. batches -------------------------------------------------------------------------------------------------------------------
def test_small_scratch_gives_the_same_results_in_batches(S, O, hooks, monkeypatch):
    """a search's step of 5 points takes 5 x ((2 + 1) x 8 + 4) = 140 bytes: a cap of 700 bytes holds 5 searches, 13 go in 3 batches, the last of 3"""
    prob, opts = cm.serial_normal(N=3, T=4, ns=500)
    st = box_starts(prob, 13, 1)
    one = S.hip_context(prob, opts).opt_slices(st, 5, 0.02, 0.5, 12)
    dprob, dopts = build_problem("c5v1", 4, 4, 0, 4, 0)
    dst = box_starts(dprob, 17, 2) * 0.5
    done = S.hip_context(dprob, dopts).opt_slices(dst, 3, 0.01, None, 6)
    assert len(set(done["cycles"])) >= 3      # (searches drop out of the batches as they stop)
    monkeypatch.setenv("SMMHIP_OPT_SCRATCH", "700")
    assert 700 // 140 == 5 and -(-13 // 5) == 3 and 13 % 5 == 3
    osr.assert_equal(S.hip_context(prob, opts).opt_slices(st, 5, 0.02, 0.5, 12), one)
    # the dense objective: 3 x ((50 + 1) x 8 + 4) = 1236 bytes a search, 5 searches a batch, 17 go in 4 (the last of 2)
    monkeypatch.setenv("SMMHIP_OPT_SCRATCH", "7000")
    assert 7000 // 1236 == 5
    osr.assert_equal(S.hip_context(dprob, dopts).opt_slices(dst, 3, 0.01, None, 6), done)
    # a user objective's candidates are scratch too: 7 x ((2 + 2 + 1) x 8 + 4) = 308 bytes a search, 3 searches a batch, 11 go in 4 (the last of 2)
    monkeypatch.delenv("SMMHIP_OPT_SCRATCH")
    prob, opts = holes_problem(S, "map_reduce")
    one = S.hip_context(prob, opts).opt_slices(holes_starts(), 7, 1e-4, 0.5, 12)
    monkeypatch.setenv("SMMHIP_OPT_SCRATCH", "1000")
    assert 1000 // 308 == 3
    osr.assert_equal(S.hip_context(prob, opts).opt_slices(holes_starts(), 7, 1e-4, 0.5, 12), one)


def test_written_out_candidates_give_the_same_results(S, hooks, monkeypatch):
    """the timing experiment's path (tools/opt_slices_time.py): the built-in objectives' candidates written out and evaluated by k_eval_batch"""
    prob, opts = build_problem("c5", 4, 4, 0, 4, 0)
    st = box_starts(prob, 17, 2) * 0.5
    one = S.hip_context(prob, opts).opt_slices(st, 3, 0.01, None, 6)
    monkeypatch.setenv("SMMHIP_OPT_MATERIALISE", "1")
    osr.assert_equal(S.hip_context(prob, opts).opt_slices(st, 3, 0.01, None, 6), one)


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_and_nothing_runs(S):
    prob, opts = cm.serial_normal(N=16, T=6, ns=500)
    h, plain = S.hip_context(prob, opts), S.hip_context(prob, opts)
    h.step(3)
    A = S._abi
    st = box_starts(prob, 6, 5)
    nan = float("nan")
    calls = [lambda: h.opt_slices(np.empty((2, 0)), 5), lambda: h.opt_slices(st, 1), lambda: h.opt_slices(st[:, :2], 2 ** 30),
             lambda: h.opt_slices(st, 5, tol=-1e-9), lambda: h.opt_slices(st, 5, tol=nan), lambda: h.opt_slices(st, 5, update=0.0),
             lambda: h.opt_slices(st, 5, update=-0.5), lambda: h.opt_slices(st, 5, max_cycles=0)]
    for i, call in enumerate(calls):
        with pytest.raises(S.SMMHipError) as e:
            call()
        assert e.value.code == A.SMM_ERR_INVALID_ARG and "smm_opt_slices" in str(e.value), i
    assert h._fn("opt_slices")(h._ctx, None, 1, 5, 1e-5, nan, 10, None) == A.SMM_ERR_INVALID_ARG
    for bad, msg in ((3.0000001, "smm_opt_slices: the start of search 5, parameter 1 is 3: outside [-3, 3]"),
                     (nan, "smm_opt_slices: the start of search 5, parameter 1 is nan: outside [-3, 3]")):
        s2 = st.copy()
        s2[0, 4] = bad
        with pytest.raises(S.SMMHipError) as e:
            h.opt_slices(s2, 5)
        assert e.value.code == A.SMM_ERR_INVALID_ARG and "search 5, parameter 1" in str(e.value)
        assert str(e.value).split(": ", 1)[1] == msg
    assert h.state().iter == 3
    h.opt_slices(st, 5, 0.02, 0.5, 3)     # ... and the context is usable afterwards
    h.step(3); plain.step(6)
    cm.assert_history_equal(h.history(0, 6), plain.history(0, 6), exact_floats=True)


# ---- 5. the context is untouched ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("persistent", [True, False])
def test_the_chains_do_not_notice(S, persistent):
    prob, opts = cm.serial_normal(N=64, T=10, ns=500)
    a, b, twin = (S.hip_context(prob, opts) for _ in range(3))
    for c in (a, b, twin):
        c.set_persistent(persistent)
    st = box_starts(prob, 13, 1)
    a.step(5)
    s0, h0 = a.state(), a.history(0, 5)
    r = a.opt_slices(st, 5, 0.02, 0.5, 12)
    cm.assert_state_equal(a.state(), s0, rtol=0)
    cm.assert_history_equal(a.history(0, 5), h0, exact_floats=True)
    b.step(5)
    osr.assert_equal(b.opt_slices(st, 5, 0.02, 0.5, 12), r)      # (nor does the search notice them: a fresh context gives the same)
    osr.assert_equal(S.hip_context(prob, opts).opt_slices(st, 5, 0.02, 0.5, 12), r)
    b.step(5)
    twin.step(10)
    cm.assert_history_equal(b.history(0, 10), twin.history(0, 10), exact_floats=True)
    cm.assert_state_equal(b.state(), twin.state(), rtol=0)
    assert (b.persistent_info()[1] >= 1) == persistent and b.persistent_info()[1] == twin.persistent_info()[1] + (1 if persistent else 0)


# ---- 6. the host layers ---------------------------------------------------------------------------------------------------------------
def make_mprob(S):
    m = S.MProb()
    S.addSampledParam(m, OrderedDict([("p1", [0.2, -3, 3]), ("p2", [-0.2, -20, 20])]))
    S.addMoment(m, {"name": ["mu1", "mu2"], "value": [-1.0, 10.0], "weight": [1.0, 1.0]})
    S.addEvalFunc(m, S.objfunc_norm)
    return m


def test_polish_and_optSlicesDevice_return_what_the_raw_call_returns(S):
    opts = {"N": 6, "maxiter": 30, "maxtemp": 3, "smpl_iters": 1000, "min_improve": [0.0] * 6, "acc_tuners": [2.0, 2.0, 2.0, 1.0, 1.0, 1.0]}
    m = make_mprob(S)
    MA = S.MAlgoBGP(m, dict(opts))
    S.run(MA)
    cs = MA._ctx.chain_stats(0, 30, True, ())
    P = MA._history().params
    starts = np.array([[P[cs["best_iter"][j] - 1, k, j] for j in range(6)] for k in range(2)])
    raw = MA._ctx.opt_slices(starts, 9, 1e-3, 0.5, 20)
    res = S.polish(MA, 9, per="chain", tol=1e-3, update=0.5, maxiter=20)
    assert len(res) == 6 and sorted(r["start"]["chain"] for r in res) == list(range(6))
    assert [r["best"]["value"] for r in res] == sorted(raw["value"])
    for r in res:
        j = r["start"]["chain"]
        assert list(r["best"]["p"].items()) == [("p1", raw["best"][0, j]), ("p2", raw["best"][1, j])]
        assert r["best"]["value"] == raw["value"][j] and r["iterations"] == raw["cycles"][j] and r["converged"] == bool(raw["converged"][j])
        assert r["start"]["value"] == cs["best_value"][j] and list(r["start"]["p"].values()) == list(starts[:, j])
    grp = S.polish(MA, 9, per="group", tol=1e-3, update=0.5, maxiter=20)     # two temperature groups: the best chain of each
    assert [g["start"]["group"] for g in sorted(grp, key=lambda g: g["start"]["group"])] == [0, 1]
    for g in grp:
        members = [0, 1, 2] if g["start"]["group"] == 0 else [3, 4, 5]
        j = members[int(np.argmin(cs["best_value"][members]))]
        assert g["best"] == [r for r in res if r["start"]["chain"] == j][0]["best"]
    assert MA.i == 30 and MA._ctx.state().iter == 30
    # callers.optSlicesDevice: the evaluation context of the MProb, keyed as the reference's optSlices
    dev = S.optSlicesDevice(m, 9, starts=starts, tol=1e-3, update=0.5, maxiter=20)
    assert [d["best"]["value"] for d in dev] == list(raw["value"]) and [d["iterations"] for d in dev] == list(raw["cycles"])
    one = S.optSlicesDevice(m, 25, tol=1e-2, update=0.4)
    host = S.optSlices(m, 25, tol=1e-2, update=0.4)
    assert len(one) == 1 and set(one[0]) == {"best", "iterations", "converged"}
    assert one[0]["best"] == host["best"] and one[0]["iterations"] == host["iterations"] and one[0]["converged"] == host["converged"]
