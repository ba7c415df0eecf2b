"""The starting population on the device (include/smmhip.h: smm_set_population, smm_scatter_population) against the reference of
tests/population_ref.py: the call's results and the run behind it, bit for bit.  Shapes are small on purpose: 70 chains are more than
one wave's and more than one workgroup's worth and no multiple of 16 or 64; 65 candidates are one past a wave."""
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import common as cm  # noqa: E402
import population_ref as pr  # noqa: E402
from test_population import all_fail_case, failbox_case  # noqa: E402
from user_objective_src import PANEL_SOURCE  # noqa: E402
from user_rng_src import AR1_RNG_SOURCE, Shim  # noqa: E402

from smm_jl_amd.workloads import build_problem  # noqa: E402

pytestmark = pytest.mark.gpu
T = 20
_refs = {}
_user = {}


def norm_case(bound=False):
    prob, opts = cm.serial_normal(N=70, T=T, ns=1000)
    if bound:
        prob.init[:] = [-3.0, 20.0]      # initial_value at a bound of either parameter
    return prob, opts


def exact(a, b, t1):
    cm.assert_history_equal(a.history(0, t1), b.history(0, t1), exact_floats=True)
    cm.assert_state_equal(a.state(), b.state(), rtol=0)


def same_result(r, want):
    for f in ("start", "value", "pick"):
        assert np.array_equal(r[f], want[f], equal_nan=True), f
    assert r["evaluated"] == want["evaluated"]


def reference(O, S, key, prob, opts, h, M, spread, keep_init):
    """the reference of a case, computed once: (results, the stepped oracle context, its value / status tables)"""
    if key not in _refs:
        o, r, tabs = pr.scatter_population(O, prob, opts, S.Tables(Z=h.Z()), M, spread, keep_init, threads=O.max_threads())
        o.step(T - 1)
        _refs[key] = (r, o, tabs)
    return _refs[key]


def check_scatter(S, O, key, prob, opts, M, spread, keep_init, persistent=None, moves=True):
    h = S.hip_context(prob, opts)
    if persistent is not None:
        h.set_persistent(persistent)
    want, o, tabs = reference(O, S, key, prob, opts, h, M, spread, keep_init)
    r = h.scatter_population(M, spread, keep_init)
    same_result(r, want)
    assert h.state().iter == 1
    first = h.history(0, 1)
    assert (first.accepted == 1).all() and (first.status == 1).all() and (first.prob == 1).all() and (first.exchanged == 0).all()
    assert np.array_equal(first.params[0], want["start"]) and np.array_equal(first.value[0], want["value"], equal_nan=True)
    h.step(T - 1)
    exact(h, o, T)
    assert h.history(0, T).accepted[1:].any() == moves
    return h, r, tabs


# ---- 1. parity with the reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,spread,keep_init,bound", [(1, 1.0, True, False), (5, 0.25, False, False), (65, 1.0, False, False),
                                                      (65, 0.25, True, True), (5, 1.0, True, False)])
def test_scatter_objfunc_norm_equals_the_reference(S, O, M, spread, keep_init, bound):
    prob, opts = norm_case(bound)
    h, r, _ = check_scatter(S, O, ("norm", M, spread, keep_init, bound), prob, opts, M, spread, keep_init)
    assert (r["pick"] >= 0).any()
    if keep_init and not bound:
        assert (r["value"] <= h.eval_batch(prob.init[:, None])[0][0]).all()
    assert (h.history(0, T).exchanged != 0).any()


def test_scatter_banana(S, O):
    prob, opts = build_problem("c4", 33, 33, 0, T, 0)
    check_scatter(S, O, "banana", prob, opts, 7, 1.0, True)


def test_scatter_dense_sim2(S, O):
    prob, opts = build_problem("c5", 17, 17, 0, T, 0)
    check_scatter(S, O, "dense2", prob, opts, 3, 0.5, True)


def user_map_reduce(S, O):
    if "mr" not in _user:
        oid = S.register_user_objective(PANEL_SOURCE, n_sums=3, lanes=256)
        O.register_user_objective(PANEL_SOURCE, oid, n_sums=3, lanes=256)
        _user["mr"] = oid
    oid = _user["mr"]
    prob = S.Problem(init=[0.3, 1.0], lb=[-0.95, 0.1], ub=[0.95, 3.0], mom=[0.0, 0.12, 0.06], w=[0.05, 0.05, 0.05], ns=1, objective_id=oid,
                     obj_params=[20.0, 300.0, 0.85])    # 20 periods x 300 agents; fails above rho = 0.85
    opts = S.BGPOpts(N=20, maxiter=T, sigma=0.05 * cm.temps(20, 4.0), acc_tuner=np.geomspace(3.0, 0.5, 20), min_improve=np.zeros(20), seed=9)
    return prob, opts


def test_scatter_map_reduce_user_objective(S, O):
    prob, opts = user_map_reduce(S, O)
    h, r, (v, st) = check_scatter(S, O, "user_mr", prob, opts, 6, 1.0, True)
    assert (st == -2).any() and (st == 1).any()      # the search skipped failing candidates


def test_scatter_stream_user_objective(S, O):
    if "rng" not in _user:
        _user["rng"] = (S.register_user_objective(AR1_RNG_SOURCE, rng=True), Shim(O, AR1_RNG_SOURCE))
    oid, shim = _user["rng"]
    prob = S.Problem(init=[0.3, 1.0], lb=[-0.95, 0.1], ub=[0.95, 3.0], mom=[0.0, 1.3, 0.6], w=[0.05, 0.1, 0.1], ns=1, objective_id=oid,
                     obj_params=[400.0, 0.8])
    opts = S.BGPOpts(N=20, maxiter=T, sigma=0.05 * cm.temps(20, 4.0), acc_tuner=np.geomspace(3.0, 0.5, 20), min_improve=np.zeros(20), seed=5)
    shim.hook(O, oid, opts.seed)      # the stream keyed by opts.seed, as in BGP steps
    h, r, (v, st) = check_scatter(S, O, "user_rng", prob, opts, 6, 1.0, False)
    assert (st == -2).any() and (st == 1).any()


# ---- 2. the persistent forms ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("persistent", [True, False])
def test_scatter_then_persistent_or_per_iteration_steps(S, O, persistent):
    prob, opts = norm_case()
    h, _, _ = check_scatter(S, O, ("norm", 5, 1.0, True, False), prob, opts, 5, 1.0, True, persistent=persistent)
    assert (h.persistent_info()[1] >= 1) == persistent
    prob, opts = build_problem("c5", 17, 17, 0, T, 0)
    tile = S.hip_context(prob, opts).persistent_info()[0]      # (where the tile form takes 17 chains)
    h, _, _ = check_scatter(S, O, "dense2", prob, opts, 3, 0.5, True, persistent=persistent)
    assert (h.persistent_info()[1] >= 1) == (persistent and tile)


# ---- 3. batches -------------------------------------------------------------------------------------------------------------------
def test_scatter_in_batches_of_chains(S, O, hooks, monkeypatch):
    """a chain's 65 candidates take 65 x ((2 + 2 + 1) x 8 + 4) = 2860 bytes: a cap of 70000 bytes holds 24 chains, 70 chains go in 3 batches"""
    prob, opts = norm_case()
    one = S.hip_context(prob, opts)
    r1 = one.scatter_population(65, 1.0, False)
    monkeypatch.setenv("SMMHIP_POP_SCRATCH", "70000")
    assert -(-70 // (70000 // 2860)) == 3
    h, r, _ = check_scatter(S, O, ("norm", 65, 1.0, False, False), prob, opts, 65, 1.0, False)
    same_result(r, r1)
    one.step(T - 1)
    exact(one, h, T)


# ---- 4. invalid candidates --------------------------------------------------------------------------------------------------------
def test_invalid_candidates_are_skipped(S, O):
    prob, opts = failbox_case(S)
    h, r, (v, st) = check_scatter(S, O, "failbox", prob, opts, 1, 1.0, False)
    failed = st[:, 0] < 1
    assert failed.sum() >= 5 and (~failed).sum() >= 5
    assert np.array_equal(r["pick"], np.where(failed, -1, 0))


def test_every_candidate_fails_equals_a_plain_run(S, O):
    prob, opts = all_fail_case(S)
    h, r, (v, st) = check_scatter(S, O, "all_fail", prob, opts, 3, 0.25, False, moves=False)   # (every proposal above the bound fails too)
    assert (st == -2).all() and (r["pick"] == -1).all()
    plain = S.hip_context(prob, opts)
    plain.step(T)
    exact(h, plain, T)


# ---- 5. smm_set_population ---------------------------------------------------------------------------------------------------------
def test_set_population_with_the_broadcast_init_is_a_fresh_context(S, O):
    for prob, opts in (norm_case(), build_problem("c4", 33, 33, 0, T, 0)):
        h, plain = S.hip_context(prob, opts), S.hip_context(prob, opts)
        r = h.set_population(np.repeat(prob.init[:, None], opts.N, axis=1))
        plain.step(1)
        assert r["evaluated"] == opts.N and (r["pick"] == 0).all() and np.array_equal(r["value"], plain.history(0, 1).value[0])
        exact(h, plain, 1)
        h.step(T - 1); plain.step(T - 1)
        exact(h, plain, T)


def test_set_population_with_distinct_starts(S, O):
    prob, opts = norm_case()
    rng = np.random.default_rng(1)
    starts = rng.uniform(prob.lb[:, None], prob.ub[:, None], (2, 70))
    starts[:, 0], starts[:, 69] = prob.lb, prob.ub      # the bounds themselves are inside
    h = S.hip_context(prob, opts)
    r = h.set_population(starts)
    o, want = pr.set_population(O, prob, opts, S.Tables(Z=h.Z()), starts)
    same_result(r, want)
    exact(h, o, 1)
    row = h.history(0, 1)
    for i in (0, 37, 69):
        p1, _ = norm_case()
        p1.init[:] = starts[:, i]
        f = S.hip_context(p1, opts)
        f.step(1)
        fr = f.history(0, 1)
        for fld in S._abi.HistoryBuffers.FIELDS:
            assert np.array_equal(getattr(fr, fld)[0][..., i], getattr(row, fld)[0][..., i]), (fld, i)
    h.step(T - 1); o.step(T - 1)
    exact(h, o, T)


def test_set_population_refuses_starts_outside_the_box(S, O):
    prob, opts = norm_case()
    h, plain = S.hip_context(prob, opts), S.hip_context(prob, opts)
    for bad, msg in ((3.0000001, "smm_set_population: the start of chain 5, parameter 1 is 3: outside [-3, 3]"),
                     (np.nan, "smm_set_population: the start of chain 5, parameter 1 is nan: outside [-3, 3]")):
        starts = np.repeat(prob.init[:, None], 70, axis=1)
        starts[0, 4] = bad
        with pytest.raises(S.SMMHipError) as e:
            h.set_population(starts)
        assert e.value.code == S._abi.SMM_ERR_INVALID_ARG and "chain 5, parameter 1" in str(e.value)
        assert str(e.value).split(": ", 1)[1] == msg
    for M, spread in ((0, 1.0), (4, 0.0), (4, 1.5), (4, np.nan), (2 ** 31 // 70 + 1, 1.0)):
        with pytest.raises(S.SMMHipError) as e:
            h.scatter_population(M, spread)
        assert e.value.code == S._abi.SMM_ERR_INVALID_ARG
    assert h.state().iter == 0
    h.step(T); plain.step(T)
    exact(h, plain, T)


# ---- 6. shards -------------------------------------------------------------------------------------------------------------------
def test_two_shards_pick_what_the_single_shard_picks(S, O):
    prob, whole = cm.serial_normal(N=64, T=4, ns=1000)
    r = S.hip_context(prob, whole).scatter_population(9, 0.5, True)
    for off in (0, 32):
        _, shard = cm.serial_normal(N=64, T=4, ns=1000, N_local=32, chain_offset=off)
        rs = S.hip_context(prob, shard).scatter_population(9, 0.5, True)
        for f in ("start", "value", "pick"):
            assert np.array_equal(rs[f], r[f][..., off:off + 32]), (f, off)
    assert len(np.unique(r["start"][0])) > 32


# ---- 7. the state machine and the host layer ---------------------------------------------------------------------------------------
def test_population_calls_after_a_step_are_refused(S, O):
    prob, opts = norm_case()
    h = S.hip_context(prob, opts)
    assert "population" not in h.describe()
    h.step(1)
    for call in (lambda: h.scatter_population(4), lambda: h.set_population(np.repeat(prob.init[:, None], 70, axis=1))):
        with pytest.raises(S.SMMHipError) as e:
            call()
        assert e.value.code == S._abi.SMM_ERR_STATE
    g = S.hip_context(prob, opts)
    g.scatter_population(4, 0.5)
    d = g.describe()
    assert d["population"] == "scatter" and d["pop_M"] == "4" and float(d["pop_spread"]) == 0.5
    with pytest.raises(S.SMMHipError) as e:      # ... and after an install
        g.scatter_population(4, 0.5)
    assert e.value.code == S._abi.SMM_ERR_STATE
    s = S.hip_context(prob, opts)
    s.set_population(np.repeat(prob.init[:, None], 70, axis=1))
    assert s.describe()["population"] == "set"


def make_mprob(S):
    m = S.MProb()
    S.addSampledParam(m, OrderedDict([("p1", [0.2, -3, 3]), ("p2", [-0.2, -20, 20])]))
    S.addMoment(m, {"name": ["mu1", "mu2"], "value": [-1.0, 10.0], "weight": [1.0, 1.0]})
    S.addEvalFunc(m, S.objfunc_norm)
    return m


def test_scatter_start_through_the_host_layer(S, O, tmp_path):
    opts = {"N": 6, "maxiter": 10, "maxtemp": 3, "smpl_iters": 1000, "min_improve": [0.0] * 6, "acc_tuners": [2.0] * 6}
    MA = S.MAlgoBGP(make_mprob(S), dict(opts))
    r = S.scatter_start(MA, M=8, spread=0.5)
    assert MA.i == 1 and r["evaluated"] == 49 and MA._ctx.describe()["population"] == "scatter"
    assert len(S.history(MA.chains[0])) == 1
    S.computeNextIteration(MA)
    assert MA.i == 2
    S.run(MA)
    assert MA.i == 10 and len(S.summary(MA)) == 6
    assert np.array_equal(MA._history().params[0], r["start"])
    # save -> readMalgo -> restart equals the uninterrupted run (the start is history row 0: save needs nothing new)
    S.save(MA, str(tmp_path / "run"))
    MB = S.readMalgo(S.MAlgoBGP(make_mprob(S), dict(opts)), str(tmp_path / "run"))
    S.restart(MB, 15)
    full = dict(opts); full["maxiter"] = 25
    MC = S.MAlgoBGP(make_mprob(S), full)
    S.scatter_start(MC, M=8, spread=0.5)
    S.run(MC)
    assert MB.i == 25 and MC.i == 25
    cm.assert_history_equal(MB._history(), MC._history(), exact_floats=True)
    cm.assert_state_equal(MB._state(), MC._state(), rtol=0)
    rh = S.rhat(MC)      # (all six chains share acc_tuner 2.0: one group of overdispersed starts)
    assert len(rh) == 1 and list(rh[0]) == ["p1", "p2"] and all(np.isfinite(v) and v > 0 for v in rh[0].values())
    MD = S.MAlgoBGP(make_mprob(S), dict(opts))
    st = S.set_start(MD, [{"p1": 0.1 * j, "p2": -1.0 * j} for j in range(6)])
    assert MD.i == 1 and np.array_equal(st["start"][1], -1.0 * np.arange(6))
