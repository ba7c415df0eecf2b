"""smm_abc_pmc on the device (include/smmhip.h; smm.jl_amd/csrc/smm_pmc.hpp, smm_pmc_host.hpp) against the contract's restatement (tests/pmc_ref.py,
held against what it restates in tests/test_abc_pmc.py): every output field bit for bit.  The restatement evaluates the built-in objectives
through the oracle's eval_batch and user objectives through the context's own eval_batch — neither is new code.  Shapes are the smallest
that can still go wrong: kept and new particles one below, at and one above the weight kernel's block of T (256) and its particles per
workgroup (256); two kept particles and one new; 1 and 64 parameters; a correlated kernel at 10; objectives with holes; once, more kept
particles than one 8192-chunk of the pairwise sums and, once, than one pass of the weight kernel (64 blocks of T); no quantile asked for; an
evaluation in three batches."""
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import common as cm  # noqa: E402
import pmc_ref as R  # noqa: E402
from test_gpu_opt_simplex import holes_problem, oracle_evaluator, registered  # noqa: E402
from user_objective_src import GENERIC_SOURCE, generic_moments  # noqa: E402

from smm_jl_amd.workloads import build_problem  # noqa: E402

pytestmark = pytest.mark.gpu
PROBS = (0.0, 0.1, 0.5, 0.975, 1.0)


def compare(O, h, evaluator, prob, opts, P, A, max_gen, p_acc_min=0.0, scale=2.0, ridge=0.0, probs=PROBS, condition=None):
    want = R.abc_pmc(O, evaluator, int(opts.seed), prob.lb, prob.ub, prob.nm, P, A, max_gen, p_acc_min, scale, ridge, probs)
    if condition:      # (a condition on the inputs, asserted on the restatement alone before the device is compared)
        condition(want)
    got = h.abc_pmc(P, A, max_gen, p_acc_min, scale, ridge, probs)
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


# ---- 1. the built-in objectives ---------------------------------------------------------------------------------------------------
def test_objfunc_norm_equals_the_restatement(S, O):
    """P = 96, A = 48, four generations: 12 evaluation tiles of 8, then the inside particles of each generation"""
    prob, opts, h, ev = norm_case(S, O)

    def condition(want):
        assert want["status"] == 0 and want["generations"] == 4 and want["n_outside"][1:].sum() > 0 and (want["n_new_kept"][1:] > 0).all()
    got, _ = compare(O, h, ev, prob, opts, 96, 48, 4, condition=condition)
    assert (np.diff(got["eps"]) <= 0).all() and got["n_kept"] == 48 and got["evaluated"] == 96 + int((48 - got["n_outside"][1:]).sum())


@pytest.mark.parametrize("A,n_new", [(255, 257), (256, 256), (257, 255), (256, 272)])
def test_kept_and_new_particles_around_the_block_of_T_and_the_workgroup(S, O, A, n_new):
    """256 kept particles are one block of T, 257 one and a block of one; 256 new particles with a finite distance fill one workgroup of the
    weight kernel, 257 start a second one.  A narrow kernel (scale 0.01) keeps nearly every new particle inside: with 257 new ones generation
    2 has exactly 257 finite distances, with 272 every generation has more than 256"""
    prob, opts, h, ev = norm_case(S, O)

    def condition(want):
        assert want["generations"] == 2 and want["n_kept"] == A
        fin = [int(np.isfinite(t["rho_new"]).sum()) for t in want["trace"] if "rho_new" in t]
        assert len(fin) == 2 and min(fin) >= 249 and (n_new != 257 or max(fin) == 257) and (n_new != 272 or min(fin) > 256), fin
    compare(O, h, ev, prob, opts, A + n_new, A, 2, scale=0.01, condition=condition)


def test_two_kept_particles_and_one_new(S, O):
    prob, opts, h, ev = norm_case(S, O)
    got, _ = compare(O, h, ev, prob, opts, 3, 2, 3, ridge=1e-3)
    assert got["n_kept"] == 2 and got["generations"] == 3


def test_banana_at_ten_parameters_equals_the_restatement(S, O):
    """a curved valley: Sigma is correlated, so the factor's off-diagonal entries work in the step and in the whitening"""
    prob, opts = build_problem("c4", 3, 3, 0, 4, 0)
    h = S.hip_context(prob, opts)

    def condition(want):
        L = want["trace"][-1]["L"]
        assert np.abs(L[np.tril_indices(10, -1)]).max() > 0.25 * np.diag(L).min() and want["generations"] == 3 and (want["n_new_kept"][1:] >= 20).all()
    compare(O, h, oracle_evaluator(S, O, prob, opts, h), prob, opts, 200, 100, 3, scale=0.25, condition=condition)


def test_more_kept_particles_than_one_chunk_of_the_pairwise_sums(S, O):
    """A = 8200: past the 8192-chunk of S; 33 blocks of T, which is one pass of the weight kernel; 100 new particles"""
    prob, opts, h, ev = norm_case(S, O, ns=20)
    got, _ = compare(O, h, ev, prob, opts, 8300, 8200, 1, probs=(0.25, 0.75))
    assert got["n_kept"] == 8200 and got["generations"] == 1


def test_more_kept_particles_than_one_pass_of_the_weight_kernel(S, O):
    """A = 16400: 65 blocks of T, one more than a pass of the weight kernel holds (64 blocks = 16384 kept particles), so the second pass
    runs from block 64 and its one block sum is added to the D the first pass left; three chunks of S; 100 new particles"""
    prob, opts, h, ev = norm_case(S, O, ns=20)

    def condition(want):
        t = want["trace"][0]
        assert want["n_kept"] == 16400 and np.isfinite(t["rho_new"]).sum() >= 30 and len(t["wn"]) == 16400 > 64 * R.T_BLOCK
    got, _ = compare(O, h, ev, prob, opts, 16500, 16400, 1, probs=(0.5,), condition=condition)
    assert got["generations"] == 1 and got["n_new_kept"][1] > 0


# ---- 2. user objectives: one parameter, sixty-four, holes --------------------------------------------------------------------------------
def test_one_parameter(S, O):
    prob, opts, h = generic_case(S, 1, 2.0)
    got, _ = compare(O, h, h.eval_batch, prob, opts, 64, 24, 3)
    assert got["generations"] == 3 and got["cov"].shape == (1, 1)


def test_64_parameters(S, O):
    """32 Philox blocks a particle and the 64-row substitution; 20 particles span 19 dimensions, so the kernel needs its ridge, and in 64
    dimensions only a narrow one (scale 0.02) leaves new particles inside the box; the evaluation
    fails (status -2) where the last parameter lies above 0.375: such particles are invalid"""
    prob, opts, h = generic_case(S, 64, 0.375)

    def condition(want):
        assert want["n_invalid"][0] > 0 and want["generations"] == 2 and want["status"] == 0 and (want["n_new_kept"][1:] > 0).all()
    got, _ = compare(O, h, h.eval_batch, prob, opts, 48, 20, 2, scale=0.02, ridge=1e-3, condition=condition)
    assert (got["theta"][63] <= 0.375).all()
    # ... and without the ridge the factor fails: status 3, the prior's best 20 are the result
    got, _ = compare(O, h, h.eval_batch, prob, opts, 48, 20, 2, scale=0.02)
    assert got["status"] == 3 and got["generations"] == 0 and got["n_kept"] == 20


def test_status_3_from_two_particles_in_three_dimensions(S, O):
    """the CPU tier's case: A = 2, np = 3, ridge = 0 over several seeds"""
    oid = registered(S, "generic", lambda: S.register_user_objective(GENERIC_SOURCE))
    mom, w = generic_moments(3)
    prob = S.Problem(init=np.zeros(3), lb=-np.ones(3), ub=np.ones(3), mom=mom, w=w, ns=1, objective_id=oid, obj_params=[37.0, 2.0, 3.0])
    status = []
    for seed in range(1, 7):
        opts = S.BGPOpts(N=1, maxiter=1, sigma=[0.05], acc_tuner=[1.0], min_improve=[0.0], seed=seed)
        h = S.hip_context(prob, opts)
        got, _ = compare(O, h, h.eval_batch, prob, opts, 24, 2, 3)
        status.append(got["status"])
    assert 3 in status, status


@pytest.mark.parametrize("form", ["one_thread", "map_reduce"])
def test_user_objectives_with_holes_equal_the_restatement(S, O, form):
    """+inf, NaN and status -2 are never kept; at generation 0 fewer than A candidates are finite"""
    prob, opts = holes_problem(S, form)
    h = S.hip_context(prob, opts)

    def condition(want):
        assert want["n_new_kept"][0] < 100 and want["n_invalid"][1:].sum() > 0 and want["generations"] == 4
    got, _ = compare(O, h, h.eval_batch, prob, opts, 128, 100, 4, condition=condition)
    n = got["n_kept"]
    th = got["theta"][:, :n]
    assert np.isfinite(got["value"][:n]).all() and (th[0] >= -1.5).all() and not ((th[0] > -1.2) & (th[0] < -0.9)).any()
    assert not ((th[1] > 0.9) & (th[1] < 1.3)).any() and (th[0] <= 1.5).all()
    # a box where nothing is finite
    prob2 = S.Problem(init=[1.8, 0.0], lb=[1.6, -2.0], ub=[2.0, 2.0], mom=prob.mom, w=prob.w, ns=1, objective_id=prob.objective_id, obj_params=[700.0])
    h2 = S.hip_context(prob2, opts)
    got, _ = compare(O, h2, h2.eval_batch, prob2, opts, 40, 10, 3)
    assert got["status"] == 2 and got["n_kept"] == 0 and got["n_invalid"][0] == 40 and np.isnan(got["theta"]).all() and (got["born"] == -1).all()


# ---- 3. batches, the stops ----------------------------------------------------------------------------------------------------------
def test_an_evaluation_in_three_batches_gives_the_same_results(S, O, hooks, monkeypatch):
    prob, opts = cm.serial_normal(N=3, T=4, ns=40)
    one = S.hip_context(prob, opts).abc_pmc(96, 48, 3, 0.0, 2.0, 0.0, PROBS)
    short = S.hip_context(prob, opts).abc_pmc(96, 48, 1, 0.0, 2.0, 0.0, PROBS)
    per_eval = (prob.np + prob.nm + 1) * 8 + 4      # include/smmhip.h (smm_abc_pmc, Scratch)
    monkeypatch.setenv("SMMHIP_OPT_SCRATCH", str(40 * per_eval + 10))      # 96 = 40 + 40 + 16
    R.assert_equal(S.hip_context(prob, opts).abc_pmc(96, 48, 3, 0.0, 2.0, 0.0, PROBS), one)
    monkeypatch.setenv("SMMHIP_OPT_SCRATCH", "1")      # less than one evaluation's bytes: one evaluation per batch
    R.assert_equal(S.hip_context(prob, opts).abc_pmc(96, 48, 1, 0.0, 2.0, 0.0, PROBS), short)


def test_the_stops(S, O):
    prob, opts, h, ev = norm_case(S, O)
    got, _ = compare(O, h, ev, prob, opts, 96, 48, 5, p_acc_min=0.99)
    assert got["status"] == 1 and got["generations"] == 1 and np.isnan(got["eps"][2]) and got["n_invalid"][2] == -1
    got, _ = compare(O, h, ev, prob, opts, 96, 48, 0)
    assert got["status"] == 0 and got["generations"] == 0 and got["evaluated"] == 96 and (got["logw"] == 0).all() and got["ess"] == 48.0
    # no quantile asked for, the binding's default: everything else is the same
    none, _ = compare(O, h, ev, prob, opts, 96, 48, 0, probs=())
    assert none["quantile"].shape == (0, 2) and np.array_equal(none["mean"], got["mean"]) and np.array_equal(none["theta"], got["theta"])
    some, _ = compare(O, h, ev, prob, opts, 96, 48, 2, probs=())
    assert some["generations"] == 2 and some["quantile"].shape == (0, 2)


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_and_nothing_runs(S):
    prob, opts = cm.serial_normal(N=16, T=6, ns=500)
    h, plain = S.hip_context(prob, opts), S.hip_context(prob, opts)
    h.step(3)
    A = S._abi
    nan = float("nan")
    calls = [lambda: h.abc_pmc(2 ** 22 + 1, 48), lambda: h.abc_pmc(96, 1), lambda: h.abc_pmc(96, 96), lambda: h.abc_pmc(96, 97),
             lambda: h.abc_pmc(96, 48, max_gen=-1), lambda: h.abc_pmc(96, 48, p_acc_min=-0.1), lambda: h.abc_pmc(96, 48, p_acc_min=1.0),
             lambda: h.abc_pmc(96, 48, p_acc_min=nan), lambda: h.abc_pmc(96, 48, scale=0.0), lambda: h.abc_pmc(96, 48, scale=nan),
             lambda: h.abc_pmc(96, 48, ridge=-1e-9), lambda: h.abc_pmc(96, 48, ridge=float("inf")), lambda: h.abc_pmc(96, 48, ridge=nan),
             lambda: h.abc_pmc(96, 48, probs=(0.5, 1.1)), lambda: h.abc_pmc(96, 48, probs=(-0.1,)), lambda: h.abc_pmc(96, 48, probs=(nan,))]
    for i, call in enumerate(calls):
        with pytest.raises(S.SMMHipError) as e:
            call()
        assert e.value.code == A.SMM_ERR_INVALID_ARG and "smm_abc_pmc" in str(e.value), i
    fn = h._fn("abc_pmc")
    assert fn(h._ctx, 96, 48, 2, 0.05, 2.0, 0.0, None, 1, None) == A.SMM_ERR_INVALID_ARG
    assert fn(h._ctx, 96, 48, 1, 0.05, 2.0, 0.0, None, 0, None) == 0      # (no output asked for: it runs)
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
    r = a.abc_pmc(96, 48, 3, 0.0, 2.0, 0.0, PROBS)
    if steps:
        cm.assert_state_equal(a.state(), s0, rtol=0)
        cm.assert_history_equal(a.history(0, steps), h0, exact_floats=True)
    assert a.describe() == d0 and a.state().iter == steps
    R.assert_equal(S.hip_context(prob, opts).abc_pmc(96, 48, 3, 0.0, 2.0, 0.0, PROBS), r)      # (nor does the sampler notice them)
    a.step(10)
    twin.step(steps + 10)
    cm.assert_history_equal(a.history(0, steps + 10), twin.history(0, steps + 10), exact_floats=True)
    cm.assert_state_equal(a.state(), twin.state(), rtol=0)
    assert a.describe() == twin.describe()


# ---- 6. the host layer ------------------------------------------------------------------------------------------------------------------
def test_host_abc_pmc_returns_what_the_raw_call_returns(S):
    m = S.MProb()
    S.addSampledParam(m, OrderedDict([("p1", [0.2, -3, 3]), ("p2", [-0.2, -20, 20])]))
    S.addMoment(m, {"name": ["mu1", "mu2"], "value": [-1.0, 10.0], "weight": [1.0, 1.0]})
    S.addEvalFunc(m, S.objfunc_norm)
    MA = S.MAlgoBGP(m, {"N": 6, "maxiter": 10, "maxtemp": 3, "smpl_iters": 200, "min_improve": [0.0] * 6, "acc_tuners": [2.0, 2.0, 2.0, 1.0, 1.0, 1.0]})
    raw = MA._ctx.abc_pmc(200, 100, 3, 0.0, 2.0, 0.0, (0.025, 0.5, 0.975))
    res = S.abc_pmc(MA, 200, keep=0.5, max_gen=3, p_acc_min=0.0)
    assert list(res.mean().items()) == [("p1", raw["mean"][0]), ("p2", raw["mean"][1])] and np.array_equal(res.cov(), raw["cov"])
    assert res.quantile()["p2"] == list(raw["quantile"][:, 1]) and res.status == 0 and res.generations == 3 and res.evaluated == raw["evaluated"]
    th, w = res.draws()
    assert np.array_equal(th, raw["theta"]) and np.array_equal(w, raw["weight"]) and MA.i == 0
    assert abs(res.mean()["p2"] - 10.0) < 5.0      # (the second data moment is the second parameter's posterior centre; the box is 40 wide)
