"""The premises of smm_abc_pmc's edge cases (tests/pmc_craft.py), CPU tier: the contract's restatement (tests/pmc_ref.py) run with the crafted
objectives' numpy twins — and, for the built-in objective, with the oracle — must meet the condition each committed size and seed was chosen
for, before tests/test_gpu_abc_pmc_edges.py asserts the same condition on the restatement run with the device's own evaluation and then
compares the device.  The sizes and seeds are thereby checked without a GPU: none is tuned against the code under test."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import common as cm  # noqa: E402
import pmc_craft as PC  # noqa: E402
import pmc_ref as R  # noqa: E402

import smm_jl_amd as S  # noqa: E402
from oracle import oracle as O  # noqa: E402


def run(f, npar, seed, P, A, max_gen, p_acc_min=0.0, scale=2.0, ridge=0.0, probs=()):
    return R.abc_pmc(O, f, seed, [-1.0] * npar, [1.0] * npar, PC.NM, P, A, max_gen, p_acc_min, scale, ridge, probs)


def norm_run(ns, P, A, max_gen, p_acc_min, scale, probs=(), seed=12):
    """the device tests' serial_normal case, evaluated by the oracle on the shocks the library draws for opts.seed"""
    prob, opts = cm.serial_normal(N=3, T=4, ns=ns, seed=seed)
    o = O.OracleContext(prob, opts, S.Tables(Z=O.gen_Z(opts.seed, prob.nm, prob.ns)), threads=O.max_threads())
    return R.abc_pmc(O, o.eval_batch, int(opts.seed), prob.lb, prob.ub, prob.nm, P, A, max_gen, p_acc_min, scale, 0.0, probs)


# ---- the twins are what the sources say ---------------------------------------------------------------------------------------------------------
def test_the_twins_at_their_edges():
    f = PC.staircase(4.0, 1.0)
    P = np.array([[0.1, -0.1, 0.25, -0.3, 0.3, 0.5, -1.0, 0.0, -0.26], [0.2, 0.2, 0.0, 0.1, -0.1, -0.74, 0.3, 0.0, 0.49]])
    v, m, st = f(P)
    assert list(v) == [-0.25, -0.25, 0.0, 0.0, 0.0, 0.25, 0.75, -0.25, 0.0] and (st == 1).all() and np.array_equal(m, P)
    assert list(np.signbit(v)) == [True, True, False, True, False, False, False, True, True]      # -0.0 where v == 0 and theta0 < 0
    v, m, st = PC.constant(P)
    assert (v == 0).all() and not np.signbit(v).any() and (st == 1).all()
    t = np.array([[0.5, 0.5039, 0.505, 0.5041, -0.5, -0.4961, -0.495, 0.0, 1.0, -0.0]])
    v, m, st = PC.islands(0.004)(t)
    assert list(st) == [1, 1, -2, -2, 1, 1, -2, -2, -2, -2] and np.array_equal(v, np.fabs(t[0])) and np.array_equal(m[1], v)
    assert (PC.islands(2.0)(t)[2] == 1).all()
    x = np.array([[0.1 * (k + 1)] for k in range(10)])
    want = 0.0
    for k in range(10):
        want = want + float(x[k, 0]) * float(x[k, 0])
    assert PC.bowl(x)[0][0] == want and PC.bowl(x)[1].shape == (2, 1)
    assert PC.zero_classes([1.0, -0.0, np.nan]) == {"-0"} and PC.zero_classes([-2.0, 0.0]) == {"negative", "+0"}


def test_assert_equal_tells_the_zeros_apart():
    a = run(PC.constant, 2, 5, 8, 4, 0, probs=(0.5,))
    R.assert_equal(a, a)
    for f in ("value", "eps", "logw"):
        b = dict(a)
        b[f] = -a[f] if f != "logw" else np.where(a[f] == 0, -0.0, a[f])
        assert (b[f] == a[f]).all()
        with pytest.raises(AssertionError):
            R.assert_equal(b, a)
    nan = dict(a, p_acc=-a["p_acc"])      # (the sign of a NaN is not compared)
    R.assert_equal(nan, a)


# ---- A, B ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,A,seed", list(PC.TIES_CASES))
def test_ties_premises(P, A, seed):
    PC.ties_condition(P, A, seed)(run(PC.staircase(*PC.TIES_UDATA), 2, seed, P, A, **PC.TIES))


def test_the_ties_cases_together_keep_negative_values_and_both_zeros():
    assert set().union(*PC.TIES_CASES.values()) == {"negative", "-0", "+0"}
    assert {(P, A) for P, A, _ in PC.TIES_CASES} == {(511, 255), (512, 256), (513, 257), (600, 300)}


def test_constant_premises():
    c = PC.CONSTANT_CASE
    PC.constant_condition(run(PC.constant, 2, c["seed"], c["P"], c["A"], c["max_gen"], c["p_acc_min"]))


# ---- C ------------------------------------------------------------------------------------------------------------------------------------------
def test_skew_premises():
    c = PC.SKEW
    kw = dict(seed=c["seed"], P=c["P"], A=c["A"], max_gen=c["max_gen"], p_acc_min=c["p_acc_min"], scale=c["scale"], ridge=c["ridge"])
    plain = run(PC.bowl, 10, **kw)
    PC.skew_condition(plain)
    probs, steps = PC.skew_probs(plain)
    assert len(probs) == 3 * len(steps) + 2 and all(0.0 <= p <= 1.0 for p in probs)
    PC.skew_quantile_condition(steps)(run(PC.bowl, 10, probs=probs, **kw))


def test_floor_premises():
    c = PC.FLOOR
    PC.floor_condition(run(PC.bowl, c["npar"], c["seed"], c["P"], c["A"], c["max_gen"], c["p_acc_min"], c["scale"], c["ridge"], c["probs"]))


# ---- D, E ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", PC.STRIDE_A)
def test_stride_premises(A):
    PC.stride_condition(A)(norm_run(20, A + PC.STRIDE_NEW, A, PC.STRIDE["max_gen"], PC.STRIDE["p_acc_min"], PC.STRIDE["scale"], seed=PC.STRIDE["seed"]))


def test_corner_premises():
    c = PC.CORNER
    PC.corner_condition(norm_run(c["ns"], c["A"] + c["n_new"], c["A"], c["max_gen"], c["p_acc_min"], c["scale"]))


def test_second_pass_premises():
    c = PC.PASS2
    PC.pass2_condition(norm_run(c["ns"], c["P"], c["A"], c["max_gen"], c["p_acc_min"], c["scale"]))


# ---- F ------------------------------------------------------------------------------------------------------------------------------------------
def test_all_outside_premises():
    c = PC.OUTSIDE
    for seed in c["seeds"]:
        PC.outside_condition(run(PC.islands(c["hw"]), 1, seed, c["P"], c["A"], c["max_gen"], c["p_acc_min"], c["scale"]))


@pytest.mark.parametrize("name", list(PC.THIN_CASES))
def test_thin_premises(name):
    hw, P, scale, seeds = PC.THIN_CASES[name]
    for seed in seeds:
        PC.thin_condition(name)(run(PC.islands(hw), 1, seed, P, PC.THIN_A, PC.THIN["max_gen"], PC.THIN["p_acc_min"], scale, probs=PC.THIN["probs"]))
