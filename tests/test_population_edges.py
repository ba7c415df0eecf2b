"""The premises of tests/test_gpu_population_edges.py, pinned on the reference alone (tests/population_ref.py and the oracle; no GPU): the
crafted objectives of tests/population_craft.py do produce the ties, the special values and the seams the device cases are made for, at
the very seeds and shapes those cases use — so that no device case passes vacuously."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import population_craft as pc  # noqa: E402
import population_ref as pr  # noqa: E402
from test_population import assert_run_equal, failbox_case  # noqa: E402

_tables = {}


def ties_tables(S, O, N, M):
    """(facts, picks with and without keep_init, value table, start of the keep_init reference) of a TIES case, computed once"""
    if (N, M) not in _tables:
        oid = pc.oracle_only(O, pc.TIES_SOURCE)
        prob, opts = pc.ties_case(S, oid, N, M)
        o, r, (v, st) = pr.scatter_population(O, prob, opts, None, M, 1.0, True, threads=O.max_threads())
        iv, _, ist = o.eval_batch(prob.init[:, None])
        assert iv[0] == 0.125 and ist[0] == 1 and (st == 1).all()                       # initial_value sits in band 1
        assert np.isin(v, 0.125 * np.arange(9)).all() and len(np.unique(v)) >= 3        # a handful of distinct values
        pick0 = pr.select(v, st, iv[0], ist[0], False)
        assert np.array_equal(pick0, (v == v.min(axis=1)[:, None]).argmax(axis=1))      # the lowest m among the tied minima
        _tables[(N, M)] = (pc.ties_facts(v, r["pick"], iv[0]), r, pick0, v, pr.candidates(O, prob, opts, M, 1.0))
    return _tables[(N, M)]


# ---- TIES ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,M", pc.TIES_CASES + sorted(set(pc.TIES_SHAPE_CASES.values())))
def test_ties_cases_tie_where_the_device_cases_need_it(S, O, N, M):
    f, r, pick0, v, th = ties_tables(S, O, N, M)
    assert 2 * len(f["tied"]) >= N                                  # at least half of the chains: the minimum attained twice or more
    if M > 64:
        assert len(f["across"]) >= 1                                # tied minima on both sides of m = 64: the same lane's two trips, or two lanes
        assert len(f["late"]) >= 1 and (pick0[f["late"]] >= 64).all()     # the winner comes from a later trip
    # keep_init: initial_value ties the best candidate exactly somewhere (pick -1 by the tie rule) and is strictly worse somewhere else
    assert len(f["init_ties"]) >= 1 and (r["pick"][f["init_ties"]] == -1).all() and (pick0[f["init_ties"]] >= 0).all()
    assert len(f["init_worse"]) >= 1 and np.array_equal(r["pick"][f["init_worse"]], pick0[f["init_worse"]])
    # the tied candidates of a chain are different points: the installed start and moments say which of them won
    for i in f["tied"][:5]:
        tied = np.flatnonzero(v[i] == v[i].min())
        assert len(np.unique(th[0, i, tied])) == len(tied)


def test_a_later_trip_can_tie_an_earlier_lane(S, O):
    """somewhere among the M > 64 cases the lowest tied m of a chain is a second-trip m (>= 64) whose lane differs from a tied first-trip
    lane's — and somewhere the tie is between m and m + 64, the same lane's two trips"""
    same_lane = other_lane = False
    winners_lane = []      # (N, M, chain): the winner's own lane meets a tied candidate on a later trip — only the per-lane loop decides there
    for N, M in pc.TIES_CASES:
        if M <= 64:
            continue
        f, r, pick0, v, th = ties_tables(S, O, N, M)
        for i in f["across"]:
            tied = np.flatnonzero(v[i] == v[i].min())
            lanes_lo, lanes_hi = set(tied[tied < 64] % 64), set(tied[tied >= 64] % 64)
            same_lane |= bool(lanes_lo & lanes_hi)
            other_lane |= bool(lanes_hi - lanes_lo)
            if ((tied > pick0[i]) & (tied % 64 == pick0[i] % 64)).any():
                winners_lane.append((N, M, int(i)))
    assert same_lane and other_lane
    assert (70, 200) in {w[:2] for w in winners_lane}, winners_lane


# ---- SPECIAL ----------------------------------------------------------------------------------------------------------------------
def special_tables(S, O, M, kind):
    oid = pc.oracle_only(O, pc.SPECIAL_SOURCE)
    prob, opts = pc.special_case(S, oid, M, kind)
    o, r, (v, st) = pr.scatter_population(O, prob, opts, None, M, 1.0, True, threads=O.max_threads())
    _, r0, _ = pr.scatter_population(O, prob, opts, None, M, 1.0, False, threads=O.max_threads())
    iv, _, ist = o.eval_batch(prob.init[:, None])
    return r, r0, v, st, iv[0], int(ist[0])


@pytest.mark.parametrize("M,kind", pc.SPECIAL_CASES)
def test_special_cases_hold_every_class_and_status(S, O, M, kind):
    r, r0, v, st, iv, ist = special_tables(S, O, M, kind)
    want_v, want_st = pc.INIT_EVAL[kind]
    assert ist == want_st and (np.isnan(iv) if np.isnan(want_v) else (iv == want_v and not np.signbit(iv)))
    ok = pr.valid(v, st)
    f = pc.special_facts(v, st, ok)
    cls = f["cls"]
    assert sorted(np.unique(st)) == [-2, 0, 1, 2]
    for c in range(7):                                              # every value class with a status >= 1 ...
        assert ((cls == c) & (st >= 1)).any(), pc.CLASSES[c]
    for s in (0, -2):                                               # ... and a valid-looking value with status 0 and with -2
        assert ((cls <= 3) & (st == s)).any(), s
    assert np.array_equal(ok, (st >= 1) & (cls <= 3))               # -0.0 and the subnormal are valid; NaN, +inf and -1.0 are not
    assert len(f["none_valid"]) >= 3 and (r0["pick"][f["none_valid"]] == -1).all()
    assert len(f["raw_invalid"]) >= 3                               # the lowest value is an invalid candidate's: skipping shows
    if M > 1:
        # the winning value is +-0.0, tied between a -0.0 and a +0.0 candidate: the lower m wins, whatever its sign
        z = f["zero_tie"]
        assert len(z) >= 1 and (r0["value"][z] == 0).all()
        first = ((cls == 1) | (cls == 2)) & ok
        assert np.array_equal(r0["pick"][z], first[z].argmax(axis=1))
        signs = np.signbit(r0["value"][z])
        assert np.array_equal(signs, cls[z, r0["pick"][z]] == 2)
    else:
        # one candidate cannot tie another: the tie is between a -0.0 candidate and an initial_value of +0.0 (kind "zero"), which wins
        # it with keep_init and loses the start to the candidate without
        z = f["minus_zero_only"]
        assert len(z) >= 1 and np.signbit(r0["value"][z]).all() and (r0["pick"][z] == 0).all()
        if kind == "zero":
            assert (r["pick"][z] == -1).all() and not np.signbit(r["value"][z]).any()
    if kind in ("nan", "fail"):                                     # an invalid initial_value does not compete, but is the start of the chains without a choice
        assert np.array_equal(r["pick"], r0["pick"])
        nv = f["none_valid"]
        assert np.isnan(r["value"][nv]).all() if kind == "nan" else (r["value"][nv] == 1.0).all()
    else:
        assert (r["pick"] != r0["pick"]).any()


# ---- the reference install with a start that fails -----------------------------------------------------------------------------------
def test_the_reference_install_of_a_failing_start_is_the_first_iteration(S, O):
    """every chain started at one point inside the failbox (status -2, value -1, NaN moments): the installed state is the first iteration
    of a plain oracle context whose initial_value is that point, and the 19 after it agree"""
    prob, opts = failbox_case(S)
    point = np.array([2.0, -0.2])
    o, r = pr.set_population(O, prob, opts, None, np.repeat(point[:, None], opts.N, axis=1))
    assert (r["value"] == -1.0).all()
    p1, _ = failbox_case(S)
    p1.init[:] = point
    plain = O.OracleContext(p1, opts)
    plain.step(1)
    first = plain.history(0, 1)
    assert (first.value[0] == -1.0).all() and (first.status[0] == 1).all() and np.isnan(first.sim_moments[0]).all()
    assert_run_equal(o, plain, 1)
    plain.step(19); o.step(19)
    assert_run_equal(o, plain, 20)
    assert o.history(0, 20).accepted[1:].any()


def test_the_reference_install_of_a_nan_start_is_the_first_iteration(S, O):
    """SPECIAL with initial_value in the NaN class, status 1: install only (the objective is no BGP objective)"""
    oid = pc.oracle_only(O, pc.SPECIAL_SOURCE)
    prob, opts = pc.special_problem(S, oid, "nan", 0.5, 9, 3)
    o, r = pr.set_population(O, prob, opts, None, np.repeat(prob.init[:, None], opts.N, axis=1))
    assert np.isnan(r["value"]).all()
    plain = O.OracleContext(prob, opts)
    plain.step(1)
    assert np.isnan(plain.history(0, 1).value[0]).all()
    assert_run_equal(o, plain, 1)

