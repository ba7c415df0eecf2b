"""The starting population on the device (smm.jl_amd/csrc/smm_population.hpp, smm_population_host.hpp) where the selection's rules meet
each other: tied candidates within a lane, across lanes and across the lanes' trips (M = 64, 65, 128, 129, 200, 1000), initial_value
tying and losing, NaN / +inf / negative / -0.0 / subnormal values under every status, odd and single parameter counts, wide user rows,
batches of a shard, starts that fail, and the forms a run continues in that tests/test_gpu_population.py does not reach.  Every comparison
is bit for bit, against tests/population_ref.py and the oracle; the objectives are tests/population_craft.py's, and what they are made
for is asserted on the reference alone in tests/test_population_edges.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import common as cm  # noqa: E402
import population_craft as pc  # noqa: E402
import population_ref as pr  # noqa: E402
from test_gpu_population import exact, same_result  # noqa: E402

from smm_jl_amd.workloads import build_problem  # noqa: E402

pytestmark = pytest.mark.gpu
T = pc.T_TIES


def same(r, want):
    """same_result, and the sign of every zero (np.array_equal holds -0.0 equal to +0.0)"""
    same_result(r, want)
    for f in ("start", "value"):
        assert np.array_equal(np.signbit(r[f]) & ~np.isnan(r[f]), np.signbit(want[f]) & ~np.isnan(want[f])), f


def installed(h, want):
    """the context stands at iteration 1 with the wanted starts and values in history row 0"""
    assert h.state().iter == 1
    first = h.history(0, 1)
    assert (first.accepted == 1).all() and (first.status == 1).all() and (first.prob == 1).all() and (first.exchanged == 0).all()
    assert np.array_equal(first.params[0], want["start"]) and np.array_equal(first.value[0], want["value"], equal_nan=True)
    assert np.array_equal(np.signbit(first.value[0]) & ~np.isnan(first.value[0]), np.signbit(want["value"]) & ~np.isnan(want["value"]))
    return first


def check(S, O, prob, opts, M, spread, keep_init, steps=T - 1, persistent=None, z=False):
    """scatter on the device against the reference — results, the installed iteration 1 —, then `steps` iterations against the oracle"""
    h = S.hip_context(prob, opts)
    if persistent is not None:
        h.set_persistent(persistent)
    o, want, tabs = pr.scatter_population(O, prob, opts, S.Tables(Z=h.Z()) if z else None, M, spread, keep_init, threads=O.max_threads())
    r = h.scatter_population(M, spread, keep_init)
    same(r, want)
    installed(h, want)
    exact(h, o, 1)
    if steps:
        h.step(steps); o.step(steps)
        exact(h, o, 1 + steps)
    return h, o, r, tabs


# ---- a. ties ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep_init", [False, True])
@pytest.mark.parametrize("N,M", pc.TIES_CASES)
def test_tied_candidates(S, O, N, M, keep_init):
    """N = 3: the last workgroup of k_pop_select has three of its four waves live.  M > 64: the lanes' second and later trips"""
    oid = pc.register(S, O, pc.TIES_SOURCE)
    prob, opts = pc.ties_case(S, oid, N, M)
    h, o, r, (v, st) = check(S, O, prob, opts, M, 1.0, keep_init)
    first = (v == v.min(axis=1)[:, None]).argmax(axis=1)
    if keep_init:
        assert np.array_equal(r["pick"], np.where(v.min(axis=1) >= 0.125, -1, first))      # initial_value (1/8) wins its ties
        assert (r["pick"] == -1).any() and (r["pick"] >= 0).any()
    else:
        assert np.array_equal(r["pick"], first)
    assert h.history(0, T).accepted[1:].any()


# ---- b. special values ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep_init", [False, True])
@pytest.mark.parametrize("M,kind", pc.SPECIAL_CASES)
def test_special_values_and_statuses(S, O, M, kind, keep_init):
    oid = pc.register(S, O, pc.SPECIAL_SOURCE)
    prob, opts = pc.special_case(S, oid, M, kind)
    h, o, r, (v, st) = check(S, O, prob, opts, M, 1.0, keep_init, steps=0)
    ok = pr.valid(v, st)
    none = ~ok.any(axis=1)
    assert none.sum() >= 3 and (r["pick"][none] == -1).all() and (r["pick"][~none & (r["pick"] >= 0)] < M).all()
    chosen = r["pick"] >= 0
    assert ok[chosen, r["pick"][chosen]].all()                      # never an invalid candidate
    row = h.history(0, 1)
    if kind == "nan":      # the NaN is installed where nothing else is valid: reported and in the history
        assert np.isnan(r["value"][none]).all() and np.isnan(row.value[0][none]).all() and not np.isnan(r["value"][~none]).any()
    else:
        assert not np.isnan(r["value"]).any()


# ---- c. odd and single parameter counts, wide user rows -----------------------------------------------------------------------------
@pytest.mark.parametrize("npar,form", [(1, "loc"), (3, "tile_sim"), (5, "tile_sim")])
def test_scatter_with_an_odd_number_of_parameters(S, O, npar, form):
    """the built-in layouts: the lone last parameter of a pair (k_pop_candidates' break); np = 1 has one thread per candidate"""
    prob, opts = cm.general_normal(npar, N=70, T=T, ns=100)
    h, o, r, _ = check(S, O, prob, opts, 5, 0.5, True, z=True)
    assert h.describe()["persistent"] == form and h.persistent_info()[1] >= 1, h.describe()
    assert (r["pick"] >= 0).any() and h.history(0, T).accepted[1:].any()


@pytest.mark.parametrize("shape", ["5x3", "1x2", "lanes"])
def test_scatter_on_wide_user_rows(S, O, shape):
    """cand [n][np] and simM [n][nm] with nm != np and np odd, int status; `lanes`: the map-reduce form"""
    lanes = pc.LANES if shape == "lanes" else {}
    oid = pc.register(S, O, pc.TIES_LANES_SOURCE if lanes else pc.TIES_SOURCE, **lanes)
    N, M = pc.TIES_SHAPE_CASES[shape]
    prob, opts = pc.ties_case(S, oid, N, M, **pc.TIES_SHAPES[shape])
    h, o, r, (v, st) = check(S, O, prob, opts, M, 1.0, True)
    assert (r["pick"] == -1).any() and (r["pick"] >= 0).any()
    row = h.history(0, 1)
    cands = np.flatnonzero(r["pick"] >= 0)
    assert len({tuple(row.sim_moments[0][:, i]) for i in cands}) == len(cands)      # the moments tell the winners apart


# ---- d. batches of a shard --------------------------------------------------------------------------------------------------------------
def shard_in_batches(S, O, monkeypatch, whole, shard, M, cap, batches, nb, keep_init=True, z=False):
    """the shard's chains [32, 64) of 64 in `batches` batches of `nb` chains (the last one partly full) against the unbatched call on the
    whole population and the reference"""
    (prob, wopts), (_, sopts) = whole, shard
    one = S.hip_context(prob, wopts)
    o, want, _ = pr.scatter_population(O, prob, wopts, S.Tables(Z=one.Z()) if z else None, M, 1.0, keep_init, threads=O.max_threads())
    r1 = one.scatter_population(M, 1.0, keep_init)
    same(r1, want)
    per_chain = M * ((prob.np + prob.nm + 1) * 8 + 4)      # include/smmhip.h: the scratch of one chain
    assert cap // per_chain == nb and -(-32 // nb) == batches >= 3 and 32 % nb != 0
    monkeypatch.setenv("SMMHIP_POP_SCRATCH", str(cap))
    h = S.hip_context(prob, sopts)
    r = h.scatter_population(M, 1.0, keep_init)
    sl = dict(start=want["start"][:, 32:], value=want["value"][32:], pick=want["pick"][32:], evaluated=32 * M + 1)
    same(r, sl)
    same(r, dict(start=r1["start"][:, 32:], value=r1["value"][32:], pick=r1["pick"][32:], evaluated=32 * M + 1))
    installed(h, sl)
    a, b = h.history(0, 1), one.history(0, 1)
    for f in S._abi.HistoryBuffers.FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f)[..., 32:], equal_nan=True), f
    assert (r["pick"] >= 0).any() and len(np.unique(r["pick"])) >= 3 and len(np.unique(r["start"][0])) > 8
    return nb * M


def test_batches_of_a_shard_of_a_user_objective(S, O, hooks, monkeypatch):
    """g = chain_offset + c0 + j / M with both terms non-zero; 9 candidates x ((5 + 3 + 1) x 8 + 4) = 684 bytes a chain: 12, 12 and 8 chains"""
    oid = pc.register(S, O, pc.TIES_SOURCE)
    N, M = pc.TIES_SHAPE_CASES["shard"]
    whole = pc.ties_case(S, oid, N, M, **pc.TIES_SHAPES["shard"])
    shard = pc.ties_case(S, oid, N, M, N_local=32, chain_offset=32, **pc.TIES_SHAPES["shard"])
    shard_in_batches(S, O, monkeypatch, whole, shard, M, 8300, 3, 12)


def test_batches_of_a_shard_of_dense2(S, O, hooks, monkeypatch):
    """3 candidates x ((50 + 50 + 1) x 8 + 4) = 2436 bytes a chain: batches of 5 chains, 15 candidates — k_eval_batch<2,16>'s only block partly
    full in every batch —, the last batch 2 chains"""
    n = shard_in_batches(S, O, monkeypatch, build_problem("c5", 64, 64, 0, 4, 0), build_problem("c5", 32, 64, 1, 4, 0), 3, 12500, 7, 5,
                         keep_init=False)
    assert n % 16 != 0


# ---- e. starts that fail ------------------------------------------------------------------------------------------------------------------
def test_set_population_with_starts_that_fail(S, O):
    """`force` with a failing evaluation: a start inside the failbox (theta_0 in [1, 3]: status -2, value -1, NaN moments) is installed as
    it evaluates, like initial_value in iteration 1"""
    A = S._abi
    kw = dict(N=70, T=T, ns=1000, seed=12, objective_id=A.SMM_OBJ_NORM_FAILBOX, obj_params=[1.0, 3.0])
    prob, opts = cm.serial_normal(**kw)
    rng = np.random.default_rng(4)
    starts = rng.uniform(prob.lb[:, None], prob.ub[:, None], (2, 70))
    starts[0, :3] = [1.0, np.nextafter(1.0, 0.0), 3.0]      # on the box's lower edge (fails), just below it (valid), on its upper edge = ub (fails)
    fails = (starts[0] >= 1.0) & (starts[0] <= 3.0)
    assert 15 <= fails.sum() <= 35 and fails[:3].tolist() == [True, False, True]
    h = S.hip_context(prob, opts)
    r = h.set_population(starts)
    o, want = pr.set_population(O, prob, opts, S.Tables(Z=h.Z()), starts)
    same(r, want)
    assert (r["value"][fails] == -1.0).all() and (r["value"][~fails] >= 0).all() and (r["pick"] == 0).all()
    exact(h, o, 1)
    row = installed(h, want)
    assert np.isnan(row.sim_moments[0][:, fails]).all() and not np.isnan(row.sim_moments[0][:, ~fails]).any()
    for i in (0, 1, int(np.flatnonzero(fails)[-1])):      # the install contract: a fresh context whose initial_value is that start
        p1, _ = cm.serial_normal(**kw)
        p1.init[:] = starts[:, i]
        f = S.hip_context(p1, opts)
        f.step(1)
        fr = f.history(0, 1)
        for fld in A.HistoryBuffers.FIELDS:
            assert np.array_equal(getattr(fr, fld)[0][..., i], getattr(row, fld)[0][..., i], equal_nan=True), (fld, i)
    h.step(T - 1); o.step(T - 1)
    exact(h, o, T)
    assert h.history(0, T).accepted[1:, fails].any()


def test_set_population_with_a_start_that_is_nan(S, O):
    """SPECIAL, initial_value's class NaN: chain 0 starts at the centre (NaN, status 1: the NaN flag), the others anywhere in the box —
    every class and status is installed as it evaluates.  Install only"""
    oid = pc.register(S, O, pc.SPECIAL_SOURCE)
    prob, opts = pc.special_problem(S, oid, "nan", 0.5, 70, 3)
    rng = np.random.default_rng(6)
    starts = rng.uniform(prob.lb[:, None], prob.ub[:, None], (3, 70))
    starts[:, 0] = prob.init
    h = S.hip_context(prob, opts)
    r = h.set_population(starts)
    o, want = pr.set_population(O, prob, opts, None, starts)
    same(r, want)
    cls = pc.value_class(r["value"])
    assert np.isnan(r["value"][0]) and sorted(np.unique(cls)) == list(range(7)) and (r["pick"] == 0).all() and r["evaluated"] == 70
    installed(h, want)
    exact(h, o, 1)
    assert np.isnan(h.history(0, 1).value[0][0]) and np.isnan(h.state().la_value[0])


# ---- f. the forms a run continues in ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("persistent", [True, False])
def test_scatter_then_steps_with_a_factor_by_chain(S, O, persistent):
    from test_gpu_persist_tile_chol import factors
    prob, opts = cm.general_normal(6, N=24, T=T, ns=100)
    opts.chol_L = factors(6, 24, True)
    h, o, r, _ = check(S, O, prob, opts, 3, 0.5, True, persistent=persistent, z=True)
    assert h.describe()["persistent"] == "tile_sim", h.describe()
    assert (h.persistent_info()[1] >= 1) == persistent
    assert (r["pick"] >= 0).any() and h.history(0, T).accepted[1:].any()


def test_scatter_then_the_rows_exchange_of_a_large_shard(S, O):
    """the smallest single shard whose exchange is k_exch_resolve_rows: its accept step writes the resolution's slots, and the install has
    run no accept step — the exchanges from iteration 2 on equal the oracle's"""
    N, steps = 8193, 3
    prob, opts = cm.serial_normal(N=N, T=1 + steps, ns=64)
    assert S.hip_context(*cm.serial_normal(N=N - 1, T=1 + steps, ns=64)).describe()["exchange"] != "rows"
    h, o, r, _ = check(S, O, prob, opts, 3, 1.0, True, steps=steps, z=True)
    d = h.describe()
    assert d["exchange"] == "rows" and d["population"] == "scatter", d
    hh = h.history(0, 1 + steps)
    assert (hh.exchanged[1] != 0).any() and (hh.exchanged != 0).sum() >= 2
