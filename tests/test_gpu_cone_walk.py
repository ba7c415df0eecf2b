"""The persistent kernels' lone-wave cone walk (lean_walk_sub64, smm.jl_amd/csrc/smm_walk_lean.hpp) on pair tables crafted for it
(tests/cone_craft.py; their depths and widths are held against a plain restatement in tests/test_cone_craft.py): every tail of the
walk's unrolled trip, the cap of 32 sub-levels and one past it (through a wide level: lists deeper than 31 levels stay off these
forms), a tile that walks nothing beside tiles that walk, levels of 64, 65, 128 and 130 pairs, a plan-window seam (the launch's first
walk), key ties — in every persistent form: k_chain_persist_loc with 8-byte slots and the guard (min_improve 0), with 16-byte slots
(one threshold), with thresholds by chain, with one and two parameters; k_chain_persist_tile (objfunc_norm, three parameters);
k_chain_persist_gen (banana; it walks the same lists with lean_walk_levels); a map-reduce user objective, whose kernel (tile_user)
hiprtc compiles from the embedded headers with the walker in it, and a one-thread one (gen_user).  Histories and states are the oracle's and, to the bit, those of a twin context on the one-launch-per-iteration
kernels.  Replaces exchangeMoves! (AlgoBGP.jl:647-716) inside run!'s loop."""
import numpy as np
import pytest

import common as cm
import cone_craft as CC
from smm_jl_amd import _abi as A

pytestmark = pytest.mark.gpu

T = 12
NS = 64


def problem(S, form, N, mi_seed=5):
    """(prob, opts, wants the SMMHIP_PERSIST_LOC seam, atol against the oracle)"""
    if form in ("loc_key2", "loc_wide2", "loc_pct2"):
        prob, opts = cm.serial_normal(N=N, T=T, ns=NS, seed=7, min_improve=0.05 if form == "loc_wide2" else 0.0)
        if form == "loc_pct2":
            opts.min_improve[:] = np.random.default_rng(mi_seed).choice([0.0, 0.0, 0.002, 0.05, 0.5], N)
            opts.min_improve[0] = 0.0; opts.min_improve[1] = 0.05      # (not uniform, whatever the draw)
        return prob, opts, form != "loc_pct2", 0.0
    if form in ("loc_key1", "loc_wide1"):
        prob, opts = cm.general_normal(1, N=N, T=T, ns=NS)
        opts.min_improve[:] = 0.05 if form == "loc_wide1" else 0.0
        return prob, opts, True, 0.0
    if form == "gen":      # banana, four parameters: k_chain_persist_gen (tiles of 32 chains)
        prob = S.Problem(init=np.full(4, 1.2), lb=-2 * np.ones(4), ub=2 * np.ones(4), mom=np.zeros(4), w=np.ones(4), ns=1, objective_id=A.SMM_OBJ_BANANA)
        opts = S.BGPOpts(N=N, maxiter=T, sigma=0.02 * cm.temps(N, 5), acc_tuner=np.geomspace(20, 1, N), min_improve=np.zeros(N), seed=3)
        return prob, opts, False, 1e-12    # (parameters pass through 0: lb + x (ub - lb) cancels — test_gpu_persist_gen.py)
    assert form == "tile"  # objfunc_norm, three parameters: k_chain_persist_tile
    prob, opts = cm.general_normal(3, N=N, T=T, ns=NS)
    return prob, opts, False, 0.0


def run(S, O, prob, opts, tab, steps, atol=0.0, fits=True, oracle_tables=None):
    tables = S.Tables(pairs=tab)
    h = S.hip_context(prob, opts, tables)
    c = S.hip_context(prob, opts, tables)
    c.set_persistent(False)
    o = O.OracleContext(prob, opts, oracle_tables if oracle_tables is not None else S.Tables(pairs=tab, Z=h.Z()))
    for n in steps:
        h.step(n); c.step(n); o.step(n)
    avail, launches, repairs = h.persistent_info()
    if fits:
        assert launches >= 1 and repairs == 0, (launches, repairs, h.describe())
    assert c.persistent_info()[1] == 0
    hh = h.history()
    cm.assert_history_equal(hh, c.history(), exact_floats=True)
    cm.assert_state_equal(h.state(), c.state(), rtol=0)
    cm.assert_history_equal(hh, o.history(), atol=atol)
    cm.assert_state_equal(h.state(), o.state(), atol=atol)
    assert (hh.exchanged != 0).any()
    return h


def seam(monkeypatch, on):
    if on:
        monkeypatch.setenv("SMMHIP_PERSIST_LOC", "1")


@pytest.mark.parametrize("form", ["loc_key2", "loc_wide2"])
@pytest.mark.parametrize("d", [1, 2, 3, 4, 5, 6, 7, 31, 32, 33])
def test_depth_every_tail_of_the_trip_the_cap_and_one_past_it(S, O, monkeypatch, hooks, form, d):
    # the tile that owns chain d walks exactly d sub-levels.  d = 32 and 33: an injected list deeper than LV_MAXLEV = 31 levels is kept
    # off the persistent forms when the context is created (smm_create_host.hpp: deep_plan), so depth alone reaches neither the cap of 32
    # sub-levels nor 33 — only the results are held there; test_the_cap_of_32_sub_levels_and_one_past_it gets there through a wide level
    prob, opts, sm, atol = problem(S, form, 80)
    seam(monkeypatch, sm)
    run(S, O, prob, opts, CC.chain_table(d), [1, 5, 6], atol, fits=d <= CC.LV_MAXLEV)


@pytest.mark.parametrize("form", ["loc_key2", "loc_wide2", "gen", "tile"])
@pytest.mark.parametrize("past", [False, True])
def test_the_cap_of_32_sub_levels_and_one_past_it(S, O, monkeypatch, hooks, form, past):
    # tile 0: 5 sub-levels of the tree and 27 single pairs behind them = 32 sub-levels in 31 levels; or 8 + 25 = 33 in 30 levels: no
    # cone (cone_ok = 0), the iteration is walked the other way and only the results are held
    prob, opts, sm, atol = problem(S, form, 320)
    seam(monkeypatch, sm)
    run(S, O, prob, opts, CC.tree_table(extra=past, tail=25 if past else 27), [3, 9], atol, fits=not past)


@pytest.mark.parametrize("form", ["loc_key2", "loc_wide2"])
def test_a_tile_without_pairs_beside_tiles_that_walk(S, O, monkeypatch, hooks, form):
    prob, opts, sm, atol = problem(S, form, 80)
    seam(monkeypatch, sm)
    h = run(S, O, prob, opts, CC.chain_table(3, skip_tiles=1), [T], atol)
    assert not (h.history().exchanged[:, 16:32] != 0).any()


@pytest.mark.parametrize("form", ["loc_key2", "loc_wide2", "loc_pct2", "loc_key1", "gen", "tile"])
@pytest.mark.parametrize("extra", [False, True])
def test_width_two_sub_levels_of_one_level(S, O, monkeypatch, hooks, form, extra):
    # the cone of tile 0: levels of 128 / 64 / 32 / 16 pairs, or 130 / 65 / 33 / 16 / 1; 240 or 244 gathered chains
    prob, opts, sm, atol = problem(S, form, 320)
    seam(monkeypatch, sm)
    h = run(S, O, prob, opts, CC.tree_table(extra), [2, 10], atol)
    if form == "loc_pct2":
        assert h.describe()["persistent"] == "loc_wide", h.describe()


@pytest.mark.parametrize("form,d,N", [("loc_key1", 6, 80), ("loc_key1", 31, 80), ("loc_wide1", 5, 80), ("loc_wide1", 30, 80), ("loc_pct2", 7, 80),
                                      ("loc_pct2", 31, 80), ("gen", 3, 96), ("gen", 31, 96), ("tile", 5, 80), ("tile", 31, 80)])
def test_depth_in_the_other_forms(S, O, monkeypatch, hooks, form, d, N):
    prob, opts, sm, atol = problem(S, form, N)
    seam(monkeypatch, sm)
    run(S, O, prob, opts, CC.chain_table(d, N=N, ct=32 if form == "gen" else 16), [1, 11], atol)


@pytest.mark.parametrize("table", ["chain31", "tree_extra"])
def test_a_map_reduce_user_objective_compiles_the_walker_from_the_embedded_headers(S, O, table):
    # tile_user: hiprtc's build of smm_chain_persist_tile.hpp with the user's text, on smm_walk_lean.hpp as the library carries it —
    # the one place where lean_walk_sub64 is instantiated outside the library's own build (18 parameters, 3 moments, 17 sums, 128 lanes)
    from test_gpu_user_shapes import problem as user_problem, register
    from user_objective_src import GENERIC_LANES_SOURCE
    oid, _host = register(S, O, GENERIC_LANES_SOURCE, n_sums=17, lanes=128)
    N = 80 if table == "chain31" else 320
    prob, opts = user_problem(S, oid, 18, 3, 17, 1500, N, T)
    tab = CC.chain_table(31) if table == "chain31" else CC.tree_table(True)
    h = run(S, O, prob, opts, tab, [1, 11], oracle_tables=S.Tables(pairs=tab))
    assert h.describe()["persistent"] == "tile_user", h.describe()


def test_a_one_thread_user_objective_on_the_crafted_lists(S, O):
    # gen_user: hiprtc's build of smm_chain_persist_gen.hpp, which walks with lean_walk_levels — the embedded smm_walk_lean.hpp is
    # parsed with the new templates in it, none of them instantiated
    from test_gpu_user_shapes import problem as user_problem, register
    from user_objective_src import GENERIC_SOURCE
    oid, _host = register(S, O, GENERIC_SOURCE)
    prob, opts = user_problem(S, oid, 3, 3, 4, 37, 96, T)
    tab = CC.chain_table(31, N=96, ct=32)
    h = run(S, O, prob, opts, tab, [1, 11], oracle_tables=S.Tables(pairs=tab))
    assert h.describe()["persistent"] == "gen_user", h.describe()


@pytest.mark.parametrize("form", ["loc_key2", "loc_wide2"])
@pytest.mark.parametrize("table", ["chain7", "tree_extra"])
def test_a_plan_window_seam_the_first_walk_of_a_launch(S, O, monkeypatch, hooks, form, table):
    # windows of four iterations: every launch but the first starts with the walk its predecessor left ("iteration 0")
    monkeypatch.setenv("SMMHIP_PLAN_CAP", "4")
    N = 80 if table == "chain7" else 320
    prob, opts, sm, atol = problem(S, form, N)
    seam(monkeypatch, sm)
    h = run(S, O, prob, opts, CC.chain_table(7) if table == "chain7" else CC.tree_table(True), [T], atol)
    assert h.persistent_info()[1] >= 2


def test_key_ties_are_decided_by_the_exact_values(S, O, monkeypatch, hooks):
    """Every chain starts from a value that differs from every other chain's only BELOW its upper 32 bits, so every pair of the walk
    ties on its 32-bit order keys until one of its chains accepts a proposal, and the guard's exact compare decides.  The values are
    tiny (hardly a proposal is accepted against them) and go in through set_state — into the persistent context, into the twin on the
    one-launch-per-iteration kernels and into the oracle, which knows no keys at all: it compares the values themselves."""
    monkeypatch.setenv("SMMHIP_PERSIST_LOC", "1")
    N = 80
    prob, opts, _, _ = problem(S, "loc_key2", N)
    pairs = CC.filler(range(N), N)           # (2k, 2k + 1) for all k, then (2k + 1, 2k + 2): two levels of 40 pairs
    tab = CC.as_table(pairs, T)
    CC.check_table(tab, N)
    tables = S.Tables(pairs=tab)
    seed = S.hip_context(prob, opts, tables)
    seed.set_persistent(False)
    seed.step(2)
    st, hist = seed.state(), seed.history()
    low = np.random.default_rng(1).permutation(N).astype(np.uint64) * np.uint64(40503) + np.uint64(1)
    bits = (np.float64(1e-3).view(np.uint64) & np.uint64(0xffffffff00000000)) | low
    st.la_value[:] = bits.view(np.float64)
    assert len(set((bits >> np.uint64(32)).tolist())) == 1 and len(set(bits.tolist())) == N
    h = S.hip_context(prob, opts, tables)
    c = S.hip_context(prob, opts, tables)
    c.set_persistent(False)
    for x in (h, c):
        x.set_state(st, hist)
        x.step(T - 2)
    avail, launches, repairs = h.persistent_info()
    assert launches >= 1 and repairs == 0, (launches, repairs)
    assert c.persistent_info()[1] == 0
    hh = h.history()
    cm.assert_history_equal(hh, c.history(), exact_floats=True)
    cm.assert_state_equal(h.state(), c.state(), rtol=0)
    o = O.OracleContext(prob, opts, S.Tables(pairs=tab, Z=h.Z()))
    o.set_state(st, hist)
    o.step(T - 2)
    cm.assert_history_equal(hh, o.history())
    cm.assert_state_equal(h.state(), o.state())
    # the ties were met and decided both ways: tied chains swapped, and not every tied pair did
    x = hh.exchanged[2:] != 0
    assert x.any() and not x.all()
