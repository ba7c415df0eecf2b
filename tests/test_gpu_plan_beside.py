"""The next plan window made BESIDE the persistent chain kernel (k_exch_plan_bg on a second stream: smm.jl_amd/csrc/smm_lookahead.hpp,
plan_beside_into in smm_launch_host.hpp).  Scheduling, not arithmetic: every history here is held to the bit against the same problem
with the path switched off (SMMHIP_PLAN_AHEAD=0 of the test build: k_exch_plan on the main stream) and against the per-iteration kernels
(set_persistent(False)), and against the oracle within the suite's standing tolerance for the CPU's libm (bookkeeping exact).  The
tables themselves — k_exch_plan_bg's of a window against k_exch_plan's for the same iterations — are read through a seam of the test build.
Replaces nothing of the reference: exchangeMoves! (AlgoBGP.jl:647-716) draws its pairs from (seed, iteration) alone, which is what makes
a window's plan independent of the chains' state."""
import ctypes as C

import numpy as np
import pytest

import common as cm
import cone_craft as CC

pytestmark = pytest.mark.gpu

NS = 64
CONE_HDRW, CONE_SUBW, CONE_GCAP, LV_OFFP = 9, 32 * 64, 512, 40


def contexts(S, O, monkeypatch, prob, opts, tab=None, cap=None, beside=True):
    """the context that plans beside, the same with the path off, the per-iteration kernels, the oracle"""
    if cap is not None:
        monkeypatch.setenv("SMMHIP_PLAN_CAP", str(cap))
    h = S.hip_context(prob, opts, tab)
    monkeypatch.setenv("SMMHIP_PLAN_AHEAD", "0")
    off = S.hip_context(prob, opts, tab)
    monkeypatch.delenv("SMMHIP_PLAN_AHEAD")
    c = S.hip_context(prob, opts, tab)
    c.set_persistent(False)
    t = tab if tab is not None else S.Tables()
    o = O.OracleContext(prob, opts, S.Tables(probs_acc=t.probs_acc, prop_normals=t.prop_normals, pairs=t.pairs, Z=h.Z()))
    assert h.plan_beside_info()[0] == beside, h.describe()
    assert not off.plan_beside_info()[0] and off.plan_beside_info()[1] == 0
    return h, off, c, o


def same(h, off, c, o, atol=0.0, exchanged=True, repairs=False):
    hh = h.history()
    for other in (off, c):
        cm.assert_history_equal(hh, other.history(), exact_floats=True)
        cm.assert_state_equal(h.state(), other.state(), rtol=0)
    cm.assert_history_equal(hh, o.history(), atol=atol)
    cm.assert_state_equal(h.state(), o.state(), atol=atol)
    if exchanged:
        assert (hh.exchanged != 0).any()
    # no launch was repaired — or (a cone past its caps: the launch reports the iteration, which is replayed on the per-iteration form) as
    # many as with the plan on the main stream
    assert h.persistent_info()[2] == off.persistent_info()[2] and (repairs or h.persistent_info()[2] == 0)


@pytest.mark.parametrize("N", [64, 256])
@pytest.mark.parametrize("steps", [[23], [2, 7, 1, 13], [5, 5, 5, 5, 3], [9, -1, 14]])
def test_window_seams(S, O, monkeypatch, hooks, N, steps):
    # windows of 5 iterations; steps that cross them, end exactly on a window's end, and a read-back of the history in the middle (-1)
    prob, opts = cm.serial_normal(N=N, T=23, ns=500, seed=7)
    h, off, c, o = contexts(S, O, monkeypatch, prob, opts, cap=5)
    for n in steps:
        if n < 0:
            cm.assert_history_equal(h.history(), off.history(), exact_floats=True)
            continue
        for x in (h, off, c, o):
            x.step(n)
    same(h, off, c, o)
    beside, wb, wi = h.plan_beside_info()
    assert wb >= 1 and wi >= 1, (wb, wi)
    if steps == [23]:
        assert (wb, wi) == (5, 1), (wb, wi)   # [1,5] on the main stream; [5,9] [9,13] [13,17] [17,21] [21,23] beside
    assert h.persistent_info()[1] >= 1


def test_a_jump_back_finds_the_window_planned_ahead_useless(S, O, monkeypatch, hooks):
    prob, opts = cm.serial_normal(N=256, T=23, ns=NS, seed=11)
    h, off, c, o = contexts(S, O, monkeypatch, prob, opts, cap=5)
    a = S.hip_context(prob, opts)
    a.step(6)
    st, hist = a.state(), a.history()
    for x in (h, off, c):
        x.step(12)
        x.set_state(st, hist)
        x.step(17)
    o.step(23)
    same(h, off, c, o)
    assert h.plan_beside_info()[2] >= 2   # the first window and the one the jump asked for


def test_the_benchmarks_population_two_windows_beside_one_in_stream(S, O, monkeypatch, hooks):
    prob, opts = cm.serial_normal(N=4096, T=520, ns=NS)
    h, off, c, o = contexts(S, O, monkeypatch, prob, opts)
    for x in (h, off, c, o):
        x.step(520)
    same(h, off, c, o, atol=1e-13)   # (atol: tests/test_gpu_persist_loc.py, a moment within 1e-5 of zero)
    assert h.plan_beside_info() == (True, 2, 1)   # [1,256] in stream; [256,511] and [511,520] beside
    assert h.persistent_info()[1] >= 3


@pytest.mark.parametrize("family", ["key1", "key2", "wide1", "wide2", "pct1", "pct2"])
def test_every_capped_family(S, O, monkeypatch, hooks, family):
    N, T = 256, 14
    if family[-1] == "2":
        prob, opts = cm.serial_normal(N=N, T=T, ns=NS, seed=7)
    else:
        prob, opts = cm.general_normal(1, N=N, T=T, ns=NS)
    opts.min_improve[:] = 0.05 if family.startswith("wide") else 0.0
    if family.startswith("pct"):
        opts.min_improve[:] = np.random.default_rng(5).choice([0.0, 0.0, 0.002, 0.05, 0.5], N)
        opts.min_improve[0] = 0.0; opts.min_improve[1] = 0.05
    h, off, c, o = contexts(S, O, monkeypatch, prob, opts, cap=4)
    for x in (h, off, c, o):
        x.step(T)
    same(h, off, c, o)
    assert h.plan_beside_info()[1] >= 3
    assert "loc" in h.describe()["persistent"]


@pytest.mark.parametrize("table", ["chain31", "chain32", "tree_extra", "tree_cap32", "tree_past33"])
def test_injected_pairs(S, O, monkeypatch, hooks, table):
    # 31 levels: the lean walk's cap; 32: deep (no persistent form, hence nothing planned beside: the results are held all the same); a level
    # wider than 64 pairs; a cone of 32 sub-levels; one of 33 (cone_ok = 0: the iteration goes to the per-iteration form), planned by k_exch_plan_bg
    T = 12
    N = 80 if table.startswith("chain") else 320
    tabs = {"chain31": lambda: CC.chain_table(31), "chain32": lambda: CC.chain_table(32), "tree_extra": lambda: CC.tree_table(True),
            "tree_cap32": lambda: CC.tree_table(tail=27), "tree_past33": lambda: CC.tree_table(extra=True, tail=25)}
    prob, opts = cm.serial_normal(N=N, T=T, ns=NS, seed=7)
    tab = S.Tables(pairs=tabs[table]())
    h, off, c, o = contexts(S, O, monkeypatch, prob, opts, tab=tab, cap=4, beside=table != "chain32")
    for n in (3, 9):
        for x in (h, off, c, o):
            x.step(n)
    same(h, off, c, o, repairs=table == "tree_past33")
    if table != "chain32":
        assert h.plan_beside_info()[1] >= 1


def test_short_windows_entered_right_behind_a_large_populations_plan(S, O, monkeypatch, hooks):
    # windows of 3 iterations at 4096 chains and 64 shocks: a window's two chain iterations take tens of microseconds, its successor's plan
    # some 500 — the launch that enters a window finds its tables only because the main stream waits for the set's event
    prob, opts = cm.serial_normal(N=4096, T=16, ns=NS, seed=5)
    h, off, c, o = contexts(S, O, monkeypatch, prob, opts, cap=3)
    for n in (7, 9):
        for x in (h, off, c, o):
            x.step(n)
    same(h, off, c, o, atol=1e-13)
    assert h.plan_beside_info()[1] >= 4


def bg_edge(hooks):
    """the largest population (pairs = chains) whose plan the background kernel's LDS takes (plan_bg_fits through the seam of the test build)"""
    lib = hooks.load_hooks()
    lib.smm_debug_plan_beside_budget.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong)]
    out = (C.c_longlong * 7)()
    assert lib.smm_debug_plan_beside_budget(2, 4096, 4096, out) == 0
    return int(out[4])


@pytest.mark.parametrize("side", ["largest", "next"])
def test_the_size_edge_of_the_background_kernel(S, O, monkeypatch, hooks, side):
    # The LDS plan takes pair lists no longer than the population (select_forms: K <= N_global), and the locally numbered persistent form
    # takes at most 256 tiles: no context on a device of 256 compute units reaches the last size k_exch_plan_bg's LDS holds (some 4390 pairs;
    # an injected list cannot be longer than its population either).  The kernel is run there all the same, through the seam, on a context of
    # that size without a persistent form: its tables against k_exch_plan's where its three LDS layouts come within bytes of the request; one
    # chain more and the seam refuses the kernel, as creation would.  The context's own run (k_exch_plan in stream) is held to the bit as well.
    N = bg_edge(hooks) + (1 if side == "next" else 0)
    assert N > 4096
    T = 6
    monkeypatch.setenv("SMMHIP_PLAN_CAP", "2")
    prob, opts = cm.serial_normal(N=N, T=T, ns=NS, seed=7)
    h = S.hip_context(prob, opts)
    assert h.plan_beside_info() == (False, 0, 0) and h.describe()["plan"] == "lds"
    lib = hooks.load_hooks()
    lib.smm_debug_plan_into.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    lib.smm_debug_plan_tables.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int32)] + [C.c_void_p] * 8
    assert lib.smm_debug_plan_into(h._ctx, 0, 2, 0) == 0
    if side == "next":
        assert lib.smm_debug_plan_into(h._ctx, 1, 2, 1) != 0      # refused: the plan does not fit the background kernel
    else:
        assert lib.smm_debug_plan_into(h._ctx, 1, 2, 1) == 0
        for w in range(2):
            a, b = read_tables(lib, h._ctx, 0, w), read_tables(lib, h._ctx, 1, w)
            assert a["K"] == N and a["tiles"] == (N + 15) // 16 and a["ok"] == 1 and a["nlev"] >= 2, (a["K"], a["tiles"], a["ok"], a["nlev"])
            assert_tables_equal(a, b)
    o = O.OracleContext(prob, opts, S.Tables(Z=h.Z()))
    h.step(T); o.step(T)
    cm.assert_history_equal(h.history(), o.history(), atol=1e-13)


@pytest.mark.parametrize("N", [4096, 4112])
def test_the_size_edge(S, O, monkeypatch, hooks, N):
    # 4096 chains: the largest population on the locally numbered persistent form (256 tiles), planned beside; the next population of whole
    # tiles keeps the per-iteration kernels and k_exch_plan on the main stream
    prob, opts = cm.serial_normal(N=N, T=10, ns=NS, seed=3)
    h, off, c, o = contexts(S, O, monkeypatch, prob, opts, cap=4, beside=N == 4096)
    for x in (h, off, c, o):
        x.step(10)
    same(h, off, c, o, atol=1e-13)


# ---- the tables ------------------------------------------------------------------------------------------------------------------
def read_tables(lib, ctx, which, w):
    info = (C.c_int32 * 8)()
    assert lib.smm_debug_plan_tables(ctx, which, w, info, None, None, None, None, None, None, None, None) == 0
    K, tiles, Kp = info[4], info[5], info[6]
    d = dict(plan=np.zeros(K, np.uint64), lv_pairs=np.zeros(K, np.uint32), lv_off=np.zeros(K + 2, np.uint32), offp=np.zeros(LV_OFFP, np.uint32),
             pairs_p=np.zeros(max(Kp, 1), np.uint32), hdr=np.zeros((tiles, CONE_HDRW), np.uint32), cpairs=np.zeros((tiles, CONE_SUBW), np.uint32),
             gather=np.zeros((tiles, CONE_GCAP), np.uint16))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.smm_debug_plan_tables(ctx, which, w, info, p(d["plan"]), p(d["lv_pairs"]), p(d["lv_off"]), p(d["offp"]), p(d["pairs_p"]), p(d["hdr"]),
                                     p(d["cpairs"]), p(d["gather"])) == 0
    d.update(t0=info[0], w=info[1], nlev=info[2], ok=info[3], K=K, tiles=tiles, lean=info[7])
    return d


def assert_tables_equal(a, b):
    """header words and level offsets equal; each level's pair words as a multiset; each gather list as a set.  A cone's words are compared
    by runs of sub-levels that end with a part-filled one: a level of more than 64 pairs spans several sub-levels and which of its words
    land in which is as arbitrary as their order (LDS atomics in both kernels)."""
    K, nlev = a["K"], a["nlev"]
    assert (a["nlev"], a["ok"], a["K"], a["tiles"]) == (b["nlev"], b["ok"], b["K"], b["tiles"])
    assert np.array_equal(a["plan"], b["plan"])
    assert np.array_equal(a["lv_off"][:nlev], b["lv_off"][:nlev]) and a["lv_off"][K + 1] == b["lv_off"][K + 1] == nlev
    start = 0
    for l in range(nlev):
        end = int(a["lv_off"][l])
        assert np.array_equal(np.sort(a["lv_pairs"][start:end]), np.sort(b["lv_pairs"][start:end])), l
        start = end
    assert start == K
    assert a["offp"][33] == b["offp"][33] and a["offp"][34] == b["offp"][34]
    if a["lean"] and a["offp"][34]:
        assert np.array_equal(a["offp"][:nlev + 1], b["offp"][:nlev + 1])
        for l in range(nlev):
            s, e = int(a["offp"][l]), int(a["offp"][l + 1])
            assert np.array_equal(np.sort(a["pairs_p"][s:e]), np.sort(b["pairs_p"][s:e])), l
    if not a["ok"]:
        return
    assert np.array_equal(a["hdr"], b["hdr"])
    for tile in range(a["tiles"]):
        hw = a["hdr"][tile]
        nsub, g = int(hw[0] & 0xffff), int(hw[0] >> 16)
        counts = [int((hw[1 + s // 4] >> (8 * (s % 4))) & 0xff) for s in range(nsub)]
        run0 = 0
        for s in range(nsub):
            if counts[s] < 64 or s == nsub - 1:
                wa = np.concatenate([a["cpairs"][tile, 64 * x:64 * x + counts[x]] for x in range(run0, s + 1)])
                wb = np.concatenate([b["cpairs"][tile, 64 * x:64 * x + counts[x]] for x in range(run0, s + 1)])
                assert np.array_equal(np.sort(wa), np.sort(wb)), (tile, s)
                run0 = s + 1
        ga, gb = a["gather"][tile, :g], b["gather"][tile, :g]
        assert len(set(ga.tolist())) == g and set(ga.tolist()) == set(gb.tolist()), tile


@pytest.mark.parametrize("case", ["n256", "n4096", "n1000_wide", "tree_cap32", "tree_past33", "chain31"])
def test_the_background_kernels_tables_are_k_exch_plans(S, monkeypatch, hooks, case):
    T, tab, mi = 9, None, 0.0
    if case.startswith("n"):
        N = int(case[1:].split("_")[0])
        mi = 0.05 if case.endswith("wide") else 0.0
    else:
        N = 80 if case == "chain31" else 320
        tab = S.Tables(pairs={"tree_cap32": lambda: CC.tree_table(tail=27, T=T), "tree_past33": lambda: CC.tree_table(extra=True, tail=25, T=T),
                              "chain31": lambda: CC.chain_table(31, T=T)}[case]())
    monkeypatch.setenv("SMMHIP_PLAN_CAP", "3")
    prob, opts = cm.serial_normal(N=N, T=T, ns=NS, seed=7, min_improve=mi)
    h = S.hip_context(prob, opts, tab)
    assert h.plan_beside_info()[0]
    lib = hooks.load_hooks()
    lib.smm_debug_plan_into.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    lib.smm_debug_plan_tables.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int32)] + [C.c_void_p] * 8
    for t in (2, 7):
        assert lib.smm_debug_plan_into(h._ctx, 0, t, 0) == 0    # k_exch_plan into set 0
        assert lib.smm_debug_plan_into(h._ctx, 1, t, 1) == 0    # k_exch_plan_bg into set 1
        for w in range(3):
            a, b = read_tables(lib, h._ctx, 0, w), read_tables(lib, h._ctx, 1, w)
            assert a["t0"] == b["t0"] == t and a["w"] == b["w"] == 3
            assert a["nlev"] >= 1 and (a["ok"] == 1) == (case != "tree_past33"), (a["nlev"], a["ok"])
            assert_tables_equal(a, b)
