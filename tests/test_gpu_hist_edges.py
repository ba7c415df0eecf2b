"""smm_get_histogram and smm_get_profile on the device with draws that ride the bin edges (include/smmhip.h; smm.jl_amd/csrc/smm_hist.hpp:
hist_bin's two corrections by one, hist_axis's two boundary rules, k_hist_edges' statuses and step == 0 branch; smm_profile.hpp's
k_prof_count, which bins with the same index).  The histories come from hist_craft.py (every edge of the table, its two neighbours, lo
and hi in every group; tests/test_hist_craft.py shows without a GPU that each checked column takes every branch), are installed with
smm_set_state into a twin context and read back; every output is equal, bit for bit, to the restatement (hist_ref.py / profile_ref.py)
over the read-back history.

  small bins : np = 2, bins 1 / 2 / 7 / 64, bins2 1 / 5 / 64, given and autodetected ranges, three selections, two windows, groups per
               chain (the store path), of four with an empty one (atomics into the u64 counts) and of all chains; the same with every
               count in the global counters (SMMHIP_HIST_LDS_BINS=1) and with one group per batch (SMMHIP_STATS_SCRATCH=1).
  batches    : np = 50, every parameter its own range: bins = 64 (kb = 50), 1000 (kb = 5: ten batches), 80 pairs at bins2 = 8.
  LDS limits : the shipped library at bins = 4096 (kb = 1), 5290 / 5291 and bins2 = 123 / 124 (the last in LDS and the first past it),
               and bins = 65536.
  statuses   : 2 from data and from a given range, 3 with the draws on the repeated edges in 1-D and as the axis of a pair, a given
               range of denormal width, (-0.0, 0.0), lo == hi at 1e17.
  profile    : n equal to the histogram's counts and everything equal to profile_ref on a small history and on the np = 50 one, in
               the LDS form and with the segments in global memory."""
import numpy as np
import pytest

import common as cm
import hist_craft as HC
import hist_ref as HR
import profile_ref as PR
import test_gpu_profile as TP
from test_gpu_reducer_caps import crafted_twin, seamed

pytestmark = pytest.mark.gpu

LDS_BYTES = 62 << 10             # smm_hist.hpp: HIST_LDS_BYTES
# smm_reducers_host.hpp, smm_get_histogram: lds1 = 12 B + 8 <= HIST_LDS_BYTES, lds2 = 16 (B2 + 1) + 4 B2 B2 <= HIST_LDS_BYTES
BINS_LDS, BINS2_LDS = 5290, 123  # the last bins / bins2 that count in LDS
assert 12 * BINS_LDS + 8 <= LDS_BYTES < 12 * (BINS_LDS + 1) + 8
assert 16 * (BINS2_LDS + 1) + 4 * BINS2_LDS ** 2 <= LDS_BYTES < 16 * (BINS2_LDS + 2) + 4 * (BINS2_LDS + 1) ** 2
assert LDS_BYTES // (12 * 4096 + 8) == 1 and LDS_BYTES // (12 * 1000 + 8) == 5 and LDS_BYTES // (12 * 64 + 8) >= 50   # kb


def check(h, back, want, t0, t1, sel, groups, bins, rng, pairs, bins2, n_groups):
    """the device against the restatement, computed once per call (want: the cache of the history)"""
    key = (t0, t1, sel, None if groups is None else groups.tobytes(), bins, None if rng is None else rng.tobytes(), tuple(pairs), bins2, n_groups)
    if key not in want:
        want[key] = HR.histogram_from_history(back, t0, t1, sel, groups, bins, rng, pairs, bins2, n_groups=n_groups)
    got = h.histogram(t0, t1, sel, groups, bins, rng, pairs, bins2, n_groups=n_groups)
    HR.assert_histogram_equal(got, want[key], auto=rng is None)
    return got


# --- small bins ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small(S):
    """case -> the twin holding hist_craft.small_history of the case, made on first use, with the cache of its expected results"""
    prob, opts = cm.serial_normal(N=HC.SMALL_N, T=HC.SMALL_T, ns=100)
    made = {}

    def get(case):
        if case not in made:
            h, state, crafted, back = crafted_twin(S, prob, opts, HC.SMALL_T, lambda c: HC.small_history(c, case))
            made[case] = dict(h=h, state=state, crafted=crafted, back=back, want={}, prob=prob, opts=opts)
        return made[case]
    return get


def check_small(d, h, case):
    for _, groups, G, sel, t0, t1, bins, bins2, rng in HC.small_calls(case):
        got = check(h, d["back"], d["want"], t0, t1, sel, groups, bins, rng, HC.SMALL_PAIRS, bins2, G)
        assert (got["status"] == 0).all()
        if rng is None:                                    # the data's min and max are the ranges the groups were built on
            for g in np.flatnonzero(got["count"] > 0):
                assert np.array_equal(np.stack([got["lo"][g], got["hi"][g]], axis=1), HC.small_ranges(case, g))
    cm.assert_history_equal(h.history(0, HC.SMALL_T), d["back"], exact_floats=True)


@pytest.mark.parametrize("case", HC.SMALL_CASES)
def test_small_bins_in_lds(small, case):
    d = small(case)
    check_small(d, d["h"], case)


@pytest.mark.parametrize("case", HC.SMALL_CASES)
def test_small_bins_in_the_global_counters(S, small, hooks, monkeypatch, case):
    d = small(case)
    check_small(d, seamed(S, monkeypatch, d["prob"], d["opts"], d["state"], d["crafted"], HIST_LDS_BINS=1), case)


@pytest.mark.parametrize("case", HC.SMALL_CASES)
def test_small_bins_one_group_per_batch(S, small, hooks, monkeypatch, case):
    d = small(case)
    check_small(d, seamed(S, monkeypatch, d["prob"], d["opts"], d["state"], d["crafted"], STATS_SCRATCH=1), case)


# --- parameter and pair batches at np = 50 ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def wide(S):
    from smm_jl_amd.workloads import build_problem
    prob, opts = build_problem("c5", HC.WIDE_N, HC.WIDE_N, 0, HC.WIDE_T, 0)
    assert prob.np == HC.WIDE_NP
    h, state, crafted, back = crafted_twin(S, prob, opts, HC.WIDE_T, HC.wide_history)
    return dict(h=h, state=state, crafted=crafted, back=back, want={}, prob=prob, opts=opts)


@pytest.mark.parametrize("sel", HC.SELECTIONS)
def test_np50_parameter_and_pair_batches(wide, sel):
    h, back = wide["h"], wide["back"]
    t0, t1 = HC.WIDE_WINDOW
    for groups, G in HC.WIDE_GROUPS:
        got = check(h, back, wide["want"], t0, t1, sel, groups, 64, HC.WIDE_RANGE, HC.WIDE_PAIRS, 8, G)     # kb = 50; 80 pairs: two batches
        assert (got["status"] == 0).all() and (got["hist"].sum(axis=2) < got["count"][:, None]).all()      # (rows one ulp outside)
        check(h, back, wide["want"], t0, t1, sel, groups, 1000, HC.WIDE_RANGE, (), None, G)                 # kb = 5: ten batches
    cm.assert_history_equal(h.history(0, HC.WIDE_T), back, exact_floats=True)


# --- the shipped library's LDS limits ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bins", sorted(HC.LIMIT_CASES))
def test_shipped_library_at_its_lds_limits(S, bins):
    assert set(HC.LIMIT_CASES) == {4096, BINS_LDS, BINS_LDS + 1, 65536} and HC.LIMIT_CASES[4096][1:] == (BINS2_LDS, BINS2_LDS + 1)
    prob, opts = cm.serial_normal(N=HC.LIMIT_N, T=HC.LIMIT_T, ns=100)
    h, _, _, back = crafted_twin(S, prob, opts, HC.LIMIT_T, lambda c: HC.limit_history(c, bins))
    want = {}
    for sel in HC.SELECTIONS:
        got = check(h, back, want, 0, HC.LIMIT_T, sel, None, bins, HC.LIMIT_RANGE, (), None, 1)
        assert (got["status"] == 0).all() and (got["hist"].sum(axis=2) < got["count"][:, None]).all()
        for bins2 in HC.LIMIT_CASES[bins][1:]:
            check(h, back, want, 0, HC.LIMIT_T, sel, None, 7, HC.LIMIT_RANGE, HC.SMALL_PAIRS, bins2, 1)
    cm.assert_history_equal(h.history(0, HC.LIMIT_T), back, exact_floats=True)


# --- statuses and degenerate tables --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["lds", "global"])
def test_statuses_and_degenerate_tables(S, request, monkeypatch, form):
    prob, opts = cm.serial_normal(N=HC.SMALL_N, T=HC.SMALL_T, ns=100)
    if form == "global":
        request.getfixturevalue("hooks")
    h, state, crafted, back = crafted_twin(S, prob, opts, HC.SMALL_T, HC.degenerate_history)
    if form == "global":
        h = seamed(S, monkeypatch, prob, opts, state, crafted, HIST_LDS_BINS=1)
    g, want = HC.DEGENERATE_GROUPS, {}
    for sel in HC.SELECTIONS:
        got = check(h, back, want, 0, HC.SMALL_T, sel, g, 64, None, HC.SMALL_PAIRS, 4, 4)
        assert got["status"].tolist() == [[2, 3], [3, 0], [3, 0], [3, 0]]                      # (by design: tests/test_hist_craft.py)
        assert (got["hist"][1, 0] == 0).all() and got["hist2"][1, 0].sum() == got["count"][1]   # status 3: no count, but cells
        check(h, back, want, 5, 50, sel, np.arange(HC.SMALL_N, dtype=np.int32), 64, None, HC.SMALL_PAIRS, 4, HC.SMALL_N)
        for rng, st in HC.DEGENERATE_RANGES:
            for bins, bins2 in HC.DEGENERATE_BINS:
                got = check(h, back, want, 0, HC.SMALL_T, sel, g, bins, rng, HC.SMALL_PAIRS, bins2, 4)
                assert (got["status"] == st[bins]).all()
    cm.assert_history_equal(h.history(0, HC.SMALL_T), back, exact_floats=True)


# --- the profile on the same histories ------------------------------------------------------------------------------------------------

def profile_small(d, h):
    groups, G = HC.GROUPINGS["four"]
    for sel in (0, 1, 2):
        for (t0, t1), (bins, bins2) in zip(HC.SMALL_WINDOWS, ((64, 5), (7, 64))):
            got = TP.check(h, d["back"], t0, t1, sel, groups, bins, HC.SMALL_GIVEN, HC.SMALL_PAIRS, bins2, n_groups=G)
            assert (got["n_scored"] == got["n"]).all() and (got["n"] > 0).sum() > bins                     # every row scored
        TP.check(h, d["back"], 0, HC.SMALL_T, sel, None, 2, HC.SMALL_GIVEN, HC.SMALL_PAIRS, 1)


def profile_wide(d, h):
    groups, G = HC.WIDE_GROUPS[1]
    for sel in (0, 1, 2):
        TP.check(h, d["back"], *HC.WIDE_WINDOW, sel, groups, 64, HC.WIDE_RANGE, HC.WIDE_PAIRS[:12], 8, n_groups=G, moments=False)


def test_profile_on_edge_riding_rows_in_lds(small, wide):
    profile_small(small("given"), small("given")["h"])
    profile_wide(wide, wide["h"])


def test_profile_on_edge_riding_rows_in_global_memory(S, small, wide, hooks, monkeypatch):
    for d, run in ((small("given"), profile_small), (wide, profile_wide)):
        run(d, seamed(S, monkeypatch, d["prob"], d["opts"], d["state"], d["crafted"], HIST_LDS_BINS=1))
