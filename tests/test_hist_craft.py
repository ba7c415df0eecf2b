"""The design of hist_craft.py's histories, checked on the restatement alone (hist_ref.py) and against numpy: for every (case, group,
parameter, selection, window, bins) that tests/test_gpu_hist_edges.py hands to the device, the selected column takes every branch of
the uniform-bins index that the range can take at all (the clamp from i == bins, the step down, the step up), the pair of parameters
takes both steps at every bins > 1, and every pair's cells see draws on e[B], on interior edges and one ulp below an edge; and
hist_ref equals np.histogram / np.histogram2d on those very columns.  Without this the GPU test could pass vacuously.  CPU only."""
import numpy as np
import pytest

import hist_craft as HC
import hist_ref as HR
import profile_ref as PR


def check_column(x, rng, want_range, bins, outside, tag):
    """the 1-D conditions on one selected column; returns (stepped down, stepped up)"""
    lo, hi, st = HR.outer_edges(x, rng)
    assert st == 0 and (lo, hi) == tuple(want_range), tag
    c = HC.branch_counts(x, lo, hi, bins)
    can_down, can_up = HC.fires(lo, hi, bins)
    assert c["clamped"] >= 1, tag
    assert (c["down"] >= 1) == can_down and (c["up"] >= 1) == can_up, (tag, c)
    assert not (bins == 1 and (can_down or can_up))
    if outside:
        assert c["below"] >= 1 and c["above"] >= 1, tag
    else:
        assert c["below"] == c["above"] == c["nan"] == 0, tag
    e = HR.linspace(lo, hi, bins)
    n, we = np.histogram(x, bins, (lo, hi))
    assert np.array_equal(HR.hist1d(x, lo, hi, e, bins), n) and np.array_equal(e, we), tag
    i = HC.branches(x, lo, hi, bins)["index"]
    assert np.array_equal(np.bincount(i[i >= 0], minlength=bins), n), tag
    return c["down"] >= 1, c["up"] >= 1


def check_cells(x, y, ra, rb, B, same, tag):
    ex, ey = HR.linspace(ra[0], ra[1], B), HR.linspace(rb[0], rb[1], B)
    c = HC.cell_counts(x, y, ex, ey, B)
    for ax in "xy":
        assert c[ax + "_last"] >= 1 and c[ax + "_below"] >= 1 and (B == 1 or c[ax + "_inner"] >= 1), (tag, c)
    H = np.histogram2d(x, y, B, [tuple(ra), tuple(rb)])[0]
    assert np.array_equal(HR.hist2d(x, y, ex, ey, B), H), tag
    if same:
        assert H.sum() == np.trace(H)


@pytest.mark.parametrize("case", HC.SMALL_CASES)
def test_small_cases_take_every_branch_and_match_numpy(case):
    h = HC.small_history(PR.zeroed_history(HC.SMALL_T, HC.SMALL_N, 2, 2), case)
    given = case == "given"
    assert len(np.unique(h.value)) == h.value.size and np.isfinite(h.value).all()
    seen_bins, seen_bins2 = set(), set()
    for gname, groups, G, sel, t0, t1, bins, bins2, rng in HC.small_calls(case):
        cols = HR.columns(h, t0, t1, HR.SELECT[sel], groups, G)
        seen_bins.add(bins), seen_bins2.add(bins2)
        for g, x in enumerate(cols):
            tag = (case, gname, g, sel, t0, bins, bins2)
            if x.shape[1] == 0:
                assert gname == "four" and g == 3
                continue
            R = HC.small_ranges(case, g)
            fired = [check_column(x[k], None if rng is None else rng[k], R[k], bins, given, tag + (k,)) for k in range(2)]
            if bins > 1:
                assert any(d for d, _ in fired) and any(u for _, u in fired), tag      # the pair of ranges takes both steps
            for a, b in HC.SMALL_PAIRS:
                check_cells(x[a], x[b], R[a], R[b], bins2, a == b, tag + (a, b))
            if given and gname == "all" and sel == "all" and t0 == 0:
                assert np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(x).any()
    assert seen_bins == set(HC.SMALL_BINS) and seen_bins2 == set(HC.SMALL_BINS2)
    if case.startswith("auto"):                                # groups and parameters differ in their ranges
        groups, G = HC.GROUPINGS[case[5:]]
        R = [tuple(map(tuple, HC.small_ranges(case, g))) for g in range(min(G, len(HC.RANGE_PAIRS)))]
        assert len(set(R)) == len(R) and all(r[0] != r[1] for r in R)
    else:
        st = HR.columns(h, 0, HC.SMALL_T, 2, *HC.GROUPINGS["chain"])
        assert np.isnan(st[1][:, :3]).all() and np.isnan(st[9][:, :3]).all()       # state rows that do not exist yet


def test_range_pairs_as_the_docstring_says():
    for i, (r0, r1) in enumerate(HC.RANGE_PAIRS):
        for b in (2, 7, 64):
            assert HC.fires(*r0, b)[0]
        assert HC.fires(*r1, 2)[1] and HC.fires(*r1, 64)[1]
        assert HC.fires(*r0, 7)[1] != (i in (1, 5)) and (i not in (1, 5) or HC.fires(*r1, 7)[1])
        assert HC.fires(*r0, 1) == HC.fires(*r1, 1) == (False, False)
    assert not HC.fires(-1 / 3, 2 / 3, 64)[1] and not HC.fires(0.7, 1.6, 64)[0]
    # the issue's probe: the counts over linspace edges +- one ulp
    for (lo, hi, b), want in (((-0.7, 0.9, 64), (37, 5)), ((-0.7, 0.9, 4096), (2303, 561)), ((-0.7, 0.9, 65536), (36863, 9009)),
                              ((-1 / 3, 2 / 3, 7), (3, 3))):
        c = HC.branch_counts(HC.riders(lo, hi, b, True), lo, hi, b)
        assert (c["down"], c["up"]) == want and c["below"] == c["above"] == 1 and c["clamped"] == 1


def test_wide_history_every_parameter_and_pair():
    h = HC.wide_history(PR.zeroed_history(HC.WIDE_T, HC.WIDE_N, HC.WIDE_NP, 2))
    R = HC.WIDE_RANGE
    assert len({tuple(r) for r in R}) == HC.WIDE_NP
    t0, t1 = HC.WIDE_WINDOW
    for groups, G in HC.WIDE_GROUPS:
        for sel in HC.SELECTIONS:
            cols = HR.columns(h, t0, t1, HR.SELECT[sel], groups, G)
            for g, x in enumerate(cols):
                for bins in (64, 1000):
                    fired = [check_column(x[k], R[k], R[k], bins, True, (G, g, sel, bins, k)) for k in range(HC.WIDE_NP)]
                    assert sum(d for d, _ in fired) >= 10 and sum(u for _, u in fired) >= 10
                for a, b in HC.WIDE_PAIRS[:51]:
                    check_cells(x[a], x[b], R[a], R[b], 8, a == b, (G, g, sel, a, b))


@pytest.mark.parametrize("bins", sorted(HC.LIMIT_CASES))
def test_limit_histories(bins):
    h = HC.limit_history(PR.zeroed_history(HC.LIMIT_T, HC.LIMIT_N, 2, 2), bins)
    R = HC.LIMIT_RANGE
    for sel in HC.SELECTIONS:
        x = HR.columns(h, 0, HC.LIMIT_T, HR.SELECT[sel], np.zeros(HC.LIMIT_N, np.int32), 1)[0]
        for b in HC.LIMIT_CASES[bins]:
            if b > 1000:
                fired = [check_column(x[k], R[k], R[k], b, True, (bins, sel, b, k)) for k in range(2)]
                assert any(d for d, _ in fired) and any(u for _, u in fired)
                if sel == "all" and bins != 65536:             # the whole table, but for what the core rows overwrote
                    for k in range(2):
                        c = HC.branch_counts(x[k], R[k][0], R[k][1], b)
                        full = HC.branch_counts(HC.riders(R[k][0], R[k][1], b, True), R[k][0], R[k][1], b)
                        assert c["down"] >= full["down"] and c["up"] >= full["up"]
            else:
                for a, c in HC.SMALL_PAIRS:
                    check_cells(x[a], x[c], R[a], R[c], b, a == c, (bins, sel, b, a, c))


def test_degenerate_history_statuses_against_numpy():
    h = HC.degenerate_history(PR.zeroed_history(HC.SMALL_T, HC.SMALL_N, 2, 2))
    g = HC.DEGENERATE_GROUPS
    for sel in HC.SELECTIONS:
        r = HR.histogram_from_history(h, 0, HC.SMALL_T, sel, g, 64, None, HC.SMALL_PAIRS, 4)
        cols = HR.columns(h, 0, HC.SMALL_T, HR.SELECT[sel], g, 4)
        assert r["status"].tolist() == [[2, 3], [3, 0], [3, 0], [3, 0]]
        assert (r["hist"][0] == 0).all() and (r["hist"][1, 0] == 0).all()
        assert (r["hist2"][0, 2] == 0).all()                       # status 2 on an axis: no cell
        assert r["hist2"][1, 0].sum() == r["count"][1] and r["hist2"][1, 2].sum() == r["count"][1]   # status 3 on an axis: counted
        for gi, k in ((1, 0), (2, 0), (0, 1)):                     # numpy raises where the restatement says 3
            with pytest.raises(ValueError):
                np.histogram(cols[gi][k], 64)
        e = r["edges"][1, 0]
        assert np.any(e[:-1] == e[1:]) and np.isin(cols[1][0], e).all()          # the draws equal the repeated edges
        for gi, (a, b) in ((1, (0, 1)), (1, (1, 0)), (1, (0, 0)), (2, (0, 1)), (3, (0, 1)), (3, (1, 0))):
            H, xe, ye = np.histogram2d(cols[gi][a], cols[gi][b], 4)
            p = HC.SMALL_PAIRS.index((a, b))
            assert np.array_equal(r["hist2"][gi, p], H) and np.array_equal(r["edges2"][gi, a], xe) and np.array_equal(r["edges2"][gi, b], ye)
        assert np.array_equal(r["hist"][1, 1], np.histogram(cols[1][1], 64)[0])
        c = HC.branch_counts(cols[1][1], r["lo"][1, 1], r["hi"][1, 1], 64)
        assert c["down"] >= 1 and c["up"] >= 1 and c["clamped"] >= 1
        # the given ranges of the GPU test: status 2, the denormal width (step == 0), (-0.0, 0.0), lo == hi at 1e17
        for rng, want_st in HC.DEGENERATE_RANGES:
            for bins, bins2 in HC.DEGENERATE_BINS:
                r = HR.histogram_from_history(h, 0, HC.SMALL_T, sel, g, bins, rng, HC.SMALL_PAIRS, bins2)
                st = want_st[bins]
                assert (r["status"] == st).all(), (rng, bins)
                for gi in range(4):
                    for k in range(2):
                        if r["status"][gi, k] == 0:
                            n, e = np.histogram(cols[gi][k], bins, tuple(rng[k]))
                            assert np.array_equal(r["hist"][gi, k], n) and np.array_equal(r["edges"][gi, k], e)
                    if st[0] != 2:
                        H = np.histogram2d(cols[gi][0], cols[gi][1], bins2, [tuple(rng[0]), tuple(rng[1])])[0]
                        assert np.array_equal(r["hist2"][gi, 0], H)
    lo, hi = HC.DENORMAL
    assert (hi - lo) / 64 == 0 and (hi - lo) / 4 != 0                # linspace's step == 0 branch in 1-D, the other in 2-D
    r = HR.histogram_from_history(h, 0, HC.SMALL_T, "all", g, 64, np.array([HC.DENORMAL, HC.DENORMAL]), HC.SMALL_PAIRS, 4)
    x = HR.columns(h, 0, HC.SMALL_T, 0, g, 4)
    assert len(np.unique(x[2][0])) == 4 and ((x[2][0] >= lo) & (x[2][0] <= hi)).all()       # draws on all four representable values
    assert (r["hist"] == 0).all() and r["hist2"][2, 2].sum() == r["count"][2] and (r["hist2"][2, 2] > 0).sum() >= 3
    assert 0 < r["hist2"][3, 1].sum() < r["count"][3]                                        # (parameter 1 of group 3: some outside)
