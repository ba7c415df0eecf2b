"""The design of trace_craft.py's history, checked on the restatement alone (trace_ref.py) and against numpy: the groups' sizes and
scattered member lists, the best member of every (iteration, group) where the table says and its ties across the seam or a multiple of
256 positions apart, an iteration with count 0 and one with count equal to the size in every group, flags on both sides of every
seam, state rows without a state in both blocks, and TR.column_stats against a plain sort on the tie columns.  CPU only."""
import numpy as np
import pytest

import profile_ref as PR
import trace_craft as TC
import trace_ref as TR


@pytest.fixture(scope="module")
def hist():
    return TC.crafted(PR.zeroed_history(TC.T, TC.N, 2, 2))


@pytest.fixture(scope="module")
def full(hist):
    return TR.trace_from_history(hist, 0, TC.T, 1, "all", True, TC.GROUPS, TC.PROBS, n_groups=TC.N_GROUPS)


def test_groups_sizes_and_scattered_members():
    assert np.bincount(TC.GROUPS[TC.GROUPS >= 0], minlength=TC.N_GROUPS).tolist() == list(TC.SIZES) and (TC.GROUPS == -1).sum() == 253
    assert TC.SIZES[:2] == (TC.LDS_N + 1, TC.LDS_N) and set(TC.SIZES[2:6]) == {2 * TC.BLOCK + 1, TC.BLOCK + 1, TC.BLOCK, TC.BLOCK - 1}
    for mem in TC.MEMBERS[:6]:
        assert (np.diff(mem) > 1).sum() > len(mem) // 4 and (np.diff(mem) == 1).any()      # neither contiguous nor strided


def test_best_member_where_intended_and_ties_at_the_seams(hist, full):
    for g, mem in enumerate(TC.MEMBERS):
        m = len(mem)
        for t in range(TC.T):
            p = TC.best_position(t, m)
            if m == 0:
                assert full["best_chain"][t, g] == 0 and np.isnan(full["best_value"][t, g])
                continue
            if p is None:
                continue
            v = hist.value[t, mem]
            assert full["best_chain"][t, g] == mem[p] + 1, (t, g)
            assert np.array_equal(full["best_value"][t, g], v[p], equal_nan=True)
            tie = np.flatnonzero(np.isnan(v) if np.isnan(v[p]) else v == v[p])
            assert tie[0] == p
            if m > TC.BLOCK + 1:
                if t == 0:
                    assert tie.tolist() == [TC.BLOCK - 1, TC.BLOCK]                           # lane 255 of one block, lane 0 of the next
                if t in (3, 4):
                    assert len(tie) >= 2 and ((tie - p) % TC.BLOCK == 0).all()                # the same lane of later blocks
                if t == 2:
                    assert p >= TC.BLOCK and np.nanmin(v) == v[10] == -7.0                    # NaN in a later block beats the first's minimum
                if t in (1, 5):
                    assert tie[-1] == m - 1
    assert full["best_chain"][4, 0] == TC.MEMBERS[0][7] + 1 and (hist.value[4, TC.MEMBERS[0]] == -5.0).sum() == 3


def test_counts_and_flags_across_blocks(hist):
    acc = TR.trace_from_history(hist, 0, TC.T, 1, "accepted", False, TC.GROUPS, (), n_groups=TC.N_GROUPS)
    for g, mem in enumerate(TC.MEMBERS):
        m = len(mem)
        want = [0, int(m > 255), int(m > 256), int(m > 0), max(0, m - 256), m]
        assert acc["count"][:, g].tolist() == want
        if m:
            assert 0 in want and want[5] == m                                                  # a count of 0 and one of the whole group
            assert np.isnan(acc["mean"][0, g]).all() and acc["best_chain"][0, g] >= 1           # count 0: NaN means, the best still given
        ex, bad = hist.exchanged[:, mem] != 0, hist.status[:, mem] < 0
        assert acc["n_exchanged"][:, g].tolist() == ex.sum(axis=1).tolist() and acc["n_failed"][:, g].tolist() == bad.sum(axis=1).tolist()
        assert acc["n_accepted"][:, g].tolist() == ((hist.accepted[:, mem] != 0) & ~ex).sum(axis=1).tolist()
        for s in range(TC.BLOCK, m, TC.BLOCK):                                                  # flags on both sides of every seam it has
            if s in (256, 512, 8192):
                assert ex[:, s - 1].any() and ex[:, s].any() and bad[:, s - 1].any() and bad[:, s].any(), (g, s)
        if m > TC.BLOCK:
            assert (acc["n_exchanged"][:, g] >= 1).all() and (acc["n_accepted"][5, g] < m)
    first = acc["count"][4]                                                                     # nobody of the first block selected
    assert first[0] == 8193 - 256 and first[4] == 0 and first[3] == 1


def test_state_rows_without_a_state_in_both_blocks(hist):
    a = TR.state_rows(hist.accepted, TC.T)
    for g in (2, 3):
        mem = TC.MEMBERS[g]
        for t in (0, 1) if g == 3 else (0, 1, 2, 3):            # (the 257th member is the one accepted at t = 2)
            assert (a[t, mem[:TC.BLOCK]] == -1).any() and (a[t, mem[TC.BLOCK:]] == -1).any()
        assert (a[1, mem] >= 0).sum() == 1 and (a[5, mem] == 5).all()
    st = TR.trace_from_history(hist, 0, TC.T, 1, "state", False, TC.GROUPS, TC.PROBS, n_groups=TC.N_GROUPS)
    assert (st["count"] == np.array(TC.SIZES)).all() and np.isnan(st["mean"][:4, :6]).all() and np.isfinite(st["mean"][5, :7]).all()


def plain_stats(x, probs):
    """mean aside: the median and the linear quantiles from a plain sort"""
    s, m = np.sort(x), len(x)
    med = s[m // 2] if m & 1 else (s[m // 2 - 1] + s[m // 2]) / 2.0
    q = []
    for p in probs:
        r = p * (m - 1)
        lo = int(np.floor(r))
        hi = min(lo + 1, m - 1)
        q.append(s[lo] + (s[hi] - s[lo]) * (r - lo))
    return med, q


def test_tie_columns_against_a_plain_sort(hist, full):
    for g in (0, 1):
        mem = TC.MEMBERS[g]
        m = len(mem)
        for t in range(TC.T):
            two, same, distinct = hist.params[t, 1, mem], hist.sim_moments[t, 0, mem], hist.params[t, 0, mem]
            assert abs(int((two == -0.5).sum()) - int((two == 1.5).sum())) == m % 2 and len(np.unique(distinct)) == m and (same == 3.25).all()
            assert (np.diff(distinct) < 0).any() and (np.diff(distinct) > 0).any()
            for x, s in ((two, 1), (same, 3), (distinct, 0)):
                mu, var, med, q = TR.column_stats(x, TC.PROBS)
                pm, pq = plain_stats(x, TC.PROBS)
                assert med == pm and np.allclose(q, pq, rtol=1e-15, atol=0) and q[0] == x.min() and q[3] == x.max()
                assert full["median"][t, g, s] == med and np.array_equal(full["quantile"][:, t, g, s], q) and full["mean"][t, g, s] == mu
            assert full["var"][t, g, 3] == 0.0
            if m % 2 == 0:
                assert full["median"][t, g, 1] == 0.5                                           # the tie straddles the median ranks
        nan_col = hist.sim_moments[2, 1, mem]
        assert np.isnan(nan_col).sum() == 1 and np.isnan(nan_col[-1])
        assert np.isnan(full["mean"][2, g, 4]) and np.isnan(full["quantile"][:, 2, g, 4]).all() and np.isfinite(full["mean"][3, g, 4])
    assert np.isnan(full["mean"][2, :7, 2]).sum() == 4 and np.isnan(full["mean"][3, :6, 2]).all()   # the NaN values reach the value series
