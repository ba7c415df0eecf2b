"""The crafted histories of adjust_craft.py held against adjust_ref.py without a GPU: every property the designs are made for is
asserted here on the restatement's output, recomputed from the history, so that tests/test_gpu_adjustment_edges.py cannot pass
vacuously.  crafted_exact: beta bit for bit, n_outside equal to the constructed counts, every class of (group, parameter), the values
on the bounds.  crafted_keys: theta* equal to theta, the six digit separations, the tie run's unequal weights, q = 1 and q = 2^20, the
targets around the run, the bandwidth on its run; adjust_ref.weighted_quantile against a Python loop in the IEEE total order.
crafted_seams: the chunk layout the batch seams are crossed with."""
import numpy as np
import pytest

import adjust_craft as AC
import adjust_ref as AR


def ref(h, prob_like, select, groups, tol, kernel, ridge, probs, n_groups=None, window=None):
    mom, w, lb, ub = prob_like
    t0, t1 = window or (0, h.value.shape[0])
    return AR.adjustment_from_history(h, t0, t1, select, groups, tol, kernel, None, ridge, probs, mom, w, lb, ub, n_groups=n_groups)


EXACT = (AC.EXACT_MOM, AC.EXACT_W, AC.EXACT_LB, AC.EXACT_UB)
KEYS = (np.array(AC.KEYS_MOM), np.ones(2), AC.KEYS_LB, AC.KEYS_UB)


@pytest.mark.parametrize("N,T", ((16, 512), (64, 512)))
def test_crafted_exact_gives_beta_and_the_bound_counts_bit_for_bit(N, T):
    h, info = AC.crafted_exact(N, T, seed=5)
    m = info["m"]
    assert m == N * T // 2 and m in (4096, 16384)
    for select in (0, 1, 2):
        r = ref(h, EXACT, select, info["groups"], 1.0, 0, 0.0, AC.EXACT_PROBS)
        assert r["status"].tolist() == [0, 0] and r["count"].tolist() == [m, m] and r["n_kept"].tolist() == [m, m]
        assert np.array_equal(AC.bits(r["beta"]), AC.bits(info["beta"]))
        assert np.array_equal(AC.bits(r["adj_mean"]), AC.bits(info["adj_mean"])) and (r["x_mean"] == 0).all()
        assert np.array_equal(r["n_outside"], info["n_outside"])
        assert np.array_equal(AC.bits(r["adj_quantile"]), AC.bits(info["quantile"]))
    # every class of (group, parameter), from the four values against the bounds
    lb, ub, v = AC.EXACT_LB[None, :, None], AC.EXACT_UB[None, :, None], info["values"]
    below, above = (v < lb).sum(axis=2), (v > ub).sum(axis=2)
    cls = np.where((below > 0) & (above > 0), "both", np.where(below > 0, "below", np.where(above > 0, "above", "none")))
    assert cls.tolist() == [list(c) for c in AC.EXACT_CLASS] and set(cls.ravel()) == {"below", "above", "both", "none"}
    assert np.array_equal(info["n_outside"], (below + above) * (m // 4))
    assert (np.diff(v, axis=2) > 0).all()
    on_lb, on_ub = AC.bits(v) == AC.bits(np.broadcast_to(lb, v.shape)), AC.bits(v) == AC.bits(np.broadcast_to(ub, v.shape))
    assert on_lb.any() and on_ub.any()                     # a value bitwise on lb and one on ub: they count as inside
    assert (on_lb | on_ub)[1, 0].sum() == 2 and info["n_outside"][1, 0] == 0
    n = info["n_outside"]
    assert all(len(set(n[g].tolist())) == 3 for g in range(2)) and (n[0] != n[1]).all()      # the counts differ between parameters and groups
    assert len(set(AC.EXACT_LB.tolist())) == 3 and len(set(AC.EXACT_UB.tolist())) == 3       # no two parameters share a bound
    # with the first parameter's lower bound in place of its own, a later parameter counts differently
    assert any(((v[g, j] < AC.EXACT_LB[0]) | (v[g, j] > AC.EXACT_UB[j])).sum() * (m // 4) != n[g, j] for g in range(2) for j in (1, 2))
    # the rows outside: in two waves of one workgroup and in two workgroups of the row pass, for every (group, parameter) that loses rows
    for g in range(2):
        for j in range(AC.EXACT_NP):
            rows = info["outside_rows"][g][j]
            assert len(rows) == n[g, j]
            if len(rows):
                wg, wave = rows // AC.ADJ_WG, rows // 64
                assert len(set(wg.tolist())) >= 2 and len(set(wave[wg == wg[0]].tolist())) >= 2
    # the waves of a workgroup hold unequal numbers of them somewhere: a count kept from one wave only is not a multiple of the rest
    rows = info["outside_rows"][0][1]
    per_wave = np.bincount(rows[rows < AC.ADJ_WG] // 64, minlength=4)
    assert len(set(per_wave.tolist())) > 1, per_wave


def keys_case(members, N=8, seed=9):
    h, info = AC.crafted_keys(N, seed)
    groups = np.full(N, -1, np.int32)
    groups[list(members)] = 0
    return h, info, groups


def recomputed(h, members, kernel, beta):
    """(theta* [m][2], q [m], kept [m]) of the pool of `members`, recomputed from the history and the reference's beta and bandwidth"""
    th = np.concatenate([h.params[:, :, c] for c in members])                    # [m][2]
    x = np.concatenate([h.sim_moments[:, :, c] for c in members]) - np.array(AC.KEYS_MOM)[None, :]
    d2 = AR.distances(x.T)
    om = AR.row_weights(d2, AR.bandwidth(d2, AC.KEYS_TOL), kernel)
    star = np.empty_like(th)
    for j in range(2):
        t = np.zeros(len(th))
        for k in range(2):
            t = t + x[:, k] * beta[k, j]
        star[:, j] = th[:, j] - t
    return star, AR.int_weights(om), om > 0, d2


@pytest.mark.parametrize("members", ((0,), (1, 2, 3), (0, 1, 2, 3, 4, 5)))
def test_crafted_keys_has_every_property_of_its_design(members):
    members = list(members)
    c = len(members)
    h, info, groups = keys_case(members)
    probs, want, marks = AC.keys_probs(info, members)
    assert len(probs) >= 7 and probs[0] == 0.0 and probs[1] == 1.0 and all(0.0 <= p <= 1.0 for p in probs)
    exp = AC.keys_expect(info, members)
    r = {k: ref(h, KEYS, 0, groups, AC.KEYS_TOL, k, AC.KEYS_RIDGE, probs) for k in (0, 1)}
    for k in (0, 1):                                       # the bandwidth lands on its run, which the two kernels treat differently
        assert r[k]["status"].tolist() == [0] and AC.bits(r[k]["bandwidth"][0]) == AC.bits(AC.KEYS_DELTA2)
        assert r[k]["n_kept"][0] == exp["n_kept"][k]
    assert r[0]["n_kept"][0] - r[1]["n_kept"][0] == c * AC.KEYS_RUN >= 10 and r[0]["n_kept"][0] > AC.KEYS_TOL * c * AC.KEYS_T + 5
    assert np.abs(r[1]["beta"]).max() < 1e-299
    star, q, kept, d2 = recomputed(h, members, 1, r[1]["beta"][0])
    assert (d2 == AC.KEYS_DELTA2).sum() == c * AC.KEYS_RUN and kept.sum() == c * AC.KEYS_KEPT
    th = info["theta"][members].reshape(-1, 2)
    assert np.array_equal(AC.bits(star[kept]), AC.bits(th[kept]))                 # a kept theta* is its theta bit for bit
    assert np.array_equal(q, info["q"][members].reshape(-1)) and np.array_equal(d2, info["d2"][members].reshape(-1))
    assert (q == 1).sum() == c and (q[d2 == 0] == AC.Q_ONE).all() and (d2 == 0).sum() == c * len(AC.KEYS_ON_DATA)
    assert np.array_equal(r[1]["n_outside"][0], exp["n_outside"]) and exp["n_outside"].tolist() == [c, 0]
    assert np.array_equal(AC.bits(r[1]["adj_quantile"][:, 0]), AC.bits(want))     # the reference's quantiles are the construction's
    for j in range(2):
        v, lv = star[:, j], AC.keys_levels(star[:, j], q)
        kv = v[kept]
        assert (kv < 0).any() and (kv > 0).any() and (np.abs(kv) >= 1).any() and ((np.abs(kv) <= 1e-300) & (kv != 0)).any()
        assert (AC.bits(kv) == AC.bits(0.0)).any() and (AC.bits(kv) == AC.bits(-0.0)).any()
        assert ((np.abs(kv) < 2.3e-308) & (kv != 0)).any()                       # subnormals
        # the tie run: at least eight equal values under at least three distinct weights
        tie = next(l for l in lv if l[0] == (AC.KEYS_TIE if j == 0 else -AC.KEYS_TIE))
        assert len(tie[3]) >= 8 and len(set(tie[3])) >= 3
        Q = int(q.sum())
        target = lambda name: max(1, int(np.ceil(np.float64(probs[marks[j][name]]) * np.float64(Q))))
        assert tie[1] < target("inside") < tie[2] and target("end") == tie[2] and target("past") == tie[2] + 1
        assert want[marks[j]["inside"], j] == want[marks[j]["end"], j] == tie[0] and want[marks[j]["past"], j] > tie[0]
        # the six digits: the answer of a requested target and the kept key before it part at that digit, agreeing above it
        apart = set()
        for name, i in marks[j].items():
            at = next(n for n, l in enumerate(lv) if l[1] < target(name) <= l[2])
            assert AC.bits(lv[at][0]) == AC.bits(want[i, j])
            if at > 0 and target(name) == lv[at][1] + 1:
                apart.add(AC.first_digit_apart(lv[at - 1][0], lv[at][0]))
        assert apart >= {0, 1, 2, 3, 4, 5}, apart
        # answers that are zeros of either sign
        assert AC.bits(want[marks[j]["+0"], j]) == AC.bits(0.0) and AC.bits(want[marks[j]["-0"], j]) == AC.bits(-0.0)
        # adjust_ref.weighted_quantile against the loop, on both kernels' weights
        for k in (0, 1):
            s, qq, _, _ = recomputed(h, members, k, r[k]["beta"][0])
            for i, p in enumerate(probs):
                a = AR.weighted_quantile(s[:, j], qq, p)
                assert AC.bits(a) == AC.bits(AC.weighted_quantile_loop(s[:, j], qq, p)) == AC.bits(r[k]["adj_quantile"][i, 0, j])


def test_crafted_keys_every_chain_a_group_of_its_own():
    """each chain holds the whole design: the bandwidth is the run's distance in every one of them"""
    N = 6
    h, info = AC.crafted_keys(N, 9)
    probs, _, _ = AC.keys_probs(info, [0])
    for k in (0, 1):
        r = ref(h, KEYS, 0, np.arange(N, dtype=np.int32), AC.KEYS_TOL, k, AC.KEYS_RIDGE, probs)
        assert r["status"].tolist() == [0] * N and (r["bandwidth"] == AC.KEYS_DELTA2).all()
        assert r["n_kept"].tolist() == [AC.keys_expect(info, [0])["n_kept"][k]] * N
    assert not np.array_equal(info["theta"][0], info["theta"][1])                 # (in an order of its own)


@pytest.mark.parametrize("members", ((0,), (0, 1, 2, 3, 4, 5)))
def test_crafted_keys_at_a_bandwidth_of_zero(members):
    """tol = KEYS_TOL_ZERO puts the bandwidth on the run of rows at distance 0: Epanechnikov's kernel drops the run and keeps nothing,
    with weights of 0.0 (not 0 / 0), the uniform kernel keeps the run alone"""
    members = list(members)
    h, info, groups = keys_case(members)
    zeros = len(members) * len(AC.KEYS_ON_DATA)
    assert (info["d2"][members] == 0).sum() == zeros >= 6
    r = ref(h, KEYS, 0, groups, AC.KEYS_TOL_ZERO, 1, AC.KEYS_RIDGE, (0.5,))
    assert r["status"].tolist() == [3] and r["n_kept"].tolist() == [0]
    assert AC.bits(r["bandwidth"][0]) == AC.bits(0.0) and AC.bits(r["sum_w"][0]) == AC.bits(0.0)
    assert np.isnan(r["ess"][0]) and np.isnan(r["adj_quantile"]).all() and (r["n_outside"] == 0).all()
    r = ref(h, KEYS, 0, groups, AC.KEYS_TOL_ZERO, 0, AC.KEYS_RIDGE, (0.5,))
    assert r["status"].tolist() == [4] and r["n_kept"].tolist() == [zeros] and r["sum_w"][0] == zeros and r["bandwidth"][0] == 0.0
    assert (r["x_mean"] == 0).all() and np.isnan(r["beta"]).all()


def test_order_key_and_the_ladder():
    v = np.array([-np.inf, -1e308, -2.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, 2.0, np.inf])
    k = [AC.order_key(a) for a in v]
    assert k == sorted(k) and len(set(k)) == len(k)
    L = AC.KEYS_LADDER
    assert (np.diff(L) > 0).all()
    assert [AC.first_digit_apart(L[i], L[i + 1]) for i in range(len(L) - 1)] == [0, 5, 4, 3, 2, 1]
    assert AC.first_digit_apart(1.0, 1.0) is None
    for a in v:
        assert AC.bits(AC.weighted_quantile_loop([a], [3], 0.5)) == AC.bits(a)


def test_assert_adjustment_bits_tells_the_zeros_apart():
    a = dict(adj_quantile=np.array([[[0.0, np.nan]]]), n_outside=np.array([[1, 2]], np.int64))
    AC.assert_adjustment_bits(a, dict(adj_quantile=np.array([[[0.0, -np.nan]]]), n_outside=np.array([[1, 2]], np.int64)))
    AR.assert_adjustment_equal(a, dict(adj_quantile=np.array([[[-0.0, np.nan]]]), n_outside=np.array([[1, 2]], np.int64)))
    with pytest.raises(AssertionError):
        AC.assert_adjustment_bits(a, dict(adj_quantile=np.array([[[-0.0, np.nan]]]), n_outside=np.array([[1, 2]], np.int64)))
    with pytest.raises(AssertionError):
        AC.assert_adjustment_bits(a, dict(adj_quantile=np.array([[[0.0, np.nan]]]), n_outside=np.array([[1, 3]], np.int64)))


def test_crafted_seams_lays_the_groups_over_the_chunks():
    h, groups, counts = AC.crafted_seams(3)
    assert h.value.shape == (AC.SEAM_T, AC.SEAM_N) and (h.accepted.sum(axis=0) == counts).all() and (h.accepted[0] == 1).all()
    G = len(AC.SEAM_ROWS)
    pooled = [int(counts[groups == g].sum()) for g in range(G)]
    assert tuple(pooled) == AC.SEAM_ROWS and 40000 < sum(pooled) < 50000
    assert len(set(counts[groups >= 0].tolist())) > 10 and (counts[groups == 0] % 2 == 1).any()   # odd lengths
    gch0 = AC.chunk_starts(pooled)
    assert gch0.tolist() == [0, 3, 5, 7, 7, 8]             # 3 chunks, 2 chunks, 1 chunk + 1 row, none, 256 rows
    assert pooled[2] - AC.LDS_N == 1 and pooled[4] == AC.ADJ_WG
    mom, w, lb, ub = np.array([-1.0, 10.0]), np.ones(2), np.array([-3.0, -20.0]), np.array([3.0, 20.0])
    r = AR.adjustment_from_history(h, 0, AC.SEAM_T, 1, groups, 0.25, 1, None, 0.0, (0.5,), mom, w, lb, ub, n_groups=G)
    assert r["count"].tolist() == list(AC.SEAM_ROWS) and r["status"].tolist() == [0, 0, 0, 1, 0]
    r = AR.adjustment_from_history(h, 0, AC.SEAM_T, 2, groups, 0.25, 0, None, 0.0, (), mom, w, lb, ub, n_groups=G)
    assert r["count"].tolist() == [n * AC.SEAM_T for n in AC.SEAM_CHAINS] and r["status"].tolist() == [0, 0, 0, 1, 0]
    assert AC.chunk_starts(r["count"]).tolist() == [0, 3, 5, 7, 7, 8]


def test_adjust_plan_of_the_existing_seam_test():
    """adjust_plan against the plan tests/test_gpu_adjustment.py states for its seamed context (N = 16, T = 600, np = nm = 2, 4096)"""
    assert AC.adjust_plan(16, 600, 2, 2, 16 * 600, 2, 4096) == (1, 1)
