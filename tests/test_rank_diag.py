"""tests/rank_diag_ref.py, the restatement of smm_get_rank_diag's contract (include/smmhip.h) the GPU tests hold the device against, held
against brute force (the ranks), statistics.NormalDist (ndtri) and theory (independent normal chains; a shifted and a scaled chain); the
tolerance of the outputs behind ndtri measured on the GPU tests' shapes; the Python argument checks, which raise without a device; and
the ctypes and Julia mirrors of smm_rank_diag_t against the header; and the preconditions of tests/test_gpu_rank_edges.py: the crafted
columns' ranks against a count, the digits of their keys, their tie runs against the sort's segments, the vectorised normal scores
against the scalar ones, and every edge shape's tolerance measured with no cell left out.  No GPU."""
import math
import os
import statistics

import numpy as np
import pytest

import chain_diag_ref as D
import rank_diag_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute(x):
    x = np.asarray(x, float)
    return np.array([2 * int(np.sum(x < v)) + int(np.sum(x == v)) + 1 for v in x], np.int64)


def test_ranks_equal_a_brute_force_count():
    rng = np.random.default_rng(1)
    cols = [rng.standard_normal(37), rng.integers(0, 3, 64).astype(float), np.zeros(9), np.array([0.0, -0.0, 1.0, -0.0, -1.0, 0.0]),
            np.repeat(rng.standard_normal(5), 7), np.array([2.5])]
    for x in cols:
        r = R.rank2(x)
        assert r.dtype == np.int64 and np.array_equal(r, brute(x)), x
        assert r.sum() == len(x) * (len(x) + 1)            # twice the sum of the average ranks
    r = R.rank2([0.0, -0.0, 1.0])
    assert r[0] == r[1] == 3                                # -0.0 and +0.0 are equal


@pytest.mark.parametrize("n,groups", [(17, [0, 0, 0, 1, -1]), (9, [0, 1, 1, 1, 1]), (8, [2, 2, 0, 0, 0])])
def test_pooled_ranks_of_groups_with_ties_a_single_member_and_an_odd_window(n, groups):
    rng = np.random.default_rng(n)
    X = rng.integers(-2, 3, (2, 5, n)).astype(float)       # heavy ties, zeros of both signs
    X[X == 0] *= rng.choice([1.0, -1.0], (X == 0).sum())
    g = np.asarray(groups)
    h, nb = n // 2, 5
    out = R.rank_diag_from_series(X, h - 1, nb, g)
    for gi in range(g.max() + 1):
        mem = np.flatnonzero(g == gi)
        if len(mem) == 0:                                   # a group without members: undefined
            assert (out["status"][:, gi] == 2).all() and np.isnan(out["rhat_rank"][gi]).all()
            continue
        for s in range(2):
            pooled = np.concatenate([X[s, c, lo:lo + h] for c in mem for lo in (0, n - h)])
            r2 = brute(pooled)
            M = len(pooled)
            want = np.zeros((nb, len(mem)), np.int64)
            for i, v in enumerate(r2):
                want[((int(v) - 1) * nb) // (2 * M), i // (2 * h)] += 1
            assert np.array_equal(out["rank_hist"][:, s, mem], want)
    assert (out["rank_hist"][:, :, g < 0] == 0).all()
    assert (out["rank_hist"].sum(axis=0)[:, g >= 0] == 2 * h).all()


def test_ndtri_is_the_standard_librarys_to_the_last_bit_or_one_ulp():
    inv = statistics.NormalDist().inv_cdf
    for M in (16, 256, 1200, 9600):
        for r2 in list(range(2, 2 * M + 1, max(1, M // 300))) + [2 * M]:
            p = R.rank_prob(r2, M)
            a, b = R.ndtri(p), inv(p)
            assert abs(a - b) <= math.ulp(b), (M, r2, a, b)
    assert R.ndtri(0.5) == 0.0 and R.ndtri(0.975) == pytest.approx(1.959963984540054, abs=1e-15)


def test_independent_normal_chains_a_shifted_and_a_scaled_chain():
    rng = np.random.default_rng(11)
    m, h = 8, 500
    Y = rng.standard_normal((m, h))
    c, _ = R.cell(Y, h - 1)
    assert abs(c["rhat_rank"] - 1) < 0.01 and abs(c["rhat_bulk"] - 1) < 0.01 and abs(c["rhat_folded"] - 1) < 0.01
    assert abs(c["ess_bulk"] / (m * h) - 1) < 0.2 and c["status"] == (0, 0, 0, 0)
    assert c["ess_tail"] > 0.5 * m * h and abs(c["ess_mean"] / (m * h) - 1) < 0.2
    shifted = Y.copy()
    shifted[0] += 2.0
    assert R.cell(shifted, h - 1)[0]["rhat_bulk"] > 1.1
    scaled = Y.copy()
    scaled[0] *= 3.0
    cs, _ = R.cell(scaled, h - 1)
    mu, var = [D.S(y) / h for y in scaled], None
    var = [D.S((y - a) * (y - a)) / (h - 1) for y, a in zip(scaled, mu)]
    assert cs["rhat_folded"] > 1.05 and cs["rhat_rank"] == cs["rhat_folded"] and D.rhat_group(mu, var, h) < 1.01


def metropolis(rng, N, T, step, thin=4):
    """[N][T] random-walk Metropolis chains on N(0, 1), every thin-th state: a state series with ties, as the library's"""
    x = rng.standard_normal(N)
    out = np.empty((N, T * thin))
    for t in range(T * thin):
        prop = x + step * rng.standard_normal(N)
        acc = np.log(rng.random(N)) < 0.5 * (x * x - prop * prop)
        x = np.where(acc, prop, x)
        out[:, t] = x
    return out[:, ::thin]


def gpu_shapes():
    """the GPU tests' shapes with synthetic series [S][N][n]: (series, max_lag, groups)"""
    rng = np.random.default_rng(2021)
    small = np.stack([metropolis(rng, R.N_SMALL, R.T_SMALL, 2.4) for _ in range(3)])
    large = np.stack([metropolis(rng, R.N_LARGE, R.T_LARGE, 2.4) for _ in range(3)])
    cases = [(small[:, :, t0:t1], (t1 - t0) // 2 - 1, R.GROUPS_SMALL) for t0, t1 in R.WINDOWS_SMALL]
    return cases + [(large, R.T_LARGE // 2 - 1, R.GROUPS_LARGE)]


def test_the_tolerance_is_eight_times_the_effect_of_a_one_ulp_logarithm():
    up = lambda x: math.nextafter(math.log(x), math.inf)
    down = lambda x: math.nextafter(math.log(x), -math.inf)
    worst, left_out, ok = 0.0, [], []
    for X, ml, g in gpu_shapes():
        base = R.rank_diag_from_series(X, ml, 4, g)
        left_out.append(R.near_sign_change(base))
        ok.append(base["status"][0] == 0)
        for log in (up, down):
            moved = R.rank_diag_from_series(X, ml, 4, g, log=log)
            for f in R.EXACT:
                assert np.array_equal(moved[f], base[f], equal_nan=True), f     # (no logarithm behind these)
            for f in R.TOLERANCED:
                a, b = moved[f], base[f]
                assert np.array_equal(np.isnan(a), np.isnan(b)), f
                fin = ~np.isnan(b)
                worst = max(worst, float(np.max(np.abs(a[fin] - b[fin]) / np.abs(b[fin]))))
    print("largest relative change: %.3g; RANK_LOG_CHANGE = %.3g, RANK_RTOL = %.3g" % (worst, R.RANK_LOG_CHANGE, R.RANK_RTOL))
    assert 0 < worst <= R.RANK_LOG_CHANGE and R.RANK_RTOL == 8 * R.RANK_LOG_CHANGE
    assert R.RANK_LOG_CHANGE <= 4 * worst                   # (the constant is the measurement, rounded up: no slack beyond that)
    assert np.mean(np.concatenate([v.ravel() for v in left_out])) <= 0.05
    assert np.mean(np.concatenate([v.ravel() for v in ok])) >= 0.9


def test_the_gpu_tests_populations_mix(O):
    """the histories the GPU tests compute, here from the CPU oracle: at least 90 % of the cells of the small and the large shape have
    status 0, at most 5 % are left out of the toleranced comparison, and max_lag = 2 comes first everywhere (status 1 occurs)"""
    import common as cm

    def history(kw):
        prob, opts = cm.serial_normal(**kw)
        o = O.OracleContext(prob, opts)
        o.step(kw["T"])
        return o.history(0, kw["T"])

    hs, hl = history(R.SMALL_KW), history(R.LARGE_KW)
    with np.errstate(invalid="ignore", divide="ignore"):
        cells = [R.rank_diag_from_history(hs, t0, t1, None, 0, R.GROUPS_SMALL) for t0, t1 in R.WINDOWS_SMALL]
        cells.append(R.rank_diag_from_history(hl, 0, R.T_LARGE, None, 0, R.GROUPS_LARGE))
        short = [R.rank_diag_from_history(hs, t0, t1, 2, 0, R.GROUPS_SMALL) for t0, t1 in R.WINDOWS_SMALL]
    print("status 0:", [(c["status"] == 0).all(axis=0).tolist() for c in cells], "ties:", 1 - hs.accepted.mean(), 1 - hl.accepted.mean())
    assert R.share_of_cells_with_status_0(cells) >= 0.9
    for c in cells + short:
        assert R.near_sign_change(c).mean() <= 0.05
    for c in short:
        assert np.isin(c["status"][[0, 2, 3]], (1, 2)).all() and (c["status"] == 1).any()
    assert 0.1 < 1 - hs.accepted.mean() < 0.3 and 0.5 < 1 - hl.accepted.mean() < 0.8       # (the series are tied as the library's are)


def test_python_argument_checks_raise_without_a_device():
    from smm_jl_amd.backend import BGPContext
    c = object.__new__(BGPContext)
    c.N, c.np, c._ctx = 16, 2, None
    g = np.zeros(16, np.int32)
    for kw in (dict(t0=5, t1=12), dict(t0=0, t1=20, max_lag=0), dict(t0=0, t1=20, max_lag=10), dict(t0=0, t1=20, n_bins=-1),
               dict(t0=0, t1=20, groups=np.zeros(15)), dict(t0=0, t1=20, groups=np.full(16, -1)), dict(t0=0, t1=20, groups=g, n_groups=0)):
        with pytest.raises(ValueError):
            c.rank_diag(**kw)
    import smm_jl_amd as S
    for name in ("rhat_rank", "ess_bulk", "ess_tail", "rank_plot"):
        assert callable(getattr(S, name)) and name in S.__all__


def test_the_mirrors_of_smm_rank_diag_t():
    from test_julia_layer import header_structs, julia_structs
    from smm_jl_amd import _abi as A
    js = julia_structs(os.path.join(ROOT, "julia", "SMMHip.jl"))
    want = header_structs()["smm_rank_diag_t"]
    ptr = {"Cdouble": "double*", "Int32": "int32_t*", "Int64": "int64_t*"}
    assert [(f, ptr[t[4:-1]]) for f, t in js["SmmRankDiag"]] == [(f, t) for f, t in want]
    assert [f for f, _ in A.smm_rank_diag_t._fields_] == [f for f, _ in want]
    argtypes = dict((n, a) for n, _, a in A.SYMBOLS)["smm_get_rank_diag"]
    assert len(argtypes) == 8 and argtypes[-1]._type_ is A.smm_rank_diag_t


# --- the preconditions of tests/test_gpu_rank_edges.py, on the CPU ----------------------------------------------------------------------

UP = lambda x: math.nextafter(math.log(x), math.inf)
DOWN = lambda x: math.nextafter(math.log(x), -math.inf)


def test_the_vectorised_scores_are_the_scalar_ones():
    rng = np.random.default_rng(3)
    for M in (8, 354, 2000, 9554, 40000):
        for r2 in (R.rank2(rng.standard_normal(M)), R.rank2(np.round(rng.standard_normal(M), 1)), R.rank2(np.zeros(M))):
            for log in (math.log, UP, DOWN):
                assert np.array_equal(R.scores(r2, log), R.scores_scalar(r2, log)), M
    p = np.r_[np.linspace(1e-7, 1 - 1e-7, 5001), 0.075, 0.925, 0.5, 1.3e-11, 1 - 1e-11]      # the three branches and their borders
    assert np.array_equal(R.ndtri_array(p), np.array([R.ndtri(float(v)) for v in p]))
    assert (np.abs(p - 0.5) <= 0.425).any() and (R.ndtri_array(p) > 5.0).any() and (R.ndtri_array(p) < -6.0).any()


def crafted_columns():
    """the pooled columns of cases 1 and 2 at a few hundred values"""
    cols = R.three_orders(R.key_values(R.KEYS_M - R.N_KEY_VALUES), 3)
    cols += R.three_orders(R.tie_column(600, (1, 2, 63, 64, 65, 301), R.TIES_SEED)[0], R.TIES_SEED)
    return cols + list(R.zeros_columns())


def test_the_ranks_of_the_crafted_columns_equal_a_count_of_less_and_equal():
    for x in crafted_columns():
        assert np.array_equal(R.rank2(x), brute(x))
    z = R.zeros_columns()
    assert np.array_equal(np.unique(R.rank2(z[0])), [R.ZEROS_M, 2 * R.ZEROS_M]) and np.array_equal(np.unique(R.rank2(z[1])), [2, R.ZEROS_M + 2])
    assert np.signbit(z[:, ::2]).all() and not np.signbit(z[:, 1::2]).any() and (np.sort(z, axis=1)[:, 1:-1] == 0).all()
    m = [float(np.median(c)) for c in z]                    # (the contract's median takes -0 as +0)
    assert m == [0.0, 0.0, 0.0]


def test_every_radix_pass_meets_at_least_three_digits_in_the_crafted_keys():
    col = R.key_values(R.KEYS_M - R.N_KEY_VALUES)
    assert len(col) == R.KEYS_M <= R.RANK_SMALL and np.array_equal(R.pooled_to_series(col, R.KEYS_N, R.KEYS_T)[:, :59].ravel(), col.reshape(3, 2, 59)[:, 0].ravel())
    for b in range(8):                                      # the values of one family differ in byte b only
        fam = col[np.isin(col.view(np.uint64) & ~np.uint64(0xFF << (8 * b)), [R.KEY_BASE & ~(0xFF << (8 * b))])]
        fam = fam[fam > 0]
        assert len(fam) >= 10 and np.isin(-fam, col).all()     # (the negated family's keys are the complements)
        for f in (fam, -fam):
            assert len(np.unique(R.key_digits(f)[b])) == len(f) and all(len(np.unique(R.key_digits(f)[o])) == 1 for o in range(8) if o != b)
    for cols in (R.three_orders(col, 3), R.ties_short_series()[1], R.ties_long_series()[1]):
        for c in cols:
            assert all(len(np.unique(d)) >= 3 for d in R.key_digits(c))
    k = R.sort_keys(col)
    assert (np.diff(k.astype(object)) >= 0).all() and (np.diff(k.astype(object)) == 0).sum() == 1   # ascending; -0 and +0 share a key
    for v in (0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, -1.7976931348623157e308, 1.7976931348623157e308, 1e16, 1e16 + 4):
        assert (col == v).any(), v
    assert np.signbit(col[col == 0]).tolist() == [True, False]


def runs_of(col):
    s = np.sort(np.asarray(col) + 0.0)
    starts = np.flatnonzero(np.r_[True, s[1:] != s[:-1]])
    return starts, np.diff(np.r_[starts, len(s)])


def test_the_tie_runs_meet_the_segments_edges():
    nseg, seg = R.rank_segments(R.TIES_SHORT_M)
    assert (nseg, seg) == (4, 512) and R.rank_nblk(R.TIES_SHORT_M) == 1
    _, cols = R.ties_short_series()
    la, lb = set(runs_of(cols[0])[1]), set(runs_of(cols[1])[1])
    assert {1, 2, 63, 64, 65, seg - 1, seg, seg + 1} <= la and la == set(runs_of(cols[2])[1])
    assert {1, 2, 63, 64, 65} <= lb and max(lb) > R.TIES_SHORT_M // 2
    M = R.TIES_LONG_M
    nseg, seg = R.rank_segments(M)
    assert (nseg, seg) == (8, 1216) and R.rank_nblk(M) == 2 and R.RANK_SMALL < M <= 10000
    _, cols = R.ties_long_series()
    for c in cols:
        starts, lens = runs_of(c)
        assert {1, 2, 63, 64, 65, seg - 1, seg, seg + 1} <= set(lens) and lens.max() > M // 2
        i = int(np.argmax(lens))
        edge = 4 * seg                                      # the first place of the second workgroup's segments
        assert starts[i] + 64 < edge < starts[i] + lens[i] - 64, (starts[i], lens[i])
        z = np.asarray(c)[np.asarray(c) == 0]
        assert len(z) == 65 and 0 < np.signbit(z).sum() < 65    # the run on zero holds both signs
    assert all(len(np.unique(np.sign(np.diff(c)))) <= 2 for c in cols[:2]) and (np.diff(cols[2]) < 0).any() and (np.diff(cols[2]) > 0).any()


def test_the_pairwise_sum_of_140_split_chains_has_the_leaves_64_and_76():
    from chain_stats_ref import pw
    x = [float(v) for v in np.random.default_rng(8).standard_normal(140) * 1e3]
    assert 2 * int((R.WIDE_GROUPS == 0).sum()) == 140
    assert D.S(x) == 0.0 + (pw(x, 0, 64) + pw(x, 64, 76)) and D.S(x) != pw(x, 0, 72) + pw(x, 72, 68)
    assert D.S(x) == float(np.sum(np.array(x)))


@pytest.fixture(scope="module")
def edge_calls(O):
    """name -> [(X [S][N][n], max_lag, groups, n_groups)]: every call of tests/test_gpu_rank_edges.py that is held to a tolerance, the
    generated histories from the CPU oracle, whose history is the device's"""
    import common as cm

    def history(kw, steps=None):
        prob, opts = cm.serial_normal(**kw)
        o = O.OracleContext(prob, opts)
        o.step(steps or kw["T"])
        return o.history(0, steps or kw["T"])

    def of(h, windows, ml, g, ng=None):
        return [(D.series_from_history(h, t0, t1)[0], (t1 - t0) // 2 - 1 if ml is None else ml, g, ng) for t0, t1 in windows]

    hl = history(R.LENGTHS_KW)
    hn = history(R.NONFINITE_KW)
    hn.accepted[...] = 1
    R.make_nonfinite(hn.params, hn.value)
    ts, tl = R.ties_short_series()[0], R.ties_long_series()[0]
    return dict(
        keys=[(R.keys_series(), R.KEYS_T // 2 - 1, None, None)],
        ties_short=[(ts, R.TIES_SHORT_T // 2 - 1, R.TIES_SHORT_GROUPS, None)],
        ties_long=[(tl, R.TIES_LONG_T // 2 - 1, None, None)],
        lengths=of(hl, R.LENGTHS_WINDOWS, None, R.LENGTHS_GROUPS, R.LENGTHS_NG),
        tiny=of(hl, R.TINY_WINDOWS, None, R.TINY_GROUPS),
        wide=of(history(R.WIDE_KW), ((0, R.WIDE_KW["T"]),), None, R.WIDE_GROUPS),
        two_long=of(history(R.TWO_LONG_KW, R.TWO_LONG_STEPS), ((0, R.TWO_LONG_STEPS),), R.TWO_LONG_LAG, R.TWO_LONG_GROUPS, R.TWO_LONG_NG),
        cap=of(history(R.CAP_KW), ((0, R.CAP_KW["T"]),), R.CAP_LAG, R.CAP_GROUPS),
        lags=of(history(R.LAGS_KW), ((0, R.LAGS_KW["T"]),), None, R.LAGS_GROUPS),
        nonfinite=of(hn, ((0, R.NONFINITE_KW["T"]),), None, R.NONFINITE_GROUPS, R.NONFINITE_NG),
    )


@pytest.mark.parametrize("name", sorted(R.EDGE_RTOL))
def test_each_edge_shape_leaves_no_cell_out_and_has_its_tolerance_measured(edge_calls, name):
    """the one-ulp logarithm moved either way on the shape's own calls: the integer outputs, ess_tail and ess_mean do not move, the
    outputs behind ndtri by less than RANK_LOG_CHANGE (then the shape is compared at RANK_RTOL) or the shape's rtol is 8 x its own
    figure; and no cell's truncating pair lies within the tolerance of zero"""
    worst = 0.0
    for X, ml, g, ng in edge_calls[name]:
        with np.errstate(all="ignore"):
            base = R.rank_diag_from_series(X, ml, 4, g, ng)
            moved = [R.rank_diag_from_series(X, ml, 4, g, ng, log=log) for log in (UP, DOWN)]
        assert not R.near_sign_change(base, R.EDGE_RTOL[name]).any(), base["pair_at_truncation"]
        for mv in moved:
            for f in R.EXACT:
                assert np.array_equal(mv[f], base[f], equal_nan=True), f
            for f in R.TOLERANCED:
                a, b = mv[f], base[f]
                assert np.array_equal(np.isnan(a), np.isnan(b)), f
                fin = ~np.isnan(b)
                worst = max(worst, float(np.max(np.abs(a[fin] - b[fin]) / np.abs(b[fin]), initial=0.0)))
    print("%s: largest relative change %.3g; rtol %.3g" % (name, worst, R.EDGE_RTOL[name]))
    if worst <= R.RANK_LOG_CHANGE:
        assert R.EDGE_RTOL[name] == R.RANK_RTOL
    else:
        assert 8 * worst <= R.EDGE_RTOL[name] <= 8 * 1.25 * worst      # (the shape's own figure, rounded up)


def test_the_edge_shapes_reach_their_paths(edge_calls):
    assert R.rank_nblk(8192) == 1 and R.rank_nblk(8704) == 2 and R.rank_segments(8704) == (8, 1088) and 7 * 1088 < 8704 <= 8 * 1088
    assert R.rank_nblk(524800) == R.RANK_NBLK and R.rank_segments(524800) == (256, 2112) and R.rank_nblk(32800) == 5
    assert R.rank_nblk(9600) == 2 and R.rank_nblk(16800) == 3
    N, T = R.TWO_LONG_KW["N"], R.TWO_LONG_KW["T"]
    per = [R.rank_bytes(int((R.TWO_LONG_GROUPS == g).sum()), R.TWO_LONG_STEPS // 2, R.TWO_LONG_LAG) for g in range(R.TWO_LONG_NG)]
    assert per[3] == 0 and sum(per[:3]) == R.TWO_LONG_SCRATCH < sum(per) and R.TWO_LONG_SCRATCH <= N * T * 20   # A, short, B | short
    (X, ml, g, ng), = edge_calls["cap"]
    assert X.shape[2] // 2 == 8200 > 8192 and R.CAP_BINS > R.RANK_HIST_LDS
    (X, ml, g, ng), = edge_calls["lags"]
    with np.errstate(all="ignore"):
        want = R.rank_diag_from_series(X, ml, 4, g, ng)
    print("lags: status", want["status"].tolist())
    assert ml == 299 and (want["status"][[0, 2, 3]] == 1).any()     # a kind of a cell still open at max_lag = 299 > 256
    (X, ml, g, ng), = edge_calls["nonfinite"]
    with np.errstate(all="ignore"):
        want = R.rank_diag_from_series(X, ml, 4, g, ng)
    st = want["status"]
    assert (st[:, 0, 1] == 3).all() and (st[:, 1, 2] == 3).all() and (st[:, 3] == 2).all() and ((st == 3).sum(), (st[:, 2] < 2).all()) == (8, True)
    assert (want["rank_hist"][:, 1, :3] == 0).all() and (want["rank_hist"][:, 2, 3:6] == 0).all()
    assert (want["rank_hist"].sum(axis=0)[[0, 2]][:, :3] == 40).all() and (want["rank_hist"].sum(axis=0)[:, 6:] == 40).all()
