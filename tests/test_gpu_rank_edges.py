"""smm_get_rank_diag's sort, ties and batches at their edges (smm.jl_amd/csrc/smm_rank.hpp, host side in smm_reducers_host.hpp), on the
shapes and crafted series that rank_diag_ref.py names (cases 1 - 7 there, each with the path it reaches; tests/test_rank_diag.py proves
their preconditions on the CPU).  Crafted series are installed with set_state as tests/test_gpu_window_walk.py does it, every iteration
accepted, so that the state series is the crafted column itself, and read back.  The reference is always rank_diag_from_history over the
history read back, compared by assert_rank_diag_close at the shape's tolerance (rank_diag_ref.EDGE_RTOL) with no cell left out; with
n_bins = 2 M the contract's bin is rank2 - 1, so that rank_hist holds every chain's exact twice-ranks (the 64-bit global-atomic
histogram, as n_bins > RANK_HIST_LDS), compared with rank_diag_ref.rank2 of the crafted column itself."""
import time

import numpy as np
import pytest

import common as cm
import moment_stats_ref as MR
import rank_diag_ref as R

pytestmark = pytest.mark.gpu


def ref_of(hist, kw):
    with np.errstate(all="ignore"):                     # (the x moments of +-DBL_MAX overflow, by the contract's arithmetic)
        return R.rank_diag_from_history(hist, kw["t0"], kw["t1"], kw.get("max_lag"), kw.get("n_bins", 20), kw.get("groups"), kw.get("n_groups"))


def check(h, hist, name, **kw):
    got, want = h.rank_diag(**kw), ref_of(hist, kw)
    print(name, kw["t0"], kw["t1"], kw.get("max_lag"), kw.get("n_bins", 20), "status", want["status"].tolist())
    R.assert_rank_diag_close(got, want, R.EDGE_RTOL[name], max_left_out=0.0)
    return got, want


def generated(S, kw, steps=None):
    prob, opts = cm.serial_normal(**kw)
    h = S.hip_context(prob, opts)
    h.step(steps or kw["T"])
    return h, h.history(0, steps or kw["T"])


def same_bits(a, b):
    return np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


def crafted(S, kw, X=None, change=None):
    """a context of serial_normal(**kw) whose history holds the series X [3][N][T] (parameter 0, parameter 1, the value), or its own
    with change(params, value) applied, every iteration accepted"""
    prob, opts = cm.serial_normal(**kw)
    T = kw["T"]
    h0 = S.hip_context(prob, opts)
    h0.step(T)
    c = MR.copy_history(h0.history(0, T))
    c.accepted[...] = 1
    if X is not None:
        c.params[:, 0, :], c.params[:, 1, :], c.value[...] = X[0].T, X[1].T, X[2].T
    if change is not None:
        change(c.params, c.value)
    h = S.hip_context(prob, opts)
    h.set_state(h0.state(), c)
    hist = h.history(0, T)
    assert same_bits(hist.params, c.params) and same_bits(hist.value, c.value) and (hist.accepted == 1).all()   # the crafted values are installed
    return h, hist


def assert_exact_ranks(got, cols, members):
    """rank_hist at n_bins = 2 M against rank2 of the pooled columns cols [3][M] of the group with these members"""
    for s, col in enumerate(cols):
        assert np.array_equal(got["rank_hist"][:, s, members].T, R.chain_ranks(col, len(members))), s


def test_keys_that_differ_in_one_byte_per_pass(S):
    """case 1: every digit position of the keys varies, negative keys, denormals, +-DBL_MAX, -0 / +0 the only tie"""
    X = R.keys_series()
    h, hist = crafted(S, dict(N=R.KEYS_N, T=R.KEYS_T, ns=100), X)
    cols = R.three_orders(R.key_values(R.KEYS_M - R.N_KEY_VALUES), 3)
    check(h, hist, "keys", t0=0, t1=R.KEYS_T, n_bins=20)
    got, _ = check(h, hist, "keys", t0=0, t1=R.KEYS_T, n_bins=2 * R.KEYS_M)
    assert_exact_ranks(got, cols, np.arange(R.KEYS_N))
    assert (got["rank_hist"].sum(axis=(0, 2)) == R.KEYS_M).all() and (got["rank_hist"].sum(axis=2).max(axis=0) == 2).all()   # (-0 and +0)


def test_tie_runs_in_a_short_column_and_zeros_of_both_signs(S):
    """case 2, one workgroup: runs of 1, 2, 63, 64, 65, a wave segment - 1, + 0, + 1 and more than half the column; -0 and +0 only"""
    X, cols = R.ties_short_series()
    T, g = R.TIES_SHORT_T, R.TIES_SHORT_GROUPS
    h, hist = crafted(S, dict(N=R.TIES_SHORT_N, T=T, ns=100), X)
    check(h, hist, "ties_short", t0=0, t1=T, n_bins=20, groups=g)
    first = np.where(g == 0, 0, -1)
    got, _ = check(h, hist, "ties_short", t0=0, t1=T, n_bins=2 * R.TIES_SHORT_M, groups=first)
    assert_exact_ranks(got, cols, np.flatnonzero(g == 0))
    got, _ = check(h, hist, "ties_short", t0=0, t1=T, n_bins=2 * R.ZEROS_M, groups=np.where(g == 1, 0, -1))
    assert_exact_ranks(got, R.zeros_columns(), np.flatnonzero(g == 1))
    hist_of = got["rank_hist"][:, :, 4]
    assert [np.flatnonzero(hist_of[:, s]).tolist() for s in range(3)] == [[499, 999], [1, 501], [499, 999]]   # one run of 499, one value
    # the LDS limit of the rank histogram and the first bin count past it, on the same column
    base = None
    for nb in (R.RANK_HIST_LDS, R.RANK_HIST_LDS + 1):
        got, _ = check(h, hist, "ties_short", t0=0, t1=T, n_bins=nb, groups=g)
        for f in R.FLOATS + ("status",):
            assert base is None or np.array_equal(got[f], base[f], equal_nan=True), f
        base = got


def test_tie_runs_across_the_segments_of_two_workgroups(S):
    """case 2, nblk = 2: the same runs in one column of 9554, the longest across the boundary between the workgroups' segments"""
    X, cols = R.ties_long_series()
    T = R.TIES_LONG_T
    h, hist = crafted(S, dict(N=R.TIES_LONG_N, T=T, ns=100), X)
    check(h, hist, "ties_long", t0=0, t1=T, n_bins=20)
    got, _ = check(h, hist, "ties_long", t0=0, t1=T, n_bins=2 * R.TIES_LONG_M)
    assert_exact_ranks(got, cols, np.arange(R.TIES_LONG_N))


def test_the_length_edges_of_the_one_workgroup_sort(S):
    """case 3: M = RANK_SMALL and the first multi-workgroup lengths, one member, no member, an odd window; M = 8 from n = 8 and n = 9"""
    h, hist = generated(S, R.LENGTHS_KW)
    for t0, t1 in R.LENGTHS_WINDOWS:
        got, want = check(h, hist, "lengths", t0=t0, t1=t1, n_bins=20, groups=R.LENGTHS_GROUPS, n_groups=R.LENGTHS_NG)
        assert (want["status"][:, 3] == 2).all() and np.isnan(got["rhat_rank"][3]).all() and (want["status"][:, :3] != 3).all()
        assert (got["rank_hist"].sum(axis=0) == 512).all()
    for t0, t1 in R.TINY_WINDOWS:
        for nb in (16, 5):                                 # (n_bins = 2 M = 16: the ranks themselves)
            got, want = check(h, hist, "tiny", t0=t0, t1=t1, n_bins=nb, groups=R.TINY_GROUPS)
        assert (got["rank_hist"].sum(axis=0)[:, 5] == 8).all() and got["rank_hist"].sum() == 24


def test_a_group_of_seventy_members(S):
    """case 3: m = 140 split chains, the recursive branch of the one-lane pairwise sums over the chains"""
    h, hist = generated(S, R.WIDE_KW)
    got, want = check(h, hist, "wide", t0=0, t1=R.WIDE_KW["T"], n_bins=20, groups=R.WIDE_GROUPS)
    assert (want["status"] != 2).all() and np.isfinite(got["rhat_rank"]).all()


def test_two_long_columns_in_one_batch_and_in_batches_of_their_own(S, monkeypatch, hooks):
    """case 4: long A, short, long B, empty, short.  All five groups in one batch against the restatement; then, equal to that, the
    smallest scratch (the batches A + short, B + empty, short) and the scratch that holds A, short and B of one series, no more"""
    T = R.TWO_LONG_STEPS
    kw = dict(t0=0, t1=T, max_lag=R.TWO_LONG_LAG, n_bins=20, groups=R.TWO_LONG_GROUPS, n_groups=R.TWO_LONG_NG)
    h, hist = generated(S, R.TWO_LONG_KW, T)
    base, want = check(h, hist, "two_long", **kw)
    assert (want["status"][:, 3] == 2).all() and (want["status"][:, [0, 1, 2, 4]] != 2).any()
    for scratch in (1, R.TWO_LONG_SCRATCH):
        monkeypatch.setenv("SMMHIP_STATS_SCRATCH", str(scratch))
        hb, _ = generated(S, R.TWO_LONG_KW, T)
        monkeypatch.delenv("SMMHIP_STATS_SCRATCH")
        got = hb.rank_diag(**kw)
        for f in base:
            assert np.array_equal(got[f], base[f], equal_nan=base[f].dtype.kind == "f"), (scratch, f)


def test_the_capped_workgroup_count_and_a_half_window_past_the_lds(S):
    """case 5: M = 524800 (nblk capped at 64) and M = 32800 (nblk = 5) at h = 8200 > 8192.  Measured on an MI355X: 0.36 s for the
    16400 iterations and their history, 0.02 s for the call, 0.37 s for the restatement: 0.8 s in all, so group 1 stays"""
    T = R.CAP_KW["T"]
    t = [time.perf_counter()]
    h, hist = generated(S, R.CAP_KW)
    t.append(time.perf_counter())
    kw = dict(t0=0, t1=T, max_lag=R.CAP_LAG, n_bins=R.CAP_BINS, groups=R.CAP_GROUPS)
    got = h.rank_diag(**kw)
    t.append(time.perf_counter())
    want = ref_of(hist, kw)
    t.append(time.perf_counter())
    print("cap: seconds for the run and its history, the call, the restatement:", np.diff(t).round(2).tolist())
    R.assert_rank_diag_close(got, want, R.EDGE_RTOL["cap"], max_left_out=0.0)
    assert (got["rank_hist"].sum(axis=0) == 2 * 8200).all() and (want["status"] != 3).all()


def test_a_second_block_of_lags(S):
    """case 6: a population that has not mixed, max_lag = 299: cells still open at lag 256"""
    T = R.LAGS_KW["T"]
    h, hist = generated(S, R.LAGS_KW)
    got, want = check(h, hist, "lags", t0=0, t1=T, n_bins=7, groups=R.LAGS_GROUPS)
    assert (want["status"][[0, 2, 3]] == 1).any() and (got["status"][[0, 2, 3]] == 1).any()


def test_non_finite_values_and_a_group_without_members(S):
    """case 7: status 3 and NaN in the cells of the non-finite values only, no count in rank_hist there; 2 and NaN without members"""
    T, g, ng = R.NONFINITE_KW["T"], R.NONFINITE_GROUPS, R.NONFINITE_NG
    h, hist = crafted(S, R.NONFINITE_KW, change=R.make_nonfinite)
    assert np.isinf(hist.params[31, 1, 1]) and np.isnan(hist.value[4, 5]) and np.isfinite(hist.params).sum() == hist.params.size - 1
    got, want = check(h, hist, "nonfinite", t0=0, t1=T, n_bins=8, groups=g, n_groups=ng)
    st = got["status"]
    three = np.zeros(st.shape, bool)
    three[:, 0, 1] = three[:, 1, 2] = True
    assert np.array_equal(st == 3, three) and (st[:, 3] == 2).all() and (st[:, 2] < 2).all()
    for f in R.FLOATS:
        assert np.isnan(got[f][0, 1]) and np.isnan(got[f][1, 2]) and np.isnan(got[f][3]).all(), f
        assert np.isfinite(got[f][2]).all(), f
    count = got["rank_hist"].sum(axis=0)                    # [S][N]
    assert (count[1, :3] == 0).all() and (count[2, 3:6] == 0).all() and count.sum() == (27 - 6) * T
    alone = h.rank_diag(t0=0, t1=T, n_bins=8, groups=np.where(g == 2, 2, -1), n_groups=ng)
    for f in R.FLOATS:
        assert np.array_equal(alone[f][2], got[f][2]), f
    assert np.array_equal(alone["status"][:, 2], st[:, 2]) and np.array_equal(alone["rank_hist"][:, :, 6:], got["rank_hist"][:, :, 6:])
    assert (alone["status"][:, [0, 1, 3]] == 2).all() and (alone["rank_hist"][:, :, :6] == 0).all()
