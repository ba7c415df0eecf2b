"""The walk over a chain's window that the history reducers share (smm.jl_amd/csrc/smm_window.hpp), at its edges, through every entry
point that reaches it: crafted accepted flags (a chain that is never accepted, one accepted at row 0 only, one accepted at rows 255,
256 and 511 only — the last lane of a block, the first of the next, the last wave's last lane —, one accepted everywhere, the run's own
flags for the rest) and windows of 1, 255, 256, 257 and 443 iterations that start on and beside a block edge, look back more than two
blocks to row 0, or look back and find nothing.  N = 6 leaves xcd_chain the identity, N = 16 swizzles.  Every output equals (array_equal,
NaN equal to NaN) the restatement in the *_ref.py files over the history read back from the same context; smm_get_rank_diag by its
restatement's own comparison (rank_diag_ref.assert_rank_diag_close: the integer outputs, ess_tail and ess_mean equal, the outputs behind
ndtri within RANK_RTOL, as the logarithm is not numpy's).  The pooled-column pipeline that smm_get_group_stats and
smm_get_moment_stats share is cross-checked bit for bit on every window."""
import numpy as np
import pytest

import chain_diag_ref as DR
import chain_stats_ref as SR
import common as cm
import group_stats_ref as GR
import hist_ref as HR
import moment_stats_ref as MR
import profile_ref as PR
import rank_diag_ref as RD
import trace_ref as TR

pytestmark = pytest.mark.gpu

T = 700
WINDOWS = ((0, 1), (0, 256), (0, 257), (1, 256), (255, 257), (256, 512), (257, 700), (600, 700), (699, 700))
PROBS = (0.025, 0.5, 0.975)
GROUPS = {6: np.array([0, 1, 0, 1, -1, 0], np.int32),                                     # 3 and 2 members, chain 4 in no group
          16: np.array([0, 1, 0, 1, -1, 0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 1], np.int32)}      # 9 and 6 members, chain 4 in no group


@pytest.fixture(scope="module", params=(6, 16))
def crafted(request, S):
    N = request.param
    prob, opts = cm.serial_normal(N=N, T=T, ns=100)
    h0 = S.hip_context(prob, opts)
    h0.step(T)
    c = MR.copy_history(h0.history(0, T))
    c.accepted[:, 0] = 0                                   # never accepted: no state row anywhere
    c.accepted[:, 1] = 0
    c.accepted[0, 1] = 1                                   # row 0 only: every look-back ends at row 0
    c.accepted[:, 2] = 0
    c.accepted[[255, 256, 511], 2] = 1                     # the last lane of a block, the first of the next, the last wave's last lane
    c.accepted[:, 3] = 1                                   # everywhere
    assert (c.accepted[:, 4:] == 0).any() and (c.accepted[:, 4:] != 0).any() and (c.exchanged != 0).any()
    h = S.hip_context(prob, opts)
    h.set_state(h0.state(), c)
    hist = h.history(0, T)
    assert np.array_equal(hist.accepted, c.accepted) and np.array_equal(hist.exchanged, c.exchanged)   # the crafted flags are installed
    return h, prob, hist, GROUPS[N]


def equal(a, b):
    return np.array_equal(a, b, equal_nan=np.asarray(a).dtype.kind == "f")


@pytest.mark.parametrize("t0,t1", WINDOWS)
def test_every_reducer_on_a_window_at_the_edges_of_the_walk(crafted, t0, t1):
    h, prob, hist, g = crafted
    n = t1 - t0
    for sel in (0, 1, 2):
        got = h.histogram(t0, t1, sel, g, 7, None, [(0, 1)], 4, n_groups=2)
        HR.assert_histogram_equal(got, HR.histogram_from_history(hist, t0, t1, sel, g, 7, None, [(0, 1)], 4, n_groups=2), auto=True)
    for stride in (1, 3):
        got = h.trace(t0, t1, stride, 2, False, g, PROBS, n_groups=2)
        TR.assert_trace_equal(got, TR.trace_from_history(hist, t0, t1, stride, 2, False, g, PROBS, n_groups=2))
    if n >= 4:                                             # the two diagnostics refuse a shorter window: (0, 1), (255, 257), (699, 700)
        with np.errstate(invalid="ignore", divide="ignore"):
            want = DR.diag_from_history(hist, t0, t1, None, 3, g)
            DR.assert_diag_equal(h.chain_diag(t0, t1, None, 3, g), want)
            want = RD.rank_diag_from_history(hist, t0, t1, None, 5, g, 2)
        RD.assert_rank_diag_close(h.rank_diag(t0, t1, None, 5, g, 2), want)
    gs = {}
    for acc in (False, True):
        gs[int(acc)] = h.group_stats(t0, t1, acc, g, PROBS, n_groups=2)
        GR.assert_group_stats_equal(gs[int(acc)], GR.group_stats_from_history(hist, t0, t1, acc, g, PROBS, n_groups=2))
    for sel in (0, 1, 2):
        ms = h.moment_stats(t0, t1, sel, g, PROBS, 0.0, n_groups=2)
        MR.assert_moment_stats_equal(ms, MR.moment_stats_from_history(hist, t0, t1, sel, g, PROBS, 0.0, prob.mom, prob.w, n_groups=2))
        same = gs[sel % 2]                                 # (select 2 takes every iteration, as select 0 does)
        assert equal(ms["count"], same["count"]), (sel, ms["count"], same["count"])
        if sel < 2:                                        # the shared pooled-column pipeline, bit for bit
            assert equal(ms["p_mean"], same["mean"]) and equal(ms["cov_pp"], same["cov"]), sel
    got = h.profile(t0, t1, 2, g, 5, None, [(0, 1)], 3, n_groups=2)
    PR.assert_profile_equal(got, PR.profile_from_history(hist, t0, t1, 2, g, 5, None, [(0, 1)], 3, n_groups=2))
    for acc in (False, True):
        SR.assert_stats_equal(h.chain_stats(t0, t1, acc, PROBS), SR.stats_from_history(hist, t0, t1, acc, PROBS))
