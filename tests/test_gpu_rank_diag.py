"""smm_get_rank_diag on the device (include/smmhip.h, smm.jl_amd/csrc/smm_rank.hpp) against the numerical contract restated in
rank_diag_ref.py over the history downloaded with smm_get_history: rank_hist, status, ess_tail and ess_mean equal (array_equal, NaN equal
to NaN), the outputs behind ndtri within rank_diag_ref.RANK_RTOL (the measured effect of a one-ulp logarithm, tests/test_rank_diag.py) —
one-workgroup and multi-workgroup ranks, the batched path through the scratch seam, a constant series, bad arguments, and a call between
two asynchronous steps."""
import ctypes as C

import numpy as np
import pytest

import common as cm
import rank_diag_ref as R

pytestmark = pytest.mark.gpu

N_SMALL, T_SMALL, GROUPS_SMALL, WINDOWS_SMALL = R.N_SMALL, R.T_SMALL, R.GROUPS_SMALL, R.WINDOWS_SMALL
BINS = (1, 7, 20)


def small_context(S, **kw):
    prob, opts = cm.serial_normal(**dict(R.SMALL_KW, **kw))
    h = S.hip_context(prob, opts)
    h.step(T_SMALL)
    return h


def small_calls(h):
    """every call of the small shape: [(arguments, result)]"""
    out = []
    for t0, t1 in WINDOWS_SMALL:
        for ml in (None, 2):
            for nb in BINS:
                kw = dict(t0=t0, t1=t1, max_lag=ml, n_bins=nb, groups=GROUPS_SMALL)
                out.append((kw, h.rank_diag(**kw)))
    return out


def ref_of(hist, kw):
    with np.errstate(invalid="ignore", divide="ignore"):
        return R.rank_diag_from_history(hist, kw["t0"], kw["t1"], kw.get("max_lag"), kw.get("n_bins", 20), kw.get("groups"), kw.get("n_groups"))


def test_small_shape_against_the_restatement(S):
    h = small_context(S)
    hist = h.history(0, T_SMALL)
    for kw, got in small_calls(h):
        want = ref_of(hist, kw)
        print(kw["t0"], kw["t1"], kw["max_lag"], kw["n_bins"], "status", want["status"].tolist(), "left out", R.near_sign_change(want).sum())
        R.assert_rank_diag_close(got, want)
        assert got["rank_hist"].shape == (kw["n_bins"], 3, N_SMALL)
        assert (got["rank_hist"].sum(axis=0)[:, GROUPS_SMALL >= 0] == 2 * ((kw["t1"] - kw["t0"]) // 2)).all()
        assert (got["rank_hist"][:, :, GROUPS_SMALL < 0] == 0).all()
        if kw["max_lag"] == 2:                              # one pair only: never truncated
            assert np.isin(want["status"][[0, 2, 3]], (1, 2)).all() and (want["status"] == 1).any()


def test_ranks_over_many_workgroups(S):
    T = R.T_LARGE                                       # M = 2 x 16 x 300 = 9600 > 8192, and a group of 2 (M = 1200) in the same call
    prob, opts = cm.serial_normal(**R.LARGE_KW)
    h = S.hip_context(prob, opts)
    h.step(T)
    kw = dict(t0=0, t1=T, n_bins=20, groups=R.GROUPS_LARGE)
    got = h.rank_diag(**kw)
    want = ref_of(h.history(0, T), kw)
    print("status", want["status"].tolist(), "ess_bulk", want["ess_bulk"].tolist(), "rhat", want["rhat_rank"].tolist())
    R.assert_rank_diag_close(got, want)
    # at least 90 % of the cells of the small and the large shape have status 0 in the restatement
    hs = small_context(S).history(0, T_SMALL)
    cells = [want] + [ref_of(hs, dict(t0=t0, t1=t1, n_bins=0, groups=GROUPS_SMALL)) for t0, t1 in WINDOWS_SMALL]
    print("status 0:", [(c["status"] == 0).all(axis=0).tolist() for c in cells])
    assert R.share_of_cells_with_status_0(cells) >= 0.9


def test_a_population_that_has_not_mixed(S):
    """the example's temperature ladder with its exchange, from one starting point: rho_t stays up, max_lag comes first"""
    h = small_context(S, sigma0=0.05, maxtemp=5.0, p2_bounds=(-20.0, 20.0), mom=(-1.0, 10.0), min_improve=0.0, acc_tuners=None, seed=12)
    kw = dict(t0=0, t1=T_SMALL, n_bins=7, groups=GROUPS_SMALL)
    want = ref_of(h.history(0, T_SMALL), kw)
    R.assert_rank_diag_close(h.rank_diag(**kw), want)
    assert (want["status"][0] == 1).sum() >= 6


def test_batched_path_equals_the_unbatched_one(S, monkeypatch, hooks):
    base = [r for _, r in small_calls(small_context(S))]
    monkeypatch.setenv("SMMHIP_STATS_SCRATCH", "1")     # the smallest batch: one series of as many groups as one column's bytes hold
    h = small_context(S)
    monkeypatch.delenv("SMMHIP_STATS_SCRATCH")
    for (kw, got), want in zip(small_calls(h), base):
        for f in want:
            assert np.array_equal(got[f], want[f], equal_nan=want[f].dtype.kind == "f"), (kw, f)


def test_a_constant_series_is_undefined(S):
    A = S._abi
    prob, opts = cm.serial_normal(N=16, T=24, ns=100, objective_id=A.SMM_OBJ_NORM_FAILBOX, obj_params=[-3.0 + 1e-9, 3.0])
    prob.init[:] = [-3.0, -0.2]                          # every candidate fails: nothing is accepted after the first row
    h = S.hip_context(prob, opts)
    h.step(24)
    hist = h.history(0, 24)
    assert (hist.accepted[1:] == 0).all() or (hist.params[1:] == hist.params[0]).all()
    kw = dict(t0=2, t1=24, n_bins=4, groups=np.arange(16) // 8)
    got = h.rank_diag(**kw)
    R.assert_rank_diag_close(got, ref_of(hist, kw))
    assert (got["status"][:3, :, :2] == 2).all() and np.isnan(got["ess_bulk"][:, :2]).all() and np.isnan(got["rhat_rank"][:, :2]).all()
    assert (got["rank_hist"][:, :2, :].sum(axis=0) == 22).all()


def test_invalid_arguments_leave_the_outputs_untouched(S):
    A = S._abi
    prob, opts = cm.serial_normal(N=16, T=30, ns=100)
    h = S.hip_context(prob, opts)
    h.step(20)
    fn = h._fn("get_rank_diag")
    g = np.zeros(16, np.int32)
    gp = g.ctypes.data_as(A.c_int32_p)
    bad_id, low_id = g.copy(), g.copy()
    bad_id[3], low_id[5] = 1, -2
    sent = {f: np.full((1, 3), -7.5) for f in R.FLOATS}
    sent.update(status=np.full((4, 1, 3), -7, np.int32), rank_hist=np.full((4, 3, 16), -7, np.int64))
    out = h._out(A.smm_rank_diag_t, sent)
    no_hist = h._out(A.smm_rank_diag_t, sent, ("rank_hist",))
    cases = [
        (None, 0, 20, 5, 4, gp, 1, out), (h._ctx, 0, 20, 5, 4, gp, 1, None),
        (h._ctx, -1, 10, 3, 4, gp, 1, out), (h._ctx, 0, 21, 5, 4, gp, 1, out),                    # the window
        (h._ctx, 5, 12, 2, 4, gp, 1, out),                                                         # n = 7 < 8
        (h._ctx, 0, 20, 0, 4, gp, 1, out), (h._ctx, 0, 20, 10, 4, gp, 1, out),                     # max_lag outside [1, h - 1]
        (h._ctx, 0, 20, 5, -1, gp, 1, no_hist), (h._ctx, 0, 20, 5, 0, gp, 1, out),                 # n_bins < 0; rank_hist without bins
        (h._ctx, 0, 20, 5, 4, gp, 0, out), (h._ctx, 0, 20, 5, 4, gp, -1, out),                     # n_groups < 1
        (h._ctx, 0, 20, 5, 4, None, 2, out),                                                       # group NULL with n_groups != 1
        (h._ctx, 0, 20, 5, 4, bad_id.ctypes.data_as(A.c_int32_p), 1, out),                         # a group id outside [-1, n_groups)
        (h._ctx, 0, 20, 5, 4, low_id.ctypes.data_as(A.c_int32_p), 1, out),
    ]
    for args in cases:
        a = list(args)
        a[7] = C.byref(a[7]) if a[7] is not None else None
        assert fn(*a) == A.SMM_ERR_INVALID_ARG, args[1:7]
        for f, v in sent.items():
            assert (v == (-7.5 if v.dtype.kind == "f" else -7)).all(), (args[1:7], f)
    for kw in (dict(t0=5, t1=12), dict(t0=0, t1=20, max_lag=10), dict(t0=0, t1=20, n_bins=-1), dict(t0=0, t1=20, groups=np.full(16, -1))):
        with pytest.raises((ValueError, S.SMMHipError)):
            h.rank_diag(**kw)
    assert fn(h._ctx, 0, 20, 9, 4, None, 1, C.byref(out)) == A.SMM_OK                              # group NULL: every chain in group 0
    assert (sent["rank_hist"].sum(axis=0) == 20).all() and (sent["status"] != -7).all()
    assert fn(h._ctx, 0, 20, 9, 0, None, 1, C.byref(A.smm_rank_diag_t())) == A.SMM_OK              # (nothing requested: valid)
    h.step(10)                                                                                     # the context still runs
    assert h.state().iter == 30


def test_a_call_between_asynchronous_steps_leaves_the_run_untouched(S):
    prob, opts = cm.serial_normal(N=64, T=60, ns=100)
    a = S.hip_context(prob, opts)
    b = S.hip_context(prob, opts)
    a.step(60)
    b.step_async(30)
    first = b.rank_diag(0, 30, groups=np.arange(64) % 4)
    b.step_async(30)
    again = b.rank_diag(0, 30, groups=np.arange(64) % 4)
    for f in first:
        assert np.array_equal(first[f], again[f], equal_nan=first[f].dtype.kind == "f"), f
    cm.assert_history_equal(a.history(), b.history(), exact_floats=True)
    cm.assert_state_equal(a.state(), b.state(), rtol=0)
