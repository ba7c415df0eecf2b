"""smm_get_moment_stats on the device (include/smmhip.h, smm.jl_amd/csrc/smm_moments.hpp): every output equal (array_equal, NaN equal to
NaN, so the medians and quantiles up to the sign of a zero) to the numerical contract restated in moment_stats_ref.py over the history
downloaded with smm_get_history of the same context.  A small serialNormal with uneven groups, all three selections, a window that
starts inside the run and outputs left NULL; the dense objective with np = 5, nm = 7; a pooled column past one chunk, alone and through
the scratch seam; the status table on crafted histories and the bad arguments; a twin context that never asked; two p2p shards; the
host layer."""
import ctypes as C

import numpy as np
import pytest

import common as cm
import moment_stats_ref as MR
import rank_diag_ref as RD

pytestmark = pytest.mark.gpu

PROBS = (0.025, 0.5, 0.975)


def check(h, prob, hist, t0, t1, select, groups, probs=PROBS, ridge=0.0, n_groups=None):
    got = h.moment_stats(t0, t1, select, groups, probs, ridge, n_groups=n_groups)
    want = MR.moment_stats_from_history(hist, t0, t1, select, groups, probs, ridge, prob.mom, prob.w, n_groups=n_groups)
    MR.assert_moment_stats_equal(got, want)
    return got


def raw(h, A, t0, t1, select, g, ng, probs, ridge, arrays, skip=()):
    s = h._out(A.smm_moment_stats_t, arrays, skip)
    gp = None if g is None else g.ctypes.data_as(A.c_int32_p)
    p = None if probs is None else A.f64(probs)
    return h._fn("get_moment_stats")(h._ctx, t0, t1, select, gp, ng, None if p is None else A.dptr(p), 0 if p is None else len(p), ridge,
                                     C.byref(s))


def sentinel(G, npar, nm, nq):
    return dict(count=np.full(G, -7, np.int64), n_chains=np.full(G, -7, np.int32), status=np.full(G, -7, np.int32),
                p_mean=np.full((G, npar), -7.5), m_mean=np.full((G, nm), -7.5), m_median=np.full((G, nm), -7.5),
                m_quantile=np.full((nq, G, nm), -7.5), cov_pp=np.full((G, npar, npar), -7.5), cov_pm=np.full((G, npar, nm), -7.5),
                cov_mm=np.full((G, nm, nm), -7.5), fit_z=np.full((G, nm), -7.5), jac=np.full((G, nm, npar), -7.5),
                sens=np.full((G, npar, nm), -7.5), se=np.full((G, npar), -7.5))


def untouched(a, fields=None):
    return all((a[f] == (-7.5 if a[f].dtype.kind == "f" else -7)).all() for f in (fields or a))


N1, T1 = 8, 40
G1 = np.array([0, 1, 1, -1, 3, 0, 3, 3], np.int32)       # three groups, a chain in no group and group 2 without a member


@pytest.fixture(scope="module")
def small(S):
    prob, opts = cm.serial_normal(**dict(RD.MIXING, N=N1, T=T1, acc_tuners=0.5, seed=4))
    h = S.hip_context(prob, opts)
    h.step(T1)
    return h, prob, h.history(0, T1)


def test_small_serial_normal_all_selections_windows_and_null_outputs(S, small):
    h, prob, hist = small
    A = S._abi
    for select in (0, 1, 2):
        for t0, t1 in ((0, T1), (7, 33)):                 # t0 > 0: the state series looks back before the window
            for probs in ((), PROBS):
                got = check(h, prob, hist, t0, t1, select, G1, probs, n_groups=4)
            assert got["n_chains"].tolist() == [2, 2, 0, 3] and got["status"].tolist() == [0, 0, 1, 0], (select, got["status"])
            if select == 1:                                # the cov_pp block is smm_get_group_stats' covariance, bit for bit
                gs = h.group_stats(t0, t1, True, G1, (), n_groups=4)
                assert np.array_equal(got["cov_pp"], gs["cov"], equal_nan=True) and np.array_equal(got["p_mean"], gs["mean"], equal_nan=True)
    acc = hist.accepted != 0
    assert (~acc[7:12]).any(), "no rejected row just inside the window: the look-back is not exercised"
    check(h, prob, hist, 0, T1, 2, None, PROBS, ridge=1e-6)                     # no group vector: every chain in group 0
    check(h, prob, hist, 12, 12, 1, G1, PROBS, n_groups=4)                      # an empty window
    want = MR.moment_stats_from_history(hist, 7, 33, 2, G1, PROBS, 0.0, prob.mom, prob.w, n_groups=4)
    for keep in (("count", "status"), ("m_mean", "fit_z"), ("se",), ("m_quantile", "jac"), ("cov_pm", "n_chains")):
        a = sentinel(4, 2, 2, 3)
        assert raw(h, A, 7, 33, 2, G1, 4, PROBS, 0.0, a, skip=[f for f in MR.FIELDS if f not in keep]) == A.SMM_OK
        MR.assert_moment_stats_equal(a, want, keep)
        assert untouched(a, [f for f in MR.FIELDS if f not in keep]), keep


def test_dense_objective_with_np_5_and_nm_7(S):
    prob, opts = MR.dense_problem(5, 7, N=16, T=64)
    h = S.hip_context(prob, opts)
    h.step(64)
    hist = h.history(0, 64)
    g = (np.arange(16) % 2).astype(np.int32)
    for select in (0, 1, 2):
        got = check(h, prob, hist, 0, 64, select, g)
        assert got["cov_pm"].shape == (2, 5, 7) and got["jac"].shape == (2, 7, 5) and (got["status"] == 0).all()
    check(h, prob, hist, 9, 50, 2, g, (0.5,), ridge=1e-8)


def test_a_pooled_column_past_one_chunk_alone_and_in_batches(S, hooks, monkeypatch):
    N, T = 24, 400
    prob, opts = cm.serial_normal(**dict(RD.MIXING, N=N, T=T, acc_tuners=1.0, seed=1))
    h0 = S.hip_context(prob, opts)
    h0.step(T)
    hist = h0.history(0, T)
    want = check(h0, prob, hist, 0, T, 0, None)           # 9600 > 8192 pooled rows: two chunks, the grid-wide select
    assert want["count"].tolist() == [N * T] and want["status"].tolist() == [0]
    cap = 4096
    monkeypatch.setenv("SMMHIP_STATS_SCRATCH", str(cap))
    h = S.hip_context(prob, opts)                          # (the seam is read at creation)
    monkeypatch.delenv("SMMHIP_STATS_SCRATCH")
    h.set_state(h0.state(), hist)
    # smm_reducers_host.hpp's plan under the seam: one pooled column and one chunk of the D = 4 joint columns are the minimum
    D, Mtot = 4, N * T
    budget = max(cap, Mtot * 8, D * 8192 * 8)
    kb, Nbc = min(D, budget // (Mtot * 8)), max(1, min(2, budget // (D * 8192 * 8), cap // (D * D * 8)))
    assert kb < D and Nbc == 1                             # the columns in more than one batch, and the two chunks one at a time
    got = check(h, prob, hist, 0, T, 0, None)
    MR.assert_moment_stats_equal(got, want)
    g = (np.arange(N) % 3).astype(np.int32)
    MR.assert_moment_stats_equal(check(h, prob, hist, 11, 390, 2, g), h0.moment_stats(11, 390, 2, g, PROBS))
    cm.assert_history_equal(h.history(0, T), hist, exact_floats=True)


def test_status_table_on_crafted_histories_and_invalid_arguments(S, small):
    h0, prob, hist = small
    A = S._abi
    st = h0.state()
    mem = np.flatnonzero(G1 == 3)
    c = MR.copy_history(hist)
    c.sim_moments[20, 1, 1], c.accepted[20, 1] = np.nan, 1  # group 1 (chains 1, 2): a NaN moment in a row the state series reads
    c.accepted[15:, mem] = 0                               # group 3: its state series never moves after row 14 ...
    c.params[:, 0, mem], c.params[:, 1, mem] = 0.5, -0.25  # ... and every member holds the same state, whose mean is exact
    h = S.hip_context(*cm.serial_normal(**dict(RD.MIXING, N=N1, T=T1, acc_tuners=0.5, seed=4)))
    h.set_state(st, c)
    back = h.history(0, T1)
    got = check(h, prob, back, 20, T1, 2, G1, n_groups=4)
    assert got["status"].tolist() == [0, 2, 1, 3], got["status"]
    assert np.isnan(got["m_mean"][1]).all() and np.isnan(got["cov_pp"][1]).all() and got["count"][1] == 40
    assert (got["cov_pp"][3] == 0).all() and np.isfinite(got["fit_z"][3]).all() and np.isnan(got["jac"][3]).all()
    one = np.full(N1, -1, np.int32)
    one[5] = 1
    got = check(h, prob, back, 10, 11, 0, one, n_groups=2)  # fewer than two rows: no member, and one chain over one iteration
    assert got["status"].tolist() == [1, 1] and got["count"].tolist() == [0, 1] and np.isfinite(got["m_median"][1]).all()
    c4 = MR.copy_history(hist)                             # moments that do not move, whose mean is exact: J = 0, J'WJ = 0
    c4.sim_moments[:, 0, mem], c4.sim_moments[:, 1, mem] = 0.5, -0.25
    h.set_state(st, c4)
    got = check(h, prob, h.history(0, T1), 0, T1, 0, G1, n_groups=4)
    assert got["status"].tolist() == [0, 0, 1, 4] and (got["jac"][3] == 0).all() and np.isnan(got["sens"][3]).all()
    p53, o53 = MR.dense_problem(5, 3, N=8, T=64)           # nm < np: J'WJ is rank-deficient, its last pivots are rounding noise
    d = S.hip_context(p53, o53)
    d.step(64)
    got = check(d, p53, d.history(0, 64), 0, 64, 0, None)
    print("nm < np:", got["status"])
    assert got["status"][0] in (0, 4)                      # (4 on the history of the CPU oracle: tests/test_moment_stats.py)

    bad_id, low_id = G1.copy(), G1.copy()
    bad_id[3], low_id[5] = 4, -2
    ok = dict(t0=3, t1=T1, select=2, g=G1, ng=4, probs=PROBS, ridge=0.0)
    bad = [dict(t0=-1), dict(t1=T1 + 1), dict(t0=9, t1=8), dict(select=3), dict(select=-1), dict(ng=-1), dict(g=None, ng=2),
           dict(g=None, ng=0), dict(g=bad_id), dict(g=low_id), dict(probs=(0.5, 1.5)), dict(probs=(np.nan,)), dict(probs=None),
           dict(ridge=-1e-9), dict(ridge=np.inf), dict(ridge=np.nan)]
    for b in bad:
        k = dict(ok, **b)
        a = sentinel(4, 2, 2, 3)
        assert raw(h0, A, k["t0"], k["t1"], k["select"], k["g"], k["ng"], k["probs"], k["ridge"], a) == A.SMM_ERR_INVALID_ARG, b
        assert len(h0._fn("last_error")(h0._ctx).decode()) > 0 and untouched(a), b
    fn = h0._fn("get_moment_stats")
    a = sentinel(4, 2, 2, 3)
    s = h0._out(A.smm_moment_stats_t, a)
    gp, pp = G1.ctypes.data_as(A.c_int32_p), A.f64(PROBS)
    assert fn(None, 3, T1, 2, gp, 4, A.dptr(pp), 3, 0.0, C.byref(s)) == A.SMM_ERR_INVALID_ARG
    assert fn(h0._ctx, 3, T1, 2, gp, 4, A.dptr(pp), 3, 0.0, None) == A.SMM_ERR_INVALID_ARG and untouched(a)
    with pytest.raises(S.SMMHipError):
        h0.moment_stats(0, T1, 5)


@pytest.mark.parametrize("persistent", (True, False))
def test_a_call_between_steps_leaves_the_run_untouched(S, persistent):
    prob, opts = cm.serial_normal(N=256, T=60)
    a, b = S.hip_context(prob, opts), S.hip_context(prob, opts)
    for h in (a, b):
        h.set_persistent(persistent)
        h.step(30)
    hist, state = b.history(0, 30), b.state()
    g = (np.arange(256) % 3).astype(np.int32)
    for select in (0, 1, 2):
        check(b, prob, hist, 5, 30, select, g)
    cm.assert_history_equal(b.history(0, 30), hist, exact_floats=True)
    cm.assert_state_equal(b.state(), state, rtol=0)
    for h in (a, b):
        h.step(30)
        assert (h.persistent_info()[1] >= 1) == persistent
    cm.assert_history_equal(a.history(), b.history(), exact_floats=True)
    cm.assert_state_equal(a.state(), b.state(), rtol=0)


def test_p2p_shards_report_their_own_groups(S):
    from test_gpu_p2p import p2p_contexts, p2p_run_lockstep
    prob, opts = cm.serial_normal(N=64, T=30, ns=1000)
    ctxs = p2p_contexts(S, prob, opts, 2)
    p2p_run_lockstep(ctxs, 30)
    g3 = (np.arange(32) % 3).astype(np.int32)
    g3[5] = -1
    for c in ctxs:
        hist = c.history(0, 30)
        assert hist.value.shape[1] == 32
        for select in (0, 1, 2):
            check(c, prob, hist, 3, 30, select, g3)
        check(c, prob, hist, 0, 30, 2, None)


def test_host_moment_fit_and_sensitivity_read_the_device(S, monkeypatch):
    from collections import OrderedDict
    Nh, Th = 64, 80
    m = S.MProb()
    S.addSampledParam(m, OrderedDict([("p1", [0.2, -3, 3]), ("p2", [-0.2, -20, 20])]))
    S.addMoment(m, {"name": ["mu1", "mu2"], "value": [-1.0, 10.0], "weight": [1.0, 2.0]})
    S.addEvalFunc(m, S.objfunc_norm)
    acc = [2.0] * 32 + [1.0] * 16 + [2.0] * 8 + [0.5] * 8
    MA = S.MAlgoBGP(m, {"N": Nh, "maxiter": Th, "maxtemp": 5, "sigma": 0.05, "min_improve": [0.0] * Nh, "acc_tuners": acc})
    S.run(MA)
    hist = MA._ctx.history(0, Th)
    MA._hist = None

    def no_download(*a, **k):
        raise AssertionError("the history was downloaded")
    monkeypatch.setattr(type(MA._ctx), "history", no_download)
    groups = np.array([0] * 32 + [1] * 16 + [0] * 8 + [2] * 8, np.int32)
    ps, ms = S.ps2s_names(m), S.ms_names(m)
    assert ps == ["p1", "p2"] and ms == ["mu1", "mu2"]
    for kw, sel in ((dict(), 2), (dict(state=False, window=(10, 70)), 1), (dict(state=False, accepted_only=False), 0)):
        w = kw.get("window", (0, Th))
        level = 0.9
        q = ((1 - level) / 2, 1 - (1 - level) / 2)
        want = MR.moment_stats_from_history(hist, w[0], w[1], sel, groups, q, 0.0, [-1.0, 10.0], [1.0, 2.0])
        fit = S.moment_fit(MA, level=level, **kw)
        sen = S.sensitivity(MA, **kw)
        assert len(fit) == len(sen) == 3
        for g in range(3):
            f, s = fit[g], sen[g]
            assert f["count"] == s["count"] == want["count"][g] and f["chains"] == want["n_chains"][g] and f["status"] == s["status"] == want["status"][g]
            assert list(f["mean"]) == list(f["z"]) == list(s["jac"]) == ms and list(s["sens"]) == list(s["se"]) == ps
            assert [f["data"][k] for k in ms] == [-1.0, 10.0]
            for i, k in enumerate(ms):
                assert np.array_equal([f["mean"][k], f["median"][k], f["z"][k]], [want["m_mean"][g, i], want["m_median"][g, i], want["fit_z"][g, i]], equal_nan=True)
                assert np.array_equal(f["band"][k], want["m_quantile"][:, g, i], equal_nan=True)
                for j, p in enumerate(ps):
                    assert np.array_equal([s["jac"][k][p], s["sens"][p][k]], [want["jac"][g, i, j], want["sens"][g, j, i]], equal_nan=True)
            assert np.array_equal([s["se"][p] for p in ps], want["se"][g], equal_nan=True)
