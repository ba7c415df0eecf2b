"""smm_get_reweighted on the device (include/smmhip.h, smm.jl_amd/csrc/smm_reweight.hpp): every output equal (array_equal, NaN equal to
NaN) to the numerical contract restated in reweight_ref.py over the history downloaded with smm_get_history of the same context.  A small
serialNormal with distinct acc_tuner per chain, uneven groups, the three selections, a window inside the run and an empty one, targets
below, at, between and above the chains' and outputs left NULL; the dense objective with np = 5, nm = 7; a pooled column past one chunk,
alone and through the scratch seam; one chain past one chunk of scored rows; 64 targets; reweight_craft.py's crafted history; every
refusal; a twin context that never asked; two p2p shards; the host layer."""
import ctypes as C

import numpy as np
import pytest

import common as cm
import moment_stats_ref as MR
import rank_diag_ref as RD
import reweight_craft as RC
import reweight_ref as RW

pytestmark = pytest.mark.gpu

PROBS = (0.0, 0.025, 0.5, 0.975, 1.0)


def check(h, hist, acc, t0, t1, select, groups, targets, probs=PROBS, n_groups=None, chain_offset=0):
    got = h.reweighted(t0, t1, select, groups, targets, probs, n_groups=n_groups)
    want = RW.reweighted_from_history(hist, t0, t1, select, groups, targets, probs, acc, n_groups=n_groups, chain_offset=chain_offset)
    RW.assert_reweighted_equal(got, want)
    return got


def raw(h, A, arrays, t0, t1, select, g, ng, targets, nt, probs, skip=()):
    s = h._out(A.smm_reweighted_t, arrays, skip)
    gp = None if g is None else g.ctypes.data_as(A.c_int32_p)
    p = None if probs is None else A.f64(probs)
    tg = None if targets is None else A.f64(targets)
    return h._fn("get_reweighted")(h._ctx, t0, t1, select, gp, ng, None if tg is None else A.dptr(tg), nt,
                                   None if p is None else A.dptr(p), 0 if p is None else len(p), C.byref(s))


def sentinel(G, N, R, npar, nm, nq):
    i64, i32, f = (lambda *s: np.full(s, -7, np.int64)), (lambda *s: np.full(s, -7, np.int32)), (lambda *s: np.full(s, -7.5))
    return dict(count=i64(G), n_scored=i64(G), n_chains=i32(G), status=i32(R, G), chain_n=i32(N), chain_ess=f(R, N), chain_logz=f(R, N),
                n_kept=i64(R, G), sum_u=f(R, G), ess=f(R, G), mean=f(R, G, npar), cov=f(R, G, npar, npar), value_mean=f(R, G),
                m_mean=f(R, G, nm), quantile=f(nq, R, G, npar))


def untouched(a, fields=None):
    return all((a[f] == (-7.5 if a[f].dtype.kind == "f" else -7)).all() for f in (fields or a))


N1, T1 = 8, 40
G1 = np.array([0, 1, 1, -1, 3, 0, 3, 3], np.int32)       # three groups, a chain in no group and group 2 without a member
ACC1 = np.array([0.2, 0.3, 0.45, 0.6, 0.8, 1.1, 1.5, 2.0])
SMALL = dict(RD.MIXING, N=N1, T=T1, acc_tuners=ACC1, seed=4)
TARGETS1 = (0.0, 2.0, 0.5, 3.5)                          # the prior, the coldest chain's, between two chains, above all


@pytest.fixture(scope="module")
def small(S):
    prob, opts = cm.serial_normal(**SMALL)
    h = S.hip_context(prob, opts)
    h.step(T1)
    return h, prob, h.history(0, T1)


def test_small_serial_normal_selections_windows_targets_and_null_outputs(S, small):
    h, prob, hist = small
    A = S._abi
    seen = set()
    for select in (0, 1, 2):
        for t0, t1 in ((0, T1), (7, 33)):
            for probs in ((), PROBS):
                got = check(h, hist, ACC1, t0, t1, select, G1, TARGETS1, probs, n_groups=4)
                assert got["n_chains"].tolist() == [2, 2, 0, 3] and (got["status"][:, 2] == 1).all() and got["chain_n"][3] == 0
                seen.update(got["status"].ravel().tolist())
    assert 0 in seen, seen
    st = h.reweighted(0, T1, 2, G1, TARGETS1, PROBS, n_groups=4)
    assert (st["status"][:, [0, 1, 3]] == 0).all() and (st["ess"][:, [0, 1, 3]] >= 1).all() and (st["n_scored"] <= st["count"]).all()
    check(h, hist, ACC1, 0, T1, 2, None, (1.0,))                                # no group vector: every chain in group 0
    got = check(h, hist, ACC1, 12, 12, 1, G1, TARGETS1, n_groups=4)             # an empty window
    assert (got["status"] == 1).all() and (got["chain_ess"] == 0).all() and np.isnan(got["chain_logz"]).all()
    want = RW.reweighted_from_history(hist, 7, 33, 2, G1, TARGETS1, PROBS, ACC1, n_groups=4)
    for f in RW.FIELDS:                                    # each output left NULL in turn
        a = sentinel(4, N1, 4, 2, 2, 5)
        assert raw(h, A, a, 7, 33, 2, G1, 4, TARGETS1, 4, PROBS, skip=[f]) == A.SMM_OK
        RW.assert_reweighted_equal(a, want, [k for k in RW.FIELDS if k != f])
        assert untouched(a, [f]), f
    for keep in (("chain_logz",), ("count", "chain_n"), ("quantile",), ("cov", "status"), ("mean", "n_kept")):
        a = sentinel(4, N1, 4, 2, 2, 5)
        assert raw(h, A, a, 7, 33, 2, G1, 4, TARGETS1, 4, PROBS, skip=[f for f in RW.FIELDS if f not in keep]) == A.SMM_OK
        RW.assert_reweighted_equal(a, want, keep)
        assert untouched(a, [f for f in RW.FIELDS if f not in keep]), keep


def test_sixty_four_targets(S, small):
    h, prob, hist = small
    targets = tuple(np.linspace(0.0, 3.0, 64))
    got = check(h, hist, ACC1, 3, T1, 2, G1, targets, (0.5,), n_groups=4)
    assert got["quantile"].shape == (1, 64, 4, 2) and got["chain_logz"].shape == (64, N1)


def test_dense_objective_with_np_5_and_nm_7(S):
    prob, opts = MR.dense_problem(5, 7, N=16, T=64)
    h = S.hip_context(prob, opts)
    h.step(64)
    hist = h.history(0, 64)
    g = (np.arange(16) % 2).astype(np.int32)
    for select in (0, 1, 2):
        got = check(h, hist, opts.acc_tuner, 0, 64, select, g, (20.0, 5.0))
        assert got["cov"].shape == (2, 2, 5, 5) and got["m_mean"].shape == (2, 2, 7) and got["quantile"].shape == (5, 2, 2, 5)
    check(h, hist, opts.acc_tuner, 9, 50, 2, g, (1.0,), (0.5,))


def test_a_pooled_column_past_one_chunk_alone_and_in_batches(S, hooks, monkeypatch):
    N, T = 16, 600
    acc = np.geomspace(2.0, 0.25, N)
    prob, opts = cm.serial_normal(**dict(RD.MIXING, N=N, T=T, acc_tuners=acc, seed=1))
    h0 = S.hip_context(prob, opts)
    h0.step(T)
    hist = h0.history(0, T)
    targets = (2.0, 0.7)
    want = check(h0, hist, acc, 0, T, 0, None, targets, (0.1, 0.5))   # 9600 > 8192 pooled rows: two chunks
    assert want["count"].tolist() == [N * T] and (want["status"] == 0).all()
    cap = 4096
    monkeypatch.setenv("SMMHIP_STATS_SCRATCH", str(cap))
    h = S.hip_context(prob, opts)                          # (the seam is read at creation)
    monkeypatch.delenv("SMMHIP_STATS_SCRATCH")
    h.set_state(h0.state(), hist)
    # smm_reducers_host.hpp's plan under the seam: five pooled columns and one chunk of the D + 3 = 7 columns are the minimum
    col8, chunk8 = N * T * 8, 7 * 8192 * 8
    avail = max(cap, 5 * col8 + chunk8) - 5 * col8
    Nbc = max(1, min(2, avail // 2 // chunk8, cap // (2 * 2 * 8)))
    jb = min(2, 1 + (avail - Nbc * chunk8) // col8)
    assert Nbc == 1 and jb == 1                            # the two chunks one at a time, and the select's parameters one at a time
    RW.assert_reweighted_equal(h.reweighted(0, T, 0, None, targets, (0.1, 0.5)), want)
    g = (np.arange(N) % 3).astype(np.int32)
    RW.assert_reweighted_equal(h.reweighted(11, 590, 2, g, targets, (0.1, 0.5)), h0.reweighted(11, 590, 2, g, targets, (0.1, 0.5)))
    check(h0, hist, acc, 11, 590, 2, g, (0.7,), (0.5,))
    cm.assert_history_equal(h.history(0, T), hist, exact_floats=True)


def test_one_chain_past_one_chunk_of_scored_rows(S):
    N, T = 2, 8200
    acc = np.array([1.0, 0.5])
    prob, opts = cm.serial_normal(N=N, T=T, ns=100, acc_tuners=acc, seed=2)
    h = S.hip_context(prob, opts)
    h.step(T)
    hist = h.history(0, T)
    got = check(h, hist, acc, 0, T, 0, np.array([0, 1], np.int32), (1.0, 0.75), (0.5,))
    assert got["chain_n"].tolist() == [T, T] and (got["status"] == 0).all()


def test_crafted_history_status_table_and_every_refusal(S, small):
    h0, prob, hist = small
    A = S._abi
    cprob, copts = cm.serial_normal(**dict(SMALL, acc_tuners=RC.CRAFT_ACC))
    hc0 = S.hip_context(cprob, copts)
    hc0.step(T1)
    crafted, info = RC.crafted(into=MR.copy_history(hc0.history(0, T1)))
    h = S.hip_context(cprob, copts)
    h.set_state(hc0.state(), crafted)
    back = h.history(0, T1)
    got = check(h, back, info["acc"], 0, T1, 0, info["groups"], info["targets"], info["probs"])
    assert np.array_equal(got["status"], info["status"]) and np.array_equal(got["chain_n"], info["chain_n"])
    assert got["chain_ess"][0, 3] == info["chain3"]["ess"] and np.array_equal(got["quantile"][:, 0, 4], info["quantile4"])
    assert (got["chain_ess"][:, 1] == 0.0).all() and np.isnan(got["chain_logz"][:, 1]).all() and (got["chain_ess"][:, 2] == 1.0).all()
    for select in (1, 2):
        check(h, back, info["acc"], 0, T1, select, info["groups"], info["targets"], info["probs"])
    one = np.full(N1, -1, np.int32)
    one[5] = 1
    got = check(h0, hist, ACC1, 10, 11, 0, one, (1.0,), n_groups=2)   # fewer than two rows: no member, and one chain over one iteration
    assert got["status"].tolist() == [[1, 1]] and got["count"].tolist() == [0, 1] and np.isnan(got["sum_u"]).all()

    bad_id, low_id = G1.copy(), G1.copy()
    bad_id[3], low_id[5] = 4, -2
    ok = dict(t0=3, t1=T1, select=2, g=G1, ng=4, targets=TARGETS1, nt=4, probs=PROBS)
    bad = [dict(t0=-1), dict(t1=T1 + 1), dict(t0=9, t1=8), dict(select=3), dict(select=-1), dict(ng=-1), dict(g=None, ng=2),
           dict(g=None, ng=0), dict(g=bad_id), dict(g=low_id), dict(probs=(0.5, 1.5)), dict(probs=(np.nan,)), dict(probs=None),
           dict(nt=0), dict(nt=-1), dict(targets=tuple(np.linspace(0, 1, 65)), nt=65), dict(targets=None),
           dict(targets=(0.5, -1e-9, 1.0, 2.0)), dict(targets=(np.nan, 1.0, 1.0, 1.0)), dict(targets=(1.0, 1.0, 1.0, np.inf))]
    for b in bad:
        k = dict(ok, **b)
        a = sentinel(4, N1, 4, 2, 2, 5)
        rc = raw(h0, A, a, k["t0"], k["t1"], k["select"], k["g"], k["ng"], k["targets"], k["nt"], k["probs"])
        assert rc == A.SMM_ERR_INVALID_ARG, b
        assert len(h0._fn("last_error")(h0._ctx).decode()) > 0 and untouched(a), b
    a = sentinel(4, N1, 4, 2, 2, 5)
    assert raw(h0, A, a, 3, T1, 2, G1, 4, TARGETS1, 4, PROBS) == A.SMM_OK and not untouched(a, ["status", "quantile", "chain_logz"])
    fn = h0._fn("get_reweighted")
    a = sentinel(4, N1, 4, 2, 2, 5)
    s = h0._out(A.smm_reweighted_t, a)
    gp, pp, tg = G1.ctypes.data_as(A.c_int32_p), A.f64(PROBS), A.f64(TARGETS1)
    assert fn(None, 3, T1, 2, gp, 4, A.dptr(tg), 4, A.dptr(pp), 5, C.byref(s)) == A.SMM_ERR_INVALID_ARG
    assert fn(h0._ctx, 3, T1, 2, gp, 4, A.dptr(tg), 4, A.dptr(pp), 5, None) == A.SMM_ERR_INVALID_ARG and untouched(a)
    with pytest.raises(S.SMMHipError):
        h0.reweighted(0, T1, 5)


@pytest.mark.parametrize("persistent", (True, False))
def test_a_call_between_steps_leaves_the_run_untouched(S, persistent):
    prob, opts = cm.serial_normal(N=256, T=60)
    a, b = S.hip_context(prob, opts), S.hip_context(prob, opts)
    for h in (a, b):
        h.set_persistent(persistent)
        h.step(30)
    hist, state = b.history(0, 30), b.state()
    g = (np.arange(256) % 3).astype(np.int32)
    for select in (0, 2):
        check(b, hist, opts.acc_tuner, 5, 30, select, g, (20.0, 3.0), (0.5,))
    cm.assert_history_equal(b.history(0, 30), hist, exact_floats=True)
    cm.assert_state_equal(b.state(), state, rtol=0)
    for h in (a, b):
        h.step(30)
        assert (h.persistent_info()[1] >= 1) == persistent
    cm.assert_history_equal(a.history(), b.history(), exact_floats=True)
    cm.assert_state_equal(a.state(), b.state(), rtol=0)


def test_p2p_shards_report_their_own_chains(S):
    from test_gpu_p2p import p2p_contexts, p2p_run_lockstep
    prob, opts = cm.serial_normal(N=64, T=30, ns=1000)
    ctxs = p2p_contexts(S, prob, opts, 2)
    p2p_run_lockstep(ctxs, 30)
    g3 = (np.arange(32) % 3).astype(np.int32)
    g3[5] = -1
    for r, c in enumerate(ctxs):
        hist = c.history(0, 30)
        assert hist.value.shape[1] == 32
        for select in (0, 1, 2):
            check(c, hist, opts.acc_tuner, 3, 30, select, g3, (20.0, 2.0), (0.5,), chain_offset=32 * r)
        check(c, hist, opts.acc_tuner, 0, 30, 2, None, (5.0,), (), chain_offset=32 * r)


def test_host_tempered_and_ladder_logz_read_the_device(S, monkeypatch):
    from collections import OrderedDict
    Nh, Th = 64, 80
    m = S.MProb()
    S.addSampledParam(m, OrderedDict([("p1", [0.2, -3, 3]), ("p2", [-0.2, -20, 20])]))
    S.addMoment(m, {"name": ["mu1", "mu2"], "value": [-1.0, 10.0], "weight": [1.0, 2.0]})
    S.addEvalFunc(m, S.objfunc_norm)
    acc = np.array([2.0] * 32 + [1.0] * 16 + [2.0] * 8 + [0.5] * 8)
    MA = S.MAlgoBGP(m, {"N": Nh, "maxiter": Th, "maxtemp": 5, "sigma": 0.05, "min_improve": [0.0] * Nh, "acc_tuners": list(acc)})
    S.run(MA)
    hist = MA._ctx.history(0, Th)
    MA._hist = None

    def no_download(*a, **k):
        raise AssertionError("the history was downloaded")
    monkeypatch.setattr(type(MA._ctx), "history", no_download)
    ps, ms = S.ps2s_names(m), S.ms_names(m)
    per = np.array([0] * 32 + [1] * 16 + [0] * 8 + [-1] * 8, np.int32)
    for kw, sel, target, groups, t0, t1 in ((dict(), 2, 2.0, None, 0, Th),
                                            (dict(target=1.0, per=per, window=(10, 70), state=False, level=0.9), 1, 1.0, per, 10, 70)):
        level = kw.get("level", 0.95)
        q = ((1 - level) / 2, 1 - (1 - level) / 2)
        want = RW.reweighted_from_history(hist, t0, t1, sel, groups, (target,), q, acc)
        got = S.tempered(MA, **kw)
        assert len(got) == len(want["count"])
        for g, r in enumerate(got):
            assert r["target"] == target and r["count"] == want["count"][g] and r["n_scored"] == want["n_scored"][g]
            assert r["chains"] == want["n_chains"][g] and r["status"] == want["status"][0, g] and r["n_kept"] == want["n_kept"][0, g]
            assert np.array_equal([r["ess"], r["value_mean"]], [want["ess"][0, g], want["value_mean"][0, g]], equal_nan=True)
            assert list(r["mean"]) == list(r["sd"]) == list(r["band"]) == ps and list(r["m_mean"]) == ms
            assert np.array_equal(r["cov"], want["cov"][0, g], equal_nan=True)
            for j, p in enumerate(ps):
                assert np.array_equal([r["mean"][p], r["sd"][p]], [want["mean"][0, g, j], np.sqrt(want["cov"][0, g, j, j])], equal_nan=True)
                assert np.array_equal(r["band"][p], want["quantile"][:, 0, g, j], equal_nan=True)
            for k, name in enumerate(ms):
                assert np.array_equal(r["m_mean"][name], want["m_mean"][0, g, k], equal_nan=True)
    lad = S.ladder_logz(MA)
    want = RW.reweighted_from_history(hist, 0, Th, 2, None, (1.0, 2.0), (), acc, want_cov=False)
    assert lad["acc_tuner"].tolist() == [0.5, 1.0, 2.0] and lad["n_chains"].tolist() == [8, 16, 40]
    step = [want["chain_logz"][0, acc == 0.5].mean(), want["chain_logz"][1, acc == 1.0].mean()]
    assert np.array_equal(lad["step"], step) and np.array_equal(lad["logz"], np.concatenate([[0.0], np.cumsum(step)]))
