"""smm_get_draws on the device (include/smmhip.h, smm.jl_amd/csrc/smm_draws.hpp) against the selection contract restated in draws_ref.py
over the history downloaded with smm_get_history of the same context: every array equal, the doubles bit for bit.  70 chains x 130
iterations (more than a wave of chains, three mask words with the last partial, a window that starts and ends inside words) with uneven
groups, all three selections, thinning and caps around a group's size; the look-back of the state series; one chain over one word and
over one word and a bit; an empty window; the batched path through the scratch seam; the calling protocol and the bad arguments; a
twin context that never asked; the host layer; two p2p shards."""
import ctypes as C

import numpy as np
import pytest

import common as cm
import draws_ref as DR

pytestmark = pytest.mark.gpu

N, T, T0, T1 = 70, 130, 3, 129
BIG = 1 << 20


def base_groups():
    """5 uneven groups: group 0 = 23 chains, group 1 = chain 40 alone, group 2 without a member, group 3 = 15 chains, group 4 = 25
    chains; 6 chains in no group"""
    g = np.full(N, -1, np.int32)
    g[1:25] = 0
    g[25:40] = 3
    g[40] = 1
    g[41:70] = 4
    g[[7, 45, 52, 59, 66]] = -1
    return g


def problem():
    return cm.general_normal(3, N=N, T=T, ns=200)       # np = nm = 3 (objfunc_norm has np == nm)


@pytest.fixture(scope="module")
def base(S):
    prob, opts = problem()
    h = S.hip_context(prob, opts)
    h.step(T)
    return h, h.history(0, T)


def check(h, hist, t0, t1, select, groups, thin, K, n_groups=None, chain_offset=0):
    got = h.draws(t0, t1, select, groups, thin, K, True, n_groups=n_groups)
    want = DR.draws_from_history(hist, t0, t1, select, groups, thin, K, n_groups=n_groups, chain_offset=chain_offset)
    DR.assert_draws_equal(got, want)
    return got


def test_base_case_selections_thinning_and_caps(base):
    h, hist = base
    g = base_groups()
    for select in (0, 1, 2):
        for thin in (1, 3):
            full = check(h, hist, T0, T1, select, g, thin, BIG, n_groups=5)          # a cap above every m_g
            m = full["count"]
            assert full["n_chains"].tolist() == [23, 1, 0, 15, 25] and m[2] == 0 and (m[[0, 1, 3, 4]] > 7).all(), m
            assert full["row0"][5] == m.sum() == len(full["value"])
            for K in (1, 7, int(m[3]), int(m[3]) - 1):
                got = check(h, hist, T0, T1, select, g, thin, K, n_groups=5)
                assert got["count"].tolist() == m.tolist() and np.diff(got["row0"]).tolist() == np.minimum(m, K).tolist()
    check(h, hist, T0, T1, 1, None, 1, 1000)                                          # no group vector: every chain in group 0
    check(h, hist, 0, T, 2, np.arange(N, dtype=np.int32), 2, 50)                      # a group per chain


def test_a_member_without_an_accepted_row_in_the_window(base):
    h, hist = base
    g = base_groups()
    acc = hist.accepted != 0
    found = None
    for L in (40, 20, 10, 5, 3, 2, 1):                   # the widest window in which a grouped chain accepts nothing while its group does
        for t0 in range(T0, T1 - L):
            none = ~acc[t0:t0 + L].any(axis=0)
            for c in np.flatnonzero(none & (g >= 0)):
                if (acc[t0:t0 + L][:, g == g[c]]).any():
                    found = (t0, t0 + L, c)
                    break
            if found:
                break
        if found:
            break
    assert found, "no window of the run leaves a grouped chain without an accepted row"
    t0, t1, c = found
    print("window", t0, t1, "chain", c, "group", g[c])
    for select in (1, 2):
        for thin in (1, 3):
            for K in (7, BIG):
                got = check(h, hist, t0, t1, select, g, thin, K, n_groups=5)
    one = check(h, hist, t0, t1, 1, np.where(np.arange(N) == c, 0, -1).astype(np.int32), 1, BIG, n_groups=1)
    assert one["count"].tolist() == [0] and one["row0"].tolist() == [0, 0] and one["params"].shape == (0, 3)


def test_state_rows_look_back_before_the_window(base):
    h, hist = base
    g = base_groups()
    for t0 in (T0, 64, 100):
        got = check(h, hist, t0, T1, 2, g, 1, BIG, n_groups=5)
        back = (got["src_iter"] > 0) & (got["src_iter"] < t0 + 1)
        assert back.any(), t0                             # a row before the window supplied a row of the window
        assert (got["iter"][back] >= t0 + 1).all() and (got["src_iter"] <= got["iter"]).all()


def test_one_chain_one_word_and_one_word_and_a_bit(S):
    for Tn in (64, 65):
        prob, opts = cm.serial_normal(N=1, T=Tn, ns=100, acc_tuners=[2.0])
        h = S.hip_context(prob, opts)
        h.step(Tn)
        hist = h.history(0, Tn)
        for select in (0, 1, 2):
            for thin, K in ((1, BIG), (2, 5), (64, BIG), (65, BIG)):
                check(h, hist, 0, Tn, select, None, thin, K)
            check(h, hist, Tn - 1, Tn, select, None, 1, BIG)
            check(h, hist, 63, Tn, select, None, 1, BIG)                                # (T = 64: the last bit; T = 65: the word's edge)
            empty = check(h, hist, 17, 17, select, np.zeros(1, np.int32), 1, 5, n_groups=3)
            assert empty["count"].tolist() == [0, 0, 0] and empty["row0"].tolist() == [0, 0, 0, 0] and len(empty["chain"]) == 0
            assert empty["n_chains"].tolist() == [1, 0, 0]


def test_batched_path_equals_the_unbatched_one(S, base, hooks, monkeypatch):
    h0, hist = base
    g = base_groups()
    cap = 1200
    monkeypatch.setenv("SMMHIP_STATS_SCRATCH", str(cap))
    prob, opts = problem()
    h = S.hip_context(prob, opts)                        # (the seam is read at creation)
    monkeypatch.delenv("SMMHIP_STATS_SCRATCH")
    h.step(T)
    cm.assert_history_equal(h.history(0, T), hist, exact_floats=True)
    scratch = min(N * T * (8 * 3 + 4), max(cap, 12 * T))  # smm_reducers_host.hpp: chain_stats_scratch_bytes, the first reducer call's
    rows_per_batch = cap // (8 * (3 + 1 + 3) + 12)
    for select in (0, 1, 2):
        for thin, K in ((1, 50), (3, BIG)):
            want = h0.draws(T0, T1, select, g, thin, K, True, n_groups=5)
            got = check(h, hist, T0, T1, select, g, thin, K, n_groups=5)
            DR.assert_draws_equal(got, want)
            R = int(want["row0"][5])
            assert -(-R // rows_per_batch) >= 3, (R, rows_per_batch)                    # the rows went out in at least 3 batches
            if select:
                W = -(-((T1 - T0) if select == 1 else T1) // 64)
                Nb = min(N, scratch // (12 * W))
                assert -(-N // Nb) >= 2, (Nb, W)                                        # the masks in at least 2 batches of chains
    cm.assert_history_equal(h.history(0, T), hist, exact_floats=True)


def raw(h, A, t0, t1, select, g, ng, thin, K, cap, arrays, skip=()):
    s = h._out(A.smm_draws_t, arrays, skip)
    gp = None if g is None else g.ctypes.data_as(A.c_int32_p)
    return h._fn("get_draws")(h._ctx, t0, t1, select, gp, ng, thin, K, cap, C.byref(s))


def test_calling_protocol_and_invalid_arguments(S, base):
    h, hist = base
    A = S._abi
    g = base_groups()
    rows = ("params", "value", "sim_moments", "chain", "iter", "src_iter")
    size = dict(count=np.full(5, -7, np.int64), n_chains=np.full(5, -7, np.int32), row0=np.full(6, -7, np.int64))
    assert raw(h, A, T0, T1, 1, g, 5, 2, 40, -5, size) == A.SMM_OK                      # the sizing call ignores rows_cap
    want = DR.draws_from_history(hist, T0, T1, 1, g, 2, 40, n_groups=5)
    DR.assert_draws_equal(size, want, ("count", "n_chains", "row0"))
    R = int(size["row0"][5])
    assert R == int(want["row0"][5]) and R > 40

    def sentinel(n):
        return dict(count=np.full(5, -7, np.int64), n_chains=np.full(5, -7, np.int32), row0=np.full(6, -7, np.int64),
                    params=np.full((n, 3), -7.5), value=np.full(n, -7.5), sim_moments=np.full((n, 3), -7.5),
                    chain=np.full(n, -7, np.int32), iter=np.full(n, -7, np.int32), src_iter=np.full(n, -7, np.int32))

    def untouched(a):
        return all((v == (-7.5 if v.dtype.kind == "f" else -7)).all() for v in a.values())

    a = sentinel(R)
    assert raw(h, A, T0, T1, 1, g, 5, 2, 40, R - 1, a) == A.SMM_ERR_INVALID_ARG         # one row short: refused, nothing written
    msg = h._fn("last_error")(h._ctx).decode()
    assert str(R) in msg and "rows_cap" in msg, msg
    assert untouched(a)
    assert raw(h, A, T0, T1, 1, g, 5, 2, 40, R, a) == A.SMM_OK
    DR.assert_draws_equal(a, want)
    a = sentinel(R + 3)                                                                 # room to spare: the rows behind R stay
    assert raw(h, A, T0, T1, 1, g, 5, 2, 40, R + 3, a, skip=("sim_moments", "iter")) == A.SMM_OK
    assert (a["sim_moments"] == -7.5).all() and (a["iter"] == -7).all() and (a["value"][R:] == -7.5).all() and (a["chain"][R:] == -7).all()
    assert np.array_equal(a["params"][:R].view(np.uint64), want["params"].view(np.uint64)) and np.array_equal(a["src_iter"][:R], want["src_iter"])
    one = sentinel(R)                                                                   # one row array is a row call
    assert raw(h, A, T0, T1, 1, g, 5, 2, 40, R - 1, one, skip=rows[1:]) == A.SMM_ERR_INVALID_ARG and untouched(one)

    bad_id, low_id = g.copy(), g.copy()
    bad_id[3], low_id[5] = 5, -2
    ok = dict(t0=T0, t1=T1, select=1, g=g, ng=5, thin=2, K=40, cap=R)
    bad = [dict(t0=-1), dict(t1=T + 1), dict(t0=9, t1=8), dict(select=3), dict(select=-1), dict(ng=-1), dict(g=None, ng=2), dict(g=None, ng=0),
           dict(g=bad_id), dict(g=low_id), dict(thin=0), dict(thin=-4), dict(K=0), dict(K=(1 << 24) + 1), dict(K=-1), dict(cap=-1)]
    for b in bad:
        k = dict(ok, **b)
        a = sentinel(R)
        assert raw(h, A, k["t0"], k["t1"], k["select"], k["g"], k["ng"], k["thin"], k["K"], k["cap"], a) == A.SMM_ERR_INVALID_ARG, b
        assert len(h._fn("last_error")(h._ctx).decode()) > 0 and untouched(a), b
    fn = h._fn("get_draws")
    keep = sentinel(R)
    s = h._out(A.smm_draws_t, keep)
    gp = g.ctypes.data_as(A.c_int32_p)
    assert fn(None, T0, T1, 1, gp, 5, 2, 40, R, C.byref(s)) == A.SMM_ERR_INVALID_ARG
    assert fn(h._ctx, T0, T1, 1, gp, 5, 2, 40, R, None) == A.SMM_ERR_INVALID_ARG
    assert raw(h, A, T0, T1, 1, g, 5, 2, 1 << 24, 0, size) == A.SMM_OK and size["row0"][5] == size["count"].sum() > R
    assert raw(h, A, T0, T1, 1, g, 5, 2, 1 << 24, R, keep) == A.SMM_ERR_INVALID_ARG and untouched(keep)   # (the largest cap: now R rows are too few)
    for kw in (dict(thin=0), dict(max_rows=0), dict(select=5), dict(t1=T + 1)):
        with pytest.raises(S.SMMHipError):
            h.draws(**dict(dict(t0=0, t1=T), **kw))


@pytest.mark.parametrize("persistent", (True, False))
def test_a_call_between_steps_leaves_the_run_untouched(S, persistent):
    prob, opts = cm.serial_normal(N=256, T=60)
    a, b = S.hip_context(prob, opts), S.hip_context(prob, opts)
    for h in (a, b):
        h.set_persistent(persistent)
        h.step(30)
    hist = b.history(0, 30)
    g = (np.arange(256) % 3).astype(np.int32)
    for select in (0, 1, 2):
        check(b, hist, 5, 30, select, g, 2, 100)
    for h in (a, b):
        h.step(30)
        print(h.describe(), h.persistent_info())
        assert (h.persistent_info()[1] >= 1) == persistent
    cm.assert_history_equal(a.history(), b.history(), exact_floats=True)
    cm.assert_state_equal(a.state(), b.state(), rtol=0)
    check(b, b.history(0, 60), 0, 60, 2, g, 1, 1000)


def test_host_draws_reads_the_device(S, monkeypatch):
    from collections import OrderedDict
    Nh, Th = 64, 80
    m = S.MProb()
    S.addSampledParam(m, OrderedDict([("p1", [0.2, -3, 3]), ("p2", [-0.2, -20, 20])]))
    S.addMoment(m, {"name": ["mu1", "mu2"], "value": [-1.0, 10.0], "weight": [1.0, 1.0]})
    S.addEvalFunc(m, S.objfunc_norm)
    acc = [2.0] * 32 + [1.0] * 16 + [2.0] * 8 + [0.5] * 8
    MA = S.MAlgoBGP(m, {"N": Nh, "maxiter": Th, "maxtemp": 5, "sigma": 0.05, "min_improve": [0.0] * Nh, "acc_tuners": acc})
    S.run(MA)
    ps = [S.params(c) for c in MA.chains]                # the download path
    MA._hist = None

    def no_download(*a, **k):
        raise AssertionError("the history was downloaded")
    monkeypatch.setattr(type(MA._ctx), "history", no_download)
    groups = np.array([0] * 32 + [1] * 16 + [0] * 8 + [2] * 8, np.int32)
    for kw, sel in ((dict(), 1), (dict(state=True, window=(10, 70), thin=3, max_rows=200, moments=True), 2),
                    (dict(accepted_only=False, max_rows=77), 0)):
        tabs = S.draws(MA, **kw)
        w = kw.get("window", (0, Th))
        r = MA._ctx.draws(w[0], w[1], sel, groups, kw.get("thin", 1), kw.get("max_rows", 10000), True)
        assert len(tabs) == 3
        names = ["chain", "iter", "value", "p1", "p2"] + (["mu1", "mu2"] if kw.get("moments") else [])
        for k, tab in enumerate(tabs):
            assert list(tab.keys()) == names
            a, b = int(r["row0"][k]), int(r["row0"][k + 1])
            cols = dict(chain=r["chain"][a:b], iter=r["iter"][a:b], value=r["value"][a:b], p1=r["params"][a:b, 0], p2=r["params"][a:b, 1],
                        mu1=r["sim_moments"][a:b, 0], mu2=r["sim_moments"][a:b, 1])
            for name in names:
                assert np.array_equal(np.asarray(tab[name]), cols[name], equal_nan=True), (k, name)
    for j in (0, 33, 63):
        tab = S.draws(MA.chains[j], max_rows=Th + 1)
        assert (np.asarray(tab["chain"]) == j + 1).all() and len(tab["iter"]) == len(ps[j]["p1"])
        for name in ("p1", "p2"):
            assert np.array_equal(np.asarray(tab[name], float).view(np.uint64), np.ascontiguousarray(ps[j][name]).view(np.uint64)), (j, name)


def test_p2p_shards_report_global_chain_ids(S):
    from test_gpu_p2p import p2p_contexts, p2p_run_lockstep
    prob, opts = cm.serial_normal(N=64, T=30, ns=1000)
    ctxs = p2p_contexts(S, prob, opts, 2)
    p2p_run_lockstep(ctxs, 30)
    g3 = (np.arange(32) % 3).astype(np.int32)
    for r, c in enumerate(ctxs):
        hist = c.history(0, 30)
        got = check(c, hist, 3, 30, 2, g3, 2, 100, chain_offset=32 * r)
        assert ((got["chain"] > 32 * r) & (got["chain"] <= 32 * (r + 1))).all() and len(got["chain"]) == 300
        check(c, hist, 0, 30, 1, None, 1, BIG, chain_offset=32 * r)
