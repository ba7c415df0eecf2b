"""smm_get_group_stats on the device (include/smmhip.h, smm.jl_amd/csrc/smm_group.hpp): every output equal (array_equal, NaN equal to
NaN) to the numerical contract restated in group_stats_ref.py over the history downloaded with smm_get_history — objfunc_norm's
persistent form with explicit, default and NULL groups, the C3 layout (pooled columns far past 8192 draws: the grid-wide select of the
shipped library), dense2 at np = 50 past the scratch cap (batches of parameters and of chunks) and at small size through the test
build's seams, a map-reduce user objective, crafted histories, p2p shards, invalid arguments, a twin context that was never asked, and
host.pooled.  Each batched case asserts the host's plan (plan(): its formulas)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import common as cm
import group_stats_ref as GR

pytestmark = pytest.mark.gpu
PROBS = (0.0, 0.025, 0.3, 0.5, 0.975, 1.0)
STATS_SCRATCH_CAP = 256 << 20    # smm_reducers_host.hpp: REDUCER_BATCH_CAP
LDS_N = 8192                     # smm_stats.hpp: STATS_LDS_N


def plan(N, T, npar, counts, cov, cap=STATS_SCRATCH_CAP, wide_min=LDS_N + 1):
    """the host's plan of a first call on a fresh context (smm_reducers_host.hpp: smm_get_group_stats, reducer_scratch): parameters per batch kb,
    chunks per cov batch Nbc, and which groups take the grid-wide select"""
    counts = np.asarray(counts, np.int64)
    Mtot = int(counts.sum())
    scr = max(min(N * T * (8 * npar + 4), max(cap, 12 * T)), N * T * 8, npar * LDS_N * 8 if cov else 0)
    kb = min(npar, scr // (Mtot * 8)) if Mtot else 0
    NC = int(sum(-(-int(m) // LDS_N) for m in counts))
    Nbc = min(NC, scr // (npar * LDS_N * 8))
    return SimpleNamespace(kb=kb, kbatches=-(-npar // kb) if kb else 0, NC=NC, Nbc=Nbc, cbatches=-(-NC // Nbc) if Nbc else 0,
                           wide=counts >= wide_min)


def check(h, t0, t1, acc, groups=None, probs=PROBS, hist=None, n_groups=None):
    hist = h.history(0, t1) if hist is None else hist
    got = h.group_stats(t0, t1, acc, groups, probs, n_groups=n_groups)
    GR.assert_group_stats_equal(got, GR.group_stats_from_history(hist, t0, t1, acc, groups, probs, n_groups=n_groups))
    return got


def raw_call(h, t0, t1, acc, groups, n_groups, probs, fields):
    """smm_get_group_stats through ctypes with only the given outputs: (rc, the outputs)"""
    from smm_jl_amd import _abi as A
    npar, n_groups_out = h.np, max(n_groups, 1)
    G = n_groups_out
    shapes = dict(count=((G,), np.int64), n_chains=((G,), np.int32), mean=((G, npar), float), median=((G, npar), float),
                  quantile=((max(len(probs), 1), G, npar), float), cov=((G, npar, npar), float))
    r = {f: np.full(shapes[f][0], -7, shapes[f][1]) for f in fields}
    s = A.smm_group_stats_t()
    for f, t in A.smm_group_stats_t._fields_:
        if f in r:
            setattr(s, f, r[f].ctypes.data_as(t))
    p = np.asarray(probs, float)
    g = None if groups is None else np.ascontiguousarray(groups, np.int32)
    rc = h._fn("get_group_stats")(h._ctx, t0, t1, int(acc), None if g is None else g.ctypes.data_as(A.c_int32_p), n_groups,
                                  p.ctypes.data_as(A.c_double_p) if len(p) else None, len(p), C.byref(s))
    return rc, r


def test_objfunc_norm_persistent_windows_and_groups(S):
    N, T = 256, 300
    prob, opts = cm.serial_normal(N=N, T=T)
    h = S.hip_context(prob, opts)
    h.step(T)
    assert h.persistent_info()[1] >= 1
    hist = h.history(0, T)
    g4 = (np.arange(N) % 4).astype(np.int32)
    g4[::7] = -1                                          # chains in no group
    g4[g4 == 2] = 4                                       # group 2 empty, n_groups = 5
    for acc in (True, False):
        for t0, t1 in ((0, T), (50, 120), (120, 120), (299, 300)):
            got = check(h, t0, t1, acc, g4, hist=hist)
            assert got["count"][2] == 0 and np.isnan(got["mean"][2]).all() and got["n_chains"][2] == 0
            if t0 == t1:
                assert (got["count"] == 0).all() and np.isnan(got["cov"]).all()
            check(h, t0, t1, acc, None, hist=hist)        # group NULL, n_groups 1
            check(h, t0, t1, acc, np.zeros(N, np.int32), hist=hist)
        check(h, 0, T, acc, g4, hist=hist, n_groups=7)    # trailing empty groups
        check(h, 0, T, acc, np.full(N, -1, np.int32), hist=hist, n_groups=2)
    ids = {}
    dflt = np.array([ids.setdefault(float(a), len(ids)) for a in opts.acc_tuner], np.int32)   # host.rhat's default groups
    check(h, 0, T, True, dflt, hist=hist)
    rc, r = raw_call(h, 0, T, True, g4, 5, (), ("count",))
    assert rc == 0 and np.array_equal(r["count"], GR.group_stats_from_history(hist, 0, T, True, g4, ())["count"])
    rc, r = raw_call(h, 0, T, False, g4, 5, (0.5,), ("quantile", "cov"))   # the order statistics without the median
    want = GR.group_stats_from_history(hist, 0, T, False, g4, (0.5,))
    assert rc == 0
    GR.assert_group_stats_equal(r, want, ("quantile", "cov"))


def test_invalid_arguments(S):
    N, T = 64, 20
    prob, opts = cm.serial_normal(N=N, T=T, ns=500)
    h = S.hip_context(prob, opts)
    h.step(T)
    g = np.zeros(N, np.int32)
    bad = [dict(t0=0, t1=T + 1), dict(t0=5, t1=4), dict(t0=-1, t1=3), dict(groups=g, n_groups=-1), dict(groups=None, n_groups=2),
           dict(groups=None, n_groups=0), dict(groups=np.where(np.arange(N) == 3, 1, 0), n_groups=1),
           dict(groups=np.where(np.arange(N) == 3, -2, 0), n_groups=1), dict(probs=(0.5, 1.5)), dict(probs=(np.nan,)),
           dict(probs=(-0.1,))]
    for b in bad:
        a = dict(t0=0, t1=T, groups=g, n_groups=1, probs=PROBS)
        a.update(b)
        rc, _ = raw_call(h, a["t0"], a["t1"], True, a["groups"], a["n_groups"], a["probs"], ("count", "mean", "quantile"))
        assert rc == S._abi.SMM_ERR_INVALID_ARG, b
    A = S._abi
    s = A.smm_group_stats_t()
    q = np.empty(64)
    s.quantile = q.ctypes.data_as(A.c_double_p)
    assert h._fn("get_group_stats")(h._ctx, 0, T, 1, None, 1, None, 0, C.byref(s)) == A.SMM_ERR_INVALID_ARG   # quantile without probs
    s = A.smm_group_stats_t()
    assert h._fn("get_group_stats")(h._ctx, 0, T, 1, None, 1, None, 2, C.byref(s)) == A.SMM_ERR_INVALID_ARG   # probs NULL, n_probs 2
    assert h._fn("get_group_stats")(h._ctx, 0, T, 1, None, 1, None, -1, C.byref(s)) == A.SMM_ERR_INVALID_ARG
    assert h._fn("get_group_stats")(h._ctx, 0, T, 1, None, 1, None, 0, None) == A.SMM_ERR_INVALID_ARG
    assert h._fn("get_group_stats")(None, 0, T, 1, None, 1, None, 0, C.byref(s)) == A.SMM_ERR_INVALID_ARG
    with pytest.raises(S.SMMHipError):
        h.group_stats(0, T + 1)
    check(h, 0, T, True, g)                               # the context still answers


def test_c3_layout_takes_the_grid_wide_select(S):
    from smm_jl_amd.workloads import build_problem
    N, T = 4096, 40
    prob, opts = build_problem("c3", N, N, 0, T, 0)
    h = S.hip_context(prob, opts)
    h.step(T)
    hist = h.history(0, T)
    levels = (np.arange(N) // (N // 8)).astype(np.int32)  # 8 levels x 512 replicas
    for acc, (t0, t1) in ((False, (0, T)), (True, (0, T)), (False, (3, 29))):
        got = check(h, t0, t1, acc, levels, hist=hist)
        p = plan(N, T, prob.np, got["count"], True)
        assert p.kbatches == 1
        if not acc:
            assert p.wide.all() and got["count"].min() > 8192
    got = check(h, 0, T, False, None, hist=hist)          # one group of every chain: 163840 draws
    assert got["count"][0] == N * T and plan(N, T, prob.np, got["count"], True).NC == 20


def test_dense2_np50_past_the_scratch_cap(S):
    from smm_jl_amd.workloads import build_problem
    N, T = 4096, 180
    prob, opts = build_problem("c5", N, N, 0, T, 0)
    assert prob.np == 50
    h = S.hip_context(prob, opts)
    h.step(T)
    hist = h.history(0, T)
    got = check(h, 0, T, False, None, probs=(0.05, 0.5, 0.95), hist=hist)
    p = plan(N, T, 50, got["count"], True)
    assert p.kb == 45 and p.kbatches == 2 and p.NC == 90 and p.Nbc == 81 and p.cbatches == 2 and p.wide.all()
    g64 = (np.arange(N) // 64).astype(np.int32)           # groups of 64 chains
    check(h, 0, T, False, g64, probs=(0.05, 0.5, 0.95), hist=hist)
    check(h, 11, 150, True, g64, probs=(0.5,), hist=hist)


def test_dense2_batches_and_the_grid_wide_seam_at_small_size(S, hooks, monkeypatch):
    from smm_jl_amd.workloads import build_problem
    N, T = 32, 60
    prob, opts = build_problem("c5", N, N, 0, T, 0)
    base = S.hip_context(prob, opts)
    base.step(T)
    snap = (base.state(), base.history())
    hist = snap[1]
    g8 = (np.arange(N) // 4).astype(np.int32)
    fields = ("count", "n_chains", "mean", "median", "quantile")
    for wide in (None, 1, 100):
        monkeypatch.setenv("SMMHIP_STATS_SCRATCH", "1")
        if wide is not None:
            monkeypatch.setenv("SMMHIP_GROUP_WIDE_MIN", str(wide))
        h = S.hip_context(prob, opts)
        for var in ("SMMHIP_STATS_SCRATCH", "SMMHIP_GROUP_WIDE_MIN"):
            monkeypatch.delenv(var, raising=False)
        h.set_state(*snap)
        for groups, ng, acc in ((None, 1, False), (g8, 8, True), (g8, 8, False)):
            want = GR.group_stats_from_history(hist, 0, T, acc, groups, PROBS, n_groups=ng)
            if groups is None and not acc:                # the first call: no cov, the scratch of one parameter's pooled columns
                p = plan(N, T, 50, want["count"], False, cap=1, wide_min=wide or LDS_N + 1)
                assert p.kb == 1 and p.kbatches == 50
                assert p.wide.all() == (wide is not None and wide <= N * T)
            rc, r = raw_call(h, 0, T, acc, groups, ng, PROBS, fields)
            assert rc == 0
            GR.assert_group_stats_equal(r, want, fields)
        got = check(h, 0, T, True, g8, hist=hist)         # with cov: the scratch grows to one chunk of every parameter
        p = plan(N, T, 50, got["count"], True, cap=1)
        assert p.Nbc == 1 and p.cbatches == 8
        check(h, 7, 41, False, g8, hist=hist)
        cm.assert_history_equal(h.history(), hist, exact_floats=True)


def test_map_reduce_user_objective(S):
    from user_objective_src import PANEL_SOURCE
    from test_user_objective import panel_problem
    prob, opts = panel_problem(S, S.register_user_objective(PANEL_SOURCE, n_sums=3, lanes=64), N=32, T=40)
    h = S.hip_context(prob, opts)
    h.step(40)
    g = (np.arange(32) % 3).astype(np.int32)
    for acc in (True, False):
        check(h, 0, 40, acc, g)
        check(h, 5, 33, acc, None)


def test_crafted_histories(S, hooks, monkeypatch):
    N, T = 16, 40
    prob, opts = cm.serial_normal(N=N, T=T, ns=100)
    h0 = S.hip_context(prob, opts)
    h0.step(2)
    st = h0.state()
    hb = h0.history(0, 2)
    rng = np.random.default_rng(11)
    from smm_jl_amd import _abi as A
    c = A.HistoryBuffers(T, N, prob.np, prob.nm)
    for f in A.HistoryBuffers.FIELDS:
        getattr(c, f)[...] = getattr(hb, f)[rng.integers(0, 2, T)]
    pool = np.array([-0.0, 0.0, 1.0, 1.0, -np.inf, np.inf, 2.0, -3.0])
    c.params[...] = rng.choice(pool, c.params.shape)
    c.params[:, :, 3] = rng.standard_normal((T, prob.np))
    c.params[5, 0, 4] = np.nan                            # group 1 (chains 4..7): a NaN among its first parameter's draws
    c.params[:, :, 8:12] = 2.5                            # group 2: all equal
    c.params[:, 1, 12:16] = -0.0                          # group 3: a column of -0 only ...
    c.params[::5, 1, 13] = 0.0                            # ... and some +0
    c.accepted[...] = rng.random(c.accepted.shape) < 0.6
    c.accepted[5, 4] = 1
    c.accepted[:, 2] = 0                                  # chain 2: no selected draw
    st.iter = T
    groups = (np.arange(N) // 4).astype(np.int32)
    for wide in (None, 1):
        if wide is not None:
            monkeypatch.setenv("SMMHIP_GROUP_WIDE_MIN", str(wide))
        h = S.hip_context(prob, opts)
        monkeypatch.delenv("SMMHIP_GROUP_WIDE_MIN", raising=False)
        h.set_state(st, c)
        back = h.history(0, T)
        for acc in (True, False):
            for t0, t1 in ((0, T), (4, 23)):
                got = check(h, t0, t1, acc, groups, probs=(0.0, 0.3, 0.5, 1.0), hist=back)
        assert np.isnan(got["mean"][1, 0]) and np.isnan(got["median"][1, 0]) and np.isnan(got["cov"][1, 0]).all()
        assert (got["median"][2] == 2.5).all() and (got["cov"][2] == 0.0).all()


def test_p2p_shards_report_their_own_groups(S):
    from test_gpu_p2p import p2p_contexts, p2p_run_lockstep
    prob, opts = cm.serial_normal(N=64, T=30, ns=1000)
    ctxs = p2p_contexts(S, prob, opts, 2)
    p2p_run_lockstep(ctxs, 30)
    g = (np.arange(32) % 3).astype(np.int32)
    g[5] = -1
    for c in ctxs:
        hist = c.history(0, 30)
        for acc in (True, False):
            check(c, 0, 30, acc, g, hist=hist)
            check(c, 4, 30, acc, None, hist=hist)


def test_group_stats_between_steps_leave_the_run_untouched(S):
    prob, opts = cm.serial_normal(N=128, T=120, ns=1000)
    a = S.hip_context(prob, opts)
    b = S.hip_context(prob, opts)
    a.step(120)
    g = (np.arange(128) % 5).astype(np.int32)
    b.step_async(40)
    b.group_stats(0, 40, True, g, PROBS)                  # right after an enqueued persistent step
    b.step(1)
    b.group_stats(10, 41, False)
    b.step_async(50)
    b.group_stats(0, 91, False, g, (0.5,))
    b.step(29)
    cm.assert_history_equal(a.history(), b.history(), exact_floats=True)
    cm.assert_state_equal(a.state(), b.state(), rtol=0)


def test_host_pooled_reads_the_device(S):
    from collections import OrderedDict
    N, T = 64, 80
    m = S.MProb()
    S.addSampledParam(m, OrderedDict([("p1", [0.2, -3, 3]), ("p2", [-0.2, -20, 20])]))
    S.addMoment(m, {"name": ["mu1", "mu2"], "value": [-1.0, 10.0], "weight": [1.0, 1.0]})
    S.addEvalFunc(m, S.objfunc_norm)
    acc = [2.0] * 32 + [1.0] * 16 + [2.0] * 8 + [0.5] * 8
    MA = S.MAlgoBGP(m, {"N": N, "maxiter": T, "maxtemp": 5, "sigma": 0.05, "min_improve": [0.0] * N, "acc_tuners": acc})
    S.run(MA)
    h = MA._ctx.history(0, T)
    groups = np.array([0] * 32 + [1] * 16 + [0] * 8 + [2] * 8, np.int32)
    names = S.ps2s_names(m)
    for window, level in ((None, 0.95), ((10, 70), 0.9)):
        t0, t1 = (0, T) if window is None else window
        q = ((1 - level) / 2, 1 - (1 - level) / 2)
        want = GR.group_stats_from_history(h, t0, t1, True, groups, q)
        got = S.pooled(MA, window=window, level=level)
        assert len(got) == 3
        for g, r in enumerate(got):
            assert r["count"] == want["count"][g] and r["chains"] == want["n_chains"][g]
            assert list(r["mean"]) == names
            assert np.array_equal([r["mean"][k] for k in names], want["mean"][g])
            assert np.array_equal([r["median"][k] for k in names], want["median"][g])
            assert np.array_equal(np.array([r["CI"][k] for k in names]).T, want["quantile"][:, g])
            assert np.array_equal(r["cov"], want["cov"][g])
    one = S.pooled(MA, groups=np.zeros(N, np.int32))[0]
    x = np.concatenate([h.params[h.accepted[:, c] != 0, :, c] for c in range(N)])
    assert one["count"] == len(x) and [one["mean"][k] for k in names] == [np.mean(np.ascontiguousarray(x[:, i])) for i in range(2)]
