"""smm_get_histogram on the device (include/smmhip.h, smm.jl_amd/csrc/smm_hist.hpp): every output equal (array_equal, NaN equal to NaN)
to the contract restated in hist_ref.py over the history downloaded with smm_get_history — objfunc_norm's persistent form with the
three selections, two windows, explicit / NULL / per-chain groups, autodetected and given ranges and pairs; the C3 layout (pooled
groups of many workgroups through the global atomics); dense2 at np = 50 (parameter batches, bins past LDS, batches of groups); the
test build's seams at small size; a map-reduce user objective; crafted histories; p2p shards; invalid arguments and subsets of
outputs; a twin context that was never asked; and host.histogram / histogram2d against numpy on params(c), without a download.
The crafted histories here draw from a small pool over ranges whose edges are exact in binary; draws that ride the edges of awkward
ranges (numpy's index corrections by one, the LDS limits, the degenerate tables) are in tests/test_gpu_hist_edges.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import common as cm
import hist_ref as HR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check(h, t0, t1, select, groups=None, bins=10, rng=None, pairs=(), bins2=None, hist=None, n_groups=None):
    hist = h.history(0, t1) if hist is None else hist
    got = h.histogram(t0, t1, select, groups, bins, rng, pairs, bins2, n_groups=n_groups)
    want = HR.histogram_from_history(hist, t0, t1, select, groups, bins, rng, pairs, bins2, n_groups=n_groups)
    HR.assert_histogram_equal(got, want, auto=rng is None)
    return got


def raw_call(h, t0, t1, select, groups, n_groups, bins, rng, pairs, bins2, fields):
    """smm_get_histogram through ctypes with only the given outputs: (rc, the outputs)"""
    from smm_jl_amd import _abi as A
    npar, G = h.np, max(n_groups, 1)
    pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    B2 = max(bins2, 1)
    shapes = dict(count=((G,), np.int64), status=((G, npar), np.int32), lo=((G, npar), float), hi=((G, npar), float),
                  edges=((G, npar, max(bins, 0) + 1), float), hist=((G, npar, max(bins, 1)), np.int64),
                  edges2=((G, npar, B2 + 1), float), hist2=((G, max(len(pr), 1), B2, B2), np.int64))
    r = {f: np.full(shapes[f][0], -7, shapes[f][1]) for f in fields}
    s = A.smm_histogram_t()
    for f, t in A.smm_histogram_t._fields_:
        if f in r:
            setattr(s, f, r[f].ctypes.data_as(t))
    g = None if groups is None else np.ascontiguousarray(groups, np.int32)
    rg = None if rng is None else np.ascontiguousarray(rng, float)
    rc = h._fn("get_histogram")(h._ctx, t0, t1, select, None if g is None else g.ctypes.data_as(A.c_int32_p), n_groups, bins,
                                None if rg is None else rg.ctypes.data_as(A.c_double_p), pr.ctypes.data_as(A.c_int32_p) if len(pr) else None,
                                len(pr), bins2, C.byref(s))
    return rc, r


def test_objfunc_norm_persistent_selections_windows_groups(S):
    N, T = 256, 300
    prob, opts = cm.serial_normal(N=N, T=T)
    h = S.hip_context(prob, opts)
    h.step(T)
    assert h.persistent_info()[1] >= 1
    hist = h.history(0, T)
    g4 = (np.arange(N) % 4).astype(np.int32)
    g4[::7] = -1
    g4[g4 == 2] = 4                                       # group 2 empty, n_groups = 5
    per_chain = np.arange(N, dtype=np.int32)
    rng = np.array([[-2.0, 1.0], [9.0, 11.0]])
    for sel in ("all", "accepted", "state"):
        for t0, t1 in ((0, T), (50, 120)):
            got = check(h, t0, t1, sel, g4, bins=13, pairs=[(0, 1), (1, 0), (1, 1)], bins2=7, hist=hist)
            assert got["count"][2] == 0 and (got["hist"][2] == 0).all()
            check(h, t0, t1, sel, None, bins=10, hist=hist)
            check(h, t0, t1, sel, per_chain, bins=5, pairs=[(0, 1)], hist=hist)
            check(h, t0, t1, sel, g4, bins=20, rng=rng, pairs=[(0, 1)], bins2=9, hist=hist)
    check(h, 120, 120, "accepted", g4, hist=hist)         # an empty window: (0, 1) everywhere
    check(h, 0, T, "all", g4, bins=1, pairs=[(0, 0)], bins2=1, hist=hist, n_groups=7)


def test_c3_layout_pools_through_global_atomics(S):
    from smm_jl_amd.workloads import build_problem
    N, T = 4096, 40
    prob, opts = build_problem("c3", N, N, 0, T, 0)
    h = S.hip_context(prob, opts)
    h.step(T)
    hist = h.history(0, T)
    levels = (np.arange(N) // (N // 8)).astype(np.int32)
    pairs = [(0, 1), (1, 2), (2, 0)] if prob.np >= 3 else [(0, 1)]
    for sel in ("all", "accepted", "state"):
        check(h, 0, T, sel, levels, bins=50, pairs=pairs, bins2=16, hist=hist)
    check(h, 3, 29, "all", None, bins=200, pairs=pairs, bins2=200, hist=hist)   # bins2 = 200: cells past LDS


def test_dense2_np50_parameter_batches_and_large_bins(S):
    from smm_jl_amd.workloads import build_problem
    N, T = 512, 60
    prob, opts = build_problem("c5", N, N, 0, T, 0)
    assert prob.np == 50
    h = S.hip_context(prob, opts)
    h.step(T)
    hist = h.history(0, T)
    g16 = (np.arange(N) // 32).astype(np.int32)
    pairs = [(j, (j * 7) % 50) for j in range(50)] + [(3, 3)] * 30   # 80 pairs: two batches
    check(h, 0, T, "all", g16, bins=10, pairs=pairs, bins2=10, hist=hist)   # kb = 50 of 64
    check(h, 0, T, "accepted", g16, bins=1000, hist=hist)                   # kb = 5: ten parameter batches
    check(h, 5, T, "state", g16, bins=7000, hist=hist)                      # past LDS: global counters
    check(h, 0, T, "all", (np.arange(N) // 256).astype(np.int32), bins=65536, hist=hist)   # the largest bins, global counters


def test_seams_at_small_size(S, hooks, monkeypatch):
    from smm_jl_amd.workloads import build_problem
    N, T = 32, 60
    prob, opts = build_problem("c5", N, N, 0, T, 0)
    base = S.hip_context(prob, opts)
    base.step(T)
    snap = (base.state(), base.history())
    hist = snap[1]
    g8 = (np.arange(N) // 4).astype(np.int32)
    for lds_bins, scratch in ((None, "1"), ("1", None), ("4", "20000")):
        for var, v in (("SMMHIP_HIST_LDS_BINS", lds_bins), ("SMMHIP_STATS_SCRATCH", scratch)):
            if v is not None:
                monkeypatch.setenv(var, v)
        h = S.hip_context(prob, opts)
        for var in ("SMMHIP_HIST_LDS_BINS", "SMMHIP_STATS_SCRATCH"):
            monkeypatch.delenv(var, raising=False)
        h.set_state(*snap)
        for groups in (None, g8, np.arange(N, dtype=np.int32)):
            for sel in ("all", "accepted", "state"):
                check(h, 0, T, sel, groups, bins=6, pairs=[(0, 1), (49, 2), (7, 7)], bins2=5, hist=hist)
        check(h, 9, 41, "accepted", g8, bins=3, rng=np.tile([-0.5, 0.5], (50, 1)), pairs=[(1, 0)], bins2=3, hist=hist)
        cm.assert_history_equal(h.history(), hist, exact_floats=True)


def test_map_reduce_user_objective(S):
    from user_objective_src import PANEL_SOURCE
    from test_user_objective import panel_problem
    prob, opts = panel_problem(S, S.register_user_objective(PANEL_SOURCE, n_sums=3, lanes=64), N=32, T=40)
    h = S.hip_context(prob, opts)
    h.step(40)
    g = (np.arange(32) % 3).astype(np.int32)
    for sel in ("all", "accepted", "state"):
        check(h, 0, 40, sel, g, bins=8, pairs=[(0, 1)], bins2=4)
        check(h, 5, 33, sel, None, bins=8)


def test_crafted_histories(S):
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
    c.params[5, 0, 4] = np.nan                            # group 1: a NaN among its first parameter's draws
    c.params[:, :, 8:12] = 2.5                            # group 2: all equal
    c.params[:, 1, 12:16] = -0.0                          # group 3: a column of -0 only ...
    c.params[::5, 1, 13] = 0.0                            # ... and some +0
    c.params[:, 0, 12:16] = 1e16 + rng.integers(0, 5, (T, 4))   # ... and a narrow range at a large magnitude
    c.accepted[...] = rng.random(c.accepted.shape) < 0.6
    c.accepted[5, 4] = 1
    c.accepted[:, 2] = 0                                  # chain 2: no selected row (and no state)
    st.iter = T
    got = None
    groups = (np.arange(N) // 4).astype(np.int32)
    h = S.hip_context(prob, opts)
    h.set_state(st, c)
    back = h.history(0, T)
    for sel in ("all", "accepted", "state"):
        for t0, t1 in ((0, T), (4, 23)):
            r = check(h, t0, t1, sel, groups, bins=64, pairs=[(0, 1), (1, 0), (0, 0)], bins2=64, hist=back)
            got = r if (sel, t0) == ("accepted", 0) else got
            check(h, t0, t1, sel, np.arange(N, dtype=np.int32), bins=4, pairs=[(0, 1)], bins2=3, hist=back)
            check(h, t0, t1, sel, groups, bins=5, rng=np.array([[-1.0, 2.5], [-0.0, 0.0]]), pairs=[(0, 1)], bins2=4, hist=back)
    assert got["status"][1, 0] == 1 and got["status"][3, 0] == 3 and got["hist2"][3, 2].sum() > 0
    assert (got["lo"][2] == 2.0).all() and (got["hi"][2] == 3.0).all()


def test_p2p_shards_report_their_own_chains(S):
    from test_gpu_p2p import p2p_contexts, p2p_run_lockstep
    prob, opts = cm.serial_normal(N=64, T=30, ns=1000)
    ctxs = p2p_contexts(S, prob, opts, 2)
    p2p_run_lockstep(ctxs, 30)
    rng = np.array([[-3.0, 3.0], [-20.0, 20.0]])
    tot, hs = None, []
    for c in ctxs:
        hist = c.history(0, 30)
        hs.append(hist)
        check(c, 0, 30, "accepted", (np.arange(32) % 3).astype(np.int32), bins=9, pairs=[(0, 1)], hist=hist)
        r = check(c, 0, 30, "state", None, bins=9, rng=rng, pairs=[(0, 1)], hist=hist)
        tot = r if tot is None else {k: tot[k] + r[k] for k in ("count", "hist", "hist2")}
    x = np.concatenate([h.params[:, :, :] for h in hs], axis=2)
    a = np.concatenate([h.accepted for h in hs], axis=1)
    from types import SimpleNamespace
    both = SimpleNamespace(params=x, accepted=a, value=np.concatenate([h.value for h in hs], axis=1),
                           exchanged=np.concatenate([h.exchanged for h in hs], axis=1))
    want = HR.histogram_from_history(both, 0, 30, "state", None, 9, rng, [(0, 1)])
    HR.assert_histogram_equal(tot, want, fields=("count", "hist", "hist2"))


def test_invalid_arguments_and_output_subsets(S):
    N, T = 64, 20
    prob, opts = cm.serial_normal(N=N, T=T, ns=500)
    h = S.hip_context(prob, opts)
    h.step(T)
    A = S._abi
    g = np.zeros(N, np.int32)
    base = dict(t0=0, t1=T, select=1, groups=g, n_groups=1, bins=10, rng=None, pairs=[(0, 1)], bins2=4)
    bad = [dict(t1=T + 1), dict(t0=5, t1=4), dict(t0=-1), dict(select=3), dict(select=-1), dict(n_groups=-1), dict(groups=None, n_groups=2),
           dict(groups=np.where(np.arange(N) == 3, 1, 0)), dict(groups=np.where(np.arange(N) == 3, -2, 0)), dict(bins=0),
           dict(bins=65537), dict(rng=[[1.0, 0.0], [0.0, 1.0]]), dict(rng=[[0.0, np.inf], [0.0, 1.0]]), dict(rng=[[np.nan, 1.0], [0.0, 1.0]]),
           dict(pairs=[(0, 2)]), dict(pairs=[(-1, 0)]), dict(pairs=[(0, 1)] * 5), dict(bins2=0), dict(bins2=513)]
    for b in bad:
        a = dict(base)
        a.update(b)
        rc, _ = raw_call(h, a["t0"], a["t1"], a["select"], a["groups"], a["n_groups"], a["bins"], a["rng"], a["pairs"], a["bins2"],
                         ("count", "hist", "hist2"))
        assert rc == A.SMM_ERR_INVALID_ARG, b
    rc, _ = raw_call(h, 0, T, 1, g, 1, 10, None, [], 4, ("hist2",))   # hist2 without pairs
    assert rc == A.SMM_ERR_INVALID_ARG
    rc, _ = raw_call(h, 0, T, 1, g, 1, 10, None, [], 4, ("edges2",))
    assert rc == A.SMM_ERR_INVALID_ARG
    s = A.smm_histogram_t()
    assert h._fn("get_histogram")(h._ctx, 0, T, 1, None, 1, 10, None, None, 1, 4, C.byref(s)) == A.SMM_ERR_INVALID_ARG   # pairs NULL
    assert h._fn("get_histogram")(h._ctx, 0, T, 1, None, 1, 10, None, None, 0, 0, None) == A.SMM_ERR_INVALID_ARG
    assert h._fn("get_histogram")(None, 0, T, 1, None, 1, 10, None, None, 0, 0, C.byref(s)) == A.SMM_ERR_INVALID_ARG
    with pytest.raises(S.SMMHipError):
        h.histogram(0, T + 1)
    hist = h.history(0, T)
    want = HR.histogram_from_history(hist, 0, T, 1, g, 10, None, [(0, 1)], 4)
    for fields in (("count",), ("hist",), ("lo", "hi", "status"), ("edges2",), ("hist2",), ("count", "edges", "hist2")):
        rc, r = raw_call(h, 0, T, 1, g, 1, 10, None, [(0, 1)], 4, fields)
        assert rc == 0
        HR.assert_histogram_equal(r, want, fields=fields)
    check(h, 0, T, "accepted", g, pairs=[(0, 1)], hist=hist)   # the context still answers


def test_histograms_between_steps_leave_the_run_untouched(S):
    prob, opts = cm.serial_normal(N=128, T=120, ns=1000)
    a = S.hip_context(prob, opts)
    b = S.hip_context(prob, opts)
    a.step(120)
    g = (np.arange(128) % 5).astype(np.int32)
    b.step_async(40)
    b.histogram(0, 40, "state", g, 12, None, [(0, 1)])    # right after an enqueued persistent step
    b.step(1)
    b.histogram(10, 41, "all")
    b.step_async(50)
    b.histogram(0, 91, "accepted", np.arange(128, dtype=np.int32), 7000)
    b.step(29)
    cm.assert_history_equal(a.history(), b.history(), exact_floats=True)
    cm.assert_state_equal(a.state(), b.state(), rtol=0)


def test_host_histogram_reads_the_device_and_matches_numpy(S, monkeypatch):
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
    ps = [S.params(c) for c in MA.chains[:3]] + [S.params(MA.chains[5], accepted_only=False)]
    MA._hist = None

    def no_download(*a, **k):
        raise AssertionError("the history was downloaded")
    monkeypatch.setattr(type(MA._ctx), "history", no_download)
    for c, p in zip(list(MA.chains[:3]), ps):
        for bins, rng, dens in ((10, None, False), (7, {"p1": (-1.0, 1.0), "p2": (9.0, 10.5)}, True), (1, None, True)):
            got = S.histogram(c, bins=bins, range=rng, density=dens)
            assert list(got) == ["p1", "p2"]
            for k in got:
                n, e = np.histogram(p[k], bins, None if rng is None else rng[k], density=dens)
                assert np.array_equal(got[k][0], n) and got[k][0].dtype == n.dtype and np.array_equal(got[k][1], e)
        for dens in (False, True):
            H, xe, ye = S.histogram2d(c, ("p1", "p2"), bins=6, density=dens)
            wH, wx, wy = np.histogram2d(p["p1"], p["p2"], 6, density=dens)
            assert np.array_equal(H, wH) and np.array_equal(xe, wx) and np.array_equal(ye, wy)
        H, xe, ye = S.histogram2d(c, ("p2", "p1"), bins=4, range=[(9.0, 11.0), (-2.0, 0.0)])
        wH, wx, wy = np.histogram2d(p["p2"], p["p1"], 4, [(9.0, 11.0), (-2.0, 0.0)])
        assert np.array_equal(H, wH) and np.array_equal(xe, wx) and np.array_equal(ye, wy)
    got = S.histogram(MA.chains[5], bins=9, accepted_only=False)
    assert all(np.array_equal(got[k][0], np.histogram(ps[3][k], 9)[0]) for k in got)
    groups = np.array([0] * 32 + [1] * 16 + [0] * 8 + [2] * 8, np.int32)
    per_group = S.histogram(MA, bins=8, window=(10, 70))
    want = HR.histogram_from_history(h, 10, 70, "accepted", groups, 8)
    assert len(per_group) == 3
    for g, d in enumerate(per_group):
        for i, k in enumerate(d):
            assert np.array_equal(d[k][0], want["hist"][g, i]) and np.array_equal(d[k][1], want["edges"][g, i])
    want = HR.histogram_from_history(h, 0, T, "state", np.zeros(N, np.int32), 8)
    if (want["status"] == 0).all():
        st = S.histogram(MA, bins=8, state=True, groups=np.zeros(N, np.int32))
        assert len(st) == 1 and all(np.array_equal(st[0][k][0], want["hist"][0, i]) for i, k in enumerate(st[0]))
    else:                                                 # a row before some chain's first acceptance: numpy raises on NaN
        with pytest.raises(ValueError):
            S.histogram(MA, bins=8, state=True, groups=np.zeros(N, np.int32))
    for bad in (dict(range={"p1": (1.0, 0.0), "p2": (0.0, 1.0)}), dict(range={"p1": (0.0, np.inf), "p2": (0.0, 1.0)}), dict(bins=0)):
        with pytest.raises(ValueError):
            S.histogram(MA.chains[0], **bad)
        with pytest.raises(ValueError):
            np.histogram([0.5], bad.get("bins", 3), bad.get("range", {}).get("p1"))


def test_host_histogram_raises_where_numpy_raises(S):
    N, T = 16, 30
    prob, opts = cm.serial_normal(N=N, T=T, ns=100)
    h0 = S.hip_context(prob, opts)
    h0.step(2)
    st, hb = h0.state(), h0.history(0, 2)
    from smm_jl_amd import _abi as A
    c = A.HistoryBuffers(T, N, prob.np, prob.nm)
    for f in A.HistoryBuffers.FIELDS:
        getattr(c, f)[...] = getattr(hb, f)[np.arange(T) % 2]
    c.accepted[...] = 1
    c.params[3, 0, 1] = np.inf
    c.params[:, 1, 2] = 1e16 + np.arange(T) % 3
    st.iter = T
    h = S.hip_context(prob, opts)
    h.set_state(st, c)
    r = h.histogram(0, T, "all", np.arange(N, dtype=np.int32), 64)
    assert r["status"][1, 0] == 1 and r["status"][2, 1] == 3 and r["status"][0, 0] == 0
    for x, want in ((c.params[:, 0, 1], 1), (c.params[:, 1, 2], 3)):
        with pytest.raises(ValueError):
            np.histogram(x, 64)
    from smm_jl_amd.host import _hist_raise
    with pytest.raises(ValueError, match="autodetected range"):
        _hist_raise(1, np.nan, np.nan, 64)
    with pytest.raises(ValueError, match="Too many bins"):
        _hist_raise(3, 0.0, 1.0, 64)
    _hist_raise(3, 0.0, 1.0, 64, one_d=False)


def test_julia_ccall_matches_the_abi():
    from smm_jl_amd import _abi as A
    src = open(os.path.join(ROOT, "julia", "SMMHip.jl")).read()
    m = re.search(r"ccall\(sym\(:smm_get_histogram\), Cint,\s*\(([^()]*(?:\{[^()]*\}[^()]*)*)\)", src)
    assert m
    jl = [t.strip() for t in m.group(1).split(",") if t.strip()]
    spell = {C.c_void_p: "Ptr{Cvoid}", C.c_int32: "Cint", A.c_int32_p: "Ptr{Int32}", A.c_double_p: "Ptr{Cdouble}",
             C.POINTER(A.smm_histogram_t): "Ref{SmmHistogram}"}
    argtypes = dict((n, a) for n, _, a in A.SYMBOLS)["smm_get_histogram"]
    assert jl == [spell[t] for t in argtypes]
    fields = re.search(r"struct SmmHistogram\n(.*?)\nend", src, re.S).group(1).split()
    assert [f.split("::")[0] for f in fields] == [f for f, _ in A.smm_histogram_t._fields_]
