"""smm_get_trace on the device (include/smmhip.h, smm.jl_amd/csrc/smm_trace.hpp): every output equal (array_equal, NaN equal to NaN) to
the contract restated in trace_ref.py over the history downloaded with smm_get_history — objfunc_norm's persistent form with the three
selections, windows, strides, explicit / NULL / per-chain groups, with and without the simulated moments; the C3 layout (columns past
LDS: a mean chunk with a remainder and the radix select); dense2 at np = 50 (series batches); the test build's seams at small size; a
map-reduce user objective; crafted histories; p2p shards; invalid arguments and subsets of outputs; a twin context that was never
asked; host.trace against numpy on params(c, accepted_only=False) / history(c), without a download; and the Julia ccall."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import common as cm
import trace_ref as TR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBS = (0.0, 0.025, 0.5, 1.0)


def check(h, t0, t1, stride, select, moments=False, groups=None, probs=PROBS, hist=None, n_groups=None, chain_offset=0):
    hist = h.history(0, t1) if hist is None else hist
    got = h.trace(t0, t1, stride, select, moments, groups, probs, n_groups=n_groups)
    want = TR.trace_from_history(hist, t0, t1, stride, select, moments, groups, probs, n_groups=n_groups, chain_offset=chain_offset)
    TR.assert_trace_equal(got, want)
    return got


def raw_call(h, t0, t1, stride, select, moments, groups, n_groups, probs, fields):
    """smm_get_trace through ctypes with only the given outputs, sentinel-filled: (rc, the outputs)"""
    from smm_jl_amd import _abi as A
    G, nt = max(n_groups, 1), TR.n_rows(t0, t1, max(stride, 1))
    S, nq = h.np + 1 + (h.nm if moments else 0), len(probs)
    shapes = dict(iter=((nt,), np.int32), n_chains=((G,), np.int32), count=((nt, G), np.int32), n_accepted=((nt, G), np.int32),
                  n_exchanged=((nt, G), np.int32), n_failed=((nt, G), np.int32), mean=((nt, G, S), float), var=((nt, G, S), float),
                  median=((nt, G, S), float), quantile=((max(nq, 1), nt, G, S), float), best_value=((nt, G), float),
                  best_chain=((nt, G), np.int32))
    r = {f: np.full(shapes[f][0], -7, shapes[f][1]) for f in fields}
    s = A.smm_trace_t()
    for f, t in A.smm_trace_t._fields_:
        if f in r:
            setattr(s, f, r[f].ctypes.data_as(t))
    g = None if groups is None else np.ascontiguousarray(groups, np.int32)
    p = np.ascontiguousarray(probs, float)
    rc = h._fn("get_trace")(h._ctx, t0, t1, stride, select, int(moments), None if g is None else g.ctypes.data_as(A.c_int32_p), n_groups,
                            p.ctypes.data_as(A.c_double_p) if nq else None, nq, C.byref(s))
    return rc, r


def test_objfunc_norm_persistent_selections_windows_strides_groups(S):
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
    for sel in ("all", "accepted", "state"):
        for t0, t1 in ((0, T), (50, 120)):
            got = check(h, t0, t1, 1, sel, True, g4, hist=hist)
            assert (got["count"][:, 2] == 0).all() and np.isnan(got["mean"][:, 2]).all() and (got["best_chain"][:, 2] == 0).all()
            check(h, t0, t1, 7, sel, False, g4, hist=hist)
            check(h, t0, t1, 7, sel, False, None, hist=hist)
            check(h, t0, t1, 1, sel, True, None, hist=hist)
            check(h, t0, t1, 7, sel, True, per_chain, hist=hist)
            one = check(h, t0, t1, 1000, sel, False, g4, hist=hist)   # a stride past the window: its first row only
            assert one["iter"].tolist() == [t0]
        check(h, 50, 120, 1, sel, False, per_chain, hist=hist)
        empty = check(h, 120, 120, 1, sel, True, g4, hist=hist)       # an empty window: no row, the groups' sizes
        assert empty["mean"].shape == (0, 5, 5) and empty["n_chains"].tolist() == np.bincount(g4[g4 >= 0], minlength=5).tolist() == [54, 55, 0, 55, 55]
    check(h, 0, T, 13, "state", False, g4, probs=(), hist=hist, n_groups=7)


def test_c3_columns_past_lds(S):
    from smm_jl_amd.workloads import build_problem
    N, T = 16384, 12
    prob, opts = build_problem("c3", N, N, 0, T, 0)
    h = S.hip_context(prob, opts)
    h.step(T)
    hist = h.history(0, T)
    two = (np.arange(N) >= 12000).astype(np.int32)        # 12000 members: a mean chunk with a remainder, the radix select; and 4384
    for sel in ("all", "accepted", "state"):
        got = check(h, 0, T, 5, sel, False, two, hist=hist)
        assert got["n_chains"].tolist() == [12000, 4384] and got["iter"].tolist() == [0, 5, 10]
    assert (got["count"] == [12000, 4384]).all()


def test_dense2_np50_series_batches(S):
    from smm_jl_amd.workloads import build_problem
    N, T = 512, 60
    prob, opts = build_problem("c5", N, N, 0, T, 0)
    assert prob.np == 50
    h = S.hip_context(prob, opts)
    h.step(T)
    hist = h.history(0, T)
    g16 = (np.arange(N) // 32).astype(np.int32)
    for sel in ("all", "accepted", "state"):
        got = check(h, 0, T, 1, sel, True, g16, hist=hist)            # S = 51 + nm: two gather workgroups per (iteration, group)
        assert got["mean"].shape == (T, 16, 51 + prob.nm)
        check(h, 7, 55, 3, sel, False, g16, hist=hist)


def test_seams_at_small_size(S, hooks, monkeypatch):
    from smm_jl_amd.workloads import build_problem
    N, T = 32, 60
    prob, opts = build_problem("c5", N, N, 0, T, 0)
    base = S.hip_context(prob, opts)
    base.step(T)
    snap = (base.state(), base.history())
    hist = snap[1]
    g8 = (np.arange(N) // 4).astype(np.int32)
    g8[5] = -1
    cases = [(0, T, 1, sel, True, g) for sel in ("all", "accepted", "state") for g in (None, g8)]
    cases += [(9, 41, 4, "state", False, np.arange(N, dtype=np.int32)), (9, 41, 1, "accepted", True, np.arange(N, dtype=np.int32))]
    want = [base.trace(t0, t1, st, sel, mo, g, PROBS) for t0, t1, st, sel, mo, g in cases]
    for (t0, t1, st, sel, mo, g), w in zip(cases, want):
        TR.assert_trace_equal(w, TR.trace_from_history(hist, t0, t1, st, sel, mo, g, PROBS))
    for scratch in ("1", "20000"):                        # one kept iteration and one series per batch; a few series per batch
        monkeypatch.setenv("SMMHIP_STATS_SCRATCH", scratch)
        h = S.hip_context(prob, opts)
        monkeypatch.delenv("SMMHIP_STATS_SCRATCH", raising=False)
        h.set_state(*snap)
        for (t0, t1, st, sel, mo, g), w in zip(cases, want):
            TR.assert_trace_equal(h.trace(t0, t1, st, sel, mo, g, PROBS), w)
        cm.assert_history_equal(h.history(), hist, exact_floats=True)


def test_map_reduce_user_objective(S):
    from user_objective_src import PANEL_SOURCE
    from test_user_objective import panel_problem
    prob, opts = panel_problem(S, S.register_user_objective(PANEL_SOURCE, n_sums=3, lanes=64), N=32, T=40)
    h = S.hip_context(prob, opts)
    h.step(40)
    g = (np.arange(32) % 3).astype(np.int32)
    for sel in ("all", "accepted", "state"):
        check(h, 0, 40, 1, sel, True, g)
        check(h, 5, 33, 4, sel, False, None)


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
    c.params[5, 0, 4] = np.nan                            # group 1: a NaN parameter at iteration 5
    c.params[:, :, 8:12] = 2.5                            # group 2: all equal
    c.sim_moments[...] = rng.choice(pool, c.sim_moments.shape)
    c.sim_moments[:, 0, 12:16] = 1e16 + rng.integers(0, 5, (T, 4))
    c.value[...] = rng.integers(0, 3, c.value.shape)      # tied minimum values
    c.value[7, 9] = np.nan                                # a NaN value: the best of its row, and a NaN in the value series
    c.value[9, [1, 2]] = np.nan                           # two of them: the first
    c.accepted[...] = rng.random(c.accepted.shape) < 0.6
    c.accepted[5, 4] = 1
    c.accepted[7, 9] = 1
    c.accepted[:, 2] = 0                                  # chain 2: never accepted, no state
    c.exchanged[...] = np.where(rng.random(c.exchanged.shape) < 0.2, rng.integers(1, N + 1, c.exchanged.shape), 0)
    c.status[...] = np.where(rng.random(c.status.shape) < 0.15, -1, 0)
    st.iter = T
    groups = (np.arange(N) // 4).astype(np.int32)
    h = S.hip_context(prob, opts)
    h.set_state(st, c)
    back = h.history(0, T)
    got = {}
    for sel in ("all", "accepted", "state"):
        for t0, t1, stride in ((0, T, 1), (4, 23, 3)):
            for mo in (False, True):
                got[sel, t0, mo] = check(h, t0, t1, stride, sel, mo, groups, hist=back)
                check(h, t0, t1, stride, sel, mo, np.arange(N, dtype=np.int32), hist=back)
                check(h, t0, t1, stride, sel, mo, None, hist=back)
    r = got["all", 0, False]
    assert np.isnan(r["mean"][5, 1, 0]) and np.isnan(r["quantile"][:, 5, 1, 0]).all() and r["count"][5, 1] == 4
    assert np.isnan(r["best_value"][7, 2]) and r["best_chain"][7, 2] == 10 and r["best_chain"][9, 0] == 2
    assert (r["var"][:, 2, :prob.np] == 0.0).all() and (r["n_exchanged"] > 0).any() and (r["n_failed"] > 0).any()
    assert (r["n_accepted"] + r["n_exchanged"] <= 4).all() and (got["accepted", 0, False]["count"] < 4).any()
    s = h.trace(0, T, 1, "state", False, np.arange(N, dtype=np.int32))
    assert np.isnan(s["mean"][:, 2]).all() and (s["count"][:, 2] == 1).all()


def test_p2p_shards_report_their_own_chains(S):
    from test_gpu_p2p import p2p_contexts, p2p_run_lockstep
    prob, opts = cm.serial_normal(N=64, T=30, ns=1000)
    ctxs = p2p_contexts(S, prob, opts, 2)
    p2p_run_lockstep(ctxs, 30)
    g3 = (np.arange(32) % 3).astype(np.int32)
    parts, hs = [], []
    for r, c in enumerate(ctxs):
        hist = c.history(0, 30)
        hs.append(hist)
        check(c, 0, 30, 1, "accepted", True, g3, hist=hist, chain_offset=32 * r)
        got = check(c, 3, 30, 2, "state", False, None, hist=hist, chain_offset=32 * r)
        assert ((got["best_chain"] > 32 * r) & (got["best_chain"] <= 32 * (r + 1))).all()
        parts.append(got)
    from types import SimpleNamespace
    cat = lambda f, ax: np.concatenate([getattr(x, f) for x in hs], axis=ax)
    both = SimpleNamespace(params=cat("params", 2), sim_moments=cat("sim_moments", 2), value=cat("value", 1), accepted=cat("accepted", 1),
                           exchanged=cat("exchanged", 1), status=cat("status", 1))
    want = TR.trace_from_history(both, 3, 30, 2, "state")
    for f in ("n_chains", "count", "n_accepted", "n_exchanged", "n_failed"):
        assert np.array_equal(parts[0][f] + parts[1][f], want[f]), f
    first = np.where((parts[0]["best_value"] <= parts[1]["best_value"]) | np.isnan(parts[0]["best_value"]), 0, 1)
    assert np.array_equal(np.where(first == 0, parts[0]["best_chain"], parts[1]["best_chain"]), want["best_chain"])


def test_invalid_arguments_and_output_subsets(S):
    N, T = 64, 20
    prob, opts = cm.serial_normal(N=N, T=T, ns=500)
    h = S.hip_context(prob, opts)
    twin = S.hip_context(prob, opts)
    h.step(T - 5)
    twin.step(T - 5)
    T1 = T - 5
    A = S._abi
    g = (np.arange(N) % 2).astype(np.int32)
    base = dict(t0=0, t1=T1, stride=2, select=1, moments=1, groups=g, n_groups=2, probs=(0.1, 0.9))
    bad = [dict(t1=T1 + 1), dict(t0=5, t1=4), dict(t0=-1), dict(stride=0), dict(stride=-3), dict(select=3), dict(select=-1),
           dict(n_groups=-1), dict(groups=None, n_groups=2), dict(groups=None, n_groups=0), dict(groups=np.where(np.arange(N) == 3, 2, 0)),
           dict(groups=np.where(np.arange(N) == 3, -2, 0)), dict(probs=(0.5, 1.5)), dict(probs=(-0.1,)), dict(probs=(np.nan,))]
    for b in bad:
        a = dict(base)
        a.update(b)
        rc, _ = raw_call(h, a["t0"], a["t1"], a["stride"], a["select"], a["moments"], a["groups"], a["n_groups"], a["probs"],
                         ("count", "mean", "quantile"))
        assert rc == A.SMM_ERR_INVALID_ARG, b
    rc, _ = raw_call(h, 0, T1, 2, 1, 1, g, 2, (), ("quantile",))   # quantile without probs
    assert rc == A.SMM_ERR_INVALID_ARG
    s = A.smm_trace_t()
    fn = h._fn("get_trace")
    assert fn(h._ctx, 0, T1, 1, 1, 0, None, 1, None, 1, C.byref(s)) == A.SMM_ERR_INVALID_ARG      # probs NULL with n_probs > 0
    assert fn(h._ctx, 0, T1, 1, 1, 0, None, 1, None, -1, C.byref(s)) == A.SMM_ERR_INVALID_ARG
    assert fn(h._ctx, 0, T1, 1, 1, 0, None, 1, None, 0, None) == A.SMM_ERR_INVALID_ARG
    assert fn(None, 0, T1, 1, 1, 0, None, 1, None, 0, C.byref(s)) == A.SMM_ERR_INVALID_ARG
    with pytest.raises(S.SMMHipError):
        h.trace(0, T1 + 1)
    hist = h.history(0, T1)
    all_fields = [f for f, _ in A.smm_trace_t._fields_]
    for sel in (1, 2):
        want = TR.trace_from_history(hist, 0, T1, 2, sel, True, g, (0.1, 0.9))
        for fields in [(f,) for f in all_fields] + [("iter", "var", "best_chain"), tuple(all_fields)]:
            rc, r = raw_call(h, 0, T1, 2, sel, 1, g, 2, (0.1, 0.9), fields)
            assert rc == 0, fields
            TR.assert_trace_equal(r, want, fields=fields)
    rc, r = raw_call(h, 0, T1, 2, 2, 1, g, 2, (0.1, 0.9), ("mean",))   # probs given, quantile NULL
    assert rc == 0
    h.step_async(3)                                       # right after an enqueued step; then the twin that never traced
    check(h, 0, T1 + 3, 1, "state", True, g)
    h.step(2)
    twin.step(5)
    cm.assert_history_equal(twin.history(), h.history(), exact_floats=True)
    cm.assert_state_equal(twin.state(), h.state(), rtol=0)


def test_host_trace_reads_the_device_and_matches_numpy(S, monkeypatch):
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
    ps = [S.params(c, accepted_only=False) for c in MA.chains]
    hs = [S.history(c) for c in MA.chains]
    MA._hist = None

    def no_download(*a, **k):
        raise AssertionError("the history was downloaded")
    monkeypatch.setattr(type(MA._ctx), "history", no_download)
    groups = np.array([0] * 32 + [1] * 16 + [0] * 8 + [2] * 8, np.int32)
    probs = (0.025, 0.5, 0.975)
    tr = S.trace(MA, state=False, moments=True)
    assert len(tr) == 3 and list(tr[0]["mean"]) == ["p1", "p2", "value", "mu1", "mu2"] and tr[0]["iter"].tolist() == list(range(T))
    for g, d in enumerate(tr):
        mem = np.flatnonzero(groups == g)
        assert d["chains"] == len(mem) and (d["count"] == len(mem)).all()
        cols = {k: np.array([[np.asarray(ps[c][k])[t] for c in mem] for t in range(T)]) for k in ("p1", "p2")}
        cols["value"] = np.array([[np.asarray(hs[c]["value"])[t] for c in mem] for t in range(T)])
        for k, X in cols.items():
            for t in range(T):
                w = TR.column_stats(X[t], probs)
                assert d["mean"][k][t] == w[0] and d["var"][k][t] == w[1] and d["median"][k][t] == w[2], (g, k, t)
                assert np.array_equal(d["quantile"][k][:, t], w[3]), (g, k, t)
        acc_t = np.array([[bool(np.asarray(hs[c]["accepted"])[t]) and np.asarray(hs[c]["exchanged"])[t] == 0 for c in mem] for t in range(T)])
        assert np.array_equal(d["n_accepted"], acc_t.sum(axis=1))
        assert np.array_equal(d["best_chain"], mem[np.argmin(cols["value"], axis=1)] + 1)
    want = TR.trace_from_history(h, 10, 70, 4, "state", False, groups, probs)
    st = S.trace(MA, window=(10, 70), stride=4)
    for g, d in enumerate(st):
        assert d["iter"].tolist() == list(range(10, 70, 4))
        for i, k in enumerate(("p1", "p2", "value")):
            assert np.array_equal(d["mean"][k], want["mean"][:, g, i], equal_nan=True)
            assert np.array_equal(d["quantile"][k], want["quantile"][:, :, g, i], equal_nan=True)
    one = S.trace(MA, groups=np.zeros(N, np.int32), probs=())
    assert len(one) == 1 and one[0]["quantile"]["p1"].shape == (0, T)


def test_julia_ccall_matches_the_abi():
    from smm_jl_amd import _abi as A
    src = open(os.path.join(ROOT, "julia", "SMMHip.jl")).read()
    m = re.search(r"ccall\(sym\(:smm_get_trace\), Cint,\s*\(([^()]*(?:\{[^()]*\}[^()]*)*)\)", src)
    assert m
    jl = [t.strip() for t in m.group(1).split(",") if t.strip()]
    spell = {C.c_void_p: "Ptr{Cvoid}", C.c_int32: "Cint", A.c_int32_p: "Ptr{Int32}", A.c_double_p: "Ptr{Cdouble}",
             C.POINTER(A.smm_trace_t): "Ref{SmmTrace}"}
    argtypes = dict((n, a) for n, _, a in A.SYMBOLS)["smm_get_trace"]
    assert jl == [spell[t] for t in argtypes]
    fields = re.search(r"struct SmmTrace\n(.*?)\nend", src, re.S).group(1).split()
    assert [f.split("::")[0] for f in fields] == [f for f, _ in A.smm_trace_t._fields_]
    glue = open(os.path.join(ROOT, "julia", "SMMHipBackend.jl")).read()
    assert re.search(r"function population_trace\(algo::MAlgoBGPHip;", glue) and "SMMHip.hip_trace(hip, t0, t1;" in glue
