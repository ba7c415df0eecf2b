"""smm_get_profile on the device (include/smmhip.h, smm.jl_amd/csrc/smm_profile.hpp): every output equal (array_equal, NaN equal to NaN,
the sign of a zero included) to the numerical contract restated in profile_ref.py over the history downloaded with smm_get_history of
the same context, and n / n2 equal to smm_get_histogram's hist / hist2 of the same arguments.  A small serialNormal with uneven groups,
all three selections, a window that starts inside the run, given ranges and outputs left NULL; the dense objective with np = 5, nm = 7;
one segment past a chunk, alone and through the scratch seam; a crafted history (unscored rows, ties, signed zeros, rows on edges,
statuses 1 and 3); the bad arguments; a twin context that never asked; two p2p shards; the host layer."""
import ctypes as C

import numpy as np
import pytest

import common as cm
import hist_ref as HR
import moment_stats_ref as MR
import profile_ref as PR
import rank_diag_ref as RD

pytestmark = pytest.mark.gpu

PAIRS = [(0, 1), (1, 0)]


def check(h, hist, t0, t1, select, groups, bins, rng=None, pairs=(), bins2=None, n_groups=None, moments=True, chain_offset=0):
    got = h.profile(t0, t1, select, groups, bins, rng, pairs, bins2, n_groups=n_groups, moments=moments)
    want = PR.profile_from_history(hist, t0, t1, select, groups, bins, rng, pairs, bins2, n_groups=n_groups, chain_offset=chain_offset,
                                   moments=moments)
    assert sorted(got) == sorted(want)
    PR.assert_profile_equal(got, want)
    hs = h.histogram(t0, t1, select, groups, bins, rng, pairs, bins2, n_groups=n_groups)
    assert np.array_equal(got["n"], hs["hist"]) and np.array_equal(got["status"], hs["status"]) and np.array_equal(got["count"], hs["count"])
    if len(pairs):
        assert np.array_equal(got["n2"], hs["hist2"])
    return got


def sentinel(G, npar, nm, B, NP, B2):
    shape = dict(count=(G,), status=(G, npar), edges=(G, npar, B + 1), theta_at_min=(G, npar, B, npar), m_mean=(G, npar, B, nm),
                 edges2=(G, npar, B2 + 1))
    a = {}
    for f, t in MR_TYPES.items():
        a[f] = np.full(shape.get(f, (G, NP, B2, B2) if f.endswith("2") else (G, npar, B)), -7.5 if t is float else -7, t)
    return a


MR_TYPES = dict(count=np.int64, status=np.int32, edges=float, n=np.int64, n_scored=np.int64, v_min=float, min_chain=np.int32,
                min_iter=np.int32, theta_at_min=float, v_mean=float, m_mean=float, edges2=float, n2=np.int64, n_scored2=np.int64,
                v_min2=float, min_chain2=np.int32, min_iter2=np.int32, v_mean2=float)


def untouched(a, fields=None):
    return all((a[f] == (-7.5 if a[f].dtype.kind == "f" else -7)).all() for f in (fields or a))


def raw(h, A, t0, t1, select, g, ng, bins, rng, pairs, bins2, arrays, skip=()):
    s = h._out(A.smm_profile_t, arrays, skip)
    gp = None if g is None else np.ascontiguousarray(g, np.int32)
    rg = None if rng is None else np.ascontiguousarray(rng, float)
    pr = None if pairs is None else np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    return h._fn("get_profile")(h._ctx, t0, t1, select, None if gp is None else gp.ctypes.data_as(A.c_int32_p), ng, bins,
                                None if rg is None else A.dptr(rg), None if pr is None or not len(pr) else pr.ctypes.data_as(A.c_int32_p),
                                0 if pr is None else len(pr), bins2, C.byref(s))


N1, T1 = 8, 40
G1 = np.array([0, 1, 1, -1, 3, 0, 3, 3], np.int32)       # three groups, a chain in no group and group 2 without a member


@pytest.fixture(scope="module")
def small(S):
    prob, opts = cm.serial_normal(**dict(RD.MIXING, N=N1, T=T1, acc_tuners=0.5, seed=4))
    h = S.hip_context(prob, opts)
    h.step(T1)
    return h, prob, opts, h.history(0, T1)


def test_small_serial_normal_selections_windows_ranges_and_null_outputs(S, small):
    h, prob, _, hist = small
    A = S._abi
    x = hist.params
    cut = np.array([[np.quantile(x[:, 0], 0.2), np.quantile(x[:, 0], 0.7)], [x[:, 1].min() - 1.0, x[:, 1].max() + 1.0]])   # cuts rows off
    flat = np.array([[float(x[20, 0, 0]), float(x[20, 0, 0])], [10.0, 10.0]])                                              # lo == hi
    for select in (0, 1, 2):
        for t0, t1 in ((0, T1), (7, 33)):                 # t0 > 0: the state series looks back before the window
            for bins in (1, 7):
                for rng in (None, cut, flat):
                    got = check(h, hist, t0, t1, select, G1, bins, rng, PAIRS, 5, n_groups=4)
                    assert got["count"][2] == 0 and (got["n"][2] == 0).all() and np.isnan(got["v_mean"][2]).all()
    acc = hist.accepted != 0
    assert (~acc[7:12]).any(), "no rejected row just inside the window: the look-back is not exercised"
    check(h, hist, 0, T1, 2, None, 7, cut, PAIRS, 5)      # no group vector: every chain in group 0
    check(h, hist, 12, 12, 1, G1, 3, None, PAIRS, 2, n_groups=4)   # an empty window
    want = PR.profile_from_history(hist, 7, 33, 2, G1, 7, cut, PAIRS, 5, n_groups=4)
    for keep in (PR.FIELDS[::2], PR.FIELDS[1::2], ("n",), ("v_min2", "count"), ("m_mean", "min_iter"), ("v_mean2",), ("theta_at_min", "edges2")):
        a = sentinel(4, 2, 2, 7, 2, 5)
        drop = [f for f in PR.FIELDS if f not in keep]
        assert raw(h, A, 7, 33, 2, G1, 4, 7, cut, PAIRS, 5, a, skip=drop) == A.SMM_OK
        PR.assert_profile_equal(a, want, keep)
        assert untouched(a, drop), keep


def test_dense_objective_with_np_5_and_nm_7(S):
    prob, opts = MR.dense_problem(5, 7, N=16, T=64)
    h = S.hip_context(prob, opts)
    h.step(64)
    hist = h.history(0, 64)
    g = (np.arange(16) % 2).astype(np.int32)
    for select in (0, 1, 2):
        got = check(h, hist, 0, 64, select, g, 6, None if select else np.tile([-0.4, 0.4], (5, 1)), [(0, 4), (3, 1), (2, 2)], 3)
        assert got["m_mean"].shape == (2, 5, 6, 7) and got["theta_at_min"].shape == (2, 5, 6, 5)
    check(h, hist, 9, 50, 2, g, 4, np.tile([-0.4, 0.4], (5, 1)), [(4, 0)], 4)


def test_a_segment_past_one_chunk_alone_and_in_batches(S, hooks, monkeypatch):
    N, T = 16, 600
    prob, opts = cm.serial_normal(**dict(RD.MIXING, N=N, T=T, acc_tuners=1.0, seed=1))
    h0 = S.hip_context(prob, opts)
    h0.step(T)
    hist = h0.history(0, T)
    want = check(h0, hist, 0, T, 0, None, 1, None, [(0, 1)], 1)   # 9600 rows in one bin: 8192 + 1408, the chunk straddling members
    assert want["n"].tolist() == [[[N * T], [N * T]]] and want["n_scored"][0, 0, 0] > 8192 and want["n2"][0, 0, 0, 0] == N * T
    monkeypatch.setenv("SMMHIP_STATS_SCRATCH", "4096")
    h = S.hip_context(prob, opts)                          # (the seam is read at creation)
    monkeypatch.delenv("SMMHIP_STATS_SCRATCH")
    h.set_state(h0.state(), hist)
    got = check(h, hist, 0, T, 0, None, 1, None, [(0, 1)], 1)     # one axis of one group at a time
    PR.assert_profile_equal(got, want)
    g = (np.arange(N) % 3).astype(np.int32)
    PR.assert_profile_equal(h.profile(11, 590, 2, g, 3, None, PAIRS, 2), h0.profile(11, 590, 2, g, 3, None, PAIRS, 2))
    cm.assert_history_equal(h.history(0, T), hist, exact_floats=True)


def test_crafted_history_unscored_rows_ties_zeros_edges_and_statuses(S, small):
    h0, prob, opts, hist = small
    c = MR.copy_history(hist)
    T = T1
    g = np.array([0, 0, 0, 1, 1, 2, 2, 3], np.int32)
    c.accepted[...] = 1
    c.accepted[::3, 1] = 0
    c.params[:, 0, :3], c.params[:, 1, :] = 0.25, 10.0     # group 0: every row in bin 1 of [0, 1] / 4 ...
    c.params[3, 0, 2] = c.params[9, 0, 1] = 0.75           # ... but two rows in bin 3, both unscored
    c.value[:, :3] = 5.0
    c.value[3, 2], c.value[9, 1] = np.nan, np.inf
    c.value[4, 1], c.value[2, 2], c.value[7, 0] = 1.0, 1.0, np.nan   # equal minima in chains 1 and 2: the earliest pooled row wins
    c.value[11, 0], c.status[11, 0] = np.inf, -1           # a failed evaluation
    c.sim_moments[5, 0, 0] = np.nan                        # a NaN moment in a scored row
    c.params[:, 0, 3:5] = np.linspace(0.1, 0.9, T)[:, None]
    c.params[6, 0, 4] = np.nan                             # group 1: a NaN among the draws (status 1 when autodetected)
    c.params[:, 0, 5:7] = 1e16 + 2.0 * (np.arange(T) % 3)[:, None]   # group 2: a narrow range at a large magnitude (status 3)
    c.params[:, 0, 7] = 0.5                                # group 3: x on an inner edge ...
    c.params[5, 0, 7], c.params[6, 0, 7] = 1.0, 0.0        # ... on hi and on lo
    c.value[:, 7] = 3.0
    c.value[8, 7], c.value[30, 7] = -0.0, 0.0              # -0 ahead of +0
    h = S.hip_context(prob, opts)
    h.set_state(h0.state(), c)
    back = h.history(0, T)
    rng = np.array([[0.0, 1.0], [9.0, 11.0]])
    for select in (0, 1, 2):
        for t0, t1 in ((0, T), (4, 37)):
            check(h, back, t0, t1, select, g, 4, rng, PAIRS, 4)
            check(h, back, t0, t1, select, g, 7, None, PAIRS, 3)
    r = h.profile(0, T, 0, g, 4, rng)
    assert r["n"][0, 0].tolist() == [0, 3 * T - 2, 0, 2] and r["n_scored"][0, 0].tolist() == [0, 3 * T - 4, 0, 0]
    assert (r["v_min"][0, 0, 1], r["min_chain"][0, 0, 1], r["min_iter"][0, 0, 1]) == (1.0, 2, 5)
    assert np.isnan(r["v_min"][0, 0, 3]) and np.isnan(r["v_mean"][0, 0, 3]) and np.isnan(r["theta_at_min"][0, 0, 3]).all()
    assert r["v_mean"][0, 0, 1] == (5.0 * (3 * T - 6) + 2.0) / (3 * T - 4)
    assert np.isnan(r["m_mean"][0, 0, 1, 0]) and np.isfinite(r["m_mean"][0, 0, 1, 1])
    assert r["n"][3, 0].tolist() == [1, 0, T - 2, 1]
    assert r["v_min"][3, 0, 2] == 0.0 and np.signbit(r["v_min"][3, 0, 2]) and r["min_iter"][3, 0, 2] == 9 and r["min_chain"][3, 0, 2] == 8
    a = h.profile(0, T, 0, g, 7)
    assert a["status"][1, 0] == 1 and a["status"][2, 0] == 3 and a["status"][0, 0] == 0
    for q in (1, 2):
        assert (a["n"][q, 0] == 0).all() and np.isnan(a["v_min"][q, 0]).all() and (a["min_chain"][q, 0] == 0).all()
    assert np.isnan(a["edges"][1, 0]).all() and np.isfinite(a["edges"][2, 0]).all()


def test_invalid_arguments_leave_the_outputs_untouched(S, small):
    h, prob, _, hist = small
    A = S._abi
    bad_id, low_id = G1.copy(), G1.copy()
    bad_id[3], low_id[5] = 4, -2
    ok = dict(t0=3, t1=T1, select=2, g=G1, ng=4, bins=7, rng=None, pairs=PAIRS, bins2=5)
    bad = [dict(t0=-1), dict(t1=T1 + 1), dict(t0=9, t1=8), dict(select=3), dict(select=-1), dict(ng=-1), dict(g=None, ng=2),
           dict(g=None, ng=0), dict(g=bad_id), dict(g=low_id), dict(bins=0), dict(bins=4097), dict(rng=[[1.0, 0.0], [0.0, 1.0]]),
           dict(rng=[[0.0, np.inf], [0.0, 1.0]]), dict(rng=[[np.nan, 1.0], [0.0, 1.0]]), dict(pairs=[(0, 2)]), dict(pairs=[(-1, 0)]),
           dict(pairs=[(0, 1)] * 5), dict(bins2=0), dict(bins2=257), dict(pairs=[])]
    for b in bad:
        k = dict(ok, **b)
        a = sentinel(4, 2, 2, 7, 2, 5)
        assert raw(h, A, k["t0"], k["t1"], k["select"], k["g"], k["ng"], k["bins"], k["rng"], k["pairs"], k["bins2"], a) == A.SMM_ERR_INVALID_ARG, b
        assert len(h._fn("last_error")(h._ctx).decode()) > 0 and untouched(a), b
    fn = h._fn("get_profile")
    a = sentinel(4, 2, 2, 7, 2, 5)
    s = h._out(A.smm_profile_t, a)
    gp = G1.ctypes.data_as(A.c_int32_p)
    assert fn(None, 3, T1, 2, gp, 4, 7, None, None, 0, 5, C.byref(s)) == A.SMM_ERR_INVALID_ARG
    assert fn(h._ctx, 3, T1, 2, gp, 4, 7, None, None, 0, 5, None) == A.SMM_ERR_INVALID_ARG
    assert fn(h._ctx, 3, T1, 2, gp, 4, 7, None, None, 2, 5, C.byref(s)) == A.SMM_ERR_INVALID_ARG and untouched(a)   # pairs NULL
    with pytest.raises(S.SMMHipError):
        h.profile(0, T1, 5)
    check(h, hist, 0, T1, 1, G1, 3, n_groups=4)          # the context still answers


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
        check(b, hist, 5, 30, select, g, 9, np.array([[-3.0, 3.0], [-20.0, 20.0]]), [(0, 1)], 6)
    cm.assert_history_equal(b.history(0, 30), hist, exact_floats=True)
    cm.assert_state_equal(b.state(), state, rtol=0)
    for h in (a, b):
        h.step(30)
        assert (h.persistent_info()[1] >= 1) == persistent
    cm.assert_history_equal(a.history(), b.history(), exact_floats=True)
    cm.assert_state_equal(a.state(), b.state(), rtol=0)


def test_p2p_shards_report_their_own_chains(S):
    from types import SimpleNamespace
    from test_gpu_p2p import p2p_contexts, p2p_run_lockstep
    prob, opts = cm.serial_normal(N=64, T=30, ns=1000)
    ctxs = p2p_contexts(S, prob, opts, 2)
    p2p_run_lockstep(ctxs, 30)
    rng = np.array([[-3.0, 3.0], [-20.0, 20.0]])
    g3 = (np.arange(32) % 3).astype(np.int32)
    g3[5] = -1
    tot, hs = None, []
    for r, c in enumerate(ctxs):
        hist = c.history(0, 30)
        hs.append(hist)
        assert hist.value.shape[1] == 32
        for select in (0, 1, 2):
            check(c, hist, 3, 30, select, g3, 5, rng, [(0, 1)], 3, chain_offset=32 * r)
        got = check(c, hist, 0, 30, 2, None, 9, rng, [(0, 1)], 4, chain_offset=32 * r)
        tot = got if tot is None else {k: tot[k] + got[k] for k in ("count", "n", "n2")}
    both = SimpleNamespace(params=np.concatenate([h.params for h in hs], axis=2), accepted=np.concatenate([h.accepted for h in hs], axis=1),
                           value=np.concatenate([h.value for h in hs], axis=1), exchanged=np.concatenate([h.exchanged for h in hs], axis=1))
    want = HR.histogram_from_history(both, 0, 30, "state", None, 9, rng, [(0, 1)], 4)
    assert np.array_equal(tot["n"], want["hist"]) and np.array_equal(tot["n2"], want["hist2"]) and np.array_equal(tot["count"], want["count"])


def test_host_profile_and_profile2d_read_the_device(S, monkeypatch):
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
    rng = {"p1": (-1.0, 1.0), "p2": (9.0, 11.0)}
    rows = np.array([rng["p1"], rng["p2"]])
    want = PR.profile_from_history(hist, 10, 70, 1, groups, 6, rows, [(1, 0)], 5)
    got = S.profile(MA, bins=6, range=rng, window=(10, 70))
    assert len(got) == 3
    for g, d in enumerate(got):
        assert list(d) == ["p1", "p2"]
        for i, k in enumerate(d):
            e = d[k]
            assert list(e) == ["edges", "n", "n_scored", "v_min", "min_chain", "min_iter", "theta_at_min", "v_mean", "m_mean"]
            assert e["edges"].shape == (7,) and e["v_min"].shape == (6,) and list(e["m_mean"]) == ["mu1", "mu2"] and list(e["theta_at_min"]) == ["p1", "p2"]
            for f in ("edges", "n", "n_scored", "v_min", "min_chain", "min_iter", "v_mean"):
                assert np.array_equal(e[f], want[f][g, i], equal_nan=True), (f, g, k)
            assert np.array_equal(e["m_mean"]["mu2"], want["m_mean"][g, i, :, 1], equal_nan=True)
            assert np.array_equal(e["theta_at_min"]["p2"], want["theta_at_min"][g, i, :, 1], equal_nan=True)
    bare = S.profile(MA, bins=6, range=rng, window=(10, 70), moments=False)
    assert all("m_mean" not in d[k] for d in bare for k in d) and np.array_equal(bare[1]["p1"]["v_mean"], got[1]["p1"]["v_mean"], equal_nan=True)
    surf = S.profile2d(MA, ("p2", "p1"), bins=5, range=[rng["p2"], rng["p1"]], window=(10, 70))
    assert len(surf) == 3
    for g, d in enumerate(surf):
        assert list(d) == ["xedges", "yedges", "n", "n_scored", "v_min", "min_chain", "min_iter", "v_mean"] and d["v_min"].shape == (5, 5)
        for f in ("n", "n_scored", "v_min", "min_chain", "min_iter", "v_mean"):
            assert np.array_equal(d[f], want[f + "2"][g, 0], equal_nan=True), (f, g)
        assert np.array_equal(d["xedges"], want["edges2"][g, 1]) and np.array_equal(d["yedges"], want["edges2"][g, 0])
    ch = MA.chains[40]
    one = PR.profile_from_history(hist, 0, Th, 2, np.where(np.arange(Nh) == 40, 0, -1).astype(np.int32), 4, rows, [(0, 1)], 3, n_groups=1)
    d = S.profile(ch, bins=4, range=rng, state=True)
    assert list(d) == ["p1", "p2"] and np.array_equal(d["p2"]["v_min"], one["v_min"][0, 1], equal_nan=True)
    assert (d["p1"]["min_chain"][d["p1"]["n_scored"] > 0] == 41).all()
    d2 = S.profile2d(ch, ("p1", "p2"), bins=3, range=[rng["p1"], rng["p2"]], state=True)
    assert np.array_equal(d2["v_mean"], one["v_mean2"][0, 0], equal_nan=True) and np.array_equal(d2["n"], one["n2"][0, 0])
    with pytest.raises(ValueError):
        S.profile(ch, bins=0)
    with pytest.raises(ValueError):
        S.profile(ch, range={"p1": (1.0, 0.0), "p2": (0.0, 1.0)})
