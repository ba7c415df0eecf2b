"""smm_get_adjustment on the device (include/smmhip.h, smm.jl_amd/csrc/smm_adjust.hpp): every output equal (array_equal, NaN equal to
NaN, so the quantiles up to the sign of a zero) to the numerical contract restated in adjust_ref.py over the history downloaded with
smm_get_history of the same context.  A small serialNormal with uneven groups, the three selections, a window that starts inside the
run, both kernels, two tolerances, a given scale and outputs left NULL; the dense objective with np = 5, nm = 7; a pooled column past
one chunk, alone, through the scratch seam and, at the small shape, with the grid-wide forms forced; np = nm = 64; the status table on
crafted histories and every refusal; a twin context that never asked; two p2p shards; the host layer."""
import ctypes as C

import numpy as np
import pytest

import adjust_ref as AR
import common as cm
import moment_stats_ref as MR
import rank_diag_ref as RD

pytestmark = pytest.mark.gpu

PROBS = (0.025, 0.5, 0.975)


def check(h, prob, hist, t0, t1, select, groups, tol=0.25, kernel=1, scale=None, ridge=0.0, probs=PROBS, n_groups=None):
    got = h.adjustment(t0, t1, select, groups, tol, kernel, scale, ridge, probs, n_groups=n_groups)
    want = AR.adjustment_from_history(hist, t0, t1, select, groups, tol, kernel, scale, ridge, probs, prob.mom, prob.w, prob.lb, prob.ub,
                                      n_groups=n_groups)
    AR.assert_adjustment_equal(got, want)
    return got


def raw(h, A, arrays, t0, t1, select, g, ng, tol, kernel, scale, ridge, probs, skip=()):
    s = h._out(A.smm_adjustment_t, arrays, skip)
    gp = None if g is None else g.ctypes.data_as(A.c_int32_p)
    p = None if probs is None else A.f64(probs)
    sc = None if scale is None else A.f64(scale)
    return h._fn("get_adjustment")(h._ctx, t0, t1, select, gp, ng, tol, kernel, None if sc is None else A.dptr(sc), ridge,
                                   None if p is None else A.dptr(p), 0 if p is None else len(p), C.byref(s))


def sentinel(G, npar, nm, nq):
    return dict(count=np.full(G, -7, np.int64), n_chains=np.full(G, -7, np.int32), status=np.full(G, -7, np.int32),
                n_kept=np.full(G, -7, np.int64), bandwidth=np.full(G, -7.5), sum_w=np.full(G, -7.5), ess=np.full(G, -7.5),
                x_mean=np.full((G, nm), -7.5), raw_mean=np.full((G, npar), -7.5), beta=np.full((G, nm, npar), -7.5),
                adj_mean=np.full((G, npar), -7.5), adj_sd=np.full((G, npar), -7.5), adj_quantile=np.full((nq, G, npar), -7.5),
                n_outside=np.full((G, npar), -7, np.int64))


def untouched(a, fields=None):
    return all((a[f] == (-7.5 if a[f].dtype.kind == "f" else -7)).all() for f in (fields or a))


N1, T1 = 8, 40
G1 = np.array([0, 1, 1, -1, 3, 0, 3, 3], np.int32)       # three groups, a chain in no group and group 2 without a member
SMALL = dict(RD.MIXING, N=N1, T=T1, acc_tuners=0.5, seed=4)


@pytest.fixture(scope="module")
def small(S):
    prob, opts = cm.serial_normal(**SMALL)
    h = S.hip_context(prob, opts)
    h.step(T1)
    return h, prob, h.history(0, T1)


def test_small_serial_normal_selections_windows_kernels_and_null_outputs(S, small):
    h, prob, hist = small
    A = S._abi
    sd = np.array([0.37, 2.5])
    kept = set()
    for select in (0, 1, 2):                               # (the state series repeats rows: tie runs for the weighted select)
        for t0, t1 in ((0, T1), (7, 33)):
            for kernel in (0, 1):
                for tol in (0.25, 1.0):
                    for probs in ((), PROBS):
                        for scale in (None, sd):
                            got = check(h, prob, hist, t0, t1, select, G1, tol, kernel, scale, 0.0, probs, n_groups=4)
                            assert got["n_chains"].tolist() == [2, 2, 0, 3] and got["status"][2] == 1
                            kept.update(got["status"].tolist())
    assert 0 in kept, kept
    st = h.adjustment(0, T1, 2, G1, 0.25, 1, None, 0.0, PROBS, n_groups=4)
    assert st["status"].tolist() == [0, 0, 1, 0] and (st["n_kept"][[0, 1, 3]] >= 4).all() and (st["ess"][[0, 1, 3]] > 1).all()
    check(h, prob, hist, 0, T1, 2, None, 0.5, 1, None, 1e-6)                    # no group vector: every chain in group 0
    check(h, prob, hist, 12, 12, 1, G1, n_groups=4)                             # an empty window
    want = AR.adjustment_from_history(hist, 7, 33, 2, G1, 0.25, 1, None, 0.0, PROBS, prob.mom, prob.w, prob.lb, prob.ub, n_groups=4)
    for keep in (("count", "status"), ("adj_mean",), ("n_outside",), ("adj_quantile", "beta"), ("ess", "n_chains", "x_mean"),
                 ("n_kept", "bandwidth", "sum_w", "raw_mean", "adj_sd")):
        a = sentinel(4, 2, 2, 3)
        assert raw(h, A, a, 7, 33, 2, G1, 4, 0.25, 1, None, 0.0, PROBS, skip=[f for f in AR.FIELDS if f not in keep]) == A.SMM_OK
        AR.assert_adjustment_equal(a, want, keep)
        assert untouched(a, [f for f in AR.FIELDS if f not in keep]), keep


def test_dense_objective_with_np_5_and_nm_7(S):
    prob, opts = MR.dense_problem(5, 7, N=16, T=64)
    h = S.hip_context(prob, opts)
    h.step(64)
    hist = h.history(0, 64)
    g = (np.arange(16) % 2).astype(np.int32)
    for select in (0, 1, 2):
        for kernel in (0, 1):
            got = check(h, prob, hist, 0, 64, select, g, 0.5, kernel)
            assert got["beta"].shape == (2, 7, 5) and got["x_mean"].shape == (2, 7) and got["adj_quantile"].shape == (3, 2, 5)
    got = check(h, prob, hist, 0, 64, 0, g, 0.5, 1)
    assert (got["status"] == 0).all(), got["status"]
    check(h, prob, hist, 9, 50, 2, g, 0.8, 1, np.linspace(0.5, 2.0, 7), 1e-8, (0.5,))
    check(h, prob, hist, 0, 64, 0, g, 0.5, 1, probs=(0.0, 0.1, 0.5, 0.9, 1.0))   # more probs than one workgroup of the select counts


def test_a_pooled_column_past_one_chunk_alone_in_batches_and_grid_wide(S, small, hooks, monkeypatch):
    N, T = 16, 600
    prob, opts = cm.serial_normal(**dict(RD.MIXING, N=N, T=T, acc_tuners=1.0, seed=1))
    h0 = S.hip_context(prob, opts)
    h0.step(T)
    hist = h0.history(0, T)
    want = check(h0, prob, hist, 0, T, 0, None)            # 9600 > 8192 pooled rows: two chunks, the grid-wide select of the bandwidth
    assert want["count"].tolist() == [N * T] and want["status"].tolist() == [0]
    check(h0, prob, hist, 0, T, 2, None, 0.1, 0)
    cap = 4096
    monkeypatch.setenv("SMMHIP_STATS_SCRATCH", str(cap))
    h = S.hip_context(prob, opts)                          # (the seam is read at creation)
    monkeypatch.delenv("SMMHIP_STATS_SCRATCH")
    h.set_state(h0.state(), hist)
    # smm_reducers_host.hpp's plan under the seam: two pooled columns and one chunk of the D + 2 = 6 columns are the minimum
    D, Mtot = 4, N * T
    col8, chunk8 = Mtot * 8, (D + 2) * 8192 * 8
    avail = max(cap, 2 * col8 + chunk8) - 2 * col8
    Nbc = max(1, min(2, avail // 2 // chunk8, cap // (D * D * 8)))
    jb = min(2, 1 + (avail - Nbc * chunk8) // col8)
    assert Nbc == 1 and jb == 1                            # the two chunks one at a time, and the adjusted parameters one at a time
    AR.assert_adjustment_equal(check(h, prob, hist, 0, T, 0, None), want)
    g = (np.arange(N) % 3).astype(np.int32)
    AR.assert_adjustment_equal(check(h, prob, hist, 11, 590, 2, g), h0.adjustment(11, 590, 2, g, 0.25, 1, None, 0.0, PROBS))
    cm.assert_history_equal(h.history(0, T), hist, exact_floats=True)
    # the small shape with every pooled column taken as a long one: the grid-wide select of the bandwidth, and the weighted select with
    # one row per workgroup (k_adjust_hist's blocks of per = 1 rows), so that the weights of columns of 40 to 120 rows are added across
    # workgroups in global memory
    hs, sprob, shist = small
    monkeypatch.setenv("SMMHIP_GROUP_WIDE_MIN", "1")
    hw = S.hip_context(*cm.serial_normal(**SMALL))
    monkeypatch.delenv("SMMHIP_GROUP_WIDE_MIN")
    hw.set_state(hs.state(), shist)
    for select in (0, 2):
        for kernel in (0, 1):
            got = check(hw, sprob, shist, 0, T1, select, G1, 0.25, kernel, n_groups=4)
            AR.assert_adjustment_equal(got, hs.adjustment(0, T1, select, G1, 0.25, kernel, None, 0.0, PROBS, n_groups=4))


def test_np_64_and_nm_64_on_a_crafted_history(S):
    """D = 128: the 16 x 16 tiles of pair sums and the 64-lane solve; moments linear in the parameters (moment_stats_ref.crafted_linear,
    the design of tests/test_gpu_reducer_caps.py), m = 320 rows"""
    N, T = 4, 80
    prob, opts = MR.dense_problem(64, 64, N=N, T=T)
    h0 = S.hip_context(prob, opts)
    h0.step(T)
    crafted = MR.crafted_linear(64, 64, N, T, 7, into=MR.copy_history(h0.history(0, T)))[0]
    h = S.hip_context(prob, opts)
    h.set_state(h0.state(), crafted)
    back = h.history(0, T)
    got = check(h, prob, back, 0, T, 0, None, 1.0, 0)
    assert got["count"].tolist() == [320] and got["status"].tolist() == [0] and got["beta"].shape == (1, 64, 64)
    check(h, prob, back, 0, T, 2, None, 0.9, 1, None, 1e-8, (0.5,))
    check(h, prob, back, 0, T, 0, None, 0.1, 0)            # 32 kept rows < nm + 2: status 3


def test_status_table_on_crafted_histories_and_every_refusal(S, small):
    h0, prob, hist = small
    A = S._abi
    st = h0.state()
    mem = np.flatnonzero(G1 == 3)
    c = MR.copy_history(hist)
    c.sim_moments[20, 1, 1], c.accepted[20, 1] = np.nan, 1  # group 1 (chains 1, 2): a NaN moment
    c.sim_moments[:30, 0, mem], c.sim_moments[:30, 1, mem] = prob.mom[0], prob.mom[1]   # group 3: three rows in four sit on the data
    h = S.hip_context(*cm.serial_normal(**SMALL))
    h.set_state(st, c)
    back = h.history(0, T1)
    got = check(h, prob, back, 0, T1, 0, G1, 0.5, 1, n_groups=4)
    assert got["status"].tolist() == [0, 2, 1, 3] and got["bandwidth"][3] == 0.0 and got["n_kept"][3] == 0, (got["status"], got["bandwidth"])
    assert np.isnan(got["raw_mean"][1]).all() and got["count"][1] == 80 and got["n_kept"][1] == 0 and np.isnan(got["adj_quantile"][:, 3]).all()
    got = check(h, prob, back, 0, T1, 0, G1, 0.03, 0, n_groups=4)   # too few kept rows: 3 of 80 < nm + 2
    assert got["status"][0] == 3 and got["n_kept"][0] == 3 and np.isfinite(got["raw_mean"][0]).all() and np.isnan(got["beta"][0]).all()
    one = np.full(N1, -1, np.int32)
    one[5] = 1
    got = check(h, prob, back, 10, 11, 0, one, n_groups=2)  # fewer than two rows: no member, and one chain over one iteration
    assert got["status"].tolist() == [1, 1] and got["count"].tolist() == [0, 1] and np.isnan(got["bandwidth"]).all()
    c4 = MR.copy_history(hist)                             # two moments that hold the same column, in values whose sums are exact
    for k in range(2):
        c4.sim_moments[:32, k, 5] = prob.mom[k] + AR.COLLINEAR_COLUMN
    h.set_state(st, c4)
    back = h.history(0, T1)
    got = check(h, prob, back, 0, 32, 0, one, 1.0, 0, n_groups=2)
    assert got["status"].tolist() == [1, 4] and got["n_kept"][1] == 32 and np.isnan(got["adj_mean"][1]).all() and (got["n_outside"] == 0).all()
    got = check(h, prob, back, 0, 32, 0, one, 1.0, 0, None, 1e-6, n_groups=2)
    assert got["status"].tolist() == [1, 0] and np.isfinite(got["beta"][1]).all() and np.isfinite(got["adj_quantile"][:, 1]).all()

    bad_id, low_id = G1.copy(), G1.copy()
    bad_id[3], low_id[5] = 4, -2
    ok = dict(t0=3, t1=T1, select=2, g=G1, ng=4, tol=0.25, kernel=1, scale=None, ridge=0.0, probs=PROBS)
    bad = [dict(t0=-1), dict(t1=T1 + 1), dict(t0=9, t1=8), dict(select=3), dict(select=-1), dict(ng=-1), dict(g=None, ng=2),
           dict(g=None, ng=0), dict(g=bad_id), dict(g=low_id), dict(probs=(0.5, 1.5)), dict(probs=(np.nan,)), dict(probs=None),
           dict(tol=0.0), dict(tol=-0.1), dict(tol=1.0000001), dict(tol=np.nan), dict(tol=np.inf), dict(kernel=2), dict(kernel=-1),
           dict(scale=(1.0, 0.0)), dict(scale=(-1.0, 1.0)), dict(scale=(1.0, np.inf)), dict(scale=(np.nan, 1.0)),
           dict(ridge=-1e-9), dict(ridge=np.inf), dict(ridge=np.nan)]
    for b in bad:
        k = dict(ok, **b)
        a = sentinel(4, 2, 2, 3)
        rc = raw(h0, A, a, k["t0"], k["t1"], k["select"], k["g"], k["ng"], k["tol"], k["kernel"], k["scale"], k["ridge"], k["probs"])
        assert rc == A.SMM_ERR_INVALID_ARG, b
        assert len(h0._fn("last_error")(h0._ctx).decode()) > 0 and untouched(a), b
    a = sentinel(4, 2, 2, 3)
    assert raw(h0, A, a, 3, T1, 2, G1, 4, 0.25, 1, None, 0.0, PROBS) == A.SMM_OK and not untouched(a, ["status", "adj_quantile"])
    fn = h0._fn("get_adjustment")
    a = sentinel(4, 2, 2, 3)
    s = h0._out(A.smm_adjustment_t, a)
    gp, pp = G1.ctypes.data_as(A.c_int32_p), A.f64(PROBS)
    assert fn(None, 3, T1, 2, gp, 4, 0.25, 1, None, 0.0, A.dptr(pp), 3, C.byref(s)) == A.SMM_ERR_INVALID_ARG
    assert fn(h0._ctx, 3, T1, 2, gp, 4, 0.25, 1, None, 0.0, A.dptr(pp), 3, None) == A.SMM_ERR_INVALID_ARG and untouched(a)
    with pytest.raises(S.SMMHipError):
        h0.adjustment(0, T1, 5)


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
    # every chain a group of its own and five probs: 512 columns of the weighted select, more than its histograms hold at a time
    got = check(b, prob, hist, 5, 30, 0, np.arange(256, dtype=np.int32), 0.5, 1, probs=(0.0, 0.1, 0.5, 0.9, 1.0))
    assert (got["status"] == 0).sum() > 200, np.bincount(got["status"])
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
        check(c, prob, hist, 0, 30, 2, None, 0.5, 0)


def test_host_adjusted_reads_the_device(S, monkeypatch):
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
    ps = S.ps2s_names(m)
    mom, w, lb, ub = [-1.0, 10.0], [1.0, 2.0], [-3.0, -20.0], [3.0, 20.0]
    sd = np.sqrt(np.diagonal(MR.moment_stats_from_history(hist, 10, 70, 1, None, (), 0.0, mom, w)["cov_mm"][0]))
    for kw, sel, scale in ((dict(), 2, None), (dict(state=False, window=(10, 70), scale="sd", kernel="uniform", tol=0.5), 1, sd)):
        t0, t1 = kw.get("window", (0, Th))
        level = 0.9
        q = ((1 - level) / 2, 1 - (1 - level) / 2)
        want = AR.adjustment_from_history(hist, t0, t1, sel, groups, kw.get("tol", 0.2), kw.get("kernel", "epanechnikov"), scale, 0.0, q,
                                          mom, w, lb, ub)
        got = S.adjusted(MA, level=level, **kw)
        assert len(got) == 3
        for g in range(3):
            r = got[g]
            assert r["count"] == want["count"][g] and r["chains"] == want["n_chains"][g] and r["status"] == want["status"][g]
            assert r["n_kept"] == want["n_kept"][g] and np.array_equal(r["ess"], want["ess"][g], equal_nan=True)
            assert list(r["raw_mean"]) == list(r["adj_mean"]) == list(r["adj_sd"]) == list(r["band"]) == list(r["n_outside"]) == ps
            for j, p in enumerate(ps):
                assert np.array_equal([r["raw_mean"][p], r["adj_mean"][p], r["adj_sd"][p]],
                                      [want["raw_mean"][g, j], want["adj_mean"][g, j], want["adj_sd"][g, j]], equal_nan=True)
                assert np.array_equal(r["band"][p], want["adj_quantile"][:, g, j], equal_nan=True) and r["n_outside"][p] == want["n_outside"][g, j]
