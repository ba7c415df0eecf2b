"""smm_get_chain_stats on the device (include/smmhip.h, smm.jl_amd/csrc/smm_stats.hpp): every field equal (array_equal, NaN equal to NaN)
to the numerical contract restated in chain_stats_ref.py over the history downloaded with smm_get_history — for the persistent and
the tile objectives, a user objective, columns past the LDS, crafted histories, p2p shards — the call leaves the run untouched, and the
host readers (mean, median, CI, best, summary) take it instead of downloading the history."""
import numpy as np
import pytest

import chain_stats_ref as R
import common as cm

pytestmark = pytest.mark.gpu
PROBS = (0.0, 0.025, 0.5, 0.975, 1.0)


def check(h, t0, t1, accepted_only, probs=PROBS, hist=None):
    hist = h.history(0, t1) if hist is None else hist
    got = h.chain_stats(t0, t1, accepted_only, probs)
    R.assert_stats_equal(got, R.stats_from_history(hist, t0, t1, accepted_only, probs))
    return got


def test_objfunc_norm_persistent_windows(S):
    prob, opts = cm.serial_normal(N=256, T=300)
    h = S.hip_context(prob, opts)
    h.step(300)
    assert h.persistent_info()[1] >= 1
    hist = h.history(0, 300)
    for acc in (True, False):
        for t0, t1 in ((0, 300), (50, 120), (120, 120)):
            got = check(h, t0, t1, acc, hist=hist)
            if t0 == t1:
                assert (got["count"] == 0).all() and np.isnan(got["mean"]).all() and (got["best_iter"] == 0).all()
    with pytest.raises(S.SMMHipError):
        h.chain_stats(0, 301)
    with pytest.raises(S.SMMHipError):
        h.chain_stats(0, 300, probs=[0.5, 1.5])
    with pytest.raises(S.SMMHipError):
        h.chain_stats(0, 300, probs=[np.nan])


def test_dense2_np50_and_a_map_reduce_user_objective(S):
    from user_objective_src import PANEL_SOURCE
    from test_user_objective import panel_problem
    from smm_jl_amd.workloads import build_problem
    prob, opts = build_problem("c5", 32, 32, 0, 60, 0)   # SMM_OBJ_DENSE2, np = nm = 50 (BASELINE config 5's instance)
    assert prob.objective_id == S._abi.SMM_OBJ_DENSE2 and prob.np == 50
    h = S.hip_context(prob, opts)
    h.step(60)
    for acc in (True, False):
        check(h, 0, 60, acc)
        check(h, 7, 41, acc)
    prob, opts = panel_problem(S, S.register_user_objective(PANEL_SOURCE, n_sums=3, lanes=64), N=32, T=40)
    h = S.hip_context(prob, opts)
    h.step(40)
    for acc in (True, False):
        check(h, 0, 40, acc)


def test_columns_longer_than_the_lds(S):
    prob, opts = cm.serial_normal(N=64, T=20000, ns=500)
    h = S.hip_context(prob, opts)
    h.step(20000)
    hist = h.history(0, 20000)
    got = check(h, 0, 20000, False, probs=(0.0, 0.025, 0.5, 0.975, 1.0), hist=hist)
    assert (got["count"] == 20000).all() and (got["n_exchanged"] > 0).all()
    check(h, 3, 19000, True, probs=(0.1, 0.9), hist=hist)


def test_crafted_histories(S):
    N, T = 16, 40
    prob, opts = cm.serial_normal(N=N, T=T, ns=100)
    h = S.hip_context(prob, opts)
    h.step(2)
    st = h.state()
    hb = h.history(0, 2)
    rng = np.random.default_rng(11)
    from smm_jl_amd import _abi as A
    c = A.HistoryBuffers(T, N, prob.np, prob.nm)
    for f in A.HistoryBuffers.FIELDS:
        getattr(c, f)[...] = getattr(hb, f)[rng.integers(0, 2, T)]
    pool = np.array([-0.0, 0.0, 1.0, 1.0, -np.inf, np.inf, 2.0, -3.0])
    c.params[...] = rng.choice(pool, c.params.shape)
    c.params[:, :, 3] = rng.standard_normal((T, prob.np))
    c.params[5, 0, 4] = np.nan                       # chain 4: NaN among its first parameter's draws
    c.params[:, 1, 6] = -0.0                         # chain 6: a column of -0 only
    c.value[...] = rng.choice(np.array([0.5, 0.25, 0.25, 1.0]), c.value.shape)
    c.value[9, 7] = np.nan; c.value[20, 7] = np.nan  # chain 7: the first NaN is the best
    c.value[:, 8] = -0.0; c.value[3, 8] = 0.0        # chain 8: all tied: the first
    c.accepted[...] = rng.random(c.accepted.shape) < 0.6
    c.accepted[:, 2] = 0                             # chain 2: no accepted draw
    c.exchanged[...] = 0
    c.exchanged[:4, 0] = [5, 3, 5, 3]                # tied partners: the smaller id
    c.exchanged[::3, 1] = rng.integers(1, N + 1, len(range(0, T, 3)))
    c.exchanged[:, 9] = 16
    st.iter = T
    h.set_state(st, c)
    back = h.history(0, T)
    for acc in (True, False):
        for t0, t1 in ((0, T), (4, 23)):
            got = check(h, t0, t1, acc, probs=(0.0, 0.3, 0.5, 1.0), hist=back)
    got = h.chain_stats(0, T, True, (0.5,))
    assert got["count"][2] == 0 and np.isnan(got["median"][:, 2]).all()
    assert np.isnan(got["mean"][0, 4]) or got["count"][4] == 0 or not c.accepted[5, 4]
    assert got["most_exchanged_with"][0] == 3 and got["most_exchanged_with"][9] == 16
    assert np.isnan(got["best_value"][7]) and got["best_iter"][7] == 10 and got["best_iter"][8] == 1


def test_p2p_shards_report_their_slice(S):
    from test_gpu_p2p import p2p_contexts, p2p_run_lockstep
    prob, opts = cm.serial_normal(N=64, T=30, ns=1000)
    single = S.hip_context(prob, opts)
    single.step(30)
    ctxs = p2p_contexts(S, prob, opts, 2)
    p2p_run_lockstep(ctxs, 30)
    for acc in (True, False):
        whole = single.chain_stats(0, 30, acc, PROBS)
        R.assert_stats_equal(whole, R.stats_from_history(single.history(0, 30), 0, 30, acc, PROBS))
        for r, c in enumerate(ctxs):
            part = c.chain_stats(0, 30, acc, PROBS)
            sl = slice(32 * r, 32 * (r + 1))
            R.assert_stats_equal(part, {k: v[..., sl] for k, v in whole.items()})


def test_stats_between_steps_leave_the_run_untouched(S):
    prob, opts = cm.serial_normal(N=128, T=120, ns=1000)
    a = S.hip_context(prob, opts)
    b = S.hip_context(prob, opts)
    a.step(120)
    b.step_async(40)
    b.chain_stats(0, 40, True, PROBS)       # right after an enqueued persistent step
    b.step(1)
    b.chain_stats(10, 41, False)
    b.step_async(50)
    b.chain_stats(0, 91, False, (0.5,))
    b.step(29)
    cm.assert_history_equal(a.history(), b.history(), exact_floats=True)
    cm.assert_state_equal(a.state(), b.state(), rtol=0)


def test_host_readers_take_the_device_path(S, monkeypatch):
    from collections import OrderedDict
    N, T = 64, 80
    m = S.MProb()
    S.addSampledParam(m, OrderedDict([("p1", [0.2, -3, 3]), ("p2", [-0.2, -20, 20])]))
    S.addMoment(m, {"name": ["mu1", "mu2"], "value": [-1.0, 10.0], "weight": [1.0, 1.0]})
    S.addEvalFunc(m, S.objfunc_norm)
    MA = S.MAlgoBGP(m, {"N": N, "maxiter": T, "maxtemp": 5, "sigma": 0.05, "min_improve": [0.0] * N, "acc_tuners": [2.0] * N})
    S.run(MA)
    h = MA._ctx.history(0, T)
    rows = []
    orig = MA._ctx.history
    monkeypatch.setattr(MA._ctx, "history", lambda t0=0, t1=None: (rows.append(t1 - t0), orig(t0, t1))[1])
    names = S.ps2s_names(m)
    for c in MA.chains:
        j = c._j
        sel = h.accepted[:, j].astype(bool)
        ps = {k: h.params[sel, i, j] for i, k in enumerate(names)}
        assert S.mean(c) == {k: float(np.mean(v)) for k, v in ps.items()}
        assert S.median(c) == {k: float(np.median(v)) for k, v in ps.items()}
        ci = S.CI(c)
        for k, v in ps.items():
            assert np.array_equal(ci[k], np.quantile(v, [(1 - 0.95) / 2, 1 - (1 - 0.95) / 2]))
        i = int(np.argmin(h.value[:, j]))
        assert S.best(c) == (float(h.value[i, j]), i + 1)
    assert rows == []
    df = S.summary(MA)
    assert sum(rows) <= 1
    rate = MA._ctx.state().accept_rate
    for j in range(N):
        ex = h.exchanged[:, j]
        ew = ex[ex != 0]
        row = df.iloc[j] if hasattr(df, "iloc") else df[j]
        assert row["id"] == j + 1 and row["acc_rate"] == rate[j]
        assert row["perc_exchanged"] == 100.0 * np.sum(ex != 0) / T
        assert row["exchanged_most_with"] == (int(np.bincount(ew).argmax()) if len(ew) else 0)
        assert row["best_val"] == float(h.best_val[-1, j])
