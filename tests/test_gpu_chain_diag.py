"""smm_get_chain_diag on the device (include/smmhip.h, smm.jl_amd/csrc/smm_diag.hpp): every output equal (array_equal, NaN equal to
NaN) to the numerical contract restated in chain_diag_ref.py over the history downloaded with smm_get_history — for the persistent and
per-iteration forms, the dense and map-reduce objectives, columns past the LDS, crafted histories, a C3-shaped population with groups,
p2p shards — the call leaves the run untouched, bad arguments raise, and host.ess / host.rhat take it instead of the history."""
import ctypes as C

import numpy as np
import pytest

import chain_diag_ref as R
import common as cm

pytestmark = pytest.mark.gpu


def check(h, t0, t1, max_lag=None, n_acf=0, groups=None, hist=None):
    hist = h.history(0, t1) if hist is None else hist
    got = h.chain_diag(t0, t1, max_lag, n_acf, groups)
    with np.errstate(invalid="ignore", divide="ignore"):
        want = R.diag_from_history(hist, t0, t1, max_lag, n_acf, groups)
    R.assert_diag_equal(got, want)
    return got


def test_objfunc_norm_persistent_windows(S):
    prob, opts = cm.serial_normal(N=256, T=300)
    h = S.hip_context(prob, opts)
    h.step(300)
    assert h.persistent_info()[1] >= 1
    hist = h.history(0, 300)
    assert (hist.exchanged[:57] != 0).any() and (hist.accepted[:57] == 0).any()
    groups = np.arange(256) % 5 - 1
    got = check(h, 0, 300, n_acf=20, groups=groups, hist=hist)
    assert (got["status"] <= 1).any()
    check(h, 57, 213, hist=hist)
    check(h, 57, 213, max_lag=9, n_acf=10, groups=groups, hist=hist)
    check(h, 296, 300, max_lag=1, n_acf=2, hist=hist)
    # the value series is curr_val
    X, _ = R.series_from_history(hist, 0, 300)
    assert np.array_equal(X[-1], hist.curr_val.T)


def test_a_per_iteration_kernel_context(S):
    prob, opts = cm.serial_normal(N=128, T=120, ns=1000)
    h = S.hip_context(prob, opts)
    h.set_persistent(False)
    h.step(120)
    check(h, 0, 120, n_acf=5, groups=np.arange(128) // 16)
    check(h, 33, 120, max_lag=40)


def test_dense2_np50_and_a_map_reduce_user_objective(S):
    from user_objective_src import PANEL_SOURCE
    from test_user_objective import panel_problem
    from smm_jl_amd.workloads import build_problem
    prob, opts = build_problem("c5", 32, 32, 0, 60, 0)   # SMM_OBJ_DENSE2, np = nm = 50
    assert prob.objective_id == S._abi.SMM_OBJ_DENSE2 and prob.np == 50
    h = S.hip_context(prob, opts)
    h.step(60)
    got = check(h, 0, 60, n_acf=12, groups=np.arange(32) // 8)
    assert got["acf"].shape == (12, 51, 32)
    check(h, 7, 41, max_lag=20, n_acf=21)
    prob, opts = panel_problem(S, S.register_user_objective(PANEL_SOURCE, n_sums=3, lanes=64), N=32, T=40)
    h = S.hip_context(prob, opts)
    h.step(40)
    check(h, 0, 40, n_acf=4, groups=np.arange(32) % 2)
    check(h, 5, 40)


def test_columns_longer_than_the_lds(S):
    prob, opts = cm.serial_normal(N=64, T=20000, ns=500)
    h = S.hip_context(prob, opts)
    h.step(20000)
    hist = h.history(0, 20000)
    check(h, 0, 20000, n_acf=3, groups=np.arange(64) // 8, hist=hist)
    check(h, 1500, 18000, hist=hist)          # 16500 > 2 x 8192: three chunks per lag
    check(h, 11000, 19193, max_lag=300, n_acf=301, hist=hist)


def test_crafted_histories(S):
    N, T = 16, 60
    prob, opts = cm.serial_normal(N=N, T=T, ns=100)
    h = S.hip_context(prob, opts)
    h.step(T)
    st = h.state()
    c = h.history(0, T)
    rng = np.random.default_rng(4)
    c.accepted[:, 0] = 0                        # chain 0: no accepted row before the window start 20, one inside it
    c.accepted[30, 0] = 1
    c.accepted[:, 1] = 0                        # chain 1: frozen in the window (its state from row 10)
    c.accepted[10, 1] = 1
    c.accepted[:, 2] = 0                        # chain 2: never accepted
    c.value[25, 3] = np.nan                     # chain 3: a non-finite value in the window's state
    c.accepted[25, 3] = 1
    c.params[40, 1, 4] = np.inf                 # chain 4: an infinite parameter
    c.accepted[40, 4] = 1
    c.exchanged[:, 5] = 3                       # chain 5: every iteration exchanged: accept rate NaN
    c.params[:, :, 6] = rng.standard_normal((T, prob.np))
    c.accepted[:, 6] = 1
    st.iter = T
    h.set_state(st, c)
    back = h.history(0, T)
    groups = np.array([0, 0, 1, 2, 2, 3, 3, -1, 4, 4, 4, 4, 5, -1, 5, 5])
    for t0, t1 in ((20, T), (0, T), (31, 50)):
        got = check(h, t0, t1, n_acf=6, groups=groups, hist=back)
    got = h.chain_diag(20, T, None, 4, groups)
    assert (got["status"][:, 0] == 3).all() and (got["status"][:, 2] == 3).all()
    assert (got["status"][:, 1] != 3).all()          # (a frozen chain: acov_0 is what rounding leaves of d = x - mean)
    assert got["status"][-1, 3] == 3 and got["status"][1, 4] == 3 and got["status"][0, 4] != 3
    assert np.isnan(got["accept_rate"][5])
    assert np.isnan(got["rhat"][1]).all() and np.isnan(got["rhat"][0]).all()


def test_a_c3_population_with_groups(S):
    from smm_jl_amd.workloads import build_problem
    N, T = 256, 400
    prob, opts = build_problem("c3", N, N, 0, T, 0)   # 8 levels x 32 replicas, chain = level * 32 + r
    h = S.hip_context(prob, opts)
    h.step(T)
    level = np.arange(N) // 32
    groups = level.copy()
    groups[level == 3] = -1                         # a level left out
    groups[5 * 32] = 8                              # a one-chain group
    got = check(h, 100, T, groups=groups, n_acf=2)
    assert got["rhat"].shape == (9, 3) and np.isnan(got["rhat"][3]).all()
    assert np.isfinite(got["rhat"][0]).all()


def test_p2p_shards_report_their_slice(S):
    from test_gpu_p2p import p2p_contexts, p2p_run_lockstep
    prob, opts = cm.serial_normal(N=64, T=40, ns=1000)
    single = S.hip_context(prob, opts)
    single.step(40)
    ctxs = p2p_contexts(S, prob, opts, 2)
    p2p_run_lockstep(ctxs, 40)
    whole = check(single, 3, 40, n_acf=7)
    for r, c in enumerate(ctxs):
        part = c.chain_diag(3, 40, None, 7)
        sl = slice(32 * r, 32 * (r + 1))
        R.assert_diag_equal(part, {k: v[..., sl] for k, v in whole.items() if k != "rhat"})
        g = np.arange(32) // 4
        R.assert_diag_equal(c.chain_diag(3, 40, None, 0, g), R.diag_from_history(c.history(0, 40), 3, 40, None, 0, g))


def test_diag_between_steps_leaves_the_run_untouched(S):
    prob, opts = cm.serial_normal(N=128, T=120, ns=1000)
    a = S.hip_context(prob, opts)
    b = S.hip_context(prob, opts)
    a.step(120)
    b.step_async(40)
    b.chain_diag(0, 40, None, 3, np.arange(128) % 4)   # right after an enqueued persistent step
    b.step(1)
    b.chain_diag(10, 41)
    b.step_async(50)
    b.chain_diag(0, 91, 30, 31)
    b.step(29)
    cm.assert_history_equal(a.history(), b.history(), exact_floats=True)
    cm.assert_state_equal(a.state(), b.state(), rtol=0)


def test_invalid_arguments_raise(S):
    A = S._abi
    prob, opts = cm.serial_normal(N=16, T=30, ns=100)
    h = S.hip_context(prob, opts)
    h.step(20)
    g = np.zeros(16, np.int32)
    bad = [dict(t0=-1, t1=10), dict(t0=0, t1=21), dict(t0=5, t1=8), dict(t0=0, t1=20, max_lag=0), dict(t0=0, t1=20, max_lag=20),
           dict(t0=0, t1=20, max_lag=5, n_acf=7), dict(t0=0, t1=20, n_acf=-1), dict(t0=0, t1=20, groups=np.full(16, -2)),
           dict(t0=0, t1=20, groups=np.r_[np.zeros(15), 7][:16] * 0 - 3)]
    for kw in bad:
        with pytest.raises(S.SMMHipError):
            h.chain_diag(**kw)
    fn = h._fn("get_chain_diag")
    out = A.smm_chain_diag_t()
    r = np.empty((1, 3))
    assert fn(None, 0, 20, 19, 0, None, 0, C.byref(out)) == A.SMM_ERR_INVALID_ARG
    assert fn(h._ctx, 0, 20, 19, 0, None, 0, None) == A.SMM_ERR_INVALID_ARG
    assert fn(h._ctx, 0, 20, 19, 0, None, 1, C.byref(out)) == A.SMM_ERR_INVALID_ARG        # group NULL with n_groups > 0
    assert fn(h._ctx, 0, 20, 19, 0, g.ctypes.data_as(A.c_int32_p), -1, C.byref(out)) == A.SMM_ERR_INVALID_ARG
    g1 = g.copy(); g1[3] = 1
    assert fn(h._ctx, 0, 20, 19, 0, g1.ctypes.data_as(A.c_int32_p), 1, C.byref(out)) == A.SMM_ERR_INVALID_ARG   # id >= n_groups
    out.rhat = r.ctypes.data_as(A.c_double_p)
    assert fn(h._ctx, 0, 20, 19, 0, None, 0, C.byref(out)) == A.SMM_ERR_INVALID_ARG        # rhat without groups
    out.rhat = None
    assert fn(h._ctx, 0, 20, 19, 20, None, 0, C.byref(out)) == A.SMM_OK                   # (nothing requested: valid)
    assert fn(h._ctx, 16, 20, 3, 4, None, 0, C.byref(out)) == A.SMM_OK
    h.step(10)                                                                               # the context still runs
    assert h.state().iter == 30


def test_host_readers_take_the_device_path(S, monkeypatch):
    from collections import OrderedDict
    N, T = 64, 150
    m = S.MProb()
    S.addSampledParam(m, OrderedDict([("p1", [0.2, -3, 3]), ("p2", [-0.2, -20, 20])]))
    S.addMoment(m, {"name": ["mu1", "mu2"], "value": [-1.0, 10.0], "weight": [1.0, 1.0]})
    S.addEvalFunc(m, S.objfunc_norm)
    tuners = np.repeat([4.0, 2.0, 1.0, 0.5], 16)
    MA = S.MAlgoBGP(m, {"N": N, "maxiter": T, "maxtemp": 5, "sigma": 0.05, "min_improve": [0.0] * N, "acc_tuners": list(tuners)})
    S.run(MA)
    h = MA._ctx.history(0, T)
    calls = []
    orig = MA._ctx.history
    monkeypatch.setattr(MA._ctx, "history", lambda t0=0, t1=None: (calls.append((t0, t1)), orig(t0, t1))[1])
    names = S.ps2s_names(m)
    groups = np.repeat(np.arange(4), 16)
    want = R.diag_from_history(h, 0, T, None, 0, groups)
    want_w = R.diag_from_history(h, 40, T, None, 0, None)
    for c in MA.chains:
        e = S.ess(c)
        assert list(e) == names
        assert np.array_equal([e[k] for k in names], want["ess"][:2, c._j], equal_nan=True)
        e = S.ess(c, window=(40, T))
        assert np.array_equal([e[k] for k in names], want_w["ess"][:2, c._j], equal_nan=True)
    rh = S.rhat(MA)
    assert len(rh) == 4 and all(list(d) == names for d in rh)
    assert np.array_equal([[d[k] for k in names] for d in rh], want["rhat"][:, :2], equal_nan=True)
    g2 = np.arange(N) % 3
    rh2 = S.rhat(MA, groups=g2, window=(10, T))
    w2 = R.diag_from_history(h, 10, T, None, 0, g2)
    assert np.array_equal([[d[k] for k in names] for d in rh2], w2["rhat"][:, :2], equal_nan=True)
    assert calls == []
