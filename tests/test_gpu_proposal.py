"""Proposal factors adapted from each chain's own history on the device (smm_get_chain_cov, smm_get_proposal, smm_set_proposal,
smm_adapt_proposal; include/smmhip.h): the device against the numpy restatement of the contract (tests/chain_cov_ref.py) bit for bit,
continuation parity against the oracle, shards, refusals and ordering, the host layer, and one statistical sanity check."""
import numpy as np
import pytest

import chain_cov_ref as CR
import common as cm
from smm_jl_amd import _abi as A
from test_gpu_p2p import p2p_contexts, p2p_run_lockstep

pytestmark = pytest.mark.gpu


def ref_cov(ctx, hh, t0, t1, accepted_only, unit_space):
    p = ctx.problem
    kw = dict(lb=p.lb, ub=p.ub) if unit_space else {}
    return CR.chain_cov(hh.params, hh.accepted, t0, t1, accepted_only, **kw)


def assert_cov_equal(got, want):
    for g, w in zip(got, want):
        assert np.array_equal(g, w, equal_nan=True)


def eye_factors(N, npar):
    return np.ascontiguousarray(np.broadcast_to(np.eye(npar), (N, npar, npar)))


def dense50(N, T):
    from smm_jl_amd import BGPOpts, Problem
    rng = np.random.default_rng(3)
    npar = 50
    prob = Problem(init=rng.uniform(-0.3, 0.3, npar), lb=-np.ones(npar), ub=np.ones(npar), mom=rng.uniform(-0.5, 0.5, npar),
                   w=rng.uniform(0.5, 2.0, npar), ns=1, objective_id=A.SMM_OBJ_DENSE)
    opts = BGPOpts(N=N, maxiter=T, sigma=0.02 * cm.temps(N, 4), acc_tuner=np.geomspace(20, 1, N), min_improve=np.zeros(N), seed=3)
    return prob, opts


def snapshot(src):
    """src's state and history now, for restore()"""
    return src.state(), src.history()


def restore(dst, snap):
    """dst continues from a snapshot (smm_set_state)"""
    dst.set_state(*snap)


@pytest.mark.parametrize("which", ["general6", "dense50"])
def test_chain_cov_matches_restatement(S, which):
    prob, opts = cm.general_normal(6, N=48, T=60, ns=200) if which == "general6" else dense50(N=40, T=120)
    h = S.hip_context(prob, opts)
    h.step(opts.maxiter)
    T = opts.maxiter
    hh = h.history()
    st0 = h.chain_stats(0, T, True, (0.1, 0.9))
    for acc in (True, False):
        for unit in (False, True):
            for (t0, t1) in ((0, T), (7, 7), (5, 6), (T // 3, T)):
                assert_cov_equal(h.chain_cov(t0, t1, acc, unit), ref_cov(h, hh, t0, t1, acc, unit))
    count, _, cov = h.chain_cov(5, 6, False, True)
    assert (count == 1).all() and np.isnan(cov).all()
    count, mean, cov = h.chain_cov(7, 7)
    assert (count == 0).all() and np.isnan(mean).all() and np.isnan(cov).all()
    cm.assert_history_equal(h.history(), hh, rtol=0, atol=0)   # read-only
    st1 = h.chain_stats(0, T, True, (0.1, 0.9))
    for k in st0:
        assert np.array_equal(st0[k], st1[k], equal_nan=True), k


def test_chain_cov_long_columns_and_nan(S):
    prob, opts = cm.serial_normal(N=4, T=8300, ns=50)
    h = S.hip_context(prob, opts)
    h.step(8300)
    hh = h.history()
    for acc in (False, True):
        assert_cov_equal(h.chain_cov(0, 8300, acc, True), ref_cov(h, hh, 0, 8300, acc, True))
    assert (h.chain_cov(0, 8300, False)[0] == 8300).all()
    # a NaN among one chain's draws, uploaded through smm_set_state
    prob, opts = cm.general_normal(5, N=16, T=30, ns=100)
    h = S.hip_context(prob, opts)
    h.step(30)
    s, hh = h.state(), h.history()
    hh.params[4, 2, 3] = np.nan
    hh.accepted[4, 3] = 1
    h.set_state(s, hh)
    for unit in (False, True):
        got = h.chain_cov(0, 30, True, unit)
        assert_cov_equal(got, ref_cov(h, hh, 0, 30, True, unit))
        assert np.isnan(got[2][2, :, 3]).all() and not np.isnan(got[2][:, :, 0]).any()


def test_adapt_matches_restatement_and_statuses(S):
    N, npar, T = 48, 6, 80
    prob, opts = cm.general_normal(npar, N=N, T=T, ns=200)
    opts.chol_L = eye_factors(N, npar)
    h = S.hip_context(prob, opts)
    h.step(T)
    hh = h.history()
    st = h.adapt_proposal(10, T, ridge=1e-9)
    count, _, cov = ref_cov(h, hh, 10, T, True, True)
    L, want = CR.adapt(count, cov, npar + 1, True, 1e-9)
    assert np.array_equal(st, want) and (st == 0).sum() >= 4
    got = h.proposal()
    for c in range(N):
        assert np.array_equal(got[c], L[c] if st[c] == 0 else np.eye(npar)), c
    # status 1: a window too short; the factors stay as they are, bit for bit
    before = h.proposal()
    st = h.adapt_proposal(T - 3, T)
    assert (st == 1).all() and np.array_equal(h.proposal(), before)
    # status 3: a parameter that never moves in one chain's history (uploaded), no ridge
    s = h.state()
    hh.params[:, 3, 5] = hh.params[0, 3, 5]
    h.set_state(s, hh)
    st = h.adapt_proposal(10, T, accepted_only=False, ridge=0.0)
    count, _, cov = ref_cov(h, hh, 10, T, False, True)
    L, want = CR.adapt(count, cov, npar + 1, True, 0.0)
    assert st[5] == 3 and np.array_equal(st, want)
    got = h.proposal()
    assert np.array_equal(got[5], before[5])
    for c in np.flatnonzero(st == 0):
        assert np.array_equal(got[c], L[c])


def test_adapt_dense50_matches_restatement(S):
    N, T = 24, 120
    prob, opts = dense50(N, T)
    opts.chol_L = eye_factors(N, 50)
    opts.smpl_iters = 100000
    h = S.hip_context(prob, opts)
    h.step(T)
    hh = h.history()
    st = h.adapt_proposal(0, T, accepted_only=False)
    count, _, cov = ref_cov(h, hh, 0, T, False, True)
    L, want = CR.adapt(count, cov, 51, True, 1e-8)
    assert np.array_equal(st, want)
    got = h.proposal()
    for c in range(N):
        assert np.array_equal(got[c], L[c] if st[c] == 0 else np.eye(50))


def test_dense50_multi_leaf_columns(S):
    # np = 50 (28 tiles of pairs) with a few hundred draws per chain: several leaves of the pairwise tree, combines, and more than one
    # staged run of COV_G draws per tile
    N, T = 16, 700
    prob, opts = dense50(N, T)
    opts.chol_L = eye_factors(N, 50)
    opts.smpl_iters = 100000
    opts.sigma_update_steps = 10 ** 6
    h = S.hip_context(prob, opts)
    h.step(T)
    hh = h.history()
    for acc in (False, True):
        assert_cov_equal(h.chain_cov(0, T, acc, True), ref_cov(h, hh, 0, T, acc, True))
    assert_cov_equal(h.chain_cov(100, T, False, False), ref_cov(h, hh, 100, T, False, False))
    st = h.adapt_proposal(0, T, accepted_only=False)
    count, _, cov = ref_cov(h, hh, 0, T, False, True)
    L, want = CR.adapt(count, cov, 51, True, 1e-8)
    assert np.array_equal(st, want) and (st == 0).any()
    got = h.proposal()
    for c in range(N):
        assert np.array_equal(got[c], L[c] if st[c] == 0 else np.eye(50))


def test_factor_layout_is_fixed_at_creation(S):
    # the caller's opts may be reused for other contexts after creation: the buffers follow the context, not the opts
    N, npar = 12, 4
    prob, opts = cm.general_normal(npar, N=N, T=10, ns=100)
    opts.chol_L = eye_factors(N, npar)
    h = S.hip_context(prob, opts)
    opts.chol_L = np.eye(npar)
    assert h.proposal().shape == (N, npar, npar)
    with pytest.raises(ValueError):
        h.set_proposal(np.eye(npar))
    opts.chol_L = None
    assert h.proposal().shape == (N, npar, npar)
    h.set_proposal(2.0 * eye_factors(N, npar))
    assert np.array_equal(h.proposal(), 2.0 * eye_factors(N, npar))


def test_adapted_run_continues_as_the_oracle(S, O):
    N, npar, T1, K = 40, 6, 40, 20
    prob, opts = cm.general_normal(npar, N=N, T=T1 + K, ns=200)
    opts.chol_L = eye_factors(N, npar)
    opts.smpl_iters = 100000
    h = S.hip_context(prob, opts)
    h.step(T1)
    st = h.adapt_proposal(5, T1, min_draws=3)
    assert (st == 0).sum() >= 4
    L = h.proposal()
    snap = snapshot(h)
    h.step(K)
    opts.chol_L = np.ascontiguousarray(L)
    o = O.OracleContext(prob, opts, S.Tables(Z=h.Z()))
    restore(o, snap)
    o.step(K)
    cm.assert_history_equal(h.history(T1, T1 + K), o.history(T1, T1 + K))
    cm.assert_state_equal(h.state(), o.state())
    # a device context created with the adapted factors and restored the same way
    h2 = S.hip_context(prob, opts)
    restore(h2, snap)
    h2.step(K)
    cm.assert_history_equal(h2.history(), h.history(), rtol=0, atol=0)


@pytest.mark.parametrize("per_chain", [False, True])
def test_set_proposal_continues_as_the_oracle(S, O, per_chain):
    N, npar, T1, K = 32, 5, 25, 15
    rng = np.random.default_rng(11)
    prob, opts = cm.general_normal(npar, N=N, T=T1 + K, ns=200)
    opts.smpl_iters = 100000

    def rchol():
        M = rng.standard_normal((npar, npar))
        return np.linalg.cholesky(M @ M.T / npar + 0.5 * np.eye(npar))

    opts.chol_L = eye_factors(N, npar) if per_chain else np.eye(npar)
    h = S.hip_context(prob, opts)
    h.step(T1)
    L = np.stack([rchol() for _ in range(N)]) if per_chain else rchol()
    junk = L.copy()
    junk[..., 0, 1] = 1e300   # above the diagonal: ignored
    h.set_proposal(junk)
    assert np.array_equal(h.proposal(), L)
    snap = snapshot(h)
    h.step(K)
    opts.chol_L = np.ascontiguousarray(L)
    o = O.OracleContext(prob, opts, S.Tables(Z=h.Z()))
    restore(o, snap)
    o.step(K)
    cm.assert_history_equal(h.history(T1, T1 + K), o.history(T1, T1 + K))
    cm.assert_state_equal(h.state(), o.state())


def test_shards_adapt_their_own_chains(S):
    G, N, npar, T1, K = 2, 64, 4, 30, 12
    prob, opts = cm.general_normal(npar, N=N, T=T1 + K, ns=200)
    opts.chol_L = eye_factors(N, npar)
    one = S.hip_context(prob, opts)
    one.step(T1)
    st1 = one.adapt_proposal(0, T1, min_draws=3)
    one.step(K)
    ctxs = p2p_contexts(S, prob, opts, G)
    p2p_run_lockstep(ctxs, T1)
    sts = [c.adapt_proposal(0, T1, min_draws=3) for c in ctxs]
    assert np.array_equal(np.concatenate(sts), st1)
    assert np.array_equal(np.concatenate([c.proposal() for c in ctxs]), one.proposal())
    for c in ctxs:
        assert c.proposal().shape == (N // G, npar, npar)
    p2p_run_lockstep(ctxs, K)
    hs = [c.history() for c in ctxs]
    ho = one.history()
    for f in ("value", "params", "accepted", "exchanged"):
        got = np.concatenate([getattr(x, f) for x in hs], axis=-1)
        assert np.array_equal(got, getattr(ho, f)), f


def test_refusals_and_ordering(S):
    N, npar, T = 16, 4, 30
    prob, opts = cm.general_normal(npar, N=N, T=T, ns=100)
    plain = S.hip_context(prob, opts)
    plain.step(5)
    for call in (lambda: plain.proposal(), lambda: plain.set_proposal(np.eye(npar)), lambda: plain.adapt_proposal(0, 5)):
        with pytest.raises(A.SMMHipError) as e:
            call()
        assert e.value.code == A.SMM_ERR_INVALID_ARG and "chol_L" in str(e.value)
    opts.chol_L = np.eye(npar)
    shared = S.hip_context(prob, opts)
    shared.step(5)
    with pytest.raises(A.SMMHipError) as e:
        shared.adapt_proposal(0, 5)
    assert e.value.code == A.SMM_ERR_INVALID_ARG and "chol_per_chain" in str(e.value)
    opts.chol_L = eye_factors(N, npar)
    h = S.hip_context(prob, opts)
    h.step(10)
    before = h.proposal()
    bad = [lambda: h.adapt_proposal(0, 11), lambda: h.adapt_proposal(5, 4), lambda: h.chain_cov(-1, 3),
           lambda: h.adapt_proposal(0, 10, min_draws=1), lambda: h.adapt_proposal(0, 10, ridge=-1.0),
           lambda: h.adapt_proposal(0, 10, ridge=np.inf)]
    for L in (np.where(np.eye(npar) > 0, np.nan, 0.0), np.eye(npar) * -1.0, np.diag([1.0, 1.0, 0.0, 1.0])):
        bad.append(lambda L=L: h.set_proposal(np.broadcast_to(L, (N, npar, npar))))
    for call in bad:
        with pytest.raises(A.SMMHipError) as e:
            call()
        assert e.value.code == A.SMM_ERR_INVALID_ARG
    assert np.array_equal(h.proposal(), before)
    # step_async, then adapt: the same as the synchronous sequence
    a = S.hip_context(prob, opts)
    a.step(10)
    a.step_async(20)
    sa = a.adapt_proposal(0, 30, min_draws=3)
    b = S.hip_context(prob, opts)
    b.step(30)
    sb = b.adapt_proposal(0, 30, min_draws=3)
    assert np.array_equal(sa, sb) and np.array_equal(a.proposal(), b.proposal())


def test_pending_hard_error_installs_nothing(S):
    N, npar = 8, 3
    prob, opts = cm.general_normal(npar, N=N, T=20, ns=100)
    opts.chol_L = eye_factors(N, npar)
    opts.smpl_iters = 1
    opts.sigma[:] = 50.0   # every draw leaves [0, 1]: mysample gives up (AlgoBGP.jl:409)
    h = S.hip_context(prob, opts)
    s0 = h.state()
    h.step_async(3)
    for call in (lambda: h.adapt_proposal(0, 0, min_draws=2), lambda: h.set_proposal(eye_factors(N, npar) * 2.0)):
        with pytest.raises(A.SMMHipError) as e:
            call()
        assert e.value.code == A.SMM_ERR_NO_DRAW_IN_SUPPORT
    assert np.array_equal(h.proposal(), eye_factors(N, npar))
    h.set_state(s0, A.HistoryBuffers(0, N, npar, npar))   # the recovery goes through at its first call: the error was told
    h.set_proposal(eye_factors(N, npar) * 2.0)
    assert np.array_equal(h.proposal(), eye_factors(N, npar) * 2.0)


def make_mprob(H):
    from collections import OrderedDict
    m = H.MProb()
    H.addSampledParam(m, OrderedDict([("p1", [0.2, -3, 3]), ("p2", [-0.2, -20, 20])]))
    H.addMoment(m, {"name": ["mu1", "mu2"], "value": [-1.0, 10.0], "weight": [1.0, 1.0]})
    H.addEvalFunc(m, H.objfunc_norm)
    return m


def test_host_layer(S, tmp_path):
    import smm_jl_amd as H
    opts = {"N": 4, "maxiter": 60, "maxtemp": 3, "smpl_iters": 1000, "min_improve": [0.0] * 4, "acc_tuners": [2.0] * 4}
    algo = H.MAlgoBGP(make_mprob(H), dict(opts))
    H.run(algo)
    for c in algo.chains:
        P = np.array(list(H.params(c).values()))
        np.testing.assert_allclose(H.cov(c), np.cov(P, ddof=1), rtol=1e-12, atol=1e-15)
    # "identity": the isotropic kernel bit for bit
    a2 = H.MAlgoBGP(make_mprob(H), dict(opts, chol_L="identity"))
    H.run(a2)
    cm.assert_history_equal(a2._ctx.history(), algo._ctx.history(), rtol=0, atol=0)

    # save -> readMalgo and restart after an adapt equal the uninterrupted run
    def pilot(maxiter):
        a = H.MAlgoBGP(make_mprob(H), dict(opts, maxiter=maxiter, chol_L="identity"))
        for _ in range(30):
            H.computeNextIteration(a)
        st = H.adapt_proposal(a, (5, 30), min_draws=3)
        assert (st == 0).any()
        return a

    full = pilot(60)
    H.run(full)
    p = pilot(60)
    H.save(p, str(tmp_path / "p"))
    q = H.MAlgoBGP(make_mprob(H), dict(opts, chol_L="identity"))
    H.readMalgo(q, str(tmp_path / "p"))
    assert np.array_equal(q._ctx.proposal(), p._ctx.proposal())
    H.run(q)
    cm.assert_history_equal(q._ctx.history(), full._ctx.history(), rtol=0, atol=0)
    r = pilot(30)
    H.restart(r, 30)
    assert r.i == 60
    cm.assert_history_equal(r._ctx.history(), full._ctx.history(), rtol=0, atol=0)


CORR_QUAD = r"""
SMM_USER_OBJECTIVE(const double* theta, int np, const double* mom, const double* w, int nm,
                   const double* udata, int n_udata, double* sim_moments, double* value, int* status)
{
    /* 0.5 x' S^-1 x, S = (1 - rho) I + rho 1 1': along 1 the variance is 1 + (np - 1) rho, across it 1 - rho */
    const double rho = udata[0];
    double s = 0.0, q = 0.0;
    for (int k = 0; k < np; ++k) { s += theta[k]; q += theta[k] * theta[k]; sim_moments[k] = theta[k]; }
    const double along = s * s / np, across = q - along;
    *value = 0.5 * (along / (1.0 + (np - 1) * rho) + across / (1.0 - rho));
    *status = 1;
}
"""


def test_adapted_proposal_moves_further_along_the_long_axis(S):
    from smm_jl_amd import BGPOpts, Problem
    npar, N, T1, K = 6, 8, 400, 400
    oid = S.register_user_objective(CORR_QUAD)

    def ctx():
        prob = Problem(init=np.zeros(npar), lb=-10 * np.ones(npar), ub=10 * np.ones(npar), mom=np.zeros(npar), w=np.ones(npar),
                       ns=1, objective_id=oid, obj_params=[0.99])
        opts = BGPOpts(N=N, maxiter=T1 + K, sigma=0.01 * cm.temps(N, 2.0), acc_tuner=np.ones(N), min_improve=1e30 * np.ones(N),
                       sigma_update_steps=10 ** 6, chol_L=eye_factors(N, npar), seed=5, smpl_iters=100000)
        return S.hip_context(prob, opts)

    def jump(h):
        hh = h.history(T1, T1 + K)
        assert (hh.exchanged[:, 0] == 0).all()
        P = hh.params[:, :, 0]   # the temperature-1 chain
        along = P.sum(axis=1) / np.sqrt(npar)
        return np.mean(np.diff(along) ** 2)

    iso, ad = ctx(), ctx()
    iso.step(T1)
    ad.step(T1)
    st = ad.adapt_proposal(0, T1, accepted_only=False)
    assert st[0] == 0
    iso.step(K)
    ad.step(K)
    assert jump(ad) >= 2.0 * jump(iso), (jump(ad), jump(iso))
