"""adjust_ref.py, the restatement of smm_get_adjustment's numerical contract (include/smmhip.h), held against what it must reproduce
without a GPU: the linear-Gaussian case where the adjustment recovers the posterior mean at the data and beta is np.linalg.lstsq's on
the weighted centred design; the identities that hold exactly (the uniform kernel's sums, tol = 1, the weighted quantile with equal
weights and on a tie run, n_outside counted by hand); and the status table on crafted histories."""
import math

import numpy as np

import adjust_ref as AR
from smm_jl_amd import _abi as A


def crafted(theta, mom, accepted=None):
    """a HistoryBuffers from params theta [T][np][N] and sim_moments mom [T][nm][N] (accepted [T][N], default every row)"""
    T, npar, N = theta.shape
    h = A.HistoryBuffers(T, N, npar, mom.shape[1])
    for f in A.HistoryBuffers.FIELDS:
        getattr(h, f)[...] = 0
    h.params[...], h.sim_moments[...] = theta, mom
    h.accepted[...] = 1 if accepted is None else accepted
    return h


def adjust(h, mom, select=0, groups=None, tol=0.2, kernel=1, scale=None, ridge=0.0, probs=(), w=None, lb=None, ub=None, n_groups=None,
           window=None):
    npar, nm = h.params.shape[1], h.sim_moments.shape[1]
    t0, t1 = window or (0, h.value.shape[0])
    return AR.adjustment_from_history(h, t0, t1, select, groups, tol, kernel, scale, ridge, probs, mom, np.ones(nm) if w is None else w,
                                      -np.ones(npar) if lb is None else lb, np.ones(npar) if ub is None else ub, n_groups=n_groups)


def linear_gaussian(seed=11, T=600, N=4):
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((3, 2))
    theta = rng.uniform(-1.0, 1.0, (T, 2, N))
    mom = np.einsum("kj,tjc->tkc", B, theta) + 0.01 * rng.standard_normal((T, 3, N))
    theta0 = np.array([0.3, -0.2])
    return crafted(theta, mom), B @ theta0, theta0


def test_linear_gaussian_recovery_and_beta_against_lstsq():
    """s = B theta + small noise, theta uniform: the intercept of the regression lies closer to the theta behind s_obs than the
    weighted mean of the kept draws, for both kernels; beta agrees with np.linalg.lstsq on the r-scaled centred design.  Measured on
    the CPU: the largest relative deviation of beta (in units of its largest entry) is 5.88e-14 over the two kernels (5.58e-14 uniform,
    5.88e-14 Epanechnikov), recorded as adjust_ref.ADJUST_LSTSQ_DEV; the test holds ten times that, as the two differ only in the
    order of the sums and in the solver."""
    h, s_obs, theta0 = linear_gaussian()
    worst = 0.0
    for kernel in (0, 1):
        r = adjust(h, s_obs, kernel=kernel, tol=0.2, probs=(0.5,))
        assert r["status"].tolist() == [0]
        raw, adj = np.abs(r["raw_mean"][0] - theta0).max(), np.abs(r["adj_mean"][0] - theta0).max()
        print("kernel", kernel, "raw error", raw, "adjusted error", adj)
        assert adj < raw and adj < 5e-3
        assert np.abs(r["adj_quantile"][0, 0] - theta0).max() < 5e-3 and (r["adj_sd"][0] < 0.02).all()
        x = (h.sim_moments.transpose(1, 2, 0).reshape(3, -1) - s_obs[:, None])     # (members in order, each in iteration order)
        th = h.params.transpose(1, 2, 0).reshape(2, -1)
        om = AR.row_weights(AR.distances(x), r["bandwidth"][0], kernel)
        rr = np.sqrt(om)
        Ex = (rr * (x - r["x_mean"][0][:, None])).T
        Et = (rr * (th - r["raw_mean"][0][:, None])).T
        ls = np.linalg.lstsq(Ex, Et, rcond=None)[0]
        dev = np.abs(ls - r["beta"][0]).max() / np.abs(ls).max()
        print("kernel", kernel, "beta against lstsq", dev)
        worst = max(worst, dev)
    print("largest relative deviation", worst)
    assert worst <= AR.ADJUST_LSTSQ_RTOL


def test_uniform_kernel_sums_and_tol_one_keep_every_row():
    h, s_obs, _ = linear_gaussian(seed=5, T=300)
    for tol in (0.1, 0.37, 1.0):
        r = adjust(h, s_obs, kernel=0, tol=tol)
        assert r["ess"][0] == r["n_kept"][0] == r["sum_w"][0]
        if tol == 1.0:
            assert r["n_kept"][0] == r["count"][0] == 1200
    r = adjust(h, s_obs, kernel=1, tol=0.37)
    assert 0 < r["ess"][0] < r["n_kept"][0] and r["sum_w"][0] < r["n_kept"][0] < 0.37 * 1200 + 1


def test_weighted_quantile_with_equal_weights_and_on_a_tie_run():
    rng = np.random.default_rng(2)
    for n in (1, 2, 7, 64):
        v = rng.standard_normal(n)
        s = np.sort(v)
        for q0 in (1, 1048576):
            q = np.full(n, q0, np.int64)
            for p in (0.0, 0.025, 0.3, 0.5, 0.975, 1.0):
                assert AR.weighted_quantile(v, q, p) == s[max(1, math.ceil(p * n)) - 1], (n, q0, p)
    v = np.array([0.5, -1.0, 0.25, 0.25, 0.25, 0.25, 3.0, 0.25])
    q = np.array([3, 1, 2, 5, 0, 7, 2, 1], np.int64)           # Q = 21; below the run 1, through it 16
    for p, want in ((0.0, -1.0), (1 / 21, -1.0), (0.06, 0.25), (0.5, 0.25), (16 / 21, 0.25), (0.8, 0.5), (0.9, 0.5), (0.91, 3.0), (1.0, 3.0)):
        assert AR.weighted_quantile(v, q, p) == want, p
    assert AR.int_weights(np.array([0.0, 2.0 ** -60, 2.0 ** -20, 0.5, 1.0])).tolist() == [0, 1, 1, 524288, 1048576]


def test_n_outside_counted_by_hand_on_six_rows():
    """one moment, one parameter, data at s_obs = 0.5, unit scale, uniform kernel, tol = 1.  The discrepancies are x = (-1, -1, 0, 0, 1,
    1): mean 0, C_xx = 4, whose factor is 2.  theta = 2 s + n with n = (0.5, -0.5, 0.25, -0.25, 1, -1), which sums to 0 and is orthogonal
    to x, so C_x,theta = 8 and beta = (8 / 2) / 2 = 2, every step exact in binary.  The adjusted draws are theta - 2 x = 1 + n =
    (1.5, 0.5, 1.25, 0.75, 2, 0).  Against [lb, ub] = [0.25, 1.25]: 1.5 and 2 lie above, 0 below, 1.25 sits on the bound and stays
    inside: three rows outside."""
    x = np.array([-1.0, -1.0, 0.0, 0.0, 1.0, 1.0])
    n = np.array([0.5, -0.5, 0.25, -0.25, 1.0, -1.0])
    s = x + 0.5
    theta = 2 * s + n
    h = crafted(theta[:, None, None], s[:, None, None])
    r = adjust(h, np.array([0.5]), kernel=0, tol=1.0, probs=(0.0, 0.5, 1.0), lb=np.array([0.25]), ub=np.array([1.25]))
    assert r["status"].tolist() == [0] and r["n_kept"].tolist() == [6]
    assert r["beta"].tolist() == [[[2.0]]] and r["x_mean"].tolist() == [[0.0]] and r["raw_mean"].tolist() == [[1.0]]
    assert r["adj_mean"].tolist() == [[1.0]]
    assert r["n_outside"].tolist() == [[3]]
    assert r["adj_quantile"][:, 0, 0].tolist() == [0.0, 0.75, 2.0]


def test_status_table_on_crafted_histories():
    rng = np.random.default_rng(8)
    T, N = 30, 3
    theta = rng.uniform(-1, 1, (T, 2, N))
    mom = np.stack([theta[:, 0] + theta[:, 1], theta[:, 0] - theta[:, 1]], axis=1) + 0.01 * rng.standard_normal((T, 2, N))
    s_obs = np.array([0.1, 0.2])
    g = np.array([0, 1, 2], np.int32)
    h = crafted(theta, mom)
    h.sim_moments[4, 1, 1] = np.inf
    r = adjust(h, s_obs, groups=g, n_groups=5, probs=(0.5,))
    assert r["status"].tolist() == [0, 2, 0, 1, 1] and r["count"].tolist() == [30, 30, 30, 0, 0]
    assert np.isnan(r["bandwidth"][1]) and np.isnan(r["raw_mean"][1]).all() and r["n_kept"][1] == 0 and (r["n_outside"][1] == 0).all()
    assert np.isnan(r["adj_quantile"][:, 3]).all() and np.isfinite(r["adj_quantile"][:, 0]).all()
    r = adjust(h, s_obs, groups=g, window=(3, 4))               # one row: status 1 before the non-finite value is looked for
    assert r["status"].tolist() == [1, 1, 1] and r["count"].tolist() == [1, 1, 1] and np.isnan(r["sum_w"]).all()
    r = adjust(h, s_obs, groups=g, window=(9, 9))               # an empty window
    assert r["status"].tolist() == [1, 1, 1] and r["count"].tolist() == [0, 0, 0]
    # status 3: too few kept rows (nm + 2 = 4 are needed; tol 0.1 of 30 rows keeps 3 under the uniform kernel) ...
    r = adjust(h, s_obs, groups=g, kernel=0, tol=0.1)
    assert r["status"].tolist() == [3, 2, 3] and r["n_kept"][0] == 3 and r["sum_w"][0] == 3.0
    assert np.isfinite(r["raw_mean"][0]).all() and np.isfinite(r["bandwidth"][0]) and np.isnan(r["beta"][0]).all() and np.isnan(r["adj_sd"][0]).all()
    # ... and Epanechnikov's kernel at a bandwidth of zero: more than tol of the rows sit on the data
    h0 = crafted(theta, mom)
    h0.sim_moments[:20, :, 0] = s_obs[None, :, None][..., 0]
    r = adjust(h0, s_obs, groups=g, kernel=1, tol=0.5)
    assert r["status"].tolist() == [3, 0, 0] and r["bandwidth"][0] == 0.0 and r["n_kept"][0] == 0 and r["sum_w"][0] == 0.0
    assert np.isnan(r["ess"][0]) and np.isnan(r["raw_mean"][0]).all()
    r = adjust(h0, s_obs, groups=g, kernel=0, tol=0.5)          # the uniform kernel keeps the rows at distance 0: a singular design
    assert r["bandwidth"][0] == 0.0 and r["n_kept"][0] == 20 and r["status"][0] == 4
    # status 4: two moments that are the same column, in values whose sums are exact (C = 16 in every entry of the block: the second
    # pivot is 16 - 4 * 4); a ridge makes the factor go through
    col = AR.COLLINEAR_COLUMN
    hc = crafted(rng.uniform(-1, 1, (32, 2, N)), np.broadcast_to(col[:, None, None], (32, 2, N)).copy())
    r = adjust(hc, np.zeros(2), groups=g, kernel=0, tol=1.0)
    assert r["status"].tolist() == [4, 4, 4] and np.isfinite(r["raw_mean"]).all() and np.isnan(r["beta"]).all()
    assert np.isnan(r["adj_mean"]).all() and (r["n_outside"] == 0).all() and (r["n_kept"] == 32).all()
    r = adjust(hc, np.zeros(2), groups=g, kernel=0, tol=1.0, ridge=1e-6, probs=(0.5,))
    assert r["status"].tolist() == [0, 0, 0] and np.isfinite(r["beta"]).all() and np.isfinite(r["adj_quantile"]).all()


def test_scale_and_selections_reach_the_rows_moment_stats_ref_selects():
    """the scale divides the discrepancy (a given scale equal to the weights changes nothing; another one changes the bandwidth), and
    the three selections pool moment_stats_ref's rows"""
    import moment_stats_ref as MR
    h, _ = MR.crafted_linear(2, 3, 4, 50, seed=3)
    mom, w = np.array([0.1, -0.2, 0.3]), np.array([0.5, 2.0, np.nan])
    base = adjust(h, mom, select=2, w=w, probs=(0.25,), lb=-3 * np.ones(2), ub=3 * np.ones(2))
    same = adjust(h, mom, select=2, w=w, scale=np.array([0.5, 2.0, 1.0]), probs=(0.25,), lb=-3 * np.ones(2), ub=3 * np.ones(2))
    AR.assert_adjustment_equal(base, same)
    other = adjust(h, mom, select=2, w=w, scale=np.array([1.0, 1.0, 1.0]))
    assert other["bandwidth"][0] != base["bandwidth"][0]
    counts = [adjust(h, mom, select=s)["count"][0] for s in (0, 1, 2)]
    assert counts[0] == counts[2] == 200 and counts[1] == int((h.accepted != 0).sum())
