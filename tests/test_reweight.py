"""reweight_ref.py, the restatement of smm_get_reweighted's numerical contract (include/smmhip.h), held without a GPU against the
identities of equal temperatures, a known answer of the estimator and reweight_craft.py's crafted history."""
import numpy as np

import group_stats_ref as GR
import reweight_craft as RC
import reweight_ref as RW
from adjust_craft import zero_history


def random_history(T, N, npar, nm, seed, accept=0.6):
    rng = np.random.default_rng(seed)
    h = zero_history(T, N, npar, nm)
    h.params[...] = rng.uniform(-1.0, 1.0, (T, npar, N))
    h.sim_moments[...] = rng.standard_normal((T, nm, N))
    h.value[...] = rng.uniform(0.0, 3.0, (T, N))
    h.accepted[...] = rng.uniform(size=(T, N)) < accept
    return h


def test_equal_temperatures_at_their_own_target_are_the_plain_pooled_group():
    """d = 0: w = u = 1, so the weighted mean is smm_get_group_stats' mean bit for bit, ess the row count, chain_logz 0 and q 2^20"""
    T, N = 50, 5
    h = random_history(T, N, 3, 2, 1)
    for select, acc_only in ((0, 0), (1, 1)):
        got = RW.reweighted_from_history(h, 4, T, select, None, (0.75,), (0.1, 0.5), np.full(N, 0.75))
        want = GR.group_stats_from_history(h, 4, T, acc_only, None, ())
        assert np.array_equal(got["mean"][0], want["mean"]) and got["count"].tolist() == want["count"].tolist()
        m = int(got["n_scored"][0])
        assert got["status"].tolist() == [[0]] and got["ess"][0, 0] == m and got["sum_u"][0, 0] == m and got["n_kept"][0, 0] == m
        assert (got["chain_logz"] == 0.0).all() and np.array_equal(got["chain_ess"][0], got["chain_n"].astype(float))
        # the population covariance: group_stats' pair sums over m - 1, here over sum_u = m
        assert np.allclose(got["cov"][0, 0] * m / (m - 1), want["cov"][0], rtol=1e-12, atol=0)
    src = RW.scored_rows(h.value, h.accepted, 4, T, 0, 2)[1]
    w, L, f, ess, logz = RW.chain_weights(h.value[src, 2], 0.75, 0.75)
    assert (w == 1.0).all() and L == 0.0 and f == 1.0 and (RW.int_weights(w * f, f) == 2 ** 20).all()
    # the state series: a row before the first accepted one carries no weight, but is counted
    h.accepted[:9, 1] = 0
    h.accepted[9, 1] = 1
    got = RW.reweighted_from_history(h, 4, T, 2, None, (0.75,), (), np.full(N, 0.75))
    assert got["count"][0] == N * (T - 4) and got["chain_n"][1] == T - 9 and got["n_scored"][0] == got["chain_n"].sum() < got["count"][0]


def test_known_answer_normal_target_from_three_temperatures():
    """v = theta^2 / 2: chain c samples N(0, 1 / a_c) and the target is N(0, 1 / a*).  The weighted variance must lie within 5 standard
    errors of 1 / a*, the standard error (1 / a*) sqrt(2 / ess) from the call's own ess; chain_logz must lie within 5 standard errors
    of log Z(a*) / Z(a_c) = log(a_c / a*) / 2, where chain_logz = L + log(mean w) has, by the delta method, the relative standard error
    of mean w: sqrt(E w^2 / (E w)^2 - 1) / sqrt(n_c) = sqrt(1 / chain_ess - 1 / n_c)"""
    acc, a_star, T = np.array([1.0, 1.5, 3.0]), 2.0, 2000
    rng = np.random.default_rng(20240607)
    h = zero_history(T, 3, 1, 1)
    h.params[:, 0, :] = rng.standard_normal((T, 3)) / np.sqrt(acc)[None, :]
    h.value[...] = 0.5 * h.params[:, 0, :] ** 2
    h.sim_moments[...] = h.params
    h.accepted[...] = 1
    got = RW.reweighted_from_history(h, 0, T, 2, None, (a_star,), (0.5,), acc)
    ess, cess = got["ess"][0, 0], got["chain_ess"][0]
    print("ess", ess, "chain_ess", cess, "var", got["cov"][0, 0, 0, 0], "logz", got["chain_logz"][0])
    assert (cess > 100).all() and ess > 100 and got["status"][0, 0] == 0
    assert np.isclose(ess, cess.sum(), rtol=1e-12)                               # each chain enters with its own effective sample size
    se = (1.0 / a_star) * np.sqrt(2.0 / ess)
    assert abs(got["cov"][0, 0, 0, 0] - 1.0 / a_star) < 5 * se, (got["cov"][0, 0, 0, 0], se)
    for c in range(3):
        se_z = np.sqrt(1.0 / cess[c] - 1.0 / T)
        assert abs(got["chain_logz"][0, c] - 0.5 * np.log(acc[c] / a_star)) < 5 * se_z, (c, got["chain_logz"][0, c], se_z)
    assert abs(got["mean"][0, 0, 0]) < 5 * np.sqrt(1.0 / a_star / ess) and abs(got["quantile"][0, 0, 0, 0]) < 5 * np.sqrt(1.0 / a_star / ess) * 1.2534
    assert np.isclose(got["value_mean"][0, 0], 0.5 / a_star, rtol=0, atol=5 * 0.5 * se)   # E v = var / 2


def test_crafted_history_reaches_every_branch():
    h, info = RC.crafted()
    got = RW.reweighted_from_history(h, 0, RC.CRAFT_T, 0, info["groups"], info["targets"], info["probs"], info["acc"])
    assert np.array_equal(got["status"], info["status"]) and np.array_equal(got["chain_n"], info["chain_n"])
    assert got["count"].tolist() == [120, 80, 40, 40, 40] and got["n_scored"].tolist() == [41, 80, 40, 40, 40]
    # a chain with no scored row, and one with a single row
    assert (got["chain_ess"][:, 1] == 0.0).all() and np.isnan(got["chain_logz"][:, 1]).all()
    assert (got["chain_ess"][:, 2] == 1.0).all()
    assert np.array_equal(got["chain_logz"][:, 2], [(0.5 - a) * 0.75 for a in info["targets"]])
    # the weights that underflow to 0: chain 3 at the target 1 keeps the 1e4 row alone, at the target 8 every row but it
    c3 = info["chain3"]
    assert got["chain_ess"][0, 3] == c3["ess"] and np.isclose(got["chain_logz"][0, 3], c3["logz"], rtol=1e-15, atol=0)
    src = np.arange(RC.CRAFT_T)
    w = RW.chain_weights(h.value[src, 3], 4.0, 1.0)[0]
    assert (w > 0).sum() == c3["kept"] and w[RC.BIG_ROW] == 1.0
    w = RW.chain_weights(h.value[src, 3], 4.0, 8.0)[0]
    assert w[RC.BIG_ROW] == 0.0 and (np.delete(w, RC.BIG_ROW) > 0).all()
    assert got["n_kept"][0, 1] == 1 + 40 and got["n_kept"][2, 1] == 39 + 40       # d of both signs in group 1 at the target 1
    # d * v overflows: +inf gives status 3 with the doubles NaN and the per-chain values as the contract's operations leave them (the
    # weight of the overflowing row is exp(inf - inf) = NaN, and smm_log reads a NaN's bits as a number: L = inf stays), -inf a weight of 0
    assert np.isnan(got["sum_u"][:2, 2]).all() and np.isnan(got["quantile"][:, :2, 2]).all() and (got["n_kept"][:2, 2] == 0).all()
    assert np.isnan(got["chain_ess"][:2, 5]).all() and (got["chain_logz"][:2, 5] == np.inf).all()
    assert got["n_kept"][2, 2] == 39 and np.isfinite(got["mean"][2, 2]).all() and np.isfinite(got["chain_logz"][2, 5])
    # a non-finite parameter: status 2, the per-chain values still there
    assert np.isnan(got["mean"][:, 3]).all() and np.isnan(got["ess"][:, 3]).all() and np.isfinite(got["chain_ess"][:, 6]).all()
    # ties at every quantile key under equal weights
    assert np.array_equal(got["quantile"][:, 0, 4], info["quantile4"]) and got["ess"][0, 4] == 40.0
    q = RW.int_weights(np.ones(40), 1.0)
    assert (q == 2 ** 20).all()
    assert np.signbit(RW.weighted_quantile(np.array([0.0, -0.0, 1.0]), np.array([1, 1, 1]), 0.0))   # -0.0 sorts before +0.0
    # a NaN simulated moment propagates into that moment's mean only
    h.sim_moments[3, 1, 0] = np.nan
    nan = RW.reweighted_from_history(h, 0, RC.CRAFT_T, 0, info["groups"], info["targets"], (), info["acc"])
    assert np.isnan(nan["m_mean"][:, 0, 1]).all() and np.array_equal(nan["m_mean"][:, 0, 0], got["m_mean"][:, 0, 0])
    assert np.array_equal(nan["mean"][:, 0], got["mean"][:, 0]) and (nan["status"][:, 0] == 0).all()


def test_pair_sums_and_quantiles_against_plain_numpy():
    """the weighted covariance and quantile against direct formulas, to rounding"""
    T, N = 60, 4
    h = random_history(T, N, 2, 2, 5)
    acc = np.array([0.5, 1.0, 2.0, 4.0])
    got = RW.reweighted_from_history(h, 0, T, 1, np.array([0, 0, 1, 1], np.int32), (1.0, 3.0), (0.3,), acc)
    for r, a in enumerate((1.0, 3.0)):
        for g, mem in enumerate(((0, 1), (2, 3))):
            th, u = [], []
            for c in mem:
                src = np.flatnonzero(h.accepted[:, c] != 0)
                w = np.exp((acc[c] - a) * h.value[src, c])
                w /= w.sum()
                ess = 1.0 / (w * w).sum()
                assert np.isclose(got["chain_ess"][r, c], ess, rtol=1e-12)
                assert np.isclose(got["chain_logz"][r, c], np.log(np.mean(np.exp((acc[c] - a) * h.value[src, c]))), rtol=1e-12)
                th.append(h.params[src, :, c])
                u.append(w * ess)
            th, u = np.concatenate(th), np.concatenate(u)
            mean = (u[:, None] * th).sum(0) / u.sum()
            cov = ((u[:, None] * (th - mean)).T @ (th - mean)) / u.sum()
            assert np.allclose(got["mean"][r, g], mean, rtol=1e-12) and np.allclose(got["cov"][r, g], cov, rtol=1e-11, atol=1e-15)
            assert np.isclose(got["ess"][r, g], u.sum() ** 2 / (u * u).sum(), rtol=1e-12)
            for j in range(2):                                                  # the weighted CDF crosses 0.3 at the quantile, to 2^-20
                below = u[th[:, j] < got["quantile"][0, r, g, j]].sum() / u.sum()
                upto = u[th[:, j] <= got["quantile"][0, r, g, j]].sum() / u.sum()
                assert below < 0.3 + 1e-4 and upto > 0.3 - 1e-4
