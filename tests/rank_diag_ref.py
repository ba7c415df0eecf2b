"""The numerical contract of smm_get_rank_diag (include/smmhip.h) restated in numpy and the standard library: the split chains of a
group pooled, twice-average ranks from a stable argsort and its tie runs, Wichura's AS 241 (PPND16) normal scores with the logarithm as
a parameter, the rank-normalised split R-hat (bulk, folded), the multi-chain ESS by the library's Geyer truncation of the combined
autocorrelation (bulk, tail, mean) and the rank histogram of every chain.  It builds on chain_diag_ref (S, series_from_history, rowsum)
and on chain_stats_ref's order statistics.  tests/test_rank_diag.py holds it against brute force, statistics.NormalDist and theory; the
GPU tests hold the device against it."""
import math

import numpy as np

from chain_diag_ref import S, rowsum, series_from_history
from chain_stats_ref import mean, median, quantile

# The outputs that pass through ndtri depend on whose logarithm is used (the contract's smm_log is within 1 ulp, as is math.log).
# RANK_LOG_CHANGE is the largest relative change of rhat_bulk / rhat_folded / rhat_rank / ess_bulk measured when the logarithm moves by
# one ulp either way, on the shapes of tests/test_gpu_rank_diag.py (tests/test_rank_diag.py measures it again and holds it under this
# figure); RANK_RTOL = 8 x that: the two logarithms erring in opposite directions, and a Geyer truncation near a sign change.
RANK_LOG_CHANGE = 1.5e-15
RANK_RTOL = 8 * RANK_LOG_CHANGE


# the shapes of tests/test_gpu_rank_diag.py, which tests/test_rank_diag.py measures the tolerance on
N_SMALL, T_SMALL = 32, 40
GROUPS_SMALL = np.r_[np.zeros(16, int), np.ones(14, int), 2, -1][np.random.default_rng(5).permutation(32)]   # 16, 14, 1 members, one chain out
WINDOWS_SMALL = ((3, 20), (0, 40))
N_LARGE, T_LARGE = 18, 600
GROUPS_LARGE = np.r_[np.zeros(16, int), 1, 1]          # M = 2 x 16 x 300 = 9600 > 8192, and a group of 2 (M = 1200)

# The populations of those shapes (keywords of workloads.serial_normal, objfunc_norm with np = 2 and ns = 100).  At least 90 % of their
# cells must have status 0, with h = 8 at the shortest, so the chains have to forget their state within a few iterations: a box that is
# symmetric about the target, a proposal as wide as the box (sigma is in units of the box), one temperature, and no exchange (with
# min_improve = 0 the exchange hands the lower value to the lower chain of each pair, so the chains of a group differ for good in their
# objective values and rho_t never comes down: status 1, rightly).  acc_tuner sets the share of rejected iterations, i.e. of ties: 15 %
# in the small shape, whose 7 lags leave no room for more, 65 % in the large one.  The seeds were chosen on the CPU oracle, whose
# history is the device's (tests/test_rank_diag.py checks the 90 % and the 5 % of cells left out on it).
MIXING = dict(ns=100, sigma0=1.0, maxtemp=1.0, p2_bounds=(-3.0, 3.0), mom=(0.0, 0.0), min_improve=1e9)
SMALL_KW = dict(MIXING, N=N_SMALL, T=T_SMALL, acc_tuners=0.15, seed=9)
LARGE_KW = dict(MIXING, N=N_LARGE, T=T_LARGE, acc_tuners=1.0, seed=1)


def share_of_cells_with_status_0(results):
    """of the (group, series) cells of these results, the share whose four statuses (bulk, folded, tail, mean) are all 0"""
    return float(np.mean(np.concatenate([(r["status"] == 0).all(axis=0).ravel() for r in results])))


def rank2(x):
    """int64 [M]: 2 L + E + 1 of every value of x (L values strictly less, E equal, itself included; -0.0 == +0.0): twice scipy's
    average rank"""
    x = np.asarray(x, float) + 0.0
    M = len(x)
    o = np.argsort(x, kind="stable")
    s = x[o]
    starts = np.flatnonzero(np.r_[True, s[1:] != s[:-1]])
    lens = np.diff(np.r_[starts, M])
    r = np.empty(M, np.int64)
    r[o] = np.repeat(2 * starts + lens + 1, lens)
    return r


def ndtri(p, log=math.log):
    """Wichura's AS 241 PPND16, every operation in its order (the algorithm of statistics.NormalDist.inv_cdf)"""
    q = p - 0.5
    if abs(q) <= 0.425:
        r = 0.180625 - q * q
        num = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r
                   + 4.5921953931549871457e+4) * r + 1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r
                + 1.3314166789178437745e+2) * r + 3.3871328727963666080e+0) * q
        den = (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r
                   + 2.1213794301586595867e+4) * r + 5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r
                + 4.2313330701600911252e+1) * r + 1.0)
        return num / den
    r = p if q <= 0.0 else 1.0 - p
    r = math.sqrt(-log(r))
    if r <= 5.0:
        r = r - 1.6
        num = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r
                   + 1.27045825245236838258e+0) * r + 3.64784832476320460504e+0) * r + 5.76949722146069140550e+0) * r
                + 4.63033784615654529590e+0) * r + 1.42343711074968357734e+0)
        den = (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r
                   + 1.48103976427480074590e-1) * r + 6.89767334985100004550e-1) * r + 1.67638483018380384940e+0) * r
                + 2.05319162663775882187e+0) * r + 1.0)
    else:
        r = r - 5.0
        num = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r
                   + 2.65321895265761230930e-2) * r + 2.96560571828504891230e-1) * r + 1.78482653991729133580e+0) * r
                + 5.46378491116411436990e+0) * r + 6.65790464350110377720e+0)
        den = (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r
                   + 7.86869131145613259100e-4) * r + 1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r
                + 5.99832206555887937690e-1) * r + 1.0)
    x = num / den
    return -x if q < 0.0 else x


def rank_prob(r2, M):
    """the probability whose normal score a value of rank r2 among M gets"""
    return (float(r2) * 0.5 - 0.375) / (float(M) + 0.25)


def scores(r2, log=math.log):
    """z [M] of the ranks r2 [M]"""
    M = len(r2)
    u, inv = np.unique(r2, return_inverse=True)
    return np.array([ndtri(rank_prob(int(v), M), log) for v in u])[inv]


def split_moments(Y):
    """(D, W, var_plus, rhat) of the m chains Y [m][h]: the split R-hat's arithmetic on the chains as they stand"""
    Y = np.ascontiguousarray(Y, float)
    m, h = Y.shape
    mu = rowsum(Y) / h
    D = Y - mu[:, None]
    var = rowsum(D * D) / (h - 1)
    W, mm = mean(var), mean(mu)
    v = S([(a - mm) * (a - mm) for a in mu]) / (m - 1)
    vp = ((h - 1.0) / h) * W + v
    with np.errstate(invalid="ignore", divide="ignore"):
        rhat = float(np.sqrt(np.float64(vp) / np.float64(W)))
    return D, W, vp, rhat


def ess_multi(Y, max_lag, block=64):
    """(ess, status, rhat, P_J) of the m chains Y [m][h]: the library's Geyer truncation on the combined autocorrelation
    rho_t = 1 - (W - mean_j acov_{j,t}) / var_plus.  P_J: the pair sum that truncated the sequence (NaN for none)"""
    D, W, vp, rhat = split_moments(Y)
    m, h = D.shape
    if W == 0.0 or vp == 0.0:
        return np.nan, 2, rhat, np.nan
    rho = [1.0]

    def need(k):
        while len(rho) <= k:
            for t in range(len(rho), min(max_lag, len(rho) + block - 1) + 1):
                ac = rowsum(D[:, : h - t] * D[:, t:]) / h
                rho.append(1.0 - (W - mean(ac)) / vp)

    Q = T = 0.0
    j, trunc, PJ = 0, False, np.nan
    while 2 * j + 1 <= max_lag:
        need(2 * j + 1)
        P = rho[2 * j] + rho[2 * j + 1]
        if j == 0:
            Q = P
            T = 0.0 + Q
        elif not (P > 0.0):
            trunc, PJ = True, P
            break
        else:
            Q = P if P < Q else Q
            T = T + Q
        j += 1
    tau = -1.0 + 2.0 * T
    if not (tau > 0.0):
        return np.nan, 2, rhat, PJ
    return float(m * h) / tau, (0 if trunc else 1), rhat, PJ


def cell(Y, max_lag, log=math.log):
    """the statistics of one (group, series) cell from its m split chains Y [m][h] (finite): a dict, and the ranks r2 [M]"""
    m, h = Y.shape
    x = np.ascontiguousarray(Y, float).reshape(-1)
    r2 = rank2(x)
    s = [float(v) for v in np.sort(x + 0.0)]
    med, q05, q95 = median(s), quantile(s, 0.05), quantile(s, 0.95)
    z = scores(r2, log).reshape(m, h)
    zf = scores(rank2(np.abs(x - med)), log).reshape(m, h)
    ess_b, st_b, rh_b, PJ = ess_multi(z, max_lag)
    _, W, vp, rh_f = split_moments(zf)
    st_f = 2 if (W == 0.0 or vp == 0.0) else 0
    e05, s05, _, _ = ess_multi(np.where(Y <= q05, 1.0, 0.0), max_lag)
    e95, s95, _, _ = ess_multi(np.where(Y <= q95, 1.0, 0.0), max_lag)
    ess_m, st_m, _, _ = ess_multi(Y, max_lag)
    rr = np.nan if (rh_b != rh_b or rh_f != rh_f) else (rh_b if rh_b > rh_f else rh_f)
    et = np.nan if (e05 != e05 or e95 != e95) else (e05 if e05 < e95 else e95)
    return dict(rhat_rank=rr, rhat_bulk=rh_b, rhat_folded=rh_f, ess_bulk=ess_b, ess_tail=et, ess_mean=ess_m,
                status=(st_b, st_f, max(s05, s95), st_m), pair_at_truncation=PJ), r2


FLOATS = ("rhat_rank", "rhat_bulk", "rhat_folded", "ess_bulk", "ess_tail", "ess_mean")


def rank_diag_from_series(X, max_lag, n_bins=20, groups=None, n_groups=None, log=math.log):
    """what smm_get_rank_diag returns for the series X [S][N][n], and pair_at_truncation [G][S] (the bulk ESS's truncating pair sum)"""
    Sn, N, n = X.shape
    h = n // 2
    g = np.zeros(N, int) if groups is None else np.asarray(groups)
    G = (int(g.max()) + 1 if groups is not None else 1) if n_groups is None else n_groups
    out = {f: np.full((G, Sn), np.nan) for f in FLOATS + ("pair_at_truncation",)}
    out["status"] = np.full((4, G, Sn), 2, np.int32)
    out["rank_hist"] = np.zeros((n_bins, Sn, N), np.int64)
    for gi in range(G):
        mem = np.flatnonzero(g == gi)
        if len(mem) == 0:
            continue
        for s in range(Sn):
            Y = np.stack([X[s, c, lo:lo + h] for c in mem for lo in (0, n - h)])
            if not np.isfinite(Y).all():
                out["status"][:, gi, s] = 3
                continue
            r, r2 = cell(Y, max_lag, log)
            for f in FLOATS + ("pair_at_truncation",):
                out[f][gi, s] = r[f]
            out["status"][:, gi, s] = r["status"]
            if n_bins > 0:
                M = len(r2)
                b = ((r2 - 1) * n_bins) // (2 * M)
                np.add.at(out["rank_hist"], (b, s, np.repeat(mem, 2 * h)), 1)
    return out


def rank_diag_from_history(hist, t0, t1, max_lag=None, n_bins=20, groups=None, n_groups=None, log=math.log):
    X, _ = series_from_history(hist, t0, t1)
    return rank_diag_from_series(X, (t1 - t0) // 2 - 1 if max_lag is None else max_lag, n_bins, groups, n_groups, log)


EXACT = ("rank_hist", "status", "ess_tail", "ess_mean")
TOLERANCED = ("rhat_bulk", "rhat_folded", "rhat_rank", "ess_bulk")


def near_sign_change(want, rtol=RANK_RTOL):
    """[G][S] bool: the cells whose bulk ESS may be left out of the toleranced comparison: the pair sum that truncated Geyer's sequence
    lies within the tolerance of zero, so that a one-ulp change of the logarithm moves J"""
    with np.errstate(invalid="ignore"):
        return np.abs(want["pair_at_truncation"]) <= rtol


def assert_rank_diag_close(got, want, rtol=RANK_RTOL, max_left_out=0.05):
    """the device's (or a batched call's) outputs against the restatement's: EXACT fields array_equal with NaNs in the same places, the
    fields behind ndtri within rtol, but for at most max_left_out of the cells near a sign change (ess_bulk only)"""
    for f in EXACT:
        assert got[f].shape == want[f].shape, (f, got[f].shape, want[f].shape)
        assert np.array_equal(got[f], want[f], equal_nan=got[f].dtype.kind == "f"), (f, got[f], want[f])
    skip = near_sign_change(want, rtol)
    assert skip.mean() <= max_left_out, skip.mean()
    for f in TOLERANCED:
        a, b = got[f], want[f]
        assert a.shape == b.shape, (f, a.shape, b.shape)
        assert np.array_equal(np.isnan(a), np.isnan(b)) or f == "ess_bulk", (f, a, b)
        with np.errstate(invalid="ignore"):
            ok = (np.isnan(a) & np.isnan(b)) | (a == b) | (np.abs(a - b) <= rtol * np.abs(b))
        if f == "ess_bulk":
            ok |= skip
        assert ok.all(), (f, np.argwhere(~ok)[:5], a[~ok][:5], b[~ok][:5])
