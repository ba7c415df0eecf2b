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


def scores_scalar(r2, log=math.log):
    """z [M] of the ranks r2 [M], one ndtri call per distinct rank"""
    M = len(r2)
    u, inv = np.unique(r2, return_inverse=True)
    return np.array([ndtri(rank_prob(int(v), M), log) for v in u])[inv]


def horner(c, r):
    """((c[0] r + c[1]) r + ...) r + c[-1], as ndtri writes its polynomials out"""
    s = c[0] * r + c[1]
    for v in c[2:]:
        s = s * r + v
    return s


NUM_C = (2.5090809287301226727e+3, 3.3430575583588128105e+4, 6.7265770927008700853e+4, 4.5921953931549871457e+4,
         1.3731693765509461125e+4, 1.9715909503065514427e+3, 1.3314166789178437745e+2, 3.3871328727963666080e+0)
DEN_C = (5.2264952788528545610e+3, 2.8729085735721942674e+4, 3.9307895800092710610e+4, 2.1213794301586595867e+4,
         5.3941960214247511077e+3, 6.8718700749205790830e+2, 4.2313330701600911252e+1, 1.0)
NUM_M = (7.74545014278341407640e-4, 2.27238449892691845833e-2, 2.41780725177450611770e-1, 1.27045825245236838258e+0,
         3.64784832476320460504e+0, 5.76949722146069140550e+0, 4.63033784615654529590e+0, 1.42343711074968357734e+0)
DEN_M = (1.05075007164441684324e-9, 5.47593808499534494600e-4, 1.51986665636164571966e-2, 1.48103976427480074590e-1,
         6.89767334985100004550e-1, 1.67638483018380384940e+0, 2.05319162663775882187e+0, 1.0)
NUM_T = (2.01033439929228813265e-7, 2.71155556874348757815e-5, 1.24266094738807843860e-3, 2.65321895265761230930e-2,
         2.96560571828504891230e-1, 1.78482653991729133580e+0, 5.46378491116411436990e+0, 6.65790464350110377720e+0)
DEN_T = (2.04426310338993978564e-15, 1.42151175831644588870e-7, 1.84631831751005468180e-5, 7.86869131145613259100e-4,
         1.48753612908506148525e-2, 1.36929880922735805310e-1, 5.99832206555887937690e-1, 1.0)


def ndtri_array(p, log=math.log):
    """ndtri over the array p: the same operations in the same order on every element (numpy's elementwise *, +, -, / and sqrt are
    IEEE's, as Python's are); the logarithm stays the scalar one, called on the elements outside the central branch only"""
    p = np.asarray(p, float)
    q = p - 0.5
    out = np.empty_like(p)
    c = np.abs(q) <= 0.425
    qc = q[c]
    r = 0.180625 - qc * qc
    out[c] = (horner(NUM_C, r) * qc) / horner(DEN_C, r)
    pt, qt = p[~c], q[~c]
    r = np.where(qt <= 0.0, pt, 1.0 - pt)
    r = np.sqrt(-np.array([log(float(v)) for v in r], float))
    x = np.empty_like(r)
    m = r <= 5.0
    rm, rt = r[m] - 1.6, r[~m] - 5.0
    x[m] = horner(NUM_M, rm) / horner(DEN_M, rm)
    x[~m] = horner(NUM_T, rt) / horner(DEN_T, rt)
    out[~c] = np.where(qt < 0.0, -x, x)
    return out


def scores(r2, log=math.log):
    """z [M] of the ranks r2 [M]: scores_scalar over arrays (tests/test_rank_diag.py holds the two equal), for the columns of half a
    million values"""
    M = len(r2)
    u, inv = np.unique(r2, return_inverse=True)
    return ndtri_array((u.astype(float) * 0.5 - 0.375) / (float(M) + 0.25), log)[inv]


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


# --- the shapes and crafted series of tests/test_gpu_rank_edges.py: the sort, the ties and the batches at their edges ------------------
# Every shape is named once here with the path it reaches; tests/test_rank_diag.py proves each precondition on the CPU (digit coverage,
# the straddling run, the open cell at lag 256, no cell left out) and measures the effect of a one-ulp logarithm per shape: where that
# stays under RANK_LOG_CHANGE the shape is compared at RANK_RTOL, else at 8 x its own figure, written next to it (EDGE_RTOL).

RANK_SMALL, RANK_NBLK, RANK_HIST_LDS, RANK_WG = 8192, 64, 4096, 256                 # smm.jl_amd/csrc/smm_rank.hpp
RANK_TABLE_BYTES = 256 * RANK_NBLK * 4 * 4


def rank_nblk(M):
    """the workgroups of a column's radix pass"""
    return 1 if M <= RANK_SMALL else min(RANK_NBLK, -(-M // RANK_SMALL))


def rank_segments(M):
    """(nseg, seg): rank_segment's split of a column of M values: segment sg is [min(M, sg seg), min(M, sg seg + seg)); four segments
    (waves) to a workgroup"""
    nseg = 4 * rank_nblk(M)
    return nseg, -(-(-(-M // nseg)) // 64) * 64


def rank_bytes(k, h, max_lag):
    """the scratch bytes of one series of a group of k members (smm_reducers_host.hpp: 72 per pooled value, 80 + 32 LB per split
    chain, a long column's digit table)"""
    M, LB = 2 * k * h, min(RANK_WG, max_lag + 1)
    return M * 72 + 2 * k * (80 + 32 * LB) + (RANK_TABLE_BYTES if M > RANK_SMALL else 0)


def sort_keys(x):
    """uint64 [M]: the order keys the device sorts (stats_key of x with -0 taken as +0)"""
    b = (np.asarray(x, float) + 0.0).view(np.uint64)
    return np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))


def key_digits(x):
    """[8][M]: the radix digit of every key at every pass"""
    k = sort_keys(x)
    return np.stack([(k >> np.uint64(8 * b)) & np.uint64(255) for b in range(8)])


KEY_BASE = 0x40355A5A5A5A5A5A                           # 21.35..., every byte its own
KEY_DIGITS = (0x00, 0x01, 0x02, 0x0F, 0x10, 0x3F, 0x41, 0x7F, 0x80, 0x81, 0xA5, 0xC0, 0xF0, 0xFE, 0xFF)
KEY_DIGITS_TOP = (0x00, 0x01, 0x02, 0x0F, 0x10, 0x20, 0x3F, 0x41, 0x5B, 0x7E, 0x7F)   # byte 7 without the sign; 0x7F35 is finite
KEY_SPECIALS = (0.0, 5e-324, 2.2250738585072014e-308, 1.7976931348623157e308)


def key_values(extra=0):
    """the crafted values, ascending in the IEEE total order (-0 before +0), all finite and but for -0 / +0 distinct: for each byte
    b = 0 .. 7 the doubles whose bit patterns differ from KEY_BASE in byte b only, and their negatives; +-0, +-5e-324, +-the least
    normal, +-DBL_MAX; the doubles from 1e16 to 1e16 + 8 (2 apart there: 1e16 + {0 .. 4} and on); and `extra` more, 3, 4, 5, ..., to fill a column"""
    bits = [(KEY_BASE & ~(0xFF << (8 * b))) | (d << (8 * b)) for b in range(8) for d in (KEY_DIGITS if b < 7 else KEY_DIGITS_TOP)]
    v = np.array(bits, np.uint64).view(np.float64)
    v = np.concatenate([v, -v, KEY_SPECIALS, -np.array(KEY_SPECIALS), 1e16 + 2.0 * np.arange(5), 3.0 + np.arange(extra)])
    assert np.isfinite(v).all() and len(np.unique(v)) == len(v) - 1                   # (-0 == +0)
    return v[np.lexsort((~np.signbit(v), v))]


N_KEY_VALUES = len(key_values())


def three_orders(col, seed):
    """the column ascending (as given), descending and shuffled: the three series of a crafted group"""
    return [col, col[::-1], col[np.random.default_rng(seed).permutation(len(col))]]


def pooled_to_series(col, k, n):
    """[k][n]: the pooled column col [2 k h] back in its members' series over a window of n iterations (the middle iteration of an
    odd window, which no split chain holds, is 0.5)"""
    h = n // 2
    c = np.asarray(col, float).reshape(k, 2, h)
    out = np.full((k, n), 0.5)
    out[:, :h], out[:, n - h:] = c[:, 0], c[:, 1]
    return out


def tie_column(M, runs, seed, zero_run=65):
    """(col [M] ascending, starts, lens): key_values with each value repeated: the tie runs `runs` and single values up to M, the
    lengths dealt to the values by seed, the run of zero_run values on zero, its members -0 and +0 in turn"""
    lens = np.array(list(runs) + [1] * (M - sum(runs)))
    pool = np.unique(key_values(max(0, len(lens) + 1 - N_KEY_VALUES)))
    idx = np.round(np.linspace(0, len(pool) - 1, len(lens))).astype(int)           # (a short column: values from the whole range)
    idx[np.argmin(np.abs(idx - np.flatnonzero(pool == 0.0)[0]))] = np.flatnonzero(pool == 0.0)[0]
    pool = pool[idx]
    lens = lens[np.random.default_rng(seed).permutation(len(lens))]
    iz, jz = int(np.flatnonzero(pool == 0.0)[0]), int(np.flatnonzero(lens == zero_run)[0])
    lens[iz], lens[jz] = lens[jz], lens[iz]
    col = np.repeat(pool, lens)
    z = np.flatnonzero(col == 0.0)
    col[z[::2]] = -0.0
    return col, np.cumsum(lens) - lens, lens


# 1. keys, one byte per pass: one group of 3, h = 59, M = 354 <= RANK_SMALL: k_rank_sort_small, segments of 128 (wave 2 part, wave 3
#    empty); every digit position of the keys varies; -0 / +0 the only tie
KEYS_N, KEYS_T = 3, 118
KEYS_M = 2 * KEYS_N * (KEYS_T // 2)


def keys_series():
    """X [3][N][T]: key_values ascending in parameter 0, descending in parameter 1, shuffled in the value"""
    return np.stack([pooled_to_series(c, KEYS_N, KEYS_T) for c in three_orders(key_values(KEYS_M - N_KEY_VALUES), 3)])


# 2. tie runs.  Short: group 0 of 4, h = 250, M = 2000 (one workgroup, wave segments of 512); the runs 1, 2, 63, 64, 65 and a whole
#    wave segment - 1, + 0, + 1 in parameter 0 (ascending) and the value (shuffled), and, as those lengths and a run longer than half
#    the column do not fit into one column, that run (1001) in parameter 1 (descending); group 1 of 1 member, M = 500: -0 and +0 only
#    but for one other value.  Long: one group of 17, h = 281, M = 9554 (nblk = 2, 8 segments of 1216): all of these runs in one
#    column, the long one (4778) across the boundary between the two workgroups' segments at 4864
TIES_SHORT_N, TIES_SHORT_T, TIES_SHORT_GROUPS = 5, 500, np.array([0, 0, 0, 0, 1])
TIES_SHORT_M, ZEROS_M = 2000, 500
TIES_SHORT_RUNS = ((1, 2, 63, 64, 65, 511, 512, 513), (1, 2, 63, 64, 65, 1001))
TIES_LONG_N, TIES_LONG_T, TIES_LONG_M = 17, 562, 9554
TIES_LONG_RUNS = (1, 2, 63, 64, 65, 1215, 1216, 1217, 4778)
TIES_SEED = 4


def zeros_columns():
    """[3][ZEROS_M]: -0 and +0 in turn and one other value: above, below, and a denormal above"""
    cols = np.zeros((3, ZEROS_M))
    cols[:, ::2] = -0.0
    cols[0, 7], cols[1, 300], cols[2, ZEROS_M - 1] = 1.5, -2.5, 5e-324
    return cols


def ties_short_series():
    """X [3][5][T] and the pooled columns of group 0"""
    a, b = (tie_column(TIES_SHORT_M, r, TIES_SEED)[0] for r in TIES_SHORT_RUNS)
    cols = [a, b[::-1], a[np.random.default_rng(TIES_SEED).permutation(TIES_SHORT_M)]]
    X = [np.concatenate([pooled_to_series(c, 4, TIES_SHORT_T), pooled_to_series(z, 1, TIES_SHORT_T)]) for c, z in zip(cols, zeros_columns())]
    return np.stack(X), cols


def ties_long_series():
    """X [3][17][T] and the pooled columns"""
    cols = three_orders(tie_column(TIES_LONG_M, TIES_LONG_RUNS, TIES_SEED)[0], TIES_SEED)
    return np.stack([pooled_to_series(c, TIES_LONG_N, TIES_LONG_T) for c in cols]), cols


def chain_ranks(col, n_chains):
    """[n_chains][2 M] int64: how often each twice-rank - 1 occurs in each member's part of the pooled column col: rank_hist [:, s, c]
    of the members at n_bins = 2 M, where the contract's bin ((rank2 - 1) n_bins) / (2 M) is rank2 - 1"""
    M = len(col)
    r = rank2(col).reshape(n_chains, -1) - 1
    return np.stack([np.bincount(v, minlength=2 * M) for v in r])


def generated(N, T, seed, **kw):
    """keywords of workloads.serial_normal for a generated history of the mixing population"""
    return dict(MIXING, N=N, T=T, acc_tuners=1.0, seed=seed, **kw)


# 3. lengths, h = 256 from the windows (0, 512) and (0, 513) (the odd one drops the middle iteration): groups of 16 (M = 8192 =
#    RANK_SMALL, the last one-workgroup length), 17 (M = 8704, nblk = 2, segments of 1088: the last workgroup's part empty), 1
#    (M = 512) and an id without members.  On the same history the windows (0, 8) and (0, 9) with one group of one member: M = 8,
#    waves 1 - 3 without values
LENGTHS_KW = generated(34, 513, 2)
LENGTHS_GROUPS, LENGTHS_NG = np.r_[np.zeros(16, int), np.ones(17, int), 2], 4
LENGTHS_WINDOWS = ((0, 512), (0, 513))
TINY_GROUPS, TINY_WINDOWS = np.r_[-np.ones(5, int), 0, -np.ones(28, int)], ((0, 8), (0, 9))
# ... and a group of 70 members: m = 140 split chains > 128, the recursive branch of rank_pw in k_rank_cell_mom and k_rank_geyer: the
#    leaves are [0, 64) and [64, 140) (tests/test_rank_diag.py asserts the split); h = 20
WIDE_KW = generated(72, 40, 3)
WIDE_GROUPS = np.r_[np.zeros(70, int), 1, 1]

# 4. two long columns and short ones between, one call: long A (16 members, M = 9600, nblk = 2), short (2), long B (28 members,
#    M = 16800, nblk = 3), an id without members, short (1); chain 47 in no group.  The digit table of B lies at large[g] = 1.  The
#    context holds 3600 iterations, of which 600 are run, so that the reducers' scratch (at most the history's compacted columns,
#    N x maxiter x 20 bytes) can hold A, the short group and B of one series at once: TWO_LONG_SCRATCH, computed from rank_bytes
TWO_LONG_KW = generated(48, 3600, 4)
TWO_LONG_STEPS, TWO_LONG_LAG = 600, 299
TWO_LONG_GROUPS, TWO_LONG_NG = np.r_[np.zeros(16, int), 1, 1, np.full(28, 2), 4, -1], 5
TWO_LONG_SCRATCH = sum(rank_bytes(k, TWO_LONG_STEPS // 2, TWO_LONG_LAG) for k in (16, 2, 28))

# 5. the cap and the long half-window: h = 8200 > 8192 (k_rank_acov reads global memory, pw_sum and diag_pw walk a second chunk);
#    group 0 of 32: M = 524800 > RANK_NBLK x RANK_SMALL (nblk capped at 64, segments of 2112); group 1 of 2: M = 32800, nblk = 5.
#    The GPU test takes 0.8 s on an MI355X (run and history 0.36 s, the call 0.02 s, the restatement 0.37 s)
#    (the example's population with its ladder and exchange: the mixing one, whose proposal is as wide as the box, does not last
#    16400 iterations)
CAP_KW = dict(N=34, T=16400, ns=100, seed=5)
CAP_GROUPS, CAP_LAG, CAP_BINS = np.r_[np.zeros(32, int), 1, 1], 4, 4100

# 6. a second block of lags: the population of test_a_population_that_has_not_mixed at N = 16, T = 600, max_lag = 299: cells still
#    open at lag 256 (status 1: max_lag came first)
LAGS_KW = dict(MIXING, N=16, T=600, sigma0=0.05, maxtemp=5.0, p2_bounds=(-20.0, 20.0), mom=(-1.0, 10.0), min_improve=0.0, acc_tuners=None,
               seed=12)
LAGS_GROUPS = np.arange(16) // 8

# 7. non-finite and empty: groups of 3: +inf once in parameter 1 of chain 1 (group 0), NaN once in the value of chain 5 (group 1),
#    a clean group 2 and group 3 without members
NONFINITE_KW = generated(9, 40, 6)
NONFINITE_GROUPS, NONFINITE_NG = np.arange(9) // 3, 4


def make_nonfinite(params, value):
    """the two non-finite values of case 7 into params [T][np][N], value [T][N]"""
    params[31, 1, 1] = np.inf
    value[4, 5] = np.nan


# the tolerance of each shape's outputs behind ndtri: RANK_RTOL where the measured effect of a one-ulp logarithm stays under
# RANK_LOG_CHANGE (tests/test_rank_diag.py measures every shape), else 8 x the shape's own figure
LENGTHS_LOG_CHANGE = 2.3e-15                            # measured: 2.29e-15, above RANK_LOG_CHANGE
EDGE_RTOL = dict(keys=RANK_RTOL, ties_short=RANK_RTOL, ties_long=RANK_RTOL, lengths=8 * LENGTHS_LOG_CHANGE, tiny=RANK_RTOL, wide=RANK_RTOL,
                 two_long=RANK_RTOL, cap=RANK_RTOL, lags=RANK_RTOL, nonfinite=RANK_RTOL)
