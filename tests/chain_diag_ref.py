"""The numerical contract of smm_get_chain_diag (include/smmhip.h) restated in Python: the carry-forward series of a downloaded
history, the autocovariances, Geyer's initial monotone sequence, the status and the split R-hat.  The sums are the chain-stats sum S
(chain_stats_ref.pw over chunks of 8192); the vectorised paths use row-wise np.sum on C-contiguous [columns][n] arrays, which
tests/test_chain_diag.py holds against it bit for bit.  The GPU tests hold the device against this restatement."""
import numpy as np

from chain_stats_ref import mean, pw


def S(x):
    """the chain-stats chunked pairwise sum of x (bit for bit np.sum of a contiguous float64 array)"""
    x = [float(v) for v in x]
    s = 0.0
    for c in range(0, len(x), 8192):
        s = s + pw(x, c, min(8192, len(x) - c))
    return s


def acov_pw(x, k):
    """acov_k by the contract, summed element by element: S(d[0:n-k] * d[k:n]) / n"""
    x = np.asarray(x, float)
    n = len(x)
    d = x - mean(x)
    return S(d[: n - k] * d[k:]) / n


def rowsum(a):
    """S of every row of a [columns][m] array"""
    return np.sum(np.ascontiguousarray(a, float), axis=1)


def geyer(rho, max_lag):
    """(tau, truncated, J) of one column from rho_0 .. rho_K, K >= the lag where the sequence is truncated (or max_lag)"""
    Q = T = 0.0
    j = 0
    while 2 * j + 1 <= max_lag:
        P = rho[2 * j] + rho[2 * j + 1]
        if j == 0:
            Q = P
            T = 0.0 + Q
        elif not (P > 0.0):
            return -1.0 + 2.0 * T, True, j
        else:
            Q = P if P < Q else Q
            T = T + Q
        j += 1
    return -1.0 + 2.0 * T, False, j


def _truncated_by(rho, K, max_lag):
    """is the sequence truncated within lags 0 .. K"""
    j = 1
    while 2 * j + 1 <= min(K, max_lag):
        P = rho[2 * j] + rho[2 * j + 1]
        if not (P > 0.0):
            return True
        j += 1
    return False


def diag_columns(X, max_lag, n_acf, block=64, pairs=None):
    """ess [C], status [C], acf [n_acf][C], hmu [2][C], hvar [2][C] of the columns X [C][n] (pairs [C], if given: J, the pairs
    Geyer's sequence kept)"""
    X = np.ascontiguousarray(X, float)
    C, n = X.shape
    ess, status = np.full(C, np.nan), np.zeros(C, np.int32)
    acf = np.full((n_acf, C), np.nan)
    hmu, hvar = np.full((2, C), np.nan), np.full((2, C), np.nan)
    fin = np.isfinite(X).all(axis=1)
    status[~fin] = 3
    cols = np.flatnonzero(fin)
    if len(cols) == 0:
        return ess, status, acf, hmu, hvar
    Xf = X[cols]
    h = n // 2
    for hf, Y in enumerate((Xf[:, :h], Xf[:, n - h:])):
        mu = rowsum(Y) / h
        e = Y - mu[:, None]
        hmu[hf, cols], hvar[hf, cols] = mu, rowsum(e * e) / (h - 1)
    D = Xf - (rowsum(Xf) / n)[:, None]
    ac = np.full((len(cols), max_lag + 1), np.nan)
    K = -1                           # lags done: 0 .. K
    live = np.arange(len(cols))      # columns still needing lags
    while K < max_lag and len(live):
        k1 = min(max_lag, K + block)
        Dl = D if len(live) == len(cols) else D[live]
        for k in range(K + 1, k1 + 1):
            ac[live, k] = rowsum(Dl[:, : n - k] * Dl[:, k:]) / n
        K = k1
        if K + 1 >= n_acf:
            live = np.array([q for q in live if not _truncated_by(ac[q] / ac[q, 0], K, max_lag)], int)
    for q, c in enumerate(cols):
        rho = ac[q] / ac[q, 0]
        tau, trunc, J = geyer(rho, max_lag)
        if pairs is not None:
            pairs[c] = J
        a0 = ac[q, 0]
        if a0 == 0.0 or not (tau > 0.0):
            status[c], ess[c] = 2, np.nan
        else:
            status[c], ess[c] = (0 if trunc else 1), n / tau
        acf[:, c] = rho[:n_acf]
    return ess, status, acf, hmu, hvar


def series_from_history(h, t0, t1):
    """X [S][N][n] (the carry-forward series: the parameters, then the value) and the accept rate [N] from a HistoryBuffers of
    iterations [0, >= t1)"""
    acc = h.accepted[:t1] != 0
    T, N = acc.shape
    rows = np.where(acc, np.arange(T)[:, None], -1)
    a = np.maximum.accumulate(rows, axis=0)[t0:t1]          # [n][N]
    npar = h.params.shape[1]
    X = np.full((npar + 1, N, t1 - t0), np.nan)
    ok = a >= 0
    j = np.broadcast_to(np.arange(N), a.shape)
    for s in range(npar):
        X[s].T[ok] = h.params[a[ok], s, j[ok]]
    X[npar].T[ok] = h.value[a[ok], j[ok]]
    noex = h.exchanged[t0:t1] == 0
    A = (noex & acc[t0:t1]).sum(axis=0)
    E = noex.sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        rate = A.astype(float) / E.astype(float)
    return X, rate


def rhat_group(mus, vars_, h):
    """split R-hat from the halves' means and variances, listed member by member, first half then second"""
    if len(mus) == 0:
        return np.nan
    W, mm = mean(vars_), mean(mus)
    v = S([(m - mm) * (m - mm) for m in mus]) / (len(mus) - 1)
    vp = ((h - 1.0) / h) * W + v
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.sqrt(np.float64(vp) / np.float64(W)))   # (IEEE: W == 0 gives inf or NaN, as on the device)


def diag_from_series(X, rate, max_lag, n_acf=0, groups=None, pairs=None):
    """what smm_get_chain_diag returns for the series X [S][N][n] (pairs: see diag_columns)"""
    Sn, N, n = X.shape
    ess, status, acf, hmu, hvar = diag_columns(X.reshape(Sn * N, n), max_lag, n_acf, pairs=pairs)
    out = dict(accept_rate=rate, ess=ess.reshape(Sn, N), status=status.reshape(Sn, N), acf=acf.reshape(n_acf, Sn, N))
    if groups is not None:
        g = np.asarray(groups)
        ng = int(g.max()) + 1 if len(g) else 0
        hmu, hvar = hmu.reshape(2, Sn, N), hvar.reshape(2, Sn, N)
        out["rhat"] = np.full((ng, Sn), np.nan)
        for gi in range(ng):
            mem = np.flatnonzero(g == gi)
            for s in range(Sn):
                if len(mem) and not (out["status"][s, mem] == 3).any():
                    mus = [float(hmu[hf, s, c]) for c in mem for hf in (0, 1)]
                    vs = [float(hvar[hf, s, c]) for c in mem for hf in (0, 1)]
                    out["rhat"][gi, s] = rhat_group(mus, vs, n // 2)
    return out


def diag_from_history(h, t0, t1, max_lag=None, n_acf=0, groups=None, pairs=None):
    X, rate = series_from_history(h, t0, t1)
    return diag_from_series(X, rate, t1 - t0 - 1 if max_lag is None else max_lag, n_acf, groups, pairs)


def assert_diag_equal(got, want):
    for f in want:
        a, b = got[f], want[f]
        assert a.shape == b.shape, (f, a.shape, b.shape)
        same = (a == b) | (np.isnan(a) & np.isnan(b)) if a.dtype.kind == "f" else a == b
        assert same.all(), (f, np.argwhere(~same)[:5], a[~same][:5], b[~same][:5])
