"""The numerical contract of smm_get_chain_stats (include/smmhip.h) restated in Python: numpy's mean, median, quantile (linear),
argmin and bincount-argmax on the compacted column.  tests/test_chain_stats.py holds it against numpy itself; the GPU tests hold the
device against it, over the history downloaded with smm_get_history."""
from math import floor

import numpy as np


def pw(x, lo, n):
    """numpy's pairwise sum"""
    if n < 8:
        r = 0.0
        for i in range(n):
            r = r + x[lo + i]
        return r
    if n <= 128:
        r = [x[lo + k] for k in range(8)]
        m = n - n % 8
        for i in range(8, m, 8):
            for k in range(8):
                r[k] = r[k] + x[lo + i + k]
        s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for i in range(m, n):
            s = s + x[lo + i]
        return s
    n2 = n // 2
    n2 -= n2 % 8
    return pw(x, lo, n2) + pw(x, lo + n2, n - n2)


def mean(x):
    x = [float(v) for v in x]
    S = 0.0
    for c in range(0, len(x), 8192):
        S = S + pw(x, c, min(8192, len(x) - c))
    return S / len(x) if len(x) else np.nan


def total_sort(x):
    """ascending in the IEEE total order (-0 before +0); x without NaN"""
    x = np.asarray(x, float)
    return x[np.lexsort((~np.signbit(x), x))]


def quantile(s, p):
    n = len(s)
    h = (n - 1) * p
    if h >= n - 1:
        a = b = s[n - 1]
        g = h + 1.0
    else:
        j = floor(h)
        a, b, g = s[j], s[j + 1], h - j
    d = b - a
    return b - d * (1 - g) if g >= 0.5 else a + d * g


def median(s):
    n = len(s)
    return (0.0 + s[n // 2]) / 1 if n % 2 else ((0.0 + s[n // 2 - 1]) + s[n // 2]) / 2


def column_stats(x, probs):
    """(mean, median, [quantile(p)]) of one compacted column"""
    x = np.asarray(x, float)
    if len(x) == 0 or np.isnan(x).any():
        return (np.nan if len(x) == 0 else mean(x)), np.nan, [np.nan] * len(probs)
    s = [float(v) for v in total_sort(x)]
    return mean(x), median(s), [quantile(s, float(p)) for p in probs]


def argmin_first(v):
    """np.argmin: the first NaN, else the first minimum"""
    v = np.asarray(v, float)
    return int(np.argmin(v))


def mode_of_partners(ex):
    ex = np.asarray(ex)
    ex = ex[ex != 0]
    return int(np.bincount(ex).argmax()) if len(ex) else 0


def stats_from_history(h, t0, t1, accepted_only, probs):
    """what smm_get_chain_stats returns, computed from a HistoryBuffers of iterations [0, >= t1)"""
    N, npar = h.value.shape[1], h.params.shape[1]
    probs = [float(p) for p in probs]
    out = dict(count=np.zeros(N, np.int32), mean=np.empty((npar, N)), median=np.empty((npar, N)),
               quantile=np.empty((len(probs), npar, N)), best_value=np.empty(N), best_iter=np.zeros(N, np.int32),
               n_exchanged=np.zeros(N, np.int32), most_exchanged_with=np.zeros(N, np.int32))
    for j in range(N):
        acc = h.accepted[t0:t1, j] != 0
        sel = acc if accepted_only else np.ones(t1 - t0, bool)
        out["count"][j] = sel.sum()
        for k in range(npar):
            m, md, q = column_stats(h.params[t0:t1, k, j][sel], probs)
            out["mean"][k, j], out["median"][k, j] = m, md
            out["quantile"][:, k, j] = q
        v = h.value[t0:t1, j]
        if len(v):
            i = argmin_first(v)
            out["best_value"][j], out["best_iter"][j] = v[i], t0 + i + 1
        else:
            out["best_value"][j], out["best_iter"][j] = np.nan, 0
        ex = h.exchanged[t0:t1, j]
        out["n_exchanged"][j] = (ex != 0).sum()
        out["most_exchanged_with"][j] = mode_of_partners(ex)
    return out


def assert_stats_equal(got, want, fields=None):
    for f in fields or want:
        assert np.array_equal(got[f], want[f], equal_nan=True), (f, np.argwhere(~((got[f] == want[f]) | (np.isnan(got[f]) & np.isnan(want[f])))
                                                                                 if got[f].dtype.kind == "f" else got[f] != want[f])[:5])
