"""The numerical contract of smm_get_trace (include/smmhip.h) restated in numpy over a downloaded history: for each kept iteration and
group the contiguous column of the selected members in ascending local index, then np.mean, np.var(ddof=1), np.median,
np.quantile(method="linear") and np.argmin.  The state look-back a(t) is chain_diag_ref.series_from_history's (tests/test_trace.py holds
the two against each other).  Columns are always C-contiguous copies: numpy sums a strided view in another order.  Columns of equal
length are stacked and reduced along the last axis, which tests/test_trace.py holds bit for bit against the one-column calls; columns
past 8192 members (numpy's buffer) are reduced one by one."""
import warnings

import numpy as np

SELECT = {"all": 0, "accepted": 1, "state": 2}


def n_rows(t0, t1, stride):
    return max(0, -(-(t1 - t0) // stride))


def state_rows(accepted, t1):
    """a [t1][N]: the last row r <= t with accepted[r] != 0, -1 for none (chain_diag_ref.series_from_history's look-back)"""
    acc = accepted[:t1] != 0
    rows = np.where(acc, np.arange(acc.shape[0])[:, None], -1)
    return np.maximum.accumulate(rows, axis=0) if acc.shape[0] else rows


def column_stats(x, probs):
    """(mean, var, median, quantile [len(probs)]) of ONE column, by the one-column numpy calls of the contract"""
    x = np.ascontiguousarray(x, np.float64)
    m = len(x)
    nan = np.full(len(probs), np.nan)
    if m == 0:
        return np.nan, np.nan, np.nan, nan
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        q = np.quantile(x, np.asarray(probs, float), method="linear") if len(probs) else nan
        return np.mean(x), (np.var(x, ddof=1) if m >= 2 else np.nan), np.median(x), q


def stacked_stats(X, probs):
    """the same of every column of X [C][m] (C-contiguous): mean, var, median [C], quantile [len(probs)][C]"""
    X = np.ascontiguousarray(X, np.float64)
    C, m = X.shape
    nq = len(probs)
    if m == 0 or C == 0:
        return np.full(C, np.nan), np.full(C, np.nan), np.full(C, np.nan), np.full((nq, C), np.nan)
    if m > 8192:
        r = [column_stats(X[c], probs) for c in range(C)]
        return (np.array([v[0] for v in r]), np.array([v[1] for v in r]), np.array([v[2] for v in r]),
                np.array([v[3] for v in r]).reshape(C, nq).T)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        q = np.quantile(X, np.asarray(probs, float), axis=-1, method="linear") if nq else np.empty((0, C))
        var = np.var(X, axis=-1, ddof=1) if m >= 2 else np.full(C, np.nan)
        return np.mean(X, axis=-1), var, np.median(X, axis=-1), q


def fields(h, moments):
    """F [S][T][N]: the parameters, the value and, with moments, the simulated moments"""
    f = [h.params[:, k, :] for k in range(h.params.shape[1])] + [h.value]
    if moments:
        f += [h.sim_moments[:, k, :] for k in range(h.sim_moments.shape[1])]
    return np.stack([np.asarray(a, np.float64) for a in f])


def trace_from_history(h, t0, t1, stride=1, select="state", moments=False, groups=None, probs=(), n_groups=None, chain_offset=0):
    """what smm_get_trace returns, from a HistoryBuffers of iterations [0, >= t1); groups None: every chain in group 0"""
    N = h.params.shape[2]
    select = SELECT[select] if isinstance(select, str) else int(select)
    groups = np.zeros(N, np.int32) if groups is None else np.asarray(groups, np.int32)
    G = (int(groups.max()) + 1 if len(groups) else 0) if n_groups is None else int(n_groups)
    probs = [float(p) for p in probs]
    nq, nt = len(probs), n_rows(t0, t1, stride)
    F = fields(h, moments)
    S = F.shape[0]
    ts = t0 + np.arange(nt) * stride
    out = dict(iter=ts.astype(np.int32), n_chains=np.zeros(G, np.int32), count=np.zeros((nt, G), np.int32),
               n_accepted=np.zeros((nt, G), np.int32), n_exchanged=np.zeros((nt, G), np.int32), n_failed=np.zeros((nt, G), np.int32),
               mean=np.full((nt, G, S), np.nan), var=np.full((nt, G, S), np.nan), median=np.full((nt, G, S), np.nan),
               quantile=np.full((nq, nt, G, S), np.nan), best_value=np.full((nt, G), np.nan), best_chain=np.zeros((nt, G), np.int32))
    a = state_rows(h.accepted, t1) if select == 2 else None
    for g in range(G):
        mem = np.flatnonzero(groups == g)
        mg = len(mem)
        out["n_chains"][g] = mg
        if nt == 0 or mg == 0:
            continue
        acc = h.accepted[ts][:, mem] != 0
        ex = h.exchanged[ts][:, mem] != 0
        out["n_accepted"][:, g] = (acc & ~ex).sum(axis=1)
        out["n_exchanged"][:, g] = ex.sum(axis=1)
        out["n_failed"][:, g] = (h.status[ts][:, mem] < 0).sum(axis=1)
        v = np.ascontiguousarray(h.value[ts][:, mem])
        j = np.array([np.argmin(row) for row in v])               # the first NaN, else the first minimum
        out["best_value"][:, g] = v[np.arange(nt), j]
        out["best_chain"][:, g] = chain_offset + mem[j] + 1
        if select == 2:
            src = a[ts][:, mem]                                    # [nt][mg]
            V = np.where(src >= 0, F[:, np.maximum(src, 0), mem[None, :]], np.nan)
            take = np.ones((nt, mg), bool)
        else:
            V = F[:, ts][:, :, mem]
            take = acc if select == 1 else np.ones((nt, mg), bool)
        cnt = take.sum(axis=1)
        out["count"][:, g] = cnt
        for m in np.unique(cnt):
            I = np.flatnonzero(cnt == m)
            X = V[:, I][:, take[I]].reshape(S, len(I), m)          # row by row, the members in ascending local index
            mu, var, med, q = stacked_stats(X.reshape(S * len(I), m), probs)
            out["mean"][I, g, :] = mu.reshape(S, len(I)).T
            out["var"][I, g, :] = var.reshape(S, len(I)).T
            out["median"][I, g, :] = med.reshape(S, len(I)).T
            out["quantile"][:, I, g, :] = q.reshape(nq, S, len(I)).transpose(0, 2, 1)
    return out


def assert_trace_equal(got, want, fields=None):
    """every field array_equal, NaN equal to NaN"""
    for f in fields or want:
        a, b = np.asarray(got[f]), np.asarray(want[f])
        assert a.shape == b.shape, (f, a.shape, b.shape)
        if a.dtype.kind == "f":
            bad = ~((a == b) | (np.isnan(a) & np.isnan(b)))
            ok = np.array_equal(a, b, equal_nan=True)
        else:
            ok, bad = np.array_equal(a, b), a != b
        assert ok, (f, np.argwhere(bad)[:5], a[bad][:5], b[bad][:5])
