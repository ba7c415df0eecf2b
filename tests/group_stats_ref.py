"""The numerical contract of smm_get_group_stats (include/smmhip.h) restated in numpy: a group's pooled column is the concatenation of its
members' compacted columns (chain_cov_ref.select), summarised by the chain-stats order statistics (chain_stats_ref) and the chain-cov
mean and covariance (chain_cov_ref.column_cov).  tests/test_group_stats.py holds it against numpy itself; the GPU tests hold the device
against it, over the history downloaded with smm_get_history."""
import numpy as np

import chain_cov_ref as V
import chain_stats_ref as R


def pooled_columns(cols, groups, n_groups, npar):
    """the pooled column [np][m_g] of every group from the members' compacted columns cols [N] of [np][m_c], members in ascending index"""
    out = []
    for g in range(n_groups):
        mem = [cols[c] for c in range(len(cols)) if groups[c] == g]
        out.append(np.ascontiguousarray(np.concatenate(mem, axis=1)) if mem else np.empty((npar, 0)))
    return out


def column_cov(x):
    """(mean [np], cov [np][np]) of one pooled column x [np][m]: chain_cov_ref.column_cov, with S(d_j * d_k) summed pair by pair as np.sum
    of the contiguous product (the chunked pairwise sum bit for bit: test_group_stats.py) to keep long columns within memory"""
    npar, m = x.shape
    mean = V.chunked_sum(x) / m if m else np.full(npar, np.nan)
    if m < 2:
        return mean, np.full((npar, npar), np.nan)
    d = x - mean[:, None]
    cov = np.empty((npar, npar))
    for j in range(npar):
        for k in range(j + 1):
            cov[j, k] = cov[k, j] = np.sum(np.ascontiguousarray(d[j] * d[k])) / (m - 1)
    return mean, cov


def order_stats(x, probs):
    """(median, [quantile(p)]) of one pooled column of one parameter: the chain-stats order statistics"""
    if len(x) == 0 or np.isnan(x).any():
        return np.nan, [np.nan] * len(probs)
    s = R.total_sort(x)
    return R.median(s), [R.quantile(s, float(p)) for p in probs]


def group_stats_from_history(h, t0, t1, accepted_only, groups, probs, n_groups=None):
    """what smm_get_group_stats returns, computed from a HistoryBuffers of iterations [0, >= t1); groups None: every chain in group 0;
    n_groups defaults to groups.max() + 1"""
    N, npar = h.value.shape[1], h.params.shape[1]
    groups = np.zeros(N, np.int32) if groups is None else np.asarray(groups, np.int32)
    G = (int(groups.max()) + 1 if len(groups) else 0) if n_groups is None else int(n_groups)
    probs = [float(p) for p in probs]
    cols = pooled_columns(V.select(h.params, h.accepted, t0, t1, accepted_only), groups, G, npar)
    out = dict(count=np.array([x.shape[1] for x in cols], np.int64), n_chains=np.array([(groups == g).sum() for g in range(G)], np.int32),
               mean=np.empty((G, npar)), median=np.empty((G, npar)), quantile=np.empty((len(probs), G, npar)), cov=np.empty((G, npar, npar)))
    with np.errstate(invalid="ignore", divide="ignore"):
        for g, x in enumerate(cols):
            out["mean"][g], out["cov"][g] = column_cov(x)
            for k in range(npar):
                out["median"][g, k], out["quantile"][:, g, k] = order_stats(x[k], probs)
    return out


def assert_group_stats_equal(got, want, fields=None):
    """every field bit for bit, NaN equal to NaN"""
    for f in fields or want:
        a, b = np.asarray(got[f]), np.asarray(want[f])
        assert a.shape == b.shape, (f, a.shape, b.shape)
        ok = np.array_equal(a, b, equal_nan=True) if a.dtype.kind == "f" else np.array_equal(a, b)
        assert ok, (f, np.argwhere(~((a == b) | (np.isnan(a) & np.isnan(b))) if a.dtype.kind == "f" else a != b)[:5])
