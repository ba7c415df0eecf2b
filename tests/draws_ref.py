"""The selection contract of smm_get_draws (include/smmhip.h) restated in numpy over a downloaded history: a Python loop over groups and
members.  Select 0 and 1 take each chain's rows as chain_cov_ref.select takes them (every row; the rows with accepted != 0), select 2
the carry-forward rows of chain_diag_ref.series_from_history (a(t), the last accepted row at or before t, looking back before t0).
Per-chain thinning, pooling in ascending local index and the cap's positions (j * m) // K are Python integers.  Nothing is computed on
a value: the rows are indexed out of the history.  tests/test_draws.py holds it against a brute-force list of tuples; the GPU tests
hold the device against it, over the history downloaded with smm_get_history."""
import numpy as np

SELECT = {"all": 0, "accepted": 1, "state": 2}
FIELDS = ("count", "n_chains", "row0", "params", "value", "sim_moments", "chain", "iter", "src_iter")


def positions(m, K):
    """the pooled positions written for a group of m kept rows under the cap K"""
    return list(range(m)) if m <= K else [(j * m) // K for j in range(K)]


def chain_rows(accepted, t0, t1, select):
    """(t [m_c], src [m_c]) of one chain's selected rows of the window in iteration order (accepted [>= t1]; src -1: no state yet)"""
    acc = np.asarray(accepted)[:t1] != 0
    if select == 1:
        t = t0 + np.flatnonzero(acc[t0:t1])
        return t, t
    t = np.arange(t0, t1)
    if select == 0:
        return t, t
    a = np.maximum.accumulate(np.where(acc, np.arange(t1), -1))[t0:t1] if t1 > 0 else np.empty(0, np.int64)
    return t, a   # (chain_diag_ref.series_from_history's a)


def draws_from_history(h, t0, t1, select=1, groups=None, thin=1, max_rows=10000, n_groups=None, chain_offset=0):
    """what smm_get_draws returns, from a HistoryBuffers of iterations [0, >= t1); groups None: every chain in group 0"""
    N, npar, nm = h.params.shape[2], h.params.shape[1], h.sim_moments.shape[1]
    select = SELECT[select] if isinstance(select, str) else int(select)
    groups = np.zeros(N, np.int32) if groups is None else np.asarray(groups, np.int32)
    G = (int(groups.max()) + 1 if len(groups) else 0) if n_groups is None else int(n_groups)
    thin, K = int(thin), int(max_rows)
    count, n_chains, row0 = np.zeros(G, np.int64), np.zeros(G, np.int32), np.zeros(G + 1, np.int64)
    cs, ts, ss = [], [], []
    for g in range(G):
        pc, pt, ps = [], [], []
        for c in np.flatnonzero(groups == g):
            t, src = chain_rows(h.accepted[:, c], t0, t1, select)
            pc += [int(c)] * len(t[::thin])
            pt += [int(v) for v in t[::thin]]
            ps += [int(v) for v in src[::thin]]
        m = len(pt)
        count[g], n_chains[g] = m, int((groups == g).sum())
        pos = positions(m, K)
        row0[g + 1] = row0[g] + len(pos)
        cs += [pc[p] for p in pos]
        ts += [pt[p] for p in pos]
        ss += [ps[p] for p in pos]
    c, t, s = np.asarray(cs, np.int64), np.asarray(ts, np.int64), np.asarray(ss, np.int64)
    ok = s >= 0
    R = len(c)
    params, value, mom = np.full((R, npar), np.nan), np.full(R, np.nan), np.full((R, nm), np.nan)
    params[ok] = h.params[s[ok], :, c[ok]]
    value[ok] = h.value[s[ok], c[ok]]
    mom[ok] = h.sim_moments[s[ok], :, c[ok]]
    return dict(count=count, n_chains=n_chains, row0=row0, params=params, value=value, sim_moments=mom,
                chain=(c + 1 + chain_offset).astype(np.int32), iter=(t + 1).astype(np.int32), src_iter=(s + 1).astype(np.int32))


def assert_draws_equal(got, want, fields=FIELDS):
    """every field equal; the doubles bit for bit (NaNs by their bits)"""
    for f in fields:
        a, b = np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f])
        assert a.shape == b.shape and a.dtype == b.dtype, (f, a.shape, b.shape, a.dtype, b.dtype)
        if a.dtype.kind == "f":
            a, b = a.view(np.uint64), b.view(np.uint64)
        assert np.array_equal(a, b), (f, np.argwhere(a != b)[:5])
