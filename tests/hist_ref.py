"""The numerical contract of smm_get_histogram (include/smmhip.h) restated in numpy: each group's column is selected as the other readers
select it (chain_cov_ref.select for "all" / "accepted", chain_diag_ref.series_from_history for the state series) and pooled as
group_stats_ref.pooled_columns pools it; then numpy's outer edges with their status codes, numpy's linspace, the uniform-bins index
step by step, and histogramdd's searchsorted.  tests/test_histogram.py holds it against np.histogram, np.histogram2d and np.linspace
themselves; the GPU tests hold the device against it, over the history downloaded with smm_get_history."""
import numpy as np

import chain_cov_ref as V
import chain_diag_ref as D
import group_stats_ref as GR

SELECT = {"all": 0, "accepted": 1, "state": 2}


def columns(h, t0, t1, select, groups, n_groups):
    """the pooled column [np][m_g] of every group (select 0 all rows, 1 accepted rows, 2 the state series)"""
    npar, N = h.params.shape[1], h.params.shape[2]
    if select == 2:
        X, _ = D.series_from_history(h, t0, t1)
        cols = [np.ascontiguousarray(X[:npar, c, :]) for c in range(N)]
    else:
        cols = V.select(h.params, h.accepted, t0, t1, select == 1)
    return GR.pooled_columns(cols, groups, n_groups, npar)


def outer_edges(x, rng=None):
    """(lo, hi, status) of one column: numpy's _get_outer_edges, status 1 where it raises on an autodetected range, 2 for a width
    that is not finite"""
    if rng is not None:
        lo, hi = float(rng[0]), float(rng[1])
    elif len(x) == 0:
        lo, hi = 0.0, 1.0
    elif not np.isfinite(x).all():
        return np.nan, np.nan, 1
    else:
        lo, hi = float(x.min()), float(x.max())
    if lo == hi:
        lo, hi = lo - 0.5, hi + 0.5
    with np.errstate(over="ignore"):
        if not np.isfinite(hi - lo):
            return lo, hi, 2
    return lo, hi, 0


def linspace(lo, hi, b):
    """numpy's linspace(lo, hi, b + 1), each operation rounded on its own"""
    delta = hi - lo
    step = delta / b
    i = np.arange(b + 1, dtype=np.float64)
    e = i * step + lo if step != 0 else (i / b) * delta + lo
    e[b] = hi
    return e


def hist1d(x, lo, hi, e, bins):
    """numpy 2.x histogram's uniform-bins path, step by step"""
    x = x[(x >= lo) & (x <= hi)]
    f = ((x - lo) / (hi - lo)) * bins
    i = f.astype(np.int64)
    i[i == bins] = bins - 1
    i = i - (x < e[i])
    i = i + ((x >= e[i + 1]) & (i != bins - 1))
    return np.bincount(i, minlength=bins).astype(np.int64)


def axis(x, e, B):
    """histogramdd's index on one axis: searchsorted right (NaN last), the last edge moved into the last bin; 1 .. B inside"""
    i = np.searchsorted(e, x, side="right")
    i[x == e[B]] -= 1
    return i


def hist2d(x, y, ex, ey, B):
    i, j = axis(x, ex, B), axis(y, ey, B)
    ok = (i >= 1) & (i <= B) & (j >= 1) & (j <= B)
    return np.bincount((i[ok] - 1) * B + (j[ok] - 1), minlength=B * B).reshape(B, B).astype(np.int64)


def histogram_from_history(h, t0, t1, select, groups, bins, range=None, pairs=(), bins2=None, n_groups=None):
    """what smm_get_histogram returns, from a HistoryBuffers of iterations [0, >= t1); groups None: every chain in group 0"""
    N, npar = h.params.shape[2], h.params.shape[1]
    select = SELECT[select] if isinstance(select, str) else int(select)
    groups = np.zeros(N, np.int32) if groups is None else np.asarray(groups, np.int32)
    G = (int(groups.max()) + 1 if len(groups) else 0) if n_groups is None else int(n_groups)
    B2 = bins if bins2 is None else bins2
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    cols = columns(h, t0, t1, select, groups, G)
    out = dict(count=np.array([x.shape[1] for x in cols], np.int64), status=np.zeros((G, npar), np.int32), lo=np.empty((G, npar)),
               hi=np.empty((G, npar)), edges=np.empty((G, npar, bins + 1)), hist=np.zeros((G, npar, bins), np.int64))
    if len(pairs):
        out.update(edges2=np.empty((G, npar, B2 + 1)), hist2=np.zeros((G, len(pairs), B2, B2), np.int64))
    with np.errstate(invalid="ignore", over="ignore"):
        for g, x in enumerate(cols):
            for k in np.arange(npar):
                lo, hi, st = outer_edges(x[k], None if range is None else range[k])
                out["lo"][g, k], out["hi"][g, k] = lo, hi
                ok = st == 0
                e = linspace(lo, hi, bins) if ok else np.full(bins + 1, np.nan)
                if ok and np.any(e[:-1] >= e[1:]):
                    st = 3
                out["status"][g, k], out["edges"][g, k] = st, e
                if st == 0:
                    out["hist"][g, k] = hist1d(x[k], lo, hi, e, bins)
                if len(pairs):
                    out["edges2"][g, k] = linspace(lo, hi, B2) if ok else np.nan
            for p, (a, b) in enumerate(pairs):
                if out["status"][g, a] in (0, 3) and out["status"][g, b] in (0, 3):
                    out["hist2"][g, p] = hist2d(x[a], x[b], out["edges2"][g, a], out["edges2"][g, b], B2)
    return out


def assert_histogram_equal(got, want, auto=True, fields=None):
    """every field bit for bit, NaN equal to NaN; the sign of a zero is compared except in autodetected lo, hi and edges (auto)"""
    for f in fields or want:
        a, b = np.asarray(got[f]), np.asarray(want[f])
        assert a.shape == b.shape, (f, a.shape, b.shape)
        if a.dtype.kind == "f":
            ok = np.array_equal(a, b, equal_nan=True)
            if ok and not auto:
                ok = np.array_equal(np.signbit(a), np.signbit(b))
            bad = ~((a == b) | (np.isnan(a) & np.isnan(b)))
        else:
            ok, bad = np.array_equal(a, b), a != b
        assert ok, (f, np.argwhere(bad)[:5])
