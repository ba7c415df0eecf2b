"""The numerical contract of smm_get_profile (include/smmhip.h) restated in numpy over a downloaded history: each group's pooled rows (the
members in ascending index, each in iteration order; every row, the accepted rows or the state series through trace_ref.state_rows) get
the bin of hist_ref's 1-D rule and the cell of its 2-D rule on hist_ref's own edges and statuses; a segment's scored rows (|value| <=
DBL_MAX) give chain_stats_ref.mean of the value and of every simulated moment as contiguous columns, and the first minimum of the value
with the row that attains it.  tests/test_profile.py holds it against np.histogram, np.histogram2d, np.mean and a plain loop; the GPU
tests hold the device against it, over the history downloaded with smm_get_history."""
import numpy as np

import chain_stats_ref as CS
import hist_ref as HR
import trace_ref as TR

SELECT = HR.SELECT
FIELDS1 = ("n", "n_scored", "v_min", "min_chain", "min_iter", "theta_at_min", "v_mean", "m_mean")
FIELDS2 = ("n2", "n_scored2", "v_min2", "min_chain2", "min_iter2", "v_mean2")
FIELDS = ("count", "status", "edges") + FIELDS1 + ("edges2",) + FIELDS2


def pooled_rows(h, t0, t1, select, groups, G):
    """per group (chain, t, src) of its pooled rows: the member's local index, the window iteration and the history row that supplies
    the parameters, the value and the moments (-1: a state row that does not exist yet)"""
    a = TR.state_rows(h.accepted, t1) if select == 2 else None
    out = []
    for g in range(G):
        cs, ts, ss = [], [], []
        for c in np.flatnonzero(groups == g):
            t = t0 + np.flatnonzero(h.accepted[t0:t1, c] != 0) if select == 1 else np.arange(t0, t1)
            cs.append(np.full(len(t), c, np.int64))
            ts.append(t.astype(np.int64))
            ss.append((a[t, c] if select == 2 else t).astype(np.int64))
        cat = lambda v: np.concatenate(v) if v else np.empty(0, np.int64)
        out.append((cat(cs), cat(ts), cat(ss)))
    return out


def bins_of(x, lo, hi, e, bins):
    """hist_ref.hist1d's index of every x, -1 where numpy drops it"""
    with np.errstate(invalid="ignore"):
        keep = (x >= lo) & (x <= hi)
    xs = x[keep]
    f = ((xs - lo) / (hi - lo)) * bins
    i = f.astype(np.int64)
    i[i == bins] = bins - 1
    i = i - (xs < e[i])
    i = i + ((xs >= e[i + 1]) & (i != bins - 1))
    out = np.full(len(x), -1, np.int64)
    out[keep] = i
    return out


def cells_of(x, y, ex, ey, B):
    """hist_ref.hist2d's cell of every (x, y), -1 outside"""
    i, j = HR.axis(x, ex, B), HR.axis(y, ey, B)
    ok = (i >= 1) & (i <= B) & (j >= 1) & (j <= B)
    return np.where(ok, (i - 1) * B + (j - 1), -1)


def scored(v):
    with np.errstate(invalid="ignore"):
        return np.abs(v) <= np.finfo(np.float64).max


def segments(seg, nseg, rows, h, chain_offset, moments):
    """the outputs of one axis: seg the segment of every pooled row (-1 none)"""
    c, t, s = rows
    npar, nm = h.params.shape[1], h.sim_moments.shape[1]
    o = dict(n=np.zeros(nseg, np.int64), n_scored=np.zeros(nseg, np.int64), v_min=np.full(nseg, np.nan), min_chain=np.zeros(nseg, np.int32),
             min_iter=np.zeros(nseg, np.int32), theta_at_min=np.full((nseg, npar), np.nan), v_mean=np.full(nseg, np.nan),
             m_mean=np.full((nseg, nm), np.nan))
    ok = s >= 0
    val = np.full(len(s), np.nan)
    val[ok] = h.value[s[ok], c[ok]]
    sc = scored(val)
    for b in np.unique(seg[seg >= 0]):
        idx = np.flatnonzero(seg == b)
        o["n"][b] = len(idx)
        idx = idx[sc[idx]]
        o["n_scored"][b] = len(idx)
        if not len(idx):
            continue
        v = val[idx]
        j = idx[int(np.argmin(v))]                        # the first minimum: -0 and +0 compare equal
        o["v_min"][b], o["min_chain"][b], o["min_iter"][b] = val[j], chain_offset + c[j] + 1, t[j] + 1
        o["theta_at_min"][b] = h.params[s[j], :, c[j]]
        o["v_mean"][b] = CS.mean(v)
        if moments:
            with np.errstate(invalid="ignore"):
                for k in range(nm):
                    o["m_mean"][b, k] = CS.mean(h.sim_moments[s[idx], k, c[idx]])
    return o


def profile_from_history(h, t0, t1, select, groups, bins, range=None, pairs=(), bins2=None, n_groups=None, chain_offset=0, moments=True):
    """what smm_get_profile returns, from a HistoryBuffers of iterations [0, >= t1); groups None: every chain in group 0"""
    N, npar, nm = h.params.shape[2], h.params.shape[1], h.sim_moments.shape[1]
    select = SELECT[select] if isinstance(select, str) else int(select)
    groups = np.zeros(N, np.int32) if groups is None else np.asarray(groups, np.int32)
    G = (int(groups.max()) + 1 if len(groups) else 0) if n_groups is None else int(n_groups)
    B2 = bins if bins2 is None else bins2
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    hs = HR.histogram_from_history(h, t0, t1, select, groups, bins, range, pairs, B2, n_groups=G)
    out = dict(count=hs["count"], status=hs["status"], edges=hs["edges"])
    shape = dict(theta_at_min=(npar,), m_mean=(nm,))
    for f in FIELDS1:
        out[f] = np.empty((G, npar, bins) + shape.get(f, ()), np.int64 if f in ("n", "n_scored") else np.int32 if "min_" in f else np.float64)
    if len(pairs):
        out["edges2"] = hs["edges2"]
        for f in FIELDS2:
            out[f] = np.empty((G, len(pairs), B2, B2), np.int64 if f in ("n2", "n_scored2") else np.int32 if "min_" in f else np.float64)
    rows = pooled_rows(h, t0, t1, select, groups, G)
    for g, (c, t, s) in enumerate(rows):
        x = np.full((npar, len(s)), np.nan)
        x[:, s >= 0] = h.params[s[s >= 0], :, c[s >= 0]].T
        for k in np.arange(npar):
            seg = np.full(len(s), -1, np.int64)
            if hs["status"][g, k] == 0:
                seg = bins_of(x[k], hs["lo"][g, k], hs["hi"][g, k], hs["edges"][g, k], bins)
            o = segments(seg, bins, (c, t, s), h, chain_offset, moments)
            for f in FIELDS1:
                out[f][g, k] = o[f]
        for p, (a, b) in enumerate(pairs):
            seg = np.full(len(s), -1, np.int64)
            if hs["status"][g, a] in (0, 3) and hs["status"][g, b] in (0, 3):
                with np.errstate(invalid="ignore"):
                    seg = cells_of(x[a], x[b], hs["edges2"][g, a], hs["edges2"][g, b], B2)
            o = segments(seg, B2 * B2, (c, t, s), h, chain_offset, False)
            for f in FIELDS2:
                out[f][g, p] = o[f[:-1]].reshape(B2, B2)
    if not moments:
        del out["m_mean"]
    return out


def assert_profile_equal(got, want, fields=None):
    """every field array_equal, NaN equal to NaN (the sign of a zero in an autodetected edge aside, as in hist_ref)"""
    for f in fields or want:
        a, b = np.asarray(got[f]), np.asarray(want[f])
        assert a.shape == b.shape, (f, a.shape, b.shape)
        if a.dtype.kind == "f":
            ok = np.array_equal(a, b, equal_nan=True)
            if ok and f not in ("edges", "edges2"):
                ok = np.array_equal(np.signbit(a[~np.isnan(a)]), np.signbit(b[~np.isnan(b)]))
            bad = ~((a == b) | (np.isnan(a) & np.isnan(b)))
        else:
            ok, bad = np.array_equal(a, b), a != b
        assert ok, (f, np.argwhere(bad)[:5])
