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


# the crafted history of the segment-cap cases (tests/test_gpu_reducer_caps.py; its design is checked in tests/test_profile.py): serialNormal's
# np = nm = 2, T = 600 (three 256-row blocks of k_prof_scatter per member), group 2 of 14 members so that one segment of it holds more
# than 8192 scored rows, group 4 without a member and chain 5 in no group
CAPS_T = 600
CAPS_GROUPS = np.array([0, 0, 0, 1, 1, -1, 2, 2, 2, 2, 3, 0] + [2] * 10, np.int32)
CAPS_NG = 5
CAPS_RANGE = np.array([[0.0, 1.0], [0.0, 1.0]])
CAPS_BINS = (2, 3, 7)                 # every bins / bins2 the cases bin CAPS_RANGE into: rows lie on all their edges
CAPS_MIN = (7, 10)                    # (chain, iteration) of the first of group 2's equal minima in pooled order


def crafted_caps(h, seed=11):
    """h (a HistoryBuffers of CAPS_T iterations of len(CAPS_GROUPS) chains, np = nm = 2) overwritten in params, sim_moments, value,
    accepted and status, a function of the seed alone:
      every chain : x uniform in [-0.05, 1.05] (rows outside CAPS_RANGE), the value 1 + |normal|, accepted at rate 0.6, row 0 accepted;
      group 2     : x = (0.4, 0.6) but for 8 rows per member: one segment (1-D) and one cell (2-D) of at least 8260 scored rows, every
                    member adding to it in each of its three blocks; the value -3 (the minimum) at chain 7's rows 10 and 300 (two blocks
                    of one member) and at chain 13's rows 5 and 400: the earliest pooled row is CAPS_MIN; chain 7's row 10 is not
                    accepted, so the accepted rows' minimum is at row 300; two unscored rows per member (NaN, +Inf);
      group 0     : unscored rows (NaN, -Inf, a failed evaluation: +Inf with status -1), a NaN moment in a scored row, and x = (0.9,
                    0.1) with the values -0.0 at chain 0's row 20 and +0.0 at chain 1's row 450: -0.0 comes first;
      group 3     : x = (0.9, 0.1) with +0.0 at row 7 and -0.0 at row 300: +0.0 comes first;
      chain 3     : x walks over every edge of CAPS_RANGE cut into CAPS_BINS bins, lo and hi included, in both parameters."""
    import hist_ref as HR
    T, N = h.value.shape
    assert T == CAPS_T and N == len(CAPS_GROUPS) and h.params.shape[1] == 2 and h.sim_moments.shape[1] == 2
    rng = np.random.default_rng(seed)
    h.params[...] = rng.uniform(-0.05, 1.05, (T, 2, N))
    h.sim_moments[...] = rng.standard_normal((T, 2, N))
    h.value[...] = 1.0 + np.abs(rng.standard_normal((T, N)))
    h.accepted[...] = rng.random((T, N)) < 0.6
    h.accepted[0] = 1
    h.status[...] = 0
    for c in np.flatnonzero(CAPS_GROUPS == 2):
        away = rng.choice(np.arange(20, T), 10, replace=False)
        keep = np.ones(T, bool)
        keep[away[:8]] = False
        h.params[keep, 0, c], h.params[keep, 1, c] = 0.4, 0.6
        h.value[away[8], c], h.value[away[9], c] = np.nan, np.inf                 # (in the big segment: x stays (0.4, 0.6) there)
    for c, t in ((7, 10), (7, 300), (13, 5), (13, 400)):
        h.params[t, :, c], h.value[t, c], h.accepted[t, c] = (0.4, 0.6), -3.0, 1
    h.accepted[10, 7] = 0
    h.value[30, 0], h.value[31, 1], h.value[290, 2] = np.nan, -np.inf, np.nan
    h.value[40, 11], h.status[40, 11] = np.inf, -1
    h.value[33, 2], h.sim_moments[33, 0, 2], h.params[33, :, 2] = 1.5, np.nan, (0.5, 0.5)
    for c, t, z in ((0, 20, -0.0), (1, 450, 0.0), (10, 7, 0.0), (10, 300, -0.0)):
        h.params[t, :, c], h.value[t, c], h.accepted[t, c] = (0.9, 0.1), z, 1
    E = np.concatenate([HR.linspace(0.0, 1.0, b) for b in CAPS_BINS])
    t = np.arange(1, T)
    h.params[1:, 0, 3], h.params[1:, 1, 3] = E[t % len(E)], E[(t // len(E)) % len(E)]
    return h


def crafted_wide(h, seed=12):
    """h (np = nm = 64 and the like: any sizes) overwritten in params, sim_moments, value, accepted and status: x uniform in [0, 1],
    standard normal moments, the value 1 + |normal| with a NaN, an Inf and a pair of equal minima in every chain, accepted at rate
    0.6 with row 0 accepted"""
    T, N = h.value.shape
    rng = np.random.default_rng(seed)
    h.params[...] = rng.uniform(0.0, 1.0, h.params.shape)
    h.sim_moments[...] = rng.standard_normal(h.sim_moments.shape)
    h.value[...] = 1.0 + np.abs(rng.standard_normal((T, N)))
    h.accepted[...] = rng.random((T, N)) < 0.6
    h.accepted[0] = 1
    h.status[...] = 0
    for c in range(N):
        t = rng.choice(T, 4, replace=False)
        h.value[t[0], c], h.value[t[1], c], h.value[t[2], c], h.value[t[3], c] = np.nan, np.inf, 0.25, 0.25
    return h


def zeroed_history(T, N, npar, nm):
    """a HistoryBuffers with every field 0, for a generator to write into without a context"""
    from smm_jl_amd import _abi as A
    h = A.HistoryBuffers(T, N, npar, nm)
    for f in A.HistoryBuffers.FIELDS:
        getattr(h, f)[...] = 0
    return h


CRAFTED_FIELDS = ("params", "sim_moments", "value", "accepted")


def assert_crafted_read_back(back, crafted):
    """the four fields a generator writes, as smm_get_history returns them after smm_set_state: bit for bit"""
    for f in CRAFTED_FIELDS:
        a, b = getattr(back, f), getattr(crafted, f)
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), f
    assert np.array_equal(np.signbit(back.value), np.signbit(crafted.value))


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
