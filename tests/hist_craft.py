"""Histories whose draws ride the bin edges, for smm_get_histogram and smm_get_profile (tests/test_gpu_hist_edges.py on the device;
tests/test_hist_craft.py checks the design here, without a GPU).  numpy's uniform-bins index truncates ((x - lo) / (hi - lo)) bins and
then corrects by one where x < e[i] or x >= e[i + 1]: the corrections fire only for draws on an edge or one ulp beside it, and only
where the range is awkward in binary, so random draws never take them.  The builders overwrite a history's params so that every group
jointly holds, for each parameter and each bins of the case, the riders of HR.linspace(lo, hi, bins): every edge, its two np.nextafter
neighbours, lo and hi (given ranges: the two values one ulp outside too; autodetected ranges: nothing outside, so that the data's min
and max are lo and hi).  Every chain holds lo, hi and, per bins, one rider that steps down, one that steps up, an interior edge and a
value one ulp below an edge in accepted rows inside every window (the core rows), so that every group, selection and window takes each
branch of the 1-D index and each boundary rule of the 2-D one; the other riders are dealt round
robin over the group's chains and iterations, those that fire a correction first.  branch_counts / cell_counts restate the indexes
step by step and say how many draws went which way.

Which ranges fire what (the riders of the whole table, `fires`): of RANGE_PAIRS' first ranges all step down at bins = 2, 7 and 64; of the
second ranges all step up at bins = 2 and 64; at bins = 7 the pairs' up comes from the first range but for pairs 1 and 5, where it comes
from the second.  (-1/3, 2/3) never steps up at 64 bins, (0.7, 1.6) never steps down below 1000: they are paired with one that does.
With bins = 1 there is no step up and no step down."""
import numpy as np

import hist_ref as HR

# (range of parameter 0, range of parameter 1): a group's pair; together they step down and up at every bins > 1 of SMALL_BINS
RANGE_PAIRS = (((-1 / 3, 2 / 3), (0.3, 2.2)), ((-0.7, 0.9), (0.7, 1.6)), ((-2.3, 1.9), (-1.9, -0.3)), ((-0.6, 1.3), (-2.7, -1.2)),
               ((-0.45, 0.35), (0.3, 2.2)), ((-3.3, 4.1), (0.7, 1.6)))
SELECTIONS = ("all", "accepted", "state")


def riders(lo, hi, bins, outside):
    """every edge of linspace(lo, hi, bins + 1) and its two neighbours; outside False: without the two values beyond lo and hi"""
    e = HR.linspace(lo, hi, bins)
    v = np.concatenate([e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf)])
    return v if outside else v[(v >= lo) & (v <= hi)]


def branches(x, lo, hi, bins):
    """masks over x of the steps of numpy's uniform-bins index (hist_ref.hist1d): dropped below / above / as NaN, clamped from
    i == bins, stepped down, stepped up; and the index (-1: dropped)"""
    x = np.asarray(x, np.float64)
    e = HR.linspace(lo, hi, bins)
    with np.errstate(invalid="ignore"):
        nan, below, above = np.isnan(x), x < lo, x > hi
    keep = ~(nan | below | above)
    xs = x[keep]
    i = (((xs - lo) / (hi - lo)) * bins).astype(np.int64)
    clamped = i == bins
    i[clamped] = bins - 1
    down = xs < e[i]
    i = i - down
    up = (xs >= e[i + 1]) & (i != bins - 1)
    i = i + up
    out = dict(below=below, above=above, nan=nan)
    for name, m in (("clamped", clamped), ("down", down), ("up", up)):
        out[name] = np.zeros(len(x), bool)
        out[name][keep] = m
    out["index"] = np.full(len(x), -1, np.int64)
    out["index"][keep] = i
    return out


def branch_counts(x, lo, hi, bins):
    """how many draws of x were dropped below, dropped above, dropped as NaN, clamped, stepped down and stepped up"""
    m = branches(x, lo, hi, bins)
    return {k: int(v.sum()) for k, v in m.items() if k != "index"}


def fires(lo, hi, bins):
    """(down, up): whether any rider of the whole table steps down / up"""
    c = branch_counts(riders(lo, hi, bins, False), lo, hi, bins)
    return c["down"] > 0, c["up"] > 0


def axis_masks(x, e, B):
    """masks over x of histogramdd's boundary cases on one axis: equal to e[B] (moved into the last cell), equal to an interior edge
    (e[m] <= x goes right), one ulp below an edge, outside, NaN"""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        nan, outside = np.isnan(x), (x < e[0]) | (x > e[B])
    return dict(last=x == e[B], inner=np.isin(x, e[1:B]), below=np.isin(x, np.nextafter(e[1:], -np.inf)) & ~outside, outside=outside, nan=nan)


def cell_counts(x, y, ex, ey, B):
    """the 2-D analogue: per axis the draws on e[B], on an interior edge and one ulp below an edge among the rows whose other
    coordinate is inside (so the row has a cell), and the rows outside or NaN in either"""
    mx, my = axis_masks(x, ex, B), axis_masks(y, ey, B)
    inx, iny = ~(mx["outside"] | mx["nan"]), ~(my["outside"] | my["nan"])
    out = dict(outside=int((mx["outside"] | my["outside"]).sum()), nan=int((mx["nan"] | my["nan"]).sum()))
    for ax, m, other in (("x", mx, iny), ("y", my, inx)):
        for k in ("last", "inner", "below"):
            out[ax + "_" + k] = int((m[k] & other).sum())
    return out


def n_core(bset, outside):
    return 2 + 2 * bool(outside) + 4 * len(bset)


def deal(h, chains, k, lo, hi, bset, outside, core0):
    """params[:, k, chains] overwritten.  The core rows core0 .. core0 + n_core(bset, outside) of every chain hold lo, hi, with outside
    the two values one ulp beyond them, and per bins of bset a rider that steps down, one that steps up (an interior rider where
    none does), an interior edge and a value one ulp below an edge, cycled over the chains.  The other rows hold the riders of every
    bins of bset, those that fire first, round robin over the chains and then the iterations, cycled when they run out and cut when
    the rows do"""
    T, nc = h.params.shape[0], len(chains)
    V = [riders(lo, hi, b, outside) for b in bset]
    every = np.unique(np.concatenate(V))
    fire = []
    for b, v in zip(bset, V):
        m = branches(v, lo, hi, b)
        fire.append((v[m["down"]], v[m["up"]]))
    firing = np.unique(np.concatenate([f for du in fire for f in du]))
    order = np.concatenate([firing, np.setdiff1d(every, firing)])
    nco = n_core(bset, outside)
    assert 0 < core0 and core0 + nco <= T
    inner = every[(every > lo) & (every < hi)]
    for ci, c in enumerate(chains):
        col = [lo, hi] + ([np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)] if outside else [])
        for j, (dn, up) in enumerate(fire):
            fill = inner[(ci + j) % len(inner)] if len(inner) else lo
            col += [dn[ci % len(dn)] if len(dn) else fill, up[ci % len(up)] if len(up) else fill]
            e = HR.linspace(lo, hi, bset[j])                   # for the cells: an interior edge, and one ulp below an edge
            col += [e[1 + ci % (bset[j] - 1)] if bset[j] > 1 else fill, np.nextafter(e[1 + ci % bset[j]], -np.inf)]
        h.params[core0:core0 + nco, k, c] = col
    free = np.array([t for t in range(T) if not core0 <= t < core0 + nco])
    s = np.arange(len(free) * nc)
    h.params[free[s // nc], k, np.asarray(chains)[s % nc]] = order[s % len(order)]
    return h


def craft_accepted(h, bset, outside, core0, seed, late=()):
    """accepted at rate 0.6, the core rows and row 0 accepted; the chains of late not before row 3 (their state series starts NaN)"""
    rng = np.random.default_rng(seed)
    h.accepted[...] = rng.random(h.accepted.shape) < 0.6
    h.accepted[0] = 1
    h.accepted[core0:core0 + n_core(bset, outside)] = 1
    for c in late:
        h.accepted[:3, c] = 0
    return h


def distinct_values(h):
    """the value of every row distinct and finite, scattered over chains and iterations: a row in the neighbouring bin moves that
    bin's v_min, min_iter and v_mean"""
    T, N = h.value.shape
    i = np.arange(T * N).reshape(T, N)
    h.value[...] = 1.0 + ((i * 7919) % (T * N)) / (T * N)
    h.status[...] = 0
    return h


# --- the small-bins cases: np = 2, N = 16, T = 64 -------------------------------------------------------------------------------------

SMALL_N, SMALL_T, SMALL_CORE0 = 16, 64, 24
SMALL_BINS, SMALL_BINS2 = (1, 2, 7, 64), (1, 5, 64)
SMALL_BSET = (1, 2, 5, 7, 64)
SMALL_CALL_BINS = ((1, 1), (2, 5), (7, 64), (64, 5))      # (bins, bins2) of a call: every bins and every bins2 once or more
SMALL_PAIRS = [(0, 1), (1, 0), (0, 0)]
SMALL_WINDOWS = ((0, SMALL_T), (19, 61))                   # both hold the core rows
_g4 = (np.arange(SMALL_N) // 4).astype(np.int32)
_g4[_g4 == 3] = 4                                          # group 3 without a member
_g4[7] = -1                                                # a chain in no group
GROUPINGS = dict(chain=(np.arange(SMALL_N, dtype=np.int32), SMALL_N), four=(_g4, 5), all=(np.zeros(SMALL_N, np.int32), 1))
SMALL_CASES = ("given", "auto-chain", "auto-four", "auto-all")
SMALL_GIVEN = np.array(RANGE_PAIRS[0])                     # the given ranges [np][2]


def small_ranges(case, g):
    """the ranges [2][2] that group g of the case bins into"""
    return SMALL_GIVEN if case == "given" else np.array(RANGE_PAIRS[g % len(RANGE_PAIRS)])


def small_groupings(case):
    return tuple(GROUPINGS) if case == "given" else (case[5:],)


def small_history(h, case):
    """h (np = 2, SMALL_T iterations of SMALL_N chains) crafted for the case.  given: every chain rides SMALL_GIVEN, with the values one
    ulp outside, a NaN, a +inf and a -inf row per parameter and two chains whose state series starts NaN.  auto-<grouping>: each group
    of the grouping rides its own pair of ranges and holds nothing outside them"""
    assert h.params.shape == (SMALL_T, 2, SMALL_N)
    given = case == "given"
    groups, G = GROUPINGS["all" if given else case[5:]]
    h.params[...] = 0.5                                    # (a chain in no group: inside every range, never read)
    for g in range(G):
        mem = np.flatnonzero(groups == g)
        if len(mem):
            for k in range(2):
                lo, hi = small_ranges(case, g)[k]
                deal(h, mem, k, lo, hi, SMALL_BSET, given, SMALL_CORE0)
    craft_accepted(h, SMALL_BSET, given, SMALL_CORE0, 5, late=(1, 9) if given else ())
    if given:
        for k in range(2):
            h.params[3 + k, k, 2], h.params[7 + k, k, 5], h.params[11 + k, k, 14] = np.nan, np.inf, -np.inf
            h.accepted[3 + k, 2] = h.accepted[7 + k, 5] = h.accepted[11 + k, 14] = 1
    return distinct_values(h)


def small_calls(case):
    """the calls of the case: (grouping, groups, n_groups, select, t0, t1, bins, bins2, range)"""
    for gname in small_groupings(case):
        groups, G = GROUPINGS[gname]
        for sel in SELECTIONS:
            for t0, t1 in SMALL_WINDOWS:
                for bins, bins2 in SMALL_CALL_BINS:
                    yield gname, groups, G, sel, t0, t1, bins, bins2, (SMALL_GIVEN if case == "given" else None)


# --- parameter and pair batches: np = 50, N = 32, T = 64, given ranges ------------------------------------------------------------------

WIDE_NP, WIDE_N, WIDE_T, WIDE_CORE0 = 50, 32, 64, 20
WIDE_BSET = (8, 64, 1000)
# even parameters straddle zero (they step down), odd ones lie above it (they step up)
WIDE_RANGE = np.array([(-0.7 - 0.11 * k, 0.9 + 0.07 * k) if k % 2 == 0 else (0.1 + 0.37 * k, 0.7 + 0.37 * k + 0.13 * (k % 7)) for k in range(WIDE_NP)])
WIDE_PAIRS = [(j, (j * 7) % 50) for j in range(50)] + [(3, 3)] * 30    # 80 pairs: two batches
WIDE_GROUPS = ((np.zeros(WIDE_N, np.int32), 1), ((np.arange(WIDE_N) // 4).astype(np.int32), 8))
WIDE_WINDOW = (0, WIDE_T)


def wide_history(h):
    """h (np = 50, WIDE_T iterations of WIDE_N chains): parameter k rides WIDE_RANGE[k] at bins 8, 64 and 1000 (3003 riders for 1984
    free rows: those that fire and the lowest of the rest), with the values one ulp outside"""
    assert h.params.shape == (WIDE_T, WIDE_NP, WIDE_N)
    for k in range(WIDE_NP):
        deal(h, np.arange(WIDE_N), k, WIDE_RANGE[k, 0], WIDE_RANGE[k, 1], WIDE_BSET, True, WIDE_CORE0)
    craft_accepted(h, WIDE_BSET, True, WIDE_CORE0, 6, late=(3,))
    return distinct_values(h)


# --- the shipped library's LDS limits: np = 2, N = 32, T = 512, one group, given ranges ------------------------------------------------

LIMIT_N, LIMIT_T, LIMIT_CORE0 = 32, 512, 100
LIMIT_RANGE = np.array(RANGE_PAIRS[1])
LIMIT_CASES = {4096: (4096, 123, 124), 5290: (5290,), 5291: (5291,), 65536: (65536,)}   # the history of a bins: the bins it rides


def limit_history(h, bins):
    """h (np = 2, LIMIT_T iterations of LIMIT_N chains) riding LIMIT_RANGE at LIMIT_CASES[bins]; at 65536 bins the first and last 64
    edges and every 16th between, with their neighbours"""
    assert h.params.shape == (LIMIT_T, 2, LIMIT_N)
    for k in range(2):
        lo, hi = LIMIT_RANGE[k]
        if bins == 65536:
            e = HR.linspace(lo, hi, bins)
            e = np.concatenate([e[:64], e[64:-64:16], e[-64:]])
            v = np.concatenate([e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf)])
            m = branches(v, lo, hi, bins)
            order = np.concatenate([v[m["down"] | m["up"]], v[~(m["down"] | m["up"])]])
            T, nc = LIMIT_T, LIMIT_N
            s = np.arange(T * nc)
            h.params[s // nc, k, s % nc] = order[s % len(order)]
            h.params[LIMIT_CORE0, k, :], h.params[LIMIT_CORE0 + 1, k, :] = lo, hi
        else:
            deal(h, np.arange(LIMIT_N), k, lo, hi, LIMIT_CASES[bins], True, LIMIT_CORE0)
    craft_accepted(h, LIMIT_CASES[bins], True, LIMIT_CORE0, 7, late=(3,))
    return distinct_values(h)


# --- statuses and degenerate tables: np = 2, N = 16, T = 64 ----------------------------------------------------------------------------

DENORMAL = (0.0, 1.5e-323)                                 # three denormal steps wide: linspace's step == 0 branch at 64 bins
DEGENERATE_GROUPS = (np.arange(SMALL_N) // 4).astype(np.int32)
DEGENERATE_BINS = ((64, 4), (1, 1))                        # (bins, bins2) of the calls with given ranges
# (given ranges [2][2], the statuses they give per bins): a finite range of infinite width; 64 bins over four doubles repeat edges, one
# bin does not; (-0.0, 0.0) becomes (-0.5, 0.5); 1e17 +- 0.5 is 1e17: even one bin has e[0] == e[1]
DEGENERATE_RANGES = ((np.array([(-1e308, 1e308), (-1.0, 1.0)]), {64: (2, 0), 1: (2, 0)}),
                     (np.array([DENORMAL, DENORMAL]), {64: (3, 3), 1: (0, 0)}),
                     (np.array([(-0.0, 0.0), (-0.0, 0.0)]), {64: (0, 0), 1: (0, 0)}),
                     (np.array([(1e17, 1e17), (2.5, 2.5)]), {64: (3, 0), 1: (3, 0)}))


def degenerate_history(h):
    """h (np = 2, SMALL_T iterations of SMALL_N chains), every row accepted but chain 2's odd ones; groups of four chains:
      group 0 : parameter 0 holds -1e308 and 1e308 (a finite range of infinite width: status 2), parameter 1 is 1e17 everywhere
                (lo == hi where +-0.5 does not move it: every edge equal, status 3, the one 2-D cell still counts);
      group 1 : parameter 0 is 1e16 + {0, .., 4} (64 bins: repeated edges, status 3, the draws on them), parameter 1 rides RANGE_PAIRS[2];
      group 2 : parameter 0 holds the four doubles of DENORMAL, parameter 1 holds -0.0 and +0.0 only;
      group 3 : parameter 0 holds DENORMAL's doubles too, parameter 1 holds values in and around (-0.0, 0.0) and DENORMAL."""
    T, N = SMALL_T, SMALL_N
    assert h.params.shape == (T, 2, N)
    t = np.arange(T)
    h.accepted[...] = 1
    h.accepted[1::2, 2] = 0
    for c in range(0, 4):
        h.params[:, 0, c] = np.where((t + c) % 3 == 0, -1e308, np.where((t + c) % 3 == 1, 1e308, (t - 30.0) * 1e306))
        h.params[:, 1, c] = 1e17
    for c in range(4, 8):
        h.params[:, 0, c] = 1e16 + (t + c) % 5
        deal(h, [c], 1, RANGE_PAIRS[2][1][0], RANGE_PAIRS[2][1][1], (4, 64), False, 10)
    d = np.array([0.0, 5e-324, 1e-323, 1.5e-323])
    for c in range(8, 12):
        h.params[:, 0, c] = d[(t + c) % 4]
        h.params[:, 1, c] = np.where((t + c) % 3 == 0, 0.0, -0.0)
    z = np.array([-0.0, 0.0, 5e-324, -5e-324, 1e-323, 1.5e-323, 2e-323, 1.0, -1.0])
    for c in range(12, 16):
        h.params[:, 0, c] = d[(t + 2 * c) % 4]
        h.params[:, 1, c] = z[(t + c) % len(z)]
    return distinct_values(h)
