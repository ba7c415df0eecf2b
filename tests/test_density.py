"""The restatement of smm_get_density's contract (density_ref.py) against brute force and plain formulas: the HDI and the half-sample
mode against an O(m^2) search over all windows on random and tied columns; the density against the plain Gaussian sum with np.exp; the
bandwidth against bw.nrd0's formula and through each fallback of its spread; the floor(p m) hazards; every ending of the mode at
m = 0 .. 5; the row-wise np.sum the density uses against the chain-stats sum.  CPU only."""
import numpy as np
import pytest

import chain_diag_ref as D
import chain_stats_ref as CS
import density_ref as DR


def brute_window(s, lo, cnt, span):
    """the first shortest window [lo + i, lo + i + span], i < cnt, by comparing every pair of windows"""
    best = 0
    for i in range(cnt):
        wi = s[lo + i + span] - s[lo + i]
        if all(wi <= s[lo + j + span] - s[lo + j] for j in range(cnt)) and all(wi < s[lo + j + span] - s[lo + j] for j in range(i)):
            best = i
            break
    return best


def brute_mode(s):
    lo, n = 0, len(s)
    while n > 3:
        h = (n + 1) // 2
        lo, n = lo + brute_window(s, lo, n - h + 1, h - 1), h
    if n == 1:
        return s[lo]
    if n == 2:
        return (s[lo] + s[lo + 1]) / 2
    a, b = s[lo + 1] - s[lo], s[lo + 2] - s[lo + 1]
    return (s[lo] + s[lo + 1]) / 2 if a < b else (s[lo + 1] + s[lo + 2]) / 2 if b < a else s[lo + 1]


def columns():
    r = np.random.default_rng(11)
    for m in (1, 2, 3, 4, 5, 6, 7, 17, 64, 101):
        yield r.normal(size=m)                               # random
        yield r.integers(0, 4, m).astype(float)             # heavily tied
        yield np.round(r.gamma(2.0, size=m), 1)              # skewed, some ties


def test_hdi_and_mode_against_brute_force():
    for x in columns():
        s = CS.total_sort(x)
        m = len(s)
        for p in (0.01, 0.29, 0.5, 0.57, 0.94, 1.0):
            k = DR.hdi_span(p, m)
            i = brute_window(s, 0, m - k, k)
            lo, hi, at = DR.hdi(s, p)
            assert (at, lo, hi) == (i, s[i], s[i + k]), (m, p)
        assert DR.half_sample_mode(s) == brute_mode(s), m


def test_floor_of_the_rounded_product():
    assert DR.hdi_span(0.29, 100) == 28 and DR.hdi_span(0.57, 100) == 56   # 0.29 * 100 = 28.999999999999996, 0.57 * 100 = 56.99999999999999
    assert DR.hdi_span(1.0, 100) == 99 and DR.hdi_span(0.5, 1) == 0 and DR.hdi_span(0.01, 50) == 0


def test_mode_endings_at_m_0_to_5():
    want = {(1.0,): "one", (1.0, 4.0): "two", (1.0, 2.0, 3.0): "middle", (0.0, 1.0, 3.0): "left", (0.0, 2.0, 3.0): "right",
            (0.0, 3.0, 4.0, 9.0): "two", (0.0, 4.0, 5.0, 5.5, 9.0): "right", (0.0, 4.0, 4.5, 5.5, 9.0): "left",
            (0.0, 1.0, 2.0, 3.0, 4.0): "middle"}
    for s, end in want.items():
        trail = []
        v = DR.half_sample_mode(np.array(s), trail)
        assert trail[-1] == end and v == brute_mode(np.array(s)), s
    c = DR.column(np.array([]), [0.5], 4)
    assert c["status"] == 2 and np.isnan(c["mode"]) and np.isnan(c["hdi_lo"]).all() and c["kde_status"] == 1
    c = DR.column(np.array([1.0, np.inf]), [0.5], 4)
    assert c["status"] == 1 and np.isnan(c["density"]).all() and np.isnan(c["bw"])
    c = DR.column(np.array([3.0]), [0.5, 1.0], 4)           # m = 1: an interval and a mode, no bandwidth
    assert c["status"] == 0 and c["mode"] == 3.0 and (c["hdi_lo"] == 3.0).all() and c["kde_status"] == 1 and np.isnan(c["bw"])


def test_bandwidth_formula_and_fallbacks(O):
    r = np.random.default_rng(3)
    x = r.normal(size=500)
    s = CS.total_sort(x)
    trail = []
    h = DR.bw_nrd0(x, s, trail=trail)
    q = np.quantile(x, [0.25, 0.75])
    plain = 0.9 * min(np.std(x, ddof=1), (q[1] - q[0]) / 1.34) * 500 ** -0.2
    assert abs(h - plain) <= 1e-14 * plain and trail[0] in ("sd", "iqr")
    for x, took, l in ((np.r_[np.full(32, 1.5), r.normal(size=8)], "sd0", None), (np.full(40, 2.5), "first", 2.5),
                       (np.full(40, -0.75), "first", 0.75), (np.zeros(40), "one", 1.0)):
        trail = []
        h = DR.bw_nrd0(x, CS.total_sort(x), trail=trail)
        assert trail == [took], (trail, took)
        l = np.std(x, ddof=1) if l is None else l
        assert abs(h - 0.9 * l * len(x) ** -0.2) <= 1e-14 * h
    for took, x in (("sd", np.r_[np.zeros(10), np.ones(10)]), ("iqr", np.r_[r.normal(size=99), 1e6])):
        trail = []
        DR.bw_nrd0(x, CS.total_sort(x), trail=trail)
        assert trail == [took]


def test_density_against_the_plain_formula(O, capsys):
    r = np.random.default_rng(4)
    worst = 0.0
    for m, n_grid in ((7, 2), (300, 33), (8208, 5)):
        x = r.gamma(2.0, size=m)
        c = DR.column(x, [0.94], n_grid)
        g, h = c["grid"], c["bw"]
        plain = np.exp(-0.5 * ((g[:, None] - x[None, :]) / h) ** 2).sum(axis=1) / (m * h * np.sqrt(2 * np.pi))
        err = np.max(np.abs(c["density"] - plain) / plain)
        worst = max(worst, err)
        assert np.array_equal(g, np.linspace(x.min() - 3.0 * h, x.max() + 3.0 * h, n_grid))
        assert c["kde_mode"] == g[np.argmax(c["density"])] and c["kde_status"] == 0
        e = DR.kernel_terms(x, g, h)
        assert [D.S(row) for row in e] == list(D.rowsum(e)), m   # the row-wise np.sum is the chain-stats sum, past one chunk too
    with capsys.disabled():
        print("\ndensity_ref against the plain formula: largest relative difference %.3g" % worst)
    assert worst <= 1e-13


def test_given_bandwidth_range_and_the_unusable_ones(O):
    x = np.array([1.0, 2.0, 4.0, 8.0])
    c = DR.column(x, [], 5, rng=(0.0, 10.0), bw=0.5)
    assert c["bw"] == 0.5 and np.array_equal(c["grid"], [0.0, 2.5, 5.0, 7.5, 10.0]) and c["hdi_lo"].shape == (0,)
    c = DR.column(np.array([-1.7e308, 1.7e308]), [1.0], 3, bw=1.0)
    assert c["kde_status"] == 2 and np.isnan(c["grid"]).all() and c["bw"] == 1.0 and c["hdi_hi"][0] == 1.7e308
    c = DR.column(x, [0.5], 0)
    assert c["kde_status"] == 0 and c["grid"].shape == (0,)
