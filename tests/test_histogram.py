"""The restatement of smm_get_histogram's contract (hist_ref.py) held against numpy itself: np.histogram, np.histogram2d and np.linspace
on random columns, values on interior edges and on hi, min == max, empty columns, +-0, a denormal-width range (linspace's step == 0
branch), repeated edges, given ranges with outliers, NaN and +-inf, and bins = 1; numpy raises exactly where the restatement reports
a status.  Also the selection of the pooled columns against params(c) of the host layer's definition.  CPU only."""
from types import SimpleNamespace

import numpy as np
import pytest

import hist_ref as HR

RNG = np.random.default_rng(7)


def ref1(x, bins, rng=None):
    lo, hi, st = HR.outer_edges(x, rng)
    if st:
        return st, None, None
    e = HR.linspace(lo, hi, bins)
    if np.any(e[:-1] >= e[1:]):
        return 3, e, None
    return 0, e, HR.hist1d(x, lo, hi, e, bins)


def check1(x, bins, rng=None):
    x = np.asarray(x, np.float64)
    st, e, n = ref1(x, bins, rng)
    if st in (1, 3):
        with pytest.raises(ValueError):
            np.histogram(x, bins, rng)
        return st
    if st == 2:                                           # numpy's index arithmetic is undefined there: nothing to compare
        return st
    wn, we = np.histogram(x, bins, rng)
    assert np.array_equal(n, wn) and n.dtype == wn.dtype
    assert np.array_equal(e, we) and (rng is None or np.array_equal(np.signbit(e), np.signbit(we)))
    return st


def check2(x, y, bins, rng=None):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    r = [HR.outer_edges(v, None if rng is None else rng[i]) for i, v in enumerate((x, y))]
    if any(s == 1 for _, _, s in r):
        with pytest.raises(ValueError):
            np.histogram2d(x, y, bins, rng)
        return
    ex, ey = (HR.linspace(lo, hi, bins) for lo, hi, _ in r)
    H, wx, wy = np.histogram2d(x, y, bins, rng)
    assert np.array_equal(ex, wx) and np.array_equal(ey, wy)
    assert np.array_equal(HR.hist2d(x, y, ex, ey, bins), H) and H.dtype == np.float64


@pytest.mark.parametrize("bins", [1, 2, 7, 10, 64, 1000])
def test_random_columns(bins):
    for n in (0, 1, 5, 1000):
        x = RNG.standard_normal(n) * 10 ** RNG.uniform(-3, 3)
        assert check1(x, bins) == 0
        check2(x, RNG.standard_normal(n), min(bins, 64))


def test_values_on_edges_and_on_hi():
    for bins in (1, 3, 10, 64, 100):
        e = np.linspace(-1.3, 2.9, bins + 1)
        x = np.concatenate([e, e[1:-1], np.nextafter(e, -np.inf), np.nextafter(e, np.inf)])
        check1(x, bins, (-1.3, 2.9))
        check1(e, bins)
        check2(e, e[::-1], bins)
        check2(x, x[::-1], bins, [(-1.3, 2.9), (-1.3, 2.9)])


def test_min_equals_max_empty_and_signed_zeros():
    check1([2.5, 2.5, 2.5], 4)
    check1([], 4)
    assert HR.outer_edges(np.empty(0)) == (0.0, 1.0, 0)
    check1([-0.0, 0.0, -0.0], 5)
    check1([-0.0, -0.0], 3)
    check1([0.0, -0.0, 1.0, -1.0], 4, (-0.0, 0.0))
    check2([2.5, 2.5], [-0.0, 0.0], 3)
    check2([], [], 3)


def test_linspace_both_branches():
    for lo, hi, b in ((0.0, 1.0, 10), (-3.0, 7.5, 7), (0.0, 5e-324, 4), (1e-320, 1.0000000000000002e-320, 64), (5.0, 5.0, 3)):
        assert np.array_equal(HR.linspace(lo, hi, b), np.linspace(lo, hi, b + 1))
    lo, hi = 0.0, 5e-324 * 3                               # a denormal width: step == 0
    assert (hi - lo) / 64 == 0
    check1([0.0, 5e-324, 1e-323, 1.5e-323], 64, (lo, hi))
    check2([0.0, 5e-324, 1e-323, 1.5e-323], [0.0, 5e-324, 1e-323, 1.5e-323], 4, [(lo, hi), (lo, hi)])


def test_repeated_edges():
    lo, hi = 1e16, 1e16 + 4
    e = HR.linspace(lo, hi, 64)
    assert np.any(e[:-1] == e[1:])
    x = np.array([lo, lo + 2, lo + 4, hi, lo - 2, hi + 2, np.nan])
    assert check1(x, 64, (lo, hi)) == 3                     # numpy: "Too many bins for data range"
    check2(x, x, 64, [(lo, hi), (lo, hi)])
    check2(x[:4], x[:4][::-1], 64)
    check2([1e17] * 3, [1.0, 2.0, 3.0], 4)                  # lo == hi where +-0.5 does not move them


def test_given_ranges_with_outliers_nan_and_inf():
    x = np.concatenate([RNG.standard_normal(500), [np.nan, np.inf, -np.inf, 10.0, -10.0, 1.0, -1.0]])
    for rng in ((-1.0, 1.0), (0.0, 0.0), (-2.0, 3.0), (1.0, 1.0)):
        assert check1(x, 10, rng) == 0
        check2(x, x[::-1], 10, [rng, (-1.0, 2.0)])
    assert check1(x, 10) == 1                                # numpy raises on the autodetected range
    check2(x, RNG.standard_normal(len(x)), 5)
    assert check1([np.nan], 3) == 1 and check1([np.inf, 0.0], 3) == 1
    assert check1([-1e308, 1e308], 3) == 2 and HR.outer_edges(np.empty(0), (-1e308, 1e308))[2] == 2
    for bad in ((1.0, 0.0), (0.0, np.inf), (np.nan, 1.0)):
        with pytest.raises(ValueError):
            np.histogram([0.5], 3, bad)


def test_histogram_from_history_selects_like_params():
    T, npar, N = 40, 3, 6
    h = SimpleNamespace(params=RNG.standard_normal((T, npar, N)), accepted=(RNG.random((T, N)) < 0.5).astype(np.int32),
                        value=RNG.standard_normal((T, N)), exchanged=np.zeros((T, N), np.int32))
    h.accepted[:7, 2] = 0                                   # chain 2: no state before row 7
    groups = np.array([0, 1, 0, -1, 1, 0], np.int32)
    pairs = [(0, 1), (2, 2), (1, 0)]
    for sel in ("all", "accepted", "state"):
        for t0, t1 in ((0, T), (5, 31)):
            r = HR.histogram_from_history(h, t0, t1, sel, groups, 6, pairs=pairs, bins2=5)
            for g in range(2):
                mem = np.flatnonzero(groups == g)
                if sel == "state":
                    a = np.maximum.accumulate(np.where(h.accepted != 0, np.arange(T)[:, None], -1), axis=0)[t0:t1]
                    x = np.concatenate([np.where(a[:, c, None] >= 0, h.params[np.maximum(a[:, c], 0), :, c], np.nan) for c in mem])
                else:
                    x = np.concatenate([h.params[t0:t1][(h.accepted[t0:t1, c] != 0) | (sel == "all"), :, c] for c in mem])
                assert r["count"][g] == len(x)
                for k in range(npar):
                    if not np.isfinite(x[:, k]).all():           # a row before the chain's first accepted one
                        assert sel == "state"
                        assert r["status"][g, k] == 1 and (r["hist"][g, k] == 0).all() and np.isnan(r["edges"][g, k]).all()
                        continue
                    n, e = np.histogram(x[:, k], 6)
                    assert r["status"][g, k] == 0 and np.array_equal(r["hist"][g, k], n) and np.array_equal(r["edges"][g, k], e)
                for p, (a_, b_) in enumerate(pairs):
                    if r["status"][g, a_] == 0 and r["status"][g, b_] == 0:
                        H, xe, ye = np.histogram2d(x[:, a_], x[:, b_], 5)
                        assert np.array_equal(r["hist2"][g, p], H) and np.array_equal(r["edges2"][g, a_], xe)
