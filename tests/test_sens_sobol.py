"""smm_sens_sobol's restatement (tests/sobol_ref.py) with numpy evaluators against closed forms, and the properties the contract
(include/smmhip.h) promises, each asserted on the restatement alone.  No GPU: tests/test_gpu_sens_sobol.py holds the device to the
restatement bit for bit.  The bounds on the closed forms follow the project's habit: the largest distance measured with the restatement
(written into each docstring) times ten — the margin covers a change of seed, not of arithmetic."""
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sobol_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20240521
N = 8192
A_LIN = np.array([1.0, 2.0, 0.5])
LB3, UB3 = np.full(3, 2.0), np.full(3, 3.0)
_cache = {}


def linear(P):
    """value = sum a_k theta_k; moment 0 = theta_0, moment 1 = theta_1 * theta_2"""
    return A_LIN @ P, np.stack([P[0], P[1] * P[2]]), np.ones(P.shape[1], np.int32)


def ishigami(P):
    v = np.sin(P[0]) + 7.0 * np.sin(P[1]) ** 2 + 0.1 * P[2] ** 4 * np.sin(P[0])
    return v, np.stack([P[0]]), np.ones(P.shape[1], np.int32)


def holes(P):
    """linear, but the evaluation fails (status -2) where theta_0 > 2.9 and its first moment is NaN where theta_1 < 2.05"""
    v, m, st = linear(P)
    st = np.where(P[0] > 2.9, -2, st).astype(np.int32)
    m = m.copy()
    m[0, P[1] < 2.05] = np.nan
    return v, m, st


def run(O, name, evaluator, n, **kw):
    key = (name, n, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _cache:
        lb, ub = (np.full(3, -np.pi), np.full(3, np.pi)) if name == "ishigami" else (LB3, UB3)
        nm = 1 if name == "ishigami" else 2
        _cache[key] = R.sens_sobol(O, evaluator, SEED, lb, ub, nm, n, **kw)
    return _cache[key]


def test_linear_function_against_its_closed_form(O):
    """first_k = total_k = a_k^2 / sum a^2 and var = sum a_k^2 (hi - lo)^2 / 12 at N = 8192.  Measured: |first - exact| <= 1.8e-3,
    |total - exact| <= 3.1e-3, |var / exact - 1| = 4.0e-3, |mean - exact| = 1.5e-3.  Moment 0 is theta_0 alone and
    moment 1 is theta_1 * theta_2: a parameter that an output does not read has total index exactly 0.0 on it"""
    r = run(O, "linear", linear, N)
    exact = A_LIN ** 2 / (A_LIN ** 2).sum()
    d_first, d_total = np.abs(r["first"][0] - exact).max(), np.abs(r["total"][0] - exact).max()
    d_var, d_mean = abs(r["var"][0] / ((A_LIN ** 2).sum() / 12.0) - 1.0), abs(r["mean"][0] - 2.5 * A_LIN.sum())
    print("linear: first %.3g total %.3g var %.3g mean %.3g" % (d_first, d_total, d_var, d_mean))
    assert d_first <= 1.8e-2 and d_total <= 3.1e-2 and d_var <= 4.0e-2 and d_mean <= 1.5e-2
    assert r["n_complete"] == N and r["n_invalid"] == 0 and r["evaluated"] == N * 5 + 256
    # moment 0 is theta_0 alone: the other parameters' totals are exactly 0.0, theirs on it 1 up to sampling error
    assert (r["total"][1, 1:] == 0.0).all() and (r["v_first"][1, 1:] == 0.0).all() and abs(r["total"][1, 0] - 1.0) < 0.05
    assert r["total"][2, 0] == 0.0 and (r["total"][2, 1:] > r["first"][2, 1:] - 3 * r["se_first"][2, 1:]).all()


def test_ishigami_against_its_known_indices(O):
    """a = 7, b = 0.1 on [-pi, pi]^3: S = (0.3139, 0.4424, 0), ST = (0.5576, 0.4424, 0.2437).  Measured at N = 8192: |first - exact| <=
    2.3e-2, |total - exact| <= 1.4e-2, |var / exact - 1| = 2.3e-2"""
    r = run(O, "ishigami", ishigami, N)
    a, b, pi = 7.0, 0.1, np.pi
    V = a * a / 8 + b * pi ** 4 / 5 + b * b * pi ** 8 / 18 + 0.5
    V1, V2, V13 = 0.5 * (1 + b * pi ** 4 / 5) ** 2, a * a / 8, 8 * b * b * pi ** 8 / 225
    first, total = np.array([V1, V2, 0.0]) / V, np.array([V1 + V13, V2, V13]) / V
    d_first, d_total, d_var = np.abs(r["first"][0] - first).max(), np.abs(r["total"][0] - total).max(), abs(r["var"][0] / V - 1.0)
    print("ishigami: first %.3g total %.3g var %.3g" % (d_first, d_total, d_var))
    assert d_first <= 2.3e-1 and d_total <= 1.4e-1 and d_var <= 2.3e-1
    assert r["total"][0, 0] - r["first"][0, 0] > 0.1 and abs(r["first"][0, 2]) < 4 * r["se_first"][0, 2] + 1e-12


def test_the_standard_errors_shrink_with_the_square_root_of_n(O):
    """se(N) / se(2N) = sqrt 2 but for the sample standard deviations' own error, a few per cent at these sizes: within [1.25, 1.6]"""
    half, full = run(O, "linear", linear, N // 2), run(O, "linear", linear, N)
    for f in ("se_first", "se_total"):
        ratio = half[f][0] / full[f][0]
        assert ((ratio > 1.25) & (ratio < 1.6)).all(), (f, ratio)


def test_the_batch_size_changes_nothing(O):
    one = R.sens_sobol(O, holes, SEED, LB3, UB3, 2, 600)
    assert 0 < one["n_complete"] < 600
    for batch in (1, 100, 256):
        R.assert_equal(R.sens_sobol(O, holes, SEED, LB3, UB3, 2, 600, batch=batch), one)


def test_incomplete_points_are_skipped_not_zero_filled(O):
    r = R.sens_sobol(O, holes, SEED, LB3, UB3, 2, 600)
    ok = r["complete"]
    n = int(ok.sum())
    assert r["n_complete"] == n and 0 < n < 600 and r["n_invalid"] >= 600 - n
    y = r["yA"][0]
    assert abs(r["mean"][0] - y[ok].mean()) < 1e-12 * abs(y[ok].mean()) and abs(r["mean"][0] - np.where(ok, y, 0.0).sum() / 600) > 0.1
    assert abs(r["var"][0] - y[ok].var()) < 1e-10 and np.isfinite(r["first"]).all() and np.isfinite(r["mean"]).all()
    # a point counts as incomplete when any of its np + 2 evaluations is invalid, not only A's
    assert n < int(((r["yA"] == r["yA"]).all(0)).sum())


def test_the_centre_shifts_nothing_and_removes_the_means_variance(O):
    """the value's mean is 8.75 and its standard deviation 0.66: without the centre the first-order terms carry the mean's variance"""
    c, z = run(O, "linear", linear, N), run(O, "linear", linear, N, centre0=True)
    assert (z["centre"] == 0.0).all() and abs(c["centre"][0] - 8.75) < 0.2
    se_num = z["se_first"][0] * z["var"][0]
    assert (np.abs(z["v_first"][0] - c["v_first"][0]) <= 4 * se_num).all()
    assert (c["se_first"][0] < 0.5 * z["se_first"][0]).all()
    for f in ("total", "v_total", "se_total", "mean", "var"):
        assert np.array_equal(c[f], z[f]), f


def test_a_frozen_parameter_has_total_index_zero(O):
    lo, hi = np.array([2.0, 2.25, 2.0]), np.array([3.0, 2.25, 2.5])
    r = R.sens_sobol(O, linear, SEED, LB3, UB3, 2, 300, lo=lo, hi=hi)
    assert (r["total"][:, 1] == 0.0).all() and (r["first"][:, 1] == 0.0).all() and (r["total"][0, [0, 2]] > 0.0).all()


def test_n_zero_gives_nan_everywhere(O):
    def nothing(P):
        return np.full(P.shape[1], np.inf), np.zeros((2, P.shape[1])), np.ones(P.shape[1], np.int32)
    r = R.sens_sobol(O, nothing, SEED, LB3, UB3, 2, 30)
    assert r["n_complete"] == 0 and r["n_invalid"] == 150 and (r["centre"] == 0.0).all()
    assert all(np.isnan(r[f]).all() for f in ("mean", "var") + R.TABLES)


def test_the_stream_is_named_in_the_generator():
    text = open(os.path.join(ROOT, "smm.jl_amd", "csrc", "smm_rng.hpp")).read()
    assert re.search(r"STREAM_GSA = 9\b", text) and "STREAM_PMC = 8" in text
    assert R.STREAM_GSA == 9
