"""The contract of smm_get_chain_diag (include/smmhip.h) as restated in chain_diag_ref.py, held against numpy and against theory: the
autocovariances and half variances bit for bit numpy's, the ESS of an independent Geyer over np.correlate, AR(1) and R-hat in their
expected ranges, every status reached — and the Julia mirror of the struct field for field."""
import os

import numpy as np
import pytest

import chain_diag_ref as R
from chain_stats_ref import mean

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ar1(n, phi, rng, cols=1):
    e = rng.standard_normal((cols, n))
    x = np.empty((cols, n))
    x[:, 0] = e[:, 0] / np.sqrt(1 - phi * phi)
    for t in range(1, n):
        x[:, t] = phi * x[:, t - 1] + e[:, t]
    return x


@pytest.mark.parametrize("n", [4, 37, 2000, 8193, 20001])
def test_acov_is_numpys_sum_bit_for_bit(n):
    rng = np.random.default_rng(n)
    x = ar1(n, 0.7, rng)[0] * 3.0 + 1.5
    d = x - mean(x)
    assert mean(x) == np.mean(x)
    lags = sorted({0, 1, 2, n // 3, n - 1} | ({8191, 8192} if n > 8192 else set()))
    X = np.stack([x, x[::-1].copy()])
    Dr = X - (R.rowsum(X) / n)[:, None]
    for k in lags:
        want = np.sum(d[: n - k] * d[k:]) / n
        assert R.acov_pw(x, k) == want, k
        assert R.rowsum(Dr[:, : n - k] * Dr[:, k:])[0] / n == want, k   # the vectorised path of the restatement


@pytest.mark.parametrize("n", [4, 5, 37, 2001, 16390, 20001])
def test_half_variances_are_np_var_ddof1(n):
    rng = np.random.default_rng(7 + n)
    x = rng.standard_normal(n) * 2.0 - 0.3
    X = x[None, :]
    _, _, _, hmu, hvar = R.diag_columns(X, 1, 0)
    h = n // 2
    for hf, y in enumerate((x[:h], x[n - h:])):
        assert hmu[hf, 0] == np.mean(y)
        assert hvar[hf, 0] == np.var(y, ddof=1)
        mu = mean(y)
        assert hvar[hf, 0] == R.S([(v - mu) * (v - mu) for v in y]) / (h - 1)


def numpy_geyer_ess(x):
    """an independent Geyer initial monotone sequence over np.correlate"""
    n = len(x)
    d = x - x.mean()
    acov = np.correlate(d, d, mode="full")[n - 1:] / n
    rho = acov / acov[0]
    pairs = rho[: 2 * ((n) // 2)].reshape(-1, 2).sum(axis=1)
    J = len(pairs)
    for j in range(1, len(pairs)):
        if pairs[j] <= 0:
            J = j
            break
    q = np.minimum.accumulate(pairs[:J])
    return n / (-1.0 + 2.0 * q.sum()), pairs[:J + 1]


def test_ess_agrees_with_an_independent_numpy_geyer():
    rng = np.random.default_rng(3)
    checked = 0
    for phi in (0.0, 0.3, 0.6, 0.9, -0.4):
        for n in (200, 1000, 3000):
            x = ar1(n, phi, rng)[0]
            want, pairs = numpy_geyer_ess(x)
            if np.min(np.abs(pairs)) < 1e-9:
                continue
            ess, status, _, _, _ = R.diag_columns(x[None, :], n - 1, 0)
            assert status[0] == 0
            assert abs(ess[0] - want) <= 1e-12 * abs(want), (phi, n, ess[0], want)
            checked += 1
    assert checked >= 12


def test_ess_of_a_long_ar1_is_near_theory():
    rng = np.random.default_rng(5)
    phi, n = 0.9, 20001
    x = ar1(n, phi, rng, cols=16)
    ess, status, _, _, _ = R.diag_columns(x, n - 1, 0)
    assert (status == 0).all()
    theory = (1 - phi) / (1 + phi)
    assert abs(np.mean(ess / n) - theory) <= 0.1 * theory, ess / n   # (one chain's estimate spreads by about 10 %)


def test_rhat_separates_mixed_from_shifted_groups():
    rng = np.random.default_rng(9)
    n, k = 2000, 8
    iid = rng.standard_normal((1, k, n))
    shifted = iid + np.linspace(0.0, 2.0, k)[None, :, None]
    X = np.concatenate([iid, shifted], axis=1)
    groups = [0] * k + [1] * k
    out = R.diag_from_series(X, np.zeros(2 * k), n - 1, 0, groups)
    assert out["rhat"][0, 0] < 1.01
    assert out["rhat"][1, 0] > 1.1


def test_every_status_is_reached():
    rng = np.random.default_rng(1)
    n = 400
    cols = np.stack([
        np.full(n, 0.25),                                      # constant: acov_0 == 0 -> 2
        np.where(np.arange(n) == 7, np.nan, rng.standard_normal(n)),   # NaN -> 3
        np.where(np.arange(n) == 300, np.inf, rng.standard_normal(n)),  # Inf -> 3
        np.cumsum(rng.standard_normal(n)),                      # a random walk: not truncated by lag 9 -> 1
        rng.standard_normal(n),                                  # i.i.d. -> 0
    ])
    with np.errstate(invalid="ignore", divide="ignore"):
        ess, status, acf, _, _ = R.diag_columns(cols, 9, 4)
    assert list(status) == [2, 3, 3, 1, 0]
    assert np.isnan(ess[:3]).all() and ess[3] > 0 and ess[4] > 0
    assert np.isnan(acf[:, 1:3]).all() and (acf[0, 3:] == 1.0).all()
    # the random walk untruncated at max_lag overstates what the whole sequence gives
    ess_all, st_all, _, _, _ = R.diag_columns(cols[3:4], n - 1, 0)
    assert st_all[0] == 0 and ess_all[0] < ess[3]


def test_the_carry_forward_series_follow_the_chains_state():
    class H:   # a history of 2 chains, 6 iterations, np = 1
        pass
    h = H()
    h.accepted = np.array([[0, 1], [1, 0], [0, 0], [1, 1], [0, 0], [0, 1]], np.uint8)
    h.exchanged = np.array([[0, 0], [0, 2], [0, 0], [0, 0], [1, 0], [0, 0]], np.int32)
    h.value = np.arange(12, dtype=float).reshape(6, 2)
    h.params = (100 + np.arange(12, dtype=float)).reshape(6, 1, 2)
    X, rate = R.series_from_history(h, 2, 6)
    assert np.array_equal(X[1, 0], [2.0, 6.0, 6.0, 6.0]) and np.array_equal(X[0, 0], [102.0, 106.0, 106.0, 106.0])
    assert np.array_equal(X[1, 1], [1.0, 7.0, 7.0, 11.0])
    assert rate[0] == 1 / 3 and rate[1] == 2 / 4
    X, _ = R.series_from_history(h, 0, 6)
    assert np.isnan(X[1, 0, 0]) and X[1, 0, 1] == 2.0


def test_the_julia_mirror_of_smm_chain_diag_t():
    from test_julia_layer import header_structs, julia_structs
    js = julia_structs(os.path.join(ROOT, "julia", "SMMHip.jl"))
    hs = header_structs()
    ptr = {"Cdouble": "double*", "Int32": "int32_t*"}
    want = [(f, t) for f, t in hs["smm_chain_diag_t"]]
    got = [(f, ptr[t[4:-1]]) for f, t in js["SmmChainDiag"]]
    assert got == want
    from smm_jl_amd import _abi as A
    assert [f for f, _ in A.smm_chain_diag_t._fields_] == [f for f, _ in want]
