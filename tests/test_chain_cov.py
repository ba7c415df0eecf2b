"""The restatement of smm_get_chain_cov / smm_adapt_proposal (tests/chain_cov_ref.py) against numpy itself: np.sum on the centered
products bit for bit, np.cov(ddof=1) and np.linalg.cholesky within 1e-12 relative.  CPU only."""
import numpy as np
import pytest

import chain_cov_ref as CR
import chain_stats_ref as R


@pytest.mark.parametrize("n", [0, 1, 5, 8, 13, 128, 129, 1000, 2000, 8192, 8193, 20000])
def test_vectorised_pairwise_sum_is_the_chain_stats_one_and_numpys(n):
    rng = np.random.default_rng(n)
    x = rng.standard_normal((3, n))
    got = CR.chunked_sum(x)
    for r in range(3):
        S = 0.0
        for c in range(0, n, 8192):
            S = S + R.pw(list(x[r]), c, min(8192, n - c))
        assert got[r] == S
        assert got[r] == np.sum(np.ascontiguousarray(x[r]))


@pytest.mark.parametrize("np_,m", [(2, 50), (6, 333), (17, 2000), (3, 9000)])
def test_covariance_is_numpys(np_, m):
    rng = np.random.default_rng(np_ * 1000 + m)
    M = rng.standard_normal((np_, np_))
    u = M @ rng.standard_normal((np_, m)) + rng.standard_normal((np_, 1))
    mean, cov = CR.column_cov(u)
    for j in range(np_):
        assert mean[j] == R.mean(u[j])
        dj = u[j] - mean[j]
        for k in range(np_):
            dk = u[k] - mean[k]
            assert cov[j, k] == np.sum(dj * dk) / (m - 1)   # bit for bit
    assert (cov == cov.T).all()
    np.testing.assert_allclose(cov, np.cov(u, ddof=1), rtol=1e-12, atol=1e-12 * np.abs(cov).max())


def test_small_and_nan_columns():
    mean, cov = CR.column_cov(np.zeros((3, 0)))
    assert np.isnan(mean).all() and np.isnan(cov).all()
    mean, cov = CR.column_cov(np.ones((3, 1)))
    assert (mean == 1).all() and np.isnan(cov).all()
    u = np.random.default_rng(0).standard_normal((3, 40))
    u[1, 7] = np.nan
    mean, cov = CR.column_cov(u)
    assert np.isnan(mean[1]) and not np.isnan(mean[[0, 2]]).any()
    assert np.isnan(cov[1]).all() and np.isnan(cov[:, 1]).all() and not np.isnan(cov[np.ix_([0, 2], [0, 2])]).any()


def test_selection_and_unit_space():
    rng = np.random.default_rng(3)
    T, np_, N = 30, 4, 5
    P = rng.uniform(-2, 3, (T, np_, N))
    acc = (rng.uniform(size=(T, N)) < 0.5).astype(np.uint8)
    lb, ub = np.full(np_, -2.0), np.full(np_, 3.0)
    count, mean, cov = CR.chain_cov(P, acc, 5, 25, True, lb, ub)
    for c in range(N):
        sel = acc[5:25, c] != 0
        assert count[c] == sel.sum()
        u = (P[5:25][sel, :, c].T - lb[:, None]) / (ub - lb)[:, None]
        if count[c] >= 2:
            np.testing.assert_allclose(cov[:, :, c], np.cov(u, ddof=1), rtol=1e-12, atol=1e-15)
    count, _, _ = CR.chain_cov(P, acc, 5, 25, False)
    assert (count == 20).all()


def test_cholesky_is_numpys_and_statuses():
    rng = np.random.default_rng(7)
    B, n = 64, 50
    M = rng.standard_normal((B, n, 2 * n))
    A = M @ np.swapaxes(M, 1, 2) / (2 * n)
    L, ok = CR.cholesky(A)
    assert ok.all()
    np.testing.assert_allclose(np.tril(L), np.linalg.cholesky(A), rtol=1e-12, atol=1e-12)
    # adapt: normalisation by the mean of the diagonal, the ridge, and the three failure kinds
    C = np.moveaxis(A, 0, -1).copy()
    count = np.full(B, 100, np.int32)
    count[3] = 10
    C[:, :, 5] = 0.0   # a never-moving chain: not positive definite without a ridge
    C[2, 4, 9] = C[4, 2, 9] = np.nan
    L2, st = CR.adapt(count, C, min_draws=51, normalize=True, ridge=0.0)
    assert st[3] == 1 and st[9] == 2 and st[5] == 3 and (np.delete(st, [3, 5, 9]) == 0).all()
    tau = np.trace(A[0]) / n
    np.testing.assert_allclose(L2[0], np.linalg.cholesky(A[0] / tau), rtol=1e-12, atol=1e-12)
    L3, st3 = CR.adapt(count, C, min_draws=2, normalize=False, ridge=0.5)
    assert st3[5] == 0 and st3[9] == 2
    np.testing.assert_allclose(L3[5], np.sqrt(0.5) * np.eye(n), rtol=1e-15)
