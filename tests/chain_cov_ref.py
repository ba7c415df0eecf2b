"""The numerical contract of smm_get_chain_cov and smm_adapt_proposal (include/smmhip.h) restated in numpy: the chain-stats mean
(chain_stats_ref.mean), the chunked pairwise sum of the centered products (chain_stats_ref.pw, here vectorised over the pairs), the
trace normalisation and the Cholesky factorisation in the contract's order, vectorised over chains.  tests/test_chain_cov.py holds it
against numpy itself; the GPU tests hold the device against it, over the history downloaded with smm_get_history."""
import numpy as np

import chain_stats_ref as R


def pw_rows(x, lo, n):
    """chain_stats_ref.pw over the last axis of x: every leading index at once (the tree depends on n only)"""
    if n < 8:
        r = np.zeros(x.shape[:-1])
        for i in range(n):
            r = r + x[..., lo + i]
        return r
    if n <= 128:
        m = n - n % 8
        r = x[..., lo:lo + 8].copy()
        for i in range(8, m, 8):
            r = r + x[..., lo + i:lo + i + 8]
        s = ((r[..., 0] + r[..., 1]) + (r[..., 2] + r[..., 3])) + ((r[..., 4] + r[..., 5]) + (r[..., 6] + r[..., 7]))
        for i in range(m, n):
            s = s + x[..., lo + i]
        return s
    n2 = n // 2
    n2 -= n2 % 8
    return pw_rows(x, lo, n2) + pw_rows(x, lo + n2, n - n2)


def chunked_sum(x):
    """S: 0.0, then + pw of every chunk of 8192 along the last axis"""
    m = x.shape[-1]
    S = np.zeros(x.shape[:-1])
    for c in range(0, m, 8192):
        S = S + pw_rows(x, c, min(8192, m - c))
    return S


def select(hist_params, accepted, t0, t1, accepted_only=True):
    """the compacted draws of every chain: a list of [np][m_c] arrays (hist_params [T][np][N], accepted [T][N])"""
    P, acc = np.asarray(hist_params)[t0:t1], np.asarray(accepted)[t0:t1]
    out = []
    for c in range(P.shape[2]):
        sel = acc[:, c] != 0 if accepted_only else np.ones(P.shape[0], bool)
        out.append(np.ascontiguousarray(P[sel, :, c].T))
    return out


def to_unit(x, lb, ub):
    """mapto_01 as the kernels compute it: (x - lb) / (ub - lb)"""
    lb, ub = np.asarray(lb, float)[:, None], np.asarray(ub, float)[:, None]
    return (x - lb) / (ub - lb)


def column_cov(u):
    """(mean [np], cov [np][np]) of one chain's compacted draws u [np][m]"""
    np_, m = u.shape
    mean = np.array([R.mean(u[j]) for j in range(np_)]) if m else np.full(np_, np.nan)
    if m < 2:
        return mean, np.full((np_, np_), np.nan)
    d = u - mean[:, None]
    S = chunked_sum(d[:, None, :] * d[None, :, :])
    return mean, S / (m - 1)


def chain_cov(hist_params, accepted, t0, t1, accepted_only=True, lb=None, ub=None):
    """(count [N], mean [np][N], cov [np][np][N]) as smm_get_chain_cov returns them; lb / ub given: unit_space"""
    cols = select(hist_params, accepted, t0, t1, accepted_only)
    N, np_ = len(cols), np.asarray(hist_params).shape[1]
    count = np.array([u.shape[1] for u in cols], np.int32)
    mean, cov = np.empty((np_, N)), np.empty((np_, np_, N))
    for c, u in enumerate(cols):
        if lb is not None:
            u = to_unit(u, lb, ub)
        mean[:, c], cov[:, :, c] = column_cov(u)
    return count, mean, cov


def cholesky(A):
    """(L [B][np][np], ok [B]) of A [B][np][np] by the contract's order; L is meaningful where ok"""
    A = np.asarray(A, float)
    B, n, _ = A.shape
    L = np.zeros_like(A)
    ok = np.ones(B, bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(n):
            for j in range(k + 1):
                s = A[:, k, j].copy()
                for i in range(j):
                    s = s - L[:, k, i] * L[:, j, i]
                if j == k:
                    ok &= s > 0
                    L[:, k, k] = np.sqrt(s)
                else:
                    L[:, k, j] = s / L[:, j, j]
    return L, ok


def adapt(count, cov, min_draws, normalize=True, ridge=1e-8):
    """(L [N][np][np], status [N]) of smm_adapt_proposal from chain_cov's count and (unit-space) cov"""
    C = np.moveaxis(np.asarray(cov, float), -1, 0)   # [N][np][np]
    N, n, _ = C.shape
    status = np.zeros(N, np.int32)
    with np.errstate(invalid="ignore", divide="ignore"):
        tau = np.zeros(N)
        for j in range(n):
            tau = tau + C[:, j, j]
        tau = tau / n
        A = C / tau[:, None, None] if normalize else C.copy()
        for j in range(n):
            A[:, j, j] = A[:, j, j] + ridge
    L, ok = cholesky(A)
    status[~ok] = 3
    status[~np.isfinite(C).all(axis=(1, 2))] = 2
    status[np.asarray(count) < min_draws] = 1
    return np.tril(L), status
