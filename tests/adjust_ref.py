"""The numerical contract of smm_get_adjustment (include/smmhip.h) restated in numpy over a downloaded history: the local-linear
regression adjustment of Beaumont, Zhang & Balding (2002) over the pooled rows of a group.  The rows are moment_stats_ref's
(joint_columns: every row, the accepted rows or the state series), the sums chain_cov_ref's chunked pairwise sums, the bandwidth
chain_stats_ref's quantile of the distance column, the factor and the substitutions moment_stats_ref's; the weights, the centred
columns, the adjusted draws and the weighted quantiles are stated here.  tests/test_adjustment.py holds it against np.linalg.lstsq, the
exact identities and the status table; the GPU tests hold the device against it, over the history downloaded with smm_get_history.
Its edges (bound counts, the weighted select's keys and weights, a tie run at the bandwidth, batch seams) are tested on adjust_craft.py's
crafted histories: tests/test_adjustment_edges.py here, tests/test_gpu_adjustment_edges.py on the device, bit for bit."""
import numpy as np

import chain_cov_ref as V
import chain_stats_ref as R
import moment_stats_ref as MR

SELECT = MR.SELECT
KERNEL = {"uniform": 0, "epanechnikov": 1}
FIELDS = ("count", "n_chains", "status", "n_kept", "bandwidth", "sum_w", "ess", "x_mean", "raw_mean", "beta", "adj_mean", "adj_sd",
          "adj_quantile", "n_outside")
Q_ONE = 1048576.0

# beta against np.linalg.lstsq on the r-scaled centred design of tests/test_adjustment.py's linear-Gaussian case: the largest relative
# deviation (in units of beta's largest entry) measured there on the CPU, and the bound the test holds it under: ten times that, the
# margin for the summation order and the solver behind np.linalg (the procedure of moment_stats_ref.MOMENT_LINALG_RTOL)
ADJUST_LSTSQ_DEV = 5.88e-14            # measured (test_linear_gaussian_recovery_and_beta_against_lstsq prints it): over its two kernels
ADJUST_LSTSQ_RTOL = 10 * ADJUST_LSTSQ_DEV

# a moment column of 32 rows whose centred sums are exact: mean 0, sum of squares 16.  Two moments that both hold it against data
# moments of 0 and unit scales give A = [[16, 16], [16, 16]], whose second pivot is 16 - 4 * 4 = 0 exactly: status 4
COLLINEAR_COLUMN = np.array([1.0] * 8 + [-1.0] * 8 + [0.0] * 16)


def scales(w, scale):
    """sc [nm]: the caller's scale, else moment_stats_ref.weights' s"""
    return MR.weights(w)[0] if scale is None else np.asarray(scale, np.float64)


def distances(x):
    """d2 [m] of the discrepancies x [nm][m]: from 0.0, + x_k * x_k over k ascending"""
    d2 = np.zeros(x.shape[1])
    for k in range(x.shape[0]):
        d2 = d2 + x[k] * x[k]
    return d2


def bandwidth(d2, tol):
    """the chain-stats quantile tol of the column d2 (without NaN)"""
    return R.quantile(R.total_sort(d2), float(tol))


def row_weights(d2, delta2, kernel):
    if kernel == 0:
        return np.where(d2 <= delta2, 1.0, 0.0)
    with np.errstate(all="ignore"):
        return np.where(d2 < delta2, 1.0 - d2 / delta2, 0.0)


def int_weights(om):
    """q [m] int64: ceil(w * 2^20), 0 for a row that is not kept"""
    return np.ceil(om * Q_ONE).astype(np.int64)


def weighted_quantile(v, q, p):
    """the smallest of the kept v (q > 0) at which the weights q of the values <= it reach max(1, ceil(p * Q)), the doubles in the
    IEEE total order"""
    keep = q > 0
    v, q = np.asarray(v, np.float64)[keep], np.asarray(q, np.int64)[keep]
    order = np.lexsort((~np.signbit(v), v))
    v, cum = v[order], np.cumsum(q[order])
    target = max(1, int(np.ceil(np.float64(p) * np.float64(int(cum[-1])))))
    return v[np.searchsorted(cum, target, side="left")]


def adjust_group(x_joint, npar, mom, sc, tol, kernel, ridge, probs, lb, ub):
    """one group's outputs from its pooled joint columns x_joint [np + nm][m] (moment_stats_ref.joint_columns' order: the parameters,
    then the simulated moments): a dict of FIELDS without count and n_chains"""
    D, m = x_joint.shape
    nm = D - npar
    nq = len(probs)
    nan = lambda *s: np.full(s, np.nan)
    out = dict(status=0, n_kept=0, bandwidth=np.nan, sum_w=np.nan, ess=np.nan, x_mean=nan(nm), raw_mean=nan(npar), beta=nan(nm, npar),
               adj_mean=nan(npar), adj_sd=nan(npar), adj_quantile=nan(nq, npar), n_outside=np.zeros(npar, np.int64))
    if m < 2:
        out["status"] = 1
        return out
    if not np.isfinite(x_joint).all():
        out["status"] = 2
        return out
    theta = x_joint[:npar]
    x = (x_joint[npar:] - mom[:, None]) / sc[:, None]
    d2 = distances(x)
    delta2 = bandwidth(d2, tol)
    om = row_weights(d2, delta2, kernel)
    r = np.sqrt(om)
    kept = om > 0
    sum_w, sum_w2 = V.chunked_sum(om), V.chunked_sum(om * om)
    out.update(bandwidth=delta2, n_kept=int(kept.sum()), sum_w=sum_w, ess=(sum_w * sum_w) / sum_w2)
    v = np.concatenate([x, theta])                        # the joint columns of the contract: the discrepancies, then the parameters
    mu = V.chunked_sum(om[None, :] * v) / sum_w
    out.update(x_mean=mu[:nm], raw_mean=mu[nm:])
    if (kernel == 1 and not delta2 > 0) or out["n_kept"] < nm + 2:
        out["status"] = 3
        return out
    e = r[None, :] * (v - mu[:, None])
    C = np.empty((D, D))
    for a in range(D):                                    # (row by row: [D][D][m] at once does not fit at the caps)
        C[a] = V.chunked_sum(e[a][None, :] * e)
    A = C[:nm, :nm].copy()
    for k in range(nm):
        A[k, k] = C[k, k] + np.float64(ridge) * C[k, k]
    L, ok = MR.cholesky_columns(A)
    if not ok:
        out["status"] = 4
        return out
    beta = MR.solve_columns(L, C[:nm, nm:])               # [nm][np]
    t, u = np.zeros(npar), np.zeros(npar)
    for k in range(nm):
        t = t + mu[k] * beta[k]
        u = u + beta[k] * C[k, nm:]
    star = np.empty((npar, int(kept.sum())))
    xk = x[:, kept]
    for j in range(npar):
        tt = np.zeros(xk.shape[1])
        for k in range(nm):
            tt = tt + xk[k] * beta[k, j]
        star[j] = theta[j, kept] - tt
    q = int_weights(om[kept])
    out.update(beta=beta, adj_mean=mu[nm:] - t, adj_sd=np.sqrt((np.diagonal(C)[nm:] - u) / sum_w),
               n_outside=((star < lb[:, None]) | (star > ub[:, None])).sum(axis=1).astype(np.int64))
    for i, p in enumerate(probs):
        for j in range(npar):
            out["adj_quantile"][i, j] = weighted_quantile(star[j], q, p)
    return out


def adjustment_from_history(h, t0, t1, select, groups, tol, kernel, scale, ridge, probs, mom, w, lb, ub, n_groups=None):
    """what smm_get_adjustment returns, from a HistoryBuffers of iterations [0, >= t1), the data moments mom [nm], the weights w [nm]
    and the bounds lb, ub [np]; groups None: every chain in group 0; n_groups defaults to groups.max() + 1"""
    N, npar, nm = h.value.shape[1], h.params.shape[1], h.sim_moments.shape[1]
    select = SELECT[select] if isinstance(select, str) else int(select)
    kernel = KERNEL[kernel] if isinstance(kernel, str) else int(kernel)
    groups = np.zeros(N, np.int32) if groups is None else np.asarray(groups, np.int32)
    G = (int(groups.max()) + 1 if len(groups) else 0) if n_groups is None else int(n_groups)
    probs = [float(p) for p in probs]
    mom, lb, ub = np.asarray(mom, np.float64), np.asarray(lb, np.float64), np.asarray(ub, np.float64)
    sc = scales(w, scale)
    cols = MR.joint_columns(h, t0, t1, select, groups, G)
    nq = len(probs)
    out = dict(count=np.array([x.shape[1] for x in cols], np.int64), n_chains=np.array([(groups == g).sum() for g in range(G)], np.int32),
               status=np.zeros(G, np.int32), n_kept=np.zeros(G, np.int64), bandwidth=np.empty(G), sum_w=np.empty(G), ess=np.empty(G),
               x_mean=np.empty((G, nm)), raw_mean=np.empty((G, npar)), beta=np.empty((G, nm, npar)), adj_mean=np.empty((G, npar)),
               adj_sd=np.empty((G, npar)), adj_quantile=np.empty((nq, G, npar)), n_outside=np.zeros((G, npar), np.int64))
    with np.errstate(all="ignore"):
        for g, x in enumerate(cols):
            r = adjust_group(x, npar, mom, sc, tol, kernel, ridge, probs, lb, ub)
            for f, val in r.items():
                if f == "adj_quantile":
                    out[f][:, g] = val
                else:
                    out[f][g] = val
    return out


def assert_adjustment_equal(got, want, fields=None):
    """every field array_equal, NaN equal to NaN (so the quantiles are compared up to the sign of a zero)"""
    for f in fields or [f for f in FIELDS if f in got]:
        a, b = np.asarray(got[f]), np.asarray(want[f])
        assert a.shape == b.shape, (f, a.shape, b.shape)
        if a.dtype.kind == "f":
            bad = ~((a == b) | (np.isnan(a) & np.isnan(b)))
        else:
            bad = a != b
        assert not bad.any(), (f, np.argwhere(bad)[:5], a[bad][:5], b[bad][:5])
