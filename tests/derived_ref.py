"""The numerical contract of smm_get_derived (include/smmhip.h) restated in numpy: the rows of each group are selected and pooled by
hist_ref.columns' rules (select 0 all rows, 1 accepted rows, 2 the state series through a(t); members in ascending index), extended
from the parameters to the simulated moments and the value of the same rows; the transform is a Python callable over whole columns;
the summaries are group_stats_ref's (column_cov, order_stats) on the derived columns.  The contract's exp and log come through
oracle.contract_math (density_ref.contract), as the device's smm_exp / smm_log.  tests/test_derived.py holds it against plain
formulas; the GPU tests hold the device against it, over the history downloaded with smm_get_history.

A transform here is f(theta [np][m], sim [nm][m], value [m], mom, w, udata, tdata) -> [Q][m], every operation in the order of the
device source it restates (numpy rounds each on its own, as -ffp-contract=off does)."""
import numpy as np

import group_stats_ref as GR
import hist_ref as HR


def chain_rows(h, t0, t1, select):
    """the history row of every selected row of every chain, in iteration order: a list [N] of int arrays (-1: a state row with no a(t))"""
    acc = np.asarray(h.accepted)[:t1] != 0
    T, N = acc.shape
    if select == 2:
        a = np.maximum.accumulate(np.where(acc, np.arange(T)[:, None], -1), axis=0)[t0:t1]
        return [a[:, c].copy() for c in range(N)]
    t = np.arange(t0, t1)
    return [t[acc[t0:t1, c]] if select == 1 else t for c in range(N)]


def pooled_rows(h, t0, t1, select, groups, n_groups):
    """(theta [np][m], sim [nm][m], value [m], valid [m]) of every group's pooled rows; a row that is not valid holds NaN"""
    npar, nm = h.params.shape[1], h.sim_moments.shape[1]
    rows = chain_rows(h, t0, t1, select)
    out = []
    for g in range(n_groups):
        th, sm, va, ok = [np.empty((npar, 0))], [np.empty((nm, 0))], [np.empty(0)], [np.empty(0, bool)]
        for c in np.flatnonzero(np.asarray(groups) == g):
            r = rows[c]
            good = r >= 0
            rr = np.where(good, r, 0)
            th.append(np.where(good, h.params[rr, :, c].T, np.nan))
            sm.append(np.where(good, h.sim_moments[rr, :, c].T, np.nan))
            va.append(np.where(good, h.value[rr, c], np.nan))
            ok.append(good)
        out.append((np.concatenate(th, axis=1), np.concatenate(sm, axis=1), np.concatenate(va), np.concatenate(ok)))
    return out


def derived_columns(h, f, Q, t0, t1, select, groups, n_groups, mom, w, udata=(), tdata=()):
    """y [Q][m] of every group: f on the valid rows, NaN on the others (the function is not called for them)"""
    mom, w, udata, tdata = (np.asarray(v, np.float64).reshape(-1) for v in (mom, w, udata, tdata))
    cols = []
    for th, sm, va, ok in pooled_rows(h, t0, t1, select, groups, n_groups):
        y = np.full((Q, len(va)), np.nan)
        if ok.any():
            with np.errstate(all="ignore"):
                got = np.asarray(f(np.ascontiguousarray(th[:, ok]), np.ascontiguousarray(sm[:, ok]), va[ok], mom, w, udata, tdata), np.float64)
            y[:, ok] = np.broadcast_to(got, (Q, int(ok.sum())))
        cols.append(y)
    return cols


def derived_from_history(h, f, Q, t0, t1, select, groups, probs, mom, w, udata=(), tdata=(), n_groups=None):
    """what smm_get_derived returns, from a HistoryBuffers of iterations [0, >= t1); groups None: every chain in group 0"""
    N = h.value.shape[1]
    select = HR.SELECT[select] if isinstance(select, str) else int(select)
    groups = np.zeros(N, np.int32) if groups is None else np.asarray(groups, np.int32)
    G = (int(groups.max()) + 1 if len(groups) else 0) if n_groups is None else int(n_groups)
    probs = [float(p) for p in probs]
    cols = derived_columns(h, f, Q, t0, t1, select, groups, G, mom, w, udata, tdata)
    out = dict(count=np.array([y.shape[1] for y in cols], np.int64), n_chains=np.array([(groups == g).sum() for g in range(G)], np.int32),
               n_nonfinite=np.array([(~np.isfinite(y)).sum(axis=1) for y in cols], np.int64).reshape(G, Q),
               mean=np.empty((G, Q)), median=np.empty((G, Q)), quantile=np.empty((len(probs), G, Q)), cov=np.empty((G, Q, Q)))
    with np.errstate(all="ignore"):
        for g, y in enumerate(cols):
            out["mean"][g], out["cov"][g] = GR.column_cov(y)
            for q in range(Q):
                out["median"][g, q], out["quantile"][:, g, q] = GR.order_stats(y[q], probs)
    return out


def assert_derived_equal(got, want, fields=None):
    """every field bit for bit, NaN equal to NaN"""
    GR.assert_group_stats_equal(got, want, fields)


def identity(Q):
    """out[k] = theta[k], k < Q"""
    return lambda th, sm, va, mom, w, ud, td: th[:Q]


def identity_source(Q):
    return TRANSFORM_HEAD + "{\n    for (int k = 0; k < %d; ++k) out[k] = theta[k];\n}\n" % Q


TRANSFORM_HEAD = ("SMM_USER_TRANSFORM(const double* theta, int np, const double* sim_moments, int nm, double value, const double* mom,\n"
                  "                   const double* w, const double* udata, int n_udata, const double* tdata, int n_tdata, double* out,\n"
                  "                   int n_out)\n")
