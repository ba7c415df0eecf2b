"""The numerical contract of smm_get_reweighted (include/smmhip.h) restated in numpy over a downloaded history: every scored row of a
chain importance-reweighted from the chain's own acc_tuner to a target, each chain self-normalised, the chains of a group combined by
their effective sample sizes.  exp and log are the contract's own (density_ref.contract: the oracle's restatement in C), the sums
chain_stats_ref.pw over chunks of 8192; the selection of the rows, the pair sums and the weighted quantile loop are stated here.
tests/test_reweight.py holds it against identities, a known answer and crafted columns (reweight_craft.py); the GPU tests hold the
device against it, over the history downloaded with smm_get_history."""
import numpy as np

import chain_stats_ref as R
import density_ref as DR

SELECT = {"all": 0, "accepted": 1, "state": 2}
FIELDS = ("count", "n_scored", "n_chains", "status", "chain_n", "chain_ess", "chain_logz", "n_kept", "sum_u", "ess", "mean", "cov",
          "value_mean", "m_mean", "quantile")
Q_ONE = 1048576.0
CHUNK = 8192
DBL_MAX = np.finfo(np.float64).max


def S(x):
    """the chunked pairwise sum: 0.0, then + pw of every chunk of 8192"""
    x = [float(v) for v in x]
    s = 0.0
    for c in range(0, len(x), CHUNK):
        s = s + R.pw(x, c, min(CHUNK, len(x) - c))
    return s


def source_rows(accepted, t0, t1, select, c):
    """the history rows chain c contributes over [t0, t1), one per selected row, -1 for a state row that does not exist yet"""
    acc = accepted[:t1, c] != 0
    if select == 0:
        return np.arange(t0, t1)
    if select == 1:
        return t0 + np.flatnonzero(acc[t0:t1])
    last = -1                                              # a(t): the last accepted row at or before t
    out = np.empty(max(t1 - t0, 0), np.int64)
    for t in range(t1):
        if acc[t]:
            last = t
        if t >= t0:
            out[t - t0] = last
    return out


def scored_rows(value, accepted, t0, t1, select, c):
    """(selected count, the history rows of the scored ones): a row with a source whose value has |v| <= DBL_MAX"""
    src = source_rows(accepted, t0, t1, select, c)
    with np.errstate(invalid="ignore"):
        ok = np.array([s >= 0 and abs(value[s, c]) <= DBL_MAX for s in src], bool)
    return len(src), src[ok]


def chain_weights(v, a_c, target, exp=None, log=None):
    """one chain and one target over the chain's scored values v [n_c]: (w [n_c], L, f_c, chain_ess, chain_logz)"""
    exp, log = exp or DR.contract("exp"), log or DR.contract("log")
    n = len(v)
    if n == 0:
        return np.zeros(0), np.nan, np.nan, 0.0, np.nan
    with np.errstate(all="ignore"):
        d = np.float64(a_c) - np.float64(target)
        lw = d * np.asarray(v, np.float64)
        L = lw.max()
        x = lw - L
        w = exp(x)
        w[x == -np.inf] = 0.0
        sw, sw2 = np.float64(S(w)), np.float64(S(w * w))
        ess = (sw * sw) / sw2
        logz = L + log(np.array([sw / np.float64(n)]))[0]
        return w, L, sw / sw2, ess, logz


def int_weights(u, F):
    """q [m] int64: ceil((u / F) * 2^20) of the kept rows, 0 for a row with u = 0"""
    with np.errstate(all="ignore"):
        q = np.ceil((u / F) * Q_ONE)
    return np.where(u > 0, q, 0.0).astype(np.int64)


def total_order_key(v):
    """the doubles as integers that sort in the IEEE total order (-0.0 before +0.0)"""
    b = np.asarray(v, np.float64).view(np.int64)
    return np.where(b < 0, np.int64(-2 ** 63) - b - 1, b)


def weighted_quantile(v, q, p):
    """the inverted weighted CDF: over the kept rows (q > 0) in the IEEE total order, the first value at which the running sum of q
    reaches max(1, ceil(p * Q))"""
    keep = q > 0
    v, q = np.asarray(v, np.float64)[keep], np.asarray(q, np.int64)[keep]
    order = np.argsort(total_order_key(v), kind="stable")
    Q = int(q.sum())
    target = max(1, int(np.ceil(np.float64(p) * np.float64(Q))))
    run = 0
    for i in order:
        run += int(q[i])
        if run >= target:
            return v[i]
    raise AssertionError("the weights do not reach the target")


def pair_sums(e):
    """C [np][np] of the columns e [np][m]: per chunk of 8192 the pairwise sum of the products, the chunks' sums added in order from 0.0"""
    k = e.shape[0]
    C = np.zeros((k, k))
    for a in range(k):
        for b in range(a + 1):
            C[a, b] = C[b, a] = S(e[a] * e[b])
    return C


def reweight_group(theta, s, v, u, Ls, F, probs, want_cov=True):
    """one (target, group) from its pooled scored rows theta [np][m], s [nm][m], v [m], u [m], the members' L and F: a dict of status,
    n_kept, sum_u, ess, mean, cov, value_mean, m_mean, quantile"""
    npar, nm, m, nq = theta.shape[0], s.shape[0], len(v), len(probs)
    nan = lambda *sh: np.full(sh, np.nan)
    out = dict(status=0, n_kept=0, sum_u=np.nan, ess=np.nan, mean=nan(npar), cov=nan(npar, npar), value_mean=np.nan, m_mean=nan(nm),
               quantile=nan(nq, npar))
    if m < 2:
        out["status"] = 1
        return out
    if not np.isfinite(theta).all():
        out["status"] = 2
        return out
    with np.errstate(all="ignore"):
        sum_u = np.float64(S(u))
        if not np.isfinite(Ls).all() or not np.isfinite(sum_u):
            out["status"] = 3
            return out
        out.update(n_kept=int((u > 0).sum()), sum_u=sum_u, ess=(sum_u * sum_u) / np.float64(S(u * u)))
        mean = np.array([np.float64(S(u * theta[j])) / sum_u for j in range(npar)])
        out.update(mean=mean, value_mean=np.float64(S(u * v)) / sum_u,
                   m_mean=np.array([np.float64(S(u * s[k])) / sum_u for k in range(nm)]))
        if want_cov:
            e = np.sqrt(u)[None, :] * (theta - mean[:, None])
            out["cov"] = pair_sums(e) / sum_u                  # (the weighted population form: no Bessel factor)
        q = int_weights(u, F)
        for i, p in enumerate(probs):
            for j in range(npar):
                out["quantile"][i, j] = weighted_quantile(theta[j], q, p)
    return out


def reweighted_from_history(h, t0, t1, select, groups, targets, probs, acc_tuner, n_groups=None, chain_offset=0, exp=None, log=None,
                            want_cov=True):
    """what smm_get_reweighted returns, from a HistoryBuffers of iterations [0, >= t1) of the local chains and acc_tuner by global chain
    id; groups None: every chain in group 0; n_groups defaults to groups.max() + 1"""
    exp, log = exp or DR.contract("exp"), log or DR.contract("log")
    N, npar, nm = h.value.shape[1], h.params.shape[1], h.sim_moments.shape[1]
    select = SELECT[select] if isinstance(select, str) else int(select)
    groups = np.zeros(N, np.int32) if groups is None else np.asarray(groups, np.int32)
    G = (int(groups.max()) + 1 if len(groups) else 0) if n_groups is None else int(n_groups)
    targets, probs = [float(a) for a in targets], [float(p) for p in probs]
    acc_tuner = np.asarray(acc_tuner, np.float64)
    Rn, nq = len(targets), len(probs)
    out = dict(count=np.zeros(G, np.int64), n_scored=np.zeros(G, np.int64), n_chains=np.array([(groups == g).sum() for g in range(G)], np.int32),
               status=np.zeros((Rn, G), np.int32), chain_n=np.zeros(N, np.int32), chain_ess=np.zeros((Rn, N)), chain_logz=np.full((Rn, N), np.nan),
               n_kept=np.zeros((Rn, G), np.int64), sum_u=np.empty((Rn, G)), ess=np.empty((Rn, G)), mean=np.empty((Rn, G, npar)),
               cov=np.empty((Rn, G, npar, npar)), value_mean=np.empty((Rn, G)), m_mean=np.empty((Rn, G, nm)),
               quantile=np.empty((nq, Rn, G, npar)))
    rows = {}
    for c in np.flatnonzero(groups >= 0):
        n_sel, src = scored_rows(h.value, h.accepted, t0, t1, select, c)
        rows[c] = src
        out["count"][groups[c]] += n_sel
        out["n_scored"][groups[c]] += len(src)
        out["chain_n"][c] = len(src)
    for g in range(G):
        mem = [c for c in np.flatnonzero(groups == g)]
        src = [rows[c] for c in mem]
        theta = np.concatenate([h.params[sr, :, c].T for sr, c in zip(src, mem)], axis=1) if mem else np.empty((npar, 0))
        s = np.concatenate([h.sim_moments[sr, :, c].T for sr, c in zip(src, mem)], axis=1) if mem else np.empty((nm, 0))
        v = np.concatenate([h.value[sr, c] for sr, c in zip(src, mem)]) if mem else np.empty(0)
        for r, a in enumerate(targets):
            us, Ls, fs = [], [], []
            for sr, c in zip(src, mem):
                w, L, f, ess, logz = chain_weights(h.value[sr, c], acc_tuner[chain_offset + c], a, exp, log)
                out["chain_ess"][r, c], out["chain_logz"][r, c] = ess, logz
                if len(sr):
                    with np.errstate(all="ignore"):
                        us.append(w * f)
                    Ls.append(L)
                    fs.append(f)
            u = np.concatenate(us) if us else np.empty(0)
            with np.errstate(all="ignore"):
                F = np.max(fs) if fs else np.nan
            res = reweight_group(theta, s, v, u, np.array(Ls), F, probs, want_cov)
            for f, val in res.items():
                if f == "quantile":
                    out[f][:, r, g] = val
                else:
                    out[f][r, g] = val
    return out


def assert_reweighted_equal(got, want, fields=None):
    """every field array_equal, NaN equal to NaN (so up to the sign of a zero)"""
    for f in fields or [f for f in FIELDS if f in got]:
        a, b = np.asarray(got[f]), np.asarray(want[f])
        assert a.shape == b.shape, (f, a.shape, b.shape)
        if a.dtype.kind == "f":
            bad = ~((a == b) | (np.isnan(a) & np.isnan(b)))
        else:
            bad = a != b
        assert not bad.any(), (f, np.argwhere(bad)[:5], a[bad][:5], b[bad][:5])
