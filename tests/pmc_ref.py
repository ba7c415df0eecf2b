"""smm_abc_pmc's numerical contract (include/smmhip.h) in numpy: the adaptive population Monte Carlo ABC sampler of Lenormand, Jabot & Deffuant
(2013) over an injected `evaluator(P [np][n]) -> (value [n], simM [nm][n], status [n])`.  Built only from what the tests already use: the
oracle's Philox and its elementary functions (oracle.contract_math: log, exp, sin2pi, cos2pi) for the uniforms, Box–Muller and the weights;
chain_cov_ref's chunked pairwise sum and Cholesky order; reweight_ref's total order and integer-weight quantile.  The generation loop, the
select, the integer CDF, the whitening and the blocked sum T are stated here.  One evaluator call per generation: also the host loop the
library offered before the device call (tools/abc_pmc_time.py).  Beyond the contract it keeps, per generation, what the tests assert on the
restatement alone (`trace`: Sigma, L, logc, the parents, r, the prefix, the new particles' u, inside, D; `selects`: every generation's
candidate distances, how many of them are old, and the candidates kept)."""
import numpy as np

import chain_cov_ref as CR
import reweight_ref as RW

STREAM_PMC = 8
Q_ONE = 1048576.0
T_BLOCK = 256
HALF_LOG_2PI = 0.9189385332046727
DBL_MAX = np.finfo(np.float64).max
DBL_MIN = np.finfo(np.float64).tiny
GEN_FIELDS = ("eps", "p_acc", "gen_ess", "n_outside", "n_invalid", "n_underflow", "n_new_kept")
FIELDS = ("theta", "value", "sim_moments", "weight", "logw", "born") + GEN_FIELDS + ("mean", "cov", "quantile")
SCALARS = ("ess", "n_kept", "generations", "status", "evaluated")


def key_of(seed):
    return [seed & 0xffffffff, ((seed >> 32) ^ (STREAM_PMC * 0x9E3779B9)) & 0xffffffff]


def u53(hi, lo):
    return float(((hi << 32) | lo) >> 11) * 2.0 ** -53


def u53_open0(hi, lo):
    return float((((hi << 32) | lo) >> 11) + 1) * 2.0 ** -53


def prior_u(O, seed, npar, P):
    """generation 0: u [np][P], particle j, parameter k from the block at counter {j, 0, k >> 1, 0}"""
    key = key_of(seed)
    u = np.empty((npar, P))
    for j in range(P):
        for q in range((npar + 1) // 2):
            x = O.philox([j, 0, q, 0], key)
            u[2 * q, j] = u53(x[0], x[1])
            if 2 * q + 1 < npar:
                u[2 * q + 1, j] = u53(x[2], x[3])
    return u


def normals(O, seed, npar, g, n):
    """n [np][n]: the library's box_muller of the block at counter {j, g, m, 2}: normals 2m and 2m + 1 of new particle j"""
    key = key_of(seed)
    nq = (npar + 1) // 2
    u1, u2 = np.empty((nq, n)), np.empty((nq, n))
    for j in range(n):
        for m in range(nq):
            x = O.philox([j, g, m, 2], key)
            u1[m, j], u2[m, j] = u53_open0(x[0], x[1]), u53(x[2], x[3])
    r = np.sqrt(-2.0 * O.contract_math("log", u1))
    z0, z1 = r * O.contract_math("cos2pi", u2), r * O.contract_math("sin2pi", u2)
    out = np.empty((npar, n))
    out[0::2] = z0
    out[1::2] = z1[:npar // 2]
    return out


def parent_draws(O, seed, g, n):
    key = key_of(seed)
    v = np.empty(n)
    for j in range(n):
        x = O.philox([j, g, 0, 1], key)
        v[j] = u53(x[0], x[1])
    return v


def to_theta(u, lb, ub):
    """mapto_ab as the kernels compute it: u * (ub - lb) + lb"""
    lb, ub = np.asarray(lb, float)[:, None], np.asarray(ub, float)[:, None]
    return u * (ub - lb) + lb


def distance(value, status):
    """rho, and which evaluations are invalid"""
    value, status = np.asarray(value, float), np.asarray(status)
    with np.errstate(invalid="ignore"):
        ok = (status >= 1) & (np.abs(value) <= DBL_MAX)
    return np.where(ok, value, np.inf), ~ok


def select(rho, A):
    """the candidates kept, in candidate order: A' = min(A, finite ones) with the smallest rho by the IEEE total order, ties to the earlier"""
    rho = np.asarray(rho, float)
    Ap = min(A, int((rho < np.inf).sum()))
    order = np.argsort(RW.total_order_key(rho), kind="stable")[:Ap]
    return np.sort(order)


def sampling_weights(O, lw):
    """(q [A'] int64, prefix [A'] int64, Q, wn [A'], ess)"""
    lw = np.asarray(lw, float)
    if len(lw) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), 0, np.zeros(0), np.nan
    w = O.contract_math("exp", lw - lw.max())
    q = np.maximum(np.ceil(w * Q_ONE), 1.0).astype(np.int64)
    Q = int(q.sum())
    q2 = sum(int(v) * int(v) for v in q)
    wn = q.astype(np.float64) / np.float64(Q)
    ess = (np.float64(Q) * np.float64(Q)) / np.float64(q2)
    return q, np.cumsum(q) - q, Q, wn, ess


def weighted_moments(x, wn):
    """mean [np] = S(wn x), C [np][np] = S(e e'), e = sqrt(wn) (x - mean): the chunked pairwise sums over the kept particles"""
    mean = CR.chunked_sum(wn[None, :] * x)
    e = np.sqrt(wn)[None, :] * (x - mean[:, None])
    C = np.empty((x.shape[0], x.shape[0]))
    for a in range(x.shape[0]):                          # (row by row: np x A doubles at a time)
        C[a] = CR.chunked_sum(e[a][None, :] * e)
    return mean, C


def kernel_factor(O, C, scale, ridge):
    """(Sigma, L, ok, logc)"""
    npar = C.shape[0]
    Sigma = scale * C
    for k in range(npar):
        Sigma[k, k] = Sigma[k, k] + ridge
    L, ok = CR.cholesky(Sigma[None])
    L, ok = np.tril(L[0]), bool(ok[0])
    logc = np.nan
    if ok:
        t = 0.0
        for k in range(npar):
            t = t + O.contract_math("log", np.array([L[k, k]]))[0]
        logc = -(np.float64(npar) * HALF_LOG_2PI) - t
    return Sigma, L, ok, logc


def whiten(L, u):
    """z [np][n] = L^-1 u by forward substitution"""
    z = np.empty_like(u)
    for k in range(u.shape[0]):
        s = u[k].copy()
        for m in range(k):
            s = s - L[k, m] * z[m]
        z[k] = s / L[k, k]
    return z


def step(L, n):
    """y [np][n] = L n: products rounded, added left to right (the Cholesky step of smm_propose.hpp)"""
    y = np.empty_like(n)
    for k in range(n.shape[0]):
        acc = L[k, 0] * n[0]
        for m in range(1, k + 1):
            acc = acc + L[k, m] * n[m]
        y[k] = acc
    return y


def inside_box(u):
    """a particle is inside when 0 <= u_k <= 1 for every k: inclusive bounds, a NaN fails"""
    with np.errstate(invalid="ignore"):
        return ((u >= 0.0) & (u <= 1.0)).all(0)


def mixture(O, z_new, z_kept, wn):
    """D [n]: T over the kept particles in stored order — blocks of 256, each from 0.0 left to right, the block sums from 0.0 left to right"""
    n = z_new.shape[1]
    D, b = np.zeros(n), np.zeros(n)
    for i in range(z_kept.shape[1]):
        d = z_new[0] - z_kept[0, i]
        d2 = d * d
        for k in range(1, z_new.shape[0]):
            d = z_new[k] - z_kept[k, i]
            d2 = d2 + d * d
        b = b + wn[i] * O.contract_math("exp", -0.5 * d2)
        if (i + 1) % T_BLOCK == 0 or i + 1 == z_kept.shape[1]:
            D = D + b
            b = np.zeros(n)
    return D


def abc_pmc(O, evaluator, seed, lb, ub, nm, P, A, max_gen, p_acc_min=0.05, scale=2.0, ridge=0.0, probs=()):
    lb, ub = np.asarray(lb, float), np.asarray(ub, float)
    npar = len(lb)
    assert 2 <= A < P <= 2 ** 22 and max_gen >= 0 and 0 <= p_acc_min < 1 and scale > 0 and ridge >= 0
    G1 = max_gen + 1
    gen = dict(eps=np.full(G1, np.nan), p_acc=np.full(G1, np.nan), gen_ess=np.full(G1, np.nan), n_outside=np.full(G1, -1, np.int32),
               n_invalid=np.full(G1, -1, np.int32), n_underflow=np.full(G1, -1, np.int32), n_new_kept=np.full(G1, -1, np.int32))
    trace, selects = [], []

    def evaluate(theta):
        v, sm, st = evaluator(np.ascontiguousarray(theta))
        rho, bad = distance(v, st)
        return rho, np.asarray(sm, float), int(bad.sum())

    # generation 0
    u_new = prior_u(O, seed, npar, P)
    th_new = to_theta(u_new, lb, ub)
    rho_new, mom_new, n_inv = evaluate(th_new)
    lw_new = np.zeros(P)
    evaluated = P
    gen["n_outside"][0], gen["n_invalid"][0], gen["n_underflow"][0] = 0, n_inv, 0
    K = dict(u=np.empty((npar, 0)), th=np.empty((npar, 0)), mom=np.empty((nm, 0)), rho=np.empty(0), lw=np.empty(0), born=np.empty(0, np.int32))
    g, n_acc, status = 0, None, None
    while True:
        # the select over the kept, then the new
        nk_old, n_new = K["rho"].shape[0], rho_new.shape[0]
        cand = dict(u=np.concatenate([K["u"], u_new], 1), th=np.concatenate([K["th"], th_new], 1), mom=np.concatenate([K["mom"], mom_new], 1),
                    rho=np.concatenate([K["rho"], rho_new]), lw=np.concatenate([K["lw"], lw_new]),
                    born=np.concatenate([K["born"], np.full(n_new, g, np.int32)]))
        keep = select(cand["rho"], A)
        K = {f: (v[:, keep] if v.ndim == 2 else v[keep]) for f, v in cand.items()}
        Ap = len(keep)
        gen["eps"][g] = K["rho"][np.argmax(RW.total_order_key(K["rho"]))] if Ap else np.nan      # (by the select's order: +0.0 above -0.0)
        selects.append(dict(rho=cand["rho"], nk_old=nk_old, keep=keep))
        gen["n_new_kept"][g] = int((keep >= nk_old).sum())
        if g >= 1:
            gen["p_acc"][g] = np.float64(n_acc) / np.float64(n_new)
        q, prefix, Q, wn, ess = sampling_weights(O, K["lw"])
        gen["gen_ess"][g] = ess
        if Ap < 2:
            status = 2
        elif g >= 1 and gen["p_acc"][g] <= p_acc_min:
            status = 1
        elif g == max_gen:
            status = 0
        if status is not None:
            break
        # the kernel of the next generation
        mean_u, C = weighted_moments(K["u"], wn)
        Sigma, L, ok, logc = kernel_factor(O, C, scale, ridge)
        t = dict(Sigma=Sigma, L=L, logc=logc, ok=ok, wn=wn, q=q, prefix=prefix, Q=Q, kept_u=K["u"].copy())
        trace.append(t)
        if not ok:
            status = 3
            break
        g += 1
        n_new = P - Ap
        v = parent_draws(O, seed, g, n_new)
        r = np.array([min(int(vj * np.float64(Q)), Q - 1) for vj in v], np.int64)
        parent = np.searchsorted(prefix, r, side="right") - 1
        u_new = K["u"][:, parent] + step(L, normals(O, seed, npar, g, n_new))
        inside = inside_box(u_new)
        th_new = to_theta(u_new, lb, ub)
        rho_new, mom_new, lw_new = np.full(n_new, np.inf), np.full((nm, n_new), np.nan), np.zeros(n_new)
        idx = np.flatnonzero(inside)
        n_inv = 0
        if len(idx):
            rho_new[idx], mom_new[:, idx], n_inv = evaluate(th_new[:, idx])
        evaluated += len(idx)
        gen["n_outside"][g], gen["n_invalid"][g] = n_new - len(idx), n_inv
        wl = np.flatnonzero(rho_new < np.inf)
        D = np.full(n_new, np.nan)
        n_und = 0
        if len(wl):
            D[wl] = mixture(O, whiten(L, u_new[:, wl]), whiten(L, K["u"]), wn)
            under = D[wl] < DBL_MIN
            n_und = int(under.sum())
            rho_new[wl[under]] = np.inf
            good = wl[~under]
            lw_new[good] = -(O.contract_math("log", D[good]) + logc)
        gen["n_underflow"][g] = n_und
        n_acc = int((rho_new < gen["eps"][g - 1]).sum())
        t.update(v=v, r=r, parent=parent, u_new=u_new, inside=inside, D=D, rho_new=rho_new.copy(), lw_new=lw_new.copy(), mom_new=mom_new)
    # the summary, in parameter space
    Ap = K["rho"].shape[0]
    out = dict(theta=np.full((npar, A), np.nan), value=np.full(A, np.nan), sim_moments=np.full((nm, A), np.nan), weight=np.full(A, np.nan),
               logw=np.full(A, np.nan), born=np.full(A, -1, np.int32), **gen)
    out["theta"][:, :Ap], out["value"][:Ap], out["sim_moments"][:, :Ap] = K["th"], K["rho"], K["mom"]
    out["weight"][:Ap], out["logw"][:Ap], out["born"][:Ap] = wn, K["lw"], K["born"]
    nq = len(probs)
    if Ap:
        out["mean"], out["cov"] = weighted_moments(K["th"], wn)
        out["quantile"] = np.array([[RW.weighted_quantile(K["th"][k], q, p) for k in range(npar)] for p in probs]).reshape(nq, npar)
    else:
        out["mean"], out["cov"], out["quantile"] = np.full(npar, np.nan), np.full((npar, npar), np.nan), np.full((nq, npar), np.nan)
    out.update(ess=float(gen["gen_ess"][g]), n_kept=Ap, generations=g, status=status, evaluated=evaluated, trace=trace, selects=selects, q=q, kept_u=K["u"])
    return out


def assert_equal(got, want):
    """every output field bit for bit (NaN equal to NaN; a zero's sign counts: -0.0 is not +0.0), and the scalars"""
    for f in FIELDS:
        a, b = np.asarray(got[f]), np.asarray(want[f])
        assert a.shape == b.shape, (f, a.shape, b.shape)
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), (f, a, b)
        if a.dtype.kind == "f":
            num = ~(np.isnan(a) | np.isnan(b))
            assert np.array_equal(np.signbit(a)[num], np.signbit(b)[num]), (f, a, b)
    for f in SCALARS:
        a, b = got[f], want[f]
        assert a == b or (f == "ess" and np.isnan(a) and np.isnan(b)), (f, a, b)
