"""smm_opt_lm's numerical contract (include/smmhip.h) in numpy: K Levenberg–Marquardt searches inside the box advancing together, over an
injected `evaluator(P [np][n]) -> (value [n], simM [nm][n], status [n])`.  Least squares on the residuals r = (sim - mom) / s with forward-
difference Jacobians, an active set at the bounds and lambda on the diagonal of J'J; every sum runs in ascending index with every operation
rounded on its own, and the factorisation and the substitutions are smm_get_moment_stats' (moment_stats_ref.cholesky, solve).  One evaluator
call per phase of a lock-step iteration for all searches in it (the Jacobians' points; a round of tries).  Beyond the contract it counts, per
search, the branches taken: `backward` differences, active coordinates met (`met_active`), `rejected` tries (evaluated and refused; of
those `not_finite` for a residual that was not finite) and `pivot` failures (tries without a factor, which cost no evaluation)."""
import numpy as np

from moment_stats_ref import cholesky, solve

FIELDS = ("best", "value", "sim_moments", "ssr", "grad", "jac", "lambda", "step", "dF", "active", "iterations", "tries", "n_eval", "status")


def scales(w):
    w = np.asarray(w, float)
    return np.where(np.isfinite(w) & (w != 0), w, 1.0)


def shifted(x, lb, ub, fd_step):
    """(y, backward): the shifted coordinate of every Jacobian point, forward, or backward where forward leaves the box"""
    h = fd_step * (ub - lb)
    y = x + h
    back = y > ub
    return np.where(back, x - h, y), back


def sum_in_order(terms):
    """0.0 + t_0 + t_1 + ... along axis 0"""
    acc = np.zeros(terms.shape[1:])
    for t in terms:
        acc = acc + t
    return acc


def opt_lm(evaluator, starts, lb, ub, mom, w, fd_step=1e-4, lambda0=1e-3, lambda_up=10.0, lambda_down=10.0, xtol=1e-8, ftol=1e-12, gtol=0.0,
           max_iter=100, max_tries=12):
    starts = np.array(starts, float)
    N, K = starts.shape
    lb, ub, mom, s = np.asarray(lb, float), np.asarray(ub, float), np.asarray(mom, float), scales(w)
    nm = len(mom)
    lambda_up, lambda_down = float(lambda_up), float(lambda_down)
    assert K >= 1 and 0 < fd_step <= 0.5 and 0 < lambda0 < np.inf and lambda_up > 1 and lambda_down >= 1
    assert xtol >= 0 and ftol >= 0 and gtol >= 0 and max_iter >= 1 and max_tries >= 1
    assert np.all((starts >= lb[:, None]) & (starts <= ub[:, None]))

    x = starts.T.copy()                                     # [K][N]
    r = np.full((K, nm), np.nan)
    F, value, simM = np.full(K, np.nan), np.full(K, np.nan), np.full((K, nm), np.nan)
    grad, jac = np.full((K, N), np.nan), np.full((K, nm, N), np.nan)
    lam, step, dF = np.full(K, float(lambda0)), np.full(K, np.nan), np.full(K, np.nan)
    active = np.zeros((K, N), np.int32)
    iterations, tries, n_eval, status = (np.zeros(K, np.int32) for _ in range(4))
    backward, met_active, rejected, not_finite, pivot = (np.zeros(K, np.int32) for _ in range(5))
    calls = [0]

    def evaluate(X):
        """X [n][N] -> values [n], moments [n][nm], residuals [n][nm], F [n]"""
        calls[0] += 1
        v, sm, _ = evaluator(np.ascontiguousarray(X.T))
        v, sm = np.asarray(v, float), np.asarray(sm, float).T
        with np.errstate(all="ignore"):
            res = (sm - mom) / s
            return v, sm, res, sum_in_order((res * res).T)

    with np.errstate(all="ignore"):
        value[:], simM[:], r[:], F[:] = evaluate(x)
        n_eval += 1
        run = []
        for q in range(K):
            if np.all(np.isfinite(r[q])):
                run.append(q)
            else:
                status[q] = 2
        while run:
            # the Jacobians: np points per running search, one launch
            pts = np.repeat(x[run], N, axis=0)              # evaluation a * N + k
            ys, dk = {}, {}
            for a, q in enumerate(run):
                y, back = shifted(x[q], lb, ub, fd_step)
                backward[q] += int(back.sum())
                dk[q] = y - x[q]
                pts[a * N + np.arange(N), np.arange(N)] = y
            _, _, rp, _ = evaluate(pts)
            g0, Amat, trying = {}, {}, []
            for a, q in enumerate(run):
                iterations[q] += 1
                n_eval[q] += N
                J = (rp[a * N:(a + 1) * N].T - r[q][:, None]) / dk[q][None, :]       # [nm][N]
                jac[q] = J
                if not np.all(np.isfinite(J)):
                    status[q] = 2
                    continue
                g = sum_in_order(J * r[q][:, None])
                A = sum_in_order(J[:, :, None] * J[:, None, :])       # (A_kl = 0.0 + J_0k J_0l + ...: every entry's own sum over j)
                grad[q] = g
                act = ((x[q] == lb) & (g > 0)) | ((x[q] == ub) & (g < 0))
                active[q] = act
                met_active[q] += int(act.sum())
                free = ~act
                if np.any(free & (np.diag(A) == 0)):
                    status[q] = 4
                    continue
                if np.all(np.abs(g[free]) <= gtol):
                    status[q] = 1
                    continue
                g = np.where(act, 0.0, g)
                for k in np.flatnonzero(act):
                    A[k, :] = 0.0
                    A[:, k] = 0.0
                    A[k, k] = 1.0
                g0[q], Amat[q] = g, A
                trying.append(q)
            # rounds of tries: one point per search with a factor, one launch
            go, made = [], {q: 0 for q in trying}
            while trying:
                cand = {}
                for q in trying:
                    B = Amat[q].copy()
                    for k in range(N):
                        B[k, k] = Amat[q][k, k] + lam[q] * Amat[q][k, k]
                    L, ok = cholesky(B)
                    if ok:
                        cand[q] = np.minimum(np.maximum(x[q] + solve(L, -g0[q]), lb), ub)
                with_point = [q for q in trying if q in cand]
                if with_point:
                    v, sm, rn, Fn = evaluate(np.array([cand[q] for q in with_point]))
                again = []
                for q in trying:
                    tries[q] += 1
                    made[q] += 1
                    accept = False
                    if q in cand:
                        b = with_point.index(q)
                        n_eval[q] += 1
                        accept = bool(np.all(np.isfinite(rn[b])) and Fn[b] < F[q])
                        if not accept:
                            rejected[q] += 1
                            not_finite[q] += int(not np.all(np.isfinite(rn[b])))
                    else:
                        pivot[q] += 1
                    if accept:
                        step[q] = np.max(np.abs(cand[q] - x[q]))
                        dF[q] = F[q] - Fn[b]
                        x[q], r[q], F[q], value[q], simM[q] = cand[q], rn[b], Fn[b], v[b], sm[b]
                        lam[q] = max(lam[q] / lambda_down, 1e-300)
                        if step[q] <= xtol or dF[q] <= ftol * F[q]:
                            status[q] = 1
                        elif iterations[q] >= max_iter:
                            status[q] = 0
                        else:
                            go.append(q)
                    else:
                        lam[q] = lam[q] * lambda_up
                        if not np.isfinite(lam[q]) or made[q] >= max_tries:
                            status[q] = 3
                        else:
                            again.append(q)
                trying = again
            run = sorted(go)
    return {"best": x.T.copy(), "value": value, "sim_moments": simM.T.copy(), "ssr": F, "grad": grad.T.copy(),
            "jac": jac.transpose(1, 2, 0).copy(), "lambda": lam, "step": step, "dF": dF, "active": active.T.copy(), "iterations": iterations,
            "tries": tries, "n_eval": n_eval, "status": status, "evaluated": int(n_eval.sum()), "backward": backward, "met_active": met_active,
            "rejected": rejected, "not_finite": not_finite, "pivot": pivot, "launches": calls[0]}


def assert_equal(got, want):
    """every output field bit for bit (NaN equal to NaN), and the evaluation count"""
    for f in FIELDS:
        assert got[f].shape == want[f].shape, (f, got[f].shape, want[f].shape)
        assert np.array_equal(got[f], want[f], equal_nan=got[f].dtype.kind == "f"), (f, got[f], want[f])
    assert got["evaluated"] == want["evaluated"], (got["evaluated"], want["evaluated"])
