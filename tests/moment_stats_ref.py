"""The numerical contract of smm_get_moment_stats (include/smmhip.h) restated in numpy over a downloaded history: a group's D = np + nm
joint columns (the parameters, then the simulated moments of the same row) pooled over its members' selected rows — every row, the
accepted rows (chain_cov_ref.select's selection) or the state series (trace_ref.state_rows, the look-back of chain_diag_ref) — then
group_stats_ref's mean, covariance and order statistics on them, and the Cholesky factors, substitutions, J'WJ, the sensitivity and the
standard errors in scalar float64 loops in the contract's order.  tests/test_moment_stats.py holds it against group_stats_ref, np.linalg
and the status table; the GPU tests hold the device against it, over the history downloaded with smm_get_history."""
import numpy as np

import group_stats_ref as GS
import trace_ref as TR

SELECT = {"all": 0, "accepted": 1, "state": 2}
FIELDS = ("count", "n_chains", "status", "p_mean", "m_mean", "m_median", "m_quantile", "cov_pp", "cov_pm", "cov_mm", "fit_z", "jac",
          "sens", "se")

# jac against np.linalg.lstsq on the centred columns, sens and se against np.linalg.solve: the largest relative deviation (in units of
# the largest entry of the matrix compared) over the status-0 groups of tests/test_moment_stats.py's cases, measured there on the CPU
# oracle's histories, and the bound the test holds it under: ten times that, the margin for the summation order of the BLAS behind
# np.linalg (the procedure of rank_diag_ref.RANK_RTOL).
MOMENT_LINALG_DEV = 9.41e-15           # measured (test_jac_sens_se_against_numpy_linalg prints it): 9.41e-15 over its 30 groups
MOMENT_LINALG_RTOL = 10 * MOMENT_LINALG_DEV
# the same on crafted_linear's histories of CAP_SHAPES (N = 8, T = 48, two groups, the three selections), and jac against the J_true
# those moments were made from, which the 1e-3 noise moves as well, in units of J_true's largest entry
MOMENT_LINALG_CAPS_DEV = 5.74e-11      # measured (test_jac_sens_se_against_numpy_linalg_at_the_caps prints it): over its 24 status-0 groups
MOMENT_LINALG_CAPS_RTOL = 10 * MOMENT_LINALG_CAPS_DEV
MOMENT_JTRUE_CAPS_DEV = 9.23e-3        # measured by the same test, over the 36 groups whose status is 0 or 4
MOMENT_JTRUE_CAPS_RTOL = 10 * MOMENT_JTRUE_CAPS_DEV


def dense_problem(npar, nm, N, T, seed=3):
    """the synthetic dense objective (SMM_OBJ_DENSE) with np = npar parameters and nm moments, np != nm allowed: the Problem / BGPOpts
    of tests/test_gpu_parity.py's dense_problem"""
    from smm_jl_amd import BGPOpts, Problem, _abi as A
    from smm_jl_amd.workloads import temps
    rng = np.random.default_rng(seed)
    objp = np.concatenate([rng.standard_normal(A.SMM_DENSE_D * npar) / np.sqrt(npar),
                           rng.standard_normal(nm * A.SMM_DENSE_D) / np.sqrt(A.SMM_DENSE_D)])
    prob = Problem(init=rng.uniform(-0.3, 0.3, npar), lb=-np.ones(npar), ub=np.ones(npar), mom=rng.uniform(-0.5, 0.5, nm),
                   w=rng.uniform(0.5, 2.0, nm), ns=1, objective_id=A.SMM_OBJ_DENSE, obj_params=objp)
    opts = BGPOpts(N=N, maxiter=T, sigma=0.02 * temps(N, 4), acc_tuner=np.geomspace(20, 1, N) if N > 1 else [2.0],
                   min_improve=np.zeros(N), N_global=N, seed=seed)
    return prob, opts


def copy_history(h):
    """a HistoryBuffers with h's contents, to craft a history from"""
    from smm_jl_amd import _abi as A
    c = A.HistoryBuffers(h.value.shape[0], h.value.shape[1], h.params.shape[1], h.sim_moments.shape[1])
    for f in A.HistoryBuffers.FIELDS:
        getattr(c, f)[...] = getattr(h, f)
    return c


def joint_columns(h, t0, t1, select, groups, G):
    """the pooled joint columns X [D][m_g] of every group: the members in ascending index, each member's selected rows in iteration
    order; a state row that does not exist yet is NaN"""
    npar, nm = h.params.shape[1], h.sim_moments.shape[1]
    a = TR.state_rows(h.accepted, t1) if select == 2 else None
    out = []
    for g in range(G):
        blocks = []
        for c in np.flatnonzero(groups == g):
            if select == 1:
                src = t0 + np.flatnonzero(h.accepted[t0:t1, c] != 0)
            elif select == 0:
                src = np.arange(t0, t1)
            else:
                src = a[t0:t1, c]
            ok = src >= 0
            b = np.full((npar + nm, len(src)), np.nan)
            b[:npar, ok] = h.params[src[ok], :, c].T
            b[npar:, ok] = h.sim_moments[src[ok], :, c].T
            blocks.append(b)
        out.append(np.ascontiguousarray(np.concatenate(blocks, axis=1)) if blocks else np.empty((npar + nm, 0)))
    return out


def cholesky(A):
    """(L, ok) of the lower triangle of A [n][n] in the contract's order (chain_cov_ref.cholesky's, one matrix, scalar loops)"""
    n = A.shape[0]
    L = np.zeros((n, n))
    for k in range(n):
        for j in range(k + 1):
            s = np.float64(A[k, j])
            for i in range(j):
                s = s - L[k, i] * L[j, i]
            if j == k:
                if not s > 0:
                    return L, False
                L[k, k] = np.sqrt(s)
            else:
                L[k, j] = s / L[j, j]
    return L, True


def solve(L, b):
    """x of L L' x = b: forward, then back substitution, the products subtracted one by one in ascending index"""
    n = L.shape[0]
    x = np.array(b, np.float64)
    for i in range(n):
        s = x[i]
        for j in range(i):
            s = s - L[i, j] * x[j]
        x[i] = s / L[i, i]
    for i in range(n - 1, -1, -1):
        s = x[i]
        for j in range(i + 1, n):
            s = s - L[j, i] * x[j]
        x[i] = s / L[i, i]
    return x


def cholesky_columns(A):
    """cholesky's (L, ok) column by column, the rows below a pivot at once: every entry by cholesky's operations in cholesky's order
    (tests/test_moment_stats.py holds the two equal bit for bit), in O(n^2) numpy calls for the shapes at the size cap"""
    n = A.shape[0]
    L = np.zeros((n, n))
    for j in range(n):
        s = np.array(A[j:, j], np.float64)
        for i in range(j):
            s = s - L[j:, i] * L[j, i]
        if not s[0] > 0:
            return L, False
        L[j, j] = np.sqrt(s[0])
        L[j + 1:, j] = s[1:] / L[j, j]
    return L, True


def solve_columns(L, B):
    """solve's x for every column of B [n][r] at once: the same subtractions in the same order, column by column"""
    n = L.shape[0]
    x = np.array(B, np.float64)
    for i in range(n):
        s = x[i].copy()
        for j in range(i):
            s = s - L[i, j] * x[j]
        x[i] = s / L[i, i]
    for i in range(n - 1, -1, -1):
        s = x[i].copy()
        for j in range(i + 1, n):
            s = s - L[j, i] * x[j]
        x[i] = s / L[i, i]
    return x


def weights(w):
    """(s, W): s_k = w_k if finite and not zero, else 1.0; W_k = 1.0 / (s_k * s_k)"""
    w = np.asarray(w, np.float64)
    s = np.where(np.isfinite(w) & (w != 0), w, 1.0)
    return s, 1.0 / (s * s)


def linear_part(cov_pp, cov_pm, w, ridge):
    """(status, jac [nm][np], sens [np][nm], se [np]) from the covariance blocks of one group: status 0, 3 or 4"""
    npar, nm = cov_pm.shape
    jac, sens, se = np.full((nm, npar), np.nan), np.full((npar, nm), np.nan), np.full(npar, np.nan)
    A = np.array(cov_pp, np.float64)
    for j in range(npar):
        A[j, j] = cov_pp[j, j] + np.float64(ridge) * cov_pp[j, j]
    L, ok = cholesky(A)
    if not ok:
        return 3, jac, sens, se
    for k in range(nm):
        jac[k] = solve(L, cov_pm[:, k])
    s, W = weights(w)
    B = np.zeros((npar, npar))
    for i in range(npar):
        for j in range(i + 1):
            S = np.float64(0.0)
            for k in range(nm):
                S = S + (jac[k, i] * W[k]) * jac[k, j]
            B[i, j] = S
    LB, ok = cholesky(B)
    if not ok:
        return 4, jac, sens, se
    for k in range(nm):
        sens[:, k] = solve(LB, [-(jac[k, i] * W[k]) for i in range(npar)])
    for j in range(npar):
        S = np.float64(0.0)
        for k in range(nm):
            S = S + (sens[j, k] * sens[j, k]) * (s[k] * s[k])
        se[j] = np.sqrt(S)
    return 0, jac, sens, se


def linear_part_columns(cov_pp, cov_pm, w, ridge):
    """linear_part's (status, jac, sens, se), bit for bit (tests/test_moment_stats.py), through cholesky_columns and solve_columns:
    what moment_stats_from_history calls, so that np = nm = 64 takes milliseconds"""
    npar, nm = cov_pm.shape
    jac, sens, se = np.full((nm, npar), np.nan), np.full((npar, nm), np.nan), np.full(npar, np.nan)
    A = np.array(cov_pp, np.float64)
    for j in range(npar):
        A[j, j] = cov_pp[j, j] + np.float64(ridge) * cov_pp[j, j]
    L, ok = cholesky_columns(A)
    if not ok:
        return 3, jac, sens, se
    jac = np.ascontiguousarray(solve_columns(L, cov_pm).T)
    s, W = weights(w)
    B = np.zeros((npar, npar))
    for k in range(nm):
        B = B + (jac[k][:, None] * W[k]) * jac[k][None, :]
    LB, ok = cholesky_columns(B)
    if not ok:
        return 4, jac, sens, se
    sens = solve_columns(LB, -(jac.T * W[None, :]))
    S = np.zeros(npar)
    for k in range(nm):
        S = S + (sens[:, k] * sens[:, k]) * (s[k] * s[k])
    return 0, jac, sens, np.sqrt(S)


def crafted_linear(npar, nm, N, T, seed, into=None):
    """(h, J_true): a history whose moments are linear in the parameters, written into the HistoryBuffers `into` (default: a zeroed
    one of T iterations, N chains) — params i.i.d. standard normal scaled per column by geomspace(1, 1e-2, np), sim_moments = J_true
    theta + 1e-3 noise with J_true [nm][np] standard normal, value half the squared distance of the moments from 0, accepted a 0/1
    pattern at rate 0.7 whose row 0 is accepted in every chain (the state series exists from the first row).  Only these four fields
    are written; everything is a function of the arguments"""
    from smm_jl_amd import _abi as A
    if into is None:
        into = A.HistoryBuffers(T, N, npar, nm)
        for f in A.HistoryBuffers.FIELDS:
            getattr(into, f)[...] = 0
    assert into.params.shape == (T, npar, N) and into.sim_moments.shape == (T, nm, N)
    rng = np.random.default_rng([seed, npar, nm, N, T])
    J = rng.standard_normal((nm, npar))
    theta = rng.standard_normal((T, npar, N)) * np.geomspace(1.0, 1e-2, npar)[None, :, None]
    mom = np.einsum("kj,tjc->tkc", J, theta) + 1e-3 * rng.standard_normal((T, nm, N))
    acc = (rng.random((T, N)) < 0.7).astype(np.uint8)
    acc[0] = 1
    into.params[...], into.sim_moments[...], into.accepted[...] = theta, mom, acc
    into.value[...] = 0.5 * (mom * mom).sum(axis=1)
    return into, J


CAP_SHAPES = ((1, 1), (1, 64), (64, 1), (64, 64), (63, 34), (33, 64))   # (np, nm) of crafted_linear's cases: the caps, and D = 97 twice


def moment_stats_from_history(h, t0, t1, select, groups, probs, ridge, mom, w, n_groups=None):
    """what smm_get_moment_stats returns, from a HistoryBuffers of iterations [0, >= t1), the data moments mom [nm] and the weights w
    [nm]; groups None: every chain in group 0; n_groups defaults to groups.max() + 1"""
    N, npar, nm = h.value.shape[1], h.params.shape[1], h.sim_moments.shape[1]
    select = SELECT[select] if isinstance(select, str) else int(select)
    groups = np.zeros(N, np.int32) if groups is None else np.asarray(groups, np.int32)
    G = (int(groups.max()) + 1 if len(groups) else 0) if n_groups is None else int(n_groups)
    probs = [float(p) for p in probs]
    mom = np.asarray(mom, np.float64)
    cols = joint_columns(h, t0, t1, select, groups, G)
    out = dict(count=np.array([x.shape[1] for x in cols], np.int64), n_chains=np.array([(groups == g).sum() for g in range(G)], np.int32),
               status=np.zeros(G, np.int32), p_mean=np.full((G, npar), np.nan), m_mean=np.full((G, nm), np.nan),
               m_median=np.full((G, nm), np.nan), m_quantile=np.full((len(probs), G, nm), np.nan), cov_pp=np.full((G, npar, npar), np.nan),
               cov_pm=np.full((G, npar, nm), np.nan), cov_mm=np.full((G, nm, nm), np.nan), fit_z=np.full((G, nm), np.nan),
               jac=np.full((G, nm, npar), np.nan), sens=np.full((G, npar, nm), np.nan), se=np.full((G, npar), np.nan))
    with np.errstate(all="ignore"):
        for g, x in enumerate(cols):
            m = x.shape[1]
            if m < 2:
                out["status"][g] = 1
            elif not np.isfinite(x).all():
                out["status"][g] = 2
                continue                                  # everything but the counts NaN
            mean, cov = GS.column_cov(x)
            out["p_mean"][g], out["m_mean"][g] = mean[:npar], mean[npar:]
            for k in range(nm):
                out["m_median"][g, k], out["m_quantile"][:, g, k] = GS.order_stats(x[npar + k], probs)
            if m < 2:
                continue                                  # the covariances and everything derived NaN
            out["cov_pp"][g], out["cov_pm"][g], out["cov_mm"][g] = cov[:npar, :npar], cov[:npar, npar:], cov[npar:, npar:]
            out["fit_z"][g] = (mean[npar:] - mom) / np.sqrt(np.diagonal(cov[npar:, npar:]))
            out["status"][g], out["jac"][g], out["sens"][g], out["se"][g] = linear_part_columns(cov[:npar, :npar], cov[:npar, npar:], w, ridge)
    return out


def assert_moment_stats_equal(got, want, fields=None):
    """every field array_equal, NaN equal to NaN (so the order statistics are compared up to the sign of a zero)"""
    for f in fields or [f for f in FIELDS if f in got]:
        a, b = np.asarray(got[f]), np.asarray(want[f])
        assert a.shape == b.shape, (f, a.shape, b.shape)
        if a.dtype.kind == "f":
            bad = ~((a == b) | (np.isnan(a) & np.isnan(b)))
        else:
            bad = a != b
        assert not bad.any(), (f, np.argwhere(bad)[:5], a[bad][:5], b[bad][:5])
