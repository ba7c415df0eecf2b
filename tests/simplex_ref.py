"""smm_opt_simplex' numerical contract (include/smmhip.h) in numpy: K Nelder–Mead searches inside the box advancing together, over an injected
`evaluator(P [np][n]) -> (value [n], simM [nm][n], status [n])`.  It is scipy's _minimize_neldermead with bounds and a given initial_simplex
made exact, per search, independent of every other search: a stable sort with NaN last, status 2 where nothing is finite, value = fsim[0].
One evaluator call per phase of a lock-step iteration for all searches in it (reflected points, second points, shrunk vertices): also the
best host loop the library offered before the device call (tools/opt_simplex_time.py).  Beyond the contract it reports, per search, whether
any sort ever saw two equal values or two NaNs (`ties`): scipy's own argsort is not stable, so only tie-free searches can be pinned to it."""
import numpy as np

MOVES = ("reflection", "expansion", "outside", "inside", "shrink")


def coefficients(N, adaptive):
    if adaptive:
        dim = float(N)
        return 1, 1 + 2 / dim, 0.75 - 1 / (2 * dim), 1 - 1 / dim
    return 1, 2, 0.5, 0.5


def initial_simplex(start, lb, ub, step, reflect=True):
    """[N + 1][N]: vertex 0 the start, vertex k + 1 the start with coordinate k at x_k + step * (ub_k - lb_k), reflected at ub_k and clipped
    (reflect=False: before that — what scipy is given, which reflects and clips itself)"""
    N = len(start)
    sim = np.repeat(np.asarray(start, float)[None, :], N + 1, 0)
    for k in range(N):
        y = start[k] + step * (ub[k] - lb[k])
        if reflect:
            if y > ub[k]:
                y = 2 * ub[k] - y
            y = min(max(y, lb[k]), ub[k])
        sim[k + 1, k] = y
    return sim


def sort_key(f):
    """the position of each value in the stable ascending order, NaN last, +inf just before NaN; and whether two values were equal or both NaN"""
    f = np.asarray(f, float)
    n = len(f)
    nan = np.isnan(f)
    order = sorted(range(n), key=lambda i: (bool(nan[i]), 0.0 if nan[i] else f[i]))      # (sorted() is stable)
    fo = f[order]
    ties = bool(np.any((fo[1:] == fo[:-1]) | (np.isnan(fo[1:]) & np.isnan(fo[:-1]))))
    return np.array(order), ties


def opt_simplex(evaluator, starts, lb, ub, nm, step=0.05, adaptive=False, xatol=1e-4, fatol=1e-4, max_iter=None):
    starts = np.array(starts, float)
    N, K = starts.shape
    lb, ub = np.asarray(lb, float), np.asarray(ub, float)
    max_iter = 200 * N if max_iter is None else int(max_iter)
    assert K >= 1 and 0 < step <= 1 and xatol >= 0 and fatol >= 0 and max_iter >= 1
    assert np.all((starts >= lb[:, None]) & (starts <= ub[:, None]))
    rho, chi, psi, sigma = coefficients(N, adaptive)
    c_r, c_e, rhochi, c_c, psirho, c_i = 1 + rho, 1 + rho * chi, rho * chi, 1 + psi * rho, psi * rho, 1 - psi
    clip = lambda x: np.minimum(np.maximum(x, lb), ub)      # noqa: E731

    sim = np.stack([initial_simplex(starts[:, s], lb, ub, step) for s in range(K)])       # [K][N + 1][N]
    fsim = np.full((K, N + 1), np.nan)
    mom = np.full((K, N + 1, nm), np.nan)
    size_x, size_f = np.full(K, np.nan), np.full(K, np.nan)
    iterations, status, n_eval = np.zeros(K, np.int32), np.zeros(K, np.int32), np.zeros(K, np.int32)
    moves = np.zeros((5, K), np.int32)
    ties = np.zeros(K, bool)
    calls = [0]

    def evaluate(X):
        """X [n][N] -> values [n], moments [n][nm]"""
        calls[0] += 1
        v, sm, _ = evaluator(np.ascontiguousarray(X.T))
        return np.asarray(v, float), np.asarray(sm, float).T

    def sort_and_test(s, ended_iteration):
        """the sort and what follows every sort; True: the search goes on"""
        order, t = sort_key(fsim[s])
        ties[s] |= t
        sim[s], fsim[s], mom[s] = sim[s][order], fsim[s][order], mom[s][order]
        if ended_iteration:
            iterations[s] += 1
        if not np.isfinite(fsim[s, 0]):
            status[s] = 2
            return False
        if iterations[s] >= max_iter:
            status[s] = 0
            return False
        with np.errstate(invalid="ignore"):
            size_x[s] = np.max(np.abs(sim[s, 1:] - sim[s, 0]))
            size_f[s] = np.max(np.abs(fsim[s, 0] - fsim[s, 1:]))
        if size_x[s] <= xatol and size_f[s] <= fatol:
            status[s] = 1
            return False
        return True

    v, m = evaluate(sim.reshape(K * (N + 1), N))
    fsim[:], mom[:] = v.reshape(K, N + 1), m.reshape(K, N + 1, nm)
    n_eval += N + 1
    run = [s for s in range(K) if sort_and_test(s, False)]
    while run:
        xbar = {}
        xr = np.empty((len(run), N))
        for a, s in enumerate(run):
            acc = sim[s, 0].copy()
            for j in range(1, N):
                acc = acc + sim[s, j]
            xbar[s] = acc / N
            xr[a] = clip(c_r * xbar[s] - rho * sim[s, N])
        fxr, mxr = evaluate(xr)
        n_eval[run] += 1
        second, kind = [], {}
        for a, s in enumerate(run):
            if fxr[a] < fsim[s, 0]:
                kind[s] = 1
            elif fxr[a] < fsim[s, N - 1]:
                sim[s, N], fsim[s, N], mom[s, N] = xr[a], fxr[a], mxr[a]
                moves[0, s] += 1
                continue
            elif fxr[a] < fsim[s, N]:
                kind[s] = 2
            else:
                kind[s] = 3
            second.append((a, s))
        shrink = []
        if second:
            x2 = np.empty((len(second), N))
            for b, (a, s) in enumerate(second):
                if kind[s] == 1:
                    x2[b] = clip(c_e * xbar[s] - rhochi * sim[s, N])
                elif kind[s] == 2:
                    x2[b] = clip(c_c * xbar[s] - psirho * sim[s, N])
                else:
                    x2[b] = clip(c_i * xbar[s] + psi * sim[s, N])
            f2, m2 = evaluate(x2)
            for b, (a, s) in enumerate(second):
                n_eval[s] += 1
                take = f2[b] < fxr[a] if kind[s] == 1 else f2[b] <= fxr[a] if kind[s] == 2 else f2[b] < fsim[s, N]
                if take:
                    sim[s, N], fsim[s, N], mom[s, N] = x2[b], f2[b], m2[b]
                    moves[kind[s], s] += 1
                elif kind[s] == 1:
                    sim[s, N], fsim[s, N], mom[s, N] = xr[a], fxr[a], mxr[a]
                    moves[0, s] += 1
                else:
                    shrink.append(s)
                    moves[4, s] += 1
        if shrink:
            for s in shrink:
                for j in range(1, N + 1):
                    sim[s, j] = clip(sim[s, 0] + sigma * (sim[s, j] - sim[s, 0]))
            v, m = evaluate(np.concatenate([sim[s, 1:] for s in shrink]))
            for b, s in enumerate(shrink):
                fsim[s, 1:], mom[s, 1:] = v[b * N:(b + 1) * N], m[b * N:(b + 1) * N]
                n_eval[s] += N
        run = [s for s in run if sort_and_test(s, True)]
    return dict(best=sim[:, 0].T.copy(), value=fsim[:, 0].copy(), sim_moments=mom[:, 0].T.copy(), simplex=sim.transpose(1, 2, 0).copy(),
                simplex_value=fsim.T.copy(), size_x=size_x, size_f=size_f, iterations=iterations, status=status, moves=moves, n_eval=n_eval,
                evaluated=int(n_eval.sum()), ties=ties, launches=calls[0])


FIELDS = ("best", "value", "sim_moments", "simplex", "simplex_value", "size_x", "size_f", "iterations", "status", "moves", "n_eval")


def assert_equal(got, want):
    """every output field bit for bit (NaN equal to NaN), and the evaluation count"""
    for f in FIELDS:
        assert got[f].shape == want[f].shape, (f, got[f].shape, want[f].shape)
        assert np.array_equal(got[f], want[f], equal_nan=got[f].dtype.kind == "f"), (f, got[f], want[f])
    assert got["evaluated"] == want["evaluated"], (got["evaluated"], want["evaluated"])
