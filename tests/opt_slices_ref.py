"""smm_opt_slices' numerical contract (include/smmhip.h) in numpy: K cyclic coordinate searches on grids advancing together, over an injected
`evaluator(P [np][n]) -> (value [n], simM [nm][n], status [n])`.  It is callers.optSlices made exact, per search, independent of every other
search: the grid is numpy's linspace, the winner the smallest finite value (strict <, lowest g), delta the left-to-right sum of the rounded
squares under a correctly rounded square root.  One evaluator call per coordinate step for all running searches (evaluation i = a * G + g,
a the search's rank among the running ones): also the best host loop the library offered before the device call (tools/opt_slices_time.py)."""
import numpy as np


def grid(lo, hi, G):
    """linspace(lo[s], hi[s], G) for every search s: [G][n].  (np.linspace itself, given arrays, switches ALL columns to the zero-step
    formula when one column's step is zero; the contract is per search)"""
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    d = hi - lo
    step = d / (G - 1)
    g = np.arange(G, dtype=float)[:, None]
    with np.errstate(invalid="ignore"):
        x = np.where(step == 0, (g / (G - 1)) * d + lo, g * step + lo)
    x[G - 1] = hi
    return x


def opt_slices(evaluator, starts, lb, ub, nm, npoints, tol=1e-5, update=None, max_cycles=1000):
    starts = np.array(starts, float)
    np_, K = starts.shape
    G = int(npoints)
    lb, ub = np.asarray(lb, float), np.asarray(ub, float)
    assert K >= 1 and G >= 2 and tol >= 0 and max_cycles >= 1 and (update is None or update > 0)
    assert np.all((starts >= lb[:, None]) & (starts <= ub[:, None]))
    best = starts.copy()
    lo, hi = np.repeat(lb[:, None], K, 1), np.repeat(ub[:, None], K, 1)
    value, simM = np.full(K, np.inf), np.full((nm, K), np.nan)
    delta = np.full(K, np.inf)
    cycle_value = np.full((max_cycles, K), np.nan)
    cycles, converged = np.zeros(K, np.int32), np.zeros(K, np.int32)
    act = np.arange(K)
    evaluated = 0
    for cyc in range(max_cycles):
        n = len(act)
        if n == 0:
            break
        dvec = np.zeros((np_, n))
        for k in range(np_):
            P = np.repeat(best[:, act], G, axis=1)                       # [np][n * G], i = a * G + g
            P[k] = grid(lo[k, act], hi[k, act], G).T.reshape(-1)
            v, sm, _ = evaluator(P)
            evaluated += n * G
            v = np.asarray(v, float).reshape(n, G)
            vf = np.where(np.isfinite(v), v, np.inf)
            g = np.argmin(vf, axis=1)                                    # (the first of equal values)
            won = vf[np.arange(n), g] < np.inf
            iw = np.arange(n) * G + g
            new = np.where(won, P[k, iw], best[k, act])
            dvec[k] = best[k, act] - new
            best[k, act] = new
            value[act] = np.where(won, v[np.arange(n), g], value[act])
            simM[:, act] = np.where(won, np.asarray(sm, float)[:, iw], simM[:, act])
        if update is not None:
            l, h, x = lo[:, act], hi[:, act], best[:, act]
            r = (h - l) / 2
            nl, nh = x - update * r, x + update * r
            lo[:, act] = np.where(l > nl, l, nl)                         # max(nl, l)
            hi[:, act] = np.where(h < nh, h, nh)                         # min(nh, h)
        acc = dvec[0] * dvec[0]
        for k in range(1, np_):
            acc = acc + dvec[k] * dvec[k]
        d = np.sqrt(acc)
        delta[act] = d
        cycle_value[cyc, act] = value[act]
        cycles[act] = cyc + 1
        converged[act] = d <= tol
        act = act[d > tol]
    return dict(best=best, value=value, sim_moments=simM, lo=lo, hi=hi, delta=delta, cycle_value=cycle_value, cycles=cycles,
                converged=converged, evaluated=evaluated)


FIELDS = ("best", "value", "sim_moments", "lo", "hi", "delta", "cycle_value", "cycles", "converged")


def assert_equal(got, want):
    """every output field bit for bit (NaN equal to NaN), and the evaluation count"""
    for f in FIELDS:
        assert got[f].shape == want[f].shape, (f, got[f].shape, want[f].shape)
        assert np.array_equal(got[f], want[f], equal_nan=got[f].dtype.kind == "f"), (f, got[f], want[f])
    assert got["evaluated"] == want["evaluated"], (got["evaluated"], want["evaluated"])
