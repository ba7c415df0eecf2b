"""How often mysample (AlgoBGP.jl:400-410) goes past its first tries, estimated from the chains' states alone: a try of chain c lands in the
unit box with probability  p_in = prod_k [Phi((1 - mu01_k) / sigma) - Phi(-mu01_k / sigma)]  (independent normals around the chain's last
accepted parameters mapped to [0, 1], mprob.jl:248), so the chain is past n tries with probability  p_fail^n,  p_fail = 1 - p_in.  Over the
population: the expected number of chains past n tries in one iteration is  sum_c p_fail_c^n,  and  P(at least one) = 1 - prod_c (1 -
p_fail_c^n).  The states are the oracle's (no GPU): tools/late_tries_estimate.py prints the table for the bench instances, and
tests/test_gpu_late_tries.py requires of each of its instances that the path it tests is the rule there."""
import math

import numpy as np

_erf = np.frompyfunc(math.erf, 1, 1)


def _Phi(x):
    return 0.5 * (1.0 + _erf(np.asarray(x, np.float64) / math.sqrt(2.0)).astype(np.float64))


def p_fail(sigma, la_params, lb, ub):
    """per chain: the probability that ONE try of the next proposal leaves the unit box; sigma [N], la_params [np][N], lb / ub [np]"""
    sigma = np.asarray(sigma, np.float64)
    lb, ub = np.asarray(lb, np.float64)[:, None], np.asarray(ub, np.float64)[:, None]
    mu01 = (np.asarray(la_params, np.float64) - lb) / (ub - lb)
    p_in = np.prod(_Phi((1.0 - mu01) / sigma[None, :]) - _Phi(-mu01 / sigma[None, :]), axis=0)
    return 1.0 - p_in


def past_tries(pf, n):
    """(expected number of chains past n tries, P(at least one chain past n tries)) of one iteration"""
    q = np.asarray(pf, np.float64) ** n
    return float(q.sum()), float(1.0 - np.prod(1.0 - q))


def oracle_series(O, S, prob, opts, T, ns_past=(4, 8), threads=1):
    """the oracle stepped one iteration at a time over T iterations (or up to a hard error): for the proposal of every iteration 2 .. T
    the estimate from the state behind the iteration before it.  Returns (rows, oracle context, error message or None, failing chains);
    rows[i] = (iteration, {n: (expected chains past n tries, P(at least one))}).
    failing chains: the oracle goes through ALL chains of the failing iteration (its message names the last one that failed, and its
    state is then part-way through that iteration).  Every chain that finds no draw in that iteration, 1-based, comes from the oracle
    too: from the state behind the last complete iteration with every sigma but one chain's at 1e-12 (a chain's tries are its own:
    seed, chain, iteration, try), one iteration per chain.  The reference raises at the FIRST of them (map(next_eval, chains))"""
    from smm_jl_amd import _abi as A
    o = O.OracleContext(prob, opts, threads=threads)
    rows, err, failing = [], None, []
    for t in range(1, T + 1):
        if t > 1:
            st = o.state()
            pf = p_fail(st.sigma, st.la_params, prob.lb, prob.ub)
            rows.append((t, {n: past_tries(pf, n) for n in ns_past}))
            hist = o.history()
        try:
            o.step(1)
        except A.SMMHipError as e:
            err = str(e)
            for j in range(opts.N):
                o2 = O.OracleContext(prob, opts)
                s2 = A.StateBuffers(opts.N, prob.np, prob.nm)
                for f in s2.FIELDS:
                    getattr(s2, f)[...] = getattr(st, f)
                s2.iter = st.iter
                s2.sigma[:] = 1e-12
                s2.sigma[j] = st.sigma[j]
                o2.set_state(s2, hist)
                try:
                    o2.step(1)
                except A.SMMHipError:
                    failing.append(j + 1)
            break
    return rows, o, err, failing
