"""CPU reference of the starting population (include/smmhip.h: smm_set_population, smm_scatter_population), built only from what tests
may use: candidates from the oracle's Philox4x32-10 and the header's contract in numpy, values from OracleContext.eval_batch, the
selection as numpy argmin with the tie and validity rules, the install as OracleContext.set_state(iter = 1) with the one-row history
that iteration 1 of the algorithm defines (AlgoBGP.jl:326-332, set_eval! :220-245)."""
import numpy as np

from smm_jl_amd import _abi as A

STREAM_POP = 7


def unit_draws(O, seed, g, M, npar):
    """u [np][M] of global chain g: block philox({g, m, k >> 1, 0}), u = (x0:x1 >> 11) 2^-53 for even k, from x2:x3 for odd k"""
    key = [seed & 0xffffffff, ((seed >> 32) ^ (STREAM_POP * 0x9E3779B9)) & 0xffffffff]
    u = np.empty((npar, M))
    for m in range(M):
        for q in range((npar + 1) // 2):
            x = O.philox([g, m, q, 0], key)
            u[2 * q, m] = float(((x[0] << 32) | x[1]) >> 11) * 2.0 ** -53
            if 2 * q + 1 < npar:
                u[2 * q + 1, m] = float(((x[2] << 32) | x[3]) >> 11) * 2.0 ** -53
    return u


def candidates(O, prob, opts, M, spread):
    """theta [np][N][M] of the context's local chains (global ids chain_offset + i)"""
    lb, ub, init = prob.lb[:, None], prob.ub[:, None], prob.init[:, None]
    span = ub - lb
    c = (init - lb) / span
    half = spread * 0.5
    lo, hi = np.maximum(0.0, c - half), np.minimum(1.0, c + half)
    out = np.empty((prob.np, opts.N, M))
    for i in range(opts.N):
        u = unit_draws(O, opts.seed, opts.chain_offset + i, M, prob.np)
        step = u * (hi - lo)
        x01 = lo + step
        sc = x01 * span
        out[:, i, :] = sc + lb
    return out


def valid(value, status):
    with np.errstate(invalid="ignore"):
        return (np.asarray(status) >= 1) & np.isfinite(value) & (np.asarray(value) >= 0)


def select(value, status, init_value, init_status, keep_init):
    """pick [N] from the value / status tables [N][M]: the valid candidate with the lowest value, ties to the lowest m; initial_value
    (-1) wins ties with keep_init and is the start when no candidate is valid"""
    value = np.asarray(value, float)
    ok = valid(value, status)
    masked = np.where(ok, value, np.inf)
    pick = np.argmin(masked, axis=1).astype(np.int32)     # the first minimum
    best = masked[np.arange(len(pick)), pick]
    init_ok = bool(valid(np.float64(init_value), init_status))
    use_init = ~ok.any(axis=1)
    if keep_init and init_ok:
        use_init |= init_value <= best
    pick[use_init] = -1
    return pick


def install(o, opts, start, value, sim_moments):
    """the oracle context o at iteration 1 with every chain's first iteration = (start, value, sim_moments)"""
    N, npar, nm = o.N, o.np, o.nm
    hb, sb = A.HistoryBuffers(1, N, npar, nm), A.StateBuffers(N, npar, nm)
    hb.value[0] = value; hb.prob[0] = 1.0; hb.curr_val[0] = value; hb.best_val[0] = value
    hb.params[0] = start; hb.sim_moments[0] = sim_moments
    hb.best_id[0] = 1; hb.exchanged[0] = 0; hb.accepted[0] = 1; hb.status[0] = 1
    sb.iter = 1
    sb.sigma[:] = opts.sigma[opts.chain_offset:opts.chain_offset + N]
    sb.accept_rate[:] = 1.0
    sb.la_value[:] = value; sb.la_prob[:] = 1.0; sb.la_params[...] = start; sb.la_sim_moments[...] = sim_moments; sb.la_status[:] = 1
    sb.n_noex[:] = 1; sb.n_acc_noex[:] = 1
    sb.best_val[:] = value; sb.best_id[:] = 1
    o.set_state(sb, hb)
    return o


def set_population(O, prob, opts, tables, starts, **kw):
    """(oracle context at iteration 1, the call's results)"""
    o = O.OracleContext(prob, opts, tables, **kw)
    starts = A.f64(starts, (prob.np, opts.N))
    v, sm, st = o.eval_batch(starts)
    install(o, opts, starts, v, sm)
    return o, dict(start=starts.copy(), value=v, pick=np.zeros(opts.N, np.int32), evaluated=opts.N)


def scatter_population(O, prob, opts, tables, M, spread=1.0, keep_init=True, **kw):
    """(oracle context at iteration 1, the call's results, the value / status tables [N][M])"""
    o = O.OracleContext(prob, opts, tables, **kw)
    N, npar, nm = opts.N, prob.np, prob.nm
    th = candidates(O, prob, opts, M, spread)
    v, sm, st = o.eval_batch(th.reshape(npar, N * M))
    v, sm, st = v.reshape(N, M), sm.reshape(nm, N, M), st.reshape(N, M)
    iv, ism, ist = o.eval_batch(prob.init[:, None])
    pick = select(v, st, iv[0], ist[0], keep_init)
    ar, pm = np.arange(N), np.maximum(pick, 0)
    start = np.where(pick < 0, prob.init[:, None], th[:, ar, pm])
    value = np.where(pick < 0, iv[0], v[ar, pm])
    simM = np.where(pick < 0, ism[:, :1], sm[:, ar, pm])
    install(o, opts, start, value, simM)
    return o, dict(start=start, value=value, pick=pick, evaluated=N * M + 1), (v, st)
