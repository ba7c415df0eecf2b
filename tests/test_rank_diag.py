"""tests/rank_diag_ref.py, the restatement of smm_get_rank_diag's contract (include/smmhip.h) the GPU tests hold the device against, held
against brute force (the ranks), statistics.NormalDist (ndtri) and theory (independent normal chains; a shifted and a scaled chain); the
tolerance of the outputs behind ndtri measured on the GPU tests' shapes; the Python argument checks, which raise without a device; and
the ctypes and Julia mirrors of smm_rank_diag_t against the header.  No GPU."""
import math
import os
import statistics

import numpy as np
import pytest

import chain_diag_ref as D
import rank_diag_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute(x):
    x = np.asarray(x, float)
    return np.array([2 * int(np.sum(x < v)) + int(np.sum(x == v)) + 1 for v in x], np.int64)


def test_ranks_equal_a_brute_force_count():
    rng = np.random.default_rng(1)
    cols = [rng.standard_normal(37), rng.integers(0, 3, 64).astype(float), np.zeros(9), np.array([0.0, -0.0, 1.0, -0.0, -1.0, 0.0]),
            np.repeat(rng.standard_normal(5), 7), np.array([2.5])]
    for x in cols:
        r = R.rank2(x)
        assert r.dtype == np.int64 and np.array_equal(r, brute(x)), x
        assert r.sum() == len(x) * (len(x) + 1)            # twice the sum of the average ranks
    r = R.rank2([0.0, -0.0, 1.0])
    assert r[0] == r[1] == 3                                # -0.0 and +0.0 are equal


@pytest.mark.parametrize("n,groups", [(17, [0, 0, 0, 1, -1]), (9, [0, 1, 1, 1, 1]), (8, [2, 2, 0, 0, 0])])
def test_pooled_ranks_of_groups_with_ties_a_single_member_and_an_odd_window(n, groups):
    rng = np.random.default_rng(n)
    X = rng.integers(-2, 3, (2, 5, n)).astype(float)       # heavy ties, zeros of both signs
    X[X == 0] *= rng.choice([1.0, -1.0], (X == 0).sum())
    g = np.asarray(groups)
    h, nb = n // 2, 5
    out = R.rank_diag_from_series(X, h - 1, nb, g)
    for gi in range(g.max() + 1):
        mem = np.flatnonzero(g == gi)
        if len(mem) == 0:                                   # a group without members: undefined
            assert (out["status"][:, gi] == 2).all() and np.isnan(out["rhat_rank"][gi]).all()
            continue
        for s in range(2):
            pooled = np.concatenate([X[s, c, lo:lo + h] for c in mem for lo in (0, n - h)])
            r2 = brute(pooled)
            M = len(pooled)
            want = np.zeros((nb, len(mem)), np.int64)
            for i, v in enumerate(r2):
                want[((int(v) - 1) * nb) // (2 * M), i // (2 * h)] += 1
            assert np.array_equal(out["rank_hist"][:, s, mem], want)
    assert (out["rank_hist"][:, :, g < 0] == 0).all()
    assert (out["rank_hist"].sum(axis=0)[:, g >= 0] == 2 * h).all()


def test_ndtri_is_the_standard_librarys_to_the_last_bit_or_one_ulp():
    inv = statistics.NormalDist().inv_cdf
    for M in (16, 256, 1200, 9600):
        for r2 in list(range(2, 2 * M + 1, max(1, M // 300))) + [2 * M]:
            p = R.rank_prob(r2, M)
            a, b = R.ndtri(p), inv(p)
            assert abs(a - b) <= math.ulp(b), (M, r2, a, b)
    assert R.ndtri(0.5) == 0.0 and R.ndtri(0.975) == pytest.approx(1.959963984540054, abs=1e-15)


def test_independent_normal_chains_a_shifted_and_a_scaled_chain():
    rng = np.random.default_rng(11)
    m, h = 8, 500
    Y = rng.standard_normal((m, h))
    c, _ = R.cell(Y, h - 1)
    assert abs(c["rhat_rank"] - 1) < 0.01 and abs(c["rhat_bulk"] - 1) < 0.01 and abs(c["rhat_folded"] - 1) < 0.01
    assert abs(c["ess_bulk"] / (m * h) - 1) < 0.2 and c["status"] == (0, 0, 0, 0)
    assert c["ess_tail"] > 0.5 * m * h and abs(c["ess_mean"] / (m * h) - 1) < 0.2
    shifted = Y.copy()
    shifted[0] += 2.0
    assert R.cell(shifted, h - 1)[0]["rhat_bulk"] > 1.1
    scaled = Y.copy()
    scaled[0] *= 3.0
    cs, _ = R.cell(scaled, h - 1)
    mu, var = [D.S(y) / h for y in scaled], None
    var = [D.S((y - a) * (y - a)) / (h - 1) for y, a in zip(scaled, mu)]
    assert cs["rhat_folded"] > 1.05 and cs["rhat_rank"] == cs["rhat_folded"] and D.rhat_group(mu, var, h) < 1.01


def metropolis(rng, N, T, step, thin=4):
    """[N][T] random-walk Metropolis chains on N(0, 1), every thin-th state: a state series with ties, as the library's"""
    x = rng.standard_normal(N)
    out = np.empty((N, T * thin))
    for t in range(T * thin):
        prop = x + step * rng.standard_normal(N)
        acc = np.log(rng.random(N)) < 0.5 * (x * x - prop * prop)
        x = np.where(acc, prop, x)
        out[:, t] = x
    return out[:, ::thin]


def gpu_shapes():
    """the GPU tests' shapes with synthetic series [S][N][n]: (series, max_lag, groups)"""
    rng = np.random.default_rng(2021)
    small = np.stack([metropolis(rng, R.N_SMALL, R.T_SMALL, 2.4) for _ in range(3)])
    large = np.stack([metropolis(rng, R.N_LARGE, R.T_LARGE, 2.4) for _ in range(3)])
    cases = [(small[:, :, t0:t1], (t1 - t0) // 2 - 1, R.GROUPS_SMALL) for t0, t1 in R.WINDOWS_SMALL]
    return cases + [(large, R.T_LARGE // 2 - 1, R.GROUPS_LARGE)]


def test_the_tolerance_is_eight_times_the_effect_of_a_one_ulp_logarithm():
    up = lambda x: math.nextafter(math.log(x), math.inf)
    down = lambda x: math.nextafter(math.log(x), -math.inf)
    worst, left_out, ok = 0.0, [], []
    for X, ml, g in gpu_shapes():
        base = R.rank_diag_from_series(X, ml, 4, g)
        left_out.append(R.near_sign_change(base))
        ok.append(base["status"][0] == 0)
        for log in (up, down):
            moved = R.rank_diag_from_series(X, ml, 4, g, log=log)
            for f in R.EXACT:
                assert np.array_equal(moved[f], base[f], equal_nan=True), f     # (no logarithm behind these)
            for f in R.TOLERANCED:
                a, b = moved[f], base[f]
                assert np.array_equal(np.isnan(a), np.isnan(b)), f
                fin = ~np.isnan(b)
                worst = max(worst, float(np.max(np.abs(a[fin] - b[fin]) / np.abs(b[fin]))))
    print("largest relative change: %.3g; RANK_LOG_CHANGE = %.3g, RANK_RTOL = %.3g" % (worst, R.RANK_LOG_CHANGE, R.RANK_RTOL))
    assert 0 < worst <= R.RANK_LOG_CHANGE and R.RANK_RTOL == 8 * R.RANK_LOG_CHANGE
    assert R.RANK_LOG_CHANGE <= 4 * worst                   # (the constant is the measurement, rounded up: no slack beyond that)
    assert np.mean(np.concatenate([v.ravel() for v in left_out])) <= 0.05
    assert np.mean(np.concatenate([v.ravel() for v in ok])) >= 0.9


def test_the_gpu_tests_populations_mix(O):
    """the histories the GPU tests compute, here from the CPU oracle: at least 90 % of the cells of the small and the large shape have
    status 0, at most 5 % are left out of the toleranced comparison, and max_lag = 2 comes first everywhere (status 1 occurs)"""
    import common as cm

    def history(kw):
        prob, opts = cm.serial_normal(**kw)
        o = O.OracleContext(prob, opts)
        o.step(kw["T"])
        return o.history(0, kw["T"])

    hs, hl = history(R.SMALL_KW), history(R.LARGE_KW)
    with np.errstate(invalid="ignore", divide="ignore"):
        cells = [R.rank_diag_from_history(hs, t0, t1, None, 0, R.GROUPS_SMALL) for t0, t1 in R.WINDOWS_SMALL]
        cells.append(R.rank_diag_from_history(hl, 0, R.T_LARGE, None, 0, R.GROUPS_LARGE))
        short = [R.rank_diag_from_history(hs, t0, t1, 2, 0, R.GROUPS_SMALL) for t0, t1 in R.WINDOWS_SMALL]
    print("status 0:", [(c["status"] == 0).all(axis=0).tolist() for c in cells], "ties:", 1 - hs.accepted.mean(), 1 - hl.accepted.mean())
    assert R.share_of_cells_with_status_0(cells) >= 0.9
    for c in cells + short:
        assert R.near_sign_change(c).mean() <= 0.05
    for c in short:
        assert np.isin(c["status"][[0, 2, 3]], (1, 2)).all() and (c["status"] == 1).any()
    assert 0.1 < 1 - hs.accepted.mean() < 0.3 and 0.5 < 1 - hl.accepted.mean() < 0.8       # (the series are tied as the library's are)


def test_python_argument_checks_raise_without_a_device():
    from smm_jl_amd.backend import BGPContext
    c = object.__new__(BGPContext)
    c.N, c.np, c._ctx = 16, 2, None
    g = np.zeros(16, np.int32)
    for kw in (dict(t0=5, t1=12), dict(t0=0, t1=20, max_lag=0), dict(t0=0, t1=20, max_lag=10), dict(t0=0, t1=20, n_bins=-1),
               dict(t0=0, t1=20, groups=np.zeros(15)), dict(t0=0, t1=20, groups=np.full(16, -1)), dict(t0=0, t1=20, groups=g, n_groups=0)):
        with pytest.raises(ValueError):
            c.rank_diag(**kw)
    import smm_jl_amd as S
    for name in ("rhat_rank", "ess_bulk", "ess_tail", "rank_plot"):
        assert callable(getattr(S, name)) and name in S.__all__


def test_the_mirrors_of_smm_rank_diag_t():
    from test_julia_layer import header_structs, julia_structs
    from smm_jl_amd import _abi as A
    js = julia_structs(os.path.join(ROOT, "julia", "SMMHip.jl"))
    want = header_structs()["smm_rank_diag_t"]
    ptr = {"Cdouble": "double*", "Int32": "int32_t*", "Int64": "int64_t*"}
    assert [(f, ptr[t[4:-1]]) for f, t in js["SmmRankDiag"]] == [(f, t) for f, t in want]
    assert [f for f, _ in A.smm_rank_diag_t._fields_] == [f for f, _ in want]
    argtypes = dict((n, a) for n, _, a in A.SYMBOLS)["smm_get_rank_diag"]
    assert len(argtypes) == 8 and argtypes[-1]._type_ is A.smm_rank_diag_t
