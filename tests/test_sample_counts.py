"""The oracle's simulation of objfunc_norm at the sample counts where the device's forms cut `ns` (tests/sample_count_ref.py: EDGES), against
a reference that does not share the contract's 512-lane shape: integer sums that are exact in any order, and math.fsum within a derived bound.
The device is held to the same helpers in tests/test_gpu_sample_counts.py; here the oracle itself is, since every other test trusts it."""
import os

import numpy as np
import pytest

import common as cm
import sample_count_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_edge_table_matches_the_headers():
    # EDGES is derived from four numbers; if a header moves one of them the table (and what the GPU rows claim to sit on) is stale
    assert R.header_constants(ROOT) == dict(WG=R.WG, ZU=R.ZU, NORM_ZU=R.NORM_ZU, PR_ZR=R.PR_ZR)
    for n in (1, 2, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4095, 4096, 4097, 6144, 6145, 8191, 8192, 8193, 12288, 12289,
              9727, 9728, 9729, 10239, 10240, 10241, 20000):
        assert n in R.EDGES, n
    assert len(set(R.EDGES)) == len(R.EDGES)
    assert R.NORM_CHUNK_EDGES == (2047, 2048, 2049, 4095, 4096, 4097, 6144, 6145)


def coded_problem(S, nm, ns):
    """np = nm parameters in [-4, 4], moments and weights that make the value depend on every simulated moment"""
    rng = np.random.default_rng(nm)
    prob = S.Problem(init=np.zeros(nm), lb=-4 * np.ones(nm), ub=4 * np.ones(nm), mom=rng.uniform(-1, 1, nm), w=rng.uniform(0.5, 2.0, nm), ns=ns)
    opts = S.BGPOpts(N=2, maxiter=2, sigma=0.05 * np.ones(2), acc_tuner=np.ones(2), min_improve=np.zeros(2), seed=3)
    return prob, opts


@pytest.mark.parametrize("nm", [1, 2, 3, 6])
def test_oracle_eval_batch_on_coded_shocks_is_the_integer_sum(S, O, nm):
    for ns in R.EDGES:
        prob, opts = coded_problem(S, nm, ns)
        th = R.dyadic_thetas(prob.lb, prob.ub, 5, seed=ns)
        v, m, st = O.OracleContext(prob, opts, S.Tables(Z=R.coded_Z(nm, ns))).eval_batch(th)
        want = R.coded_mean(nm, ns, th)
        bad = np.argwhere(m != want)
        assert bad.size == 0, "ns %d: moment %s is off by %r codes of 2^-12" % (ns, bad[0], (m - want)[tuple(bad[0])] * ns * 4096)
        assert np.all(st == 1)
        assert np.array_equal(v, R.value_from_moments(m, prob.mom, prob.w))


@pytest.mark.parametrize("ns", R.EDGES)
def test_oracle_chain_run_against_the_plain_reference(S, O, ns):
    prob, opts = cm.serial_normal(N=20, T=12, ns=ns, seed=7)
    Z = O.gen_Z(opts.seed, prob.nm, ns)
    o = O.OracleContext(prob, opts, S.Tables(Z=Z))
    o.step(12)
    h = o.history()
    worst, where = R.mean_check(Z, h.params, h.sim_moments)
    assert worst <= 1.0, "ns %d: error / bound %.3g at (iteration, moment, chain) %s" % (ns, worst, where)
    ok = h.status == 1
    assert ok.any()
    assert np.array_equal(h.value[ok], R.value_from_moments(h.sim_moments, prob.mom, prob.w)[ok])


def test_the_bound_leaves_a_wrong_sum_no_room():
    # what the reference must notice: the smallest draw of a row dropped, at the count where it weighs least
    ns = max(R.EDGES)
    Z = np.random.default_rng(1).standard_normal((1, ns))
    x = Z[0] + 0.3
    drop = np.abs(x).min() / ns
    assert drop > 100 * R.mean_bound(Z[0], 0.3, ns)
    assert abs(float(np.sum(x)) / ns - R.exact_mean(Z[0], 0.3)) <= R.mean_bound(Z[0], 0.3, ns)    # numpy's pairwise sum: another order of the same depth


@pytest.mark.parametrize("nm", [1, 2, 3, 5, 6])
@pytest.mark.parametrize("ns", [1, 513, 4097])
def test_oracle_noseed_evaluations_equal_eval_batch_on_generated_shocks(S, O, nm, ns):
    # smm_oracle.c: "bit-identical to a cached Z" — one Philox block gives the shocks of moments 2q and 2q + 1, an odd nm drops half a block
    prob, opts = coded_problem(S, nm, ns)
    th = np.random.default_rng(ns + nm).uniform(prob.lb[:, None], prob.ub[:, None], (nm, 4))
    base = 1000 + 17 * nm
    v, m, st = O.OracleContext(prob, opts).eval_batch_noseed(th, base)
    for i in range(th.shape[1]):
        Z = O.gen_Z(base + i, nm, ns)
        vi, mi, si = O.OracleContext(prob, opts, S.Tables(Z=Z)).eval_batch(th[:, i:i + 1])
        assert np.array_equal(m[:, i], mi[:, 0]) and v[i] == vi[0] and st[i] == si[0] == 1, (nm, ns, i)
        worst, where = R.mean_check(Z, th[:, i:i + 1], m[:, i:i + 1])
        assert worst <= 1.0, (worst, where)
