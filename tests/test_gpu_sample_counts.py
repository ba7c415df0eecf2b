"""Every hand-written form of objfunc_norm's simulation at the sample counts where it cuts `ns` into pieces (tests/sample_count_ref.py: EDGES
— chunk edges of 2048 and 4096 draws, an even and an odd number of chunks, a ragged last chunk, the persistent `loc` forms' FULL template
at 9728 .. 10239 and their limit at 10240, fewer draws than a wave or a tile has lanes).  Each row asserts the form that runs (describe()),
then holds it to
  1. the oracle, history and state, to the bit;
  2. a reference that does not share the contract's 512-lane shape: every simulated moment within mean_bound of math.fsum's mean;
  3. the objective recomputed from the returned moments, to the bit;
  4. the other form that serves the same problem (persistent against per-iteration, shards against the single shard), to the bit.
eval_batch runs on shocks whose sum is exact in any order, so that a lost, doubled or misplaced draw changes an integer.

Forms that are not the ones a reader might expect from the parameter count, as the dispatch (smmhip.hip: select_forms) decides them:
four parameters take the norm kernel (`iter_norm`, np <= 4), so the general kernel's np = 4 rows go through the seam SMMHIP_NORM_FAST=0;
past ns = 10240 the one- and two-parameter problems take the persistent tile kernel (`tile_sim`) instead of `loc` / `loc_wide`."""
import types

import numpy as np
import pytest

import common as cm
import sample_count_ref as R
from smm_jl_amd import _abi as A
from test_sample_counts import coded_problem

pytestmark = pytest.mark.gpu

STEPS = {17: [1, 4, 7], 48: [2, 13, 5]}      # a partly filled 16-chain tile, 12 iterations; three tiles, 20 iterations
N48_AT = (513, 9728)                         # the three-tile rows (the one-tile rows cover every edge; the plain reference's fsum is what costs)
RATIOS = {}                                  # form -> largest error / bound seen (printed with -s by the last test)


def rows(edges):
    return [(17, ns) for ns in edges] + [(48, ns) for ns in edges if ns in N48_AT]


def problem(npar, N, ns, mi=0.0):
    T = sum(STEPS[N])
    if npar == 2:
        return cm.serial_normal(N=N, T=T, ns=ns, seed=7, min_improve=mi)
    prob, opts = cm.general_normal(npar, N=N, T=T, ns=ns)
    opts.min_improve[:] = mi
    return prob, opts


def plain_checks(form, prob, Z, h):
    """checks 2 and 3 on a history"""
    worst, where = R.mean_check(Z, h.params, h.sim_moments)
    RATIOS[form] = max(RATIOS.get(form, 0.0), worst)
    print("%s np %d N %d ns %d: error / bound %.3f" % (form, prob.np, h.value.shape[1], prob.ns, worst))
    assert worst <= 1.0, "error / bound %.3g at (iteration, moment, chain) %s" % (worst, where)
    ok = h.status == 1
    assert ok.any()
    assert np.array_equal(h.value[ok], R.value_from_moments(h.sim_moments, prob.mom, prob.w)[ok])


def run(S, O, prob, opts, steps, chain=None, persistent=None, plain=True):
    """one device context against the oracle and the plain reference (checks 1 to 3); persistent=None: the per-iteration kernels.
    plain=False: the caller holds this run to the bits of one that passed checks 2 and 3 (same()), which is the same statement"""
    h = S.hip_context(prob, opts)
    if persistent is None:
        h.set_persistent(False)
    d = h.describe()
    if chain is not None:
        assert d["chain"] == chain, d
    if persistent is not None:
        assert d["persistent"] == persistent, d
    Z = h.Z()
    assert np.array_equal(Z, O.gen_Z(opts.seed, prob.nm, prob.ns))
    o = O.OracleContext(prob, opts, S.Tables(Z=Z))
    for n in steps:
        h.step(n); o.step(n)
    avail, launches, repairs = h.persistent_info()
    if persistent is None or persistent == "none":
        assert launches == 0
    else:
        assert launches >= 1 and repairs == 0, (launches, repairs)
    hh, st = h.history(), h.state()
    cm.assert_history_equal(hh, o.history(), exact_floats=True)
    cm.assert_state_equal(st, o.state(), rtol=0)
    if plain:
        plain_checks(persistent or d["chain"], prob, Z, hh)
    return hh, st


def same(a, b):
    cm.assert_history_equal(a[0], b[0], exact_floats=True)
    cm.assert_state_equal(a[1], b[1], rtol=0)


# ---- evaluations ----
@pytest.mark.parametrize("nm", [1, 2, 3, 6])
@pytest.mark.parametrize("ns", R.EDGES)
def test_eval_batch_on_coded_shocks_is_the_integer_sum(S, O, ns, nm):
    prob, opts = coded_problem(S, nm, ns)
    tab = S.Tables(Z=R.coded_Z(nm, ns))
    h, o = S.hip_context(prob, opts, tab), O.OracleContext(prob, opts, tab)
    for M in (1, 16, 17):
        th = R.dyadic_thetas(prob.lb, prob.ub, M, seed=ns + M)
        v, m, st = h.eval_batch(th)
        want = R.coded_mean(nm, ns, th)
        bad = np.argwhere(m != want)
        assert bad.size == 0, "batch of %d: moment %s is off by %r codes of 2^-12" % (M, bad[0], (m - want)[tuple(bad[0])] * ns * 4096)
        assert np.all(st == 1)
        assert np.array_equal(v, R.value_from_moments(m, prob.mom, prob.w))
        vo, mo, so = o.eval_batch(th)
        assert np.array_equal(v, vo) and np.array_equal(m, mo) and np.array_equal(st, so)


@pytest.mark.parametrize("nm", [1, 2, 3, 6])
@pytest.mark.parametrize("ns", [1, 2, 63, 65, 513, 2049, 4096, 4097, 8193, 9728, 10241, 20000])
def test_eval_batch_noseed_draws_the_oracles_shocks(S, O, ns, nm):
    # one Philox block gives the shocks of moments 2q and 2q + 1: an odd nm drops half a block
    prob, opts = coded_problem(S, nm, ns)
    h, o = S.hip_context(prob, opts), O.OracleContext(prob, opts)
    th = np.random.default_rng(ns + nm).uniform(prob.lb[:, None], prob.ub[:, None], (nm, 17))
    base = 5000 + ns
    v, m, st = h.eval_batch_noseed(th, base)
    vo, mo, so = o.eval_batch_noseed(th, base)
    assert np.array_equal(m, mo) and np.array_equal(v, vo) and np.array_equal(st, so)
    for i in (0, 16):
        worst, where = R.mean_check(O.gen_Z(base + i, nm, ns), th[:, i:i + 1], m[:, i:i + 1])
        RATIOS["eval_batch_noseed"] = max(RATIOS.get("eval_batch_noseed", 0.0), worst)
        assert worst <= 1.0, (worst, where)
    assert np.array_equal(v, R.value_from_moments(m, prob.mom, prob.w))


# ---- the per-iteration kernels ----
@pytest.mark.parametrize("npar", [1, 2])
@pytest.mark.parametrize("N,ns", rows(R.EDGES))
def test_norm_kernel_per_iteration(S, O, N, ns, npar):
    run(S, O, *problem(npar, N, ns), STEPS[N], chain="iter_norm")


@pytest.mark.parametrize("npar", [1, 2])
@pytest.mark.parametrize("N,ns", rows(R.NORM_CHUNK_EDGES))
def test_narrow_norm_kernel_at_its_chunk_edges(S, O, hooks, monkeypatch, N, ns, npar):
    monkeypatch.setenv("SMMHIP_NORM_NARROW", "1")
    narrow = run(S, O, *problem(npar, N, ns), STEPS[N], chain="iter_norm_narrow")
    monkeypatch.delenv("SMMHIP_NORM_NARROW")
    same(narrow, run(S, O, *problem(npar, N, ns), STEPS[N], chain="iter_norm", plain=False))


@pytest.mark.parametrize("N,ns", rows(R.EDGES))
def test_general_kernel_with_six_parameters(S, O, N, ns):
    run(S, O, *problem(6, N, ns), STEPS[N], chain="iter<sim,8>")


@pytest.mark.parametrize("N,ns", rows(R.EDGES))
def test_general_kernel_with_four_parameters(S, O, hooks, monkeypatch, N, ns):
    # four parameters are the norm kernel's (smmhip.hip: F.norm_fast, np <= 4): the general kernel through the seam, then the kernel they really take
    monkeypatch.setenv("SMMHIP_NORM_FAST", "0")
    general = run(S, O, *problem(4, N, ns), STEPS[N], chain="iter<sim,8>")
    monkeypatch.delenv("SMMHIP_NORM_FAST")
    same(general, run(S, O, *problem(4, N, ns), STEPS[N], chain="iter_norm", plain=False))


# ---- the persistent kernels ----
@pytest.mark.parametrize("npar", [1, 2])
@pytest.mark.parametrize("mi,form,chain", [(0.0, "loc", "iter_norm"), (0.05, "loc_wide", "iter_norm_wide")])
@pytest.mark.parametrize("N,ns", rows(R.EDGES))
def test_persistent_kernel_on_local_cones(S, O, N, ns, mi, form, chain, npar):
    if ns > R.LOC_MAX:
        form = "tile_sim"       # the draws no longer fit the lanes' registers: the form is refused, the tile kernel takes the problem
    prob, opts = problem(npar, N, ns, mi)
    pers = run(S, O, prob, opts, STEPS[N], persistent=form)
    same(pers, run(S, O, prob, opts, STEPS[N], chain=chain, plain=False))
    if N > 2:
        assert (pers[0].exchanged != 0).any()


@pytest.mark.parametrize("npar,chain", [(3, "iter_norm"), (6, "iter<sim,8>")])
@pytest.mark.parametrize("N,ns", rows(R.EDGES))
def test_persistent_tile_kernel(S, O, N, ns, npar, chain):
    prob, opts = problem(npar, N, ns)
    pers = run(S, O, prob, opts, STEPS[N], persistent="tile_sim")
    same(pers, run(S, O, prob, opts, STEPS[N], chain=chain, plain=False))


@pytest.mark.parametrize("ns", [63, 513, 9728, 10239, 10240])
def test_two_shards_in_the_persistent_form(S, O, tmp_path, ns):
    from test_gpu_p2p import shard_opts
    from test_gpu_p2p_persist import _run
    G, N, T = 2, 64, 12
    prob, opts = cm.serial_normal(N=N, T=T, ns=ns)      # (the launcher's problem)
    assert S.hip_context(prob, shard_opts(opts, G, G - 1)).describe()["persistent"] == "loc_shard"
    res = _run(tmp_path, G, N, T, ns, 0.0, "plain")
    for r, (h, st, pinfo, err, it) in enumerate(res):
        assert err is None, err
        assert pinfo[1] >= 1 and pinfo[2] == 0, (r, pinfo)
    hist = types.SimpleNamespace(**{f: np.concatenate([res[r][0][f] for r in range(G)], axis=-1) for f in A.HistoryBuffers.FIELDS})
    single = S.hip_context(prob, opts)
    single.step(T)
    Z = single.Z()
    o = O.OracleContext(prob, opts, S.Tables(Z=Z))
    o.step(T)
    cm.assert_history_equal(hist, o.history(), exact_floats=True)
    cm.assert_history_equal(hist, single.history(), exact_floats=True)
    ss, so = single.state(), o.state()
    for f in A.StateBuffers.FIELDS:
        both = np.concatenate([res[r][1][f] for r in range(G)], axis=-1)
        assert np.array_equal(both, getattr(ss, f), equal_nan=True) and np.array_equal(both, getattr(so, f), equal_nan=True), f
    plain_checks("loc_shard", prob, Z, hist)


@pytest.mark.parametrize("ns", [100, 9728, 10240])
def test_timestamp_mode_keeps_the_bits(S, O, monkeypatch, ns):
    # SMMHIP_TS=1 (read when a context is created) puts per-wave stamps inside persist_simulate and grows the kernel's LDS
    prob, opts = problem(2, 17, ns)
    plain = run(S, O, prob, opts, STEPS[17], persistent="loc")
    monkeypatch.setenv("SMMHIP_TS", "1")
    same(plain, run(S, O, prob, opts, STEPS[17], persistent="loc", plain=False))


def test_report_the_largest_error_by_form():
    for form, r in sorted(RATIOS.items()):
        print("largest error / bound, %-18s %.3f" % (form, r))
        assert r <= 1.0
