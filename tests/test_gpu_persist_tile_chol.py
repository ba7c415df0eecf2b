"""Cholesky (adapted) proposals in the persistent tile kernel (smm.jl_amd/csrc/smm_chain_persist_tile.hpp, its CH form) and in the
per-iteration kernel's cooperative proposal (coop_mysample<CT, true>, smm_propose.hpp): x = mu01 + sigma_c (L z), the sum of
include/smmhip.h — products rounded, added left to right.  Every case runs three contexts — the persistent one, its twin with
set_persistent(False) on the per-iteration kernels, the oracle — and compares histories and states to the bit.  The tries of mysample
(AlgoBGP.jl:400-410), their order and the winner are the serial loop's; a factor installed between two steps (smm_set_proposal,
smm_adapt_proposal) is the next launch's."""
import re

import numpy as np
import pytest

import common as cm
from smm_jl_amd import _abi as A
from test_gpu_parity import _random_chol, dense_problem
from test_gpu_proposal import eye_factors

pytestmark = pytest.mark.gpu

NP_MAX_TILE = 60   # objfunc_norm with np = nm: the tile form's LDS is 158.3 KiB at 60 parameters, 160.4 at 61 (MAX_DIM = 64 is not the bound)


def factors(npar, N, per_chain, seed=5, scale=1.0):
    rng = np.random.default_rng(seed)
    L = np.stack([_random_chol(rng, npar, scale) for _ in range(N)]) if per_chain else _random_chol(rng, npar, scale)
    return np.ascontiguousarray(L)


def same(a, b):
    cm.assert_history_equal(a.history(), b.history(), exact_floats=True)
    cm.assert_state_equal(a.state(), b.state(), rtol=0)


def oracle_tables(S, h, tab):
    t = tab if tab is not None else S.Tables()
    return S.Tables(probs_acc=t.probs_acc, prop_normals=t.prop_normals, pairs=t.pairs, Z=h.Z())


def three(S, O, prob, opts, tab=None, expect=None):
    """(persistent context, per-iteration context, oracle)"""
    h = S.hip_context(prob, opts, tab)
    c = S.hip_context(prob, opts, tab)
    c.set_persistent(False)
    if expect is not None:
        assert h.describe()["persistent"] == expect, h.describe()
    return h, c, O.OracleContext(prob, opts, oracle_tables(S, h, tab), threads=O.max_threads())


def check(h, c, o, persistent=True):
    same(h, c); same(h, o); same(c, o)
    avail, launches, repairs = h.persistent_info()
    if persistent:
        assert launches >= 1 and repairs == 0, (launches, repairs, h.describe())
    else:
        assert launches == 0, (launches, h.describe())
    assert c.persistent_info()[1] == 0


def run(S, O, prob, opts, steps, tab=None, expect=None, persistent=True):
    h, c, o = three(S, O, prob, opts, tab, expect)
    for n in steps:
        for x in (h, c, o):
            x.step(n)
    check(h, c, o, persistent)
    return h, c, o


def error_of(ctx, T):
    """(iteration, chain) of the no-draw error that ends ctx's run"""
    with pytest.raises(A.SMMHipError) as e:
        ctx.step(T)
    assert e.value.code == A.SMM_ERR_NO_DRAW_IN_SUPPORT, str(e.value)
    m = re.search(r"chain (\d+),? iter(?:ation)? (\d+)", str(e.value))
    return int(m.group(2)), int(m.group(1))


# ---- 1. the forms ----

def user_row(chol, np_=18, nm=3, sums=17, lanes=128, N=40, form="mr", pers="tile_user"):
    return ("chol", form, np_, nm, sums, lanes, N, [1, 9, 6], 1500 if form == "mr" else 37, pers, 8, {"chol": True} if chol else {})


def test_forms_with_and_without_a_factor(S, O):
    from test_dense2 import dense2_problem
    from test_gpu_p2p import shard_opts
    from test_gpu_user_shapes import make
    prob, opts = cm.general_normal(6, N=32, T=8, ns=64)
    opts.chol_L = factors(6, 32, True)
    assert S.hip_context(prob, opts).describe()["persistent"] == "tile_sim"
    prob, opts = dense_problem(S, O, 50, 50, N=48, T=8)
    opts.chol_L = factors(50, 48, True)
    assert S.hip_context(prob, opts).describe()["persistent"] == "tile_dense"
    prob, opts = dense2_problem(50, 50, N=16, T=8)
    opts.chol_L = factors(50, 16, False)
    assert S.hip_context(prob, opts).describe()["persistent"] == "tile_dense2"
    prob, opts, _ = make(S, O, user_row(True))
    assert opts.chol_L is not None and opts.chol_L.ndim == 2
    assert S.hip_context(prob, opts).describe()["persistent"] == "tile_user"
    # out of scope: a shard, a one-thread user objective past PG_MAXP
    prob, opts = cm.general_normal(6, N=64, T=8, ns=64)
    opts.chol_L = factors(6, 64, True)
    assert S.hip_context(prob, shard_opts(opts, 2, 1)).describe()["persistent"] == "none"
    prob, opts, _ = make(S, O, user_row(True, 18, 18, 9, None, 32, "one", "none"))
    assert S.hip_context(prob, opts).describe()["persistent"] == "none"
    # the largest objfunc_norm the tile form holds, with and without a factor (no LDS of the factor's own)
    for npar, form in ((NP_MAX_TILE, "tile_sim"), (NP_MAX_TILE + 1, "none")):
        prob, opts = cm.general_normal(npar, N=16, T=8, ns=64)
        assert S.hip_context(prob, opts).describe()["persistent"] == form
        opts.chol_L = factors(npar, 16, False)
        assert S.hip_context(prob, opts).describe()["persistent"] == form
    # without a factor: the forms the existing tile tests pin at their LDS edges
    prob, opts, _ = make(S, O, user_row(False, 48, 48, 64, 512, 24))
    d = S.hip_context(prob, opts).describe()
    assert (d["chain"], d["persistent"], d["ct"]) == ("user_lanes_3launches", "tile_user", "8"), d
    prob, opts = dense_problem(S, O, 56, 60, N=16, T=8)
    d = S.hip_context(prob, opts).describe()
    assert (d["chain"], d["persistent"]) == ("iter<dense,16>", "tile_dense"), d
    opts.chol_L = factors(56, 16, True)
    assert S.hip_context(prob, opts).describe()["persistent"] == "tile_dense"


# ---- 2. objfunc_norm, bit-exact ----

@pytest.mark.parametrize("npar,N", [(3, 24), (6, 2), (18, 70), (33, 16), (50, 33), (NP_MAX_TILE, 16)])
@pytest.mark.parametrize("per_chain", [False, True])
@pytest.mark.parametrize("mi", [0.0, 0.5])
def test_objfunc_norm_with_a_factor(S, O, npar, N, per_chain, mi):
    steps = [1, 5, 2, 12]
    prob, opts = cm.general_normal(npar, N=N, T=sum(steps), ns=100)
    opts.chol_L = factors(npar, N, per_chain)
    opts.sigma[:] = 0.05 * min(1.0, np.sqrt(6.0 / npar)) * cm.temps(N, 3.0)
    opts.min_improve[:] = mi
    opts.smpl_iters = 100000
    h, c, o = run(S, O, prob, opts, steps, expect="tile_sim")
    if N > 2 and mi == 0.0:
        assert (h.history().exchanged != 0).any()


def test_two_parameters_with_a_factor(S, O):
    """(with a factor the objfunc_norm fast path is off, so one and two parameters reach the tile form too: one pair, one lane of 32 at work)"""
    steps = [1, 5, 2, 12]
    prob, opts = cm.general_normal(2, N=24, T=sum(steps), ns=100)
    opts.chol_L = factors(2, 24, True)
    opts.sigma[:] = 0.05 * cm.temps(24, 3.0)
    opts.smpl_iters = 100000
    h, c, o = run(S, O, prob, opts, steps, expect="tile_sim")
    assert (h.history().exchanged != 0).any()


@pytest.mark.parametrize("kind", ["sim", "dense"])
def test_thresholds_by_chain_with_a_factor(S, O, kind):
    """(min_improve by chain: the PCT instantiations of the CH form)"""
    steps = [1, 5, 2, 12]
    if kind == "sim":
        npar, N = 18, 40
        prob, opts = cm.general_normal(npar, N=N, T=sum(steps), ns=100)
        opts.sigma[:] = 0.05 * np.sqrt(6.0 / npar) * cm.temps(N, 3.0)
    else:
        npar, N = 17, 32
        prob, opts = dense_problem(S, O, npar, 33, N=N, T=sum(steps), smpl_iters=100000)
    opts.chol_L = factors(npar, N, True)
    opts.min_improve[:] = np.linspace(0.0, 0.5, N)
    opts.smpl_iters = 100000
    h, c, o = run(S, O, prob, opts, steps, expect="tile_" + kind)
    assert (h.history().exchanged != 0).any()


# ---- 3. every phase of mysample ----

def late_problem(smpl_iters, T=8):
    npar, N = 18, 24   # (more than 8 parameters: two tries are preloaded, rb_tries)
    prob, opts = cm.general_normal(npar, N=N, T=T, ns=64)
    opts.chol_L = factors(npar, N, True, seed=11)
    opts.sigma[:] = 0.2
    opts.smpl_iters = smpl_iters
    return prob, opts


SHARED_ROUNDS_TRIES = 2 + 2 * 16   # the preloaded tries and SMM_SCOUT_AFTER = 2 rounds of at most 16 tries of one chain


def late_premise(S, O, Z):
    """(the oracle alone) with as many tries as the preloaded ones, or as the shared rounds cover, the run ends without a draw — the
    real run, with 100000, needs the tries behind them"""
    for si in (2, SHARED_ROUNDS_TRIES):
        prob, opts = late_problem(si)
        it, chain = error_of(O.OracleContext(prob, opts, S.Tables(Z=Z)), opts.maxiter)
        assert 2 <= it <= opts.maxiter


@pytest.mark.parametrize("scout_after", [None, "0", "1000000"])
def test_late_tries_of_mysample(S, O, request, monkeypatch, scout_after):
    # (the Cholesky form has no scouting phase and does not read scout_after: the two runs with the hook show that the hook changes nothing,
    # they cover no second schedule.  The per-iteration twin runs the same form where its history row holds the staged normals.)
    if scout_after is not None:
        request.getfixturevalue("hooks")
        monkeypatch.setenv("SMMHIP_SCOUT_AFTER", scout_after)
    prob, opts = late_problem(100000)
    h, c, o = run(S, O, prob, opts, [opts.maxiter], expect="tile_sim")
    late_premise(S, O, h.Z())


def injected(prob, opts, K, inside):
    """tables with K tries per iteration: the first K - 1 far outside the box, the last one inside (or not)"""
    tab = cm.random_tables(prob, opts, tries=K)
    tab.prop_normals[:, :K - 1] = 1e9
    tab.prop_normals[:, K - 1] *= 0.01 if inside else 1.0
    return tab


def test_injected_normals_the_last_try_wins(S, O):
    K, T = 5, 12
    prob, opts = cm.general_normal(18, N=40, T=T, ns=64)
    opts.chol_L = factors(18, 40, True)
    tab = injected(prob, opts, K, True)
    h, c, o = run(S, O, prob, opts, [T], tab=tab, expect="tile_sim")
    # the winner is the injected try K - 1: the proposals of iteration 2 by the contract's sum, from the initial value every chain
    # accepted in iteration 1 (for the chains the exchanges of iterations 1 and 2 left alone: swap_ev_ij! rewrites the row)
    hh = h.history()
    lb, ub = prob.lb, prob.ub
    alone = np.flatnonzero((hh.exchanged[0] == 0) & (hh.exchanged[1] == 0))
    assert alone.size >= 4
    for ch in alone:
        z, L = tab.prop_normals[1, K - 1, :, ch], opts.chol_L[ch]
        m01 = (hh.params[0, :, ch] - lb) / (ub - lb)
        want = np.empty(18)
        for k in range(18):
            y = L[k, 0] * z[0]
            for j in range(1, k + 1):
                y = y + L[k, j] * z[j]
            want[k] = (m01[k] + opts.sigma[ch] * y) * (ub[k] - lb[k]) + lb[k]
        assert np.array_equal(hh.params[1, :, ch], want), ch


@pytest.mark.parametrize("last", [22, 40])
def test_injected_normals_no_try_inside(S, O, last):
    K, T, tf = 4, 14, 9
    prob, opts = cm.general_normal(18, N=40, T=T, ns=64)
    opts.chol_L = factors(18, 40, False)
    tab = injected(prob, opts, K, True)
    tab.prop_normals[tf - 1, K - 1, :, 21:last] = 1e9   # iteration tf: chains 22 .. last have no try inside
    h, c, o = three(S, O, prob, opts, tab, expect="tile_sim")
    h.step(1); c.step(1)
    # one failing chain: the oracle names it.  Several: the oracle goes through all the chains of the iteration (on several threads) and
    # names one of the failing ones, whichever wrote its message last; the device names the lowest
    it, chain = error_of(o, T)
    assert it == tf and 22 <= chain <= last
    want = (tf, 22)
    assert error_of(h, T - 1) == want and error_of(c, T - 1) == want
    assert h.persistent_info()[1] >= 1 and h.persistent_info()[2] >= 1   # (the launch ran on; the step was replayed)
    same(h, c)
    assert h.state().iter == tf == o.state().iter + 1   # (the device completes the failing iteration for all chains)
    ho, hh = o.history(0, T), h.history(0, T)
    for f in cm.INT_FIELDS + cm.F64_FIELDS:
        assert np.array_equal(getattr(hh, f)[:tf - 1], getattr(ho, f)[:tf - 1], equal_nan=True), f


# ---- 4. dense and user objectives ----

@pytest.mark.parametrize("npar,nm,N,per_chain", [(50, 50, 48, True), (17, 33, 32, False)])
def test_dense_with_a_factor(S, O, npar, nm, N, per_chain):
    prob, opts = dense_problem(S, O, npar, nm, N=N, T=20, smpl_iters=100000)
    opts.chol_L = factors(npar, N, per_chain)
    h, c, o = run(S, O, prob, opts, [1, 5, 2, 12], expect="tile_dense")
    assert (h.history().exchanged != 0).any() and h.history().accepted[1:].any()


def test_dense2_with_a_factor(S, O):
    from test_dense2 import dense2_problem
    prob, opts = dense2_problem(50, 50, N=16, T=20, smpl_iters=100000)   # (whole tiles: 16 chains is the smallest population)
    opts.chol_L = factors(50, 16, True)
    run(S, O, prob, opts, [1, 5, 2, 12], expect="tile_dense2")


@pytest.mark.parametrize("rng", [False, True])
def test_user_objective_with_a_factor(S, O, rng):
    from test_gpu_user_shapes import check_premise, check_run, make
    row = user_row(True)
    prob, opts, _ = make(S, O, row, rng=rng)
    h = S.hip_context(prob, opts)
    check_premise(h, row)
    check_run(S, O, h, prob, opts, row)   # (the three contexts, to the bit; launches >= 1, repairs == 0, the twin's launches == 0)


def test_user_objective_with_dense_factors_by_chain(S, O):
    """(the module built for a factor with full triangles, one per chain: the rows above have a shared identity with one subdiagonal)"""
    from test_gpu_user_shapes import make
    row = user_row(True)
    prob, opts, _ = make(S, O, row)
    opts.chol_L = factors(18, 40, True, scale=0.5)
    h = S.hip_context(prob, opts)
    c = S.hip_context(prob, opts)
    c.set_persistent(False)
    o = O.OracleContext(prob, opts, threads=O.max_threads())
    assert h.describe()["persistent"] == "tile_user", h.describe()
    for n in row[7]:
        for x in (h, c, o):
            x.step(n)
    check(h, c, o)
    assert h.history().accepted[1:].any() and (h.history().exchanged != 0).any()


# ---- 5. a factor installed between two steps ----

def test_adapt_then_continue_in_the_same_loop(S, O):
    N, npar, T1, T2 = 32, 6, 60, 40
    prob, opts = cm.general_normal(npar, N=N, T=T1 + T2, ns=100)
    opts.chol_L = eye_factors(N, npar)
    opts.smpl_iters = 100000
    h, c, o1 = three(S, O, prob, opts, expect="tile_sim")
    for x in (h, c, o1):
        x.step(T1)
    check(h, c, o1)
    before = h.persistent_info()[1]
    st = h.adapt_proposal(0, T1, accepted_only=False)
    assert np.array_equal(st, c.adapt_proposal(0, T1, accepted_only=False)) and (st == 0).any()
    L = h.proposal()
    assert np.array_equal(L, c.proposal()) and not np.array_equal(L, eye_factors(N, npar))
    # the oracle goes on from the same state with the factor read back
    opts.chol_L = np.ascontiguousarray(L)
    o = O.OracleContext(prob, opts, S.Tables(Z=h.Z()), threads=O.max_threads())
    o.set_state(o1.state(), o1.history())
    for x in (h, c, o):
        x.step(T2)
    check(h, c, o)
    assert h.persistent_info()[1] > before


def test_set_proposal_between_steps_and_restart(S, O):
    N, npar, T1, T2 = 40, 18, 12, 14
    prob, opts = cm.general_normal(npar, N=N, T=T1 + T2, ns=100)
    opts.chol_L = eye_factors(N, npar)
    opts.sigma *= 0.5
    opts.smpl_iters = 100000
    h, c, o1 = three(S, O, prob, opts, expect="tile_sim")
    for x in (h, c, o1):
        x.step(T1)
    check(h, c, o1)
    L = factors(npar, N, True, seed=9)
    h.set_proposal(L); c.set_proposal(L)
    opts.chol_L = L
    o = O.OracleContext(prob, opts, S.Tables(Z=h.Z()), threads=O.max_threads())
    o.set_state(o1.state(), o1.history())
    # a restart through get_state / set_state with the factor installed
    r = S.hip_context(prob, opts)
    r.set_state(h.state(), h.history())
    for x in (h, c, o, r):
        x.step(T2)
    check(h, c, o)
    assert r.persistent_info()[1] >= 1 and r.persistent_info()[2] == 0
    same(r, o)


# ---- 6. L = I is the isotropic kernel ----

@pytest.mark.parametrize("npar", [5, 4])
def test_identity_factor_equals_the_isotropic_form(S, npar):
    prob, opts = cm.general_normal(npar, N=30, T=30, ns=100)
    a = S.hip_context(prob, opts)
    opts.chol_L = np.eye(npar)
    b = S.hip_context(prob, opts)
    # (four parameters without a factor run k_chain_iter_norm between the launches, with a factor the general kernel: the persistent form is the same)
    assert a.describe()["persistent"] == b.describe()["persistent"] == "tile_sim", (a.describe(), b.describe())
    a.step(30); b.step(30)
    for x in (a, b):
        assert x.persistent_info()[1] >= 1 and x.persistent_info()[2] == 0
    ha, hb = a.history(), b.history()
    for f in cm.INT_FIELDS + cm.F64_FIELDS:
        assert np.array_equal(getattr(ha, f), getattr(hb, f), equal_nan=True), f


# ---- 7. the per-iteration kernel's cooperative proposal ----

@pytest.mark.parametrize("what", ["negative threshold", "dist_fun", "np 18", "np 50"])
def test_per_iteration_kernels_with_a_factor(S, O, what):
    npar, N, T = (50, 33, 12) if what == "np 50" else (18, 40, 16)
    kw = {"dist_fun": A.SMM_DIST_ABSDIFF} if what == "dist_fun" else {}
    prob, opts = cm.general_normal(npar, N=N, T=T, ns=100, **kw)
    opts.chol_L = factors(npar, N, True)
    opts.sigma[:] = 0.05 * min(1.0, np.sqrt(6.0 / npar)) * cm.temps(N, 3.0)
    opts.smpl_iters = 100000
    if what == "negative threshold":
        opts.min_improve[:] = -0.01
    per_iteration = what in ("negative threshold", "dist_fun")
    h, c, o = run(S, O, prob, opts, [1, T - 1], expect="none" if per_iteration else "tile_sim", persistent=not per_iteration)
    assert (h.history().exchanged != 0).any()


def test_two_shards_with_a_factor(S, O):
    from test_gpu_parity import sharded_run_fused
    npar, Ng, T = 18, 64, 12
    prob, opts = cm.general_normal(npar, N=Ng, T=T, ns=100)
    opts.chol_L = factors(npar, Ng, True)
    opts.sigma[:] = 0.03 * cm.temps(Ng, 3.0)
    opts.smpl_iters = 100000
    ctxs = sharded_run_fused(S, prob, opts, 2, T)
    o = O.OracleContext(prob, opts, S.Tables(Z=ctxs[0].Z()), threads=O.max_threads())
    o.step(T)
    ho = o.history()
    for r, c in enumerate(ctxs):
        assert c.describe()["persistent"] == "none" and c.persistent_info()[1] == 0
        hr = c.history()
        for f in A.HistoryBuffers.FIELDS:
            assert np.array_equal(getattr(hr, f), getattr(ho, f)[..., r * 32:(r + 1) * 32], equal_nan=True), (f, r)
    assert (ho.exchanged != 0).any()
