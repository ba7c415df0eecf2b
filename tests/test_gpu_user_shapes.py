"""User objectives at the shapes real models have: the generic objective (user_objective_src.GENERIC_*) across parameter, moment and
partial-sum counts and lane widths, through every device path a row reaches — the stand-alone kernel of eval_batch, the three launches per
iteration (k_chain_iter<0, CT> proposing, the user's kernel, the accept launch; CT = 64 or 8 by the tile's LDS), and the persistent kernels
compiled with the user's source inside (gen_user: k_chain_persist_gen; tile_user: k_chain_persist_tile).  Every row asserts the forms it was
given (describe: persistent, ct), then compares the device with the oracle (the gcc build of the same text) and, at dyadic theta, with the
numpy restatement — to the bit — and a persistent run with its twin on the three launches, to the bit."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import common as cm  # noqa: E402
from user_objective_src import (GENERIC_LANES_RNG_SOURCE, GENERIC_LANES_SOURCE, GENERIC_RNG_SOURCE, GENERIC_SOURCE,  # noqa: E402
                                dyadic_thetas, generic_moments, generic_numpy)
from user_rng_src import Shim  # noqa: E402

pytestmark = pytest.mark.gpu

FAIL_ABOVE = 0.125   # an evaluation fails (status -2, NaN last moment) where its last parameter lies above this
_reg = {}


def register(S, O, source, n_sums=None, lanes=256, rng=False, seed=None):
    """one device registration and one host build per (source, form) and process; the oracle's hook is set again at every use (another
    test may have hooked the same handle meanwhile; an RNG objective's stream is keyed by the context's seed)"""
    key = (source, n_sums, lanes)
    if key not in _reg:
        oid = S.register_user_objective(source, n_sums=n_sums, lanes=lanes, rng=rng)
        host = Shim(O, source, n_sums=n_sums) if rng else C.CDLL(O.register_user_objective(source, oid, n_sums=n_sums, lanes=lanes))
        _reg[key] = (oid, host)
    oid, host = _reg[key]
    if rng:
        host.hook(O, oid, seed, lanes=lanes)
    else:
        O.hook_user_objective(host, oid, n_sums, lanes)
    return oid, host


@contextlib.contextmanager
def fresh_registrations():
    """registrations made inside are kept apart from the process's: for callers that make another library current (the test build has a
    registry of its own, and a handle of one registry means nothing to the other)"""
    global _reg
    saved, _reg = _reg, {}
    try:
        yield
    finally:
        _reg = saved


def problem(S, oid, np_, nm, sums, A, N, T, seed=17, mi=0.0, batch_size=None, chol=None):
    rng = np.random.default_rng(np_ * 1000 + nm)
    init = rng.integers(-256, 257, np_) / 1024.0
    init[-1] = 0.0
    mom, w = generic_moments(nm)
    prob = S.Problem(init=init, lb=-np.ones(np_), ub=np.ones(np_), mom=mom, w=w, ns=1, objective_id=oid,
                     obj_params=[float(A), FAIL_ABOVE, float(sums)])
    opts = S.BGPOpts(N=N, maxiter=T, sigma=0.05 * min(1.0, np.sqrt(4.0 / np_)) * cm.temps(N, 4.0), acc_tuner=np.geomspace(3.0, 0.5, N), min_improve=np.broadcast_to(mi, (N,)),
                     seed=seed, N_global=N, batch_size=batch_size, chol_L=chol)
    return prob, opts


# (id, form, np, nm, n_sums, lanes, N, steps, A, persistent, ct, extra)  — form: "one" (SMM_USER_OBJECTIVE, its sums from udata) or "mr"
# (SMM_USER_PARTIAL / SMM_USER_FINISH, n_sums = SMM_NSUMS); A units, a multiple of no lane count.
# ct: k_chain_iter<0, 64> where tile_smem_doubles(64, ...) fits in 60 KB — one-thread form up to np = nm = 4 (55.2 KB), 5 x 5 is 63.7 KB;
# the map-reduce form's layout (kind 4) adds a partial-sum block.  tile_user wants persist_tile_smem <= 160 KiB: its wave totals are
# 16 chains x lanes / 64 x n_sums doubles (64 KiB at 64 sums and 512 lanes) — 48 x 48 parameters and moments take 148.4 KiB, 64 x 64 166.9.
ROWS = [
    ("one 1x1: gen_user, ct 64",                 "one", 1, 1, 2, None, 64, [1, 9, 6], 37, "gen_user", 64, {}),
    ("one 3x3: gen_user, ct 64",                 "one", 3, 3, 4, None, 32, [1, 9, 6], 37, "gen_user", 64, {}),
    ("one 4x4: gen_user, the last ct 64",        "one", 4, 4, 3, None, 32, [1, 9, 6], 37, "gen_user", 64, {}),
    ("one 5x5: gen_user, the first ct 8",        "one", 5, 5, 7, None, 32, [1, 9, 6], 37, "gen_user", 8, {}),
    ("one 6x6: gen_user, ct 8",                  "one", 6, 6, 5, None, 64, [1, 9, 6], 37, "gen_user", 8, {}),
    ("one 16x16: gen_user at PG_MAXP",           "one", 16, 16, 16, None, 64, [1, 9, 6], 37, "gen_user", 8, {}),
    ("one 17x16: past PG_MAXP",                  "one", 17, 16, 3, None, 32, [1, 9, 6], 37, "none", 8, {}),
    ("one 16x17: past PG_MAXP",                  "one", 16, 17, 20, None, 32, [1, 9, 6], 37, "none", 8, {}),
    ("one 18x18, batch_size 6",                  "one", 18, 18, 18, None, 32, [1, 9, 6], 37, "none", 8, {"batch_size": 6}),
    ("one 64x64, 44 chains: MAX_DIM",            "one", 64, 64, 64, None, 44, [1, 9, 6], 37, "none", 8, {}),
    ("one 64x1",                                 "one", 64, 1, 17, None, 32, [1, 9, 6], 37, "none", 8, {}),
    ("one 1x64",                                 "one", 1, 64, 7, None, 32, [1, 9, 6], 37, "none", 8, {}),
    ("one 18x18, shared chol_L",                 "one", 18, 18, 9, None, 32, [1, 9, 6], 37, "none", 8, {"chol": True}),
    ("one 18x18, per-chain min_improve",         "one", 18, 18, 18, None, 32, [1, 9, 6], 37, "none", 8, {"mi": "per_chain"}),
    ("mr 1x1x1, 64 lanes: tile_user",            "mr", 1, 1, 1, 64, 40, [1, 9, 6], 1500, "tile_user", 64, {}),
    ("mr 18x3x17, 128 lanes: tile_user",         "mr", 18, 3, 17, 128, 40, [1, 9, 6], 1500, "tile_user", 8, {}),
    ("mr 6x50x3, 256 lanes: tile_user",          "mr", 6, 50, 3, 256, 40, [1, 9, 6], 1500, "tile_user", 8, {}),
    ("mr 48x48x64, 512 lanes: spilling tile_user", "mr", 48, 48, 64, 512, 24, [1, 6, 5], 1500, "tile_user", 8, {}),
    ("mr 64x64x64, 512 lanes: past 160 KiB",     "mr", 64, 64, 64, 512, 24, [1, 6, 5], 1500, "none", 8, {}),
    ("mr 64x64x64, 1024 lanes: spilling",        "mr", 64, 64, 64, 1024, 24, [1, 6, 5], 1500, "none", 8, {}),
]


def chol_factor(np_):
    L = np.eye(np_)
    L[np.arange(1, np_), np.arange(np_ - 1)] = 0.25
    return L


def make(S, O, row, rng=False):
    what, form, np_, nm, n_sums, lanes, N, steps, A, pers, ct, extra = row
    src = {("one", False): GENERIC_SOURCE, ("mr", False): GENERIC_LANES_SOURCE, ("one", True): GENERIC_RNG_SOURCE,
           ("mr", True): GENERIC_LANES_RNG_SOURCE}[(form, rng)]
    seed = 17
    oid, host = register(S, O, src, n_sums=n_sums if form == "mr" else None, lanes=lanes or 256, rng=rng, seed=seed)
    mi = np.linspace(0.0, 0.5, N) if extra.get("mi") == "per_chain" else 0.0
    prob, opts = problem(S, oid, np_, nm, n_sums, A, N, sum(steps), seed=seed, mi=mi, batch_size=extra.get("batch_size"),
                         chol=chol_factor(np_) if extra.get("chol") else None)
    return prob, opts, host


def check_premise(h, row):
    d = h.describe()
    assert (d["persistent"], d["ct"]) == (row[9], str(row[10])), (row[0], d)
    assert h.persistent_info()[0] is (row[9] != "none"), (row[0], d)


def check_eval_batch(h, o, prob, row, restate=True):
    np_, n_sums = row[2], row[4]
    th = dyadic_thetas(np_, 50, seed=np_ * 7 + prob.nm, last_above=FAIL_ABOVE)
    got = h.eval_batch(th)
    want = o.eval_batch(th)
    for a, b in zip(got, want):
        assert np.array_equal(a, b, equal_nan=True), row[0]
    if restate:
        for a, b in zip(got, generic_numpy(th, prob.mom, prob.w, prob.obj_params, n_sums)):
            assert np.array_equal(a, b, equal_nan=True), row[0]
    assert (got[2] == -2).any() and (got[2] == 1).any()


def check_run(S, O, h, prob, opts, row):
    steps, pers = row[7], row[9]
    o = O.OracleContext(prob, opts, threads=O.max_threads())
    c = None
    if pers != "none":
        c = S.hip_context(prob, opts)
        c.set_persistent(False)
    for n in steps:
        h.step(n); o.step(n)
        if c is not None:
            c.step(n)
    hh = h.history()
    cm.assert_history_equal(hh, o.history(), exact_floats=True)
    cm.assert_state_equal(h.state(), o.state(), rtol=0)
    if c is not None:
        avail, launches, repairs = h.persistent_info()
        assert launches >= 1 and repairs == 0, (row[0], launches, repairs)
        assert c.persistent_info()[1] == 0
        cm.assert_history_equal(hh, c.history(), exact_floats=True)
        cm.assert_state_equal(h.state(), c.state(), rtol=0)
    assert hh.accepted[1:].any() and (hh.exchanged != 0).any() and (hh.status == -2).any(), row[0]
    assert np.isnan(hh.sim_moments[..., -1, :][hh.status == -2]).all()
    return hh


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_user_objective_shape(S, O, row):
    prob, opts, _ = make(S, O, row)
    h = S.hip_context(prob, opts)
    check_premise(h, row)
    check_eval_batch(h, O.OracleContext(prob, opts), prob, row)
    check_run(S, O, h, prob, opts, row)


RNG_ROWS = [
    ("rng one 18x18",                    "one", 18, 18, 18, None, 32, [1, 9, 6], 37, "none", 8, {}),
    ("rng mr 18x40x40, 256 lanes",       "mr", 18, 40, 40, 256, 40, [1, 9, 6], 700, "tile_user", 8, {}),
]


@pytest.mark.parametrize("row", RNG_ROWS, ids=[r[0] for r in RNG_ROWS])
def test_rng_user_objective_shape(S, O, row):
    from test_user_rng import oracle_noseed
    prob, opts, shim = make(S, O, row, rng=True)
    h = S.hip_context(prob, opts)
    check_premise(h, row)
    check_eval_batch(h, O.OracleContext(prob, opts), prob, row, restate=False)
    th = dyadic_thetas(row[2], 12, seed=3, last_above=FAIL_ABOVE)
    base = 2 ** 33 + 5
    got = h.eval_batch_noseed(th, base)
    for a, b in zip(got, oracle_noseed(O, shim, prob, opts, th, base)):
        assert np.array_equal(a, b, equal_nan=True)
    assert len({tuple(got[1][:-1, i]) for i in range(12)}) == 12
    check_run(S, O, h, prob, opts, row)


def test_two_shards_of_a_wide_user_objective(S, O):
    from test_gpu_parity import sharded_run_fused
    from smm_jl_amd import _abi as A
    row = ("shards one 18x18", "one", 18, 18, 11, None, 32, [20], 37, "none", 8, {})
    prob, opts, _ = make(S, O, row)
    single = S.hip_context(prob, opts)
    check_premise(single, row)
    single.step(20)
    o = O.OracleContext(prob, opts, threads=O.max_threads())
    o.step(20)
    hs = single.history()
    cm.assert_history_equal(hs, o.history(), exact_floats=True)
    ctxs = sharded_run_fused(S, prob, opts, 2, 20)
    for r, c in enumerate(ctxs):
        hr = c.history()
        for f in A.HistoryBuffers.FIELDS:
            assert np.array_equal(getattr(hr, f), getattr(hs, f)[..., r * 16:(r + 1) * 16], equal_nan=True), (f, r)
    assert (hs.exchanged != 0).any() and (hs.status == -2).any() and hs.accepted[1:].any()
