"""A SHARD of the objectives a whole tile evaluates in the persistent form (smm.jl_amd/csrc/smm_chain_persist_tile.hpp, SH = true;
include/smmhip.h: smm_bgp_p2p_step): objfunc_norm with more than two parameters, the dense objective (v1 and BASELINE config 5's
SMM_OBJ_DENSE2) and a map-reduce user objective.  The ring lives in every rank's p2p window; a tile publishes its chains' whole records
into its own window and their values and parameters into every peer's, fetches the rest of an exchanged chain's donor record from the
donor's owner, and the ranks' launches meet in a start barrier.  No multi-GPU node is available to this build: the ranks are PROCESSES
on the one GPU, their windows mapped through HIP IPC (all tiles co-resident), free running; every shard's whole history and state must
equal the single shard's slice to the bit, and the single shard's the oracle's where that is affordable.
Replaces the pmap branch of computeNextIteration! (AlgoBGP.jl:596-605) + exchangeMoves! (:647-691) + swap_ev_ij! (:734-749)."""
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest

import common as cm
from smm_jl_amd import _abi as A

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_problem(S, kind, Ng, T, mi=0.0):
    """(prob, opts of the whole population) of one of this file's cases — built the same way in the workers and in the test"""
    if kind == "c5":   # BASELINE config 5 as bench.py builds it: dense2, np = nm = 50
        from smm_jl_amd.workloads import build_problem
        prob, opts = build_problem("c5", Ng, Ng, 0, T, 0)
    elif kind in ("dense2", "dense2_error"):
        from test_dense2 import dense2_problem
        prob, opts = dense2_problem(50, 50, N=Ng, T=T, **({"smpl_iters": 2} if kind == "dense2_error" else {}))
        # (0.02 x temps(N, 4) fails at 256 chains within 40 iterations; 0.02 x 1 .. 2 with two trials: no draw in support after 2 trials
        # (AlgoBGP.jl:409) in the middle of a launch — iteration 15 at 256 chains)
        opts.sigma[:] = (0.02 if kind == "dense2_error" else 0.01) * np.linspace(1.0, 2.0, Ng)
    elif kind == "dense":
        from test_gpu_parity import dense_problem
        prob, opts = dense_problem(None, None, 6, 5, N=Ng, T=T)
    elif kind == "norm6":
        prob, opts = cm.general_normal(6, N=Ng, T=T, ns=300)
    elif kind == "user":
        from user_objective_src import PANEL_SOURCE
        from test_user_objective import panel_problem
        prob, opts = panel_problem(S, S.register_user_objective(PANEL_SOURCE, n_sums=3, lanes=64), N=Ng, T=T, fail_above=0.6)
    elif kind == "user_rng":
        from user_rng_src import PANEL_RNG_SOURCE
        from test_user_rng import panel_problem
        prob, opts = panel_problem(S, S.register_user_objective(PANEL_RNG_SOURCE, n_sums=3, lanes=64, rng=True), N=Ng, T=T)
    else:
        raise ValueError(kind)
    opts.min_improve[:] = mi
    return prob, opts


def steps_of(mode, T):
    return [1, 7, 2, 1, T - 11] if mode == "chunks" else [1, T // 3, T - 1 - T // 3]


WORKER = r"""
import os, sys, pickle, time
import numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import smm_jl_amd as S, common as cm
from smm_jl_amd import _abi as A
if os.environ.get("SMM_TEST_BUILD") == "hooks":
    S._abi.use_test_hooks(True)
from test_gpu_p2p import shard_opts
from test_gpu_p2p_persist_tile import make_problem, steps_of
rank, G, Ng, T, d, kind, mi, mode = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5], sys.argv[6], float(sys.argv[7]), sys.argv[8]
prob, opts = make_problem(S, kind, Ng, T, mi)
c = S.hip_context(prob, shard_opts(opts, G, rank))
form = c.describe()["persistent"]
handle, _ = c.p2p_init()
def put(tag, data=b""):
    open(os.path.join(d, "%s_%d.tmp" % (tag, rank)), "wb").write(data); os.rename(os.path.join(d, "%s_%d.tmp" % (tag, rank)), os.path.join(d, "%s_%d" % (tag, rank)))
def get(tag, r):
    p = os.path.join(d, "%s_%d" % (tag, r)); t0 = time.time()
    while not os.path.exists(p):
        time.sleep(0.002)
        if time.time() - t0 > 120: raise SystemExit("rank %d: no %s from rank %d" % (rank, tag, r))
    return open(p, "rb").read()
put("handle", handle)
for r in range(G):
    if r != rank: c.p2p_attach(r, handle=get("handle", r))
put("mapped"); [get("mapped", r) for r in range(G)]
err, t_nan, dt = None, None, None
try:
    for k, n in enumerate(steps_of(mode, T)):     # free running: kernels of different processes wait for each other on the device
        c.p2p_step(n)
        if mode == "chunks" and k == 2:
            c.p2p_finish(); c.sync(); put("mid"); [get("mid", r) for r in range(G)]     # a read-back in the middle (the ranks meet)
            assert c.history().value.shape[0] == 10
        if mode == "nanstate" and k == 1:
            # an uploaded state with a NaN value in ONE shard: the flag smm_set_state derives from it is that rank's own
            c.p2p_finish(); c.sync(); put("mid"); [get("mid", r) for r in range(G)]
            st0, h0 = c.state(), c.history()
            if rank == G - 1:
                st0.la_value[3] = np.nan
            c.set_state(st0, h0)
            put("up"); [get("up", r) for r in range(G)]
            t_nan = time.time()
    c.p2p_finish(); c.sync()
except A.SMMHipError as e:
    err = str(e)
if t_nan is not None:
    dt = time.time() - t_nan
h, st = c.history(), c.state()
put("result", pickle.dumps(({{f: getattr(h, f) for f in h.FIELDS}}, {{f: getattr(st, f) for f in st.FIELDS}}, c.persistent_info(), err, st.iter, form, dt)))
[get("result", r) for r in range(G)]            # nobody unmaps a window a peer may still store into
"""


def _run(tmp_path, G, Ng, T, kind, mi=0.0, mode="plain", env_extra=None, env_rank=None):
    """env_extra: for every rank; env_rank: {rank: environment of that rank alone}"""
    script = tmp_path / "worker.py"
    script.write_text(WORKER.format(root=ROOT))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.update(env_extra or {})
    envs = [dict(env, **(env_rank or {}).get(r, {})) for r in range(G)]
    procs = [subprocess.Popen([sys.executable, str(script), str(r), str(G), str(Ng), str(T), str(tmp_path), kind, repr(float(mi)), mode], env=envs[r],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(G)]
    outs = [p.communicate(timeout=300)[0] for p in procs]
    for r, p in enumerate(procs):
        assert p.returncode == 0, "rank %d failed:\n%s" % (r, outs[r][-3000:])
    return [pickle.loads((tmp_path / ("result_%d" % r)).read_bytes()) for r in range(G)]


def _single(S, kind, Ng, T, mi, steps, nan_at=None):
    prob, opts = make_problem(S, kind, Ng, T, mi)
    single = S.hip_context(prob, opts)
    for k, n in enumerate(steps):
        single.step(n)
        if nan_at is not None and k == 1:   # the same uploaded state as the shards' (worker: mode nanstate)
            st0, h0 = single.state(), single.history()
            st0.la_value[nan_at] = np.nan
            single.set_state(st0, h0)
    return prob, opts, single


def _check(S, res, G, Ng, T, kind, mi=0.0, mode="plain", form=None, oracle=None, repairs=0):
    prob, opts, single = _single(S, kind, Ng, T, mi, steps_of(mode, T), nan_at=(Ng - Ng // G + 3) if mode == "nanstate" else None)
    hs, ss = single.history(), single.state()
    n = Ng // G
    for r in range(G):
        h, st, pinfo, err, it, f, dt = res[r]
        assert err is None, err
        if form is not None:
            assert f == form, (r, f)
        assert pinfo[1] >= 1 and (pinfo[2] == 0 if repairs == 0 else pinfo[2] >= repairs), "rank %d: launches of the persistent form %d, repairs %d" % (r, pinfo[1], pinfo[2])
        for fld in A.HistoryBuffers.FIELDS:
            a, b = h[fld], getattr(hs, fld)[..., r * n:(r + 1) * n]
            if not np.array_equal(a, b, equal_nan=True):
                bad = np.argwhere(~((a == b) | ((a != a) & (b != b))))
                raise AssertionError("history field %s of rank %d: %d entries differ, first at %s" % (fld, r, len(bad), bad[0].tolist()))
        for fld in A.StateBuffers.FIELDS:
            assert np.array_equal(st[fld], getattr(ss, fld)[..., r * n:(r + 1) * n], equal_nan=True), (fld, r)
    if mi == 0.0:
        assert (hs.exchanged != 0).any()
    if oracle is not None:
        o = oracle.OracleContext(prob, opts, S.Tables(Z=single.Z()), threads=oracle.max_threads())
        o.step(T)
        cm.assert_history_equal(hs, o.history())
        cm.assert_state_equal(ss, o.state())


def _form(S, kind, G, Ng, mi=0.0, edit=None):
    from test_gpu_p2p import shard_opts
    prob, opts = make_problem(S, kind, Ng, 8, mi)
    if edit is not None:
        edit(opts)
    return S.hip_context(prob, shard_opts(opts, G, 0)).describe()["persistent"]


def test_the_shards_of_tile_objectives_take_the_persistent_form(S):
    for G, Ng in ((2, 4096), (4, 4096), (8, 4096)):
        assert _form(S, "c5", G, Ng) == "tile_dense2_shard", (G, Ng)
    assert _form(S, "norm6", 2, 128) == "tile_sim_shard"
    assert _form(S, "dense", 2, 128) == "tile_dense_shard"
    assert _form(S, "user", 2, 128) == "tile_user_shard"
    # the per-iteration forms stay where the shard form does not apply
    assert _form(S, "norm6", 2, 128, mi=-1.0) == "none"                                            # a negative threshold

    def by_chain(o):
        o.min_improve[:] = np.linspace(0.0, 0.1, len(o.min_improve))
    assert _form(S, "norm6", 2, 128, edit=by_chain) == "none"                                      # thresholds by chain
    assert _form(S, "dense2", 2, 2000) == "none"                                                   # 1000 chains per rank: not whole tiles
    assert _form(S, "dense2", 2, 16384) == "none"                                                  # N_global past 8192: the big plan


@pytest.mark.parametrize("G", [2, 4])
def test_c5_objective_as_a_sharded_run(S, tmp_path, G):
    # BASELINE config 5's population of 4096 chains, dense2 with np = nm = 50, split over 2 and 4 ranks
    Ng, T = 4096, 60
    res = _run(tmp_path, G, Ng, T, "c5")
    _check(S, res, G, Ng, T, "c5", form="tile_dense2_shard")


@pytest.mark.parametrize("kind,mi,form", [("dense2", 0.0, "tile_dense2_shard"), ("norm6", 0.05, "tile_sim_shard"), ("dense", 0.0, "tile_dense_shard")])
def test_small_shards_against_the_oracle(S, O, tmp_path, kind, mi, form):
    G, Ng, T = 2, 256, 40
    res = _run(tmp_path, G, Ng, T, kind, mi)
    _check(S, res, G, Ng, T, kind, mi, form=form, oracle=O)


@pytest.mark.parametrize("kind", ["user", "user_rng"])
def test_map_reduce_user_objective_as_shards(S, tmp_path, kind):
    G, Ng, T = 2, 128, 30
    res = _run(tmp_path, G, Ng, T, kind)
    _check(S, res, G, Ng, T, kind, form="tile_user_shard")


def test_read_backs_in_the_middle_of_a_sharded_run(S, tmp_path):
    G, Ng, T = 2, 256, 40
    res = _run(tmp_path, G, Ng, T, "dense2", mode="chunks")
    _check(S, res, G, Ng, T, "dense2", mode="chunks")


@pytest.mark.parametrize("kind,Ng,slow_rank,slow_read", [("dense2", 256, 0, False), ("dense2", 256, 1, False), ("c5", 4096, 1, False), ("c5", 4096, 1, True)])
def test_skew_and_a_short_ring(S, tmp_path, kind, Ng, slow_rank, slow_read):
    # one tile of ONE rank idles before each publication and the ring holds 2 iterations: the overrun guard (progress words of all ranks'
    # tiles in every window, announced once the donors' records from the owners have landed) must keep the OTHER rank back — its tiles
    # take the minimum over every rank's words, not their own rank's.  An overrun would end in a tag that never comes: a time-out, a repair
    # (at 2 x 2048 a tile's cone reaches a few of the 256 tiles: the ranks are coupled through their gathers far less than at 2 x 128.
    # slow_read: the slow tile idles while it still has to read its donors' granules out of the OTHER rank's windows — before the progress word
    # that releases the slot; idling before the publication, as the other cases do, comes after every read of the ring's entry)
    G, T = 2, 40
    slow = dict(SMMHIP_PR_SLOW_TILE="3", SMMHIP_PR_SLOW_US="100" if slow_read else "30", **({"SMMHIP_PR_SLOW_READ": "1"} if slow_read else {}))
    res = _run(tmp_path, G, Ng, T, kind, env_extra=dict(SMM_TEST_BUILD="hooks", SMMHIP_PR_RING="2"), env_rank={slow_rank: slow})
    _check(S, res, G, Ng, T, kind)


def test_hard_error_is_replayed_on_every_rank_to_the_same_iteration(S, tmp_path):
    # AlgoBGP.jl:409 (no draw in support after smpl_iters trials) inside a launch of the shard form: the ranks agree on the error word,
    # roll back and replay up to and including the failing iteration on the per-iteration forms
    G, Ng, T = 2, 256, 30
    res = _run(tmp_path, G, Ng, T, "dense2_error")
    prob, opts = make_problem(S, "dense2_error", Ng, T)
    single = S.hip_context(prob, opts)
    with pytest.raises(A.SMMHipError) as ei:
        for n in steps_of("plain", T):
            single.step(n)
    msg = str(ei.value)
    assert "no draw in support" in msg
    hs = single.history()
    n = Ng // G
    its = set()
    for r in range(G):
        h, st, pinfo, err, it, f, dt = res[r]
        assert f == "tile_dense2_shard", f
        assert err == msg, (err, msg)
        assert pinfo[1] >= 1 and pinfo[2] >= 1, pinfo            # the persistent form ran, and was replayed
        its.add(it)
        for fld in A.HistoryBuffers.FIELDS:
            assert np.array_equal(h[fld], getattr(hs, fld)[..., r * n:(r + 1) * n], equal_nan=True), (fld, r)
    assert its == {single.state().iter}, its
    assert single.state().iter > 2                               # (inside a launch, not its first one-iteration step)


def test_a_nan_in_one_shards_uploaded_state_reaches_every_rank_together(S, tmp_path):
    # smm_set_state's NaN flag is the shard's own, so it does not decide the form: every rank launches the shard form, the launch of the
    # rank holding the NaN reports it (kind 3) at its first iteration, the ranks agree on the word at their rendezvous and replay the
    # step on the per-iteration forms — every rank once, promptly (no start barrier's or rendezvous' time-out), with the single shard's results
    G, Ng, T = 2, 256, 30
    res = _run(tmp_path, G, Ng, T, "dense2", mode="nanstate")
    for r in range(G):
        assert res[r][5] == "tile_dense2_shard", res[r][5]
        assert res[r][6] < 15.0, res[r][6]
        assert res[r][2][2] == res[0][2][2], [x[2] for x in res]          # (the ranks replayed together)
    _check(S, res, G, Ng, T, "dense2", mode="nanstate", repairs=1)
