"""The proposal's tries past the first four in the persistent chain kernel on locally numbered cones (smm.jl_amd/csrc/smm_chain_persist_loc.hpp,
persist_late_tries in smm_chain_persist.hpp): the batch of tries 5-8 is drawn AHEAD, under the simulation, into LDS (PR_AHEAD batches; the
table path always staged it), and the in-kernel generator resumes at try 9 with unchanged counters — the numbers are the ones the
generator would have produced late, so every history and state equals the oracle's to the bit.
Every instance here makes late tries the rule: before anything runs on the device the test requires, from the oracle's own states and in the
form of tools/late_tries_estimate.py (tests/late_tries_ref.py), more than 1 chain expected past 4 tries per iteration — and more than 0.2
past 8 tries where the generator's resumption is what the case is about.  An instance that falls short FAILS.
Replaces mysample's rejection loop (AlgoBGP.jl:400-410) inside run!'s loop over computeNextIteration! (AlgoBGP.jl:589-640)."""
import functools
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest

import common as cm
import late_tries_ref as LT
from smm_jl_amd import _abi as A

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, NS = 60, 500
HOT = dict(sigma0=0.3)              # sigma = 0.3 .. 1.5 of the unit box: 26 of 64 chains expected past 4 tries, 15 past 8, every iteration
EDGE = dict(sigma0=0.12, seed=3)    # the smpl_iters edges: 2.5 .. 4.3 chains past 4 tries, the hard error at iterations 2, 2, 3, 10, 25


def _instance(kind, N, **kw):
    if kind == "np1":   # one parameter: general_normal's sigma (0.05 .. 0.15) scaled to 0.5 .. 1.5
        prob, opts = cm.general_normal(1, N=N, T=T, ns=NS)
        opts.sigma[:] = opts.sigma * 10.0
        return prob, opts
    return cm.serial_normal(N=N, T=T, ns=NS, **kw)


@functools.lru_cache(maxsize=None)
def _reference(kind, N, kw):
    """the oracle's run of an instance, once per session: (history fields, state fields, iterations done, error message, mean over the
    iterations of the expected number of chains past 4 / past 8 tries, every chain without a draw in the failing iteration)"""
    import smm_jl_amd as S
    from oracle import oracle as O
    O.load()
    prob, opts = _instance(kind, N, **dict(kw))
    rows, o, err, failing = LT.oracle_series(O, S, prob, opts, T)
    h, st = o.history(), o.state()
    e4 = float(np.mean([r[1][4][0] for r in rows]))
    e8 = float(np.mean([r[1][8][0] for r in rows]))
    return ({f: getattr(h, f).copy() for f in h.FIELDS}, {f: getattr(st, f).copy() for f in st.FIELDS}, st.iter, err, e4, e8, failing)


def _ref(kind, N, past8, **kw):
    ref = _reference(kind, N, tuple(sorted(kw.items())))
    e4, e8 = ref[4], ref[5]
    print("%s N=%d %s: expected chains per iteration past 4 tries %.2f, past 8 tries %.3f; the oracle's error: %s" % (kind, N, kw, e4, e8, ref[3]))
    assert e4 > 1.0, "the instance does not exercise the late tries: %.2f chains expected past 4 tries per iteration" % e4
    if past8:
        assert e8 > 0.2, "the instance does not exercise the generator's resumption: %.3f chains expected past 8 tries per iteration" % e8
    return ref


def _equal(h, st, ref, sl=slice(None)):
    for f in A.HistoryBuffers.FIELDS:
        a, b = getattr(h, f) if not isinstance(h, dict) else h[f], ref[0][f][..., sl]
        if not np.array_equal(a, b, equal_nan=True):
            bad = np.argwhere(~((a == b) | ((a != a) & (b != b))))
            raise AssertionError("history field %s: %d entries differ from the oracle's, first at %s" % (f, len(bad), bad[0].tolist()))
    for f in A.StateBuffers.FIELDS:
        a = getattr(st, f) if not isinstance(st, dict) else st[f]
        assert np.array_equal(a, ref[1][f][..., sl], equal_nan=True), "state field %s differs from the oracle's" % f


def _loc(h):
    assert h.describe()["persistent"].startswith("loc"), h.describe()


@pytest.mark.parametrize("N", [64, 100])
def test_tries_five_to_eight_from_lds_and_the_generator_from_try_nine(S, N):
    # most chains of the hot end need the batch drawn ahead, some the generator behind it, in every iteration; 100 chains: a ragged last tile
    ref = _ref("norm2", N, True, **HOT)
    prob, opts = _instance("norm2", N, **HOT)
    h = S.hip_context(prob, opts)
    _loc(h)
    for n in (1, 19, 40):
        h.step(n)
    avail, launches, repairs = h.persistent_info()
    assert launches > 0 and repairs == 0, (launches, repairs)
    assert ref[3] is None and h.state().iter == ref[2] == T
    _equal(h.history(), h.state(), ref)


def _err_fields(msg):
    m = re.search(r"no draw in support after (\d+) trials.*?chain (\d+).*?iter(?:ation)? (\d+)", msg)
    assert m, msg
    return tuple(int(x) for x in m.groups())


@pytest.mark.parametrize("smpl_iters", [4, 5, 6, 8, 9])
def test_smpl_iters_at_the_edges_of_the_batches(S, smpl_iters):
    # the last try allowed is the last of the inline batch (4), inside the batch drawn ahead (5, 6), its last (8), the generator's first (9).
    # On this instance the oracle runs into AlgoBGP.jl:409 at iterations 2, 2, 3, 10, 25: the device reports the same trials and iteration,
    # and the first of the chains the oracle finds without a draw; the iterations before it are the oracle's to the bit; and the run stands
    # where the one-launch-per-iteration kernels leave it (include/smmhip.h: the failing iteration completes for all chains, its exchange
    # is not applied)
    kw = dict(EDGE, smpl_iters=smpl_iters)
    ref = _ref("norm2", 64, smpl_iters > 8, **kw)
    prob, opts = _instance("norm2", 64, **kw)
    h = S.hip_context(prob, opts)
    _loc(h)
    c = S.hip_context(prob, opts)
    c.set_persistent(False)
    errs = []
    for ctx in (h, c):
        try:
            ctx.step(T)
            errs.append(None)
        except A.SMMHipError as e:
            errs.append(str(e))
    assert errs[0] == errs[1], errs
    assert h.persistent_info()[1] > 0 and c.persistent_info()[1] == 0
    hh, hc = h.history(), c.history()
    for f in A.HistoryBuffers.FIELDS:
        assert np.array_equal(getattr(hh, f), getattr(hc, f), equal_nan=True), f
    sh, sc = h.state(), c.state()
    for f in A.StateBuffers.FIELDS:
        assert np.array_equal(getattr(sh, f), getattr(sc, f), equal_nan=True), f
    if ref[3] is None:
        assert errs[0] is None and h.persistent_info()[2] == 0
        _equal(hh, sh, ref)
        return
    assert errs[0] is not None, "the oracle stops with '%s', the device ran through" % ref[3]
    # (the oracle's message names the LAST chain of the iteration that found no draw, the library's the first, as the reference's
    #  map(next_eval, chains) would: tests/late_tries_ref.py lists all of them from the oracle)
    trials, chain, it = _err_fields(ref[3])
    assert ref[6] and chain == max(ref[6]), (ref[3], ref[6])
    assert _err_fields(errs[0]) == (trials, min(ref[6]), it), (errs[0], ref[3], ref[6])
    assert sh.iter == it
    for f in A.HistoryBuffers.FIELDS:       # (iteration-major rows)
        a, b = getattr(hh, f), ref[0][f]
        assert np.array_equal(a[:it - 1], b[:it - 1], equal_nan=True), f


@pytest.mark.parametrize("kind,kw", [("np1", {}), ("norm2", dict(HOT, min_improve=0.5))])
def test_one_parameter_and_the_wide_form_with_and_without_the_persistent_kernel(S, kind, kw):
    ref = _ref(kind, 64, True, **kw)
    prob, opts = _instance(kind, 64, **kw)
    h = S.hip_context(prob, opts)
    _loc(h)
    c = S.hip_context(prob, opts)
    c.set_persistent(False)
    h.step(T); c.step(T)
    avail, launches, repairs = h.persistent_info()
    assert launches > 0 and repairs == 0, (launches, repairs)
    assert c.persistent_info()[1] == 0
    assert ref[3] is None
    _equal(h.history(), h.state(), ref)
    _equal(c.history(), c.state(), ref)


WORKER = r"""
import os, sys, pickle, time
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import smm_jl_amd as S, common as cm
from test_gpu_p2p import shard_opts
rank, G, N, T, ns, s0, d = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), float(sys.argv[6]), sys.argv[7]
prob, opts = cm.serial_normal(N=N, T=T, ns=ns, sigma0=s0)
c = S.hip_context(prob, shard_opts(opts, G, rank))
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
for n in (1, T // 3, T - 1 - T // 3):
    c.p2p_step(n)
c.p2p_finish(); c.sync()
h, st = c.history(), c.state()
put("result", pickle.dumps(({{f: getattr(h, f) for f in h.FIELDS}}, {{f: getattr(st, f) for f in st.FIELDS}}, c.persistent_info(), c.describe(), st.iter)))
[get("result", r) for r in range(G)]            # nobody unmaps a window a peer may still store into
"""


def test_two_shards_as_processes_on_one_device(S, tmp_path):
    # 2 x 32 chains, the ranks free running over HIP IPC windows (tests/test_gpu_p2p_persist.py): the shard form of the same template
    G, N = 2, 64
    ref = _ref("norm2", N, True, **HOT)
    script = tmp_path / "worker.py"
    script.write_text(WORKER.format(root=ROOT))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, str(script), str(r), str(G), str(N), str(T), str(NS), repr(HOT["sigma0"]), str(tmp_path)], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(G)]
    outs = [p.communicate(timeout=300)[0] for p in procs]
    for r, p in enumerate(procs):
        assert p.returncode == 0, "rank %d failed:\n%s" % (r, outs[r][-3000:])
    n = N // G
    for r in range(G):
        h, st, pinfo, desc, it = pickle.loads((tmp_path / ("result_%d" % r)).read_bytes())
        assert desc["persistent"].startswith("loc"), desc
        assert pinfo[1] > 0 and pinfo[2] == 0, "rank %d: launches of the persistent form %d, repairs %d" % (r, pinfo[1], pinfo[2])
        assert it == T
        _equal(h, st, ref, slice(r * n, (r + 1) * n))
