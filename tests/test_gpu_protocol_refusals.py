"""What the stepping entry points refuse, and in which words (smm.jl_amd/csrc/smm_run_host.hpp): the three-phase, values,
two-enqueue and p2p calls in the states in which they must not be made.  Every case makes calls that are refused on the host before
any launch, plus the few one-iteration steps that reach the state; each asserts the return code and the text smm_last_error gives.
The table is what the library answered before these rules were written once each: it pins codes, texts and the order of checks."""
import ctypes as C

import pytest

import common as cm
from smm_jl_amd import _abi as A
from test_gpu_p2p import shard_opts

pytestmark = pytest.mark.gpu

INVALID, STATE, MAXITER = A.SMM_ERR_INVALID_ARG, A.SMM_ERR_STATE, A.SMM_ERR_MAXITER

GATHER = "records are in the gather buffer: call smm_bgp_sharded_finish first"
WINDOWS = "the records of the last iteration are in the p2p windows: call smm_bgp_p2p_finish first"
INIT_FIRST = "smm_bgp_p2p_init comes first"
BEFORE_FIRST = "exchange before the first local step"
RESOLVED = "exchange already resolved for this iteration"
BEYOND = "step beyond maxiter (history capacity)"
ANOTHER = "smm_bgp_p2p_attach: rank of ANOTHER shard, 0 <= rank < N_global / N"


def call(c, name, *args):
    """the C entry point itself: its return code"""
    return c._fn(name)(c._ctx, *args)


def refused(c, code, text, name, *args):
    rc = call(c, name, *args)
    msg = c._fn("last_error")(c._ctx).decode()
    assert rc == code, (name, rc, msg)
    assert text in msg, (name, msg)


@pytest.fixture(scope="module")
def setup(S):
    """the problem, its options, and one device buffer that serves as any argument: larger than every buffer a call here may ask for"""
    import torch
    prob, opts = cm.serial_normal(N=32, T=4, ns=50)
    buf = torch.zeros(1 << 16, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    return S, prob, opts, buf


def ptr(buf, offset=0):
    return C.c_void_p(buf.data_ptr() + 8 * offset)


def test_single_shard(setup):
    S, prob, opts, buf = setup
    c = S.hip_context(prob, opts)
    refused(c, MAXITER, BEYOND, "bgp_step", 5)
    refused(c, MAXITER, BEYOND, "bgp_step_async", 5)
    refused(c, STATE, BEFORE_FIRST, "bgp_exchange_dev", ptr(buf))
    assert call(c, "bgp_step", 1) == 0


def test_shard_three_phase_and_values(setup):
    S, prob, opts, buf = setup
    c = S.hip_context(prob, shard_opts(opts, 2, 0))
    assert c.a2a_capacity() * 2 * c.record_doubles() <= 1 << 15
    refused(c, STATE, "smm_bgp_step needs a single shard (N == N_global); use the sharded calls", "bgp_step", 1)
    refused(c, STATE, "no iteration yet", "bgp_export_values_dev", ptr(buf))
    refused(c, STATE, "smm_bgp_a2a_pack_dev comes first", "bgp_a2a_apply_dev", ptr(buf))
    refused(c, STATE, BEFORE_FIRST, "bgp_exchange_dev", ptr(buf))
    refused(c, STATE, BEFORE_FIRST, "bgp_a2a_pack_dev", ptr(buf), ptr(buf))
    c.local_step()
    c.exchange_dev(buf.data_ptr())
    refused(c, STATE, RESOLVED, "bgp_exchange_dev", ptr(buf))
    refused(c, STATE, RESOLVED, "bgp_a2a_pack_dev", ptr(buf), ptr(buf))
    c.sync()
    c = S.hip_context(prob, shard_opts(opts, 2, 0))
    c.local_step()
    assert call(c, "bgp_a2a_pack_dev", ptr(buf), ptr(buf, 1 << 15)) == 0
    refused(c, STATE, "smm_bgp_a2a_pack_dev without smm_bgp_a2a_apply_dev: the exchange of this iteration would be dropped", "bgp_local_step")
    refused(c, STATE, RESOLVED, "bgp_exchange_dev", ptr(buf))
    refused(c, STATE, RESOLVED, "bgp_a2a_pack_dev", ptr(buf), ptr(buf))
    c.sync()


def test_shard_two_enqueue(setup):
    S, prob, opts, buf = setup
    c = S.hip_context(prob, shard_opts(opts, 2, 0))
    assert 32 * c.record_doubles() <= buf.numel()
    c.sharded_step(None, buf.data_ptr())
    refused(c, STATE, GATHER, "bgp_local_step")
    refused(c, STATE, GATHER, "bgp_export_records_dev", ptr(buf))
    refused(c, STATE, GATHER, "bgp_export_values_dev", ptr(buf))
    refused(c, INVALID, "gathered_prev required: the last records live there", "bgp_sharded_step", None, ptr(buf))
    assert call(c, "bgp_sharded_finish", None) == INVALID
    assert call(c, "bgp_sharded_step", ptr(buf), None) == INVALID
    c.sharded_finish(buf.data_ptr())
    c.sync()
    c.local_step()
    c.sync()


def test_shard_p2p_before_the_windows_stand(setup):
    S, prob, opts, buf = setup
    c = S.hip_context(prob, shard_opts(opts, 2, 0))
    refused(c, STATE, INIT_FIRST, "bgp_p2p_step", 1)
    refused(c, STATE, INIT_FIRST, "bgp_p2p_attach", 1, None, ptr(buf))
    assert call(c, "bgp_p2p_finish") == 0   # (nothing in the windows: nothing to settle)
    _, w = c.p2p_init()
    refused(c, STATE, "smm_bgp_p2p_step: not every rank's window is attached", "bgp_p2p_step", 1)
    refused(c, INVALID, ANOTHER, "bgp_p2p_attach", 0, None, C.c_void_p(w))
    refused(c, INVALID, ANOTHER, "bgp_p2p_attach", 5, None, C.c_void_p(w))
    handle = C.create_string_buffer(A.SMM_P2P_HANDLE_BYTES)
    assert call(c, "bgp_p2p_attach", 1, handle, C.c_void_p(w)) == INVALID
    assert call(c, "bgp_p2p_attach", 1, None, None) == INVALID
    assert call(c, "bgp_p2p_step", -1) == INVALID


def test_unequal_shard(setup):
    S, prob, opts, buf = setup
    o = shard_opts(opts, 2, 0)
    o.chain_offset = 8
    c = S.hip_context(prob, o)
    refused(c, STATE, "the p2p form needs equal shards (N_global a multiple of N, chain_offset a multiple of N)", "bgp_p2p_init", None, None)
    refused(c, STATE, "the values form needs equal shards (N_global a multiple of N, chain_offset a multiple of N)", "bgp_a2a_pack_dev", ptr(buf), ptr(buf))


def test_two_attached_contexts(setup):
    S, prob, opts, buf = setup
    ctxs = [S.hip_context(prob, shard_opts(opts, 2, r)) for r in range(2)]
    wins = [c.p2p_init()[1] for c in ctxs]
    for r, c in enumerate(ctxs):
        c.p2p_attach(1 - r, window=wins[1 - r])
    refused(ctxs[0], STATE, "smm_bgp_p2p_attach: this rank's window is attached already", "bgp_p2p_attach", 1, None, C.c_void_p(wins[1]))
    for c in ctxs:
        refused(c, MAXITER, BEYOND, "bgp_p2p_step", 5)
    for c in ctxs:   # in lockstep, one iteration at a time (test_gpu_p2p.p2p_run_lockstep)
        c.p2p_step(1)
    for c in ctxs:
        c.sync()
    for c in ctxs:
        refused(c, STATE, WINDOWS, "bgp_sharded_step", ptr(buf), ptr(buf))
        refused(c, STATE, WINDOWS, "bgp_sharded_finish", ptr(buf))
        refused(c, STATE, GATHER, "bgp_local_step")
        refused(c, STATE, GATHER, "bgp_export_records_dev", ptr(buf))
    for c in ctxs:
        c.p2p_finish()
    for c in ctxs:
        c.sync()
    for c in ctxs:
        c.local_step()
    for c in ctxs:
        c.sync()


def test_every_call_refuses_a_null_context(S):
    lib = A.load()
    n = 0
    for name, res, args in A.SYMBOLS:
        if res is not C.c_int or not args or args[0] is not C.c_void_p:
            continue
        rest = [None if hasattr(t, "contents") or t in (C.c_void_p, C.c_char_p) else t(0) for t in args[1:]]
        assert getattr(lib, name)(None, *rest) == INVALID, name
        n += 1
    assert n >= 40
