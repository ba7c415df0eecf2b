"""Every site that stages and reads out a walk of the WHOLE exchange list (smm_walk_lean.hpp, smm_walk_slots.hpp and their callers in
smm_chain.hpp, smm_chain_norm.hpp, smm_exchange.hpp), at the population sizes where its staging can go wrong: fewer chains than a
slot piece holds, sizes that are and are not a multiple of 4 (the slots' padding, the dummy slots right behind the chains'), one
chain past a wave, a 16-byte piece or a 1 KB LDS-DMA piece, a share of the workgroup's lanes that is exactly absent, more chains than
lanes.  Each case is one small context without the persistent form against the CPU oracle on the same shocks: the oracle is the only
reference that shares no code with the walks."""
import numpy as np
import pytest

import common as cm
from smm_jl_amd import _abi as A

pytestmark = pytest.mark.gpu

NS, T = 64, 40


def by_chain(N):
    """thresholds by chain, one of them negative (no lean plan, no persistent form: the walks on 16-byte slots and the level plan)"""
    mi = np.linspace(0.0, 0.05, N)
    mi[N // 2] = -0.02
    return mi


def serial(N, mi, T=T, **kw):
    return cm.serial_normal(N=N, T=T, ns=NS, min_improve=mi, **kw)


def general6(N, mi, T=T, **kw):
    prob, opts = cm.general_normal(6, N=N, T=T, ns=NS, **kw)
    opts.min_improve[:] = mi
    return prob, opts


def banana10(N, mi, T=T):
    prob = cm.S.Problem(init=np.zeros(10), lb=-2 * np.ones(10), ub=2 * np.ones(10), mom=np.zeros(10), w=np.ones(10), ns=1,
                        objective_id=A.SMM_OBJ_BANANA)
    opts = cm.S.BGPOpts(N=N, maxiter=T, sigma=0.01 * cm.temps(N, 4), acc_tuner=np.geomspace(2.0, 0.1, N), min_improve=np.full(N, float(mi)),
                        seed=3, N_global=N)
    return prob, opts


# (site, builder, thresholds, what describe() must say, SMMHIP_* seams, population sizes, further arguments of the builder)
SITES = [
    ("lean_registers", serial, 0.0, dict(walk="inline_lean"), {}, (2, 3, 5, 127, 129, 1000), {}),
    # (whole 1 KB pieces of slots straight into LDS; 384: the second piece of wave 1 is exactly absent)
    ("lean_lds_dma", serial, 0.0, dict(walk="inline_lean"), {}, (128, 384, 512), {}),
    ("lean_wide", serial, 0.05, dict(walk="inline_lean_wide"), {}, (2, 3, 5, 129, 1000), {}),
    ("tile_lean16_keys_plan", general6, 0.0, dict(walk="inline_lean16"), {}, (2, 3, 5, 130, 1000), {}),
    ("tile_lean16_wide_plan", general6, 0.05, dict(walk="inline_lean16"), {}, (2, 3, 5, 130, 1000), {}),
    ("slots_fast", serial, by_chain, dict(walk="inline_slots", chain="iter_norm_any"), {}, (2, 3, 65, 1000), {}),
    ("slots_tile", general6, by_chain, dict(walk="inline_slots", chain="iter<sim,8>"), {}, (3, 65, 1000), {}),
    ("slots_tile_absdiff", general6, by_chain, dict(walk="inline_slots", chain="iter<sim,8>"), {}, (65,), dict(dist_fun=A.SMM_DIST_ABSDIFF)),
    ("resolve_lean_keys", serial, 0.0, dict(walk="standalone", exchange="lean"), {"SMMHIP_INLINE_WALK": "0"}, (2, 3, 5, 129, 1000), {}),
    ("resolve_lean_wide", serial, 0.05, dict(walk="standalone", exchange="lean"), {"SMMHIP_INLINE_WALK": "0"}, (2, 3, 5, 129, 1000), {}),
    ("resolve_lvl", serial, by_chain, dict(walk="standalone", exchange="lvl"), {"SMMHIP_INLINE_WALK": "0"}, (3, 65, 1000), {}),
    ("resolve_lvl_soa", serial, by_chain, dict(walk="standalone", exchange="lvl_soa"), {}, (4100,), dict(T=12)),
    # (not whole groups of 32 chains: no cones, every workgroup walks the whole list)
    ("tile_keys", banana10, 0.0, dict(walk="inline_keys"), {}, (4100,), dict(T=12)),
]
CASES = [pytest.param(site, build, mi, want, env, N, kw, id="%s-%d" % (site, N)) for site, build, mi, want, env, Ns, kw in SITES for N in Ns]


def problem_of(build, mi, N, kw):
    return build(N, mi(N) if callable(mi) else mi, **kw)


@pytest.mark.parametrize("site,build,mi,want,env,N,kw", CASES)
def test_whole_list_walk_site_against_oracle(S, O, monkeypatch, hooks, site, build, mi, want, env, N, kw):
    prob, opts = problem_of(build, mi, N, kw)
    steps = opts.maxiter
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    h = S.hip_context(prob, opts)
    h.set_persistent(False)
    d = h.describe()
    print(site, N, d)
    assert {k: d[k] for k in want} == want, d
    h.step(steps)
    assert h.persistent_info()[1] == 0, h.persistent_info()   # (no persistent launch: the per-iteration site did the walking)
    o = O.OracleContext(prob, opts, S.Tables(Z=h.Z()))
    o.step(steps)
    hh = h.history()
    assert (hh.exchanged != 0).any()   # (a walk that never swaps proves nothing)
    cm.assert_history_equal(hh, o.history())
    cm.assert_state_equal(h.state(), o.state())
