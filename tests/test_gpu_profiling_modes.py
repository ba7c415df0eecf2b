"""Profiling mode 2 (smm_set_profiling(ctx, 2): the dispatches' own begin/end stamps), the mode bench.py measures with: which stand-alone
resolutions of the exchange take the stamps and which leave the iteration to event brackets, and that no mode changes what is computed."""
import numpy as np
import pytest

import common as cm

pytestmark = pytest.mark.gpu

N, T = 32, 16   # two 16-chain tiles; exchangeMoves! is active from iteration 2 on

CASES = {
    # one min_improve = 0 for all chains: the lean kernel, stamped
    "lean": dict(min_improve=0.0, env={}, exchange="lean", stamped=True),
    # a threshold of its own per chain: k_exch_resolve_lvl<1024>, stamped
    "lvl": dict(min_improve=np.random.default_rng(N).uniform(-0.2, 0.4, N), env={}, exchange="lvl", stamped=True),
    # ... on the workgroup of 256 lanes the test build offers: not stamped, the iteration is bracketed by events
    "lvl_wg256": dict(min_improve=np.random.default_rng(N).uniform(-0.2, 0.4, N), env={"SMMHIP_LVL_WG": "256"}, exchange="lvl", stamped=False),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_profiling_modes_compute_the_same_and_mode_2_stamps_the_resolutions_it_always_did(S, hooks, monkeypatch, case):
    """objfunc_norm, 2 parameters, 32 chains, ns = 64, one launch per iteration with the inline walk off (every exchange goes to the
    stand-alone kernel).  The same step under profiling 0, 1 and 2 gives one history and one state; mode 2 reports the exchange kernel's
    own time where the resolution is stamped (lean, lvl<1024>) and only there."""
    spec = CASES[case]
    monkeypatch.setenv("SMMHIP_INLINE_WALK", "0")
    for k, v in spec["env"].items():
        monkeypatch.setenv(k, v)
    prob, opts = cm.serial_normal(N=N, T=T, ns=64, min_improve=spec["min_improve"])
    runs = {}
    for mode in (0, 1, 2):
        h = S.hip_context(prob, opts)
        d = h.describe()
        assert d["exchange"] == spec["exchange"] and d["walk"] == "standalone", d
        h.set_persistent(False)
        h.set_profiling(mode)
        h.step(T)
        t = h.timing()
        runs[mode] = (h.history(), h.state(), t)
        print(case, "mode", mode, "step_ms", t.step_ms, "iter_kernel_ms", t.iter_kernel_ms, "exch_kernel_ms", t.exch_kernel_ms,
              "null_bracket_ms", t.null_bracket_ms, "iters", t.iters, "chain_evals", t.chain_evals)
    h0, s0, t0 = runs[0]
    assert int((h0.exchanged != 0).any(axis=1).sum()) >= 2   # iterations with a resolved exchange that moved somebody
    for mode in (1, 2):
        hm, sm, tm = runs[mode]
        cm.assert_history_equal(hm, h0, exact_floats=True)
        assert sm.iter == s0.iter
        for f in ("la_status", "n_noex", "n_acc_noex", "best_id", "sigma", "accept_rate", "la_value", "la_prob", "la_params", "la_sim_moments", "best_val"):
            assert np.array_equal(getattr(sm, f), getattr(s0, f), equal_nan=True), f
        assert tm.iters == t0.iters == T and tm.chain_evals == t0.chain_evals == T * N
    for mode in (0, 1, 2):
        t = runs[mode][2]
        assert all(np.isfinite(x) for x in (t.step_ms, t.iter_kernel_ms, t.exch_kernel_ms, t.null_bracket_ms)), mode
    t2 = runs[2][2]
    if spec["stamped"]:
        assert t2.exch_kernel_ms > 0 and t2.null_bracket_ms == 0
    else:
        assert t2.exch_kernel_ms == 0 and t2.iter_kernel_ms > 0
