"""The end of a chain's iteration — doAcceptReject! (AlgoBGP.jl:324-392), set_acceptRate! (:253-257), the sigma update (:381-390), set_eval!
(:220-245) and the swapped row of swap_ev_ij! (:734-749) — in each of the five chain kernels at its smallest shape, against the oracle
to the bit: k_chain_iter_norm*, k_chain_persist_loc, k_chain_iter, k_chain_persist_tile and k_chain_persist_gen.  The launches end at
iterations 1, 5 and 10 and sigma is updated every third iteration (3, 6, 9): updates inside a launch, and two launches whose last iteration
is no update (the accept rate a launch leaves behind is computed for its last iteration too).  Iteration 1 runs on the per-iteration
kernel, as the persistent forms require.  Every case must have worked: swapped rows, rejections, plain acceptances (iteration 1's, accepted
whatever the objective says, are not counted) and a changed sigma in every chain, counted on the ORACLE's history."""
import numpy as np
import pytest

import common as cm
from smm_jl_amd import _abi as A

pytestmark = pytest.mark.gpu

STEPS = (1, 4, 5)
T = sum(STEPS)


def failbox(S):
    return cm.serial_normal(N=32, T=T, ns=512, objective_id=A.SMM_OBJ_NORM_FAILBOX, obj_params=[-0.2, 0.1], sigma_update_steps=3)


def norm6(S):
    return cm.general_normal(6, N=32, T=T, ns=256, sigma_update_steps=3)


def banana(S):
    prob = S.Problem(init=np.zeros(10), lb=-2 * np.ones(10), ub=2 * np.ones(10), mom=np.zeros(10), w=np.ones(10), ns=1, objective_id=A.SMM_OBJ_BANANA)
    return prob, S.BGPOpts(N=64, maxiter=T, sigma=0.002 * cm.temps(64, 5), acc_tuner=np.geomspace(20, 1, 64), min_improve=np.zeros(64), seed=3,
                           sigma_update_steps=3)


# (kernel, problem, persistent, describe()["chain"] starts with, describe()["persistent"], rows of status -2 wanted)
CASES = [
    ("k_chain_iter_norm", failbox, False, "iter_norm", "loc", 5),
    ("k_chain_persist_loc", failbox, True, "iter_norm", "loc", 5),
    ("k_chain_iter", norm6, False, "iter<sim", "tile_sim", 0),
    ("k_chain_persist_tile", norm6, True, "iter<sim", "tile_sim", 0),
    ("k_chain_persist_gen", banana, True, "iter<gen", "gen", 0),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_accept_step_of_every_chain_kernel_against_the_oracle(S, O, case):
    kernel, build, persistent, chain, form, failed = case
    prob, opts = build(S)
    h = S.hip_context(prob, opts)
    d = h.describe()
    assert d["chain"].startswith(chain) and d["persistent"] == form, d
    if not persistent:
        h.set_persistent(False)
    o = O.OracleContext(prob, opts, S.Tables(Z=h.Z()))
    for n in STEPS:
        h.step(n); o.step(n)
    avail, launches, repairs = h.persistent_info()
    assert (launches == 2 and repairs == 0) if persistent else launches == 0, (kernel, launches, repairs)
    oh = o.history()
    swapped = oh.exchanged != 0
    n_swapped, n_rejected = int(swapped.sum()), int((~swapped & (oh.accepted == 0)).sum())
    n_accepted = int((~swapped & (oh.accepted != 0))[1:].sum())
    n_failed = int((oh.status == -2).sum())
    print("%s: %d swapped, %d rejected, %d accepted behind iteration 1, %d of status -2" % (kernel, n_swapped, n_rejected, n_accepted, n_failed))
    assert n_swapped >= 30 and n_rejected >= 30 and n_accepted >= 30 and n_failed >= failed, (n_swapped, n_rejected, n_accepted, n_failed)
    assert (o.state().sigma != np.asarray(opts.sigma)).all()
    cm.assert_history_equal(h.history(), oh, exact_floats=True)
    cm.assert_state_equal(h.state(), o.state(), rtol=0)
