"""A crafted history for smm_get_reweighted's edges (include/smmhip.h, smm.jl_amd/csrc/smm_reweight.hpp): crafted() writes params,
sim_moments, value and accepted into a HistoryBuffers (`into`, as adjust_craft.py's builders do) and returns what its construction
implies, so that an expected value comes neither from reweight_ref.py nor from the device.  Eight chains of CRAFT_T rows, np = nm = 2,
every row selected by select 0, with the acc_tuner of CRAFT_ACC and the targets of CRAFT_TARGETS:

  group 0 : chain 0 plain; chain 1 without a scored row (every value NaN or infinite); chain 2 with one scored row.
  group 1 : chains 3 and 4, acc_tuner 4 and 0.25 around the target 1: d of both signs in one group.  Chain 3 holds one value of 1e4
            among values below 2: at the target 1, d = 3, lw - L <= -29994 for every other row, so their weights are exactly 0 and the
            chain's sums are 1; at the target 8, d = -4 and the 1e4 row is the one whose weight is 0.
  group 2 : chain 5 with one value of 1e308: at the targets below its acc_tuner 3 (d >= 2) d * v overflows to +inf, L is not finite:
            status 3; at the target 8 (d = -5) the product is -inf, the row's weight 0 and the group's status 0.
  group 3 : chain 6 with an infinite parameter in a scored row: status 2 at every target.
  group 4 : chain 7, parameters on a grid of quarters with both zeros, so every quantile key is a tie run; its acc_tuner is the target
            1, so w = u = 1 and q = 2^20 for every row: the quantiles are those of equal weights.

tests/test_reweight.py holds these against reweight_ref.py without a GPU; tests/test_gpu_reweighted.py holds the device against both."""
import numpy as np

from adjust_craft import zero_history

CRAFT_N, CRAFT_T = 8, 40
CRAFT_ACC = np.array([2.0, 1.5, 0.5, 4.0, 0.25, 3.0, 1.0, 1.0])
CRAFT_GROUPS = np.array([0, 0, 0, 1, 1, 2, 3, 4], np.int32)
CRAFT_TARGETS = (1.0, 0.0, 8.0)
CRAFT_PROBS = (0.0, 0.25, 0.5, 1.0)
BIG_ROW, ONE_ROW, HUGE_ROW, INF_ROW = 17, 23, 5, 31


def crafted(seed=11, into=None):
    """(h, info): info holds groups, acc, targets, probs and what the construction implies: status [R][G], chain_n [N], the exact
    per-chain results of chain 3 at the target 1 and the equal-weight quantiles of group 4 [len(probs)][np]"""
    N, T = CRAFT_N, CRAFT_T
    h = zero_history(T, N, 2, 2) if into is None else into
    assert h.value.shape == (T, N) and h.params.shape == (T, 2, N)
    rng = np.random.default_rng([seed, N, T])
    theta = rng.uniform(-1.0, 1.0, (T, 2, N))
    theta[:, :, 7] = np.round(rng.uniform(-1.0, 1.0, (T, 2)) * 4.0) / 4.0      # quarters: tie runs at every key
    theta[0, 0, 7], theta[1, 0, 7] = 0.0, -0.0
    mom = theta + 0.125 * rng.standard_normal((T, 2, N))
    value = 0.5 * (theta * theta).sum(axis=1) + rng.uniform(0.0, 1.0, (T, N))  # in [0, 2)
    value[:, 1] = np.where(np.arange(T) % 2 == 0, np.nan, np.inf)             # chain 1: nothing scored
    value[::3, 1] = -np.inf
    value[:, 2] = np.inf                                                      # chain 2: one scored row
    value[ONE_ROW, 2] = 0.75
    value[BIG_ROW, 3] = 1e4
    value[HUGE_ROW, 5] = 1e308
    theta[INF_ROW, 1, 6] = np.inf
    h.params[...], h.sim_moments[...], h.value[...] = theta, mom, value
    h.accepted[...] = 1
    R, G = len(CRAFT_TARGETS), 5
    status = np.zeros((R, G), np.int32)
    status[:, 3] = 2
    status[0, 2] = status[1, 2] = 3
    chain_n = np.array([T, 0, 1, T, T, T, T, T], np.int32)
    # group 4 at the target 1: equal weights q = 2^20, Q = T 2^20; the inverted CDF at p is the ceil(p T)-th smallest (at least the first)
    from reweight_ref import total_order_key
    quant = np.empty((len(CRAFT_PROBS), 2))
    for j in range(2):
        col = theta[:, j, 7]
        srt = col[np.argsort(total_order_key(col), kind="stable")]
        for i, p in enumerate(CRAFT_PROBS):
            quant[i, j] = srt[max(1, int(np.ceil(p * T))) - 1]
    info = dict(groups=CRAFT_GROUPS, acc=CRAFT_ACC, targets=CRAFT_TARGETS, probs=CRAFT_PROBS, status=status, chain_n=chain_n,
                chain3=dict(ess=1.0, logz=3.0 * 1e4 + np.log(1.0 / T), kept=1), quantile4=quant)
    return h, info
