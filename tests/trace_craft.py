"""A history for smm_get_trace's member-block seams (tests/test_gpu_trace_seams.py on the device; tests/test_trace_craft.py checks the
design here, without a GPU).  k_trace_gather walks a group's members 256 at a time and carries the rank base and the best (value,
position) across the blocks; k_trace_column sorts a column in LDS up to 8192 members and selects by radix past that.  So: groups of
8193, 8192, 513, 257, 256, 255, 1 and 0 members (and chains in no group), the chains dealt to them by a fixed permutation so that the
member lists are scattered; and per iteration a pattern of accepted rows, a placement of the best value, flags at the seams and
columns with ties, all stated by the member's position in its group's list (ascending chain index), the same for every group that has
the position:

  t  accepted                                    value (else distinct, >= 2)
  0  nobody                                      -5 at positions 255 and 256: the earlier one is the best
  1  only position 255                           -5 at position 0 and at the last
  2  only position 256                           -7 at position 10, NaN at position 300 (at the last of a group of 257): NaN is the best
  3  only the last position                      NaN at positions 5 and 261: the first
  4  nobody below 256, everybody from there on   -5 at positions 7, 263 and (where it exists) 7943: the first
  5  everybody                                   -9 at the last position alone

A position a group does not have is skipped.  exchanged is set at the positions of SEAMS where position + t is even, status -1 where
it is a multiple of 3.  Parameter 0 holds distinct values in scattered order, parameter 1 the two values -0.5 and 1.5 in equal shares
(alternating along the list, shifted by t), moment 0 is 3.25 everywhere, moment 1 is distinct with a single NaN at iteration 2 in the
last position.  The state series (select 2) is NaN for everybody at t = 0 and for all but one, two, three members at t = 1, 2, 3: the
rows without a state lie in every block."""
import numpy as np

SIZES = (8193, 8192, 513, 257, 256, 255, 1, 0)
N_GROUPS = len(SIZES)
N = 17920                                                  # 17667 members and 253 chains in no group
T = 6
BLOCK = 256                                                # smm_trace.hpp: TRACE_WG, the members of one block of k_trace_gather
LDS_N = 8192                                               # smm_stats.hpp: STATS_LDS_N, the longest column sorted in LDS
SEAMS = (0, 254, 255, 256, 257, 511, 512, 513, 8190, 8191, 8192)
PROBS = (0.0, 0.025, 0.5, 1.0)


def groups():
    """int32 [N]: the group of every chain, -1 for none"""
    perm = np.random.default_rng(3).permutation(N)
    g = np.full(N, -1, np.int32)
    at = 0
    for i, m in enumerate(SIZES):
        g[perm[at:at + m]] = i
        at += m
    return g


GROUPS = groups()
MEMBERS = [np.flatnonzero(GROUPS == g) for g in range(N_GROUPS)]   # ascending chain index: the position is the index into this list


def accepted_positions(t, m):
    """the positions of a group of m members that are accepted at iteration t"""
    p = np.arange(m)
    return p[[np.zeros(m, bool), p == 255, p == 256, p == m - 1, p >= 256, np.ones(m, bool)][t]]


def best_placement(t, m):
    """[(position, value)] written at iteration t into a group of m members, positions the group lacks left out"""
    last = m - 1
    w = [[(255, -5.0), (256, -5.0)], [(0, -5.0), (last, -5.0)], [(10, -7.0), (300 if m > 300 else last if m > 256 else -1, np.nan)],
         [(5, np.nan), (261, np.nan)], [(7, -5.0), (263, -5.0), (7943, -5.0)], [(last, -9.0)]][t]
    return [(p, v) for p, v in w if 0 <= p < m]


def best_position(t, m):
    """the position smm_get_trace reports at iteration t: the first NaN, else the first minimum (-1 for an empty group)"""
    w = best_placement(t, m)
    if m == 0:
        return -1
    if not w:
        return None                                        # no placement fits (a group of one at some iterations): whatever argmin says
    nan = [p for p, v in w if v != v]
    if nan:
        return min(nan)
    lo = min(v for _, v in w)
    return min(p for p, v in w if v == lo)


def crafted(h):
    """h (np = nm = 2, T iterations of N chains) overwritten in every field the trace reads"""
    assert h.value.shape == (T, N) and h.params.shape[1] == 2 and h.sim_moments.shape[1] == 2
    i = np.arange(T * N).reshape(T, N)
    scat = lambda mul: ((i * mul) % (T * N)) / 1024.0
    h.value[...] = 2.0 + scat(7919)
    h.params[:, 0, :] = scat(10007) - 40.0
    h.sim_moments[:, 0, :] = 3.25
    h.sim_moments[:, 1, :] = scat(4999) * 0.5
    h.params[:, 1, :] = 0.0
    h.accepted[...] = 0
    h.exchanged[...] = 0
    h.status[...] = 0
    for mem in MEMBERS:
        m = len(mem)
        pos = np.arange(m)
        for t in range(T):
            h.params[t, 1, mem] = np.where((pos + t) % 2 == 0, -0.5, 1.5)
            h.accepted[t, mem[accepted_positions(t, m)]] = 1
            for p, v in best_placement(t, m):
                h.value[t, mem[p]] = v
            for p in SEAMS:
                if p < m:
                    h.exchanged[t, mem[p]] = mem[(p + 1) % m] + 1 if (p + t) % 2 == 0 else 0
                    h.status[t, mem[p]] = -1 if (p + t) % 3 == 0 else 0
        if m:
            h.sim_moments[2, 1, mem[m - 1]] = np.nan
    return h
