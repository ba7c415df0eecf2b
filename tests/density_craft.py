"""Crafted histories for smm_get_density (include/smmhip.h), to be installed with crafted_twin / seamed of test_gpu_reducer_caps.py.
Each is a function of the history of a real run, overwriting params and accepted; tests/test_density_craft.py shows without a GPU
that every branch named here is taken.

  small_history : 12 chains x 40 iterations.  Accepted-row columns of 0 .. 5 rows whose values walk every ending of the half-sample
                  mode; a state series with long holds; a chain whose row 0 is not accepted (its state series starts with NaN:
                  status 1); a column with more than 75 % equal values (IQR 0), a constant column and a constant zero column (the
                  fallbacks of the bandwidth's spread).
  seam_history  : 12 x 40.  Pooled accepted-row columns of 64, 65 and 200 rows whose shortest windows are placed: under
                  SMMHIP_GROUP_WIDE_MIN = 65 the columns of 65 and 200 rows take the grid-wide argmin in blocks of 64 windows' worth.
  long_history  : 16 chains x 513 iterations, every row below 512 accepted and row 512 of chain 0 alone: pooled columns of exactly
                  8192 (either selection over (0, 512)), 8193 (accepted rows over (0, 513)) and 8208 rows (all rows over (0, 513)).
                  The sorted column of all 8208 rows is a unit lattice with runs of half gaps, so that the shortest window of a mass
                  starts where the case says: in the first block, in the last, at the two sides of a seam between blocks, or twice
                  with equal widths in two blocks (the earlier one wins).
The placement is by gaps: a sorted column with gaps of 1 but for a run of k gaps of 1/2 from row i has its only shortest window of
k + 1 rows at i (all widths are multiples of 1/2: exact)."""
import numpy as np

import density_ref as DR

# --- small_history: per-chain columns --------------------------------------------------------------------------------------------------
HOLDS, LATE_START, IQR0, CONST, CONST_ZERO, GENERIC = 6, 7, 8, 9, 10, 11
# the accepted values of chains 1 .. 5 (parameter 0, parameter 1) and the ending of the mode each reaches
FEW = {1: ([7.0], [-0.0]), 2: ([1.0, 4.0], [2.0, 2.0]), 3: ([1.0, 2.0, 3.0], [0.0, 1.0, 3.0]), 4: ([0.0, 3.0, 4.0, 9.0], [5.0, 1.0, 0.0, 6.5]),
       5: ([0.0, 4.0, 5.0, 5.5, 9.0], [9.0, 5.5, 4.5, 4.0, 0.0])}
FEW_ENDINGS = {1: ("one", "one"), 2: ("two", "two"), 3: ("middle", "left"), 4: ("two", "two"), 5: ("right", "left")}


def small_history(h):
    T, N = h.accepted.shape
    assert (T, N) == (40, 12) and h.params.shape[1] == 2
    r = np.random.default_rng(5)
    h.params[...] = r.normal(size=h.params.shape)           # the rows nobody accepted: noise that select 0 reads
    h.accepted[...] = 0
    for c in range(6):                                      # chain c: c accepted rows, none at row 0
        rows = 2 + 3 * np.arange(c)
        h.accepted[rows, c] = 1
        for k in range(2):
            if c:
                h.params[rows, k, c] = FEW[c][k]
    h.accepted[[0, 17, 33], HOLDS] = 1                      # three states, held 17, 16 and 7 iterations
    h.accepted[3:, LATE_START] = r.random(37) < 0.5
    h.accepted[3, LATE_START] = 1
    for c in (IQR0, CONST, CONST_ZERO, GENERIC):
        h.accepted[:, c] = 1
    h.params[:, :, IQR0] = 1.5
    h.params[::5, 0, IQR0] = r.normal(size=8)               # 32 of 40 equal: both quartiles 1.5
    h.params[::5, 1, IQR0] = -3.0
    h.params[:, 0, CONST], h.params[:, 1, CONST] = 2.5, -0.75
    h.params[:, :, CONST_ZERO] = 0.0
    return h


# --- placed windows ----------------------------------------------------------------------------------------------------------------------
def placed(m, runs, k):
    """a sorted column of m rows: gaps of 1, but k gaps of 1/2 from each row of runs"""
    gaps = np.ones(m - 1)
    for i in runs:
        gaps[i: i + k] = 0.5
    return np.concatenate([[0.0], np.cumsum(gaps)]) - 16.0


def blocks_of(m, wmax, wide_min):
    """NB, the blocks of a grid-wide argmin in a call whose longest long column has wmax rows (smm_reducers_host.hpp: smm_get_density)"""
    per = min(256 * 16, max(1, wide_min - 1))
    return min(1024, max(1, -(-wmax // per)))


def window_block(i, cnt, NB):
    """the block whose slice of the cnt windows holds window i (smm_density.hpp: k_dens_win)"""
    return i // -(-cnt // NB)


def hdi_placement(s, p, NB):
    """(first row of the HDI, its block, the blocks of every window as short as it)"""
    m = len(s)
    k = DR.hdi_span(p, m)
    w = s[k:] - s[: m - k]
    i = int(np.argmin(w))
    return i, window_block(i, m - k, NB), sorted({window_block(int(j), m - k, NB) for j in np.flatnonzero(w == w[i])})


# --- seam_history: pooled columns of 64 / 65 / 200 accepted rows ------------------------------------------------------------------------
SEAM_GROUPS = np.array([0, 0, 1, 1, 2, 2, 2, 2, 2, 3, 3, -1], np.int32)
SEAM_NG, SEAM_MASS, SEAM_WIDE_MIN = 4, 0.25, 65
SEAM_ROWS = {0: 64, 1: 65, 2: 200}                          # (group 3: 80 rows of noise)
# (group, parameter): the runs of half gaps (k = floor(0.25 m)): 65 rows: k = 16, 49 windows; 200 rows: k = 50, 150 windows, 4 blocks of 38
SEAM_RUNS = {(0, 0): [30], (0, 1): [0], (1, 0): [13], (1, 1): [12], (2, 0): [10, 80], (2, 1): [149]}


def seam_history(h):
    T, N = h.accepted.shape
    assert (T, N) == (40, 12) and h.params.shape[1] == 2
    r = np.random.default_rng(6)
    h.params[...] = r.normal(size=h.params.shape)
    h.accepted[...] = 1
    h.accepted[32:, [0, 1, 2]] = 0                          # 32 + 32 = 64, 32 + 33 = 65 accepted rows
    h.accepted[33:, 3] = 0
    for (g, k), runs in SEAM_RUNS.items():
        m = SEAM_ROWS[g]
        s = r.permutation(placed(m, runs, DR.hdi_span(SEAM_MASS, m)))
        at = 0
        for c in np.flatnonzero(SEAM_GROUPS == g):
            rows = np.flatnonzero(h.accepted[:, c])
            h.params[rows, k, c] = s[at: at + len(rows)]
            at += len(rows)
        assert at == m
    return h


# --- long_history ------------------------------------------------------------------------------------------------------------------------
LONG_N, LONG_T = 16, 513
LONG_M = LONG_N * LONG_T                                    # 8208
LONG_CASES = ("first", "last", "seam", "tie")
# parameter 0's runs per case, with the mass whose HDI they place (k = floor(mass 8208)); parameter 1: the seam's other side, or noise
LONG_MASS = {"first": 0.5, "last": 0.5, "seam": 0.5, "tie": 0.25}
LONG_RUNS = {"first": ([5], None), "last": ([4000], None), "seam": ([1367], [1368]), "tie": ([100, 2652], None)}


def long_history(case):
    def craft(h):
        T, N = h.accepted.shape
        assert (T, N) == (LONG_T, LONG_N) and h.params.shape[1] == 2
        r = np.random.default_rng(7)
        h.accepted[...] = 1
        h.accepted[512, 1:] = 0
        k = DR.hdi_span(LONG_MASS[case], LONG_M)
        for par, runs in enumerate(LONG_RUNS[case]):
            s = placed(LONG_M, runs, k) if runs is not None else r.normal(size=LONG_M)
            h.params[:, par, :] = r.permutation(s).reshape(T, N)
        return h
    return craft
