"""The design of density_craft.py's histories, checked on the restatement alone (density_ref.py): the columns have the row counts, the
statuses, the endings of the mode and the fallbacks of the bandwidth that the GPU tests rely on, and the shortest windows of the placed
columns start in the blocks the cases name, with the tie's two windows in two blocks.  Without this the GPU tests could pass
vacuously.  CPU only."""
import numpy as np
import pytest

import chain_stats_ref as CS
import density_craft as DC
import density_ref as DR
import hist_ref as HR
import profile_ref as PR

PER_CHAIN = np.arange(12, dtype=np.int32)


def test_small_history_counts_statuses_endings_and_fallbacks(O):
    h = DC.small_history(PR.zeroed_history(40, 12, 2, 2))
    cols = HR.columns(h, 0, 40, 1, PER_CHAIN, 12)
    assert [x.shape[1] for x in cols[:6]] == [0, 1, 2, 3, 4, 5]
    for c, ends in DC.FEW_ENDINGS.items():
        for k in range(2):
            trail = []
            DR.half_sample_mode(CS.total_sort(cols[c][k]), trail)
            assert trail[-1] == ends[k], (c, k, trail)
    assert {e for ends in DC.FEW_ENDINGS.values() for e in ends} == {"one", "two", "left", "right", "middle"}
    took = {}
    for c in (DC.IQR0, DC.CONST, DC.CONST_ZERO, DC.GENERIC):
        trail = []
        DR.bw_nrd0(cols[c][0], CS.total_sort(cols[c][0]), trail=trail)
        took[c] = trail[0]
    assert took[DC.IQR0] == "sd0" and took[DC.CONST] == "first" and took[DC.CONST_ZERO] == "one" and took[DC.GENERIC] in ("sd", "iqr")
    assert (cols[DC.IQR0][0] == 1.5).sum() == 32
    state = HR.columns(h, 0, 40, 2, PER_CHAIN, 12)
    x = state[DC.HOLDS][0]
    assert len(np.unique(x)) == 3 and sorted(np.unique(x, return_counts=True)[1]) == [7, 16, 17]   # long holds
    assert np.isnan(state[DC.LATE_START][0][:3]).all() and np.isfinite(state[DC.LATE_START][0][3:]).all()
    want = DR.density_from_history(h, 0, 40, 2, PER_CHAIN, [0.5], 4)
    assert (want["status"][DC.LATE_START] == 1).all() and (want["status"][DC.HOLDS] == 0).all()
    want = DR.density_from_history(h, 0, 40, 1, PER_CHAIN, [0.5], 4)
    assert (want["status"][0] == 2).all() and (want["kde_status"][1] == 1).all() and (want["kde_status"][2:6] == 0).all()


def test_seam_history_rows_and_placements():
    h = DC.seam_history(PR.zeroed_history(40, 12, 2, 2))
    cols = HR.columns(h, 0, 40, 1, DC.SEAM_GROUPS, DC.SEAM_NG)
    assert [x.shape[1] for x in cols] == [64, 65, 200, 80]
    NB = DC.blocks_of(200, 200, DC.SEAM_WIDE_MIN)
    assert NB == 4
    seen = {}
    for (g, k), runs in DC.SEAM_RUNS.items():
        i, blk, tied = DC.hdi_placement(CS.total_sort(cols[g][k]), DC.SEAM_MASS, NB)
        assert i == runs[0], (g, k, i)
        seen[(g, k)] = (blk, tied)
    assert seen[(1, 0)][0] == 1 and seen[(1, 1)][0] == 0              # the two sides of the first seam between blocks
    assert seen[(2, 0)] == (0, [0, 2])                                # a tie across blocks: the earlier wins
    assert seen[(2, 1)] == (3, [3])                                   # the last window of the last block
    # under the seam the mode of the 200 rows takes two grid-wide levels (200, 100 >= 65), that of the 65 rows one
    for m, levels in ((200, 2), (65, 1), (64, 0)):
        n, lv = m, 0
        while n > 3 and n >= DC.SEAM_WIDE_MIN:
            n, lv = (n + 1) // 2, lv + 1
        assert lv == levels


@pytest.mark.parametrize("case", DC.LONG_CASES)
def test_long_history_rows_and_placements(case):
    h = DC.long_history(case)(PR.zeroed_history(DC.LONG_T, DC.LONG_N, 2, 2))
    assert HR.columns(h, 0, 512, 0, np.zeros(16, np.int32), 1)[0].shape[1] == 8192
    assert HR.columns(h, 0, 512, 1, np.zeros(16, np.int32), 1)[0].shape[1] == 8192
    assert HR.columns(h, 0, 513, 1, np.zeros(16, np.int32), 1)[0].shape[1] == 8193
    x = HR.columns(h, 0, 513, 0, np.zeros(16, np.int32), 1)[0]
    assert x.shape[1] == DC.LONG_M == 8208
    NB = DC.blocks_of(8208, 8208, 8193)
    assert NB == 3
    i, blk, tied = DC.hdi_placement(CS.total_sort(x[0]), DC.LONG_MASS[case], NB)
    assert i == DC.LONG_RUNS[case][0][0]
    assert (blk, tied) == {"first": (0, [0]), "last": (2, [2]), "seam": (0, [0]), "tie": (0, [0, 1])}[case]
    if case == "seam":
        assert DC.hdi_placement(CS.total_sort(x[1]), DC.LONG_MASS[case], NB)[:2] == (1368, 1)
