"""smm_get_density on the device at its seams (include/smmhip.h, smm.jl_amd/csrc/smm_density.hpp and its plan in
smm_reducers_host.hpp), every output equal bit for bit to density_ref.py over the read-back history of density_craft.py's crafted
histories (their design is checked without a GPU in tests/test_density_craft.py):

  the shipped library at 8192 / 8193 / 8208 pooled rows: the sort in LDS against the segmented radix sort, the window argmin in one
      workgroup against the grid-wide one in 3 blocks, one chunk of the density's sum against two; the shortest window placed in the
      first block, in the last, at both sides of a seam between blocks, and tied across blocks;
  the placed columns of 64 / 65 / 200 rows on the shipped library (all in LDS) and under SMMHIP_GROUP_WIDE_MIN = 65 (65 and 200 rows
      grid-wide in 4 blocks, the mode's grid-wide levels run twice), equal to each other;
  SMMHIP_STATS_SCRATCH = 1: one group and one parameter per batch, equal to the unbatched results."""
import numpy as np
import pytest

import common as cm
import density_craft as DC
import density_ref as DR
from test_gpu_reducer_caps import crafted_twin, seamed

pytestmark = pytest.mark.gpu

MASS = [0.25, 0.5, 0.94, 1.0]
ONE = np.zeros(DC.LONG_N, np.int32)


@pytest.mark.parametrize("case", DC.LONG_CASES)
def test_shipped_library_at_8192_8193_8208_rows(S, request, monkeypatch, case):
    prob, opts = cm.serial_normal(N=DC.LONG_N, T=DC.LONG_T, ns=100)
    h, state, crafted, back = crafted_twin(S, prob, opts, DC.LONG_T, DC.long_history(case))
    got = {}
    for t1, select, rows in ((512, 0, 8192), (513, 1, 8193), (513, 0, 8208), (512, 2, 8192)):
        want = DR.density_from_history(back, 0, t1, select, ONE, MASS, 5)
        assert want["count"][0] == rows and (want["status"] == 0).all()
        got[(t1, select)] = h.density(0, t1, select, None, MASS, 5)
        DR.assert_density_equal(got[(t1, select)], want)
    if case == "tie":   # the same from the test build under the batch seam: one parameter at a time
        request.getfixturevalue("hooks")
        hs = seamed(S, monkeypatch, prob, opts, state, crafted, STATS_SCRATCH=1)
        for (t1, select), g in got.items():
            DR.assert_density_equal(hs.density(0, t1, select, None, MASS, 5), g)


@pytest.fixture(scope="module")
def placed(S):
    prob, opts = cm.serial_normal(N=12, T=40, ns=100)
    h, state, crafted, back = crafted_twin(S, prob, opts, 40, DC.seam_history)
    calls = [(0, 40, 1, DC.SEAM_GROUPS, DC.SEAM_NG, 8), (0, 40, 0, DC.SEAM_GROUPS, DC.SEAM_NG, 3), (0, 40, 2, None, 1, 2),
             (3, 40, 1, np.arange(12, dtype=np.int32), 12, 4)]
    want = [DR.density_from_history(back, t0, t1, sel, g, MASS, ng_, n_groups=G) for t0, t1, sel, g, G, ng_ in calls]
    assert want[0]["count"].tolist() == [64, 65, 200, 80]
    return dict(prob=prob, opts=opts, h=h, state=state, crafted=crafted, calls=calls, want=want)


def run_calls(h, placed):
    for (t0, t1, sel, g, G, n_grid), want in zip(placed["calls"], placed["want"]):
        DR.assert_density_equal(h.density(t0, t1, sel, g, MASS, n_grid, n_groups=G), want)


def test_placed_windows_on_the_shipped_library(placed):
    run_calls(placed["h"], placed)


@pytest.mark.parametrize("seams", (dict(GROUP_WIDE_MIN=65), dict(STATS_SCRATCH=1), dict(GROUP_WIDE_MIN=65, STATS_SCRATCH=1),
                                   dict(GROUP_WIDE_MIN=2)))
def test_placed_windows_under_the_seams(S, hooks, monkeypatch, placed, seams):
    h = seamed(S, monkeypatch, placed["prob"], placed["opts"], placed["state"], placed["crafted"], **seams)
    run_calls(h, placed)
    cm.assert_history_equal(h.history(), placed["h"].history(), exact_floats=True)
