"""smm_get_trace on the device at its member-block seams (include/smmhip.h, smm.jl_amd/csrc/smm_trace.hpp): k_trace_gather's walk over a
group's members 256 at a time (block_rank's base and the best (value, position) carried across the blocks, the counts summed over
them) and k_trace_column's switch from the LDS sort to the radix select past 8192 members.  One context holds trace_craft.py's history
(groups of 8193, 8192, 513, 257, 256, 255, 1 and 0 scattered members; per iteration a pattern of accepted rows, ties of the best value
across the seam, NaN in later blocks, flags at the seams, tie columns; tests/test_trace_craft.py checks that design without a GPU),
installed with smm_set_state into a twin context and read back; every output is equal, bit for bit, to trace_ref.py over the read-back
history: three selections, strides 1 and 4, with and without the moments, and the same with one kept iteration and one series per
batch (SMMHIP_STATS_SCRATCH=1)."""
import numpy as np
import pytest

import common as cm
import trace_craft as TC
import trace_ref as TR
from test_gpu_reducer_caps import crafted_twin, seamed

pytestmark = pytest.mark.gpu

CALLS = [(sel, stride, mo) for sel in ("all", "accepted", "state") for stride in (1, 4) for mo in (True, False)]


@pytest.fixture(scope="module")
def seams(S):
    prob, opts = cm.serial_normal(N=TC.N, T=TC.T, ns=10)
    h, state, crafted, back = crafted_twin(S, prob, opts, TC.T, TC.crafted)
    assert np.array_equal(back.exchanged, crafted.exchanged) and np.array_equal(back.status, crafted.status)
    want = {}

    def ref(sel, stride, mo):
        if (sel, stride, mo) not in want:
            want[sel, stride, mo] = TR.trace_from_history(back, 0, TC.T, stride, sel, mo, TC.GROUPS, TC.PROBS, n_groups=TC.N_GROUPS)
        return want[sel, stride, mo]
    return dict(h=h, state=state, crafted=crafted, back=back, ref=ref, prob=prob, opts=opts)


def trace(h, sel, stride, mo):
    return h.trace(0, TC.T, stride, sel, mo, TC.GROUPS, TC.PROBS, n_groups=TC.N_GROUPS)


@pytest.mark.parametrize("sel,stride,mo", CALLS)
def test_member_block_seams(seams, sel, stride, mo):
    got, want = trace(seams["h"], sel, stride, mo), seams["ref"](sel, stride, mo)
    TR.assert_trace_equal(got, want)
    assert got["n_chains"].tolist() == list(TC.SIZES) and got["iter"].tolist() == list(range(0, TC.T, stride))
    for i, t in enumerate(got["iter"]):                    # the best member where trace_craft's table puts it
        for g, mem in enumerate(TC.MEMBERS):
            p = TC.best_position(t, len(mem))
            if p is not None:
                assert got["best_chain"][i, g] == (mem[p] + 1 if p >= 0 else 0), (t, g)
    if sel == "accepted":
        assert (got["count"][0] == 0).all() and np.isnan(got["mean"][0]).all()


def test_one_kept_iteration_and_one_series_per_batch(S, seams, hooks, monkeypatch):
    h = seamed(S, monkeypatch, seams["prob"], seams["opts"], seams["state"], seams["crafted"], STATS_SCRATCH=1)
    for sel, stride, mo in CALLS:
        TR.assert_trace_equal(trace(h, sel, stride, mo), seams["ref"](sel, stride, mo))
    cm.assert_history_equal(h.history(0, TC.T), seams["back"], exact_floats=True)
    cm.assert_history_equal(seams["h"].history(0, TC.T), seams["back"], exact_floats=True)
