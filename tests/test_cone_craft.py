"""The crafted pair tables of tests/cone_craft.py have the depths and widths tests/test_gpu_cone_walk.py says they have: held against
the plain restatement of levels and cones (no device)."""
import numpy as np
import pytest

import cone_craft as CC

CLAIMS = CC.claims()


@pytest.mark.parametrize("name", sorted(CLAIMS))
def test_crafted_table_has_the_claimed_cones(name):
    tab, N, ct, want, fits = CLAIMS[name]
    CC.check_table(tab, N)
    assert (tab == tab[0]).all()
    got = CC.cones(tab[0], N, ct)
    assert len(got) == -(-N // ct)
    for tile, (nsub, widths, gathered) in want.items():
        assert got[tile]["nsub"] == nsub, (name, tile, got[tile])
        if widths is not None:
            assert got[tile]["widths"] == widths, (name, tile, got[tile])
        if gathered is not None:
            assert got[tile]["gathered"] == gathered, (name, tile, got[tile])
    # every cone meant to stay in the persistent form fits its caps; the one table meant to leave it does not
    assert all(c["fits"] for c in got) == fits, (name, [c["nsub"] for c in got])
    if fits:
        assert max(c["nsub"] for c in got) <= CC.CONE_LEVELS and max(c["gathered"] for c in got) <= CC.CONE_GCAP
    assert any(c["nsub"] > 0 for c in got)
    # an injected list deeper than LV_MAXLEV = 31 levels is kept off the persistent forms at creation (smm_create_host.hpp: deep_plan):
    # only the two chains of 32 and 33 pairs are that deep — the cap of 32 sub-levels, and 33, are reached through a wide level instead
    assert (max(CC.levels(tab[0])[0]) > CC.LV_MAXLEV) == (name in ("chain32", "chain33")), name


def test_restatement_on_a_list_worked_by_hand():
    # (0,1) (2,3) | (1,2) | (0,1)' is not allowed twice, so (0,2): 0's previous pair is level 1, 2's is level 2 -> level 3
    pairs = [(0, 1), (2, 3), (1, 2), (0, 2), (4, 5)]
    lev, pred, last = CC.levels(pairs)
    assert lev == [1, 1, 2, 3, 1]
    assert pred == [(-1, -1), (-1, -1), (0, 1), (0, 2), (-1, -1)]
    got = CC.cones(pairs, 6, 2)
    assert [c["widths"] for c in got] == [[2, 1, 1], [2, 1, 1], [1]]
    assert [c["gathered"] for c in got] == [2, 2, 0]
    # 65 disjoint pairs that all end in tile 0 through one later pair each would be 2 sub-levels: ceil(65 / 64)
    wide = [(2 * k + 200, 2 * k + 201) for k in range(65)]
    c = CC.cones(wide, 400, 400)[0]
    assert c["widths"] == [65] and c["nsub"] == 2


def test_filler_rounds_are_disjoint_and_distinct():
    p = CC.filler(range(16, 80), 79)
    assert len(set(p)) == 79
    lev, _, _ = CC.levels(p)
    assert max(lev) == 3 and lev[:32] == [1] * 32 and lev[32:64] == [2] * 32
    assert np.asarray(p).min() == 16
