"""smm_get_adjustment on the device at its edges (include/smmhip.h, smm.jl_amd/csrc/smm_adjust.hpp and its plan in
smm_reducers_host.hpp): every call equal bit for bit (adjust_craft.assert_adjustment_bits: the doubles through their int64 views, so
-0.0 is not +0.0) to adjust_ref.py over the history downloaded with smm_get_history of the same context, and, where the construction
gives a value, to that value.  The histories are adjust_craft.py's (functions of a seed, their designs checked without a GPU in
tests/test_adjustment_edges.py), installed with smm_set_state into a twin context and read back.

  bounds : crafted_exact at np = 3, nm = 4, two groups of 4096 rows (one chunk each) and of 16384 rows (two full chunks each): n_outside
           non-zero, unequal between parameters and groups, with values on lb and on ub, the rows outside spread over the waves and
           workgroups of k_adjust_apply; in the shipped plan (every parameter at once), with the parameters one and two at a time
           (lb[j0 + jj]), with n_outside the only output and with the quantiles but no n_outside.
  select : crafted_keys at np = 2: keys of both signs, signed zeros, subnormals, pairs that part at each of the six digits, a tie run
           of unequal weights with targets inside it, on its last unit of weight and one past it, q = 1 and q = 2^20; the bandwidth on
           a run of equal distances (n_kept of the two kernels apart by the run), at 1.0 and at 0.0.  In the shipped library (a column inside one
           workgroup of k_adjust_hist), with one row per workgroup (SMMHIP_GROUP_WIDE_MIN = 1: a key's weights added across workgroups
           in global memory) and with every chain a group of its own (more columns than the histograms hold at a time).
  seams  : crafted_seams, 41,025 pooled rows in groups of three chunks, two chunks, one chunk and one row, no row and 256 rows: batches
           of three, two and one chunk (k_adjust_sum_acc and k_moment_cov_acc clamping a group's chunks against the batch's), a batch
           that holds the tail of one group and the head of the next, a group spread over several batches."""
import numpy as np
import pytest

import adjust_craft as AC
import adjust_ref as AR
import common as cm
import test_gpu_adjustment as TA
import test_gpu_reducer_caps as RC

pytestmark = pytest.mark.gpu

GROUP_HIST_CAP, GROUP_BINS = 32 << 20, 2048              # smm_group.hpp


def reference(back, prob, t0, t1, select, groups, tol, kernel, ridge, probs, n_groups=None):
    return AR.adjustment_from_history(back, t0, t1, select, groups, tol, kernel, None, ridge, probs, prob.mom, prob.w, prob.lb, prob.ub,
                                      n_groups=n_groups)


# --- bounds: crafted_exact ---------------------------------------------------------------------------------------------------------

BT = 512                                                   # iterations held; the capacity 4 BT leaves the scratch room for every parameter


@pytest.fixture(scope="module", params=(16, 64), ids=("m4096", "m16384"))
def bounds(S, request):
    """the unseamed twin holding crafted_exact's history of N chains (two groups of N BT / 2 rows), and the restatement's result"""
    N = request.param
    prob, opts = AC.exact_problem(N, 4 * BT)
    made = {}

    def craft(c):
        made["info"] = AC.crafted_exact(N, BT, 5, into=c)[1]
        return c
    h, state, crafted, back = RC.crafted_twin(S, prob, opts, BT, craft)
    info = made["info"]
    want = {select: reference(back, prob, 0, BT, select, info["groups"], 1.0, 0, 0.0, AC.EXACT_PROBS) for select in (0, 2)}
    m = info["m"]
    return dict(N=N, h=h, state=state, crafted=crafted, back=back, prob=prob, opts=opts, info=info, want=want, m=m,
                NC=2 * (m // AC.LDS_N if m > AC.LDS_N else 1))


def bounds_plan(b, cap=0):
    return AC.adjust_plan(b["N"], 4 * BT, AC.EXACT_NP, AC.EXACT_NM, 2 * b["m"], b["NC"], cap)


def check_bounds(b, h):
    """the full call on h for two selections: the restatement bit for bit, and the construction's beta, counts, intercepts, quantiles"""
    info = b["info"]
    for select in (0, 2):
        got = h.adjustment(0, BT, select, info["groups"], 1.0, 0, None, 0.0, AC.EXACT_PROBS)
        assert np.array_equal(got["n_outside"], info["n_outside"]), (select, got["n_outside"].tolist(), info["n_outside"].tolist())
        assert (got["n_outside"].sum(axis=0) > 0).all()
        AC.assert_adjustment_bits(got, b["want"][select])
        AC.assert_adjustment_bits(got, dict(beta=info["beta"], adj_mean=info["adj_mean"], adj_quantile=info["quantile"]),
                                  ("beta", "adj_mean", "adj_quantile"))
        assert got["status"].tolist() == [0, 0] and got["n_kept"].tolist() == [b["m"]] * 2


def check_bounds_subsets(S, b, h):
    """n_outside as the only output (the adjust pass without a select), and the quantiles without n_outside"""
    A, info = S._abi, b["info"]
    for keep in (("n_outside",), ("adj_quantile",), ("adj_quantile", "n_outside", "status")):
        a = TA.sentinel(2, AC.EXACT_NP, AC.EXACT_NM, len(AC.EXACT_PROBS))
        drop = [f for f in AR.FIELDS if f not in keep]
        assert TA.raw(h, A, a, 0, BT, 0, info["groups"], 2, 1.0, 0, None, 0.0, AC.EXACT_PROBS, skip=drop) == A.SMM_OK
        AC.assert_adjustment_bits(a, b["want"][0], keep)
        assert TA.untouched(a, drop), keep
        if "n_outside" in keep:
            assert np.array_equal(a["n_outside"], info["n_outside"])
        if "adj_quantile" in keep:
            AC.assert_adjustment_bits(a, dict(adj_quantile=info["quantile"]), ("adj_quantile",))


def test_bounds_in_the_shipped_plan(S, bounds):
    b = bounds
    Nbc, jb = bounds_plan(b)
    assert jb == AC.EXACT_NP and Nbc == (1 if b["m"] == 4096 else 2) and b["NC"] == (2 if b["m"] == 4096 else 4)
    for g in range(2):                                     # the rows outside lie in two waves of one workgroup and in two workgroups
        for rows in b["info"]["outside_rows"][g]:
            if len(rows):
                at = rows % AC.LDS_N                       # (the row within its chunk: what k_adjust_apply's lanes index)
                wg, wave = at // AC.ADJ_WG, at // 64
                assert len(set(wg.tolist())) >= 2 and len(set(wave[wg == wg[0]].tolist())) >= 2
    check_bounds(b, b["h"])
    check_bounds_subsets(S, b, b["h"])
    cm.assert_history_equal(b["h"].history(0, BT), b["back"], exact_floats=True)


@pytest.mark.parametrize("jb", (1, 2))
def test_bounds_with_the_parameters_in_batches(S, bounds, hooks, monkeypatch, jb):
    b = bounds
    D = AC.EXACT_NP + AC.EXACT_NM
    col8, chunk8 = 2 * b["m"] * 8, (D + 2) * AC.LDS_N * 8
    cap = 4096 if jb == 1 else 2 * col8 + chunk8 + col8   # the least scratch, and one packed column more
    assert bounds_plan(b, cap) == (1, jb) and 1 <= jb < AC.EXACT_NP and b["NC"] > 1     # the chunks one at a time as well
    h = RC.seamed(S, monkeypatch, b["prob"], b["opts"], b["state"], b["crafted"], STATS_SCRATCH=cap)
    check_bounds(b, h)
    check_bounds_subsets(S, b, h)
    cm.assert_history_equal(h.history(0, BT), b["back"], exact_floats=True)


# --- select: crafted_keys ----------------------------------------------------------------------------------------------------------

KN = 64
KG = np.full(KN, -1, np.int32)
KG[0:6], KG[6:9], KG[9] = 0, 1, 2                          # pools of 1200, 600 and 200 rows; the other chains in no group
KMEMBERS = ([0, 1, 2, 3, 4, 5], [6, 7, 8], [9])
KCAP = 4 * AC.KEYS_T                                       # the capacity: the scratch has room for both adjusted parameters at once


def keys_problem():
    return cm.serial_normal(N=KN, T=KCAP, ns=100, acc_tuners=1.0, seed=1)


def keys_plan(groups):
    """(Nbc, jb) of a call on a context of keys_problem with the chains grouped by `groups` (no seam on the scratch)"""
    counts = np.bincount(groups[groups >= 0]) * AC.KEYS_T
    return AC.adjust_plan(KN, KCAP, 2, 2, int(counts.sum()), int(AC.chunk_starts(counts)[-1]))


@pytest.fixture(scope="module")
def keys(S):
    prob, opts = keys_problem()
    assert prob.mom.tolist() == list(AC.KEYS_MOM) and prob.w.tolist() == [1.0, 1.0]
    assert np.array_equal(prob.lb, AC.KEYS_LB) and np.array_equal(prob.ub, AC.KEYS_UB)
    made = {}

    def craft(c):
        made["info"] = AC.crafted_keys(KN, 9, into=c)[1]
        return c
    h, state, crafted, back = RC.crafted_twin(S, prob, opts, AC.KEYS_T, craft)
    info = made["info"]
    probs, want_q, marks = AC.keys_probs(info, KMEMBERS[0])
    assert len(probs) >= 7
    want = {k: reference(back, prob, 0, AC.KEYS_T, 0, KG, AC.KEYS_TOL, k, AC.KEYS_RIDGE, probs) for k in (0, 1)}
    return dict(h=h, state=state, crafted=crafted, back=back, prob=prob, opts=opts, info=info, probs=probs, want_q=want_q, want=want)


def check_keys(k, h):
    """both kernels on h: the restatement bit for bit; the construction's bandwidth, n_kept of both kernels, and under Epanechnikov's
    kernel the counts outside and the first group's quantiles"""
    info, out = k["info"], {}
    assert keys_plan(KG) == (1, 2)                         # the three pools' chunks one at a time, both parameters' columns in one select
    for kernel in (0, 1):
        got = out[kernel] = h.adjustment(0, AC.KEYS_T, 0, KG, AC.KEYS_TOL, kernel, None, AC.KEYS_RIDGE, k["probs"])
        AC.assert_adjustment_bits(got, k["want"][kernel])
        assert got["status"].tolist() == [0, 0, 0]
        for g, members in enumerate(KMEMBERS):
            exp = AC.keys_expect(info, members)
            assert got["n_kept"][g] == exp["n_kept"][kernel] and AC.bits(got["bandwidth"][g]) == AC.bits(exp["bandwidth"])
            if kernel == 1:
                assert np.array_equal(got["n_outside"][g], exp["n_outside"]) and got["n_outside"][g, 0] == len(members)
    assert ((out[0]["n_kept"] - out[1]["n_kept"]) == [AC.KEYS_RUN * len(m) for m in KMEMBERS]).all()
    AC.assert_adjustment_bits(dict(adj_quantile=np.ascontiguousarray(out[1]["adj_quantile"][:, 0])), dict(adj_quantile=k["want_q"]))
    return out


def test_select_in_the_shipped_library(keys):
    """every pool shorter than a block of 4096 rows: each column inside one workgroup of k_adjust_hist"""
    assert max(len(m) for m in KMEMBERS) * AC.KEYS_T < 4096
    check_keys(keys, keys["h"])
    cm.assert_history_equal(keys["h"].history(0, AC.KEYS_T), keys["back"], exact_floats=True)


def test_select_with_one_row_per_workgroup(S, keys, hooks, monkeypatch):
    """SMMHIP_GROUP_WIDE_MIN = 1: per = 1, so the 1200 rows of the first pool go round 1024 workgroups and the unequal weights of one
    key meet in global memory; the bandwidth comes from the grid-wide select as well"""
    h = RC.seamed(S, monkeypatch, keys["prob"], keys["opts"], keys["state"], keys["crafted"], GROUP_WIDE_MIN=1)
    wide, own = check_keys(keys, h), check_keys(keys, keys["h"])
    for kernel in (0, 1):
        AC.assert_adjustment_bits(wide[kernel], own[kernel])
    cm.assert_history_equal(h.history(0, AC.KEYS_T), keys["back"], exact_floats=True)


def test_a_bandwidth_of_zero_on_the_rows_at_the_data(keys):
    """tol = KEYS_TOL_ZERO: the bandwidth is the distance 0.0 of the run of rows on the data.  Epanechnikov's kernel keeps none of them,
    at weights of 0.0 (d2 < delta2 fails before 0 / 0 is formed): status 3 with sum_w 0.0; the uniform kernel keeps the run alone,
    whose discrepancies are all zero: status 4"""
    h, info = keys["h"], keys["info"]
    zeros = [len(m) * len(AC.KEYS_ON_DATA) for m in KMEMBERS]
    for kernel in (0, 1):
        got = h.adjustment(0, AC.KEYS_T, 0, KG, AC.KEYS_TOL_ZERO, kernel, None, AC.KEYS_RIDGE, keys["probs"])
        AC.assert_adjustment_bits(got, reference(keys["back"], keys["prob"], 0, AC.KEYS_T, 0, KG, AC.KEYS_TOL_ZERO, kernel, AC.KEYS_RIDGE,
                                                 keys["probs"]))
        assert got["status"].tolist() == [3 + (kernel == 0)] * 3 and got["n_kept"].tolist() == ([0] * 3 if kernel else zeros)
        for g in range(3):
            assert AC.bits(got["bandwidth"][g]) == AC.bits(0.0) and AC.bits(got["sum_w"][g]) == AC.bits(float(0 if kernel else zeros[g]))
        assert np.isnan(got["adj_quantile"]).all() and (got["n_outside"] == 0).all()


def test_select_with_every_chain_a_group_of_its_own(keys):
    """64 groups x 2 parameters = 128 columns at R probs in one select: more than the histograms hold at a time, on these keys"""
    info, h = keys["info"], keys["h"]
    probs, want_q, _ = AC.keys_probs(info, [0])
    R = len(probs)
    g = np.arange(KN, dtype=np.int32)
    Nbc, jb = keys_plan(g)
    WB = max(1, GROUP_HIST_CAP // (R * GROUP_BINS * 8))
    assert (Nbc, jb) == (1, 2) and WB < KN * jb            # radix_digits takes the 128 columns in two batches of histograms
    assert R >= 7 and (R + 2) // 3 >= 3                    # three slices of probs or more
    for kernel in (0, 1):
        got = h.adjustment(0, AC.KEYS_T, 0, g, AC.KEYS_TOL, kernel, None, AC.KEYS_RIDGE, probs)
        AC.assert_adjustment_bits(got, reference(keys["back"], keys["prob"], 0, AC.KEYS_T, 0, g, AC.KEYS_TOL, kernel, AC.KEYS_RIDGE, probs))
        exp = AC.keys_expect(info, [0])
        assert got["status"].tolist() == [0] * KN and got["n_kept"].tolist() == [exp["n_kept"][kernel]] * KN
        assert (got["bandwidth"] == AC.KEYS_DELTA2).all()
        if kernel == 1:
            assert got["n_outside"].tolist() == [[1, 0]] * KN
            AC.assert_adjustment_bits(dict(adj_quantile=np.ascontiguousarray(got["adj_quantile"][:, 0])), dict(adj_quantile=want_q))


# --- seams: crafted_seams ----------------------------------------------------------------------------------------------------------

ST, SCAP = AC.SEAM_T, 4 * AC.SEAM_T                       # iterations held and the capacity: the scratch has room for three chunks
SG = len(AC.SEAM_ROWS)
SCALLS = tuple((select, kernel) for select in (1, 2) for kernel in (0, 1))
SPROBS = (0.025, 0.5, 0.975)


def seam_rows(select):
    return AC.SEAM_ROWS if select == 1 else tuple(n * ST for n in AC.SEAM_CHAINS)


def seam_plan(select, cap=0):
    rows = seam_rows(select)
    return AC.adjust_plan(AC.SEAM_N, SCAP, 2, 2, sum(rows), int(AC.chunk_starts(rows)[-1]), cap)


@pytest.fixture(scope="module")
def seams(S):
    prob, opts = cm.serial_normal(N=AC.SEAM_N, T=SCAP, ns=100, acc_tuners=1.0, seed=1)
    made = {}

    def craft(c):
        _, made["groups"], made["counts"] = AC.crafted_seams(3, into=c)
        return c
    h, state, crafted, back = RC.crafted_twin(S, prob, opts, ST, craft)
    g = made["groups"]
    want = {(s, k): reference(back, prob, 0, ST, s, g, 0.25, k, 0.0, SPROBS, n_groups=SG) for s, k in SCALLS}
    for s, k in SCALLS:
        assert want[s, k]["count"].tolist() == list(seam_rows(s)) and want[s, k]["status"].tolist() == [0, 0, 0, 1, 0]
        # the counts outside (random draws: held against the restatement only) are not zero in the groups that span chunks, so the
        # seamed runs add nout across batches of chunks
        assert (want[s, k]["n_outside"][:3].sum(axis=1) > 0).all(), want[s, k]["n_outside"].tolist()
    return dict(h=h, state=state, crafted=crafted, back=back, prob=prob, opts=opts, groups=g, want=want)


def check_seams(s, h):
    for select, kernel in SCALLS:
        got = h.adjustment(0, ST, select, s["groups"], 0.25, kernel, None, 0.0, SPROBS, n_groups=SG)
        AC.assert_adjustment_bits(got, s["want"][select, kernel])


def test_seams_in_the_shipped_plan(seams):
    for select in (1, 2):
        assert seam_plan(select) == (3, 2)                 # three chunks at a time: 0-2, 3-5 (two groups and the head of a third), 6-7
    check_seams(seams, seams["h"])
    cm.assert_history_equal(seams["h"].history(0, ST), seams["back"], exact_floats=True)


@pytest.mark.parametrize("Nbc", (2, 1))
def test_seams_with_the_chunks_in_batches(S, seams, hooks, monkeypatch, Nbc):
    chunk8 = (2 + 2 + 2) * AC.LDS_N * 8
    cap = 4096 if Nbc == 1 else 2 * max(sum(seam_rows(1)), sum(seam_rows(2))) * 8 + 4 * chunk8
    for select in (1, 2):
        assert seam_plan(select, cap)[0] == Nbc
        gch0 = AC.chunk_starts(seam_rows(select))
        assert gch0.tolist() == [0, 3, 5, 7, 7, 8]
        batches = [(cb0, min(cb0 + Nbc, gch0[-1])) for cb0 in range(0, gch0[-1], Nbc)]
        # a group spread over several batches; with two chunks a batch, one that holds the tail of a group and the head of the next
        assert sum(1 for lo, hi in batches if lo < gch0[1] and hi > gch0[0]) >= 2
        mixed = [(lo, hi) for lo, hi in batches if any(lo < e < hi for e in gch0[1:-1])]
        assert (len(mixed) >= 2) == (Nbc == 2), mixed
    h = RC.seamed(S, monkeypatch, seams["prob"], seams["opts"], seams["state"], seams["crafted"], STATS_SCRATCH=cap)
    check_seams(seams, h)
    cm.assert_history_equal(h.history(0, ST), seams["back"], exact_floats=True)
