"""smm_get_profile, smm_get_moment_stats and smm_get_draws on the device at their segment and size caps (include/smmhip.h;
smm.jl_amd/csrc/smm_profile.hpp, smm_moments.hpp, smm_cov.hpp, smm_draws.hpp and their plans in smm_reducers_host.hpp), every output
equal (array_equal, NaN equal to NaN; the draws bit for bit) to the restatements in profile_ref.py, moment_stats_ref.py and draws_ref.py
over the history downloaded with smm_get_history of the same context.  The histories are crafted (profile_ref.crafted_caps /
crafted_wide, moment_stats_ref.crafted_linear: functions of a seed, their design checked without a GPU in tests/test_profile.py,
tests/test_moment_stats.py and tests/test_draws.py), installed with smm_set_state into a twin context and read back.

  profile : the counters and cursors in global memory (nseg > min(4096, SMMHIP_HIST_LDS_BINS): forced through the seam at bins = 7 and
            bins2 = 3, and in the shipped library at bins2 = 65 and 256), next to the LDS form at its limits (nseg equal to the seam;
            bins = 4096; bins2 = 64); one segment past a chunk with 14 members adding to it in each of their three 256-row blocks; groups
            and axes one at a time; output subsets (the minima alone: k_prof_scatter without a list); rows of 64 parameters and 64
            moments, 4095 pairs.
  moments : (np, nm) = (1, 1), (1, 64), (64, 1), (64, 64), (63, 34), (33, 64): k_cov_pairs on D = 128 and D = 97 joint columns (17 and 13
            tile rows, the clamp of the last tile), k_moment_solve with 64 lanes and one; a group short of rows; D = 128 with kb < D and
            one chunk at a time against the call that takes all at once; output subsets.
  draws   : rows of 129 doubles, alone and in row batches (rb < R), output subsets."""
import numpy as np
import pytest

import common as cm
import draws_ref as DR
import moment_stats_ref as MR
import profile_ref as PR
import rank_diag_ref as RD
import test_gpu_draws as TD
import test_gpu_moment_stats as TM
import test_gpu_profile as TP

pytestmark = pytest.mark.gpu

PROBS = (0.025, 0.5, 0.975)
LDS_N = 8192                     # smm_stats.hpp: STATS_LDS_N, the rows of a chunk
BATCH_CAP = 256 << 20            # smm_reducers_host.hpp: REDUCER_BATCH_CAP
PROF_LDS_SEGS = 4096             # smm_profile.hpp


def crafted_twin(S, prob, opts, T, craft):
    """(h, state, crafted, back): a run of T iterations, its history overwritten by craft and installed in a twin context h, whose
    read-back equals what was written"""
    h0 = S.hip_context(prob, opts)
    h0.step(T)
    crafted, state = craft(MR.copy_history(h0.history(0, T))), h0.state()
    h = S.hip_context(prob, opts)
    h.set_state(state, crafted)
    back = h.history(0, T)
    PR.assert_crafted_read_back(back, crafted)
    return h, state, crafted, back


def seamed(S, monkeypatch, prob, opts, state, crafted, **seams):
    """a context of the test build created under the seams SMMHIP_<NAME>=value (read at creation), holding the crafted history"""
    for k, v in seams.items():
        monkeypatch.setenv("SMMHIP_" + k, str(v))
    h = S.hip_context(prob, opts)
    for k in seams:
        monkeypatch.delenv("SMMHIP_" + k)
    h.set_state(state, crafted)
    PR.assert_crafted_read_back(h.history(0, crafted.value.shape[0]), crafted)
    return h


def profile_plan(n_chains, n, npar, nm, NP, B, B2, cap, all_bytes):
    """smm_get_profile's batches under SMMHIP_STATS_SCRATCH = cap, every output asked for: [(g0, gn, mb, an1, an2)] (smm_reducers_host.hpp).
    The scratch budget is the least scratch (one axis of the largest group) where the cap is below it, else the cap, which the scratch
    of a context of all_bytes = N T (8 np + 4) or more reaches at its first allocation"""
    nseg1, nseg2 = B, B2 * B2
    nsegx = max(nseg1, nseg2)
    seg_bytes = 8 * 3 + 4 * 3 + 8 * 2 + 4 * 2 + 8 * npar + 8 * nm + (8 + 4 + 8 * (1 + nm))
    scratch_of = lambda mb, an, nseg: mb * n * 12 + an * mb * (8 * n + 4 * nseg)
    least = scratch_of(max(n_chains), 1, nsegx)
    assert cap <= least or cap <= all_bytes
    budget = max(cap, least)
    plan, g0, G = [], 0, len(n_chains)
    while g0 < G:
        gn = mb = 0
        while g0 + gn < G:
            m2 = mb + n_chains[g0 + gn]
            if gn > 0 and (scratch_of(m2, 1, nsegx) > budget or (gn + 1) * nsegx * seg_bytes > cap):
                break
            mb, gn = m2, gn + 1

        def axes(A, nseg):
            an = A
            if mb > 0:
                fixed, per = mb * n * 12, mb * (8 * n + 4 * nseg)
                an = min(an, (budget - fixed) // per if budget > fixed else 0)
            return max(1, min(an, cap // (gn * nseg * seg_bytes)))
        plan.append((g0, gn, mb, axes(npar, nseg1), axes(NP, nseg2)))
        g0 += gn
    return plan


# --- A. the profile: the global-memory form and the LDS caps ------------------------------------------------------------------------

PAIRS3 = [(0, 1), (1, 0), (1, 1)]
WINDOWS = ((0, PR.CAPS_T), (137, 590))                     # the second starts inside the run, and inside a block
CAPS_CALLS = (dict(bins=3, bins2=2), dict(bins=7, bins2=3))   # under the seam 4: LDS (3 and 2 x 2 = 4, at the limit), global (7 and 9)
SEAM = 4


def caps_problem():
    return cm.serial_normal(**dict(RD.MIXING, N=len(PR.CAPS_GROUPS), T=PR.CAPS_T, acc_tuners=1.0, seed=1))


@pytest.fixture(scope="module")
def caps(S):
    """the unseamed twin holding profile_ref.crafted_caps' history, and the restatement's results, computed once per call"""
    prob, opts = caps_problem()
    h, state, crafted, back = crafted_twin(S, prob, opts, PR.CAPS_T, PR.crafted_caps)
    want = {}

    def ref(t0, t1, select, bins, rng, bins2):
        key = (t0, t1, select, bins, rng is None, bins2)
        if key not in want:
            want[key] = PR.profile_from_history(back, t0, t1, select, PR.CAPS_GROUPS, bins, rng, PAIRS3, bins2, n_groups=PR.CAPS_NG)
        return want[key]
    return dict(h=h, state=state, crafted=crafted, back=back, ref=ref, prob=prob, opts=opts)


def caps_calls():
    for select in (0, 1, 2):
        for w, (t0, t1) in enumerate(WINDOWS):
            for kw in CAPS_CALLS:
                yield t0, t1, select, kw["bins"], (PR.CAPS_RANGE if w == 0 else None), kw["bins2"]   # the second window: its own range


def caps_profile(h, t0, t1, select, bins, rng, bins2):
    return h.profile(t0, t1, select, PR.CAPS_GROUPS, bins, rng, PAIRS3, bins2, n_groups=PR.CAPS_NG)


def check_caps(caps, h):
    """every call of caps_calls on h against the restatement, the unseamed twin and smm_get_histogram's counts"""
    for t0, t1, select, bins, rng, bins2 in caps_calls():
        got, want = caps_profile(h, t0, t1, select, bins, rng, bins2), caps["ref"](t0, t1, select, bins, rng, bins2)
        assert sorted(got) == sorted(want)
        PR.assert_profile_equal(got, want)
        if h is not caps["h"]:
            PR.assert_profile_equal(got, caps_profile(caps["h"], t0, t1, select, bins, rng, bins2))
        hs = h.histogram(t0, t1, select, PR.CAPS_GROUPS, bins, rng, PAIRS3, bins2, n_groups=PR.CAPS_NG)
        assert np.array_equal(got["n"], hs["hist"]) and np.array_equal(got["n2"], hs["hist2"]) and np.array_equal(got["count"], hs["count"])
    full = caps["ref"](0, PR.CAPS_T, 0, 7, PR.CAPS_RANGE, 3)
    assert full["n_scored"][2, 0].max() > LDS_N and full["n_scored2"][2].max() > LDS_N    # a second chunk of k_prof_chunk, 1-D and 2-D
    assert full["min_chain"][2, 0, int(np.argmax(full["n_scored"][2, 0]))] == PR.CAPS_MIN[0] + 1


def test_profile_unseamed_twin_on_the_crafted_history(caps):
    """the shipped library on the crafted history: every segment count in LDS (nseg <= 9)"""
    check_caps(caps, caps["h"])
    cm.assert_history_equal(caps["h"].history(0, PR.CAPS_T), caps["back"], exact_floats=True)


def test_profile_counters_and_cursors_in_global_memory(S, caps, hooks, monkeypatch):
    lim = min(PROF_LDS_SEGS, SEAM)
    assert 3 <= lim and 2 * 2 <= lim and 7 > lim and 3 * 3 > lim      # per call: both axes' forms in LDS (one at the limit), then both global
    h = seamed(S, monkeypatch, caps["prob"], caps["opts"], caps["state"], caps["crafted"], HIST_LDS_BINS=SEAM)
    check_caps(caps, h)
    cm.assert_history_equal(h.history(0, PR.CAPS_T), caps["back"], exact_floats=True)


def test_profile_global_form_one_group_and_one_axis_at_a_time(S, caps, hooks, monkeypatch):
    cap = 1
    h = seamed(S, monkeypatch, caps["prob"], caps["opts"], caps["state"], caps["crafted"], HIST_LDS_BINS=SEAM, STATS_SCRATCH=cap)
    n_chains = np.bincount(PR.CAPS_GROUPS[PR.CAPS_GROUPS >= 0], minlength=PR.CAPS_NG).tolist()
    for t0, t1 in WINDOWS:
        for kw in CAPS_CALLS:
            plan = profile_plan(n_chains, t1 - t0, 2, 2, len(PAIRS3), kw["bins"], kw["bins2"], cap, 0)
            assert len(plan) == PR.CAPS_NG and all(b[1] == 1 for b in plan)                    # a batch per group ...
            assert all(b[3] == 1 < 2 and b[4] == 1 < len(PAIRS3) for b in plan)                # ... and per axis: an < A
    check_caps(caps, h)
    cm.assert_history_equal(h.history(0, PR.CAPS_T), caps["back"], exact_floats=True)


def test_profile_output_subsets_in_the_global_form(S, caps, hooks, monkeypatch):
    A = S._abi
    h = seamed(S, monkeypatch, caps["prob"], caps["opts"], caps["state"], caps["crafted"], HIST_LDS_BINS=SEAM)
    t0, t1 = WINDOWS[1]
    assert 7 > min(PROF_LDS_SEGS, SEAM) and 3 * 3 > min(PROF_LDS_SEGS, SEAM)
    for select, rng in ((2, PR.CAPS_RANGE), (0, None)):
        want = PR.profile_from_history(caps["back"], t0, t1, select, PR.CAPS_GROUPS, 7, rng, PAIRS3, 3, n_groups=PR.CAPS_NG)
        for keep in (("v_min", "min_chain", "min_iter", "v_min2", "min_chain2", "min_iter2"),   # k_prof_scatter with want_list == 0
                     ("v_min", "min_chain", "min_iter"), ("min_iter2",),
                     ("v_mean", "m_mean", "v_mean2"), ("m_mean",), ("v_mean2",),               # the means only
                     ("n",), ("n_scored2",)):
            a = TP.sentinel(PR.CAPS_NG, 2, 2, 7, len(PAIRS3), 3)
            drop = [f for f in PR.FIELDS if f not in keep]
            assert TP.raw(h, A, t0, t1, select, PR.CAPS_GROUPS, PR.CAPS_NG, 7, rng, PAIRS3, 3, a, skip=drop) == A.SMM_OK, keep
            PR.assert_profile_equal(a, want, keep)
            assert TP.untouched(a, drop), keep
    cm.assert_history_equal(h.history(0, PR.CAPS_T), caps["back"], exact_floats=True)


def test_profile_shipped_library_at_the_lds_limit_and_past_it(S):
    """no seam: bins = 4096 (32 KB of counters in LDS) with bins2 = 64 (4096 cells, the last LDS size); bins2 = 65 (4225 cells, the first
    in global memory); bins2 = 256 (65,536 cells) with one pair"""
    T = 40
    prob, opts = cm.serial_normal(**dict(RD.MIXING, N=len(PR.CAPS_GROUPS), T=T, acc_tuners=1.0, seed=1))
    h, _, _, back = crafted_twin(S, prob, opts, T, PR.crafted_wide)
    assert 4096 <= PROF_LDS_SEGS and 64 * 64 <= PROF_LDS_SEGS and 65 * 65 > PROF_LDS_SEGS and 256 * 256 > PROF_LDS_SEGS
    rng = np.array([[0.0, 1.0], [0.0, 1.0]])
    for select, t0, bins, r, pairs, bins2 in ((2, 0, 4096, None, PAIRS3, 64), (1, 3, 4096, rng, [(1, 0)], 64), (0, 0, 5, rng, PAIRS3, 65),
                                              (2, 3, 5, None, PAIRS3, 65), (2, 0, 3, None, [(1, 0)], 256), (0, 3, 3, rng, [(0, 1)], 256)):
        got = TP.check(h, back, t0, T, select, PR.CAPS_GROUPS, bins, r, pairs, bins2, n_groups=PR.CAPS_NG)
        assert got["n2"].shape == (PR.CAPS_NG, len(pairs), bins2, bins2) and got["n"].shape == (PR.CAPS_NG, 2, bins)
        assert (got["n2"].sum(axis=(2, 3)) == got["count"][:, None]).all()                   # every row of x in [0, 1] has a cell
    cm.assert_history_equal(h.history(0, T), back, exact_floats=True)


# --- wide rows: np = nm = 64 (the profile's 65 columns and theta_at_min, the draws' rows of 129 doubles) -----------------------------

WN, WT = 8, 40


@pytest.fixture(scope="module")
def wide(S):
    prob, opts = MR.dense_problem(64, 64, N=WN, T=WT)
    h, state, crafted, back = crafted_twin(S, prob, opts, WT, PR.crafted_wide)
    return dict(h=h, state=state, crafted=crafted, back=back, prob=prob, opts=opts)


def test_profile_wide_rows_and_all_but_one_pair(S, wide, hooks, monkeypatch):
    h, back = wide["h"], wide["back"]
    g = (np.arange(WN) % 2).astype(np.int32)
    pairs = np.stack(np.divmod(np.random.default_rng(5).permutation(64 * 64)[:64 * 64 - 1], 64), axis=1).astype(np.int32)
    assert len(pairs) == 64 * 64 - 1 and len({(a, b) for a, b in pairs.tolist()}) == len(pairs)
    rng = np.tile([0.0, 1.0], (64, 1))
    got = TP.check(h, back, 0, WT, 2, g, 5, rng, pairs, 2, moments=True)
    assert got["m_mean"].shape == (2, 64, 5, 64) and got["theta_at_min"].shape == (2, 64, 5, 64) and got["v_mean2"].shape == (2, 4095, 2, 2)
    assert (got["n"].sum(axis=2) == 4 * WT).all() and np.isfinite(got["theta_at_min"]).all() and np.isfinite(got["m_mean"]).all()
    cap = 100000                                           # the axes in batches: smm_reducers_host.hpp's plan, recomputed
    plan = profile_plan([4, 4], WT, 64, 64, len(pairs), 5, 2, cap, WN * WT * (8 * 64 + 4))
    assert len(plan) == 1 and 1 < plan[0][3] < 64 and 1 < plan[0][4] < len(pairs), plan      # an1 < np, an2 < n_pairs
    hs = seamed(S, monkeypatch, wide["prob"], wide["opts"], wide["state"], wide["crafted"], STATS_SCRATCH=cap)
    PR.assert_profile_equal(hs.profile(0, WT, 2, g, 5, rng, pairs, 2), got)
    cm.assert_history_equal(hs.history(0, WT), back, exact_floats=True)
    cm.assert_history_equal(h.history(0, WT), back, exact_floats=True)


WG3 = np.array([0, 1, 1, -1, 2, 0, 2, 2], np.int32)      # three groups and a chain in none


def test_draws_wide_rows_alone_and_in_row_batches(S, wide, hooks, monkeypatch):
    A = S._abi
    h, back = wide["h"], wide["back"]
    cap = 5000
    row_bytes = 8 * (64 + 1 + 64) + 12                     # smm_reducers_host.hpp: a batch holds cap / row_bytes rows
    rb = max(1, cap // row_bytes)
    hs = seamed(S, monkeypatch, wide["prob"], wide["opts"], wide["state"], wide["crafted"], STATS_SCRATCH=cap)
    t0 = 3
    for select in (0, 1, 2):
        for thin, K in ((1, TD.BIG), (3, TD.BIG), (1, 50), (3, 11)):
            want = DR.draws_from_history(back, t0, WT, select, WG3, thin, K, n_groups=3)
            one = h.draws(t0, WT, select, WG3, thin, K, True, n_groups=3)
            DR.assert_draws_equal(one, want)
            DR.assert_draws_equal(hs.draws(t0, WT, select, WG3, thin, K, True, n_groups=3), one)
            R = int(want["row0"][3])
            assert one["params"].shape == (R, 64) and one["sim_moments"].shape == (R, 64) and rb < R and -(-R // rb) >= 3, (R, rb)
            assert K == TD.BIG or (want["count"] > K).any()                                    # the cap cuts a group
    want = DR.draws_from_history(back, t0, WT, 2, WG3, 3, 11, n_groups=3)
    R = int(want["row0"][3])
    for ctx in (h, hs):
        for keep in (("sim_moments",), ("params", "src_iter")):
            a = dict(count=np.full(3, -7, np.int64), n_chains=np.full(3, -7, np.int32), row0=np.full(4, -7, np.int64),
                     params=np.full((R, 64), -7.5), value=np.full(R, -7.5), sim_moments=np.full((R, 64), -7.5),
                     chain=np.full(R, -7, np.int32), iter=np.full(R, -7, np.int32), src_iter=np.full(R, -7, np.int32))
            drop = [f for f in DR.FIELDS if f not in keep]
            assert TD.raw(ctx, A, t0, WT, 2, WG3, 3, 3, 11, R, a, skip=drop) == A.SMM_OK
            DR.assert_draws_equal(a, want, keep)
            assert all((a[f] == (-7.5 if a[f].dtype.kind == "f" else -7)).all() for f in drop), keep
    cm.assert_history_equal(hs.history(0, WT), back, exact_floats=True)
    cm.assert_history_equal(h.history(0, WT), back, exact_floats=True)


# --- B. moment stats across (np, nm) up to the cap -----------------------------------------------------------------------------------

LN, LT = 8, 48
LG = (np.arange(LN) % 2).astype(np.int32)


@pytest.fixture(scope="module")
def linear(S):
    """shape -> (h, prob, back): the twin holding crafted_linear's history of the shape, made on first use"""
    made = {}

    def get(npar, nm):
        if (npar, nm) not in made:
            prob, opts = MR.dense_problem(npar, nm, N=LN, T=LT)
            h, _, _, back = crafted_twin(S, prob, opts, LT, lambda c: MR.crafted_linear(npar, nm, LN, LT, npar * 100 + nm, into=c)[0])
            made[npar, nm] = h, prob, back
        return made[npar, nm]
    return get


@pytest.mark.parametrize("npar,nm", MR.CAP_SHAPES)
def test_moment_stats_across_shapes_up_to_the_cap(linear, npar, nm):
    h, prob, back = linear(npar, nm)
    for select in (0, 1, 2):
        for ridge in (0.0, 1e-8):
            got = TM.check(h, prob, back, 0, LT, select, LG, PROBS, ridge)
            want_st = MR.moment_stats_from_history(back, 0, LT, select, LG, (), ridge, prob.mom, prob.w)["status"]
            print("np %d nm %d select %d ridge %g: status %s" % (npar, nm, select, ridge, got["status"].tolist()))
            assert got["status"].tolist() == want_st.tolist()
            assert got["cov_pm"].shape == (2, npar, nm) and got["jac"].shape == (2, nm, npar) and got["sens"].shape == (2, npar, nm)
            for g in range(2):
                if got["status"][g] == 0:
                    assert np.isfinite(got["jac"][g]).all() and np.isfinite(got["sens"][g]).all() and np.isfinite(got["se"][g]).all()
        if select < 2:                                     # the cov_pp block is smm_get_group_stats' covariance, bit for bit
            gs = h.group_stats(0, LT, bool(select), LG, ())
            assert np.array_equal(got["cov_pp"], gs["cov"], equal_nan=True) and np.array_equal(got["p_mean"], gs["mean"], equal_nan=True)
    all_rows = h.moment_stats(0, LT, 0, LG, (), 0.0)
    assert all_rows["count"].tolist() == [4 * LT, 4 * LT] and 4 * LT > npar + 1
    if nm >= npar:                                         # the statuses by design (tests/test_moment_stats.py, on the restatement)
        assert all_rows["status"].tolist() == [0, 0]
    cm.assert_history_equal(h.history(0, LT), back, exact_floats=True)


def test_moment_stats_a_group_short_of_rows_and_output_subsets_at_64_by_64(S, linear):
    A = S._abi
    h, prob, back = linear(64, 64)
    g3 = np.array([0, 1, 0, 1, 0, 1, 0, 2], np.int32)     # group 2: one member over 40 rows, fewer than np + 1
    for select in (0, 2):
        got = TM.check(h, prob, back, 5, 45, select, g3, PROBS)
        assert got["count"].tolist() == [160, 120, 40]
        print("select %d: status %s" % (select, got["status"].tolist()))
    got = TM.check(h, prob, back, 5, 45, 0, g3, PROBS)
    want = MR.moment_stats_from_history(back, 5, 45, 0, g3, PROBS, 0.0, prob.mom, prob.w)
    assert got["status"].tolist() == want["status"].tolist() and got["status"][2] == 3      # (3 on the restatement: test_moment_stats.py)
    assert np.isnan(got["jac"][2]).all() and np.isnan(got["sens"][2]).all() and np.isnan(got["se"][2]).all()
    assert np.isfinite(got["cov_pp"][2]).all() and np.isfinite(got["fit_z"][2]).all() and np.isfinite(got["m_quantile"][:, 2]).all()
    want = MR.moment_stats_from_history(back, 0, LT, 2, LG, PROBS, 1e-8, prob.mom, prob.w)
    for keep in (("se",), ("jac", "status"), ("cov_pm",), ("m_quantile", "fit_z")):
        a = TM.sentinel(2, 64, 64, 3)
        drop = [f for f in MR.FIELDS if f not in keep]
        assert TM.raw(h, A, 0, LT, 2, LG, 2, PROBS, 1e-8, a, skip=drop) == A.SMM_OK
        MR.assert_moment_stats_equal(a, want, keep)
        assert TM.untouched(a, drop), keep
    cm.assert_history_equal(h.history(0, LT), back, exact_floats=True)


def test_moment_stats_128_joint_columns_in_batches_of_columns_and_chunks(S, hooks, monkeypatch):
    N, T, Tcap, D = 24, 400, 1400, 128
    prob, opts = MR.dense_problem(64, 64, N=N, T=Tcap)    # a capacity whose scratch holds every joint column and both chunks at once
    opts.sigma = 0.02 * opts.sigma                         # (short steps: 400 iterations of 24 chains stay inside the 64 bounds)
    h0, state, crafted, back = crafted_twin(S, prob, opts, T, lambda c: MR.crafted_linear(64, 64, N, T, 7, into=c)[0])
    Mtot, NC = N * T, 2                                    # 9600 pooled rows: 8192 + 1408
    assert Mtot > LDS_N
    # smm_reducers_host.hpp's plan: the scratch is the capped chain-stats scratch, but never less than one chunk of every joint column
    scr0 = max(min(N * Tcap * (8 * 64 + 4), BATCH_CAP), N * Tcap * 8, D * LDS_N * 8)
    kb0, Nbc0 = min(D, scr0 // (Mtot * 8)), max(1, min(NC, scr0 // (D * LDS_N * 8), BATCH_CAP // (D * D * 8)))
    assert kb0 == D and Nbc0 == NC                         # the twin takes every column and both chunks at once
    cap = 4096
    scr = max(min(N * Tcap * (8 * 64 + 4), max(cap, 12 * Tcap)), N * Tcap * 8, D * LDS_N * 8)
    budget = min(scr, max(cap, Mtot * 8, D * LDS_N * 8))
    kb, Nbc = min(D, budget // (Mtot * 8)), max(1, min(NC, budget // (D * LDS_N * 8), cap // (D * D * 8)))
    assert kb < D and Nbc == 1 and NC > 1                  # two batches of columns, and the two chunks one at a time
    want = TM.check(h0, prob, back, 0, T, 0, None, (0.5,))
    assert want["count"].tolist() == [Mtot] and want["status"].tolist() == [0] and np.isfinite(want["se"]).all()
    h = seamed(S, monkeypatch, prob, opts, state, crafted, STATS_SCRATCH=cap)
    MR.assert_moment_stats_equal(h.moment_stats(0, T, 0, None, (0.5,)), want)
    cm.assert_history_equal(h.history(0, T), back, exact_floats=True)
    cm.assert_history_equal(h0.history(0, T), back, exact_floats=True)
