"""tests/moment_stats_ref.py, the restatement of smm_get_moment_stats' contract (include/smmhip.h) the GPU tests hold the device against,
held on histories of the CPU oracle against group_stats_ref (the cov_pp block, bit for bit), a direct covariance of one parameter and
one moment (np != nm: a transposed index cannot pass), the weights' reading, the status table, and np.linalg.lstsq / np.linalg.solve
for jac, sens and se, at the earlier small shapes and on moment_stats_ref.crafted_linear's histories of the shapes at the size cap (np, nm up
to 64: the statuses by design, J_true as a second anchor, linear_part_columns equal to linear_part bit for bit); and the ctypes mirror of
smm_moment_stats_t against the header compiled with gcc.  No GPU."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import common as cm
import group_stats_ref as GS
import moment_stats_ref as MR
import rank_diag_ref as RD
from smm_jl_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBS = (0.025, 0.5, 0.975)


@pytest.fixture(scope="module")
def mixing(O):
    """a mixing population (rank_diag_ref.MIXING): Cov(theta, theta) is well conditioned"""
    prob, opts = cm.serial_normal(**dict(RD.MIXING, N=24, T=60, acc_tuners=0.5, seed=4))
    o = O.OracleContext(prob, opts)
    o.step(60)
    return prob, o.history(0, 60)


@pytest.fixture(scope="module")
def dense57(O):
    prob, opts = MR.dense_problem(5, 7, N=16, T=64)
    o = O.OracleContext(prob, opts)
    o.step(64)
    return prob, o.history(0, 64)


GROUPS = np.array([0, 0, 1, 1, 1, -1, 0, 0, 3, 3, 1, 1, 0, 3, 3, 3, 1, 0, -1, 3, 0, 1, 3, 0], np.int32)   # group 2 has no member


def ref(case, t0, t1, select, groups, probs=PROBS, ridge=0.0, w=None, n_groups=None):
    prob, h = case
    return MR.moment_stats_from_history(h, t0, t1, select, groups, probs, ridge, prob.mom, prob.w if w is None else w, n_groups=n_groups)


def test_cov_pp_is_group_stats_cov_and_the_blocks_mirror(mixing, dense57):
    for case, groups, ng in ((mixing, GROUPS, 4), (dense57, (np.arange(16) % 2).astype(np.int32), 2)):
        h = case[1]
        T = h.value.shape[0]
        for t0, t1 in ((0, T), (5, T - 9)):
            r = ref(case, t0, t1, 1, groups, n_groups=ng)
            want = GS.group_stats_from_history(h, t0, t1, True, groups, PROBS, n_groups=ng)
            assert np.array_equal(r["cov_pp"], want["cov"], equal_nan=True) and np.array_equal(r["p_mean"], want["mean"], equal_nan=True)
            assert np.array_equal(r["count"], want["count"]) and np.array_equal(r["n_chains"], want["n_chains"])
            for sel in (0, 1, 2):
                r = ref(case, t0, t1, sel, groups, n_groups=ng)
                assert np.array_equal(r["cov_pp"], np.swapaxes(r["cov_pp"], 1, 2), equal_nan=True)
                assert np.array_equal(r["cov_mm"], np.swapaxes(r["cov_mm"], 1, 2), equal_nan=True)
                cols = MR.joint_columns(h, t0, t1, sel, groups, ng)
                npar = h.params.shape[1]
                for g in range(ng):                           # cov_pm is the lower-left block of the joint covariance, transposed
                    if r["count"][g] >= 2:
                        full = GS.column_cov(cols[g])[1]
                        assert np.array_equal(r["cov_pm"][g], full[npar:, :npar].T) and np.array_equal(r["cov_pm"][g], full[:npar, npar:])


def test_shapes_and_orientation_with_np_5_and_nm_7(dense57):
    prob, h = dense57
    groups = (np.arange(16) % 2).astype(np.int32)
    r = ref(dense57, 0, 64, 2, groups)
    assert r["p_mean"].shape == (2, 5) and r["m_mean"].shape == r["m_median"].shape == r["fit_z"].shape == (2, 7)
    assert r["m_quantile"].shape == (3, 2, 7) and r["cov_pp"].shape == (2, 5, 5) and r["cov_pm"].shape == (2, 5, 7)
    assert r["cov_mm"].shape == (2, 7, 7) and r["jac"].shape == (2, 7, 5) and r["sens"].shape == (2, 5, 7) and r["se"].shape == (2, 5)
    assert (r["status"] == 0).all(), r["status"]
    cols = MR.joint_columns(h, 0, 64, 2, groups, 2)
    for g in range(2):
        x = cols[g]
        for j, k in ((0, 6), (4, 0), (2, 3)):                 # parameter j against moment k, by numpy
            c = np.cov(x[j], x[5 + k])[0, 1]
            assert r["cov_pm"][g, j, k] == pytest.approx(c, rel=1e-10)
        assert r["m_mean"][g] == pytest.approx(x[5:].mean(axis=1), rel=1e-12)
        assert r["m_median"][g] == pytest.approx(np.median(x[5:], axis=1), rel=1e-12)
        assert r["m_quantile"][:, g] == pytest.approx(np.quantile(x[5:], PROBS, axis=1), rel=1e-12)
        assert r["fit_z"][g] == pytest.approx((x[5:].mean(axis=1) - prob.mom) / x[5:].std(axis=1, ddof=1), rel=1e-9)


def test_nan_and_zero_weights_count_as_one(mixing):
    a = ref(mixing, 0, 60, 2, GROUPS, w=[np.nan, 0.0], n_groups=4)
    b = ref(mixing, 0, 60, 2, GROUPS, w=[1.0, 1.0], n_groups=4)
    c = ref(mixing, 0, 60, 2, GROUPS, w=[2.0, np.inf], n_groups=4)
    MR.assert_moment_stats_equal(a, b)
    assert np.array_equal(MR.weights([np.nan, 0.0, -0.0, np.inf, -2.0, 3.0])[0], [1.0, 1.0, 1.0, 1.0, -2.0, 3.0])
    assert (c["status"][[0, 1, 3]] == 0).all() and not np.array_equal(c["se"], b["se"], equal_nan=True)
    assert np.array_equal(c["jac"], b["jac"], equal_nan=True)               # the Jacobian does not read the weights


def test_status_cases(mixing, dense57, O):
    prob, h = mixing
    # 1: fewer than two rows — a group without a member, and one chain over one iteration
    one = np.full(24, -1, np.int32)
    one[7] = 1
    r = ref(mixing, 10, 11, 0, one, n_groups=2)
    assert r["status"].tolist() == [1, 1] and r["count"].tolist() == [0, 1]
    assert np.isnan(r["p_mean"][0]).all() and np.isfinite(r["p_mean"][1]).all() and np.isfinite(r["m_median"][1]).all()
    for f in ("cov_pp", "cov_pm", "cov_mm", "fit_z", "jac", "sens", "se"):
        assert np.isnan(r[f]).all(), f
    # 2: an injected NaN moment
    h2 = MR.copy_history(h)
    h2.sim_moments[20, 1, 3] = np.nan                          # chain 3 is in group 1
    r = MR.moment_stats_from_history(h2, 0, 60, 0, GROUPS, PROBS, 0.0, prob.mom, prob.w, n_groups=4)
    assert r["status"].tolist() == [0, 2, 1, 0] and r["count"][1] == 60 * 7
    for f in MR.FIELDS[3:]:
        assert np.isnan(r[f][..., 1, :] if f == "m_quantile" else r[f][1]).all(), f
        assert np.isfinite(r[f][..., 0, :] if f == "m_quantile" else r[f][0]).all(), f
    # 3: a group whose state series never moves in the window
    h3 = MR.copy_history(h)
    mem = np.flatnonzero(GROUPS == 3)
    h3.accepted[30:, mem] = 0
    h3.params[:, 0, mem], h3.params[:, 1, mem] = 0.5, -0.25    # ... and every member holds the same state, whose mean is exact
    r = MR.moment_stats_from_history(h3, 35, 60, 2, GROUPS, PROBS, 0.0, prob.mom, prob.w, n_groups=4)
    assert r["status"].tolist() == [0, 0, 1, 3]
    assert (r["cov_pp"][3] == 0).all() and np.isfinite(r["m_mean"][3]).all() and np.isnan(r["jac"][3]).all() and np.isnan(r["se"][3]).all()
    # 4: nm < np, J'WJ is rank-deficient.  In exact arithmetic np - nm pivots are zero; rounded, each is a tiny number of either sign,
    # so the more of them the surer the status: np = 5, nm = 3 over the whole run, where the oracle's history gives 4
    p53, o53 = MR.dense_problem(5, 3, N=8, T=64)
    o = O.OracleContext(p53, o53)
    o.step(64)
    r = MR.moment_stats_from_history(o.history(0, 64), 0, 64, 0, None, PROBS, 0.0, p53.mom, p53.w)
    assert r["status"].tolist() == [4]
    assert np.isfinite(r["jac"]).all() and np.isnan(r["sens"]).all() and np.isnan(r["se"]).all() and np.isfinite(r["cov_pm"]).all()
    # ... and with no rounding in the way: moments that do not move, whose mean is exact — J = 0, J'WJ = 0
    h4 = MR.copy_history(h)
    h4.sim_moments[:, 0, mem], h4.sim_moments[:, 1, mem] = 0.5, -0.25
    r = MR.moment_stats_from_history(h4, 0, 60, 0, GROUPS, PROBS, 0.0, prob.mom, prob.w, n_groups=4)
    assert r["status"].tolist() == [0, 0, 1, 4] and (r["jac"][3] == 0).all() and np.isnan(r["sens"][3]).all() and np.isnan(r["se"][3]).all()


def linalg(x, npar, w, ridge=0.0):
    """jac, sens, se of one group's joint columns x [D][m] by np.linalg"""
    d = x - x.mean(axis=1, keepdims=True)
    jac = np.linalg.lstsq(d[:npar].T, d[npar:].T, rcond=None)[0].T            # the regression of the moments on the parameters
    s, W = MR.weights(w)
    JW = jac.T * W
    sens = -np.linalg.solve(JW @ jac, JW)
    return jac, sens, np.sqrt(np.diag((sens * (s * s)) @ sens.T))


def test_jac_sens_se_against_numpy_linalg(mixing, dense57):
    worst, cells = 0.0, 0
    for case, groups, ng in ((mixing, GROUPS, 4), (dense57, (np.arange(16) % 2).astype(np.int32), 2)):
        prob, h = case
        T, npar = h.value.shape[0], h.params.shape[1]
        for t0, t1 in ((0, T), (5, T - 9)):
            for sel in (0, 1, 2):
                r = ref(case, t0, t1, sel, groups, n_groups=ng)
                cols = MR.joint_columns(h, t0, t1, sel, groups, ng)
                for g in range(ng):
                    if r["n_chains"][g] == 0:
                        assert r["status"][g] == 1
                        continue
                    assert r["status"][g] == 0, (t0, t1, sel, g)             # every cell meant to have status 0 has it
                    cells += 1
                    for got, want in zip((r["jac"][g], r["sens"][g], r["se"][g]), linalg(cols[g], npar, prob.w)):
                        worst = max(worst, float(np.max(np.abs(got - want)) / np.max(np.abs(want))))
    print("largest relative deviation from np.linalg over %d groups: %.3g (MOMENT_LINALG_DEV %.3g)" % (cells, worst, MR.MOMENT_LINALG_DEV))
    assert cells == 2 * 3 * (3 + 2)
    assert worst <= MR.MOMENT_LINALG_RTOL


CAP_N, CAP_T = 8, 48
CAP_GROUPS = (np.arange(CAP_N) % 2).astype(np.int32)


@pytest.fixture(scope="module")
def capped():
    """crafted_linear's history of every shape of MR.CAP_SHAPES with dense_problem's data moments and weights: (prob, h, J_true)"""
    out = {}
    for npar, nm in MR.CAP_SHAPES:
        prob, _ = MR.dense_problem(npar, nm, N=CAP_N, T=CAP_T)
        h, J = MR.crafted_linear(npar, nm, CAP_N, CAP_T, seed=npar * 100 + nm)
        out[npar, nm] = prob, h, J
    return out


def test_linear_part_columns_is_linear_part_bit_for_bit(mixing, dense57, capped):
    def same(cov_pp, cov_pm, w, ridge):
        a, b = MR.linear_part(cov_pp, cov_pm, w, ridge), MR.linear_part_columns(cov_pp, cov_pm, w, ridge)
        assert a[0] == b[0]
        for x, y in zip(a[1:], b[1:]):
            assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True) and np.array_equal(np.signbit(x), np.signbit(y))
        return a[0]
    seen = set()
    for prob, h in (mixing, dense57):
        npar = h.params.shape[1]
        for x in MR.joint_columns(h, 0, h.value.shape[0], 2, np.zeros(h.value.shape[1], np.int32), 1):
            cov = GS.column_cov(x)[1]
            for ridge in (0.0, 1e-6):
                seen.add(same(cov[:npar, :npar], cov[:npar, npar:], prob.w, ridge))
    for (npar, nm), (prob, h, _) in capped.items():            # one group of each shape at the caps, and one short of rows
        for t1, ridge in ((CAP_T, 0.0), (CAP_T, 1e-8), (3, 0.0)) if (npar, nm) != (64, 64) else ((CAP_T, 0.0), (3, 0.0)):
            cov = GS.column_cov(MR.joint_columns(h, 0, t1, 0, CAP_GROUPS, 2)[0])[1]
            seen.add(same(cov[:npar, :npar], cov[:npar, npar:], prob.w, ridge))
    seen.add(same(np.eye(3), np.zeros((3, 2)), [1.0, 2.0], 0.0))
    assert seen == {0, 3, 4}, seen                             # both early exits were compared too


def test_capped_shapes_statuses_by_design(capped):
    """every shape with nm >= np: J'WJ has full rank, status 0 in both groups over all 192 pooled rows; np = 64 against nm = 1: rank 1"""
    for (npar, nm), (prob, h, _) in capped.items():
        r = MR.moment_stats_from_history(h, 0, CAP_T, 0, CAP_GROUPS, PROBS, 0.0, prob.mom, prob.w)
        assert r["count"].tolist() == [4 * CAP_T] * 2 and 4 * CAP_T > npar + 1
        print("np %d nm %d: status %s" % (npar, nm, r["status"].tolist()))
        if nm >= npar:
            assert r["status"].tolist() == [0, 0], (npar, nm)
            assert np.isfinite(r["jac"]).all() and np.isfinite(r["sens"]).all() and np.isfinite(r["se"]).all()
        elif (npar, nm) == (64, 1):
            # the 63 later pivots of J'WJ are zero in exact arithmetic; rounded they are noise of either sign.  On this history the first
            # of them is not positive: 4.  (A 0 would be accepted as the existing nm < np case accepts it: the GPU test follows this table)
            assert r["status"].tolist() == [4, 4] and np.isfinite(r["jac"]).all() and np.isnan(r["sens"]).all()
        else:
            assert set(r["status"].tolist()) <= {0, 4}
    prob, h, _ = capped[64, 64]                                # a group short of rows: 40 < np + 1, Cov(theta, theta) is singular
    g3 = np.array([0, 1, 0, 1, 0, 1, 0, 2], np.int32)
    r = MR.moment_stats_from_history(h, 5, 45, 0, g3, PROBS, 0.0, prob.mom, prob.w)
    print("a group of 40 rows at np = 64: status", r["status"].tolist())
    assert r["count"].tolist() == [160, 120, 40] and r["status"][2] == 3 and np.isnan(r["jac"][2]).all() and np.isnan(r["se"][2]).all()
    assert np.isfinite(r["cov_pp"][2]).all() and np.isfinite(r["fit_z"][2]).all()


def test_jac_sens_se_against_numpy_linalg_at_the_caps(capped):
    """the independent anchor of the capped shapes: jac against lstsq, sens and se against solve, jac against the J_true the moments
    were made from (1e-3 noise on top), over every status-0 group (jac alone where the status is 4)"""
    worst, worst_true, cells = 0.0, 0.0, 0
    for (npar, nm), (prob, h, J) in capped.items():
        for sel in (0, 1, 2):
            r = MR.moment_stats_from_history(h, 0, CAP_T, sel, CAP_GROUPS, (), 0.0, prob.mom, prob.w)
            cols = MR.joint_columns(h, 0, CAP_T, sel, CAP_GROUPS, 2)
            for g in range(2):
                if r["status"][g] not in (0, 4):
                    continue
                d = cols[g] - cols[g].mean(axis=1, keepdims=True)
                want = np.linalg.lstsq(d[:npar].T, d[npar:].T, rcond=None)[0].T
                worst = max(worst, float(np.max(np.abs(r["jac"][g] - want)) / np.max(np.abs(want))))
                worst_true = max(worst_true, float(np.max(np.abs(r["jac"][g] - J)) / np.max(np.abs(J))))
                if r["status"][g] == 0:
                    cells += 1
                    for got, want in zip((r["jac"][g], r["sens"][g], r["se"][g]), linalg(cols[g], npar, prob.w)):
                        worst = max(worst, float(np.max(np.abs(got - want)) / np.max(np.abs(want))))
    print("largest relative deviation from np.linalg over %d status-0 groups at the caps: %.3g (MOMENT_LINALG_CAPS_DEV %.3g); from J_true: "
          "%.3g (MOMENT_JTRUE_CAPS_DEV %.3g)" % (cells, worst, MR.MOMENT_LINALG_CAPS_DEV, worst_true, MR.MOMENT_JTRUE_CAPS_DEV))
    assert cells >= 2 * 5                                      # at least select 0 of the five shapes with nm >= np
    assert worst <= MR.MOMENT_LINALG_CAPS_RTOL
    assert worst_true <= MR.MOMENT_JTRUE_CAPS_RTOL


def test_a_ridge_moves_the_jacobian_a_little(mixing):
    a, b = ref(mixing, 0, 60, 2, GROUPS, n_groups=4), ref(mixing, 0, 60, 2, GROUPS, ridge=1e-6, n_groups=4)
    assert np.array_equal(a["cov_pp"], b["cov_pp"], equal_nan=True) and not np.array_equal(a["jac"][0], b["jac"][0])
    assert b["jac"][0] == pytest.approx(a["jac"][0], rel=1e-4, abs=1e-6)


def test_ctypes_layout_matches_the_header():
    names = [f for f, _ in A.smm_moment_stats_t._fields_]
    assert names == list(MR.FIELDS)
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "smmhip.h"', "int main(void) {",
             'printf("size %zu\\n", sizeof(smm_moment_stats_t));']
    lines += ['printf("%s %%zu\\n", offsetof(smm_moment_stats_t, %s));' % (f, f) for f in names]
    lines.append("return 0; }")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "p.c"), "-o", os.path.join(d, "p")])
        out = dict(l.rsplit(" ", 1) for l in subprocess.check_output([os.path.join(d, "p")]).decode().strip().splitlines())
    assert int(out["size"]) == C.sizeof(A.smm_moment_stats_t)
    for f in names:
        assert getattr(A.smm_moment_stats_t, f).offset == int(out[f]), f
    argtypes = dict((n, a) for n, _, a in A.SYMBOLS)["smm_get_moment_stats"]
    assert argtypes == [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, A.c_int32_p, C.c_int32, A.c_double_p, C.c_int32, C.c_double,
                        C.POINTER(A.smm_moment_stats_t)]
    assert hasattr(A.load(), "smm_get_moment_stats")
