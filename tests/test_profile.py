"""tests/profile_ref.py, the restatement of smm_get_profile's contract (include/smmhip.h) the GPU tests hold the device against, held on a
history of the CPU oracle against numpy itself (np.histogram, np.histogram2d, np.mean) and a plain loop over the rows for the minimum;
the tie, -0 / +0, NaN-value and empty-bin rules on a crafted history; and the ctypes mirror of smm_profile_t and the Julia struct and
ccall against the header compiled with gcc.  No GPU."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import common as cm
import moment_stats_ref as MR
import profile_ref as PR
import rank_diag_ref as RD
from smm_jl_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = np.array([0, 0, 1, 1, 1, -1, 0, 0, 3, 3, 1, 1, 0, 3, 3, 3, 1, 0, -1, 3, 0, 1, 3, 0], np.int32)   # group 2 has no member
PAIRS = [(0, 1), (1, 1)]


@pytest.fixture(scope="module")
def mixing(O):
    prob, opts = cm.serial_normal(**dict(RD.MIXING, N=24, T=60, acc_tuners=0.5, seed=4))
    o = O.OracleContext(prob, opts)
    o.step(60)
    return o.history(0, 60)


def rows_of(h, t0, t1, select, members):
    """(chain, t, src) of the pooled rows of the members, by a plain loop"""
    out = []
    for c in members:
        last = -1
        for t in range(t1):
            if h.accepted[t, c] != 0:
                last = t
            if t < t0 or (select == 1 and h.accepted[t, c] == 0):
                continue
            out.append((c, t, last if select == 2 else t))
    return out


def test_counts_are_numpys_and_means_are_np_mean(mixing):
    h = mixing
    rng = np.array([[-0.5, 0.9], [9.5, 10.5]])
    for select in (0, 1, 2):
        for t0, t1 in ((0, 60), (7, 41)):
            for bins, r in ((6, None), (5, rng)):
                got = PR.profile_from_history(h, t0, t1, select, GROUPS, bins, r, PAIRS, 4, n_groups=4)
                assert got["m_mean"].shape == (4, 2, bins, 2) and got["v_mean2"].shape == (4, 2, 4, 4)
                for g in (0, 1, 3):
                    rows = [q for q in rows_of(h, t0, t1, select, np.flatnonzero(GROUPS == g)) if q[2] >= 0]
                    if select == 2 and len(rows) < (t1 - t0) * (GROUPS == g).sum() and r is None:
                        assert (got["status"][g] == 1).all() and (got["n"][g] == 0).all() and np.isnan(got["v_mean"][g]).all()
                        continue
                    c, t, s = (np.array(v) for v in zip(*rows))
                    x, v = h.params[s, :, c], h.value[s, c]
                    for k in range(2):
                        n, e = np.histogram(x[:, k], bins, None if r is None else r[k])
                        assert np.array_equal(got["n"][g, k], n) and np.array_equal(got["edges"][g, k], e)
                        b = np.clip(np.searchsorted(e, x[:, k], "right") - 1, 0, bins - 1)
                        inside = (x[:, k] >= e[0]) & (x[:, k] <= e[-1])
                        for i in range(bins):
                            idx = np.flatnonzero(inside & (b == i))
                            assert len(idx) == n[i]
                            if len(idx):
                                assert got["v_mean"][g, k, i] == np.mean(v[idx])
                                assert got["m_mean"][g, k, i, 1] == np.mean(np.ascontiguousarray(h.sim_moments[s[idx], 1, c[idx]]))
                    for p, (a, b2) in enumerate(PAIRS):
                        H, _, _ = np.histogram2d(x[:, a], x[:, b2], 4, None if r is None else [r[a], r[b2]])
                        assert np.array_equal(got["n2"][g, p], H.astype(np.int64))
                assert (got["n"][2] == 0).all() and got["count"][2] == 0 and np.isnan(got["v_min"][2]).all()


def test_minimum_chain_iteration_and_theta_agree_with_a_plain_loop(mixing):
    h = mixing
    for select, t0, t1 in ((0, 0, 60), (1, 7, 41), (2, 20, 60)):
        got = PR.profile_from_history(h, t0, t1, select, GROUPS, 5, np.array([[-0.5, 0.9], [9.5, 10.5]]), [(0, 1)], 3, n_groups=4, chain_offset=100)
        for g in (0, 1, 3):
            rows = rows_of(h, t0, t1, select, np.flatnonzero(GROUPS == g))
            for k in range(2):
                e = got["edges"][g, k]
                best = {}
                for c, t, s in rows:
                    if s < 0:
                        continue
                    x, v = h.params[s, k, c], h.value[s, c]
                    if not (e[0] <= x <= e[-1]) or not abs(v) <= np.finfo(float).max:
                        continue
                    i = min(int(np.searchsorted(e, x, "right")) - 1, 4)
                    if i not in best or v < best[i][0]:
                        best[i] = (v, 100 + c + 1, t + 1, h.params[s, :, c].copy())
                for i in range(5):
                    if i in best:
                        assert got["v_min"][g, k, i] == best[i][0] and got["min_chain"][g, k, i] == best[i][1]
                        assert got["min_iter"][g, k, i] == best[i][2] and np.array_equal(got["theta_at_min"][g, k, i], best[i][3])
                    else:
                        assert np.isnan(got["v_min"][g, k, i]) and got["min_chain"][g, k, i] == 0 and got["min_iter"][g, k, i] == 0
                        assert np.isnan(got["theta_at_min"][g, k, i]).all() and got["n_scored"][g, k, i] == 0


def test_ties_signed_zeros_unscored_rows_and_empty_bins(mixing):
    c = MR.copy_history(mixing)
    T, N = c.value.shape
    c.accepted[...] = 1
    c.params[:, 0, :] = 0.25                               # every row in bin 1 of [0, 1] / 4 ...
    c.params[:, 1, :] = 10.0
    c.params[3, 0, 2] = c.params[9, 0, 1] = 0.75           # ... but two rows in bin 3, both unscored
    c.value[...] = 5.0
    c.value[3, 2], c.value[9, 1] = np.nan, np.inf
    c.value[4, 1], c.value[2, 2], c.value[7, 0] = 1.0, 1.0, np.nan   # equal minima in chains 1 and 2: chain 1 pools first
    c.value[11, 0], c.status[11, 0] = -np.inf, -1          # a failed evaluation
    c.sim_moments[5, 0, 0] = np.nan                        # a NaN moment in a scored row
    g = np.full(N, -1, np.int32)
    g[:3] = 0
    r = PR.profile_from_history(c, 0, T, 0, g, 4, np.array([[0.0, 1.0], [9.0, 11.0]]), n_groups=1)
    assert r["n"][0, 0].tolist() == [0, 3 * T - 2, 0, 2] and r["n_scored"][0, 0].tolist() == [0, 3 * T - 4, 0, 0]
    assert (r["v_min"][0, 0, 1], r["min_chain"][0, 0, 1], r["min_iter"][0, 0, 1]) == (1.0, 2, 5)
    assert np.isnan(r["v_min"][0, 0, [0, 2, 3]]).all() and (r["min_chain"][0, 0, [0, 2, 3]] == 0).all()
    assert np.isnan(r["v_mean"][0, 0, 3]) and np.isnan(r["theta_at_min"][0, 0, 3]).all()
    assert r["v_mean"][0, 0, 1] == (5.0 * (3 * T - 6) + 2.0) / (3 * T - 4)
    assert np.isnan(r["m_mean"][0, 0, 1, 0]) and np.isfinite(r["m_mean"][0, 0, 1, 1])
    c.value[...] = 5.0
    c.value[6, 1], c.value[2, 2] = -0.0, 0.0               # -0 ahead of +0 in pooled order: the earlier one, with its sign
    c.value[:, 0] = 7.0
    r = PR.profile_from_history(c, 0, T, 0, g, 4, np.array([[0.0, 1.0], [9.0, 11.0]]), n_groups=1, moments=False)
    assert "m_mean" not in r and r["v_min"][0, 0, 1] == 0.0 and np.signbit(r["v_min"][0, 0, 1])
    assert (r["min_chain"][0, 0, 1], r["min_iter"][0, 0, 1]) == (2, 7)
    c.value[6, 1], c.value[2, 2] = 0.0, -0.0
    r = PR.profile_from_history(c, 0, T, 0, g, 4, np.array([[0.0, 1.0], [9.0, 11.0]]), n_groups=1)
    assert r["v_min"][0, 0, 1] == 0.0 and not np.signbit(r["v_min"][0, 0, 1]) and r["min_chain"][0, 0, 1] == 2
    PR.assert_profile_equal(r, r)
    bad = dict(r, v_min=-r["v_min"])
    with pytest.raises(AssertionError):
        PR.assert_profile_equal(bad, r)


@pytest.fixture(scope="module")
def caps():
    return PR.crafted_caps(PR.zeroed_history(PR.CAPS_T, len(PR.CAPS_GROUPS), 2, 2))


def test_crafted_caps_history_holds_what_the_cap_cases_need(caps):
    """the design of profile_ref.crafted_caps, on the restatement alone, and its counts against np.histogram / np.histogram2d"""
    h, g, T = caps, PR.CAPS_GROUPS, PR.CAPS_T
    pairs = [(0, 1), (1, 0), (1, 1)]
    for bins, B2 in ((3, 2), (7, 3)):
        r = PR.profile_from_history(h, 0, T, 0, g, bins, PR.CAPS_RANGE, pairs, B2, n_groups=PR.CAPS_NG)
        assert r["count"].tolist() == [4 * T, 2 * T, 14 * T, T, 0] and (r["status"] == 0).all()
        big = int(np.argmax(r["n_scored"][2, 0]))
        assert r["n_scored"][2, 0, big] >= 8260 > 8192 and r["n_scored2"][2, 0].max() >= 8260     # a second chunk, 1-D and 2-D
        assert (r["v_min"][2, 0, big], r["min_chain"][2, 0, big], r["min_iter"][2, 0, big]) == (-3.0, PR.CAPS_MIN[0] + 1, PR.CAPS_MIN[1] + 1)
        hot = int(np.searchsorted(r["edges"][0, 0], 0.9, "right")) - 1                            # the segment of x = 0.9
        assert r["v_min"][0, 0, hot] == 0.0 and np.signbit(r["v_min"][0, 0, hot]) and r["min_iter"][0, 0, hot] == 21
        assert r["v_min"][3, 0, hot] == 0.0 and not np.signbit(r["v_min"][3, 0, hot]) and r["min_iter"][3, 0, hot] == 8
        assert (r["n"][0] > r["n_scored"][0]).any() and np.isnan(r["m_mean"][0, ..., 0]).any() and np.isfinite(r["m_mean"][0, ..., 1]).all()
        assert r["n"][0, 0].sum() < 4 * T                                                          # rows outside the range
        for q in (0, 1, 2, 3):                                                                     # the rows on edges land where numpy puts them
            x = np.concatenate([h.params[:, :, c] for c in np.flatnonzero(g == q)])
            for k in range(2):
                n, e = np.histogram(x[:, k], bins, PR.CAPS_RANGE[k])
                assert np.array_equal(r["n"][q, k], n) and np.array_equal(r["edges"][q, k], e)
            for p, (a, b) in enumerate(pairs):
                H = np.histogram2d(x[:, a], x[:, b], B2, [PR.CAPS_RANGE[a], PR.CAPS_RANGE[b]])[0]
                assert np.array_equal(r["n2"][q, p], H.astype(np.int64))
        e = r["edges"][1, 0]
        assert all((h.params[:, 0, 3] == v).any() and (h.params[:, 1, 3] == v).any() for v in e)  # on every edge, lo and hi included
    acc = PR.profile_from_history(h, 0, T, 1, g, 3, PR.CAPS_RANGE, n_groups=PR.CAPS_NG)
    big = int(np.argmax(acc["n_scored"][2, 0]))
    assert (acc["v_min"][2, 0, big], acc["min_chain"][2, 0, big], acc["min_iter"][2, 0, big]) == (-3.0, 8, 301)   # the same member's next block
    late = PR.profile_from_history(h, 137, 590, 0, g, 3, PR.CAPS_RANGE, n_groups=PR.CAPS_NG)
    assert (late["min_chain"][2, 0, big], late["min_iter"][2, 0, big]) == (8, 301)
    # the means of the big segment against np.mean (numpy's pairwise sum of one chunk is not the chunked sum: to rounding)
    full = PR.profile_from_history(h, 0, T, 0, g, 3, PR.CAPS_RANGE, n_groups=PR.CAPS_NG)
    mem = np.flatnonzero(g == 2)
    x, v = np.concatenate([h.params[:, 0, c] for c in mem]), np.concatenate([h.value[:, c] for c in mem])
    m1 = np.concatenate([h.sim_moments[:, 1, c] for c in mem])
    idx = (x >= full["edges"][2, 0, big]) & (x < full["edges"][2, 0, big + 1]) & PR.scored(v)
    assert idx.sum() == full["n_scored"][2, 0, big]
    assert full["v_mean"][2, 0, big] == pytest.approx(v[idx].mean(), rel=1e-13) and full["m_mean"][2, 0, big, 1] == pytest.approx(m1[idx].mean(), rel=1e-11)


def test_profile_ref_at_the_segment_caps_against_numpy():
    """bins = 4096 and bins2 = 256 (65,536 cells a pair) on 40 iterations: the counts are numpy's (the restatement walks the occupied
    segments only: well under a second)"""
    h = PR.crafted_wide(PR.zeroed_history(40, len(PR.CAPS_GROUPS), 2, 2))
    r = PR.profile_from_history(h, 0, 40, 2, PR.CAPS_GROUPS, 4096, None, [(1, 0)], 256, n_groups=PR.CAPS_NG)
    assert r["n"].shape == (5, 2, 4096) and r["v_mean2"].shape == (5, 1, 256, 256)
    assert r["n"].sum(axis=2).tolist() == [[160] * 2, [80] * 2, [560] * 2, [40] * 2, [0] * 2] and r["n2"].sum() == 840
    c, _, s = PR.pooled_rows(h, 0, 40, 2, PR.CAPS_GROUPS, 5)[2]
    xs = h.params[s, :, c]
    assert np.array_equal(r["n"][2, 0], np.histogram(xs[:, 0], 4096)[0])
    assert np.array_equal(r["n2"][2, 0], np.histogram2d(xs[:, 1], xs[:, 0], 256)[0].astype(np.int64))


def test_ctypes_layout_matches_the_header():
    names = [f for f, _ in A.smm_profile_t._fields_]
    assert names == list(PR.FIELDS) and len(names) == 18
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "smmhip.h"', "int main(void) {",
             'printf("size %zu\\n", sizeof(smm_profile_t));']
    lines += ['printf("%s %%zu\\n", offsetof(smm_profile_t, %s));' % (f, f) for f in names]
    lines.append("return 0; }")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "p.c"), "-o", os.path.join(d, "p")])
        out = dict(l.rsplit(" ", 1) for l in subprocess.check_output([os.path.join(d, "p")]).decode().strip().splitlines())
    assert int(out["size"]) == C.sizeof(A.smm_profile_t) == 18 * C.sizeof(C.c_void_p)
    for f in names:
        assert getattr(A.smm_profile_t, f).offset == int(out[f]), f
    argtypes = dict((n, a) for n, _, a in A.SYMBOLS)["smm_get_profile"]
    assert argtypes == [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, A.c_int32_p, C.c_int32, C.c_int32, A.c_double_p, A.c_int32_p,
                        C.c_int32, C.c_int32, C.POINTER(A.smm_profile_t)]
    assert hasattr(A.load(), "smm_get_profile")


def test_julia_struct_and_ccall_match_the_abi():
    src = open(os.path.join(ROOT, "julia", "SMMHip.jl")).read()
    m = re.search(r"ccall\(sym\(:smm_get_profile\), Cint,\s*\(([^()]*(?:\{[^()]*\}[^()]*)*)\)", src)
    assert m
    jl = [t.strip() for t in m.group(1).split(",") if t.strip()]
    spell = {C.c_void_p: "Ptr{Cvoid}", C.c_int32: "Cint", A.c_int32_p: "Ptr{Int32}", A.c_double_p: "Ptr{Cdouble}",
             C.POINTER(A.smm_profile_t): "Ref{SmmProfile}"}
    argtypes = dict((n, a) for n, _, a in A.SYMBOLS)["smm_get_profile"]
    assert jl == [spell[t] for t in argtypes]
    fields = re.search(r"struct SmmProfile\n(.*?)\nend", src, re.S).group(1).split()
    assert [f.split("::")[0] for f in fields] == [f for f, _ in A.smm_profile_t._fields_]
    ptr = {A.c_double_p: "Ptr{Cdouble}", A.c_int32_p: "Ptr{Int32}", C.POINTER(C.c_int64): "Ptr{Int64}"}
    assert [f.split("::")[1] for f in fields] == [ptr[t] for _, t in A.smm_profile_t._fields_]
    backend = open(os.path.join(ROOT, "julia", "SMMHipBackend.jl")).read()
    assert "function profile_objective(algo::MAlgoBGPHip" in backend and "SMMHip.hip_profile(" in backend
    assert re.search(r"^export .*\bhip_profile\b", src, re.M) and re.search(r"^export .*\bprofile_objective\b", backend, re.M)
