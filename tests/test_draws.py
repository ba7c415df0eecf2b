"""tests/draws_ref.py, the restatement of smm_get_draws' selection contract (include/smmhip.h) the GPU tests hold the device against,
held against a brute-force list of (chain, iteration, source row) tuples on a history of the CPU oracle, for all three selections; the
cap's position rule for every small (m, K); and the ctypes mirror of smm_draws_t against the header compiled with gcc.  No GPU."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import common as cm
import draws_ref as DR
from smm_jl_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute(h, t0, t1, select, groups, G, thin, K):
    """the contract with explicit lists: per group the (chain, t, src) tuples of every member, thinned and capped by list indexing"""
    out = []
    for g in range(G):
        pooled = []
        for c in range(len(groups)):
            if groups[c] != g:
                continue
            rows = []
            for t in range(t0, t1):
                if select == 1 and not h.accepted[t, c]:
                    continue
                src = t
                if select == 2:
                    src = -1
                    for r in range(t, -1, -1):
                        if h.accepted[r, c]:
                            src = r
                            break
                rows.append((c, t, src))
            pooled += [rows[i] for i in range(len(rows)) if i % thin == 0]
        m = len(pooled)
        out.append((m, pooled if m <= K else [pooled[(j * m) // K] for j in range(K)]))
    return out


def test_draws_ref_against_a_brute_force_restatement(O):
    N, T = 24, 40
    prob, opts = cm.general_normal(3, N=N, T=T, ns=200)
    o = O.OracleContext(prob, opts)
    o.step(T)
    h = o.history(0, T)
    groups = np.array([0, 1, 1, -1, 3, 3, 3, 0, 1, 4, 4, 4, 4, -1, 1, 0, 3, 3, 4, 4, 1, 1, 0, 3], np.int32)   # group 2 has no member
    assert 0 < h.accepted[5:37].mean() < 1
    seen_lookback = False
    for select in (0, 1, 2):
        for t0, t1 in ((0, T), (5, 37), (11, 11), (0, 2)):
            for thin in (1, 3):
                for K in (1, 7, 50, 10000):
                    want = brute(h, t0, t1, select, groups, 5, thin, K)
                    got = DR.draws_from_history(h, t0, t1, select, groups, thin, K, n_groups=5, chain_offset=100)
                    assert got["count"].tolist() == [m for m, _ in want]
                    assert got["n_chains"].tolist() == np.bincount(groups[groups >= 0], minlength=5).tolist()
                    assert got["row0"].tolist() == np.concatenate([[0], np.cumsum([len(r) for _, r in want])]).tolist()
                    rows = [r for _, rs in want for r in rs]
                    assert got["chain"].tolist() == [c + 101 for c, _, _ in rows]
                    assert got["iter"].tolist() == [t + 1 for _, t, _ in rows]
                    assert got["src_iter"].tolist() == [s + 1 for _, _, s in rows]
                    for q, (c, t, s) in enumerate(rows):
                        if s < 0:
                            assert np.isnan(got["params"][q]).all() and np.isnan(got["value"][q]) and np.isnan(got["sim_moments"][q]).all()
                        else:
                            seen_lookback |= s < t0
                            assert np.array_equal(got["params"][q].view(np.uint64), np.ascontiguousarray(h.params[s, :, c]).view(np.uint64))
                            assert got["value"][q] == h.value[s, c]
                            assert np.array_equal(got["sim_moments"][q], h.sim_moments[s, :, c])
    assert seen_lookback
    one = DR.draws_from_history(h, 0, T, "accepted")            # no groups: every chain in group 0
    assert one["count"].tolist() == [int((h.accepted != 0).sum())] and one["row0"].tolist() == [0, min(one["count"][0], 10000)]
    h.accepted[:, 4] = 0                                        # a chain that never accepts: no state at all
    got = DR.draws_from_history(h, 3, 9, 2, groups, 1, 10000, n_groups=5)
    assert (got["src_iter"][got["chain"] == 5] == 0).all() and np.isnan(got["value"][got["chain"] == 5]).all() and (got["chain"] == 5).sum() == 6


def test_wide_rows_case_by_brute_force():
    """the design of the wide-row case of tests/test_gpu_reducer_caps.py (np = nm = 64, three groups, a chain in no group, a cap that
    cuts a group) on profile_ref.crafted_wide's history, against the brute-force list"""
    import profile_ref as PR
    N, T = 8, 40
    h = PR.crafted_wide(PR.zeroed_history(T, N, 64, 64))
    groups = np.array([0, 1, 1, -1, 2, 0, 2, 2], np.int32)
    for select in (0, 1, 2):
        for thin, K in ((1, 10000), (3, 10000), (1, 50), (3, 17)):
            want = brute(h, 3, T, select, groups, 3, thin, K)
            got = DR.draws_from_history(h, 3, T, select, groups, thin, K, n_groups=3)
            rows = [r for _, rs in want for r in rs]
            assert got["count"].tolist() == [m for m, _ in want] and len(rows) == got["row0"][3]
            assert K > 50 or (got["count"] > K).any()                              # the cap cuts a group
            assert got["chain"].tolist() == [c + 1 for c, _, _ in rows] and got["src_iter"].tolist() == [s + 1 for _, _, s in rows]
            assert got["params"].shape == (len(rows), 64) and got["sim_moments"].shape == (len(rows), 64)
            for q, (c, t, s) in enumerate(rows):
                assert np.array_equal(got["params"][q], h.params[s, :, c]) and np.array_equal(got["sim_moments"][q], h.sim_moments[s, :, c])
                assert np.array_equal(got["value"][q], h.value[s, c], equal_nan=True)


def test_position_rule():
    for m in range(0, 41):
        for K in range(1, 13):
            p = DR.positions(m, K)
            assert len(p) == min(m, K)
            assert all(0 <= v < m for v in p)
            assert all(a < b for a, b in zip(p, p[1:]))
            if m <= K:
                assert p == list(range(m))


def test_ctypes_layout_matches_the_header():
    names = [f for f, _ in A.smm_draws_t._fields_]
    assert names == ["count", "n_chains", "row0", "params", "value", "sim_moments", "chain", "iter", "src_iter"] == list(DR.FIELDS)
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "smmhip.h"', "int main(void) {",
             'printf("size %zu\\n", sizeof(smm_draws_t));']
    lines += ['printf("%s %%zu\\n", offsetof(smm_draws_t, %s));' % (f, f) for f in names]
    lines.append("return 0; }")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "p.c"), "-o", os.path.join(d, "p")])
        out = dict(l.rsplit(" ", 1) for l in subprocess.check_output([os.path.join(d, "p")]).decode().strip().splitlines())
    assert int(out["size"]) == C.sizeof(A.smm_draws_t)
    for f in names:
        assert getattr(A.smm_draws_t, f).offset == int(out[f]), f
    argtypes = dict((n, a) for n, _, a in A.SYMBOLS)["smm_get_draws"]
    assert argtypes == [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, A.c_int32_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64,
                        C.POINTER(A.smm_draws_t)]
    assert hasattr(A.load(), "smm_get_draws")
