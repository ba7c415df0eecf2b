"""tests/trace_ref.py, the restatement of smm_get_trace's contract (include/smmhip.h) the GPU tests hold the device against, held
against hand-worked small cases: the rows a stride keeps, the look-back before t0, a member with no state, columns of 0, 1 and 2
members, the first-NaN and tie order of the best value; its stacked reductions against the one-column numpy calls and its look-back
against chain_diag_ref's series; and the ctypes mirror of smm_trace_t against the header compiled with gcc.  No GPU."""
import ctypes as C
import os
import subprocess
import tempfile
from types import SimpleNamespace

import numpy as np

import chain_diag_ref as D
import trace_ref as TR
from smm_jl_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = np.nan


def history(T, N, npar=1, nm=1, seed=0):
    r = np.random.default_rng(seed)
    return SimpleNamespace(params=r.standard_normal((T, npar, N)), sim_moments=r.standard_normal((T, nm, N)), value=r.standard_normal((T, N)),
                           accepted=(r.random((T, N)) < 0.5).astype(np.uint8), exchanged=np.zeros((T, N), np.int32),
                           status=np.zeros((T, N), np.int8))


def test_stride_keeps_every_stride_th_row_of_the_window():
    for t0, t1, stride, want in ((0, 10, 1, 10), (0, 10, 3, 4), (2, 10, 4, 2), (2, 11, 4, 3), (5, 5, 1, 0), (5, 6, 1000, 1), (0, 300, 7, 43)):
        assert TR.n_rows(t0, t1, stride) == want == len(range(t0, t1, stride))
    h = history(12, 3)
    r = TR.trace_from_history(h, 2, 11, 4, "all")
    assert r["iter"].tolist() == [2, 6, 10] and r["mean"].shape == (3, 1, 2) and r["quantile"].shape == (0, 3, 1, 2)
    for i, t in enumerate((2, 6, 10)):
        assert r["mean"][i, 0, 0] == np.mean(np.ascontiguousarray(h.params[t, 0, :]))
        assert r["mean"][i, 0, 1] == np.mean(np.ascontiguousarray(h.value[t]))
    e = TR.trace_from_history(h, 5, 5, 2, "state", groups=[0, 1, 1])
    assert e["iter"].shape == (0,) and e["count"].shape == (0, 2) and e["n_chains"].tolist() == [1, 2]


def test_state_looks_back_before_t0_and_a_member_without_state_is_nan():
    T, N = 6, 3
    h = history(T, N)
    h.accepted[...] = 0
    h.accepted[1, 0] = 1                      # chain 0: its state is row 1 from iteration 1 on
    h.accepted[[0, 4], 1] = 1                 # chain 1: row 0, then row 4
    #                                           chain 2: never accepted
    h.params[:, 0, :] = np.arange(T)[:, None] * 10.0 + np.arange(N)     # params[t][c] = 10 t + c
    h.value[...] = -h.params[:, 0, :]
    h.sim_moments[:, 0, :] = 0.5 * h.params[:, 0, :]
    r = TR.trace_from_history(h, 3, 6, 1, "state", moments=True, groups=[0, 1, 2])
    assert r["iter"].tolist() == [3, 4, 5] and (r["count"] == 1).all()
    assert r["mean"][:, 0, 0].tolist() == [10.0, 10.0, 10.0]            # row 1, before t0 = 3
    assert r["mean"][:, 1, 0].tolist() == [1.0, 41.0, 41.0]             # row 0, then row 4
    assert r["mean"][:, 1, 1].tolist() == [-1.0, -41.0, -41.0] and r["mean"][:, 1, 2].tolist() == [0.5, 20.5, 20.5]
    assert np.isnan(r["mean"][:, 2, :]).all() and np.isnan(r["median"][:, 2, :]).all() and (r["count"][:, 2] == 1).all()
    assert np.isnan(r["var"]).all()           # one member per group
    pooled = TR.trace_from_history(h, 3, 6, 1, "state", groups=None, probs=(0.5,))
    assert (pooled["count"] == 3).all() and np.isnan(pooled["mean"]).all() and np.isnan(pooled["quantile"]).all()   # the NaN member
    two = TR.trace_from_history(h, 3, 6, 2, "state", groups=[0, 0, -1], probs=(0.0, 0.5, 1.0))
    assert two["iter"].tolist() == [3, 5] and two["mean"][:, 0, 0].tolist() == [5.5, 25.5] and two["var"][:, 0, 0].tolist() == [40.5, 480.5]
    assert two["quantile"][:, 1, 0, 0].tolist() == [10.0, 25.5, 41.0] and two["n_chains"].tolist() == [2]
    X, _ = D.series_from_history(h, 3, 6)     # chain_diag_ref's series: [S][N][n]
    per = TR.trace_from_history(h, 3, 6, 1, "state", groups=[0, 1, 2])
    assert np.array_equal(per["mean"].transpose(2, 1, 0), X, equal_nan=True)


def test_columns_of_zero_one_and_two_members():
    h = history(4, 4)
    h.accepted[...] = 0
    h.accepted[1, 2] = 1
    h.accepted[2, [1, 3]] = 1
    h.exchanged[2, 3] = 2
    h.status[3, :2] = -1
    r = TR.trace_from_history(h, 0, 4, 1, "accepted", groups=None, probs=(0.25,))
    assert r["count"][:, 0].tolist() == [0, 1, 2, 0] and r["n_chains"].tolist() == [4]
    assert r["n_accepted"][:, 0].tolist() == [0, 1, 1, 0] and r["n_exchanged"][:, 0].tolist() == [0, 0, 1, 0]
    assert r["n_failed"][:, 0].tolist() == [0, 0, 0, 2]
    for f in ("mean", "var", "median"):
        assert np.isnan(r[f][[0, 3]]).all()
    assert np.isnan(r["quantile"][:, [0, 3]]).all()
    assert r["mean"][1, 0, 0] == h.params[1, 0, 2] == r["median"][1, 0, 0] == r["quantile"][0, 1, 0, 0] and np.isnan(r["var"][1, 0, 0])
    a, b = h.params[2, 0, 1], h.params[2, 0, 3]
    mu = (a + b) / 2
    assert r["mean"][2, 0, 0] == mu and r["var"][2, 0, 0] == ((a - mu) * (a - mu) + (b - mu) * (b - mu)) / 1.0
    lo, hi = min(a, b), max(a, b)
    assert r["median"][2, 0, 0] == mu and r["quantile"][0, 2, 0, 0] == lo + (hi - lo) * 0.25
    assert not np.isnan(r["best_value"]).any()             # the best is over every member, whatever is selected
    empty = TR.trace_from_history(h, 0, 4, 1, "all", groups=[0, 0, 2, 2], probs=(0.5,))
    assert empty["n_chains"].tolist() == [2, 0, 2] and (empty["count"][:, 1] == 0).all() and (empty["best_chain"][:, 1] == 0).all()
    assert np.isnan(empty["best_value"][:, 1]).all() and np.isnan(empty["mean"][:, 1]).all()


def test_best_is_the_first_nan_else_the_first_minimum():
    h = history(3, 5)
    h.value[0] = [3.0, 1.0, 2.0, 1.0, 4.0]                 # a tie: the first
    h.value[1] = [3.0, NAN, 0.0, NAN, -1.0]                # a NaN wins, the first of them
    h.value[2] = [np.inf, 7.0, -np.inf, 7.0, -np.inf]
    r = TR.trace_from_history(h, 0, 3, 1, "all", groups=None, chain_offset=10)
    assert r["best_chain"][:, 0].tolist() == [12, 12, 13] and r["best_value"][0, 0] == 1.0 and np.isnan(r["best_value"][1, 0])
    assert r["best_value"][2, 0] == -np.inf
    g = TR.trace_from_history(h, 0, 3, 1, "accepted", groups=[1, 0, 0, 1, 1])
    assert g["best_chain"].tolist() == [[2, 4], [2, 4], [3, 5]]
    TR.assert_trace_equal(g, g)
    bad = dict(g, best_chain=g["best_chain"] + 1)
    try:
        TR.assert_trace_equal(bad, g)
    except AssertionError:
        pass
    else:
        raise AssertionError("assert_trace_equal let a difference through")


def test_stacked_reductions_equal_the_one_column_calls():
    r = np.random.default_rng(5)
    pool = np.array([-0.0, 0.0, 1.0, 1.0, -np.inf, np.inf, 2.0, -3.0, NAN])
    probs = (0.0, 0.025, 0.5, 0.9, 1.0)
    for m in (1, 2, 3, 7, 8, 9, 64, 129, 1000, 8192):
        X = r.standard_normal((6, m)) * 10.0 ** r.integers(-3, 4, (6, 1))
        if m <= 64:
            X[3:] = r.choice(pool, (3, m))
        mu, var, med, q = TR.stacked_stats(X, probs)
        for c in range(6):
            w = TR.column_stats(X[c].copy(), probs)
            for a, b in ((mu[c], w[0]), (var[c], w[1]), (med[c], w[2])):
                assert a == b or (np.isnan(a) and np.isnan(b)), (m, c)
            assert np.array_equal(q[:, c], w[3], equal_nan=True), (m, c)
    long = TR.stacked_stats(r.standard_normal((2, 9000)), (0.5,))      # past numpy's buffer: one column at a time
    assert long[0].shape == (2,) and long[3].shape == (1, 2)
    h = history(9, 40, npar=2, nm=3, seed=3)
    got = TR.trace_from_history(h, 1, 9, 3, "accepted", True, np.arange(40) % 3, probs)
    for i, t in enumerate((1, 4, 7)):
        for g in range(3):
            mem = np.flatnonzero(np.arange(40) % 3 == g)
            mem = mem[h.accepted[t, mem] != 0]
            cols = [h.params[t, 0, mem], h.params[t, 1, mem], h.value[t, mem]] + [h.sim_moments[t, k, mem] for k in range(3)]
            for s, x in enumerate(cols):
                w = TR.column_stats(x, probs)
                got_s = (got["mean"][i, g, s], got["var"][i, g, s], got["median"][i, g, s])
                assert np.array_equal(np.array(got_s), np.array(w[:3], float), equal_nan=True)
                assert np.array_equal(got["quantile"][:, i, g, s], w[3], equal_nan=True)
            assert got["count"][i, g] == len(mem)


def test_ctypes_layout_matches_the_header():
    names = [f for f, _ in A.smm_trace_t._fields_]
    assert names == ["iter", "n_chains", "count", "n_accepted", "n_exchanged", "n_failed", "mean", "var", "median", "quantile",
                     "best_value", "best_chain"]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "smmhip.h"', "int main(void) {",
             'printf("size %zu\\n", sizeof(smm_trace_t));']
    lines += ['printf("%s %%zu\\n", offsetof(smm_trace_t, %s));' % (f, f) for f in names]
    lines.append("return 0; }")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "p.c"), "-o", os.path.join(d, "p")])
        out = dict(l.rsplit(" ", 1) for l in subprocess.check_output([os.path.join(d, "p")]).decode().strip().splitlines())
    assert int(out["size"]) == C.sizeof(A.smm_trace_t)
    for f in names:
        assert getattr(A.smm_trace_t, f).offset == int(out[f]), f
    argtypes = dict((n, a) for n, _, a in A.SYMBOLS)["smm_get_trace"]
    assert argtypes == [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, A.c_int32_p, C.c_int32, A.c_double_p, C.c_int32,
                        C.POINTER(A.smm_trace_t)]
    assert hasattr(A.load(), "smm_get_trace")
