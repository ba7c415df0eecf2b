"""smm_opt_slices (include/smmhip.h), CPU tier: the contract's restatement (tests/opt_slices_ref.py) pinned to callers.optSlices and to
numpy's linspace before the device is compared with it (tests/test_gpu_opt_slices.py), the independence of the searches, and the ABI."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import common as cm  # noqa: E402,F401  (path set-up)
import opt_slices_ref as osr  # noqa: E402
from test_callers import linear_evaluator, toy_problem  # noqa: E402

import smm_jl_amd as S  # noqa: E402
from smm_jl_amd import _abi as A  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def toy_restated(m, npoints, tol, update, max_cycles=1000):
    names = S.ps2s_names(m)
    lb = [m.params_to_sample[k]["lb"] for k in names]
    ub = [m.params_to_sample[k]["ub"] for k in names]
    start = np.array([[m.initial_value[k]] for k in names], float)
    return osr.opt_slices(lambda P: linear_evaluator(m, P), start, lb, ub, 3, npoints, tol, update, max_cycles)


@pytest.mark.parametrize("update", [0.5, None])
def test_one_search_from_initial_value_is_callers_optSlices(update):
    m = toy_problem()
    tol, G = 1e-3, 41
    r = toy_restated(m, G, tol, update)
    n = int(r["cycles"][0])
    assert n >= 2 and r["converged"][0] == 1
    # np.linalg.norm sums in BLAS order, the contract left to right: the two may differ in the last bits, so the stopping decisions of
    # the cases compared here must not hang on them — delta of the last two cycles is not within a few ulp of tol
    for cycles in (n - 1, n):
        d = toy_restated(m, G, tol, update, max_cycles=cycles)["delta"][0]
        assert abs(d - tol) > 8 * np.spacing(tol), (cycles, d)
    out = S.optSlices(m, G, tol=tol, update=update, evaluator=linear_evaluator)
    assert [out["best"]["p"]["a"], out["best"]["p"]["b"]] == [r["best"][0, 0], r["best"][1, 0]]
    assert out["best"]["value"] == r["value"][0] and out["iterations"] == n and out["converged"] is True
    assert r["evaluated"] == G * 2 * n and np.isnan(r["cycle_value"][n:, 0]).all() and r["cycle_value"][n - 1, 0] == r["value"][0]
    res = S.callers.opt_results(m, r)
    assert res == [{"best": out["best"], "iterations": out["iterations"], "converged": out["converged"]}]


def test_a_search_cut_by_max_cycles_is_callers_optSlices_cut_by_maxiter():
    m = toy_problem()
    r = toy_restated(m, 41, 1e-3, 0.5, max_cycles=2)
    out = S.optSlices(m, 41, tol=1e-3, update=0.5, evaluator=linear_evaluator, maxiter=2)
    assert out["iterations"] == 2 == r["cycles"][0] and out["converged"] is False and r["converged"][0] == 0
    assert [out["best"]["p"]["a"], out["best"]["p"]["b"]] == list(r["best"][:, 0]) and out["best"]["value"] == r["value"][0]


@pytest.mark.parametrize("G", [2, 3, 5, 16, 41, 100])
def test_the_grid_is_numpys_linspace_bit_for_bit(G):
    rng = np.random.default_rng(G)
    lo = np.concatenate([[0.1, -1 / 3, 1e-300, -2.0, 0.7, 1e15 / 3, 5e-324, 0.0, -0.0, 1 / 3], rng.uniform(-10, 10, 200) / 3])
    hi = np.concatenate([[0.3, 2 / 3, 3e-300, 2.0, 0.7, 1e15 / 3 + 0.5, 1.5e-323, 5e-324, 0.0, 1 / 3], lo[10:] + rng.uniform(0, 7, 200) / 7])
    X = osr.grid(lo, hi, G)
    zero_steps = 0
    for s in range(len(lo)):
        want = np.linspace(lo[s], hi[s], G)
        assert np.array_equal(X[:, s], want), (s, lo[s], hi[s])
        assert X[G - 1, s] == hi[s]
        zero_steps += (hi[s] - lo[s]) / (G - 1) == 0
    assert zero_steps >= 3   # (collapsed ranges lo == hi, and a denormal range whose step rounds to zero, among the cases)
    if G > 2:
        assert zero_steps >= 4 and np.array_equal(X[:, 7], np.linspace(0.0, 5e-324, G))


def holes_evaluator(P):
    """a bowl around (0.3, -0.4) with +inf on a band of x, NaN on a band of y, flat in y inside |y + 0.4| < 0.25 (ties) and nothing finite
    at all for x > 1.5"""
    x, y = P
    yy = np.where(np.abs(y + 0.4) < 0.25, 0.0, np.abs(y + 0.4) - 0.25)
    v = (x - 0.3) ** 2 + yy
    v = np.where((x > -1.2) & (x < -0.9), np.inf, v)
    v = np.where((y > 0.9) & (y < 1.3), np.nan, v)
    v = np.where(x > 1.5, np.where(y > 0, np.nan, np.inf), v)
    return v, np.stack([x + y, v]), np.ones(P.shape[1], np.int8)


HOLES_LB, HOLES_UB = [-2.0, -2.0], [2.0, 2.0]


def holes_starts():
    rng = np.random.default_rng(3)
    st = rng.uniform(-2, 1.4, (2, 11))
    st[:, 0] = [0.3, -0.4]      # on a grid-free optimum: converges at once or nearly
    st[:, 1] = [1.9, 1.0]       # nothing finite anywhere along x at y in the NaN band; along y: x > 1.5, nothing finite
    st[:, 2] = [0.0, 1.1]       # the first coordinate step (along x at y = 1.1) sees no finite value, the second does
    return st


@pytest.mark.parametrize("update,G", [(0.5, 7), (None, 6)])
def test_search_s_of_a_K_start_run_is_the_one_start_run_from_that_start(update, G):
    st = holes_starts()
    r = osr.opt_slices(holes_evaluator, st, HOLES_LB, HOLES_UB, 2, G, 1e-4, update, 12)
    assert len(set(r["cycles"])) >= 3   # searches drop out at different cycles: the others must not notice
    assert r["value"][1] == np.inf and np.isnan(r["sim_moments"][:, 1]).all() and np.array_equal(r["best"][:, 1], st[:, 1])
    assert np.isfinite(r["value"][2]) and r["best"][1, 2] != st[1, 2]
    total = 0
    for s in range(st.shape[1]):
        one = osr.opt_slices(holes_evaluator, st[:, s:s + 1], HOLES_LB, HOLES_UB, 2, G, 1e-4, update, 12)
        for f in osr.FIELDS:
            assert np.array_equal(one[f][..., 0], r[f][..., s], equal_nan=one[f].dtype.kind == "f"), (f, s)
        total += one["evaluated"]
    assert total == r["evaluated"] == G * 2 * int(r["cycles"].sum())


def test_ties_go_to_the_lowest_grid_point():
    st = np.array([[0.3], [-2.0]])
    r = osr.opt_slices(holes_evaluator, st, HOLES_LB, HOLES_UB, 2, 33, 1e-4, None, 1)   # y grid step 0.125: -0.625, -0.5, -0.375, -0.25 are flat
    bx = r["best"][0, 0]
    assert bx == 0.25 and r["best"][1, 0] == -0.625 and r["value"][0] == (bx - 0.3) ** 2
    assert r["delta"][0] == np.sqrt((0.3 - bx) * (0.3 - bx) + (-2.0 + 0.625) * (-2.0 + 0.625))


def test_symbol_and_layout_match_the_header():
    names = dict((s[0], s) for s in A.SYMBOLS)
    assert names["smm_opt_slices"][1:] == (C.c_int, [C.c_void_p, A.c_double_p, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_int32,
                                                     C.POINTER(A.smm_opt_slices_t)])
    for lib in (A.load(), A.load_hooks()):
        assert hasattr(lib, "smm_opt_slices")
    fields = [f for f, _ in A.smm_opt_slices_t._fields_]
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "smmhip.h"
#define O(T, f) printf(#f " %zu\n", offsetof(T, f))
#ifdef CHECK_PROTOTYPES
int (*f1)(void*, const double*, int32_t, int32_t, double, double, int32_t, smm_opt_slices_t*) = smm_opt_slices;
#endif
int main(void) {
  printf("sizeof %zu\n", sizeof(smm_opt_slices_t));
  ''' + " ".join("O(smm_opt_slices_t, %s);" % f for f in fields) + r'''
  printf("abi %d\n", SMMHIP_ABI_VERSION);
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(prog)
        inc = ["-I", os.path.join(ROOT, "include")]
        subprocess.check_call(["gcc", "-Werror", "-DCHECK_PROTOTYPES", "-c"] + inc + [os.path.join(d, "p.c"), "-o", os.path.join(d, "p.o")])   # the arity
        subprocess.check_call(["gcc"] + inc + [os.path.join(d, "p.c"), "-o", os.path.join(d, "p")])
        out = dict(l.rsplit(" ", 1) for l in subprocess.check_output([os.path.join(d, "p")]).decode().strip().splitlines())
    assert int(out["sizeof"]) == C.sizeof(A.smm_opt_slices_t) and int(out["abi"]) == 3
    assert fields == ["best", "value", "sim_moments", "lo", "hi", "delta", "cycle_value", "cycles", "converged", "evaluated"]
    for f in fields:
        assert getattr(A.smm_opt_slices_t, f).offset == int(out[f]), f


def test_the_call_refuses_a_null_context():
    lib = A.load()
    st = np.zeros((2, 1))
    assert lib.smm_opt_slices(None, A.dptr(st), 1, 5, 1e-5, float("nan"), 10, None) == A.SMM_ERR_INVALID_ARG
