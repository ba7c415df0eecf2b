"""smm_opt_simplex (include/smmhip.h), CPU tier: the contract's restatement (tests/simplex_ref.py) pinned to scipy's own Nelder–Mead before the
device is compared with it (tests/test_gpu_opt_simplex.py); the five moves, the stop without a finite value and the stable sort on an
objective with holes; the independence of the searches; the ABI."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import common as cm  # noqa: E402,F401  (path set-up)
import simplex_ref as sxr  # noqa: E402

import smm_jl_amd as S  # noqa: E402
from smm_jl_amd import _abi as A  # noqa: E402


def banana(P):
    """the banana objective's formula (value = sum_{i < np - 1} 100 (x_{i+1} - x_i^2)^2 + (1 - x_i)^2) over P [np][n]; one parameter has no
    such term: (1 - x_0)^2 then"""
    P = np.asarray(P, float)
    if P.shape[0] == 1:
        v = (1.0 - P[0]) ** 2
    else:
        v = np.zeros(P.shape[1])
        for i in range(P.shape[0] - 1):
            v = v + (100.0 * (P[i + 1] - P[i] * P[i]) ** 2 + (1.0 - P[i]) ** 2)
    return v, np.stack([P.sum(0), v]), np.ones(P.shape[1], np.int8)


# ---- 1. the restatement is scipy's bounded Nelder–Mead, bit for bit ----------------------------------------------------------------------
PIN_NP = (1, 2, 5, 10, 15)
PIN_STEP, PIN_XATOL, PIN_FATOL, PIN_MAX_ITER = 0.05, 1e-3, 1e-3, 150


def pin_cases():
    """per np and coefficient set: four random interior starts, and one within `step` of the upper bound in some coordinates"""
    rng = np.random.default_rng(11)
    cases = []
    for N in PIN_NP:
        lb, ub = np.full(N, -2.0), np.linspace(2.0, 3.0, N)
        st = rng.uniform(lb[:, None] + 0.1, (ub - PIN_STEP * (ub - lb))[:, None] - 0.1, (N, 5))
        st[::2, 4] = (ub - 0.3 * PIN_STEP * (ub - lb))[::2]      # y = x + step * range passes ub: reflected back inside, to ub - 0.7 step * range
        if N > 1:
            st[1, 4] = ub[1]                                     # on the bound itself: reflected to ub - step * range
        for adaptive in (False, True):
            cases.append((N, adaptive, lb, ub, st))
    return cases


@pytest.fixture(scope="module")
def pinned():
    return [(c, sxr.opt_simplex(banana, c[4], c[2], c[3], 2, PIN_STEP, c[1], PIN_XATOL, PIN_FATOL, PIN_MAX_ITER)) for c in pin_cases()]


def test_the_restatement_is_scipys_nelder_mead_bit_for_bit(pinned):
    so = pytest.importorskip("scipy.optimize", reason="scipy is the reference this restatement is pinned to")
    # a condition on the cases, asserted on the restatement alone before anything is compared: scipy's argsort is not stable, so a search
    # in which a sort saw equal values is left out — at most one in ten
    n_all = sum(c[4].shape[1] for c, _ in pinned)
    n_ties = sum(int(r["ties"].sum()) for _, r in pinned)
    assert n_all == 50 and 10 * n_ties <= n_all, (n_ties, n_all)
    seen_reflected_start = False
    stops = set()
    for (N, adaptive, lb, ub, st), r in pinned:
        for s in range(st.shape[1]):
            if r["ties"][s]:
                continue
            raw = sxr.initial_simplex(st[:, s], lb, ub, PIN_STEP, reflect=False)
            seen_reflected_start |= bool((raw > ub).any())
            res = so.minimize(lambda x: float(banana(x[:, None])[0][0]), st[:, s], method="Nelder-Mead", bounds=list(zip(lb, ub)),
                              options=dict(initial_simplex=raw, xatol=PIN_XATOL, fatol=PIN_FATOL, maxiter=PIN_MAX_ITER + 1, maxfev=np.inf,
                                           adaptive=adaptive))
            sim, fsim = res.final_simplex
            where = (N, adaptive, s)
            assert np.array_equal(sim, r["simplex"][:, :, s]), where
            assert np.array_equal(fsim, r["simplex_value"][:, s]), where
            assert res.nit == r["iterations"][s] + 1 and res.nfev == r["n_eval"][s], where
            assert np.array_equal(res.x, r["best"][:, s]) and res.fun == r["value"][s], where
            assert (res.status == 0) == (r["status"][s] == 1) and r["status"][s] in (0, 1), where
            stops.add(int(r["status"][s]))
    assert seen_reflected_start and stops == {0, 1}      # (both ways to stop were pinned)


def test_the_pinned_cases_take_every_move_but_the_shrink(pinned):
    total = sum(r["moves"].sum(1) for _, r in pinned)
    assert (total[:4] > 0).all(), total
    for _, r in pinned:
        assert np.array_equal(r["moves"].sum(0), r["iterations"])
        assert r["evaluated"] == r["n_eval"].sum()


# ---- 2. holes: +inf bands, a NaN band, a flat region -------------------------------------------------------------------------------------
def holes(P):
    """tests/test_gpu_opt_slices.py's objective in numpy: a bowl around (0.3, -0.4), flat in y inside |y + 0.4| < 0.25, +inf on a band of x, NaN
    on a band of y, nothing finite for x > 1.5; the status says "failed" left of x = -1.5"""
    x, y = np.asarray(P, float)
    ay = np.abs(y + 0.4)
    v = (x - 0.3) * (x - 0.3) + np.where(ay < 0.25, 0.0, ay - 0.25)
    v = np.where((x > -1.2) & (x < -0.9), np.inf, v)
    v = np.where((y > 0.9) & (y < 1.3), np.nan, v)
    v = np.where(x > 1.5, np.where(y > 0.0, np.nan, np.inf), v)
    return v, np.stack([x + y, x * y - 0.5]), np.where(x < -1.5, -2, 1).astype(np.int8)


def holes_starts():
    rng = np.random.default_rng(3)
    st = rng.uniform(-2, 1.4, (2, 11))
    st[:, 0] = [0.3, -0.4]      # at the optimum, in the flat band: ties
    st[:, 1] = [1.7, 1.0]       # nothing finite at any vertex
    st[:, 2] = [0.0, 1.1]       # starts in the NaN band
    st[:, 3] = [-1.9, -2.0]     # status -2 at perfectly good values
    return st


LB2, UB2 = [-2.0, -2.0], [2.0, 2.0]


def test_every_move_occurs_and_nothing_finite_stops_with_status_2():
    st = holes_starts()
    r = sxr.opt_simplex(holes, st, LB2, UB2, 2, 0.05, False, 1e-6, 1e-6, 80)
    assert (r["moves"].sum(1) > 0).all(), r["moves"].sum(1)      # reflection, expansion, both contractions, shrink
    assert r["status"][1] == 2 and r["n_eval"][1] == 3 and r["iterations"][1] == 0 and not np.isfinite(r["value"][1])
    assert np.isnan(r["size_x"][1]) and np.isnan(r["size_f"][1]) and np.array_equal(r["best"][:, 1], st[:, 1])
    assert set(r["status"]) == {0, 1, 2} and r["ties"].any()
    assert np.isfinite(r["value"][2]) and np.isfinite(r["value"][3]) and r["best"][0, 3] > -1.5      # the misleading status is ignored
    for s in np.flatnonzero(r["status"] != 2):
        f = r["simplex_value"][:, s]
        key = np.where(np.isnan(f), np.inf, f)
        assert (key[1:] >= key[:-1]).all() and not (np.isnan(f[:-1]) & ~np.isnan(f[1:])).any()      # ascending, +inf before NaN
    assert np.array_equal(r["moves"].sum(0), r["iterations"]) and r["evaluated"] == r["n_eval"].sum()


def test_the_evaluation_count_follows_the_moves():
    """a reflection costs one evaluation or two (a failed expansion), expansion and contractions two, a shrink 2 + N"""
    r = sxr.opt_simplex(holes, holes_starts(), LB2, UB2, 2, 0.05, False, 1e-6, 1e-6, 80)
    lo = 3 + r["moves"][0] + 2 * r["moves"][1:4].sum(0) + 4 * r["moves"][4]
    assert (r["n_eval"] >= lo).all() and (r["n_eval"] <= lo + r["moves"][0]).all()


def test_ties_resolve_stably():
    """equal values keep their current order: on a constant objective the initial order survives the first sort and every reflection (fxr <
    fsim[0] and every other < fail: inside contraction fails, shrink) leaves vertex 0 in place"""
    f = np.array([3.0, np.nan, 1.0, np.inf, 1.0, np.nan, -np.inf, 3.0, np.inf])
    order, ties = sxr.sort_key(f)
    assert list(order) == [6, 2, 4, 0, 7, 3, 8, 1, 5] and ties
    assert not sxr.sort_key(np.array([2.0, 1.0, np.nan, np.inf]))[1] and sxr.sort_key(np.array([np.nan, 1.0, np.nan]))[1]
    flat = lambda P: (np.zeros(P.shape[1]), np.asarray(P, float)[:2], np.ones(P.shape[1], np.int8))      # noqa: E731
    st = np.array([[0.5], [-0.5]])
    r = sxr.opt_simplex(flat, st, LB2, UB2, 2, 0.05, False, 1e-3, 1e-3, 30)
    assert r["ties"][0] and np.array_equal(r["best"][:, 0], st[:, 0]) and np.array_equal(r["sim_moments"][:, 0], st[:, 0])
    assert r["moves"][4, 0] == r["iterations"][0] > 0 and r["status"][0] == 1      # every iteration shrinks towards the start, until xatol


def test_the_searches_are_independent():
    """a search gives the same alone as among others, whatever stops around it"""
    st = holes_starts()
    both = sxr.opt_simplex(holes, st, LB2, UB2, 2, 0.05, True, 1e-6, 1e-6, 40)
    for s in (0, 1, 5, 10):
        one = sxr.opt_simplex(holes, st[:, s:s + 1], LB2, UB2, 2, 0.05, True, 1e-6, 1e-6, 40)
        for f in sxr.FIELDS:
            assert np.array_equal(one[f][..., 0], both[f][..., s], equal_nan=True), (f, s)


def test_the_coefficients():
    assert sxr.coefficients(7, False) == (1, 2, 0.5, 0.5)
    assert sxr.coefficients(10, True) == (1, 1 + 2 / 10.0, 0.75 - 1 / 20.0, 1 - 1 / 10.0)
    assert sxr.coefficients(1, True) == (1, 3.0, 0.25, 0.0)


# ---- 3. the ABI ------------------------------------------------------------------------------------------------------------------------------
def test_the_struct_and_the_prototype_are_the_headers():
    names = [f[0] for f in A.smm_opt_simplex_t._fields_]
    assert names == ["best", "value", "sim_moments", "simplex", "simplex_value", "size_x", "size_f", "iterations", "status", "moves", "n_eval",
                     "evaluated"]
    assert C.sizeof(A.smm_opt_simplex_t) == 12 * 8
    sym = dict((s[0], s) for s in A.SYMBOLS)["smm_opt_simplex"]
    assert sym[1] is C.c_int and len(sym[2]) == 9 and sym[2][3] is C.c_double and sym[2][4] is C.c_int32
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "smmhip.h")).read()
    body = header[header.index("smm_opt_slices_t;"):header.index("} smm_opt_simplex_t;")]
    body = body[body.rindex("typedef struct"):]
    declared = [line.split(";")[0].split()[-1] for line in body.splitlines()[1:] if ";" in line]
    assert declared == names
    assert hasattr(S, "optSimplexDevice") and "method" in S.polish.__code__.co_varnames
