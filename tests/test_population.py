"""The starting population (include/smmhip.h: smm_set_population, smm_scatter_population), CPU tier: the contract's candidates, the
selection rules, and the reference of tests/population_ref.py pinned to the existing first iteration before the device is compared
with it (tests/test_gpu_population.py)."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import common as cm  # noqa: E402
import population_ref as pr  # noqa: E402

from smm_jl_amd import _abi as A  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def failbox_case(S):
    """objfunc_norm that fails for theta_0 in [1, 3]: initial_value (0.2) is valid, a candidate of the whole box fails about one time in three"""
    return cm.serial_normal(N=70, T=20, ns=1000, seed=12, objective_id=S._abi.SMM_OBJ_NORM_FAILBOX, obj_params=[1.0, 3.0])


def all_fail_case(S):
    """initial_value at the lower bound of theta_0, the box everything above it: every candidate fails, initial_value does not"""
    prob, opts = cm.serial_normal(N=70, T=20, ns=1000, seed=12, objective_id=S._abi.SMM_OBJ_NORM_FAILBOX, obj_params=[-3.0 + 1e-9, 3.0])
    prob.init[:] = [-3.0, -0.2]
    return prob, opts


def assert_run_equal(a, b, t1):
    cm.assert_history_equal(a.history(0, t1), b.history(0, t1), exact_floats=True)
    cm.assert_state_equal(a.state(), b.state(), rtol=0)


@pytest.mark.parametrize("spread", [1.0, 0.25])
def test_candidates_lie_in_the_box_and_in_the_spread_box(S, O, spread):
    prob, opts = cm.general_normal(5, N=6, T=4)
    prob.init[0], prob.init[1] = prob.lb[0], prob.ub[1]     # at a bound; the others inside
    prob.init[2] = 0.5 * (prob.lb[2] + prob.ub[2])          # the centre
    th = pr.candidates(O, prob, opts, 40, spread)
    lb, ub = prob.lb[:, None, None], prob.ub[:, None, None]
    assert (th >= lb).all() and (th <= ub).all()
    x01 = (th - lb) / (ub - lb)
    c = ((prob.init - prob.lb) / (prob.ub - prob.lb))[:, None, None]
    assert (np.abs(x01 - c) <= spread / 2 + 1e-12).all()
    # clipped at the edges: from the lower bound only upwards, by at most spread / 2; from the centre both ways
    assert x01[0].min() >= 0 and x01[0].max() <= spread / 2 + 1e-12 and x01[0].max() > 0.8 * spread / 2
    assert x01[1].max() <= 1 and x01[1].min() >= 1 - spread / 2 - 1e-12
    assert x01[2].min() < 0.5 - 0.4 * spread and x01[2].max() > 0.5 + 0.4 * spread
    if spread == 1.0:
        assert x01[2].min() < 0.1 and x01[2].max() > 0.9    # the whole box around a centred init
    assert len(np.unique(th[3])) == th[3].size              # chains and candidates all differ


def test_candidates_of_a_chain_do_not_depend_on_the_shard(S, O):
    prob, opts = cm.general_normal(3, N=8, T=4)
    whole = pr.candidates(O, prob, opts, 5, 0.5)
    _, shard = cm.general_normal(3, N=8, T=4, N_local=3, chain_offset=4)
    assert np.array_equal(pr.candidates(O, prob, shard, 5, 0.5), whole[:, 4:7])
    _, more = cm.general_normal(3, N=20, T=4)
    assert np.array_equal(pr.candidates(O, prob, more, 5, 0.5)[:, :8], whole)
    # the draws are the contract's: stream 7, counter {g, m, k >> 1, 0}, the first word pair for even k, the second for odd k
    x = O.philox([6, 2, 1, 0], [opts.seed & 0xffffffff, ((opts.seed >> 32) ^ (7 * 0x9E3779B9)) & 0xffffffff])
    u = pr.unit_draws(O, opts.seed, 6, 5, 3)
    assert u[2, 2] == float(((x[0] << 32) | x[1]) >> 11) * 2.0 ** -53 and ((u >= 0) & (u < 1)).all()


def test_the_reference_install_reproduces_the_first_iteration(S, O):
    """starts = the broadcast initial_value: the installed state is the oracle's own first iteration, and the 19 after it agree"""
    for prob, opts in (cm.serial_normal(N=70, T=20, ns=1000), failbox_case(S), cm.general_normal(5, N=9, T=20, ns=300)):
        plain = O.OracleContext(prob, opts)
        plain.step(1)
        starts = np.repeat(prob.init[:, None], opts.N, axis=1)
        o, r = pr.set_population(O, prob, opts, None, starts)
        assert o.state().iter == 1 and r["evaluated"] == opts.N
        assert_run_equal(o, plain, 1)
        plain.step(19); o.step(19)
        assert_run_equal(o, plain, 20)
        hh = o.history(0, 20)
        assert hh.accepted[1:].any() and (hh.exchanged != 0).any()


def test_selection_rules_on_a_hand_made_table():
    nan, inf = np.nan, np.inf
    v = np.array([[3.0, 1.0, 1.0, 2.0],      # a tie: the lowest m
                  [nan, 5.0, -1.0, 4.0],     # NaN and negative values are skipped
                  [0.5, 0.4, 0.3, 0.2],      # status decides before the value
                  [nan, -2.0, inf, 1.0],     # nothing valid
                  [2.0, 2.0, 2.0, 2.0],      # equal to initial_value
                  [9.0, 8.0, 7.0, 0.0],
                  [1.0, 0.0, -0.0, 0.0],     # -0.0 ties +0.0: the lowest m, whatever its sign
                  [1.0, -0.0, 0.0, 2.0 ** -1074],
                  [0.1, 0.5, 0.3, 0.2]])     # status 0 is as invalid as -2; status 2 is valid
    st = np.array([[1, 1, 1, 1], [1, 1, 1, 1], [1, -2, -2, -2], [1, 1, 1, -2], [1, 1, 1, 1], [1, 1, 1, 1], [1, 1, 1, 1], [1, 1, 1, 1],
                   [0, 1, 2, -2]])
    assert pr.select(v, st, 2.0, 1, False).tolist() == [1, 3, 0, -1, 0, 3, 1, 1, 2]
    assert pr.select(v, st, 2.0, 1, True).tolist() == [1, -1, 0, -1, -1, 3, 1, 1, 2]      # initial_value wins ties and whatever is worse
    assert pr.select(v, st, 2.0, -2, True).tolist() == [1, 3, 0, -1, 0, 3, 1, 1, 2]       # an invalid initial_value does not compete ...
    assert pr.select(v, st, nan, 1, True).tolist() == [1, 3, 0, -1, 0, 3, 1, 1, 2]
    assert pr.select(v, st, 2.0, 0, True).tolist() == [1, 3, 0, -1, 0, 3, 1, 1, 2]        # (status 0)
    assert pr.select(v, st, 0.0, 1, True).tolist() == [-1, -1, -1, -1, -1, -1, -1, -1, -1]   # +0.0 ties -0.0 and wins the tie
    assert pr.select(v, st, -0.0, 1, True).tolist() == [-1, -1, -1, -1, -1, -1, -1, -1, -1]
    assert pr.select(v[3:4], st[3:4], -1.0, -2, False).tolist() == [-1]          # ... but is the start when nothing else is valid


def test_invalid_candidates_show_both_outcomes_in_the_reference(S, O):
    prob, opts = failbox_case(S)
    o, r, (v, st) = pr.scatter_population(O, prob, opts, None, 1, 1.0, False)
    failed = st[:, 0] < 1
    assert failed.sum() >= 5 and (~failed).sum() >= 5
    assert np.array_equal(r["pick"], np.where(failed, -1, 0))
    assert np.array_equal(r["start"][:, failed], np.repeat(prob.init[:, None], failed.sum(), axis=1))
    assert (r["start"][0, ~failed] < 1.0).all() and r["evaluated"] == 71
    prob, opts = all_fail_case(S)
    o, r, (v, st) = pr.scatter_population(O, prob, opts, None, 3, 0.25, False)
    assert (st == -2).all() and (r["pick"] == -1).all()
    plain = O.OracleContext(prob, opts)
    plain.step(20); o.step(19)
    assert_run_equal(o, plain, 20)


def test_symbols_and_layout_match_the_header():
    names = dict((s[0], s) for s in A.SYMBOLS)
    assert names["smm_set_population"][1:] == (C.c_int, [C.c_void_p, A.c_double_p, C.POINTER(A.smm_population_t)])
    assert names["smm_scatter_population"][1:] == (C.c_int, [C.c_void_p, C.c_int32, C.c_double, C.c_int32, C.POINTER(A.smm_population_t)])
    for lib in (A.load(), A.load_hooks()):
        assert hasattr(lib, "smm_set_population") and hasattr(lib, "smm_scatter_population")
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "smmhip.h"
#define O(T, f) printf(#f " %zu\n", offsetof(T, f))
#ifdef CHECK_PROTOTYPES
int (*f1)(void*, const double*, smm_population_t*) = smm_set_population;
int (*f2)(void*, int32_t, double, int32_t, smm_population_t*) = smm_scatter_population;
#endif
int main(void) {
  printf("sizeof %zu\n", sizeof(smm_population_t));
  O(smm_population_t, start); O(smm_population_t, value); O(smm_population_t, pick); O(smm_population_t, evaluated);
  printf("abi %d\n", SMMHIP_ABI_VERSION);
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(prog)
        inc = ["-I", os.path.join(ROOT, "include")]
        subprocess.check_call(["gcc", "-Werror", "-DCHECK_PROTOTYPES", "-c"] + inc + [os.path.join(d, "p.c"), "-o", os.path.join(d, "p.o")])   # the arities
        subprocess.check_call(["gcc"] + inc + [os.path.join(d, "p.c"), "-o", os.path.join(d, "p")])
        out = dict(l.rsplit(" ", 1) for l in subprocess.check_output([os.path.join(d, "p")]).decode().strip().splitlines())
    assert int(out["sizeof"]) == C.sizeof(A.smm_population_t) and int(out["abi"]) == 3
    for f in ("start", "value", "pick", "evaluated"):
        assert getattr(A.smm_population_t, f).offset == int(out[f]), f


def test_the_calls_refuse_a_null_context():
    lib = A.load()
    assert lib.smm_set_population(None, None, None) == A.SMM_ERR_INVALID_ARG
    assert lib.smm_scatter_population(None, 4, 1.0, 1, None) == A.SMM_ERR_INVALID_ARG
