"""The generic user objective (user_objective_src.GENERIC_*) in the oracle against its numpy restatement, across parameter, moment and
partial-sum counts; and the oracle's table of user objectives, which must refuse a handle it cannot hold.  CPU only."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from user_objective_src import AR1_SOURCE, GENERIC_LANES_SOURCE, GENERIC_SOURCE, dyadic_thetas, generic_moments, generic_numpy  # noqa: E402

SHAPES = [(1, 1), (3, 64), (64, 1), (64, 64)]   # (np, nm)
FAIL_ABOVE = 0.375
_hooked = {}


def oracle_only(O, source, n_sums=None, lanes=256):
    """an oracle-only handle from the top of the oracle's table (the library hands out its handles from the bottom): built once per
    (source, form), hooked again at every use (another test may have taken the same handle meanwhile)"""
    key = (source, n_sums, lanes)
    if key not in _hooked:
        oid = 1000 + O.load().orc_max_user() - 1 - len(_hooked)
        _hooked[key] = (oid, C.CDLL(O.register_user_objective(source, oid, n_sums=n_sums, lanes=lanes)))
    oid, lib = _hooked[key]
    O.hook_user_objective(lib, oid, n_sums, lanes)
    return oid


def generic_problem(S, oid, np_, nm, A, n_sums):
    mom, w = generic_moments(nm)
    return S.Problem(init=np.zeros(np_), lb=-np.ones(np_), ub=np.ones(np_), mom=mom, w=w, ns=1, objective_id=oid,
                     obj_params=[float(A), FAIL_ABOVE, float(n_sums)])


def one_opts(S):
    return S.BGPOpts(N=1, maxiter=1, sigma=[0.05], acc_tuner=[1.0], min_improve=[0.0])


def check_against_restatement(O, S, oid, n_sums, A):
    for np_, nm in SHAPES:
        prob = generic_problem(S, oid, np_, nm, A, n_sums)
        th = dyadic_thetas(np_, 40, seed=np_ * 100 + nm, last_above=FAIL_ABOVE)
        v, sm, st = O.OracleContext(prob, one_opts(S)).eval_batch(th)
        vr, smr, str_ = generic_numpy(th, prob.mom, prob.w, prob.obj_params, n_sums)
        assert np.array_equal(st, str_), (np_, nm)
        assert np.array_equal(sm, smr, equal_nan=True), (np_, nm)
        assert np.array_equal(v, vr), (np_, nm)
        assert (st == -2).any() and (st == 1).any() and np.isnan(sm[nm - 1, st == -2]).all()
        assert len(np.unique(v[st == 1])) > 1


@pytest.mark.parametrize("n_sums", [1, 17, 64])
def test_one_thread_generic_objective_equals_its_restatement(O, S, n_sums):
    oid = oracle_only(O, GENERIC_SOURCE)
    check_against_restatement(O, S, oid, n_sums, A=37)


@pytest.mark.parametrize("lanes", [64, 1024])
@pytest.mark.parametrize("n_sums", [1, 17, 64])
def test_map_reduce_generic_objective_equals_its_restatement(O, S, n_sums, lanes):
    # A = 1500 is a multiple of neither lane count: the lanes' shares of units differ (at 1024 lanes, by one or two units, some none)
    oid = oracle_only(O, GENERIC_LANES_SOURCE, n_sums=n_sums, lanes=lanes)
    check_against_restatement(O, S, oid, n_sums, A=1500)


def test_restatement_is_not_blind_to_the_sums(O, S):
    # the restatement with one sum fewer, or with the sums' parameter held at theta[0], differs from the oracle where the shape reaches it
    oid = oracle_only(O, GENERIC_SOURCE)
    prob = generic_problem(S, oid, 3, 64, 37, 17)
    th = dyadic_thetas(3, 20, seed=5)
    v, sm, st = O.OracleContext(prob, one_opts(S)).eval_batch(th)
    assert not np.array_equal(sm, generic_numpy(th, prob.mom, prob.w, prob.obj_params, 16)[1], equal_nan=True)
    th0 = th.copy()
    th0[1:] = th[:1]
    assert not np.array_equal(sm, generic_numpy(th0, prob.mom, prob.w, prob.obj_params, 17)[1], equal_nan=True)


def test_the_oracle_refuses_handles_past_its_table(O, S):
    lib = O.load()
    n = lib.orc_max_user()
    assert n == 64
    fn = C.c_void_p(1)   # (never called: the handle is refused before it is stored)
    for oid in (999, 1000 + n, 1000 + n + 5, -3):
        assert lib.orc_set_user_objective(oid, fn) == -1, oid
        assert lib.orc_set_user_objective_lanes(oid, fn, fn, 3, 64) == -1, oid
        with pytest.raises(ValueError, match="outside the oracle's table"):
            O.register_user_objective(AR1_SOURCE, oid)
        with pytest.raises(ValueError, match="outside the oracle's table"):
            O.register_user_objective(GENERIC_LANES_SOURCE, oid, n_sums=3, lanes=64)
    # the last handle it holds still works, and is what evaluates
    oid = 1000 + n - 1
    O.register_user_objective(GENERIC_SOURCE, oid)
    prob = generic_problem(S, oid, 2, 3, 5, 3)
    th = dyadic_thetas(2, 4, seed=1)
    v, sm, st = O.OracleContext(prob, one_opts(S)).eval_batch(th)
    assert np.array_equal(v, generic_numpy(th, prob.mom, prob.w, prob.obj_params, 3)[0])


def test_the_rng_shim_refuses_handles_past_the_table(O):
    from user_rng_src import Shim
    from user_objective_src import GENERIC_RNG_SOURCE
    shim = Shim(O, GENERIC_RNG_SOURCE)
    with pytest.raises(ValueError, match="outside the oracle's table"):
        shim.hook(O, 1000 + O.load().orc_max_user(), 7)


def test_a_handle_registered_again_takes_its_new_form(O, S):
    # one handle: the map-reduce form, then a one-thread objective, then the map-reduce form again — what evaluates is the one registered last
    from user_objective_src import ar1_numpy
    from test_user_objective import ar1_problem
    oid = 1000 + O.load().orc_max_user() - 1
    prob = generic_problem(S, oid, 3, 5, 1500, 3)
    th = dyadic_thetas(3, 6, seed=2)
    pa, oa = ar1_problem(S, oid, N=1, T=1)
    tha = np.array([[0.2, -0.4], [1.0, 0.5]])
    for step in range(3):
        if step == 1:
            O.register_user_objective(AR1_SOURCE, oid)
            v, sm, st = O.OracleContext(pa, oa).eval_batch(tha)
            for i in range(2):
                assert np.allclose(sm[:, i], ar1_numpy(tha[:, i], pa.mom, pa.w, pa.obj_params)[0], rtol=1e-13, atol=1e-15)
        else:
            O.register_user_objective(GENERIC_LANES_SOURCE, oid, n_sums=3, lanes=64)
            v, sm, st = O.OracleContext(prob, one_opts(S)).eval_batch(th)
            assert np.array_equal(sm, generic_numpy(th, prob.mom, prob.w, prob.obj_params, 3)[1], equal_nan=True)
