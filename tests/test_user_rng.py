"""User objectives that draw from the library's generator (include/smmhip.h: smm_register_user_objective_rng, SMM_USER_OBJECTIVE_RNG,
SMM_USER_PARTIAL_RNG, smm_normal / smm_normal2 / smm_uniform) and their noseed evaluations.  The CPU side is the oracle with the
same source built by gcc over a C restatement of the stream (user_rng_src.Shim)."""
import ctypes as C
import os
import subprocess
import sys
import tempfile
from collections import OrderedDict

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import common as cm  # noqa: E402
from user_objective_src import AR1_SOURCE  # noqa: E402
from user_rng_src import AR1_RNG_SOURCE, MOMENTS_RNG_SOURCE, PANEL_RNG_SOURCE, PROBE_SOURCE, Shim  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "smm.jl_amd", "csrc")

# draw indices of the probe: around 2^32 and up to 2^52 (the counter's high word)
PROBE_NORMALS = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 5, 2 ** 45 + 2, 2 ** 52 + 3, 77]
PROBE_UNIFORMS = [0, 3, 2 ** 32 - 1, 2 ** 32 + 1, 2 ** 40 + 9, 2 ** 52 + 7, 12345, 2 ** 33]

_registered = {}


def register(S, source, n_sums=None, lanes=256):
    """one device registration per (source, form) and session: the handles are a finite resource of the oracle's hooks"""
    key = (source, n_sums, lanes)
    if key not in _registered:
        _registered[key] = S.register_user_objective(source, n_sums=n_sums, lanes=lanes, rng=True)
    return _registered[key]


def probe_problem(S, oid, seed=21):
    idx = [float(i) for i in PROBE_NORMALS + PROBE_UNIFORMS]
    nm = len(idx)
    prob = S.Problem(init=[0.5], lb=[0.0], ub=[1.0], mom=np.zeros(nm), w=np.ones(nm), ns=1, objective_id=oid, obj_params=idx)
    opts = S.BGPOpts(N=1, maxiter=1, sigma=[0.05], acc_tuner=[1.0], min_improve=[0.0], seed=seed)
    return prob, opts


def ar1_problem(S, oid, N, T, fail_above=None, seed=5):
    udata = [400.0] + ([fail_above] if fail_above is not None else [])
    prob = S.Problem(init=[0.3, 1.0], lb=[-0.95, 0.1], ub=[0.95, 3.0], mom=[0.0, 1.3, 0.6], w=[0.05, 0.1, 0.1], ns=1,
                     objective_id=oid, obj_params=udata)
    opts = S.BGPOpts(N=N, maxiter=T, sigma=0.05 * cm.temps(N, 4.0), acc_tuner=np.geomspace(3.0, 0.5, N) if N > 1 else [2.0],
                     min_improve=np.zeros(N), seed=seed, N_global=N)
    return prob, opts


def panel_problem(S, oid, N, T, fail_above=None, seed=9, agents=300, periods=20):
    prob = S.Problem(init=[0.3, 1.0], lb=[-0.95, 0.1], ub=[0.95, 3.0], mom=[0.0, 1.3, 0.6], w=[0.05, 0.1, 0.1], ns=1,
                     objective_id=oid, obj_params=[float(periods), float(agents)] + ([fail_above] if fail_above is not None else []))
    opts = S.BGPOpts(N=N, maxiter=T, sigma=0.05 * cm.temps(N, 4.0), acc_tuner=np.geomspace(3.0, 0.5, N) if N > 1 else [2.0],
                     min_improve=np.zeros(N), seed=seed, N_global=N)
    return prob, opts


def oracle_noseed(O, shim, prob, opts, th, base_seed):
    """the CPU reference of eval_batch_noseed: evaluation i through the oracle with the shim's stream keyed by base_seed + i"""
    o = O.OracleContext(prob, opts)
    M = th.shape[1]
    v, sm, st = np.empty(M), np.empty((prob.nm, M)), np.empty(M, np.int8)
    for i in range(M):
        shim.set_seed(base_seed + i)
        v[i:i + 1], sm[:, i:i + 1], st[i:i + 1] = o.eval_batch(th[:, i:i + 1])
    shim.set_seed(opts.seed)
    return v, sm, st


def random_thetas(M, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-0.9, 0.9, M), rng.uniform(0.2, 2.5, M)])


def assert_same(a, b):
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)


# ------------------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_rng_registration():
    from smm_jl_amd import _abi as A
    lib = A.load()
    assert hasattr(lib, "smm_register_user_objective_rng")
    assert ("smm_register_user_objective_rng", C.c_int, [C.c_char_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]) in A.SYMBOLS


@pytest.mark.parametrize("n_sums,lanes", [(-1, 256), (65, 256), (1, 0), (1, 100), (1, 1088), (3, 32)])
def test_bad_registration_arguments_are_refused(n_sums, lanes):
    from smm_jl_amd import _abi as A
    lib = A.load()
    oid = C.c_int32(-7)
    assert lib.smm_register_user_objective_rng(PANEL_RNG_SOURCE.encode(), n_sums, lanes, C.byref(oid)) == A.SMM_ERR_INVALID_ARG
    assert oid.value == -7 and b"n_sums" in lib.smm_last_error(None)
    assert lib.smm_register_user_objective_rng(None, 0, 0, C.byref(oid)) == A.SMM_ERR_INVALID_ARG
    assert lib.smm_register_user_objective_rng(AR1_RNG_SOURCE.encode(), 0, 0, None) == A.SMM_ERR_INVALID_ARG
    assert b"null" in lib.smm_last_error(None)


def test_the_shim_restates_the_librarys_stream(O):
    # the C restatement (orc_philox4x32_10 + the contract's log / sin / cos) against a host build of the library's own smm_rng.hpp
    shim = Shim(O)
    rng = np.random.default_rng(4)
    idx = np.concatenate([np.arange(64), rng.integers(0, 2 ** 63, 2000, dtype=np.uint64).astype(np.uint64),
                          2 ** 32 + np.arange(-8, 8)]).astype(np.uint64)
    for seed in (0, 21, 2 ** 40 + 17):
        for i in idx[:200]:
            a, b = shim.normal2(seed, int(i) >> 1)
            assert shim.normal(seed, int(i)) == (b if int(i) & 1 else a)
    d = tempfile.mkdtemp(prefix="smm_rng_host_")
    src, so = os.path.join(d, "probe.hip"), os.path.join(d, "probe.so")
    with open(src, "w") as f:
        f.write('#include "smm_rng.hpp"\n'
                'extern "C" void probe(uint64_t seed, const uint64_t* idx, int n, double* z0, double* z1, double* u) {\n'
                '    for (int k = 0; k < n; ++k) { smm::user_normal2(seed, idx[k], z0[k], z1[k]); u[k] = smm::user_uniform(seed, idx[k]); }\n'
                '}\n')
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O2", "-ffp-contract=off",
                           "-fno-fast-math", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, "-o", so, src])
    lib = C.CDLL(so)
    n = len(idx)
    for seed in (0, 21, 2 ** 40 + 17):
        z0, z1, u = np.empty(n), np.empty(n), np.empty(n)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
        lib.probe(C.c_uint64(seed), idx.ctypes.data_as(C.POINTER(C.c_uint64)), n, dp(z0), dp(z1), dp(u))
        for k in range(n):
            assert shim.normal2(seed, int(idx[k])) == (z0[k], z1[k]), (seed, int(idx[k]))
            assert shim.uniform(seed, int(idx[k])) == u[k], (seed, int(idx[k]))
        assert (u >= 0).all() and (u < 1).all() and np.isfinite(z0).all() and np.isfinite(z1).all()


def test_the_rng_forms_compile():
    # registration compiles the source through hiprtc (no device needed)
    import smm_jl_amd as S
    ids = [S.register_user_objective(PROBE_SOURCE, rng=True), S.register_user_objective(PANEL_RNG_SOURCE, n_sums=3, lanes=128, rng=True)]
    assert len(set(ids)) == 2 and min(ids) >= 1000
    with pytest.raises(RuntimeError) as e:
        S.register_user_objective(AR1_SOURCE, rng=True)   # the plain form's function is not the _RNG one: nothing defines smm_user_objective_rng
    assert "smm_register_user_objective failed" in str(e.value)


# ------------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_draw_probe_bit_for_bit(S, O):
    oid = register(S, PROBE_SOURCE)
    shim = Shim(O)
    prob, opts = probe_problem(S, oid, seed=21)
    h = S.hip_context(prob, opts)
    th = np.full((1, 5), 0.5)
    want = lambda seed: np.array([shim.normal(seed, i) for i in PROBE_NORMALS] + [shim.uniform(seed, i) for i in PROBE_UNIFORMS])  # noqa: E731
    v, sm, st = h.eval_batch(th)
    assert (st == 1).all() and (v == 0).all()
    for i in range(5):
        assert np.array_equal(sm[:, i], want(21))
    base = 2 ** 32 - 2
    v, sm, st = h.eval_batch_noseed(th, base)
    assert (st == 1).all()
    for i in range(5):
        assert np.array_equal(sm[:, i], want(base + i)), i
    for i in range(3):   # noseed evaluation i == a seeded evaluation under seed base + i
        p2, o2 = probe_problem(S, oid, seed=base + i)
        assert np.array_equal(S.hip_context(p2, o2).eval_batch(th[:, :1])[1][:, 0], sm[:, i])
    assert not np.array_equal(sm[:, 0], sm[:, 1])


@pytest.mark.gpu
def test_one_thread_model_every_form_equals_the_oracle(S, O):
    oid = register(S, AR1_RNG_SOURCE)
    shim = Shim(O, AR1_RNG_SOURCE)
    steps = [1, 20, 9]
    prob, opts = ar1_problem(S, oid, N=64, T=sum(steps), fail_above=0.8)
    shim.hook(O, oid, opts.seed)
    h = S.hip_context(prob, opts)
    assert h.persistent_info()[0] is True and h.describe()["persistent"] == "gen_user", h.describe()
    c = S.hip_context(prob, opts)
    c.set_persistent(False)
    o = O.OracleContext(prob, opts, threads=O.max_threads())
    th = random_thetas(300, 1)
    eh, eo = h.eval_batch(th), o.eval_batch(th)
    assert_same(eh, eo)
    assert (eh[2] == -2).any() and (eh[2] == 1).any()
    for n in steps:
        h.step(n); c.step(n); o.step(n)
    avail, launches, repairs = h.persistent_info()
    assert launches >= 1 and repairs == 0, (launches, repairs)
    assert c.persistent_info()[1] == 0
    hh = h.history()
    for other in (c, o):
        cm.assert_history_equal(hh, other.history(), exact_floats=True)
        cm.assert_state_equal(h.state(), other.state(), rtol=0)
    assert (hh.exchanged != 0).any() and hh.accepted[1:].any() and (hh.status == -2).any()


@pytest.mark.gpu
@pytest.mark.parametrize("lanes,N,steps,mi", [(64, 48, [30], 0.0), (256, 40, [2, 3, 15], 0.05), (1024, 32, [12], 0.0)])
def test_map_reduce_model_every_form_equals_the_oracle(S, O, lanes, N, steps, mi):
    oid = register(S, PANEL_RNG_SOURCE, n_sums=3, lanes=lanes)
    shim = Shim(O, PANEL_RNG_SOURCE, n_sums=3)
    prob, opts = panel_problem(S, oid, N=N, T=sum(steps), fail_above=0.5)
    opts.min_improve[:] = mi
    shim.hook(O, oid, opts.seed, lanes=lanes)
    h = S.hip_context(prob, opts)
    if lanes <= 512:
        assert h.describe()["persistent"] == "tile_user", h.describe()
    else:
        assert h.persistent_info()[0] is False
    c = S.hip_context(prob, opts)
    c.set_persistent(False)
    o = O.OracleContext(prob, opts, threads=O.max_threads())
    th = random_thetas(60, 2)
    assert_same(h.eval_batch(th), o.eval_batch(th))
    for n in steps:
        h.step(n); c.step(n); o.step(n)
    if lanes <= 512:
        avail, launches, repairs = h.persistent_info()
        assert launches >= 1 and repairs == 0, (launches, repairs)
    assert c.persistent_info()[1] == 0
    hh = h.history()
    for other in (c, o):
        cm.assert_history_equal(hh, other.history(), exact_floats=True)
        cm.assert_state_equal(h.state(), other.state(), rtol=0)
    assert hh.accepted[1:].any() and (hh.status == -2).any()


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["one_thread", "map_reduce"])
def test_noseed_evaluations(S, O, form):
    if form == "one_thread":
        oid = register(S, AR1_RNG_SOURCE)
        shim = Shim(O, AR1_RNG_SOURCE)
        prob, opts = ar1_problem(S, oid, N=1, T=1, fail_above=0.8)
        shim.hook(O, oid, opts.seed)
    else:
        oid = register(S, PANEL_RNG_SOURCE, n_sums=3, lanes=256)
        shim = Shim(O, PANEL_RNG_SOURCE, n_sums=3)
        prob, opts = panel_problem(S, oid, N=1, T=1, fail_above=0.8)
        shim.hook(O, oid, opts.seed, lanes=256)
    h = S.hip_context(prob, opts)
    th = random_thetas(40, 3)
    base = 2 ** 40 + 3
    got = h.eval_batch_noseed(th, base)
    assert_same(got, oracle_noseed(O, shim, prob, opts, th, base))
    assert (got[2] == -2).any() and (got[2] == 1).any()
    same = np.repeat(th[:, :1], 6, axis=1)   # repetitions at one point draw different shocks
    v, sm, st = h.eval_batch_noseed(same, 7)
    assert len({tuple(sm[:, i]) for i in range(6)}) == 6
    assert np.array_equal(h.eval_batch(same)[1], np.repeat(h.eval_batch(th[:, :1])[1], 6, axis=1))   # the seeded ones do not
    plain = S.register_user_objective(AR1_SOURCE)   # a user objective without a stream has no noseed evaluations
    p2, o2 = ar1_problem(S, plain, N=1, T=1)
    with pytest.raises(S.SMMHipError) as e:
        S.hip_context(p2, o2).eval_batch_noseed(th, 0)
    assert "noseed" in str(e.value)


@pytest.mark.gpu
def test_standard_errors_through_the_host_api(S, O):
    m = S.MProb()
    S.addSampledParam(m, {"rho": [0.5, -0.95, 0.95], "sigma": [1.0, 0.1, 3.0]})
    S.addMoment(m, {"name": ["m1", "m2", "m3"], "value": [0.0, 1.3, 0.6], "weight": [0.05, 0.1, 0.1]})
    obj = S.user_objective(AR1_RNG_SOURCE, name="ar1_gauss", rng=True)
    S.addEvalFunc(m, obj)
    m.objfunc_opts["obj_params"] = [400.0]
    from smm_jl_amd.host import _flat_problem
    prob = _flat_problem(m)
    eval_opts = S.BGPOpts(N=1, maxiter=1, sigma=[0.05], acc_tuner=[1.0], min_improve=[0.0])   # (what the device's evaluation context is made with)
    shim = Shim(O, AR1_RNG_SOURCE)
    shim.hook(O, obj.objective_id, eval_opts.seed)

    def cpu_evaluator(m_, P, noseed_base=None):
        if noseed_base is not None:
            return oracle_noseed(O, shim, prob, eval_opts, P, noseed_base)
        return O.OracleContext(prob, eval_opts).eval_batch(P)

    p = OrderedDict([("rho", 0.5), ("sigma", 1.0)])
    Sd = S.getSigma(m, p, 60, seed=11)
    assert np.array_equal(Sd, S.getSigma(m, p, 60, seed=11, evaluator=cpu_evaluator))
    assert not np.array_equal(Sd, S.getSigma(m, p, 60, seed=12))
    sed = S.get_stdErrors(m, p, reps=60, seed=11)
    sec = S.get_stdErrors(m, p, reps=60, seed=11, evaluator=cpu_evaluator)
    assert list(sed) == ["rho", "sigma"] and np.array_equal(list(sed.values()), list(sec.values()))
    se = np.array(list(sed.values()))
    assert np.isfinite(se).all() and (se > 0).all(), sed
    evs = S.evaluateObjectives(m, [p, p], noseed_base=5)
    assert evs[0].simMoments != evs[1].simMoments


@pytest.mark.gpu
def test_two_shards_equal_one(S, O):
    from test_gpu_parity import sharded_run
    from smm_jl_amd import _abi as A
    oid = register(S, AR1_RNG_SOURCE)
    prob, opts = ar1_problem(S, oid, N=32, T=20, fail_above=0.8)
    single = S.hip_context(prob, opts)
    single.step(20)
    ctxs = sharded_run(S, prob, opts, 2, 20)
    hs = single.history()
    for r, c in enumerate(ctxs):
        hr = c.history()
        for f in A.HistoryBuffers.FIELDS:
            assert np.array_equal(getattr(hr, f), getattr(hs, f)[..., r * 16:(r + 1) * 16], equal_nan=True), (f, r)
    assert (hs.exchanged != 0).any()


@pytest.mark.gpu
def test_distribution_of_the_draws(S):
    K, lanes, M = 1024, 256, 12   # 3.1 million normals and as many uniforms
    oid = register(S, MOMENTS_RNG_SOURCE, n_sums=5, lanes=lanes)
    prob = S.Problem(init=[0.5], lb=[0.0], ub=[1.0], mom=np.zeros(5), w=np.ones(5), ns=1, objective_id=oid, obj_params=[float(K)])
    h = S.hip_context(prob, S.BGPOpts(N=1, maxiter=1, sigma=[0.05], acc_tuner=[1.0], min_improve=[0.0], seed=3))
    v, sm, st = h.eval_batch_noseed(np.full((1, M), 0.5), 1000)
    assert (st == 1).all()
    n = float(K * lanes * M)
    t = sm.sum(axis=1)
    assert t[4] == 0.0   # every uniform in [0, 1)
    assert abs(t[0] / n) < 5 / np.sqrt(n)
    assert abs(t[1] / n - 1.0) < 5 * np.sqrt(2.0 / n)
    assert abs(t[2] / n - 0.5) < 5 * np.sqrt(1.0 / 12.0 / n)
    assert abs(t[3] / n - 1.0 / 3.0) < 5 * np.sqrt(4.0 / 45.0 / n)
