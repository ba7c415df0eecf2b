"""smm_get_density on the device (include/smmhip.h, smm.jl_amd/csrc/smm_density.hpp): every output equal bit for bit (NaN equal to NaN,
the sign of a zero compared) to the contract restated in density_ref.py over the history downloaded with smm_get_history —
objfunc_norm with per-chain, pooled and NULL groups, the three selections, two windows, four masses, n_grid 0 / 2 / 64, given and
automatic ranges and bandwidths; the crafted short columns of density_craft.py (statuses, every ending of the mode, every fallback of
the bandwidth's spread); np = 50 in batches of parameters; every refusal by its message; a twin context that was never asked; each
output asked for alone; host.hdi / mode / kde without a download.  The long columns and the batched paths are in tests/test_gpu_density_seams.py."""
import ctypes as C

import numpy as np
import pytest

import common as cm
import density_craft as DC
import density_ref as DR
from test_gpu_reducer_caps import crafted_twin

pytestmark = pytest.mark.gpu

MASS = [0.01, 0.5, 0.94, 1.0]


def check(h, hist, t0, t1, select, groups=None, mass=MASS, n_grid=64, rng=None, bw=None, n_groups=None):
    got = h.density(t0, t1, select, groups, mass, n_grid, rng, bw, n_groups=n_groups)
    want = DR.density_from_history(hist, t0, t1, select, groups, mass, n_grid, rng, bw, n_groups=n_groups)
    assert set(got) == set(want)
    DR.assert_density_equal(got, want)
    return got


def raw_call(h, t0, t1, select, groups, n_groups, mass, n_grid, rng, bw, fields):
    """smm_get_density through ctypes with only the given outputs: (rc, the outputs)"""
    from smm_jl_amd import _abi as A
    npar, G, nm, ng = h.np, max(n_groups, 1), max(len(mass or ()), 1), max(n_grid, 1)
    shapes = dict(count=((G,), np.int64), status=((G, npar), np.int32), hdi_lo=((nm, G, npar), float), hdi_hi=((nm, G, npar), float),
                  mode=((G, npar), float), bw=((G, npar), float), kde_status=((G, npar), np.int32), grid=((G, npar, ng), float),
                  density=((G, npar, ng), float), kde_mode=((G, npar), float))
    r = {f: np.full(shapes[f][0], -7, shapes[f][1]) for f in fields}
    s = A.smm_density_t()
    for f, t in A.smm_density_t._fields_:
        if f in r:
            setattr(s, f, r[f].ctypes.data_as(t))
    ptr = lambda a, t, p: None if a is None else np.ascontiguousarray(a, t).ctypes.data_as(p)
    keep = [ptr(groups, np.int32, A.c_int32_p), ptr(mass, float, A.c_double_p), ptr(rng, float, A.c_double_p), ptr(bw, float, A.c_double_p)]
    rc = h._fn("get_density")(h._ctx, t0, t1, select, keep[0], n_groups, keep[1], 0 if mass is None else len(mass), n_grid, keep[2], keep[3],
                              C.byref(s))
    return rc, r


@pytest.fixture(scope="module")
def run(S):
    N, T = 12, 40
    prob, opts = cm.serial_normal(N=N, T=T, ns=100)
    h = S.hip_context(prob, opts)
    h.step(T)
    return dict(h=h, hist=h.history(0, T), prob=prob, opts=opts, N=N, T=T)


def groupings(N):
    g4 = (np.arange(N) % 4).astype(np.int32)
    g4[g4 == 2] = -1                                        # group 2 empty, its chains in none
    return (np.arange(N, dtype=np.int32), None), (g4, 4), (None, None)


@pytest.mark.parametrize("select", ("all", "accepted", "state"))
def test_real_run_groups_selections_windows_masses(run, select):
    h, hist, N = run["h"], run["hist"], run["N"]
    for groups, ng in groupings(N):
        for t0, t1 in ((3, 20), (0, 40)):
            got = check(h, hist, t0, t1, select, groups, n_groups=ng)
            if ng == 4:
                assert got["count"][2] == 0 and (got["status"][2] == 2).all() and np.isnan(got["density"][2]).all()


def test_real_run_kde_arguments(run):
    h, hist, N = run["h"], run["hist"], run["N"]
    g3 = (np.arange(N) % 3).astype(np.int32)
    rng = np.array([[-2.0, 1.0], [9.0, 11.0]])
    for n_grid in (0, 2, 64):
        for r in (None, rng):
            for bw in (None, [0.25, 1.0 / 3.0]):
                check(h, hist, 0, 40, "accepted", g3, n_grid=n_grid, rng=r, bw=bw)
    check(h, hist, 3, 20, "state", np.arange(N, dtype=np.int32), mass=[], n_grid=64)
    check(h, hist, 20, 20, "all", g3, n_grid=5)              # an empty window: status 2 everywhere
    check(h, hist, 0, 40, "all", g3, n_grid=4096, mass=[0.5])


@pytest.fixture(scope="module")
def small(S, run):
    h, state, crafted, back = crafted_twin(S, run["prob"], run["opts"], run["T"], DC.small_history)
    return dict(h=h, back=back)


@pytest.mark.parametrize("select", (0, 1, 2))
def test_crafted_short_columns_statuses_and_mode_endings(small, select):
    h, back = small["h"], small["back"]
    per_chain = np.arange(12, dtype=np.int32)
    got = check(h, back, 0, 40, select, per_chain, n_grid=16)
    if select == 1:
        assert got["count"].tolist()[:6] == [0, 1, 2, 3, 4, 5] and got["status"][0].tolist() == [2, 2]
        assert (got["kde_status"][:2] == 1).all() and (got["kde_status"][2:6] == 0).all()   # m < 2: no bandwidth
    if select == 2:
        assert (got["status"][DC.LATE_START] == 1).all() and np.isnan(got["mode"][DC.LATE_START]).all()
        assert got["count"][DC.LATE_START] == 40
    check(h, back, 0, 40, select, (np.arange(12) // 6).astype(np.int32), n_grid=7)
    check(h, back, 5, 33, select, None, n_grid=3, bw=[0.5, 2.0])


def test_np50_parameters_in_batches(S):
    from smm_jl_amd.workloads import build_problem
    N, T = 8, 30
    prob, opts = build_problem("c5", N, N, 0, T, 0)
    assert prob.np == 50
    h = S.hip_context(prob, opts)
    h.step(T)
    hist = h.history(0, T)
    for select in ("all", "accepted", "state"):
        check(h, hist, 0, T, select, np.arange(N, dtype=np.int32), mass=[0.5, 0.94], n_grid=9)
    check(h, hist, 4, 27, "accepted", (np.arange(N) // 4).astype(np.int32), n_grid=33, rng=np.tile([-0.5, 0.5], (50, 1)))


REFUSALS = [
    (dict(select=3), "select must be 0 (all), 1 (accepted) or 2 (state)"),
    (dict(n_groups=-1), "n_groups < 0, or group NULL with n_groups != 1"),
    (dict(groups=None, n_groups=2), "n_groups < 0, or group NULL with n_groups != 1"),
    (dict(groups=[0] * 11 + [2], n_groups=2), "a group id outside [-1, n_groups)"),
    (dict(t0=5, t1=4), None),
    (dict(t1=41), None),
    (dict(mass=None, n_mass=-1), "n_mass < 0, or mass NULL with n_mass > 0"),
    (dict(mass=None, n_mass=1), "n_mass < 0, or mass NULL with n_mass > 0"),
    (dict(mass=[0.5, 0.0]), "a mass must lie in (0, 1]"),
    (dict(mass=[1.0000000000000002]), "a mass must lie in (0, 1]"),
    (dict(mass=[np.nan]), "a mass must lie in (0, 1]"),
    (dict(mass=[], fields=("hdi_lo",)), "hdi_lo or hdi_hi requested with n_mass == 0"),
    (dict(mass=[], fields=("hdi_hi",)), "hdi_lo or hdi_hi requested with n_mass == 0"),
    (dict(n_grid=1), "n_grid must be 0 or lie in [2, 4096]"),
    (dict(n_grid=-2), "n_grid must be 0 or lie in [2, 4096]"),
    (dict(n_grid=4097), "n_grid must be 0 or lie in [2, 4096]"),
    (dict(n_grid=0, fields=("grid",)), "grid, density or kde_mode requested with n_grid == 0"),
    (dict(n_grid=0, fields=("density",)), "grid, density or kde_mode requested with n_grid == 0"),
    (dict(n_grid=0, fields=("kde_mode",)), "grid, density or kde_mode requested with n_grid == 0"),
    (dict(rng=[[0.0, 1.0], [2.0, 1.0]]), "a range row must be finite with lo <= hi"),
    (dict(rng=[[0.0, np.inf], [0.0, 1.0]]), "a range row must be finite with lo <= hi"),
    (dict(rng=[[np.nan, 1.0], [0.0, 1.0]]), "a range row must be finite with lo <= hi"),
    (dict(bw=[1.0, 0.0]), "a bw entry must be finite and > 0"),
    (dict(bw=[-1.0, 1.0]), "a bw entry must be finite and > 0"),
    (dict(bw=[np.inf, 1.0]), "a bw entry must be finite and > 0"),
    (dict(bw=[1.0, np.nan]), "a bw entry must be finite and > 0"),
]


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_every_refusal_by_its_message(S, run, case):
    from smm_jl_amd import _abi as A
    h = run["h"]
    kw, message = REFUSALS[case]
    a = dict(t0=0, t1=40, select=1, groups=[0] * 12, n_groups=1, mass=[0.5], n_grid=8, rng=None, bw=None, fields=("status", "mode"))
    a.update(kw)
    mass = a["mass"]
    if "n_mass" in a:                                       # (a NULL mass with a count of its own)
        s = A.smm_density_t()
        rc = h._fn("get_density")(h._ctx, 0, 40, 1, None, 1, None, a["n_mass"], 8, None, None, C.byref(s))
        r = {}
    else:
        rc, r = raw_call(h, a["t0"], a["t1"], a["select"], a["groups"], a["n_groups"], mass, a["n_grid"], a["rng"], a["bw"], a["fields"])
    assert rc == A.SMM_ERR_INVALID_ARG
    if message is not None:
        assert message in h._fn("last_error")(h._ctx).decode()
    for v in r.values():
        assert (v == -7).all()                              # nothing is written
    assert h._fn("get_density")(h._ctx, 0, 40, 1, None, 1, None, 0, 0, None, None, None) == A.SMM_ERR_INVALID_ARG   # NULL out


def test_history_and_next_step_unchanged_against_a_twin(S):
    N, T = 12, 40
    prob, opts = cm.serial_normal(N=N, T=T + 5, ns=100)
    a, b = S.hip_context(prob, opts), S.hip_context(prob, opts)
    a.step(T); b.step(T)
    for select in ("all", "accepted", "state"):
        a.density(0, T, select, np.arange(N, dtype=np.int32), MASS, 16)
        a.density(3, 20, select, None, MASS, 16)
    cm.assert_history_equal(a.history(), b.history(), exact_floats=True)
    a.step(5); b.step(5)
    cm.assert_history_equal(a.history(), b.history(), exact_floats=True)
    cm.assert_state_equal(a.state(), b.state(), rtol=0.0)


def test_each_output_alone(run):
    h, hist, N = run["h"], run["hist"], run["N"]
    g3 = (np.arange(N) % 3).astype(np.int32)
    want = DR.density_from_history(hist, 2, 37, 2, g3, MASS, 10, n_groups=3)
    for f in ("count", "status", "hdi_lo", "hdi_hi", "mode", "bw", "kde_status", "grid", "density", "kde_mode"):
        rc, r = raw_call(h, 2, 37, 2, g3, 3, MASS, 10, None, None, (f,))
        assert rc == 0, (f, h._fn("last_error")(h._ctx).decode())
        DR.assert_density_equal(r, want, fields=(f,))


def test_host_hdi_mode_kde_read_the_device(S, monkeypatch):
    from collections import OrderedDict
    import chain_stats_ref as CS
    N, T = 64, 80
    m = S.MProb()
    S.addSampledParam(m, OrderedDict([("p1", [0.2, -3, 3]), ("p2", [-0.2, -20, 20])]))
    S.addMoment(m, {"name": ["mu1", "mu2"], "value": [-1.0, 10.0], "weight": [1.0, 1.0]})
    S.addEvalFunc(m, S.objfunc_norm)
    acc = [2.0] * 32 + [1.0] * 16 + [2.0] * 8 + [0.5] * 8
    MA = S.MAlgoBGP(m, {"N": N, "maxiter": T, "maxtemp": 5, "sigma": 0.05, "min_improve": [0.0] * N, "acc_tuners": acc})
    S.run(MA)
    ps = [S.params(c) for c in MA.chains[:3]]
    MA._hist = None

    def no_download(*a, **k):
        raise AssertionError("the history was downloaded")
    monkeypatch.setattr(type(MA._ctx), "history", no_download)
    for c, p in zip(list(MA.chains[:3]), ps):
        iv, md, kd = S.hdi(c, 0.8), S.mode(c), S.kde(c, n_grid=16, bw={"p1": 0.5, "p2": 0.25})
        assert list(iv) == list(md) == list(kd) == ["p1", "p2"]
        for k in iv:
            s = CS.total_sort(np.asarray(p[k], float))
            lo, hi, _ = DR.hdi(s, 0.8)
            assert iv[k] == (lo, hi) and md[k] == DR.half_sample_mode(s)
            want = DR.column(np.asarray(p[k], float), [], 16, bw={"p1": 0.5, "p2": 0.25}[k])
            assert np.array_equal(kd[k][0], want["grid"]) and np.array_equal(kd[k][1], want["density"]) and kd[k][2] == want["bw"]
    groups = S.hdi(MA, 0.94)                              # the default groups: equal acc_tuners
    assert len(groups) == 3 and all(lo <= hi for g in groups for lo, hi in g.values())
    assert len(S.kde(MA, n_grid=8)) == 3 and len(S.mode(MA, window=(10, 70))) == 3
    with pytest.raises(ValueError, match="no draw"):
        S.mode(MA.chains[0], window=(5, 5))
