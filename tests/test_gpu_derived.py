"""smm_get_derived on the device (include/smmhip.h; smm.jl_amd/csrc/smm_derived.hpp, the kernel around the user's function in
smm_user_host.hpp, the plan in smm_reducers_host.hpp): every output equal bit for bit (NaN equal to NaN) to the contract restated in
derived_ref.py over the history downloaded with smm_get_history of the same context —

  the identity transform on objfunc_norm (np = nm = 2, 12 chains x 60 iterations) for the three selections and NULL, per-chain and
      scattered groups, also against smm_get_group_stats itself; a transform of products, quotients, roots, the contract's exp and log,
      the moments, mom, w and tdata; every word of the row one by one at np = 3, nm = 5 and at np = nm = 1 (rows of 16 and 10 doubles);
  pooled columns of 9600, 8192 and 8193 rows with members across the chunk seam, on the shipped library and under
      SMMHIP_STATS_SCRATCH in 5 batches of rows, 3 of outputs and 5 of the covariance's chunks (counted from the sizes);
  64 outputs; values that are not finite; every refusal by its code and message; a twin context that was never asked; host.derived."""
import ctypes as C
from collections import OrderedDict

import numpy as np
import pytest

import common as cm
import density_ref as DR
import derived_ref as DV
import group_stats_ref as GR
from test_gpu_reducer_caps import crafted_twin, seamed

pytestmark = pytest.mark.gpu

PROBS = (0.025, 0.5, 0.975)
LDS_N = 8192                     # smm_stats.hpp: STATS_LDS_N, the rows of a chunk


def vectors(prob):
    return prob.mom, prob.w, (() if prob.obj_params is None else prob.obj_params)


def check(h, prob, hist, tr, f, t0, t1, select, groups=None, n_groups=None, tdata=(), probs=PROBS):
    mom, w, ud = vectors(prob)
    got = h.derived(tr, t0, t1, select, groups, probs, tdata, n_groups=n_groups)
    want = DV.derived_from_history(hist, f, tr.n_out, t0, t1, select, groups, probs, mom, w, ud, tdata, n_groups=n_groups)
    assert set(got) == set(want)
    DV.assert_derived_equal(got, want)
    return got


@pytest.fixture(scope="module")
def run(S):
    N, T = 12, 60
    prob, opts = cm.serial_normal(N=N, T=T, ns=100)
    h = S.hip_context(prob, opts)
    h.step(T)
    return dict(h=h, hist=h.history(0, T), prob=prob, opts=opts, N=N, T=T)


def groupings(N):
    g4 = (np.arange(N) * 7 % 4).astype(np.int32)
    g4[g4 == 2] = -1                                        # group 2 empty, its chains in none
    return (None, None), (np.arange(N, dtype=np.int32), None), (g4, 4)


# --- the identity ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("select", (0, 1, 2))
def test_identity_equals_group_stats_on_the_parameters(S, run, select):
    h, hist, N, T = run["h"], run["hist"], run["N"], run["T"]
    tr = S.user_transform(DV.identity_source(2), 2)
    for groups, ng in groupings(N):
        for t0, t1 in ((0, T), (7, 41)):
            got = check(h, run["prob"], hist, tr, DV.identity(2), t0, t1, select, groups, ng)
            if select < 2:
                assert (got["n_nonfinite"] == 0).all()
                dev = h.group_stats(t0, t1, select == 1, groups, PROBS, n_groups=ng)
                GR.assert_group_stats_equal(got, dev)
                GR.assert_group_stats_equal(got, GR.group_stats_from_history(hist, t0, t1, select == 1, groups, PROBS, n_groups=ng))
            else:                                           # the rows before a chain's first accepted one, and only they
                acc = hist.accepted[:t1] != 0
                lead = np.array([max(0, (int(np.argmax(acc[:, c])) if acc[:, c].any() else t1) - t0) for c in range(N)])
                gv = np.zeros(N, np.int32) if groups is None else groups
                for g in range(len(got["count"])):
                    assert (got["n_nonfinite"][g] == lead[gv == g].sum()).all()
            if ng == 4:
                assert got["count"][2] == 0 and got["n_chains"][2] == 0 and np.isnan(got["mean"][2]).all() and np.isnan(got["cov"][2]).all()
    check(h, run["prob"], hist, tr, DV.identity(2), 20, 20, select, groupings(N)[2][0], 4)   # an empty window


# --- a real transform -----------------------------------------------------------------------------------------------------------------

REAL_SOURCE = DV.TRANSFORM_HEAD + """{
    out[0] = theta[0] * theta[1];
    out[1] = theta[0] / theta[1];
    out[2] = sqrt(value);
    out[3] = smm_exp(theta[0]) + sim_moments[1] * tdata[0];
    out[4] = smm_log(value) - mom[0] / w[1] + 0.25;
}
"""


def real(th, sm, va, mom, w, ud, td):
    exp, log = DR.contract("exp"), DR.contract("log")
    return [th[0] * th[1], th[0] / th[1], np.sqrt(va), exp(th[0]) + sm[1] * td[0], log(va) - mom[0] / w[1] + 0.25]


@pytest.mark.parametrize("select", ("all", "accepted", "state"))
def test_products_quotients_roots_exp_log_moments_and_tdata(S, run, select):
    h, hist, N, T = run["h"], run["hist"], run["N"], run["T"]
    tr = S.user_transform(REAL_SOURCE, 5)
    for groups, ng in groupings(N):
        check(h, run["prob"], hist, tr, real, 0, T, select, groups, ng, tdata=[1.0 / 3.0, -7.0])
    check(h, run["prob"], hist, tr, real, 5, 37, select, (np.arange(N) // 6).astype(np.int32), tdata=[-0.7], probs=())


def test_each_output_alone(S, run):
    h, hist, N, T = run["h"], run["hist"], run["N"], run["T"]
    tr = S.user_transform(REAL_SOURCE, 5)
    g3 = (np.arange(N) % 3).astype(np.int32)
    mom, w, ud = vectors(run["prob"])
    want = DV.derived_from_history(hist, real, 5, 2, 55, 2, g3, PROBS, mom, w, ud, [0.5], n_groups=3)
    for f in ("count", "n_chains", "n_nonfinite", "mean", "median", "quantile", "cov"):
        rc, r = raw_call(h, tr, 2, 55, 2, g3, 3, [0.5], PROBS, (f,))
        assert rc == 0, (f, h._fn("last_error")(h._ctx).decode())
        DV.assert_derived_equal(r, want, fields=(f,))


# --- every word of the row ------------------------------------------------------------------------------------------------------------

def words_source(np_, nm):
    return DV.TRANSFORM_HEAD + """{
    for (int j = 0; j < nm; ++j) out[j] = sim_moments[j];
    for (int k = 0; k < np; ++k) out[nm + k] = theta[k];
    out[nm + np] = value;
    out[nm + np + 1] = (udata[n_udata - 1] + mom[nm - 1] * w[nm - 1]) + ((double)(100 * np + nm) + tdata[n_tdata - 1] * (double)(10 * n_udata + n_tdata));
}
"""


def words(th, sm, va, mom, w, ud, td):
    np_, nm = len(th), len(sm)
    last = (ud[-1] + mom[-1] * w[-1]) + (float(100 * np_ + nm) + td[-1] * float(10 * len(ud) + len(td)))
    return list(sm) + list(th) + [va, np.full(len(va), last)]


@pytest.mark.parametrize("shape", ((3, 5), (1, 1)))
def test_every_word_of_the_row_at_its_offset(S, shape):
    from test_gpu_user_shapes import problem
    from user_objective_src import GENERIC_SOURCE
    np_, nm = shape
    N, T = 8, 40
    prob, opts = problem(S, S.register_user_objective(GENERIC_SOURCE), np_, nm, 4, 37, N, T)
    h = S.hip_context(prob, opts)
    h.step(T)
    hist = h.history(0, T)
    assert np.isfinite(hist.sim_moments).any()
    tr = S.user_transform(words_source(np_, nm), nm + np_ + 2)
    for select in (0, 1, 2):
        check(h, prob, hist, tr, words, 0, T, select, (np.arange(N) % 3).astype(np.int32), tdata=[2.0, 0.125, -3.0])
        check(h, prob, hist, tr, words, 3, 29, select, None, tdata=[0.5])


# --- long columns, the chunk seam and the batches ------------------------------------------------------------------------------------------

LONG_N, LONG_T = 66, 400
LONG_GROUPS = np.repeat(np.arange(3), (24, 21, 21)).astype(np.int32)
LONG_ROWS = [9600, 8192, 8193]


def long_history(h):
    """every row accepted, but the last member of group 1 keeps 192 accepted rows and that of group 2 193: pooled accepted-row columns of
    24 x 400 = 9600, 20 x 400 + 192 = 8192 and 20 x 400 + 193 = 8193 rows; row 8192 of each lies inside a member"""
    assert h.accepted.shape == (LONG_T, LONG_N)
    h.accepted[...] = 1
    h.accepted[1::2, 44] = 0
    h.accepted[384::2, 44] = 0                              # 200 - 8 = 192 accepted rows
    h.accepted[0::2, 65] = 0
    h.accepted[1:15:2, 65] = 0                              # 200 - 7 = 193 accepted rows, the first at row 15 (no state before it)
    assert (h.accepted[:, 44] != 0).sum() == 192 and (h.accepted[:, 65] != 0).sum() == 193
    return h


def derived_plan(clens, Q, cov, cap, N, T, npar):
    """(batches of outputs, batches of rows per batch of outputs, batches of the covariance's chunks) of smm_get_derived as the first
    reducer call of a context of N chains x T iterations under SMMHIP_STATS_SCRATCH = cap (0: the shipped 256 MiB): smm_reducers_host.hpp"""
    L, Mtot, NC, limit = LDS_N, sum(clens), len(clens), cap or 256 << 20
    all_bytes = N * T * (8 * npar + 4)
    scr = max(min(all_bytes, max(limit, 12 * T)), (N * T + L) * 8, (Q + 1) * L * 8 if cov else 0, min(limit, (Q + 1) * N * T * 8))
    least = max((Mtot + L) * 8, (Q + 1) * L * 8 if cov else 0)
    budget = min(scr, max(cap, least)) if cap else scr
    qb = min(Q, (budget - L * 8) // (Mtot * 8))
    rcap = (budget - qb * Mtot * 8) // 8
    nrow, at = 0, 0
    while at < NC:
        rows, nb = clens[at], 1
        while at + nb < NC and rows + clens[at + nb] <= rcap:
            rows, nb = rows + clens[at + nb], nb + 1
        nrow, at = nrow + 1, at + nb
    Nbc = min(NC, budget // ((Q + 1) * L * 8))
    return -(-Q // qb), nrow, -(-NC // Nbc)


def test_long_columns_the_chunk_seam_and_the_batched_paths(S, request, monkeypatch):
    prob, opts = cm.serial_normal(N=LONG_N, T=LONG_T, ns=100)
    h, state, crafted, back = crafted_twin(S, prob, opts, LONG_T, long_history)
    tr = S.user_transform(REAL_SOURCE, 5)
    clens = [LDS_N, 9600 - LDS_N, LDS_N, LDS_N, 1]
    assert derived_plan(clens, 5, True, 0, LONG_N, LONG_T, 2) == (1, 1, 2)          # the shipped library: outputs and rows at once
    calls = [(0, LONG_T, 1, LONG_GROUPS, 3), (0, LONG_T, 2, LONG_GROUPS, 3), (0, LONG_T, 0, np.where(LONG_GROUPS == 0, 0, -1).astype(np.int32), 1)]
    got = []
    for t0, t1, sel, g, ng in calls:
        got.append(check(h, prob, back, tr, real, t0, t1, sel, g, ng, tdata=[0.75]))
    assert got[0]["count"].tolist() == LONG_ROWS and got[2]["count"].tolist() == [9600]
    # the same from the test build with a scratch of two outputs' columns and one chunk's row indexes
    Mtot = sum(LONG_ROWS)
    cap = (2 * Mtot + LDS_N) * 8
    n_out_batches, n_row_batches, n_cov_batches = derived_plan(clens, 5, True, cap, LONG_N, LONG_T, 2)
    assert (n_out_batches, n_row_batches, n_cov_batches) == (3, 5, 5)
    request.getfixturevalue("hooks")
    hs = seamed(S, monkeypatch, prob, opts, state, crafted, STATS_SCRATCH=cap)
    seam = hs.derived(tr, 0, LONG_T, 1, LONG_GROUPS, PROBS, [0.75], n_groups=3)
    DV.assert_derived_equal(seam, got[0])
    DV.assert_derived_equal(hs.derived(tr, 0, LONG_T, 2, LONG_GROUPS, PROBS, [0.75], n_groups=3), got[1])
    cm.assert_history_equal(hs.history(0, LONG_T), back, exact_floats=True)


# --- 64 outputs ------------------------------------------------------------------------------------------------------------------------

def test_64_outputs_and_their_covariance(S, run):
    h, hist, N, T = run["h"], run["hist"], run["N"], run["T"]
    tr = S.user_transform(DV.TRANSFORM_HEAD + "{ for (int j = 0; j < 64; ++j) out[j] = theta[0] * (double)j; }", 64)
    f = lambda th, sm, va, mom, w, ud, td: th[0][None, :] * np.arange(64.0)[:, None]
    got = check(h, run["prob"], hist, tr, f, 0, T, "accepted", (np.arange(N) // 4).astype(np.int32))
    assert got["cov"].shape == (3, 64, 64) and np.isfinite(got["cov"]).all() and (got["cov"][:, 1, 1] > 0).all()
    check(h, run["prob"], hist, tr, f, 4, 50, "state", None)


# --- values that are not finite --------------------------------------------------------------------------------------------------------

def test_nonfinite_outputs_are_counted_and_propagate(S, run):
    h, hist, N, T, prob = run["h"], run["hist"], run["N"], run["T"], run["prob"]
    src = DV.TRANSFORM_HEAD + "{ out[0] = 1.0 / (theta[0] - tdata[0]); out[1] = smm_log(theta[1] - tdata[1]); }"
    log = DR.contract("log")
    f = lambda th, sm, va, mom, w, ud, td: [1.0 / (th[0] - td[0]), log(th[1] - td[1])]
    tr = S.user_transform(src, 2)
    groups = (np.arange(N) % 2).astype(np.int32)
    tdata = [hist.params[17, 0, 4], np.median(hist.params[:, 1, :])]   # a row of chain 4 (group 0) under select 0
    mom, w, ud = vectors(prob)
    want = DV.derived_from_history(hist, f, 2, 0, T, 0, groups, PROBS, mom, w, ud, tdata)
    bad = want["n_nonfinite"].sum(axis=1)
    assert bad.sum() >= 1 and (2 * want["n_nonfinite"] < want["count"][:, None]).all()
    assert want["n_nonfinite"][0, 0] == 1 and want["n_nonfinite"][1, 0] == 0
    assert np.isinf(want["mean"][0, 0]) and np.isnan(want["cov"][0, 0, 0]) and np.isfinite(want["mean"][1]).all()
    got = check(h, prob, hist, tr, f, 0, T, 0, groups, tdata=tdata)
    assert np.array_equal(got["n_nonfinite"], want["n_nonfinite"])


# --- refusals ----------------------------------------------------------------------------------------------------------------------------

def raw_call(h, tr, t0, t1, select, groups, n_groups, tdata, probs, fields, tid=None, n_tdata=None, n_probs=None):
    """smm_get_derived through ctypes with only the given outputs: (rc, the outputs)"""
    from smm_jl_amd import _abi as A
    Q, G, npr = tr.n_out, max(n_groups, 1), max(len(probs or ()), 1)
    shapes = dict(count=((G,), np.int64), n_chains=((G,), np.int32), n_nonfinite=((G, Q), np.int64), mean=((G, Q), float),
                  median=((G, Q), float), quantile=((npr, G, Q), float), cov=((G, Q, Q), float))
    r = {f: np.full(shapes[f][0], -7, shapes[f][1]) for f in fields}
    s = A.smm_derived_t()
    for f, t in A.smm_derived_t._fields_:
        if f in r:
            setattr(s, f, r[f].ctypes.data_as(t))
    ptr = lambda a, t, p: None if a is None else np.ascontiguousarray(a, t).ctypes.data_as(p)
    keep = [ptr(groups, np.int32, A.c_int32_p), ptr(tdata, float, A.c_double_p), ptr(probs, float, A.c_double_p)]
    rc = h._fn("get_derived")(h._ctx, tr.handle(h._lib) if tid is None else tid, t0, t1, select, keep[0], n_groups, keep[1],
                              (0 if tdata is None else len(tdata)) if n_tdata is None else n_tdata, keep[2],
                              (0 if probs is None else len(probs)) if n_probs is None else n_probs, C.byref(s))
    return rc, r


REFUSALS = [
    (dict(tid=-1), "transform_id is no handle of smm_register_user_transform"),
    (dict(tid=1 << 20), "transform_id is no handle of smm_register_user_transform"),
    (dict(t0=5, t1=4), "window must satisfy 0 <= t0 <= t1 <= completed iterations"),
    (dict(t0=-1), "window must satisfy 0 <= t0 <= t1 <= completed iterations"),
    (dict(t1=61), "window must satisfy 0 <= t0 <= t1 <= completed iterations"),
    (dict(n_tdata=-1), "n_tdata outside [0, 4096], or tdata NULL with n_tdata > 0"),
    (dict(tdata=[0.0] * 4097), "n_tdata outside [0, 4096], or tdata NULL with n_tdata > 0"),
    (dict(tdata=None, n_tdata=1), "n_tdata outside [0, 4096], or tdata NULL with n_tdata > 0"),
    (dict(select=3), "select must be 0 (all), 1 (accepted) or 2 (state)"),
    (dict(select=-1), "select must be 0 (all), 1 (accepted) or 2 (state)"),
    (dict(n_groups=-1), "n_groups < 0, or group NULL with n_groups != 1"),
    (dict(groups=None, n_groups=2), "n_groups < 0, or group NULL with n_groups != 1"),
    (dict(groups=[0] * 11 + [2], n_groups=2), "a group id outside [-1, n_groups)"),
    (dict(groups=[0] * 11 + [-2], n_groups=2), "a group id outside [-1, n_groups)"),
    (dict(n_probs=-1), "n_probs < 0, or probs NULL with n_probs > 0"),
    (dict(probs=None, n_probs=2, fields=("mean",)), "n_probs < 0, or probs NULL with n_probs > 0"),
    (dict(probs=[0.5, 1.5]), "probs must lie in [0, 1]"),
    (dict(probs=[np.nan]), "probs must lie in [0, 1]"),
    (dict(probs=[], fields=("quantile",)), "quantile requested without probs"),
]


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_every_refusal_by_its_code_and_message(S, run, case):
    from smm_jl_amd import _abi as A
    h = run["h"]
    tr = S.user_transform(REAL_SOURCE, 5)
    kw, message = REFUSALS[case]
    a = dict(t0=0, t1=60, select=1, groups=[0] * 12, n_groups=1, tdata=[1.0], probs=[0.5], fields=("count", "mean", "quantile", "cov"),
             tid=None, n_tdata=None, n_probs=None)
    a.update(kw)
    rc, r = raw_call(h, tr, a["t0"], a["t1"], a["select"], a["groups"], a["n_groups"], a["tdata"], a["probs"], a["fields"], a["tid"],
                     a["n_tdata"], a["n_probs"])
    assert rc == A.SMM_ERR_INVALID_ARG
    assert message in h._fn("last_error")(h._ctx).decode()
    for v in r.values():
        assert (v == -7).all()                              # nothing is written
    assert h._fn("get_derived")(h._ctx, tr.handle(h._lib), 0, 60, 1, None, 1, None, 0, None, 0, None) == A.SMM_ERR_INVALID_ARG   # NULL out
    s = A.smm_derived_t()
    assert h._fn("get_derived")(None, tr.handle(h._lib), 0, 60, 1, None, 1, None, 0, None, 0, C.byref(s)) == A.SMM_ERR_INVALID_ARG   # NULL ctx


def test_the_largest_tdata_is_taken(S, run):
    tr = S.user_transform(DV.TRANSFORM_HEAD + "{ out[0] = theta[0] + tdata[n_tdata - 1]; }", 1)
    td = np.arange(4096.0)
    check(run["h"], run["prob"], run["hist"], tr, lambda th, sm, va, mom, w, ud, t: [th[0] + t[-1]], 0, 60, 1, None, tdata=td)


# --- read-only ---------------------------------------------------------------------------------------------------------------------------

def test_history_and_next_steps_unchanged_against_a_twin(S):
    N, T = 12, 30
    prob, opts = cm.serial_normal(N=N, T=T + 10, ns=100)
    a, b = S.hip_context(prob, opts), S.hip_context(prob, opts)
    a.step(T); b.step(T)
    tr = S.user_transform(REAL_SOURCE, 5)
    for select in ("all", "accepted", "state"):
        a.derived(tr, 0, T, select, np.arange(N, dtype=np.int32), PROBS, [0.5])
        a.derived(tr, 3, 20, select, None, PROBS, [0.5])
    a.step(10); b.step(10)
    ha, hb = a.history(), b.history()
    cm.assert_history_equal(ha, hb, exact_floats=True)
    cm.assert_state_equal(a.state(), b.state(), rtol=0.0)


# --- the host layer ----------------------------------------------------------------------------------------------------------------------

def test_host_derived_equals_the_context_and_names_its_columns(S, monkeypatch):
    N, T = 64, 80
    m = S.MProb()
    S.addSampledParam(m, OrderedDict([("p1", [0.2, -3, 3]), ("p2", [-0.2, -20, 20])]))
    S.addMoment(m, {"name": ["mu1", "mu2"], "value": [-1.0, 10.0], "weight": [1.0, 1.0]})
    S.addEvalFunc(m, S.objfunc_norm)
    acc = [2.0] * 32 + [1.0] * 16 + [2.0] * 8 + [0.5] * 8
    MA = S.MAlgoBGP(m, {"N": N, "maxiter": T, "maxtemp": 5, "sigma": 0.05, "min_improve": [0.0] * N, "acc_tuners": acc})
    S.run(MA)
    tr = S.user_transform(REAL_SOURCE, 5)
    names = ["product", "ratio", "root", "shifted", "logv"]
    groups = np.array([0] * 32 + [1] * 16 + [0] * 8 + [2] * 8, np.int32)   # the default groups: equal acc_tuners, by first appearance
    want = MA._ctx.derived(tr, 10, 70, "state", groups, (0.05, 0.95), [0.25])
    MA._hist = None

    def no_download(*a, **k):
        raise AssertionError("the history was downloaded")
    monkeypatch.setattr(type(MA._ctx), "history", no_download)
    got = S.derived(MA, tr, names, t0=10, t1=70, select="state", probs=(0.05, 0.95), tdata=[0.25])
    assert len(got) == 3
    for g, d in enumerate(got):
        assert list(d) == ["count", "chains", "n_nonfinite", "mean", "median", "CI", "cov"]
        assert d["count"] == want["count"][g] and d["chains"] == want["n_chains"][g] and np.array_equal(d["cov"], want["cov"][g], equal_nan=True)
        for f, key in (("n_nonfinite", "n_nonfinite"), ("mean", "mean"), ("median", "median")):
            assert list(d[f]) == names
            assert np.array_equal(np.array(list(d[f].values()), float), want[key][g].astype(float), equal_nan=True)
        assert list(d["CI"]) == names and all(np.array_equal(d["CI"][k], want["quantile"][:, g, i], equal_nan=True) for i, k in enumerate(names))
    assert list(S.derived(MA, tr, tdata=[0.25])[0]["mean"]) == ["out0", "out1", "out2", "out3", "out4"]
    with pytest.raises(ValueError, match="distinct names"):
        S.derived(MA, tr, ["a", "b"], tdata=[0.25])
