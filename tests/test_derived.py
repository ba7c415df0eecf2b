"""The restatement of smm_get_derived's contract (derived_ref.py) against plain formulas on a synthetic history, and what of the feature
runs without a device: the identity transform against group_stats_ref on the parameters and against hist_ref.columns for the state
series; a ratio and a function of the moments against np.mean / np.quantile / np.cov; the state rows without a(t) as NaN, counted in
n_nonfinite; the registration of transforms through hiprtc (which cross-compiles without a GPU) with its refusals; the refusals of
smm_get_derived that are reached before the device is touched.  CPU only."""
import ctypes as C

import numpy as np
import pytest

import derived_ref as DV
import group_stats_ref as GR
import hist_ref as HR
from smm_jl_amd import _abi as A

T, N, NP, NM = 50, 7, 3, 4
GROUPS = np.array([0, 1, 0, -1, 2, 1, 0], np.int32)       # group 3 of 4 stays empty
PROBS = (0.025, 0.5, 0.975)


@pytest.fixture(scope="module")
def hist():
    r = np.random.default_rng(3)
    h = A.HistoryBuffers(T, N, NP, NM)
    h.params[...] = r.normal(size=h.params.shape)
    h.sim_moments[...] = r.normal(size=h.sim_moments.shape)
    h.value[...] = r.gamma(2.0, size=h.value.shape)
    h.accepted[...] = r.random(h.accepted.shape) < 0.4
    h.accepted[:5, 2] = 0                                  # chain 2: no state before row 5
    h.accepted[5, 2] = 1
    h.accepted[:, 4] = 0                                   # chain 4 (alone in group 2): never accepted
    return h


def ref(h, f, Q, t0, t1, select, groups=GROUPS, G=4, tdata=()):
    return DV.derived_from_history(h, f, Q, t0, t1, select, groups, PROBS, np.arange(NM) + 1.0, np.ones(NM), (), tdata, n_groups=G)


@pytest.mark.parametrize("select", (0, 1))
@pytest.mark.parametrize("window", ((0, T), (7, 31), (9, 9)))
def test_identity_equals_group_stats_ref_on_the_parameters(hist, select, window):
    t0, t1 = window
    got = ref(hist, DV.identity(NP), NP, t0, t1, select)
    want = GR.group_stats_from_history(hist, t0, t1, select == 1, GROUPS, PROBS, n_groups=4)
    GR.assert_group_stats_equal(got, want)
    assert (got["n_nonfinite"] == 0).all() and got["count"][3] == 0 and np.isnan(got["mean"][3]).all()


def test_identity_on_the_state_series_equals_hist_ref_columns(hist):
    for t0, t1 in ((0, T), (3, 40), (8, 20)):
        cols = DV.derived_columns(hist, DV.identity(NP), NP, t0, t1, 2, GROUPS, 4, np.zeros(NM), np.ones(NM))
        want = HR.columns(hist, t0, t1, 2, GROUPS, 4)
        for y, x in zip(cols, want):
            assert np.array_equal(y, x, equal_nan=True)


def test_state_rows_without_a_state_are_nan_and_counted(hist):
    got = ref(hist, lambda th, sm, va, mom, w, ud, td: [th[0] * 0.0 + 1.0, va], 2, 0, T, 2)
    first = [int(np.argmax(hist.accepted[:, c] != 0)) if hist.accepted[:, c].any() else T for c in range(N)]
    assert first[2] == 5 and first[4] == T
    for g in range(3):
        lead = sum(first[c] for c in np.flatnonzero(GROUPS == g))
        assert (got["n_nonfinite"][g] == lead).all() and got["count"][g] == T * (GROUPS == g).sum()
        assert np.isnan(got["mean"][g]).all() == (lead > 0) and np.isnan(got["cov"][g]).all() == (lead > 0)
    assert (got["n_nonfinite"][2] == T).all()             # the function was never called: a constant output is NaN too
    late = ref(hist, lambda th, sm, va, mom, w, ud, td: [th[0] * 0.0 + 1.0, va], 2, 6, T, 2, groups=np.where(np.arange(N) == 2, 0, -1), G=1)
    assert (late["n_nonfinite"] == 0).all() and late["mean"][0, 0] == 1.0 and late["cov"][0, 0, 0] == 0.0


def test_summaries_against_numpy(hist):
    f = lambda th, sm, va, mom, w, ud, td: [th[0] / th[1], sm[2] * td[0] - mom[1] / w[0], np.sqrt(va)]
    got = ref(hist, f, 3, 2, 47, 1, tdata=[1.5])
    for g in range(3):
        rows = [(t, c) for c in np.flatnonzero(GROUPS == g) for t in range(2, 47) if hist.accepted[t, c]]
        assert got["count"][g] == len(rows)
        if not rows:
            assert np.isnan(got["mean"][g]).all()
            continue
        y = np.array([[hist.params[t, 0, c] / hist.params[t, 1, c], hist.sim_moments[t, 2, c] * 1.5 - 2.0 / 1.0, np.sqrt(hist.value[t, c])]
                      for t, c in rows]).T
        np.testing.assert_allclose(got["mean"][g], y.mean(axis=1), rtol=1e-13)
        np.testing.assert_allclose(got["median"][g], np.median(y, axis=1), rtol=0, atol=0)
        np.testing.assert_allclose(got["quantile"][:, g], np.quantile(y, PROBS, axis=1), rtol=1e-14)
        np.testing.assert_allclose(got["cov"][g], np.cov(y), rtol=1e-11)
        assert (got["n_nonfinite"][g] == 0).all()


def test_nonfinite_values_are_kept_and_counted(hist):
    x = hist.params[10, 0, 0]                              # a row of group 0 under select 0
    f = lambda th, sm, va, mom, w, ud, td: [1.0 / (th[0] - td[0]), th[1]]
    got = ref(hist, f, 2, 0, T, 0, tdata=[x])
    assert got["n_nonfinite"].tolist() == [[1, 0], [0, 0], [0, 0], [0, 0]]
    assert np.isinf(got["mean"][0, 0]) and np.isnan(got["cov"][0, 0, 0]) and np.isnan(got["cov"][0, 0, 1])
    assert np.isfinite(got["cov"][0, 1, 1]) and np.isfinite(got["median"][0, 0]) and np.isfinite(got["mean"][1]).all()


# --- registration: hiprtc cross-compiles without a device ------------------------------------------------------------------------------

def register(source, n_out):
    lib = A.load()
    tid = C.c_int32(-7)
    rc = lib.smm_register_user_transform(None if source is None else source.encode(), n_out, C.byref(tid))
    return rc, tid.value, lib.smm_last_error(None).decode()


SOURCE = DV.TRANSFORM_HEAD + """{
    out[0] = theta[0] * theta[np - 1];
    out[1] = smm_exp(theta[0]) + smm_log(value) - sqrt(sim_moments[nm - 1] * sim_moments[nm - 1]) + tdata[0] * udata[0] - mom[0] / w[0];
}
"""


def test_a_valid_source_registers_and_two_registrations_get_distinct_handles():
    rc, a, msg = register(SOURCE, 2)
    assert rc == 0 and a >= 0, msg
    rc, b, msg = register(SOURCE, 3)                       # (an output left unwritten is allowed: it stays NaN)
    assert rc == 0 and b >= 0 and b != a, msg
    import smm_jl_amd as S
    t = S.user_transform(DV.identity_source(4), 4)
    assert t.n_out == 4 and t.handle(A.load()) not in (a, b) and t.handle(A.load()) == t.handle(A.load())


def test_a_source_that_does_not_compile_is_refused_with_the_compilers_log():
    rc, tid, msg = register(DV.TRANSFORM_HEAD + "{ out[0] = no_such_name; }", 1)
    assert rc == A.SMM_ERR_INVALID_ARG and tid == -7
    assert "user transform does not compile" in msg and "no_such_name" in msg
    rc, tid, msg = register(DV.TRANSFORM_HEAD + "{ out[0] = theta[0] +; }", 1)   # a syntax error
    assert rc == A.SMM_ERR_INVALID_ARG and tid == -7 and "error: expected expression" in msg
    import smm_jl_amd as S
    with pytest.raises(A.SMMHipError, match="no_such_name") as e:
        S.user_transform(DV.TRANSFORM_HEAD + "{ out[0] = no_such_name; }", 1)
    assert e.value.code == A.SMM_ERR_INVALID_ARG


@pytest.mark.parametrize("n_out", (0, 65, -1))
def test_n_out_outside_1_to_64_is_refused(n_out):
    rc, tid, msg = register(SOURCE, n_out)
    assert rc == A.SMM_ERR_INVALID_ARG and tid == -7 and "1 <= n_out <= 64" in msg


def test_64_outputs_register():
    rc, tid, msg = register(DV.TRANSFORM_HEAD + "{ for (int j = 0; j < 64; ++j) out[j] = theta[0] * (double)j; }", 64)
    assert rc == 0 and tid >= 0, msg


def test_null_arguments_are_refused():
    lib = A.load()
    rc, tid, msg = register(None, 2)
    assert rc == A.SMM_ERR_INVALID_ARG and tid == -7 and "null argument" in msg
    assert lib.smm_register_user_transform(SOURCE.encode(), 2, None) == A.SMM_ERR_INVALID_ARG


def test_get_derived_refuses_a_null_context_before_touching_the_device():
    lib = A.load()
    s = A.smm_derived_t()
    assert lib.smm_get_derived(None, 0, 0, 1, 0, None, 1, None, 0, None, 0, C.byref(s)) == A.SMM_ERR_INVALID_ARG
    assert lib.smm_get_derived(None, 0, 0, 1, 0, None, 1, None, 0, None, 0, None) == A.SMM_ERR_INVALID_ARG
