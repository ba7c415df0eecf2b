"""smm_get_group_stats without a GPU: the restatement of its contract (group_stats_ref.py) against numpy itself — np.mean, np.median,
np.quantile(method="linear") of np.concatenate(...) and np.sum-based covariance — on pooled columns past 2 x 8192 draws, with NaN, +-0,
ties, empty groups and chains in no group; the ABI declaration, the built library's export and the Julia mirror of the struct."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

import group_stats_ref as GR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBS = (0.0, 0.025, 0.3, 0.5, 0.975, 1.0)


def fake_history(rng, T, N, npar, pool=None):
    """a HistoryBuffers-like namespace: params [T][np][N], accepted [T][N], value [T][N]"""
    params = rng.standard_normal((T, npar, N)) if pool is None else rng.choice(pool, (T, npar, N))
    return SimpleNamespace(params=params, accepted=(rng.random((T, N)) < 0.55).astype(np.uint8), value=rng.standard_normal((T, N)))


def numpy_pooled(h, t0, t1, acc, groups, G, probs):
    """the same summaries by numpy's own readers, NaN-free columns"""
    npar = h.params.shape[1]
    out = []
    for g in range(G):
        mem = [c for c in range(len(groups)) if groups[c] == g]
        cols = []
        for c in mem:
            sel = h.accepted[t0:t1, c] != 0 if acc else np.ones(t1 - t0, bool)
            cols.append(h.params[t0:t1, :, c][sel].T)
        x = np.ascontiguousarray(np.concatenate(cols, axis=1)) if mem else np.empty((npar, 0))
        m = x.shape[1]
        r = dict(count=m)
        if m:
            r["mean"] = np.array([np.mean(x[k]) for k in range(npar)])
            r["median"] = np.array([np.median(x[k]) for k in range(npar)])
            r["quantile"] = np.array([[np.quantile(x[k], p, method="linear") for k in range(npar)] for p in probs])
        if m >= 2:
            d = x - r["mean"][:, None]
            r["cov"] = np.array([[np.sum(np.ascontiguousarray(d[j] * d[k])) / (m - 1) for k in range(npar)] for j in range(npar)])
        out.append(r)
    return out


@pytest.mark.parametrize("T,N,G", [(40, 12, 3), (700, 64, 2), (1200, 40, 1)])
@pytest.mark.parametrize("acc", [True, False])
def test_restatement_is_numpy_on_the_concatenated_columns(T, N, G, acc):
    rng = np.random.default_rng(T + N)
    h = fake_history(rng, T, N, 3)
    groups = np.where(rng.random(N) < 0.15, -1, rng.integers(0, G, N)).astype(np.int32)
    groups[0] = G - 1                                    # (max + 1 = G groups)
    longest = 0
    for t0, t1 in ((0, T), (T // 7, T - T // 5)):
        got = GR.group_stats_from_history(h, t0, t1, acc, groups, PROBS)
        longest = max(longest, got["count"].max())
        want = numpy_pooled(h, t0, t1, acc, groups, G, PROBS)
        for g, w in enumerate(want):
            assert got["count"][g] == w["count"] and got["n_chains"][g] == (groups == g).sum()
            if w["count"] == 0:
                assert np.isnan(got["mean"][g]).all() and np.isnan(got["cov"][g]).all()
                continue
            assert np.array_equal(got["mean"][g], w["mean"])
            assert np.array_equal(got["median"][g], w["median"])
            assert np.array_equal(got["quantile"][:, g], w["quantile"])
            assert np.array_equal(got["cov"][g], w["cov"])
    if G == 1:
        assert longest > 2 * 8192                        # the mean's chunks straddle the members' boundaries


def test_nan_zeros_ties_and_empty_groups():
    rng = np.random.default_rng(5)
    T, N = 300, 60
    h = fake_history(rng, T, N, 2, pool=np.array([-0.0, 0.0, 1.0, 1.0, 2.0, -3.0, np.inf]))
    groups = np.repeat(np.arange(6), 10).astype(np.int32)
    groups[50:] = -1                                     # group 5 is empty: its chains are in no group
    h.params[:, :, 40:50] = 0.0                          # group 4: ties only
    h.params[:, :, 40:45] = -0.0
    h.params[7, 0, 13] = np.nan                          # group 1: a NaN in parameter 0
    h.accepted[7, 13] = 1
    h.accepted[:, 20:30] = 0                             # group 2: no accepted draw
    with np.errstate(invalid="ignore"):
        got = GR.group_stats_from_history(h, 0, T, True, groups, PROBS, n_groups=6)
    assert got["count"].tolist()[2] == 0 and got["count"][5] == 0 and got["n_chains"].tolist() == [10, 10, 10, 10, 10, 0]
    assert np.isnan(got["mean"][[2, 5]]).all() and np.isnan(got["median"][[2, 5]]).all() and np.isnan(got["cov"][[2, 5]]).all()
    assert np.isnan(got["mean"][1, 0]) and np.isnan(got["median"][1, 0]) and np.isnan(got["quantile"][:, 1, 0]).all()
    assert not np.isnan(got["median"][1, 1]) and np.isnan(got["cov"][1, 0]).all() and np.isnan(got["cov"][1, :, 0]).all()
    assert got["median"][4].tolist() == [0.0, 0.0] and got["cov"][4].tolist() == [[0.0, 0.0], [0.0, 0.0]]
    for g in (0, 3):                                     # numpy agrees where no sign of a zero decides
        x = np.concatenate([h.params[:, :, c][h.accepted[:, c] != 0].T for c in range(N) if groups[c] == g], axis=1)
        assert np.array_equal(got["mean"][g], x.mean(axis=1))
        assert np.array_equal(np.abs(got["median"][g]), np.abs(np.median(x, axis=1)))
    GR.assert_group_stats_equal(got, got)
    with pytest.raises(AssertionError):
        GR.assert_group_stats_equal(dict(mean=got["mean"] + 1), dict(mean=got["mean"]))


@pytest.mark.parametrize("m", [1, 2, 9, 130, 8192, 8193, 20000])
def test_pairwise_cov_is_chain_cov_ref(m):
    import chain_cov_ref as V
    x = np.random.default_rng(m).standard_normal((3, m)) * [[1.0], [1e-3], [1e6]]
    a, b = GR.column_cov(x), V.column_cov(x)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1], equal_nan=True)


def test_one_group_by_default():
    rng = np.random.default_rng(2)
    h = fake_history(rng, 50, 8, 2)
    a = GR.group_stats_from_history(h, 0, 50, False, None, (0.5,))
    b = GR.group_stats_from_history(h, 0, 50, False, np.zeros(8, np.int32), (0.5,))
    GR.assert_group_stats_equal(a, b)
    assert a["count"].tolist() == [400] and a["n_chains"].tolist() == [8]


def test_abi_declares_and_the_library_exports_smm_get_group_stats():
    from smm_jl_amd import _abi as A
    import ctypes as C
    table = {name: args for name, _, args in A.SYMBOLS}
    assert "smm_get_group_stats" in table and len(table["smm_get_group_stats"]) == 9
    assert [f for f, _ in A.smm_group_stats_t._fields_] == ["count", "n_chains", "mean", "median", "quantile", "cov"]
    lib = C.CDLL(A.LIB_PATH)
    assert hasattr(lib, "smm_get_group_stats")
    assert hasattr(C.CDLL(A.HOOKS_LIB_PATH), "smm_get_group_stats")
    assert b"SMMHIP_GROUP_WIDE_MIN" in open(A.HOOKS_LIB_PATH, "rb").read()
    assert b"SMMHIP_GROUP_WIDE_MIN" not in open(A.LIB_PATH, "rb").read()


def test_the_julia_mirror_of_smm_group_stats_t():
    from test_julia_layer import header_structs, julia_structs
    js = julia_structs(os.path.join(ROOT, "julia", "SMMHip.jl"))
    hs = header_structs()
    ptr = {"Cdouble": "double*", "Int32": "int32_t*", "Int64": "int64_t*"}
    want = [(f, t) for f, t in hs["smm_group_stats_t"]]
    got = [(f, ptr[t[4:-1]]) for f, t in js["SmmGroupStats"]]
    assert got == want
    src = open(os.path.join(ROOT, "julia", "SMMHip.jl")).read()
    assert "hip_group_stats" in src.split("export hip_chain_stats", 1)[1].split("\n", 1)[0]
    back = open(os.path.join(ROOT, "julia", "SMMHipBackend.jl")).read()
    assert "pooled_summary" in back.split("export MAlgoBGPHip", 1)[1].split("\n", 1)[0]
