"""smm_get_chain_stats without a device: its numerical contract (include/smmhip.h, restated in chain_stats_ref.py) against numpy,
argument rejection before any device is touched, and the ctypes / Julia mirrors of smm_chain_stats_t against the header."""
import ctypes as C
import os
import re
import subprocess
import tempfile
import warnings

import numpy as np
import pytest

import chain_stats_ref as R
from smm_jl_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBS = (0.0, 0.025, 0.05, 0.1, 0.5, 0.95, 0.975, 1.0)


def numpy_column(x, probs):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return np.mean(x), np.median(x), [np.quantile(x, p) for p in probs]


def column(rng, n, special):
    x = rng.standard_normal(n)
    if special:
        pool = np.array([-np.inf, np.inf, -0.0, 0.0, 1.0, -1.0, 2.5])
        x = np.where(rng.random(n) < 0.3, rng.choice(pool, n), x)
    return x


@pytest.mark.parametrize("special", [False, True])
def test_restatement_equals_numpy_on_random_columns(special):
    rng = np.random.default_rng(3 if special else 4)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for n in list(range(1, 140)) + [255, 256, 257, 1999, 2000]:
            x = column(rng, n, special)
            probs = PROBS + (float(rng.random()),)
            m, md, q = R.column_stats(x, probs)
            nm, nmd, nq = numpy_column(x, probs)
            assert np.array_equal(m, nm, equal_nan=True) and np.signbit(m) == np.signbit(nm), (n, m, nm)
            assert np.array_equal(md, nmd, equal_nan=True), (n, md, nmd)
            assert np.array_equal(np.array(q), np.array(nq), equal_nan=True), (n, q, nq)


@pytest.mark.parametrize("n", [8192, 8193, 16385, 20000])
def test_restatement_equals_numpy_past_one_chunk(n):
    """columns longer than the device's LDS path (8192): the mean's chunks and the radix-select path's ranks"""
    x = np.random.default_rng(n).standard_normal(n) * 1e3 + 7.0
    m, md, q = R.column_stats(x, PROBS)
    nm, nmd, nq = numpy_column(x, PROBS)
    assert m == nm and md == nmd and q == list(nq)


def test_ties_zeros_nan_and_empty():
    for x in ([-0.0], [-0.0, -0.0], [0.0, -0.0, 0.0], [-0.0] * 9, [1.0] * 7 + [2.0] * 7, [np.inf], [-np.inf, np.inf], [np.inf] * 3):
        m, md, q = R.column_stats(np.array(x), PROBS)
        nm, nmd, nq = numpy_column(np.array(x), PROBS)
        assert np.array_equal(m, nm, equal_nan=True) and np.signbit(m) == np.signbit(nm), x
        assert np.array_equal(md, nmd, equal_nan=True), x
        assert np.array_equal(np.array(q), np.array(nq), equal_nan=True), x
        if len(set(np.signbit(x))) == 1:   # (numpy's partition does not order -0 and +0: a uniform column fixes the sign)
            assert np.signbit(md) == np.signbit(nmd) and list(np.signbit(q)) == list(np.signbit(nq)), x
    m, md, q = R.column_stats(np.array([1.0, np.nan, 2.0]), PROBS)
    assert np.isnan(m) and np.isnan(md) and np.isnan(q).all()
    m, md, q = R.column_stats(np.array([]), PROBS)
    assert np.isnan(m) and np.isnan(md) and np.isnan(q).all()


def test_best_and_mode_follow_argmin_and_bincount():
    assert R.argmin_first([3.0, 1.0, 1.0, np.nan, np.nan]) == 3
    assert R.argmin_first([3.0, -0.0, 0.0, -1.0, -1.0]) == 3
    assert R.argmin_first([0.0, -0.0]) == 0
    assert R.mode_of_partners([0, 5, 3, 5, 3, 0, 7]) == 3
    assert R.mode_of_partners([0, 0]) == 0
    assert R.mode_of_partners([9, 2, 9, 2, 2, 9]) == 2


def test_arguments_are_rejected_before_touching_the_device():
    lib = A.load()
    s = A.smm_chain_stats_t()
    p = np.array([0.5])
    assert lib.smm_get_chain_stats(None, 0, 0, 1, None, 0, C.byref(s)) == A.SMM_ERR_INVALID_ARG
    assert lib.smm_get_chain_stats(None, 0, 0, 1, A.dptr(p), 1, None) == A.SMM_ERR_INVALID_ARG
    assert lib.smm_get_chain_stats(None, -1, 5, 0, A.dptr(p), 1, C.byref(s)) == A.SMM_ERR_INVALID_ARG


def test_struct_layout_matches_the_header():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "smmhip.h"
#define O(f) printf(#f " %zu\n", offsetof(smm_chain_stats_t, f))
int main(void) {
  printf("size %zu\n", sizeof(smm_chain_stats_t));
  O(count); O(mean); O(median); O(quantile); O(best_value); O(best_iter); O(n_exchanged); O(most_exchanged_with);
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "p.c"), "-o", os.path.join(d, "p")])
        out = dict(l.rsplit(" ", 1) for l in subprocess.check_output([os.path.join(d, "p")]).decode().strip().splitlines())
    assert int(out.pop("size")) == C.sizeof(A.smm_chain_stats_t)
    assert [f for f, _ in A.smm_chain_stats_t._fields_] == list(out)
    for f, v in out.items():
        assert getattr(A.smm_chain_stats_t, f).offset == int(v), f


def test_julia_mirror_names_the_header_fields_in_order():
    src = open(os.path.join(ROOT, "julia", "SMMHip.jl")).read()
    body = re.search(r"struct SmmChainStats\n(.*?)\nend", src, re.S).group(1)
    fields = [l.split("::")[0].strip() for l in body.splitlines() if l.strip()]
    assert fields == [f for f, _ in A.smm_chain_stats_t._fields_]
    assert "smm_get_chain_stats" in src and "function chain_stats(algo::MAlgoBGPHip" in open(os.path.join(ROOT, "julia", "SMMHipBackend.jl")).read()
