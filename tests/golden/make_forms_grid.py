#!/usr/bin/env python
"""Generates tests/golden/forms_grid.json: a grid of contexts' inputs, each with the one line the test seam smm_debug_forms gives for it
without a device (smm_describe's text, every field of Forms, the DeviceFacts; kept without the fields' names: forms_grid.pack / unpack) — what select_forms decides, recorded so that a change of
the selection logic that moves a case shows up in tests/test_forms.py on a machine without a GPU.

The grid is no full product.  It holds every row of tests/test_gpu_forms.py (by its name there), and around them the sizes at which
select_forms tests something: the population against XLVL_MAX, XLDS_MAX, 32768 and 65535 at +-1 chain and +-1 whole tile, the limits
found by bisection on the seam's own answer (the wide lean walk's ~7400 chains; the largest population whose tile still leaves room for
the inline walk, where the LDS admission test holds with equality), tiles against the compute units, the occupancy, parameter counts,
thresholds, dist_fun, Cholesky factors, injected tables, window lengths, shards and every hook select_forms reads.

    python tests/golden/make_forms_grid.py        # rewrites tests/golden/forms_grid.json
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import forms_grid as G  # noqa: E402
from oracle import oracle as O  # noqa: E402
from smm_jl_amd import _abi as A  # noqa: E402


def last_with(spec, field, value, lo, hi, step=1):
    """the largest N in [lo, hi] (multiples of step from lo) whose line has F.<field> == value: lo has it, hi has not"""
    has = lambda n: G.fields(G.line_of_spec(dict(spec, N=n)))["F." + field] == value
    assert has(lo) and not has(hi), (spec, field, lo, hi)
    a, b = 0, (hi - lo) // step
    while b - a > 1:
        m = (a + b) // 2
        a, b = (m, b) if has(lo + m * step) else (a, m)
    return lo + a * step


def specs():
    out = []
    add = lambda **kw: out.append(kw)
    # the population against the sizes select_forms names: +-1 chain, +-1 tile of 16
    for N in (1, 2, 3, 16, 4080, 4095, 4096, 4097, 4112, 8176, 8191, 8192, 8193, 8208, 32752, 32767, 32768, 32769, 32784, 65534, 65535, 65536):
        add(N=N)
        if N <= 8208:
            add(N=N, mi=0.5)
            add(obj="banana", np=10, N=N)
    for N in (4064, 4128, 8160, 8224, 2048, 2080, 1000, 32):
        add(obj="banana", np=10, N=N)
    # the wide lean walk's limit (resolve_lean_bytes(N, N, true) against a CU's LDS), by bisection on F.lean_plan
    n = last_with({"mi": 0.5}, "lean_plan", "1", 4097, 8192)
    for N in (n - 1, n, n + 1):
        add(N=N, mi=0.5)
        add(N=N // 2 * 2, Ng=N // 2 * 2, mi=0.5)
    for G_ in (2, 4):   # ... and a shard of such a population (shard_wide_big)
        Ng = (n + 1 + 16 * G_) // (16 * G_) * (16 * G_)
        add(N=Ng // G_, Ng=Ng, offset=Ng // G_, mi=0.5)
        add(N=Ng // G_, Ng=Ng, offset=Ng // G_, mi=0.0)
    # the inline walk's LDS: the largest population whose tile still leaves room for the 16-byte slots (equality holds there: the slots
    # are 16 bytes a chain and the tile is a multiple of 16), and its lean form
    for npar in (18, 50):
        n = last_with({"np": npar}, "inline_walk", "1", 64, 4096)
        for N in (n - 1, n, n + 1):
            add(np=npar, N=N)
        n = last_with({"np": npar}, "gen_lean", "1", 64, 4096)
        for N in (n - 1, n, n + 1):
            add(np=npar, N=N)
        n = last_with({"np": npar, "n_cus": 16}, "tpw", "2", 256, 4096)
        for N in (n - 1, n, n + 1):
            add(np=npar, N=N, n_cus=16)
    # tiles against the compute units (N / 16 for the loc form, N / 32 for gen, N / 16 against 2 x for the tile form), 256 units and 64
    for n_cus in (256, 64):
        for N in (16 * n_cus - 16, 16 * n_cus, 16 * n_cus + 16):
            add(N=N, n_cus=n_cus)
            add(N=N, Ng=2 * N, offset=N, n_cus=n_cus)
        for N in (32 * n_cus - 32, 32 * n_cus, 32 * n_cus + 32):
            add(obj="banana", np=10, N=N, n_cus=n_cus)
            add(np=6, N=N, n_cus=n_cus, per_cu=2)
            add(np=6, N=N // 2, Ng=N, n_cus=n_cus // 2, per_cu=2)
        add(np=6, N=8 * n_cus + 1, n_cus=n_cus)
        add(np=6, N=8 * n_cus, n_cus=n_cus)
    # the occupancy: not asked, not available, one and two workgroups per unit
    for per_cu in (-1, 0, 1, 2):
        add(N=4096, per_cu=per_cu)
        add(N=2048, Ng=4096, offset=2048, per_cu=per_cu)
        add(np=6, N=8192, per_cu=per_cu)
        add(np=6, N=4096, Ng=8192, per_cu=per_cu)
        add(obj="banana", np=10, N=8192, per_cu=per_cu)
        add(obj="banana", np=10, N=2048, per_cu=per_cu)
        add(obj="dense", np=50, N=4096, per_cu=per_cu)
        add(N=4096, Ng=32768, offset=4096, per_cu=per_cu)
    # parameter counts; batches smaller than the parameters
    for npar in (1, 2, 4, 5, 6, 10, 18, 50, 64):
        for N in (64, 1024, 4096):
            add(np=npar, N=N)
        add(obj="banana", np=npar, N=2048)
        add(obj="banana", np=npar, N=8192)
        add(obj="dense", np=npar, nm=npar, N=1024)
        add(obj="dense2", np=npar, nm=npar, N=1024)
        if npar % 2 == 0:
            add(np=npar, N=64, batch=npar // 2)
            add(obj="banana", np=npar, N=2048, batch=npar // 2)
    add(obj="dense", np=50, nm=50, N=4096)
    add(obj="dense2", np=50, nm=50, N=4096)
    add(obj="dense", np=50, nm=50, N=4095)
    add(obj="dense", np=50, nm=50, N=4112)
    add(obj="dense", np=50, nm=50, N=2048, Ng=4096)
    add(obj="dense", np=64, nm=64, N=256)
    add(obj="dense2", np=64, nm=64, N=256)
    # thresholds x dist_fun
    for mi in (0.0, 0.5, "nan", -0.1, ["lin", 0.0, 0.5], ["lin", -0.1, 0.5]):
        for dist in (0, 1, 2):
            add(N=64, mi=mi, dist=dist)
            add(N=4096, mi=mi, dist=dist)
            add(np=6, N=64, mi=mi, dist=dist)
        add(N=8192, mi=mi)
        add(N=32768, mi=mi)
        add(N=2048, Ng=4096, offset=2048, mi=mi)
        add(np=6, N=2048, Ng=4096, offset=2048, mi=mi)
        add(obj="banana", np=10, N=2048, mi=mi)
        add(obj="banana", np=10, N=8192, mi=mi)
        add(obj="dense", np=50, N=4096, mi=mi)
    add(N=32768, dist=1)
    add(N=40000, dist=2)
    # Cholesky factors
    for chol in ("shared", "per_chain"):
        add(N=64, chol=chol)
        add(np=6, N=64, chol=chol)
        add(np=6, N=32, Ng=64, offset=32, chol=chol)
        add(obj="banana", np=10, N=2048, chol=chol)
        add(obj="dense", np=50, N=256, chol=chol)
    # injected tables: a pair list at and past LV_MAXLEV = 31 levels, normals, uniforms
    for pairs in (31, 32):
        add(N=64, pairs=pairs)
        add(N=64, mi=0.5, pairs=pairs)
        add(np=6, N=64, pairs=pairs)
        add(obj="banana", np=10, N=64, pairs=pairs)
        add(N=32, Ng=64, offset=32, pairs=pairs)
    add(N=64, normals=3)
    add(N=64, uniforms=True)
    add(N=64, normals=12, uniforms=True)
    add(np=6, N=64, normals=3)
    add(N=4096, normals=2, T=2)
    # window lengths
    for T in (1, 8, 50000):
        add(N=3, T=T)
        add(N=4096, T=T)
        add(N=32768, T=T)
        add(np=6, N=64, T=T)
        add(obj="banana", np=10, N=8192, T=T)
    add(N=4096, T=300)
    add(np=18, N=4096, T=300)
    add(N=32768, T=300)
    # shards of 2, 4 and 8
    for G_ in (2, 4, 8):
        for Ng in (256, 4096, 8192, 32768, 65536):
            add(N=Ng // G_, Ng=Ng, offset=Ng // G_)
            add(N=Ng // G_, Ng=Ng, offset=Ng // G_, mi=0.5)
        add(np=6, N=4096 // G_, Ng=4096, offset=0)
        add(obj="dense", np=50, N=4096 // G_, Ng=4096, offset=4096 // G_)
        add(obj="banana", np=10, N=4096 // G_, Ng=4096, offset=4096 // G_)
    add(N=1000, Ng=2000, offset=1000)
    add(N=8, Ng=16 * 8, offset=8)
    add(N=16, Ng=16 * 16, offset=16)      # more ranks than the p2p windows hold
    add(np=6, N=16, Ng=16 * 16, offset=16)
    # every hook select_forms reads, each alone
    bases = [dict(N=64), dict(N=4096), dict(N=8192), dict(N=32768), dict(np=6, N=64), dict(np=6, N=4096), dict(obj="banana", np=10, N=8192),
             dict(obj="banana", np=10, N=2048), dict(obj="dense", np=50, N=4096), dict(N=2048, Ng=4096, offset=2048), dict(N=4096, T=300)]
    values = {"SMMHIP_ANY_EXCHANGE": ["1"], "SMMHIP_DATAFLOW_EXCHANGE": ["1"], "SMMHIP_BIG_EXCHANGE": ["1"], "SMMHIP_NORM_NARROW": ["0", "1"],
              "SMMHIP_TPW": ["1", "2"], "SMMHIP_NO_CONE": ["1"], "SMMHIP_PLAN_CAP": ["3"], "SMMHIP_DBG": ["1"]}
    for hook in G.FORM_HOOKS:
        for v in values.get(hook, ["0"]):
            for b in bases:
                add(hooks={hook: v}, **b)
    # (the ticket kernel stands in only where no lean plan does: thresholds below 0, another dist_fun)
    add(N=64, mi=-0.1, hooks={"SMMHIP_DATAFLOW_EXCHANGE": "1"})
    add(N=8192, dist=1, hooks={"SMMHIP_DATAFLOW_EXCHANGE": "1"})
    add(np=6, N=4096, mi=["lin", -0.1, 0.5], hooks={"SMMHIP_DATAFLOW_EXCHANGE": "1"})
    return out


def main():
    A._lib = A.load_hooks()   # (user objectives register with the build that has the seam)
    O.load()
    cases = [dict(G.pack(v), row=k) for k, v in G.rows_of_test_gpu_forms(O).items()]
    seen = set()
    for s in specs():
        key = json.dumps(s, sort_keys=True)
        if key in seen:
            continue
        seen.add(key)
        line = G.line_of_spec(s)
        assert G.unpack(G.pack(line)) == line
        cases.append(dict(G.pack(line), spec=s))
    path = os.path.join(HERE, "forms_grid.json")
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(c, sort_keys=True) for c in cases) + "\n]\n")
    print(len(cases), "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
