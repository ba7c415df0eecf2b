"""The residency of the background plan kernel beside the persistent chain kernel, held to the figures it is argued from
(smm.jl_amd/csrc/smm_create_host.hpp, choose_plan_beside): read from the kernel metadata of the BUILT library's gfx950 code object and
from the sizes the host code computes.  No device.  Without this a later change that costs k_chain_persist_loc a register or
k_exch_plan_bg a kilobyte silently serialises the two kernels again — same results, the plan back on the critical path."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

from smm_jl_amd import _abi as A

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
FILE, GRANT = 512, 8          # registers per lane and SIMD of the unified file; granted in steps of 8
CHAIN_CAP, BG_CAP = 120, 32


@pytest.fixture(scope="module")
def kernels():
    """name (demangled) -> metadata of every kernel of libsmmhip.so"""
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "dev.co")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, A.LIB_PATH, os.path.join(d, "copy.so")])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                               "--input=" + fat, "--output=" + co])
        notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
    out = {}
    for block in re.split(r"\n  - \.agpr_count:", "\n" + notes)[1:]:
        m = re.search(r"\n    \.name:\s+(\S+)", block)
        if not m:
            continue
        num = lambda key: int(re.search(r"\n    \." + key + r":\s+(\d+)", block).group(1))
        out[m.group(1)] = dict(agpr=int(block.split()[0]), vgpr=num("vgpr_count"), lds=num("group_segment_fixed_size"),
                               wg=num("max_flat_workgroup_size"), scratch=num("private_segment_fixed_size"))
    names = subprocess.check_output(["c++filt"], input="\n".join(out), text=True).split("\n")
    return {n: v for n, v in zip(names, out.values())}


def allocated(k):
    return -(-(k["vgpr"] + k["agpr"]) // GRANT) * GRANT


def budget(np_, Ng=4096, K=4096):
    lib = A.load_hooks()
    lib.smm_debug_plan_beside_budget.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong)]
    out = (C.c_longlong * 7)()
    assert lib.smm_debug_plan_beside_budget(np_, Ng, K, out) == 0
    return dict(chain_lds=out[0], bg_lds=out[1], cu_lds=out[2], granule=out[3], max_n=out[4], fits=out[5], bg_static=out[6])


def test_every_chain_instantiation_is_capped_and_the_background_kernel_fits_what_is_left(kernels):
    chain = {n: k for n, k in kernels.items() if "k_chain_persist_loc<" in n}
    bg = {n: k for n, k in kernels.items() if "k_exch_plan_bg" in n}
    assert len(chain) == 10 and len(bg) == 1, (sorted(chain), sorted(bg))
    b = next(iter(bg.values()))
    assert allocated(b) <= BG_CAP and b["wg"] == 256, b
    for n, k in chain.items():
        assert k["wg"] == 1024, n
        assert allocated(k) <= CHAIN_CAP, (n, k)
        assert FILE // allocated(k) >= 4, (n, k)                      # occupancy 4: the workgroup's four waves per SIMD
        assert 4 * allocated(k) + allocated(b) <= FILE, (n, k, b)     # ... and a fifth wave of the background kernel beside them
        assert k["lds"] == 0, (n, k)                                  # (all of its LDS is the dynamic request: persist_loc_smem_bytes)
    assert 16 + 4 <= 32                                               # wave slots of a compute unit: 16 chain waves, 4 background waves


@pytest.mark.parametrize("np_", [1, 2])
def test_lds_of_one_chain_workgroup_and_one_background_workgroup(kernels, np_):
    b = next(k for n, k in kernels.items() if "k_exch_plan_bg" in n)
    f = budget(np_)
    assert f["cu_lds"] == 160 * 1024 and f["granule"] == 1280
    up = lambda x: -(-x // f["granule"]) * f["granule"]
    assert b["lds"] <= f["bg_static"]                                  # what the host's residency rule allows the compiler to add (PBG_LDS_STATIC)
    request = f["bg_lds"] + b["lds"]                                  # the dynamic request and what the compiler adds to it
    assert f["chain_lds"] + request <= f["cu_lds"]
    assert up(f["chain_lds"]) + up(request) <= f["cu_lds"]            # ... as the hardware grants them
    assert f["bg_lds"] <= f["cu_lds"] - f["chain_lds"] - f["granule"]
    assert f["bg_lds"] > 80 * 1024                                    # two background workgroups never share a compute unit
    assert f["fits"] == 1 and f["max_n"] >= 4096                      # the benchmark's population is planned beside


def test_the_size_rule():
    f = budget(2)
    n = f["max_n"]
    assert budget(2, n, n)["fits"] == 1 and budget(2, n + 1, n + 1)["fits"] == 0
    assert budget(2, 8192, 8192)["fits"] == 0
