"""phase stamps of k_exch_plan (workgroup 0 of the last launch) and of k_exch_plan_bg, beside a running chain kernel and alone:
python tools/plan_ts.py [chains]   (the test build: the background kernel is launched alone through its seam)"""
import ctypes as C, os, sys
import numpy as np
os.environ["SMMHIP_TS"] = "1"
sys.path.insert(0, '.'); sys.path.insert(0, 'tests')
import smm_jl_amd as S, common as cm
N = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
lib = S._abi.use_test_hooks(True)
prob, opts = cm.serial_normal(N=N, T=600)
ctx = S.hip_context(prob, opts)
ctx.step(300)
names = ["pairs sampled", "histogram..ranks", "levels (Jacobi sweeps)", "level sort + lean list", "cone: zero + seed", "cone: propagate", "cone: count", "cone: layout", "cone: scatter + gather"]


def stamps(first, title, last_pass_only):
    x = np.zeros(100, np.uint64)
    lib.smm_debug_ts(ctx._ctx, x.ctypes.data_as(C.c_void_p), -1)
    t = x[first:first + 10].astype(np.float64) / 100.0
    if not t[9]:
        print("%s: no stamps (the kernel did not run)" % title)
        return
    print(title)
    for i, n in enumerate(names):
        # (the background kernel passes over the tiles several times: the cone stamps are the LAST pass's, the time from the level sort to the
        # last pass's start is the earlier passes')
        print("  %-28s %8.2f us" % (("earlier cone passes + " if last_pass_only and i == 4 else "") + n, t[i + 1] - t[i]))
    print("  %-28s %8.2f us" % ("total", t[9] - t[0]))


stamps(80, "k_exch_plan, on the main stream (the first window's)", False)
beside = ctx.plan_beside_info()
print("plans beside the chain kernel: %s, windows beside / in stream: %d / %d" % beside)
if beside[0]:
    stamps(90, "k_exch_plan_bg beside k_chain_persist_loc (the window entered last)", True)
    lib.smm_debug_plan_into.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    assert lib.smm_debug_plan_into(ctx._ctx, 1, 301, 1) == 0
    stamps(90, "k_exch_plan_bg alone", True)
