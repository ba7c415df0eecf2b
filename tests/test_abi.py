"""The drop-in boundary: libsmmhip.so loads, exports every symbol include/smmhip.h declares, and the
ctypes mirror has the C layout.  No compute calls: there is no GPU in this tier."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

from smm_jl_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smmhip.h")


def declared_symbols():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(smm_[a-zA-Z_0-9]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    lib = A.load()
    names = declared_symbols()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), "libsmmhip.so does not export %s" % n
    assert sorted(s[0] for s in A.SYMBOLS) == names  # the ctypes table mirrors the header exactly
    assert lib.smm_abi_version() == 3


def test_ctypes_layout_matches_the_header():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "smmhip.h"
#define P(T) printf(#T " %zu\n", sizeof(T))
#define O(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
  P(smm_problem_t); P(smm_bgp_opts_t); P(smm_tables_t); P(smm_history_t); P(smm_state_t); P(smm_timing_t);
  O(smm_problem_t, init); O(smm_problem_t, n_obj_params);
  O(smm_bgp_opts_t, sigma); O(smm_bgp_opts_t, sigma_adjust_by); O(smm_bgp_opts_t, seed); O(smm_bgp_opts_t, device);
  O(smm_tables_t, pairs); O(smm_tables_t, Z); O(smm_history_t, status); O(smm_state_t, best_id); O(smm_timing_t, chain_evals);
  printf("SMM_REDUCE_LANES %d\n", SMM_REDUCE_LANES);
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "p.c"), "-o", os.path.join(d, "p")])
        out = dict(l.rsplit(" ", 1) for l in subprocess.check_output([os.path.join(d, "p")]).decode().strip().splitlines())
    for T in (A.smm_problem_t, A.smm_bgp_opts_t, A.smm_tables_t, A.smm_history_t, A.smm_state_t, A.smm_timing_t):
        assert int(out[T.__name__]) == C.sizeof(T), T.__name__
    for key, v in out.items():
        if "." in key:
            t, f = key.split(".")
            assert getattr(getattr(A, t), f).offset == int(v), key
    assert int(out["SMM_REDUCE_LANES"]) == A.SMM_REDUCE_LANES


def test_no_cpu_fallback_without_a_device():
    """the product fails loudly when there is no HIP device (this tier has none)"""
    import smm_jl_amd as S
    import common as cm
    lib = A.load()
    if lib.smm_device_count() > 0:
        pytest.skip("a GPU is present")
    prob, opts = cm.serial_normal(N=3, T=2)
    with pytest.raises(A.SMMHipError) as e:
        S.hip_context(prob, opts)
    assert e.value.code == A.SMM_ERR_NO_DEVICE and "no CPU fallback" in str(e.value)


def test_invalid_arguments_are_rejected_before_touching_the_device():
    import smm_jl_amd as S
    import common as cm
    prob, opts = cm.general_normal(4, N=3, T=4, batch_size=3)
    with pytest.raises(A.SMMHipError) as e:
        S.hip_context(prob, opts)
    assert e.value.code == A.SMM_ERR_BAD_BATCH
    prob = S.Problem(init=[0.0, 0.0], lb=[-1, -1], ub=[1, 1], mom=[0.0], w=[1.0])  # objfunc_norm needs np == nm
    _, opts = cm.serial_normal(N=3, T=2)
    with pytest.raises(A.SMMHipError) as e:
        S.hip_context(prob, opts)
    assert e.value.code == A.SMM_ERR_INVALID_ARG


def test_zero_initialised_structs_and_bad_tables_are_rejected():
    """a C or Julia caller with a zero-initialised opts struct, NULL vectors or an out-of-range injected pair list
    gets SMM_ERR_INVALID_ARG with a message, not a segfault or a silently different algorithm (exchanges from iteration 1)"""
    import numpy as np
    import smm_jl_amd as S
    import common as cm
    lib = A.load()

    def create(prob, opts, tab=None):
        ps, os_ = prob.struct(), opts.struct(prob.np)
        ts = tab.struct() if tab is not None else None
        return ps, os_, ts

    def rc_of(ps, os_, ts=None):
        ctx = C.c_void_p()
        rc = lib.smm_ctx_create(C.byref(ps), C.byref(os_), C.byref(ts) if ts is not None else None, C.byref(ctx))
        assert not ctx.value
        return rc, lib.smm_last_error(None).decode()

    prob, opts = cm.serial_normal(N=3, T=4)
    for field, value, word in (("exchange_from_iter", 0, "exchange_from_iter"), ("exchange_from_iter", 1, "exchange_from_iter"),
                               ("smpl_iters", 0, "smpl_iters"), ("sigma_update_steps", 0, "sigma_update_steps")):
        ps, os_, _ = create(prob, opts)
        setattr(os_, field, value)
        rc, msg = rc_of(ps, os_)
        assert rc == A.SMM_ERR_INVALID_ARG and word in msg, (field, rc, msg)
    for field in ("sigma", "acc_tuner", "min_improve"):
        ps, os_, _ = create(prob, opts)
        setattr(os_, field, None)
        rc, msg = rc_of(ps, os_)
        assert rc == A.SMM_ERR_INVALID_ARG and "NULL" in msg, field
    for field in ("init", "lb", "ub", "mom", "w"):
        ps, os_, _ = create(prob, opts)
        setattr(ps, field, None)
        rc, msg = rc_of(ps, os_)
        assert rc == A.SMM_ERR_INVALID_ARG and "NULL" in msg, field
    zero = A.smm_bgp_opts_t()      # all zeros
    ps, _, _ = create(prob, opts)
    assert rc_of(ps, zero)[0] in (A.SMM_ERR_INVALID_ARG, A.SMM_ERR_BAD_BATCH)
    for bad in ([[0, 3]], [[2, 1]], [[1, 1]], [[-1, 2]]):
        pairs = np.tile(np.array([[0, 1], [0, 2], [1, 2]], np.int32), (4, 1, 1))
        pairs[2, 1] = bad[0]
        ps, os_, ts = create(prob, opts, S.Tables(pairs=pairs))
        rc, msg = rc_of(ps, os_, ts)
        assert rc == A.SMM_ERR_INVALID_ARG and "pairs" in msg, bad


def test_product_does_not_reference_the_oracle():
    """only tests/, bench.py's cpu_baseline leg and __graft_entry__.smoke() may touch oracle/"""
    pkg = os.path.join(ROOT, "smm.jl_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h", ".cpp")) or f == "Makefile":
                txt = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "oracle" not in txt.lower().replace("# oracle", ""), os.path.join(dirpath, f)
    out = subprocess.check_output(["ldd", A.LIB_PATH]).decode()
    assert "smm_oracle" not in out


def test_the_shipped_library_has_no_test_seams():
    """VERDICT r2 #6 / ADVICE: the switches that force a kernel or shrink a capacity live in libsmmhip_hooks.so only.  The shipped
    library reads three environment variables, all diagnostics (SMMHIP_TS, SMMHIP_DBG, and SMMHIP_VERBOSE: why a user objective's
    persistent kernel did not compile).  (Round 5: the library carries its device headers as text — hiprtc compiles them with a user's
    objective inside —, so the public header's own macros SMMHIP_H / SMMHIP_ABI_VERSION appear in the file too: not variables.)"""
    blob = open(A.LIB_PATH, "rb").read()
    names = sorted(set(m.decode() for m in re.findall(rb"SMMHIP_[A-Z0-9_]+", blob)) - {"SMMHIP_H", "SMMHIP_ABI_VERSION"})
    assert names == ["SMMHIP_DBG", "SMMHIP_TS", "SMMHIP_VERBOSE"], names
    lib = A.load()
    lib.smm_debug_has_test_hooks.restype = C.c_int
    assert lib.smm_debug_has_test_hooks() == 0
    hooks = A.load_hooks()
    assert hooks.smm_debug_has_test_hooks() == 1
    for n in declared_symbols():
        assert hasattr(hooks, n), "libsmmhip_hooks.so does not export %s" % n
    seams = sorted(set(m.decode() for m in re.findall(rb"SMMHIP_[A-Z0-9_]+", open(A.HOOKS_LIB_PATH, "rb").read())))
    assert "SMMHIP_INLINE_WALK" in seams and "SMMHIP_A2A_CAP" in seams
    assert "SMMHIP_STATS_SCRATCH" in seams and "SMMHIP_STATS_MODE_BINS" in seams


def test_chain_kernel_instantiations_are_named_in_the_chooser_only():
    """The host sources name the per-iteration chain kernels (k_chain_iter*, smm_chain.hpp and smm_chain_norm.hpp) in chain_instance()
    (smm_launch_host.hpp) and nowhere else: the launchers, the dynamic-LDS attribute at context creation and smm_describe all go through it, so a kernel that can
    be launched has its attribute set and its name reported by construction.  Reads the sources only."""
    csrc = os.path.join(ROOT, "smm.jl_amd", "csrc")
    strip = lambda txt: re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))
    code = strip(open(os.path.join(csrc, "smm_launch_host.hpp")).read())
    head = "ChainKernel chain_instance(int family, int np, bool b) {"
    assert code.count(head) == 1
    a = code.index(head)
    b = code.index("\n}\n", a)
    body, rest = code[a:b], code[:a] + code[b:] + "".join(strip(open(os.path.join(csrc, f)).read())
                                                           for f in ("smmhip.hip", "smm_user_host.hpp", "smm_run_host.hpp", "smm_forms_host.hpp", "smm_create_host.hpp"))
    assert not re.findall(r"\bk_chain_iter\w*", rest), "a chain kernel is named outside chain_instance()"
    declared = set()
    for h in ("smm_chain.hpp", "smm_chain_norm.hpp"):
        declared |= set(re.findall(r"__global__[^;{]*?\b(k_chain_iter\w*)\s*\(", strip(open(os.path.join(csrc, h)).read())))
    assert len(declared) >= 9 and set(re.findall(r"\bk_chain_iter\w*", body)) == declared
    for line in code.splitlines():
        assert not ("hipFuncAttributeMaxDynamicSharedMemorySize" in line and "k_chain_iter" in line), line
    assert "chain_instance(family, np, b != 0).fn, hipFuncAttributeMaxDynamicSharedMemorySize" in rest


def test_exchange_kernel_instantiations_are_named_in_the_table_only():
    """The host sources name the stand-alone kernels of the exchange (k_exch_*, k_cone_*: smm_exchange.hpp, smm_lookahead.hpp,
    smm_cone_big.hpp) in exch_instance() and nowhere else: every launch of the family, the dynamic-LDS attribute at context creation and
    the name smm_describe prints after exchange= go through that table, so a kernel that can be launched has its attribute set and its
    launch checked by construction.  Reads the sources only."""
    csrc = os.path.join(ROOT, "smm.jl_amd", "csrc")
    strip = lambda txt: re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))
    src = lambda name: strip(open(os.path.join(csrc, name)).read())
    code = src("smm_launch_host.hpp")
    head = "ExchInstance exch_instance(int id, int Ng) {"
    assert code.count(head) == 1
    a = code.index(head)
    b = code.index("\n}\n", a)
    body = code[a:b]
    rest = code[:a] + code[b:] + "".join(src(f) for f in ("smmhip.hip", "smm_user_host.hpp", "smm_forms_host.hpp", "smm_create_host.hpp", "smm_run_host.hpp", "smm_p2p.hpp"))
    family = r"\bk_(?:exch|cone)_\w+"
    assert not re.findall(family + r"\s*[<,)]", rest), "an exchange kernel is named outside exch_instance()"
    declared = set()
    for h in ("smm_exchange.hpp", "smm_lookahead.hpp", "smm_cone_big.hpp"):
        declared |= set(re.findall(r"__global__[^;{]*?\b(k_(?:exch|cone)_\w+)\s*\(", src(h)))
    assert len(declared) >= 14 and set(re.findall(family, body)) == declared
    # the bound of the rows kernel that keeps a shard's own partners: once, in any source of the tree
    hits = 0
    for top in ("smm.jl_amd", "tests", "tools", "oracle", "include", "julia"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith((".hip", ".hpp", ".h", ".py", ".c", ".jl", ".sh")) and os.path.join(dirpath, f) != os.path.abspath(__file__):
                    hits += len(re.findall(r"158 \* 1024", open(os.path.join(dirpath, f), errors="ignore").read()))
    assert hits == 1 and "158 * 1024" in code
    forms = src("smm_forms_host.hpp")
    a = forms.index("std::string describe_text(")
    describe = forms[a:forms.index("\n}\n", a)]
    assert "[]" not in describe and '"lean"' not in describe and '"lvl_big"' not in describe
    assert "exch_instance(resolve_kernel(c, P).id" in describe
    create = src("smm_create_host.hpp")
    assert "exch_instance(id, c->P.Ng)" in create and "id < XI_COUNT" in create


def test_persistent_kernel_instantiations_are_named_in_the_table_only():
    """The host sources name the persistent chain kernels (k_chain_persist_*: smm_chain_persist_gen.hpp, _loc.hpp, _tile.hpp) in
    persist_instance() (smm_launch_host.hpp) and nowhere else: persist_kernel() picks a row of that table, and the occupancy check, every
    launch and the name smm_describe prints after persistent= go through its pick.  Reads the sources only."""
    csrc = os.path.join(ROOT, "smm.jl_amd", "csrc")
    strip = lambda txt: re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))
    src = lambda name: strip(open(os.path.join(csrc, name)).read())
    code = src("smm_launch_host.hpp")
    head = "PersistInstance persist_instance(int id) {"
    assert code.count(head) == 1
    a = code.index(head)
    b = code.index("\n}\n", a)
    body = code[a:b]
    hosts = sorted(f for f in os.listdir(csrc) if f.endswith("_host.hpp") and f != "smm_launch_host.hpp")
    assert "smm_user_host.hpp" in hosts and "smm_create_host.hpp" in hosts
    rest = code[:a] + code[b:] + src("smmhip.hip") + "".join(src(f) for f in hosts)
    family = r"\bk_chain_persist_\w+"
    assert not re.findall(family, rest), "a persistent kernel is named outside persist_instance()"
    declared = set()
    for h in sorted(f for f in os.listdir(csrc) if re.fullmatch(r"smm_chain_persist\w*\.hpp", f)):
        declared |= set(re.findall(r"__global__[^;{]*?\b(k_chain_persist_\w+)\s*\(", src(h)))
    assert len(declared) == 3 and set(re.findall(family, body)) == declared
    assert len(re.findall(family, body)) == 21   # one row per instantiation
    for fn, home in (("PersistKernel persist_kernel(", code), ("int persist_occupancy(", src("smm_create_host.hpp"))):
        assert home.count(fn) == 1, fn
        a = home.index(fn)
        assert "k_chain_persist" not in home[a:home.index("\n}\n", a)], fn
    a = code.index("PersistKernel persist_kernel(")
    assert "persist_instance(id)" in code[a:code.index("\n}\n", a)]


def test_reducer_kernels_and_shared_rules_live_in_the_reducers_host_file():
    """The host side of the history reducers is smm_reducers_host.hpp: smmhip.hip names none of their kernels (smm_stats.hpp, smm_cov.hpp,
    smm_diag.hpp, smm_group.hpp, smm_hist.hpp, smm_trace.hpp, smm_rank.hpp, smm_draws.hpp, smm_moments.hpp, smm_profile.hpp), and the
    rules the family's members share are written there once, so that every member refuses the same arguments in the same words; the
    order statistics of pooled columns are launched from one place, and the max-scan of the state walk lives in smm_window.hpp only.
    Reads the sources only."""
    csrc = os.path.join(ROOT, "smm.jl_amd", "csrc")
    strip = lambda txt: re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))
    src = lambda name: strip(open(os.path.join(csrc, name)).read())
    kernels = r"\bk_(?:stats|cov|diag|group|hist|trace|rank|draws|moment|prof)_\w*"
    main = src("smmhip.hip")
    assert not re.findall(kernels, main), "smmhip.hip names a reducer kernel"
    assert not re.findall(kernels, src("smm_run_host.hpp")), "smm_run_host.hpp names a reducer kernel"
    assert main.count('#include "smm_reducers_host.hpp"') == 1
    host = src("smm_reducers_host.hpp")
    declared = set()
    for h in ("smm_stats.hpp", "smm_cov.hpp", "smm_diag.hpp", "smm_group.hpp", "smm_hist.hpp", "smm_trace.hpp", "smm_rank.hpp",
              "smm_draws.hpp", "smm_moments.hpp", "smm_profile.hpp"):
        declared |= set(re.findall(r"__global__[^;{]*?\b(k_\w+)\s*\(", src(h)))
    assert len(declared) >= 20 and set(re.findall(kernels, host)) == declared
    for k in ("k_group_small", "k_group_hist", "k_group_pick", "k_group_finish"):
        assert len(re.findall(r"launch_checked\(c, %s\b" % k, host)) == 1, k
    for h in ("smm_diag.hpp", "smm_hist.hpp", "smm_trace.hpp"):
        assert "__shfl_up" not in src(h), h
    assert "__shfl_up" in src("smm_window.hpp")
    for message in ("a group id outside [-1, n_groups)", "probs must lie in [0, 1]", "quantile requested without probs",
                    "select must be 0 (all), 1 (accepted) or 2 (state)", "n_groups < 0, or group NULL with n_groups > 0",
                    "n_groups < 0, or group NULL with n_groups != 1"):
        assert host.count('"%s"' % message) == 1, message
        assert message not in main, message


def test_the_run_lives_in_the_run_host_file_with_one_frame_and_one_rule_book():
    """The host side of everything that advances or settles a run is smm_run_host.hpp, included once by smmhip.hip ahead of the reducers'
    host side (whose prelude settles and flushes through it).  Every entry point that takes a context and can throw goes through one frame,
    api_call; the refusals of the sharded protocol that several entry points give are written once; the state a failed persistent launch
    is rolled back to is one struct (Run), not loose members.  Reads the sources only."""
    csrc = os.path.join(ROOT, "smm.jl_amd", "csrc")
    strip = lambda txt: re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))
    names = sorted(f for f in os.listdir(csrc) if f.endswith((".hip", ".hpp")))
    code = {f: strip(open(os.path.join(csrc, f)).read()) for f in names}
    main = code["smmhip.hip"]
    assert main.count('#include "smm_run_host.hpp"') == 1
    assert main.index('#include "smm_run_host.hpp"') < main.index('#include "smm_reducers_host.hpp"')
    assert sum(c.count('"smm_run_host.hpp"') for c in code.values()) == 1
    assert "smm_run_host.hpp" not in open(os.path.join(csrc, "Makefile")).read()   # (not among the sources hiprtc is given)
    everything = "\n".join(code.values())
    for text in ("records are in the gather buffer: call smm_bgp_sharded_finish first", "step beyond maxiter (history capacity)",
                 "the records of the last iteration are in the p2p windows: call smm_bgp_p2p_finish first", "smm_bgp_p2p_init comes first",
                 "exchange before the first local step", "exchange already resolved for this iteration"):
        assert everything.count(text) == 1, text
        assert code["smm_run_host.hpp"].count(text) == 1, text

    def functions_with(pattern):
        """the functions (by name) whose definitions hold the pattern: the nearest line above that starts a definition at column 0"""
        found = set()
        for f in ("smmhip.hip", "smm_user_host.hpp", "smm_forms_host.hpp", "smm_launch_host.hpp", "smm_create_host.hpp", "smm_run_host.hpp",
                  "smm_reducers_host.hpp", "smm_population_host.hpp"):
            lines = code[f].splitlines()
            for i, line in enumerate(lines):
                if pattern not in line:
                    continue
                j = i
                while not re.match(r"[A-Za-z_].*\b\w+\(.*\{", lines[j]):
                    j -= 1
                found.add(re.match(r"[^(]*?(\w+)\(", lines[j]).group(1))
        return found

    no_throw = {"smm_last_error", "smm_stream", "smm_ctx_destroy", "smm_bgp_record_doubles", "smm_bgp_a2a_capacity", "smm_get_timing",
                "smm_set_persistent", "smm_get_persistent", "smm_describe", "smm_set_profiling", "smm_debug_ts", "smm_debug_ts_waves",
                "smm_debug_cone", "smm_debug_forms"}
    assert functions_with("(Ctx*)ctx") == {"api_call"} | no_throw
    assert functions_with("catch (const std::string") == {"api_call", "smm_ctx_create"}
    assert "reducer_call" not in everything
    assert not re.findall(r"\bsnap_(?:iter|cur|pending|prev_open|unresolved|exch_done|slots_iter)\b", everything)
    assert re.search(r"struct Run \{[^}]*\};", main) and len(re.findall(r"^    Run (?:run|snap);", main, flags=re.M)) == 2
    run = code["smm_run_host.hpp"]
    assert "c->snap = c->run;" in run and "c->run = c->snap;" in run
    assert everything.count("k_flush,") == 1 and "void launch_flush(" in run
    assert not re.findall(r"c->kev[01] = |c->ext_(?:rec_in|rec_out|vals_out) = ", main + code["smm_user_host.hpp"] + code["smm_launch_host.hpp"] + code["smm_reducers_host.hpp"] + code["smm_population_host.hpp"])
    assert len(re.findall(r"c->kev0 = ", run)) == 2 and len(re.findall(r"c->ext_rec_in = ", run)) == 2   # (the two scope objects)


def test_the_forms_and_context_creation_live_in_their_host_files_with_each_rule_once():
    """What a context runs and how much LDS that takes is smm_forms_host.hpp, which calls nothing of the HIP API; how a context is made is
    smm_create_host.hpp.  smmhip.hip includes each once and defines none of their functions, hiprtc is given neither.  A compute unit's
    160 KiB of LDS and the key walk's slot block are written once, and every refusal of check_create_args is one text in the tree.
    Reads the sources only."""
    csrc = os.path.join(ROOT, "smm.jl_amd", "csrc")
    strip = lambda txt: re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))
    names = sorted(f for f in os.listdir(csrc) if f.endswith((".hip", ".hpp")))
    code = {f: strip(open(os.path.join(csrc, f)).read()) for f in names}
    main, forms, create = code["smmhip.hip"], code["smm_forms_host.hpp"], code["smm_create_host.hpp"]
    makefile = open(os.path.join(csrc, "Makefile")).read()
    for f in ("smm_user_host.hpp", "smm_forms_host.hpp", "smm_launch_host.hpp", "smm_create_host.hpp"):
        assert main.count('#include "%s"' % f) == 1 and sum(c.count('"%s"' % f) for c in code.values()) == 1, f
        assert f not in makefile, f   # (not among the sources hiprtc is given)
    order = [main.index('#include "%s"' % f) for f in ("smm_user_host.hpp", "smm_forms_host.hpp", "smm_launch_host.hpp", "smm_run_host.hpp",
                                                        "smm_create_host.hpp")]
    assert order == sorted(order)
    assert not re.findall(r"\bhip[A-Z]\w*\(", forms) and "HIPCHK" not in forms
    user, launch = code["smm_user_host.hpp"], code["smm_launch_host.hpp"]
    for fn, home in (("select_forms", forms), ("smm_ctx_create", create), ("alloc_persist", create), ("persist_occupancy", create),
                     ("tile_smem", forms), ("check_create_args", create), ("create_facts", create), ("describe_text", forms),
                     ("rtc_compile", user), ("user_form_compile", user), ("user_form_wanted", user), ("register_user_source", user),
                     ("smm_register_user_objective", user), ("smm_register_user_objective_lanes", user), ("smm_register_user_objective_rng", user),
                     ("exchange_K", launch), ("ensure_windows", launch), ("plan_window_into", launch), ("point_tables", launch),
                     ("chain_instance", launch), ("chain_kernel", launch), ("chain_kernel_p2p", launch), ("launch_chain_iter", launch),
                     ("exch_instance", launch), ("resolve_kernel", launch), ("resolve_rows_window_kernel", launch), ("launch_resolve_p", launch),
                     ("launch_p2p_push", launch), ("launch_resolve_rows_window", launch), ("persist_instance", launch), ("persist_kernel", launch),
                     ("launch_persist", launch)):
        definition = r"^[A-Za-z_][\w:<>\*& ]*\b%s\([^;]*\) \{" % fn
        assert len(re.findall(definition, home, flags=re.M)) == 1, fn
        assert not re.findall(definition, main, flags=re.M), fn
    # the way through hiprtc is smm_user_host.hpp's alone, and so are its one refusal and the map-reduce reduction's text
    hosts = "\n".join(code[f] for f in names if f == "smmhip.hip" or f.endswith("_host.hpp"))
    assert not re.findall(r"\bhiprtc\w*\(", main) and "g_rtc" not in main
    assert hosts.count('"hiprtcCreateProgram failed"') == 1 and '"hiprtcCreateProgram failed"' in user
    assert hosts.count("a = a + __shfl_xor(a, off, 64);") == 1 and "a = a + __shfl_xor(a, off, 64);" in user
    three = main + user + forms + launch + create   # (the three files this code stood in, and the two that took the rest of smmhip.hip's)
    assert len(re.findall(r"160 \* 1024", three)) == 1 and "160 * 1024" in forms
    assert not re.findall(r"\b80 \* 1024", three)
    # (the key walk's slot block: the host takes it from the layout description of smm_walk_lean.hpp, the one place that states it)
    assert not re.findall(r"\(\(\(\w+ \+ 3\) & ~3\) \+ \d+\) \* (?:8|16)", "\n".join(code.values()))
    assert "size_t key_slot_bytes(int Ng) { return LeanLayout<LEAN_KEYS>::slot_bytes(Ng); }" in forms
    assert "\n".join(code.values()).count("SLOT * (Ng4 + PAD)") == 1 and "SLOT * (Ng4 + PAD)" in code["smm_walk_lean.hpp"]
    a = create.index("int check_create_args(")
    refusals = re.findall(r'fail\(nullptr, SMM_ERR_\w+, "([^"]+)"\)', create[a:create.index("\n}\n", a)])
    assert len(refusals) == 17 and len(set(refusals)) == 17
    everything = "\n".join(code.values())
    for text in refusals:
        assert everything.count('"%s"' % text) == 1, text
    assert "hipGetDeviceCount" not in create[a:create.index("\n}\n", a)]
    assert create.index("check_create_args(prob, opts, tab, out)") < create.index("hipGetDeviceCount(&ndev)")


def test_the_accept_step_is_written_once_in_smm_accept_hpp():
    """What a chain does at the end of an iteration — the accept decision, the accept rate and the sigma update, best and best_id, the head
    of a history row, the swapped row, the banana — is written in smm_accept.hpp and nowhere else: the five chain kernels, k_flush, the two
    apply kernels of the sharded paths and the population's install call it.  hiprtc is given the header ahead of the files that use it.
    Reads the sources only."""
    csrc = os.path.join(ROOT, "smm.jl_amd", "csrc")
    strip = lambda txt: re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))
    names = sorted(f for f in os.listdir(csrc) if f.endswith(".hpp") or f == "smmhip.hip")
    code = {f: strip(open(os.path.join(csrc, f)).read()) for f in names}
    assert "smm_accept.hpp" in code
    for what, pattern in (("the sigma update's threshold", r"0\.234"), ("the test for a finite prob", r"isfinite\(prob\)"),
                          ("an assignment to a row's exchanged field", r"\[H_EXCH\]\s*="), ("the banana's term", r"100\.0 \*")):
        holders = [f for f in names if re.search(pattern, code[f])]
        assert holders == ["smm_accept.hpp"], (what, holders)
    assert not any("make_swapped_history" in c for c in code.values())
    embed = re.search(r"^EMBED = (.*)$", open(os.path.join(csrc, "Makefile")).read(), flags=re.M).group(1).split()
    assert embed.index("smm_accept.hpp") < embed.index("smm_chain.hpp")
