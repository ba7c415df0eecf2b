"""The grid of tests/golden/forms_grid.json: how a case's inputs are written down (a small dict), how they become Problem / BGPOpts / Tables,
and how the test seam smm_debug_forms of libsmmhip_hooks.so is asked for the one line that says which forms such a context is given —
without a device (ctx == NULL: check_create_args, create_facts, select_forms) or of a live context.  Shared by the generator
(tests/golden/make_forms_grid.py), tests/test_forms.py and tests/test_gpu_forms.py."""
import ctypes as C
import os

import numpy as np

import smm_jl_amd as S
from smm_jl_amd import _abi as A

FORMS_FIELDS = ("plan", "xk", "rows_cap", "lean_plan", "lean_wide", "plan_ahead", "win_cap", "plan_cap", "ct", "norm_fast", "norm_narrow",
                "tpw", "tile_off", "inline_walk", "gen_lean", "gen_keys", "dense_keys", "cone", "cone_big", "walk_slots", "cone_tiles",
                "cone_ct", "cone_gather", "persist", "persist_wide", "persist_sh", "persist_sh_big", "persist_user", "max_tiles",
                "defer_resolve")
XK = ("lean", "lvl", "lvl_soa", "tickets", "rows", "key", "lvl_big", "any")   # ExchKernel, in order
PLAN = ("none", "lds", "big")                                                    # PlanKind
PERSIST = ("none", "gen", "loc", "tile")                                         # PersistKind
# every variable read_hooks reads into a field select_forms tests, and SMMHIP_DBG (no hook: the shipped library reads it too, into P.dbg)
FORM_HOOKS = ("SMMHIP_DBG", "SMMHIP_ANY_EXCHANGE", "SMMHIP_DATAFLOW_EXCHANGE", "SMMHIP_BIG_EXCHANGE", "SMMHIP_KEY_EXCHANGE", "SMMHIP_KEY_WALK",
              "SMMHIP_INLINE_WALK", "SMMHIP_NORM_FAST", "SMMHIP_NORM_NARROW", "SMMHIP_TPW", "SMMHIP_DENSE_KEYS", "SMMHIP_NO_CONE",
              "SMMHIP_PERSIST", "SMMHIP_PERSIST_LOC", "SMMHIP_PERSIST_TILE", "SMMHIP_CONE_BIG", "SMMHIP_PLAN_AHEAD", "SMMHIP_PLAN_CAP")


def seam():
    lib = A.load_hooks()
    fn = lib.smm_debug_forms
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.POINTER(A.smm_problem_t), C.POINTER(A.smm_bgp_opts_t), C.POINTER(A.smm_tables_t), C.c_int, C.c_int,
                   C.c_char_p, C.c_int]
    return lib, fn


def line_without_device(prob, opts, tab=None, n_cus=256, per_cu=1, hooks=None):
    """the seam's line for what creation would choose; hooks: SMMHIP_* variables set for the call only"""
    lib, fn = seam()
    ps, os_ = prob.struct(), opts.struct(prob.np)
    ts = tab.struct() if tab is not None else None
    buf = C.create_string_buffer(2048)
    saved = {k: os.environ.get(k) for k in (hooks or {})}
    os.environ.update(hooks or {})
    try:
        rc = fn(None, C.byref(ps), C.byref(os_), C.byref(ts) if ts is not None else None, n_cus, per_cu, buf, 2048)
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    if rc != 0:
        return "error %d: %s" % (rc, lib.smm_last_error(None).decode())
    return buf.value.decode()


def line_of_context(ctx):
    """the seam's line for a live BGPContext of the hooks build: its forms and the DeviceFacts it was created with"""
    _, fn = seam()
    buf = C.create_string_buffer(2048)
    assert fn(ctx._ctx, None, None, None, 0, 0, buf, 2048) == 0
    return buf.value.decode()


def fields(line):
    """the line as a dict: smm_describe's keys, the fields of Forms as "F.<name>", n_cus and per_cu"""
    return dict(kv.split("=", 1) for kv in line.split())


def pack(line):
    """a line as the grid file keeps it: smm_describe's text, the values of Forms' fields in FORMS_FIELDS' order, the DeviceFacts — the
    names are the same in every line (unpack puts them back)"""
    toks = line.split()
    k = next(i for i, t in enumerate(toks) if t.startswith("F."))
    tail = toks[k:]
    assert [t.split("=")[0] for t in tail] == ["F." + f for f in FORMS_FIELDS] + ["n_cus", "per_cu"], line
    vals = [int(t.split("=")[1]) for t in tail]
    return {"describe": " ".join(toks[:k]), "F": vals[:-2], "dev": vals[-2:]}


def unpack(rec):
    """the exact line of a packed record"""
    assert len(rec["F"]) == len(FORMS_FIELDS) and len(rec["dev"]) == 2
    return " ".join([rec["describe"]] + ["F.%s=%d" % (f, v) for f, v in zip(FORMS_FIELDS, rec["F"])] + ["n_cus=%d per_cu=%d" % tuple(rec["dev"])])


def build(spec):
    """(Problem, BGPOpts, Tables or None, n_cus, per_cu, hooks) of a case's spec"""
    obj, npar = spec.get("obj", "norm"), spec.get("np", 2)
    N = spec["N"]
    Ng, T, ns = spec.get("Ng", N), spec.get("T", 8), spec.get("ns", 64)
    if obj == "norm":
        prob = S.Problem(init=np.zeros(npar), lb=-3 * np.ones(npar), ub=3 * np.ones(npar), mom=np.zeros(npar), w=np.ones(npar), ns=ns)
    elif obj == "banana":
        prob = S.Problem(init=np.zeros(npar), lb=-2 * np.ones(npar), ub=2 * np.ones(npar), mom=np.zeros(npar), w=np.ones(npar), ns=1,
                         objective_id=A.SMM_OBJ_BANANA)
    else:
        nm = spec.get("nm", npar)
        prob = S.Problem(init=np.zeros(npar), lb=-np.ones(npar), ub=np.ones(npar), mom=np.zeros(nm), w=np.ones(nm), ns=1,
                         objective_id=A.SMM_OBJ_DENSE2 if obj == "dense2" else A.SMM_OBJ_DENSE)
    mi = spec.get("mi", 0.0)
    if mi == "nan":
        mi = np.full(Ng, np.nan)
    elif isinstance(mi, list):      # ["lin", a, b]: per chain, a .. b
        mi = np.linspace(mi[1], mi[2], Ng)
    else:
        mi = np.full(Ng, float(mi))
    chol = {None: None, "shared": np.eye(npar), "per_chain": np.tile(np.eye(npar), (Ng, 1, 1))}[spec.get("chol")]
    opts = S.BGPOpts(N=N, maxiter=T, sigma=np.full(Ng, 0.05), acc_tuner=np.ones(Ng), min_improve=mi, N_global=Ng,
                     chain_offset=spec.get("offset", 0), batch_size=spec.get("batch"), dist_fun=spec.get("dist", 0), chol_L=chol)
    tab = None
    if spec.get("pairs") or spec.get("normals") or spec.get("uniforms"):
        pairs = None
        if spec.get("pairs"):       # a chain of `pairs` pairs (0,1), (1,2), ...: as many dependency levels as pairs
            d = spec["pairs"]
            pairs = np.tile(np.stack([np.arange(d), np.arange(1, d + 1)], 1).astype(np.int32), (T, 1, 1))
        tab = S.Tables(pairs=pairs, prop_normals=np.zeros((T, spec["normals"], npar, N)) if spec.get("normals") else None,
                       probs_acc=np.zeros((T, N)) if spec.get("uniforms") else None)
    return prob, opts, tab, spec.get("n_cus", 256), spec.get("per_cu", 1), spec.get("hooks")


def line_of_spec(spec):
    prob, opts, tab, n_cus, per_cu, hooks = build(spec)
    return line_without_device(prob, opts, tab, n_cus, per_cu, hooks)


def own_registrations():
    """user objectives registered inside belong to the library that is current inside (tests/test_gpu_user_shapes.py keeps one
    registration per source and process)"""
    import test_gpu_user_shapes as U
    return U.fresh_registrations()


class RowRecorder:
    """stands in for the smm_jl_amd module in the tests of tests/test_gpu_forms.py: hip_context(...) gives an object whose describe() is the
    describe part of the seam's line without a device (n_cus = 256); the lines are kept in the order of the calls"""

    def __init__(self, per_cu=1):
        self.per_cu, self.lines = per_cu, []
        self.Problem, self.BGPOpts, self.Tables, self.register_user_objective = S.Problem, S.BGPOpts, S.Tables, S.register_user_objective

    def hip_context(self, prob, opts, tab=None):
        line = line_without_device(prob, opts, tab, 256, self.per_cu)
        self.lines.append(line)
        class Described:
            def describe(self):
                d = fields(line)
                return {k: v for k, v in d.items() if not k.startswith("F.") and k not in ("n_cus", "per_cu")}
        return Described()


class LiveRecorder:
    """the same stand-in on the GPU: hip_context(...) creates the context (of the library that is current: the hooks build) and keeps
    (prob, opts, tables, context) in the order of the calls"""

    def __init__(self):
        self.made = []
        self.Problem, self.BGPOpts, self.Tables, self.register_user_objective = S.Problem, S.BGPOpts, S.Tables, S.register_user_objective

    def hip_context(self, prob, opts, tab=None):
        ctx = S.hip_context(prob, opts, tab)
        self.made.append((prob, opts, tab, ctx))
        return ctx


def rows_of_test_gpu_forms(O):
    """{key: line} of every row of TABLE and SHARDS and of the contexts of the user-objective test of tests/test_gpu_forms.py, each through
    that file's own test function (so its expectations are asserted as it states them)"""
    import test_gpu_forms as G
    out = {}
    for row in G.TABLE:
        R = RowRecorder()
        G.test_forms_of_single_shards(R, row)
        out["table: " + row[0]] = R.lines[0]
    for row in G.SHARDS:
        R = RowRecorder()
        G.test_forms_of_shards(R, row)
        out["shards: " + row[0]] = R.lines[0]
    R = RowRecorder()
    with own_registrations():
        G.test_form_of_a_user_objective(R, O)
    for i, line in enumerate(R.lines):
        out["user: context %d" % i] = line
    return out
