"""Which forms a context is given, without a GPU: the grid of tests/golden/forms_grid.json replayed through the test seam smm_debug_forms
of libsmmhip_hooks.so (ctx == NULL: check_create_args, create_facts and select_forms as creation calls them, on the DeviceFacts the case
names; no device is touched).  Every case's line — smm_describe's text, every field of Forms, the DeviceFacts — must be the recorded one,
to the character.  The rows of tests/test_gpu_forms.py (TABLE, SHARDS, the user objectives' contexts) are in the grid under their names
there, and their expectations are asserted by that file's own test functions, run here on a stand-in for the module whose contexts
describe themselves through the seam (forms_grid.RowRecorder) with 256 compute units and one workgroup of the candidate persistent
kernel per unit — what every row needs on the MI355X too (tests/test_gpu_forms.py ties the live contexts to the seam).

The grid was recorded (tests/golden/make_forms_grid.py) on the commit BEFORE select_forms and smm_ctx_create were rewritten, with the
seam on a copy of that commit whose facts were the lines of its smm_ctx_create, copied; this file passed there and has not been edited
since.  Forms.ct is the one field with a single value across the grid: no line of select_forms assigns it (8 chains per simulation
tile)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forms_grid as G  # noqa: E402

GRID = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forms_grid.json")))
SPECS = [c for c in GRID if "spec" in c]
ROWS = {c["row"]: c for c in GRID if "row" in c}


def test_the_grid_file_is_no_larger_than_the_largest_fixture():
    assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forms_grid.json")) <= 273901


def test_every_case_of_the_grid_gives_its_recorded_line(hooks):
    assert len(SPECS) >= 400
    wrong = []
    for c in SPECS:
        got = G.line_of_spec(c["spec"])
        if got != G.unpack(c):
            wrong.append((c["spec"], got, G.unpack(c)))
    assert not wrong, "%d of %d cases moved; the first: %s\n  now      %s\n  recorded %s" % ((len(wrong), len(SPECS)) + wrong[0])


def test_the_rows_of_test_gpu_forms_hold_without_a_device(hooks, O):
    """TABLE, SHARDS and the user objectives' contexts of tests/test_gpu_forms.py: that file's assertions, and the recorded lines"""
    import test_gpu_forms as T
    got = G.rows_of_test_gpu_forms(O)   # (runs test_forms_of_single_shards, test_forms_of_shards and test_form_of_a_user_objective)
    assert sorted(got) == sorted(ROWS)
    assert len(got) == len(T.TABLE) + len(T.SHARDS) + 5
    for key, line in got.items():
        assert line == G.unpack(ROWS[key]), key
        assert G.fields(line)["n_cus"] == "256", key


def test_the_grid_cannot_go_quiet():
    """every field of Forms takes at least two values across the grid (ct: one, see above), every value of xk, plan and persist occurs —
    XK_TICKETS under its hook —, and the sizes select_forms tests are straddled"""
    values = {f: set() for f in G.FORMS_FIELDS}
    for c in GRID:
        for f, v in zip(G.FORMS_FIELDS, c["F"]):
            values[f].add(v)
    for f, vs in values.items():
        assert len(vs) >= (1 if f == "ct" else 2), (f, vs)
    assert values["ct"] == {8}
    assert values["xk"] == set(range(len(G.XK))) and values["plan"] == set(range(len(G.PLAN))) and values["persist"] == set(range(len(G.PERSIST)))
    tickets = [c for c in SPECS if c["F"][G.FORMS_FIELDS.index("xk")] == G.XK.index("tickets")]
    assert tickets and all(c["spec"].get("hooks") == {"SMMHIP_DATAFLOW_EXCHANGE": "1"} for c in tickets)
    describes = {}
    for c in GRID:
        for kv in c["describe"].split():
            describes.setdefault(kv.split("=")[0], set()).add(kv.split("=")[1])
    assert len(describes["chain"]) >= 12 and len(describes["walk"]) >= 8 and len(describes["persistent"]) >= 12, describes

    plain = lambda s, **kw: {k: v for k, v in s.items() if k != "N"} == kw   # a case of this family, whatever its N
    def sizes(**kw):
        return {c["spec"]["N"] for c in SPECS if plain(c["spec"], **kw)}
    single = sizes()
    for edge in (4096, 8192, 32768):   # XLVL_MAX, XLDS_MAX, XKEY_MAX: +-1 chain, +-1 tile of 16
        assert {edge - 16, edge - 1, edge, edge + 1, edge + 16} <= single, edge
    assert {65534, 65535, 65536} <= single
    # limits found by bisection: neighbours in N whose answers differ
    def flips(field, **kw):
        i = G.FORMS_FIELDS.index(field)
        by_n = {c["spec"]["N"]: c["F"][i] for c in SPECS if plain(c["spec"], **kw)}
        return [n for n in by_n if n + 1 in by_n and by_n[n] != by_n[n + 1]]
    wide = [n for n in flips("lean_plan", mi=0.5) if n > 4096]
    assert len(wide) == 1 and 7000 < wide[0] < 8192, wide    # the wide lean walk's limit (resolve_lean_bytes against a CU's LDS)
    for npar in (18, 50):
        assert flips("inline_walk", np=npar) and flips("gen_lean", np=npar) and flips("tpw", np=npar, n_cus=16), npar
    # tiles against the compute units, 256 and a smaller count; the occupancy; parameter counts; thresholds; dist_fun; factors; tables;
    # window lengths; shards; hooks
    for n_cus in (256, 64):
        kw = {"n_cus": n_cus}
        assert {16 * n_cus - 16, 16 * n_cus, 16 * n_cus + 16} <= sizes(**kw), n_cus
        assert {32 * n_cus - 32, 32 * n_cus, 32 * n_cus + 32} <= sizes(obj="banana", np=10, **kw), n_cus
        assert {32 * n_cus - 32, 32 * n_cus, 32 * n_cus + 32} <= sizes(np=6, per_cu=2, **kw), n_cus
    seen = lambda key: {json.dumps(c["spec"].get(key), sort_keys=True) for c in SPECS}
    assert {c["spec"].get("per_cu", 1) for c in SPECS} == {-1, 0, 1, 2}
    assert {1, 2, 4, 5, 6, 10, 18, 50, 64} <= {c["spec"].get("np", 2) for c in SPECS}
    assert any(c["spec"].get("batch") for c in SPECS)
    assert {json.dumps(m) for m in (None, 0.5, "nan", -0.1, ["lin", 0.0, 0.5], ["lin", -0.1, 0.5])} <= seen("mi")
    assert {c["spec"].get("dist", 0) for c in SPECS} == {0, 1, 2}
    assert {c["spec"].get("chol") for c in SPECS} == {None, "shared", "per_chain"}
    assert {c["spec"].get("pairs") for c in SPECS} == {None, 31, 32}
    assert any(c["spec"].get("normals") for c in SPECS) and any(c["spec"].get("uniforms") for c in SPECS)
    assert {1, 8, 50000} <= {c["spec"].get("T", 8) for c in SPECS}
    assert {2, 4, 8} <= {c["spec"]["Ng"] // c["spec"]["N"] for c in SPECS if "Ng" in c["spec"]}
    hooked = {}
    for c in SPECS:
        for h in c["spec"].get("hooks", {}):
            hooked[h] = hooked.get(h, 0) + 1
    assert sorted(hooked) == sorted(G.FORM_HOOKS) and min(hooked.values()) >= 3, hooked
