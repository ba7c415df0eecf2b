"""Registers / spills / scratch / LDS of the kernels a user objective with the library's stream is compiled into, as the compiler reports them
(cross-compiles for gfx950, no GPU needed).  The translation units are assembled from the same prelude and kernel texts libsmmhip hands to
hiprtc (the string constants of smm_user_host.hpp), around tests/user_rng_src.py's sources:
  python tools/user_rng_resources.py"""
import ast
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "smm.jl_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tests"))
from user_objective_src import AR1_SOURCE, PANEL_SOURCE  # noqa: E402
from user_rng_src import AR1_RNG_SOURCE, PANEL_RNG_SOURCE  # noqa: E402

HIP = open(os.path.join(CSRC, "smm_user_host.hpp")).read()
# (the map-reduce kernels' shared ending is a macro of string literals: put where it is used)
_reduce = re.search(r"#define USER_REDUCE_LANES \\\n((?:[^\n]*\\\n)*[^\n]*)\n", HIP)
HIP = HIP[:_reduce.start()] + HIP[_reduce.end():].replace("USER_REDUCE_LANES", _reduce.group(1).replace("\\\n", "\n"))


def text(name):
    """the C string constant `const char* name = "..." "...";` of smm_user_host.hpp"""
    m = re.search(r"const char\* %s =\s*((?:\s*\"(?:[^\"\\]|\\.)*\")+)\s*;" % name, HIP)
    return "".join(ast.literal_eval(s) for s in re.findall(r"\"(?:[^\"\\]|\\.)*\"", m.group(1)))


HEADS = ('#include "smmhip.h"\n#include "smm_rng.hpp"\nusing namespace smm;\n#include "smm_params.hpp"\n#include "smm_walk_lean.hpp"\n'
         '#include "smm_propose.hpp"\n#include "smm_chain.hpp"\n#include "smm_p2p.hpp"\n#include "smm_chain_norm.hpp"\n#include "smm_chain_persist.hpp"\n')
UNITS = {
    "per-iteration, one thread": (text("USER_RNG_API") + text("USER_PRELUDE_RNG") + AR1_RNG_SOURCE + text("USER_KERNEL_RNG"), 1),
    "per-iteration, map-reduce": (text("USER_RNG_API") + text("USER_PRELUDE_LANES_RNG") + PANEL_RNG_SOURCE + text("USER_KERNEL_LANES_RNG"), 3),
    "persistent gen_user": ("#include <type_traits>\n" + text("USER_RNG_API") + text("USER_PRELUDE_RNG") + "#define SMM_USER_RNG 1\n" + AR1_RNG_SOURCE +
                            "\n#define SMM_GEN_USER 1\n" + HEADS + '#include "smm_chain_persist_gen.hpp"\n', 1),
    "persistent tile_user": ("#include <type_traits>\n" + text("USER_RNG_API") + text("USER_PRELUDE_LANES_RNG") + "#define SMM_USER_RNG 1\n" +
                             PANEL_RNG_SOURCE + "\n#define SMM_TILE_USER 1\n" + HEADS + '#include "smm_chain_persist_loc.hpp"\n#include "smm_chain_persist_tile.hpp"\n', 3),
    # the same persistent kernels around the hand-rolled LCG sources, for comparison
    "persistent gen_user, LCG": ("#include <type_traits>\n#include <stdint.h>\n" + text("USER_PRELUDE") + AR1_SOURCE + "\n#define SMM_GEN_USER 1\n" + HEADS +
                                 '#include "smm_chain_persist_gen.hpp"\n', 1),
    "persistent tile_user, LCG": ("#include <type_traits>\n#include <stdint.h>\n" + text("USER_PRELUDE_LANES") + PANEL_SOURCE + "\n#define SMM_TILE_USER 1\n" +
                                  HEADS + '#include "smm_chain_persist_loc.hpp"\n#include "smm_chain_persist_tile.hpp"\n', 3),
}
d = tempfile.mkdtemp(prefix="smm_user_rng_res_")
for what, (tu, nsums) in UNITS.items():
    src = os.path.join(d, "tu.hip")
    with open(src, "w") as f:
        f.write(tu)
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-DSMM_NSUMS=%d" % nsums,
                        "-I", CSRC, "-I", os.path.join(ROOT, "include"), "--cuda-device-only", "-c", src, "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    if r.returncode != 0:
        print(what, "DOES NOT COMPILE\n", r.stderr[-3000:])
        sys.exit(1)
    cur, rows = None, {}
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = m.group(1); rows[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass", line)
        if m and cur:
            rows[cur][m.group(1)] = m.group(2)
    for n, row in rows.items():
        if "smm_user" in n and "kernel" in n:
            print("%-27s %-30s" % (what, n), " ".join("%s=%s" % (k.replace(" ", ""), v) for k, v in row.items() if k not in ("Dynamic Stack", "AGPRs")))
