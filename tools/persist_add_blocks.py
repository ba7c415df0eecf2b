"""the add blocks of k_chain_persist_loc in the compiler's assembly: python tools/persist_add_blocks.py [src_dir | file.s]   (cross-compiles for gfx950, no GPU needed)
For every instantiation: per block between the s_setprio that raises the adds and the one that lowers them again — instructions, v_add_f64,
accesses to scratch (spills and reloads) inside the block — and every scratch access of the kernel with where it stands: the s_setprio
before it (its ordinal in the kernel's text and its value), the barriers between that s_setprio and the access, and whether a return
(s_endpgm) follows it before the next s_setprio.  In the kernel's text the workers' add block comes first, the control wave's second: an
access behind the FIRST lowering s_setprio and ahead of the second raising one stands in the workers' side job or, behind that job's
last barrier, in their once-per-launch epilogue; the control wave's path from BA to BB and on to the publication is what follows the workers' s_endpgm."""
import os, re, subprocess, sys, tempfile

src = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "smm.jl_amd", "csrc")
if src.endswith(".s"):   # (an assembly file made earlier)
    text = open(src).read()
else:
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # (smmhip.hip includes the device headers as text: the Makefile generates that file, and states the flags)
    subprocess.check_call(["make", "-s", "-C", src, "smm_embedded.inc"])
    flags = re.search(r"^HIPFLAGS = (.*)$", open(os.path.join(src, "Makefile")).read(), flags=re.M).group(1).split()
    flags = [f for f in flags if not f.startswith("-Wl,")]
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "dev.s")
        r = subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", "smmhip.hip", "-o", out], cwd=src, capture_output=True, text=True)
        if r.returncode:
            sys.exit("%s failed:\n%s" % (hipcc, r.stderr[-4000:]))
        text = open(out).read()
for m in re.finditer(r"^(_ZN\S*k_chain_persist_loc\S*):[^\n]*\n(.*?)^\.Lfunc_end", text, flags=re.S | re.M):
    name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
    name = re.search(r"k_chain_persist_loc<[^>]*>", name).group(0)
    body = m.group(2)
    ins = [l.split(";")[0].strip() for l in body.splitlines() if re.match(r"^\s+[a-z_]+[0-9a-z_]*(\s|$)", l) and not l.strip().startswith(".")]
    prios = [(i, int(l.split()[1])) for i, l in enumerate(ins) if l.startswith("s_setprio")]
    top = max(p for _, p in prios)
    blocks, start = [], None
    for i, p in prios:
        if p == top and start is None:
            start = i
        elif p < top and start is not None:
            blocks.append((start, i)); start = None
    scratch = [i for i, l in enumerate(ins) if l.startswith("scratch_")]
    print("%-46s priorities %s  scratch accesses %d (stores %d, loads %d)" % (name, sorted(set(p for _, p in prios)), len(scratch), sum(ins[i].startswith("scratch_store") for i in scratch),
                                                                            sum(ins[i].startswith("scratch_load") for i in scratch)))
    for a, b in blocks:
        blk = ins[a:b]
        print("    add block: %5d instructions, %5d v_add_f64, %d scratch accesses inside" % (len(blk), sum(l.startswith("v_add_f64") for l in blk), sum(a < s < b for s in scratch)))
    for s in scratch:
        before = [(k, i, p) for k, (i, p) in enumerate(prios) if i < s]
        after = [i for i, _ in prios if i > s]
        k, i0, p = before[-1] if before else (-1, 0, -1)
        nxt = after[0] if after else len(ins)
        where = "ahead of the first s_setprio" if k < 0 else "behind s_setprio #%d (%d)" % (k, p)
        print("    %-13s at %6d: %s, %d barrier(s) between, s_endpgm before the next s_setprio: %s" % (
            ins[s].split()[0][:13], s, where, sum(l.startswith("s_barrier") for l in ins[i0:s]), "yes" if any(l.startswith("s_endpgm") for l in ins[s:nxt]) else "no"))
