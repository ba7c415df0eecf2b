"""where the plan kernels ran, from a rocprofv3 --kernel-trace of bench.py: python tools/plan_overlap.py DIR [ITERS_PER_STEP]
Reads every *kernel_trace.csv under DIR.  Prints the chain-kernel dispatches in order (duration, gap to the one before, microseconds of it
that a plan kernel ran beside), every plan dispatch (k_exch_plan: on the main stream; k_exch_plan_bg: beside) with the share of it that lay
inside chain-kernel dispatches, and the summary the overlap criterion asks for: does every k_exch_plan_bg dispatch begin and end inside the
span of chain dispatches, and the largest gap between consecutive chain dispatches."""
import csv, glob, sys

rows = []
for f in glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
rows.sort()
chain = [r for r in rows if "k_chain_persist" in r[2]]
plans = [r for r in rows if "k_exch_plan" in r[2]]


def overlap(a, b):
    return max(0, min(a[1], b[1]) - max(a[0], b[0]))


print("chain dispatches: %d, plan dispatches: %d (%d beside)" % (len(chain), len(plans), sum("plan_bg" in p[2] for p in plans)))
gaps = []
for i, c in enumerate(chain):
    gap = (c[0] - chain[i - 1][1]) / 1e3 if i else 0.0
    between = [p for p in plans if i and "plan_bg" not in p[2] and p[0] >= chain[i - 1][1] and p[1] <= c[0]]
    if i:
        gaps.append((gap, bool(between)))
    beside = sum(overlap(c, p) for p in plans if "plan_bg" in p[2]) / 1e3
    print("  chain %2d  dur %9.1f us  gap %7.1f us%s  plan beside for %7.1f us" % (i, (c[1] - c[0]) / 1e3, gap, " (k_exch_plan in it)" if between else "", beside))
ok = True
for p in plans:
    inside = sum(overlap(p, c) for c in chain)
    dur = p[1] - p[0]
    bg = "plan_bg" in p[2]
    within = bool(chain) and p[0] >= chain[0][0] and p[1] <= chain[-1][1]
    print("  %-14s dur %7.1f us  inside chain dispatches %5.1f %%%s" % ("k_exch_plan_bg" if bg else "k_exch_plan", dur / 1e3, 100.0 * inside / max(dur, 1),
                                                                       "" if not bg else ("  within the chain span" if within else "  OUTSIDE the chain span")))
    ok = ok and (not bg or within)
plain = [g for g, pl in gaps if not pl]
print("every k_exch_plan_bg dispatch within the span of chain dispatches: %s" % ok)
print("largest gap between consecutive chain dispatches: %.1f us (without a plan kernel in it: %.1f us)" % (max([g for g, _ in gaps], default=0.0), max(plain, default=0.0)))
print("chain total %.1f us, k_exch_plan total %.1f us, k_exch_plan_bg total %.1f us" % (sum(c[1] - c[0] for c in chain) / 1e3, sum(p[1] - p[0] for p in plans if "plan_bg" not in p[2]) / 1e3,
                                                                                   sum(p[1] - p[0] for p in plans if "plan_bg" in p[2]) / 1e3))
