"""The accept step's rule book (smm.jl_amd/csrc/smm_accept.hpp) on the CPU: the header is host + device code, so a small host program built
at test time calls every rule on cases read from stdin and prints the results as hex doubles.  The known answers are written out here from
the reference's lines (AlgoBGP.jl:324-392 doAcceptReject!, :253-257 set_acceptRate!, :381-390 the sigma update, :220-245 set_eval!,
:734-749 swap_ev_ij!; ObjExamples.jl:79-110 and :251-265) — not taken from a second implementation; the exponential is the contract's
(oracle.contract_math).  No GPU."""
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "smm.jl_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include "smm_rng.hpp"
using namespace smm;
#include "smm_accept.hpp"

static double num() { char s[128]; if (scanf("%127s", s) != 1) exit(2); return strtod(s, nullptr); }
static void out(double x) { printf(" %a", x); }

int main() {
    char op[32];
    while (scanf("%31s", op) == 1) {
        if (!strcmp(op, "decide")) {
            const bool first = num() != 0.0; const int status = (int)num();
            const double value = num(), old = num(), atun = num(), u = num();
            const AcceptDecision d = accept_decide(first, status, value, old, atun, u, smm_exp);
            out(d.prob); out(d.acc ? 1.0 : 0.0); out((double)d.status); out(d.negative ? 1.0 : 0.0);
        } else if (!strcmp(op, "rate")) {
            const int na = (int)num(), nn = (int)num(); const bool acc = num() != 0.0;
            out(accept_rate(na, nn, acc));
        } else if (!strcmp(op, "sigma")) {
            const double sig = num(), rate = num(), adj = num();
            out(sigma_next(sig, rate, adj));
        } else if (!strcmp(op, "best")) {
            const double value = num(); const int t = (int)num(); const double bp = num(), bpid = num();
            const Best b = best_of(value, t, bp, bpid);
            out(b.best); out(b.best_id);
        } else if (!strcmp(op, "swapped")) {
            const int partner = (int)num(), tp = (int)num(); const double bestp[2] = {num(), num()};
            double donor[3], h[H_PARAMS];
            for (double& x : donor) x = num();
            const Best b = swapped_head(h, donor, partner, tp, bestp);
            for (double x : h) out(x);
            out(b.best); out(b.best_id);
        } else if (!strcmp(op, "head")) {
            double a[8], h[H_PARAMS];
            for (double& x : a) x = num();
            history_head(h, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7]);
            out(h[H_VALUE]); out(h[H_PROB]); out(h[H_CURR]); out(h[H_BEST]); out(h[H_BESTID]); out(h[H_EXCH]); out(h[H_ACC]); out(h[H_STATUS]);
        } else if (!strcmp(op, "record")) {
            const bool acc = num() != 0.0; const double value = num(), prob = num(); const int status = (int)num();
            double in[3], o[3];
            for (double& x : in) x = num();
            record_head(o, in, acc, value, prob, status);
            for (double x : o) out(x);
        } else if (!strcmp(op, "msq")) {
            const double m = num(), mom = num(), w = num();
            out(moment_sq(m, mom, w));
        } else if (!strcmp(op, "sum") || !strcmp(op, "banana")) {
            const int n = (int)num();
            double v[64];
            for (int k = 0; k < n; ++k) v[k] = num();
            out(op[0] == 's' ? sum_in_order(v, n) : banana_value(v, n));
        } else if (!strcmp(op, "failbox")) {
            const double th = num(); const double box[2] = {num(), num()};
            out(in_failbox(th, box) ? 1.0 : 0.0);
        } else {
            return 3;
        }
        printf("\n");
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def rules():
    """ask(op, *numbers) -> the rule's results as a list of floats (one run of the host program per call: they are few)"""
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "accept_rules.hip"), os.path.join(tmp, "accept_rules")
        open(src, "w").write(PROGRAM)
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "--cuda-host-only", "-O2", "-ffp-contract=off",
                               "-fno-fast-math", "-std=c++17", "-I", CSRC, "-o", exe, src])

        def ask(op, *numbers):
            line = op + " " + " ".join(float(x).hex() for x in numbers) + "\n"
            res = subprocess.run([exe], input=line, capture_output=True, text=True, check=True).stdout.split()
            return [float.fromhex(x) for x in res]
        yield ask


def same(got, want):
    """bit for bit, NaN equal to NaN"""
    assert len(got) == len(want), (got, want)
    for g, w in zip(got, want):
        assert (math.isnan(g) and math.isnan(w)) or (g == w and math.copysign(1.0, g) == math.copysign(1.0, w)), (got, want)


def contract_exp(x):
    from oracle import oracle
    return float(oracle.contract_math("exp", np.array([x]))[0])


NAN, INF = float("nan"), float("inf")


def test_accept_decision(rules):
    # decide: first, status, value, old, atun, u -> prob, accepted, status, negative
    same(rules("decide", 1, -2, NAN, 5.0, 1.0, 0.9), [1.0, 1, 1, 0])          # :326-332: iteration 1, whatever the evaluation said
    same(rules("decide", 0, -2, -1.0, 2.0, 1.0, 0.0), [0.0, 0, -2, 0])        # :336-338: a failed evaluation keeps its status
    same(rules("decide", 0, 1, NAN, 2.0, 1.0, 0.5), [0.0, 0, -1, 1])          # :341 negative; exp(NaN) is NaN, :350-353
    same(rules("decide", 0, 1, -1.0, 2.0, 1.0, 0.5), [1.0, 1, 1, 1])          # :341 negative; exp(3) clipped to 1 > u
    same(rules("decide", 0, 3, 1.0, INF, 1.0, 0.5), [1.0, 1, 3, 0])           # :355-359: old not finite -> accepted, status unchanged
    same(rules("decide", 0, 3, 1.0, INF, 0.0, 0.5), [0.0, 0, -1, 0])          # 0 * inf = NaN -> :350-353
    same(rules("decide", 0, 1, 1.0, NAN, 1.0, 0.5), [0.0, 0, -1, 0])          # old NaN -> prob NaN -> :350-353
    same(rules("decide", 0, 2, 1.0, 2.0, 20.0, 0.999999), [1.0, 1, 1, 0])     # :344: exp(20) clipped to exactly 1.0
    same(rules("decide", 0, 2, 1.0, 2.0, 20.0, 1.0), [1.0, 0, 1, 0])          # ... which does not exceed u = 1 (strict >, :362-367)
    p = contract_exp(2.0 * (1.0 - 1.5))
    assert 0.36 < p < 0.37
    same(rules("decide", 0, 1, 1.5, 1.0, 2.0, p), [p, 0, 1, 0])               # prob == u: rejected
    same(rules("decide", 0, 1, 1.5, 1.0, 2.0, math.nextafter(p, 0.0)), [p, 1, 1, 0])   # prob one ulp above u: accepted


def test_accept_rate_sigma_and_best(rules):
    same(rules("rate", 0, 0, 1), [1.0])                                       # :253-257 with no iteration counted yet
    same(rules("rate", 0, 0, 0), [0.0])
    same(rules("rate", 2, 6, 1), [3.0 / 7.0])
    sig, adj = 0.159, 0.3
    assert sig * (1.0 + adj) != sig + sig * adj and sig * (1.0 - adj) != sig - sig * adj      # (another association: another last bit)
    same(rules("sigma", sig, 0.234, adj), [sig * (1.0 - adj)])                # :381-390: not > 0.234 -> down
    same(rules("sigma", sig, math.nextafter(0.234, 1.0), adj), [sig * (1.0 + adj)])
    same(rules("best", 2.0, 7, 2.0, 3.0), [2.0, 3.0])                         # :231-243: a tie keeps the older iteration
    same(rules("best", NAN, 7, 2.0, 3.0), [2.0, 3.0])
    same(rules("best", 1.5, 7, 2.0, 3.0), [1.5, 7.0])


def test_rows_and_records(rules):
    # swapped: partner, tp, bestp, bestp_id, donor {value, prob, status} -> value, prob, curr, best, best_id, exchanged, accepted, status; best, best_id
    same(rules("swapped", 9, 4, 0.75, 2.0, 0.5, 0.25, 1.0), [0.5, 0.25, 0.5, 0.5, 4.0, 9.0, 1.0, 1.0, 0.5, 4.0])       # :734-749
    same(rules("swapped", 9, 4, 0.75, 2.0, 0.9, 0.25, -1.0), [0.9, 0.25, 0.9, 0.75, 2.0, 9.0, 1.0, -1.0, 0.75, 2.0])
    same(rules("head", 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0), [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0])
    same(rules("record", 1, 0.5, 0.25, 1, 7.0, 8.0, -1.0), [0.5, 0.25, 1.0])                     # :209-215: accepted -> this iteration's
    same(rules("record", 0, 0.5, 0.25, 1, 7.0, 8.0, -1.0), [7.0, 8.0, -1.0])                      # rejected -> the one it continued from


def test_moments_and_objectives(rules):
    same(rules("msq", 1.5, 1.0, NAN), [0.25])                                 # ObjExamples.jl:79-100: no weight
    same(rules("msq", 1.5, 1.0, 0.0), [INF])
    same(rules("msq", 1.5, 1.0, 0.25), [4.0])
    same(rules("msq", NAN, 1.0, 2.0), [NAN])
    for n in (1, 7, 8, 9, 17):
        v = [1.0] + [1e-16] * (n - 1)
        want = v[0]
        for x in v[1:]:
            want = want + x
        assert want == 1.0 and (n == 1 or sum(reversed(v)) != want)             # (the small terms first: another last bit)
        same(rules("sum", n, *v), [want])
    rng = np.random.default_rng(5)
    for npar in (2, 10):
        th = rng.uniform(-2.0, 2.0, npar).tolist()
        want = None
        for i in range(npar - 1):                                             # ObjExamples.jl:251-265, the terms in order
            a, b = th[i], th[i + 1]
            t1, t2 = b - a * a, 1.0 - a
            term = 100.0 * (t1 * t1) + t2 * t2
            want = term if i == 0 else want + term
        same(rules("banana", npar, *th), [want])
    same(rules("failbox", -0.2, -0.2, 0.1), [1.0])                            # mprob.jl:183-186: the bounds belong to the box
    same(rules("failbox", 0.1, -0.2, 0.1), [1.0])
    same(rules("failbox", math.nextafter(0.1, 1.0), -0.2, 0.1), [0.0])
    same(rules("failbox", NAN, -0.2, 0.1), [0.0])
