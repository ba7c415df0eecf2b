"""The plain reference for the simulation of objfunc_norm (simM[k] = mean over s of z[k,s] + theta[k], ObjExamples.jl:76-79) and the sample
counts at which the six hand-written forms of it cut `ns` into pieces (tests/test_sample_counts.py, tests/test_gpu_sample_counts.py).

Everything else in the suite compares the device with the C oracle, whose sum has the device's 512-lane shape by contract: a draw that both
lose or both read twice at an edge would pass.  Nothing in here knows that shape — `exact_mean` is an exactly rounded sum and one division,
`coded_mean` an integer sum — except `mean_bound`, which only uses the LENGTH of the contract's longest chain of additions."""
import math
import os
import re

import numpy as np

# the four numbers the forms cut `ns` by (tests/test_sample_counts.py reads them out of the headers and fails if they moved)
WG = 512        # lanes that own a tile; a lane sums the draws l, l + 512, ...       (include/smmhip.h: SMM_REDUCE_LANES, smm_params.hpp: WG)
ZU = 8          # shock rows per chunk of simulate_tile_v: chunks of ZU * WG draws   (smm_chain.hpp)
NORM_ZU = 4     # shock rows per chunk of simulate_tile16: chunks of NORM_ZU * WG    (smm_chain_norm.hpp)
PR_ZR = 20      # draws per lane the persistent `loc` forms hold in registers: ns <= WG * PR_ZR, FULL at ns / WG == PR_ZR - 1 (smm_chain_persist.hpp)

CHUNKS = (NORM_ZU * WG, ZU * WG)
LOC_MAX = PR_ZR * WG            # the last ns the `loc` forms take
PAST_EVERY_LIMIT = 20000


def _edges():
    e = [1, 2, 63, 64, 65, WG - 1, WG, WG + 1]                        # fewer draws than a wave has lanes, than a tile has lanes
    for C in CHUNKS:                                                  # one chunk, two (the even path), three (the odd path), each full and ragged
        e += [C - 1, C, C + 1, 2 * C - 1, 2 * C, 2 * C + 1, 3 * C, 3 * C + 1]
    e += [(PR_ZR - 1) * WG - 1, (PR_ZR - 1) * WG, (PR_ZR - 1) * WG + 1,   # FULL switches on
          PR_ZR * WG - 1, PR_ZR * WG, PR_ZR * WG + 1]                     # FULL switches off; the last count of the form; the first one refused
    e.append(PAST_EVERY_LIMIT)
    return tuple(sorted(set(e)))


EDGES = _edges()
NORM_CHUNK_EDGES = tuple(n for n in EDGES if any(abs(n - m * CHUNKS[0]) <= 1 for m in (1, 2, 3)))   # the 2048-chunk edges


def header_constants(root):
    """WG, ZU, NORM_ZU, PR_ZR as the headers' text defines them"""
    def grab(path, pattern):
        m = re.search(pattern, open(os.path.join(root, path)).read(), re.M)
        assert m, "%s: no match for %r" % (path, pattern)
        return m.group(1)
    csrc = os.path.join("smm.jl_amd", "csrc")
    assert grab(os.path.join(csrc, "smm_params.hpp"), r"^constexpr int WG = (\w+);") == "SMM_REDUCE_LANES"
    return dict(WG=int(grab(os.path.join("include", "smmhip.h"), r"^#define SMM_REDUCE_LANES (\d+)")),
                ZU=int(grab(os.path.join(csrc, "smm_chain.hpp"), r"^constexpr int ZU = (\d+);")),
                NORM_ZU=int(grab(os.path.join(csrc, "smm_chain_norm.hpp"), r"^constexpr int NORM_ZU = (\d+);")),
                PR_ZR=int(grab(os.path.join(csrc, "smm_chain_persist.hpp"), r"^constexpr int PR_ZR = (\d+);")))


# ---- the plain reference ----
U = 2.0 ** -53      # unit roundoff of binary64


def _exact_and_bound(Zk, theta):
    xs = (np.asarray(Zk, np.float64) + float(theta)).tolist()      # one rounding each, as the contract words it
    ns = len(xs)
    exact = math.fsum(xs) / ns
    return exact, (math.ceil(ns / WG) + 9) * U * math.fsum(map(abs, xs)) / ns + U * abs(exact)


def exact_mean(Zk, theta):
    """mean of fl(Zk[s] + theta): the exactly rounded sum (math.fsum), one division"""
    return _exact_and_bound(Zk, theta)[0]


def mean_bound(Zk, theta, ns):
    """What any summation order of the contract's shape may differ from exact_mean by.  Derived, not measured: the longest chain of
    additions is a lane's ceil(ns / 512) draws plus the 9 levels over 512 partials, each addition errs by at most 2^-53 of a partial sum
    that is at most sum|x|; then the half ulp of the division:
        |simM - exact| <= (ceil(ns / 512) + 9) * 2^-53 * sum|x| / ns + 2^-53 * |exact|
    (9 = log2(512) is the depth of a halving tree over the partials.  The contract's own combination — six halving levels inside each
    group of 64, then the 8 group totals left to right — has 13 additions on its longest path; the bound keeps the smaller figure, which
    is the stricter one.  The oracle's largest error over all of EDGES is a third of it, a single dropped draw more than 1e3 times it.)"""
    assert len(Zk) == ns
    return _exact_and_bound(Zk, theta)[1]


def mean_check(Z, params, sim_moments):
    """Every simulated moment of a history (params [T][nm][N], sim_moments [T][nm][N]; or of a batch: [nm][M] both) against exact_mean.
    Returns (largest error / bound, its index); no row is left out."""
    Z = np.asarray(Z, np.float64)
    p = np.asarray(params, np.float64); m = np.asarray(sim_moments, np.float64)
    if p.ndim == 2:
        p, m = p[None], m[None]
    assert p.shape == m.shape and p.shape[1] == Z.shape[0], (p.shape, m.shape, Z.shape)
    worst, where = 0.0, None
    for k in range(Z.shape[0]):
        zk = Z[k]
        for t in range(p.shape[0]):
            for c in range(p.shape[2]):
                exact, bound = _exact_and_bound(zk, p[t, k, c])
                err = abs(m[t, k, c] - exact)
                r = err / bound if bound > 0.0 else (0.0 if err == 0.0 else math.inf)
                if not r <= worst:      # (a NaN moment is the worst there is)
                    worst, where = (r if r == r else math.inf), (t, k, c)
    return worst, where


# ---- sums that are exact in any order ----
CODE_SCALE = 2.0 ** -12


def codes(nm, ns):
    """1 + (s * 40503 + k * 9973) mod 65536: a value per position (k, s); a lost, doubled or misplaced draw changes the integer sum"""
    k = np.arange(nm, dtype=np.int64)[:, None]; s = np.arange(ns, dtype=np.int64)[None, :]
    return 1 + (s * 40503 + k * 9973) % 65536


def coded_Z(nm, ns):
    """shocks that are integer multiples of 2^-12, at most 16"""
    return codes(nm, ns) * CODE_SCALE


def dyadic_thetas(lb, ub, M, seed=5):
    """[np][M] parameters, multiples of 2^-8 inside [lb, ub]"""
    rng = np.random.default_rng(seed)
    lo = np.ceil(np.asarray(lb, float) * 256).astype(np.int64); hi = np.floor(np.asarray(ub, float) * 256).astype(np.int64)
    return rng.integers(lo[:, None], hi[:, None] + 1, size=(len(lo), M)) / 256.0


def coded_mean(nm, ns, thetas):
    """simM [nm][M] of coded_Z at dyadic thetas: every partial sum of z + theta is an integer multiple of 2^-12 below 2^53, so the sum is
    the integer's float in any order, and one division follows"""
    ti = np.asarray(thetas, float) * 4096
    assert np.all(ti == np.round(ti)), "thetas must be multiples of 2^-12"
    csum = codes(nm, ns).sum(axis=1)
    out = np.empty((nm, ti.shape[1]))
    for k in range(nm):
        for c in range(ti.shape[1]):
            isum = int(csum[k]) + ns * int(ti[k, c])
            assert abs(isum) < 2 ** 53 and (int(csum[k]) + ns * abs(int(ti[k, c]))) < 2 ** 53
            out[k, c] = float(isum) * CODE_SCALE / ns
    return out


def value_from_moments(simM, mom, w):
    """The objective from the moments in the header's order of operations (include/smmhip.h, objfunc_norm): d = simM - mom, divided by the
    weight unless that is NaN, squared, added left to right, divided by nm.  simM [..., nm, N] -> [..., N]"""
    simM = np.asarray(simM, np.float64)
    nm = simM.shape[-2]
    vsum = None
    for k in range(nm):
        d = simM[..., k, :] - mom[k]
        if not math.isnan(w[k]):
            d = d / w[k]
        v = d * d
        vsum = v if vsum is None else vsum + v
    return vsum / float(nm)
