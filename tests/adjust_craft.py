"""Crafted histories for smm_get_adjustment's edges (include/smmhip.h, smm.jl_amd/csrc/smm_adjust.hpp): each builder is a function of its
arguments and a seed, writes params, sim_moments, value and accepted into a HistoryBuffers (`into`, as moment_stats_ref.crafted_linear
does) and returns what its construction implies, so that an expected value comes neither from adjust_ref.py nor from the device.

  crafted_exact : an exact design for the bound counts.  The discrepancies are Walsh rows, the parameters dyadic combinations of Walsh
                  rows: beta comes out bit for bit and every adjusted draw takes one of four known values, m / 4 rows each, placed below,
                  on, inside and above [lb, ub].
  crafted_keys  : a design for the weighted select and the bandwidth.  Under Epanechnikov's kernel and a ridge of 1e300 every kept
                  adjusted draw is its parameter bit for bit, so the builder chooses the keys (both signs, signed zeros, subnormals,
                  pairs that part at each digit of the radix select), the integer weights (1, 2^20, unequal ones inside one key) and the
                  distance the bandwidth lands on.
  crafted_seams : moment_stats_ref.crafted_linear with an `accepted` column that gives every chain a chosen number of rows.

tests/test_adjustment_edges.py holds every property of the designs against adjust_ref.py without a GPU; tests/test_gpu_adjustment_edges.py
holds the device against both."""
import numpy as np

import adjust_ref as AR
import moment_stats_ref as MR

LDS_N = 8192                     # smm_stats.hpp: STATS_LDS_N, the rows of a chunk
ADJ_WG = 256                     # smm_adjust.hpp: the lanes of a row pass
BATCH_CAP = 256 << 20            # smm_reducers_host.hpp: REDUCER_BATCH_CAP
DIGITS = ((53, 11), (42, 11), (31, 11), (20, 11), (9, 11), (0, 9))   # smm_group.hpp: group_digit's (shift, width) of the six digits


def adjust_plan(N, Tcap, npar, nm, Mtot, NC, cap=0):
    """(Nbc, jb): smm_get_adjustment's batch plan (smm_reducers_host.hpp) of a context of N chains and a capacity of Tcap iterations
    whose only reducer calls are smm_get_adjustment's: the chunks and the adjusted parameters taken at a time; cap: the seam
    SMMHIP_STATS_SCRATCH, 0 for the shipped plan"""
    D = npar + nm
    chunk8, col8 = (D + 2) * LDS_N * 8, Mtot * 8
    rcap = cap or BATCH_CAP
    scr = max(min(N * Tcap * (8 * npar + 4), max(rcap, 12 * Tcap)), 2 * N * Tcap * 8 + chunk8)
    budget = min(scr, max(cap, 2 * col8 + chunk8)) if cap else scr
    avail = budget - 2 * col8
    Nbc = max(1, min(NC, avail // 2 // chunk8, rcap // (D * D * 8)))
    return Nbc, min(npar, 1 + (avail - Nbc * chunk8) // col8)


def chunk_starts(counts):
    """gch0 [G + 1] of smm_reducers_host.hpp's pool_plan: a group's pooled rows are cut into chunks of 8192 from its own first row"""
    return np.concatenate([[0], np.cumsum([-(-int(m) // LDS_N) for m in counts])]).astype(int)


def zero_history(T, N, npar, nm):
    from smm_jl_amd import _abi as A
    h = A.HistoryBuffers(T, N, npar, nm)
    for f in A.HistoryBuffers.FIELDS:
        getattr(h, f)[...] = 0
    return h


def write(into, theta, mom, accepted):
    """the four crafted fields from theta [T][np][N], mom [T][nm][N], accepted [T][N]; value as crafted_linear's"""
    assert into.params.shape == theta.shape and into.sim_moments.shape == mom.shape
    into.params[...], into.sim_moments[...], into.accepted[...] = theta, mom, accepted
    into.value[...] = 0.5 * (mom * mom).sum(axis=1)
    return into


# --- crafted_exact -----------------------------------------------------------------------------------------------------------------

EXACT_NP, EXACT_NM = 3, 4
EXACT_MOM = np.array([0.5, -0.25, 1.0, -2.0])            # the data moments, the scales (the problem's weights) and the bounds: dyadic,
EXACT_W = np.array([1.0, 2.0, 0.5, 4.0])                 # and no two parameters share a bound
EXACT_LB = np.array([-1.0, -0.5, -2.0])
EXACT_UB = np.array([1.0, 0.75, 1.5])
EXACT_X_ROWS = (21, 127, 1929, 3072)                     # the Walsh rows of the four discrepancy columns
# per parameter the two Walsh rows of its noise: bit 6 or 7 of the first makes whole waves of 64 rows differ, bit 8 or above of the
# second whole workgroups of 256
EXACT_N_ROWS = ((64 + 3, 256 + 5), (128, 512 + 1), (1024 + 64, 6))
# per group and parameter (c, a, b): theta* takes the values c - a - b, c - a + b, c + a - b, c + a + b
EXACT_CAB = (((-1.0, 0.5, 0.25), (0.25, 0.5, 0.25), (0.125, 2.25, 0.125)),
             ((0.0, 0.75, 0.25), (0.125, 0.75, 0.125), (0.0, 1.0, 0.75)))
EXACT_CLASS = (("below", "above", "both"), ("none", "both", "above"))   # where each (group, parameter) loses rows
EXACT_PROBS = (0.0, 0.25, 0.5, 0.6, 1.0)                 # the quantiles of four equally weighted values: values 0, 0, 1, 2, 3
EXACT_PROB_VALUE = (0, 0, 1, 2, 3)


def exact_problem(N, T, seed=3):
    """moment_stats_ref.dense_problem(3, 4) with dyadic data moments, weights and bounds (the starting point lies inside them)"""
    prob, opts = MR.dense_problem(EXACT_NP, EXACT_NM, N=N, T=T, seed=seed)
    prob.mom[...], prob.w[...], prob.lb[...], prob.ub[...] = EXACT_MOM, EXACT_W, EXACT_LB, EXACT_UB
    assert (prob.init > prob.lb).all() and (prob.init < prob.ub).all()
    return prob, opts


def walsh(r, m):
    """row r of the Sylvester-Hadamard matrix of order m: (-1)^popcount(r & i)"""
    i = np.arange(m, dtype=np.int64) & r
    par = np.zeros(m, np.int64)
    while i.any():
        par ^= i & 1
        i >>= 1
    return 1.0 - 2.0 * par


def crafted_exact(N, T, seed, into=None):
    """(h, info): two groups, the first and the second half of the N chains, m = N T / 2 pooled rows each (a power of 4: 4096 or 16384),
    every row selected and accepted.  For the uniform kernel at tol = 1 with the problem of exact_problem: the discrepancy columns are
    distinct Walsh rows (mean 0, mutually orthogonal: C_xx = m I, whose factor sqrt(m) is exact), theta_j = c_j + n_j + sum_k beta_kj x_k
    with a dyadic beta drawn from the seed and n_j = a_j W_p + b_j W_q from Walsh rows no x uses, so every sum is exact in any order, beta
    is reproduced bit for bit and theta*_j = c_j + n_j takes four values, m / 4 rows each.  info: groups [N], beta [2][nm][np], values
    [2][np][4] ascending, n_outside [2][np] counted from the values against the bounds, adj_mean [2][np] (c_j), quantile
    [len(EXACT_PROBS)][2][np], outside_rows [g][j] (the pooled row indices that leave the bounds)"""
    m = N * T // 2
    assert N % 2 == 0 and m in (4096, 16384) and N * T == 2 * m
    into = zero_history(T, N, EXACT_NP, EXACT_NM) if into is None else into
    rng = np.random.default_rng([seed, N, T])
    used = set(EXACT_X_ROWS) | {r for pq in EXACT_N_ROWS for r in pq}
    assert 0 not in used and len(used) == EXACT_NM + 2 * EXACT_NP and max(used) < 4096
    beta = rng.integers(-16, 17, (2, EXACT_NM, EXACT_NP)) / 8.0
    theta, mom = np.empty((T, EXACT_NP, N)), np.empty((T, EXACT_NM, N))
    values, n_out = np.empty((2, EXACT_NP, 4)), np.zeros((2, EXACT_NP), np.int64)
    cs, rows = np.empty((2, EXACT_NP)), [[None] * EXACT_NP for _ in range(2)]
    for g in range(2):
        x = np.stack([walsh(r, m) for r in EXACT_X_ROWS])                          # [nm][m]
        s = EXACT_MOM[:, None] + EXACT_W[:, None] * x
        th = np.empty((EXACT_NP, m))
        for j in range(EXACT_NP):
            c, a, b = EXACT_CAB[g][j]
            n = a * walsh(EXACT_N_ROWS[j][0], m) + b * walsh(EXACT_N_ROWS[j][1], m)
            star = c + n
            th[j] = star + beta[g, :, j] @ x
            values[g, j] = [c - a - b, c - a + b, c + a - b, c + a + b]
            out = (values[g, j] < EXACT_LB[j]) | (values[g, j] > EXACT_UB[j])
            n_out[g, j] = out.sum() * (m // 4)
            rows[g][j] = np.flatnonzero((star < EXACT_LB[j]) | (star > EXACT_UB[j]))
            cs[g, j] = c
        members = np.arange(N // 2) + g * (N // 2)                                 # pooled row i: member i // T at iteration i % T
        theta[:, :, members] = th.reshape(EXACT_NP, N // 2, T).transpose(2, 0, 1)
        mom[:, :, members] = s.reshape(EXACT_NM, N // 2, T).transpose(2, 0, 1)
    write(into, theta, mom, 1)
    quant = np.stack([values[:, :, v] for v in EXACT_PROB_VALUE])
    return into, dict(groups=(np.arange(N) // (N // 2)).astype(np.int32), m=m, beta=beta, values=values, n_outside=n_out, adj_mean=cs,
                      quantile=quant, outside_rows=rows)


# --- crafted_keys ------------------------------------------------------------------------------------------------------------------

KEYS_T = 200                     # rows of a chain: KEYS_KEPT below the bandwidth, KEYS_RUN on it, the rest beyond
KEYS_KEPT, KEYS_RUN = 100, 12
KEYS_TOL = 0.525                 # (c T - 1) tol lies in [100 c, 112 c - 2] for every count c of pooled chains: delta2 is the run's distance
KEYS_DELTA2 = 1.0
KEYS_TOL_ZERO = 0.02             # (c T - 1) tol lies below 6 c - 1: both rows the bandwidth is read from lie on the data, delta2 = 0.0
KEYS_RIDGE = 1e300
KEYS_MOM = (-1.0, 10.0)          # serial_normal's data moments, unit weights, bounds [-3, 3] x [-20, 20]
KEYS_LB, KEYS_UB = np.array([-3.0, -20.0]), np.array([3.0, 20.0])
KEYS_TIE = 0.75                  # the value of the tie run
KEYS_TIE_X = ((1, 0), (0, 2), (2, 1), (-2, 2), (3, 0), (-1, 3), (3, 2), (0, -1), (1, 0))   # in quarters: its members' discrepancies
Q_ONE = 1 << 20


def bits(v):
    return np.asarray(v, np.float64).view(np.int64)


def from_bits(b):
    return np.asarray(b, np.int64).view(np.float64)


def order_key(v):
    """smm_stats.hpp's stats_key as a Python int: the IEEE total order, -0 before +0"""
    b = int(bits(v)) & 0xFFFFFFFFFFFFFFFF
    return b ^ 0xFFFFFFFFFFFFFFFF if b >> 63 else b | (1 << 63)


def first_digit_apart(a, b):
    """the first digit of the radix select in which the keys of a and b differ (None: the same key)"""
    ka, kb = order_key(a), order_key(b)
    for d, (shift, width) in enumerate(DIGITS):
        if (ka >> shift) & ((1 << width) - 1) != (kb >> shift) & ((1 << width) - 1):
            return d
    return None


TWO = int(bits(2.0))
# seven values whose neighbours part at digit 0 (the sign), 5, 4, 3, 2 and 1 of the radix select
KEYS_LADDER = np.concatenate([[-2.0], from_bits([TWO, TWO + 1, TWO + (1 << 12), TWO + (1 << 25), TWO + (1 << 35)]), [3.0]])
# values between the ladder's, for rows that are not kept: a select that counted them would move
KEYS_DECOYS = np.concatenate([from_bits([TWO + 2, TWO + (1 << 11), TWO + (1 << 20), TWO + (1 << 30), TWO + (1 << 40)]),
                              [KEYS_TIE, 0.0, -0.0, 1e308, -1e308, 2.5, -2.5]])
# the rows on the data (x = 0: their adjusted value is the parameter itself, whatever beta): signed zeros, subnormals, tiny numbers
KEYS_ON_DATA = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-305, -1e-302])


def keys_chain(rng):
    """one chain's KEYS_T rows (theta0 [T], x [T][2] in quarters but for the q = 1 row): the kept rows first, then the run, then the rest;
    the caller shuffles"""
    th, x = [], []
    for v in KEYS_ON_DATA:
        th.append(v); x.append((0.0, 0.0))
    th.append(1.5); x.append((1.0 - 2.0 ** -31, 0.0))                              # d2 = 1 - 2^-30: w = 2^-30, q = 1
    for xx in KEYS_TIE_X:
        th.append(KEYS_TIE); x.append((xx[0] / 4, xx[1] / 4))
    inner = [(a / 4, b / 4) for a in range(-3, 4) for b in range(-3, 4) if 0 < a * a + b * b < 16]
    for v in KEYS_LADDER:
        th.append(v); x.append(inner[rng.integers(len(inner))])
    th.append(-4.0); x.append((0.5, -0.5))                                         # below lb_0, and above ub_0 once negated
    while len(th) < KEYS_KEPT:
        th.append(rng.uniform(-1.9, 1.9)); x.append(inner[rng.integers(len(inner))])
    on = [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)]
    for i in range(KEYS_RUN):                                                      # the run at the bandwidth: d2 = 1 exactly
        th.append(KEYS_DECOYS[i % 8]); x.append(on[i % 4])
    outer = [(a / 4, b / 4) for a in range(-8, 9) for b in range(-8, 9) if a * a + b * b > 16]
    while len(th) < KEYS_T:
        th.append(KEYS_DECOYS[rng.integers(len(KEYS_DECOYS))]); x.append(outer[rng.integers(len(outer))])
    return np.array(th), np.array(x)


def crafted_keys(N, seed, into=None):
    """(h, info): N chains of KEYS_T rows, every row selected and accepted, for serial_normal's problem (np = nm = 2, unit scales).  Each
    chain holds the whole design in an order of its own: KEYS_KEPT rows of squared distance below 1, KEYS_RUN rows at exactly 1, the rest
    beyond, so that the bandwidth of any pool of whole chains at tol = KEYS_TOL is 1.0.  theta_1 = -theta_0.  Under Epanechnikov's
    kernel with ridge = KEYS_RIDGE beta is ~1e-301, so a kept row's theta* is its theta bit for bit: the rows whose theta is a zero, a
    subnormal or tiny lie on the data (x = 0), every other kept theta is a normal number of ordinary size.  At tol = KEYS_TOL_ZERO the
    bandwidth is the distance 0.0 of the rows on the data: Epanechnikov's kernel keeps none (status 3, sum_w 0.0), the uniform kernel
    keeps them, whose discrepancies are all zero (status 4).  info: theta [N][T][2], d2 [N][T], q
    [N][T] (Epanechnikov's integer weights, 0 for a row not kept), all in iteration order"""
    into = zero_history(KEYS_T, N, 2, 2) if into is None else into
    rng = np.random.default_rng([seed, N])
    theta, mom = np.empty((KEYS_T, 2, N)), np.empty((KEYS_T, 2, N))
    th_all, d2_all, q_all = np.empty((N, KEYS_T, 2)), np.empty((N, KEYS_T)), np.empty((N, KEYS_T), np.int64)
    for c in range(N):
        th, x = keys_chain(rng)
        p = rng.permutation(KEYS_T)
        th, x = th[p], x[p]
        theta[:, 0, c], theta[:, 1, c] = th, -th
        mom[:, 0, c], mom[:, 1, c] = KEYS_MOM[0] + x[:, 0], KEYS_MOM[1] + x[:, 1]
        xb = np.stack([mom[:, 0, c] - KEYS_MOM[0], mom[:, 1, c] - KEYS_MOM[1]], axis=1)
        assert np.array_equal(xb, x)                                               # (the discrepancy comes back exactly)
        d2 = x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]
        w = np.where(d2 < KEYS_DELTA2, 1.0 - d2 / KEYS_DELTA2, 0.0)
        th_all[c, :, 0], th_all[c, :, 1], d2_all[c], q_all[c] = th, -th, d2, np.ceil(w * Q_ONE).astype(np.int64)
    write(into, theta, mom, 1)
    return into, dict(theta=th_all, d2=d2_all, q=q_all)


def weighted_quantile_loop(v, q, p):
    """adjust_ref.weighted_quantile stated a second time: a Python loop over the kept rows in the IEEE total order (Python ints)"""
    rows = sorted((order_key(a), int(b)) for a, b in zip(v, q) if b > 0)
    Q = sum(b for _, b in rows)
    target = max(1, int(np.ceil(np.float64(p) * np.float64(Q))))
    cum = 0
    for k, b in rows:
        cum += b
        if cum >= target:
            u = k ^ (1 << 63) if k >> 63 else k ^ 0xFFFFFFFFFFFFFFFF
            return from_bits(np.array(u, np.uint64).astype(np.int64))[()]
    raise AssertionError("no row reaches the target")


def keys_levels(v, q):
    """the kept values of one column in the IEEE total order: [(value, cumulative weight before it, through it, the weights at it)]"""
    rows = sorted((order_key(a), i) for i, (a, b) in enumerate(zip(v, q)) if b > 0)
    out, cum = [], 0
    for k, i in rows:
        if out and order_key(out[-1][0]) == k:
            out[-1][3].append(int(q[i]))
        else:
            out.append([v[i], cum, cum, [int(q[i])]])
        cum += int(q[i])
        out[-1][2] = cum
    return out


def keys_probs(info, members):
    """(probs, want, marks) for the pool of the chains `members` under Epanechnikov's kernel: 0 and 1; per column a prob whose target
    lies strictly inside the tie run, one whose ceil(p Q) is the cumulative weight through the run and one a unit of weight past it; and
    per column and ladder value (and for -0.0 and +0.0) the prob whose target is the first unit of weight of that value, so that the
    answer and the kept key before it part at each digit in turn.  want [len(probs)][2]: the quantiles by the construction
    (weighted_quantile_loop over theta and q); marks: {name: index into probs} per column"""
    th = info["theta"][members].reshape(-1, 2)
    q = info["q"][members].reshape(-1)
    Q = int(q.sum())
    probs, marks = [0.0, 1.0], [{}, {}]

    def add(j, name, target):
        p = (target - 0.5) / Q
        assert int(np.ceil(np.float64(p) * np.float64(Q))) == target
        marks[j][name] = len(probs)
        probs.append(p)
    for j in range(2):
        lv = keys_levels(th[:, j], q)
        tie = next(l for l in lv if l[0] == (KEYS_TIE if j == 0 else -KEYS_TIE))
        add(j, "inside", (tie[1] + tie[2]) // 2)
        add(j, "end", tie[2])
        add(j, "past", tie[2] + 1)
        for name, v in [("ladder%d" % i, (v if j == 0 else -v)) for i, v in enumerate(KEYS_LADDER)] + [("-0", -0.0), ("+0", 0.0)]:
            l = next(l for l in lv if order_key(l[0]) == order_key(v))
            if l[1] > 0:                                                           # (the smallest kept value has no key before it)
                add(j, name, l[1] + 1)
    want = np.array([[weighted_quantile_loop(th[:, j], q, p) for j in range(2)] for p in probs])
    return tuple(probs), want, marks


def keys_expect(info, members):
    """what the construction implies for the pool of the chains `members`: n_kept under the two kernels, the bandwidth, n_outside [2]
    under Epanechnikov's kernel"""
    c = len(members)
    th = info["theta"][members].reshape(-1, 2)
    kept = info["q"][members].reshape(-1) > 0
    n_out = [int((kept & ((th[:, j] < KEYS_LB[j]) | (th[:, j] > KEYS_UB[j]))).sum()) for j in range(2)]
    return dict(n_kept={0: c * (KEYS_KEPT + KEYS_RUN), 1: c * KEYS_KEPT}, bandwidth=KEYS_DELTA2, n_outside=np.array(n_out, np.int64))


# --- crafted_seams -----------------------------------------------------------------------------------------------------------------

SEAM_N, SEAM_T = 64, 700
# the accepted rows of the five groups: three chunks, two chunks, one chunk and one row, no member, exactly one workgroup of rows
SEAM_ROWS = (2 * LDS_N + 3000, LDS_N + 5000, LDS_N + 1, 0, ADJ_WG)
SEAM_CHAINS = (28, 19, 12, 0, 1)                         # their member chains; the last four chains are in no group


def crafted_seams(seed, into=None):
    """(h, groups, counts): moment_stats_ref.crafted_linear(2, 2, SEAM_N, SEAM_T) with an accepted column whose chains have chosen
    numbers of accepted rows (row 0 among them: the state series exists from the first row), so that with select = 1 the groups pool
    exactly SEAM_ROWS rows; counts [N] the accepted rows per chain"""
    into = MR.crafted_linear(2, 2, SEAM_N, SEAM_T, seed, into=into)[0]
    rng = np.random.default_rng([seed, 77])
    groups, counts = np.full(SEAM_N, -1, np.int32), np.zeros(SEAM_N, np.int64)
    c0 = 0
    for g, (rows, nc) in enumerate(zip(SEAM_ROWS, SEAM_CHAINS)):
        if nc == 0:
            continue
        groups[c0:c0 + nc] = g
        short = nc * SEAM_T - rows                                                 # spread over the members: odd lengths
        assert 0 <= short <= nc * (SEAM_T - 1)
        cut = rng.multinomial(short, np.full(nc, 1.0 / nc)) if nc > 1 else np.array([short])
        assert (cut < SEAM_T).all()
        counts[c0:c0 + nc] = SEAM_T - cut
        c0 += nc
    counts[c0:] = rng.integers(1, SEAM_T, SEAM_N - c0)
    acc = np.zeros((SEAM_T, SEAM_N), np.uint8)
    for c in range(SEAM_N):
        acc[0, c] = 1
        acc[1 + rng.choice(SEAM_T - 1, int(counts[c]) - 1, replace=False), c] = 1
    into.accepted[...] = acc
    return into, groups, counts


def assert_adjustment_bits(got, want, fields=None):
    """every field equal bit for bit: the float fields through their int64 views, so that -0.0 != +0.0, with any NaN equal to any NaN"""
    for f in fields or [f for f in AR.FIELDS if f in got]:
        a, b = np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f])
        assert a.shape == b.shape and a.dtype == b.dtype, (f, a.shape, b.shape, a.dtype, b.dtype)
        if a.dtype.kind == "f":
            bad = ~((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b)))
        else:
            bad = a != b
        assert not bad.any(), (f, np.argwhere(bad)[:5], a[bad][:5], b[bad][:5])
