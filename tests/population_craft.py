"""Crafted user objectives for the starting population's edge tests (tests/test_population_edges.py, tests/test_gpu_population_edges.py).
The same C text is compiled for the device (S.register_user_objective) and for the oracle (O.register_user_objective); the user kernel and
the oracle's eval_batch hand value and status back unchanged, so the selection of smm_scatter_population sees exactly what is written here.
Everything depends on theta and udata alone.

TIES     value: theta[0] (box [0, 1]) quantised on geometric bands — [0, cut) -> 0, [cut, 2 cut) -> 1/8, [2 cut, 4 cut) -> 2/8, ... up to 1;
         status 1 always; sim_moments: weighted sums of ALL of theta, so the installed moments identify the winner among tied candidates.
         A legal BGP objective (value >= 0, status 1): runs continue on it.  With cut = (1 - 2^(-1/M)) / 2 and initial_value at 1.5 cut
         (band 1, value 1/8; the candidates' window is [0, 0.5 + 1.5 cut]) about half of the chains have a candidate in band 0 — few of them, so
         the lowest tied m is anywhere in 0 .. M - 1 — and the others have their minimum at initial_value's own 1/8 or above.
SPECIAL  theta[0] (box [0, 1]) picks the value class by seven equal bands, rotated by udata[0]: a positive finite value (0.5 + theta[0]),
         +0.0, -0.0, the smallest subnormal, NaN, +inf, -1.0.  theta[1] (box [0, 1]) picks the status by its distance from the centre,
         t = 2 |theta[1] - 0.5|: t < pv / 2 -> 1, t < pv -> 2, then 0, then -2 in equal shares of the rest (pv = udata[1]; udata[2] != 0
         mirrors t, so that the centre fails).  initial_value is the centre of the box: udata sets its class.  Not a BGP objective (a
         negative value with status >= 1 is a hard error in a step): install only."""
import ctypes as C

import numpy as np

import common as cm

_MOMENTS = r"""
    for (int k = 0; k < nm; ++k) {
        double s = 0.0;
        for (int j = 0; j < np; ++j) s += theta[j] * (double)(1 + (j + k) % 3);
        sim_moments[k] = s;
    }
"""
_TIES_VALUE = r"""
    double edge = udata[0], v = 0.0;
    for (int b = 0; b < 8 && theta[0] >= edge; ++b) { v += 0.125; edge += edge; }
    *value = v;
    *status = 1;
"""
_ONE_HEAD = ("SMM_USER_OBJECTIVE(const double* theta, int np, const double* mom, const double* w, int nm,\n"
             "                   const double* udata, int n_udata, double* sim_moments, double* value, int* status)\n{")

TIES_SOURCE = _ONE_HEAD + _MOMENTS + _TIES_VALUE + "}\n"

# the map-reduce form: udata[1] units (>= np, so that every parameter is in the sums), lane l takes units l, l + n_lanes, ...
TIES_LANES_SOURCE = r"""
SMM_USER_PARTIAL(const double* theta, int np, const double* udata, int n_udata, int lane, int n_lanes, double* partial)
{
    const int A = (int)udata[1];
    for (int a = lane; a < A; a += n_lanes)
        for (int i = 0; i < SMM_NSUMS; ++i) partial[i] += theta[(a + i) % np] * (double)(1 + (a + 2 * i) % 5);
}

SMM_USER_FINISH(const double* theta, int np, const double* totals, int n_sums, const double* mom, const double* w, int nm,
                const double* udata, int n_udata, double* sim_moments, double* value, int* status)
{
    for (int k = 0; k < nm; ++k) sim_moments[k] = totals[k % n_sums] + theta[k % np];
""" + _TIES_VALUE + "}\n"

CLASSES = ("positive", "+0", "-0", "subnormal", "nan", "+inf", "negative")      # value class 0 .. 6
SPECIAL_SOURCE = _ONE_HEAD + _MOMENTS + r"""
    int band = (int)(theta[0] * 7.0);
    if (band > 6) band = 6;
    const int cls = (band + (int)udata[0]) % 7;
    const double pv = udata[1];
    double t = theta[1] - 0.5;
    if (t < 0.0) t = -t;
    t = t + t;
    if (udata[2] != 0.0) t = 1.0 - t;
    *status = t < 0.5 * pv ? 1 : t < pv ? 2 : t < 0.5 + 0.5 * pv ? 0 : -2;
    *value = cls == 0 ? 0.5 + theta[0] : cls == 1 ? 0.0 : cls == 2 ? -0.0 : cls == 3 ? 0x1p-1074 : cls == 4 ? __builtin_nan("")
           : cls == 5 ? __builtin_inf() : -1.0;
}
"""
SUBNORMAL = 2.0 ** -1074
# initial_value (the centre: band 3, t = 0) by class -> (udata[0], udata[2]).  "zero" is the valid class of the M = 1 cases: one candidate
# cannot tie another, so the +-0 tie is the one between a -0.0 candidate and an initial_value of +0.0
INIT_KINDS = {"valid": (4, 0), "zero": (5, 0), "nan": (1, 0), "fail": (4, 1)}
INIT_EVAL = {"valid": (1.0, 1), "zero": (0.0, 1), "nan": (np.nan, 1), "fail": (1.0, -2)}      # what initial_value evaluates to


# ---- registration ---------------------------------------------------------------------------------------------------------------------
_device = {}      # (library, source, n_sums, lanes) -> (handle, host build)
_oracle = {}      # (source, n_sums, lanes) -> (handle, host build)


def register(S, O, source, n_sums=None, lanes=256):
    """the handle of `source` in the device library that is current (the test build has a registry of its own) and the same text hooked
    into the oracle under it — again at every use: another test may have taken the handle in the oracle's table meanwhile"""
    from smm_jl_amd import _abi as A
    key = (id(A.load()), source, n_sums, lanes)
    if key not in _device:
        oid = S.register_user_objective(source, n_sums=n_sums, lanes=lanes)
        _device[key] = (oid, C.CDLL(O.register_user_objective(source, oid, n_sums=n_sums, lanes=lanes)))
    oid, host = _device[key]
    O.hook_user_objective(host, oid, n_sums, lanes)
    return oid


def oracle_only(O, source, n_sums=None, lanes=256):
    """without a device: a handle from the upper half of the oracle's table (the library hands its handles out from the bottom)"""
    key = (source, n_sums, lanes)
    if key not in _oracle:
        oid = 1000 + O.load().orc_max_user() - 20 - len(_oracle)
        _oracle[key] = (oid, C.CDLL(O.register_user_objective(source, oid, n_sums=n_sums, lanes=lanes)))
    oid, host = _oracle[key]
    O.hook_user_objective(host, oid, n_sums, lanes)
    return oid


# ---- problems -------------------------------------------------------------------------------------------------------------------------
def ties_cut(M):
    return 0.5 * (1.0 - 0.5 ** (1.0 / M))


def ties_problem(S, oid, M, N, T, seed, npar=2, nm=2, units=0, N_local=None, chain_offset=0):
    cut = ties_cut(M)
    init = np.concatenate([[1.5 * cut], 0.1 * np.arange(1, npar)])
    lb, ub = np.concatenate([[0.0], -np.ones(npar - 1)]), np.ones(npar)
    prob = S.Problem(init=init, lb=lb, ub=ub, mom=np.zeros(nm), w=np.ones(nm), ns=1, objective_id=oid, obj_params=[cut, float(units)])
    opts = S.BGPOpts(N=N if N_local is None else N_local, maxiter=T, sigma=0.05 * cm.temps(N, 4.0), acc_tuner=np.geomspace(3.0, 0.5, N),
                     min_improve=np.zeros(N), seed=seed, N_global=N, chain_offset=chain_offset)
    return prob, opts


def special_problem(S, oid, init_kind, pv, N, seed, T=2):
    shift, flip = INIT_KINDS[init_kind]
    prob = S.Problem(init=[0.5, 0.5, 0.0], lb=[0.0, 0.0, -1.0], ub=[1.0, 1.0, 1.0], mom=np.zeros(2), w=np.ones(2), ns=1, objective_id=oid,
                     obj_params=[float(shift), pv, float(flip)])
    opts = S.BGPOpts(N=N, maxiter=T, sigma=0.05 * cm.temps(N, 4.0), acc_tuner=np.geomspace(3.0, 0.5, N), min_improve=np.zeros(N), seed=seed,
                     N_global=N)
    return prob, opts


# ---- the cases of the GPU tier (their premises: tests/test_population_edges.py) -------------------------------------------------------
T_TIES = 10
# (N, M) -> opts.seed.  The seeds are searched: with three chains the premises of a case (a tie across the lane trips, a winner from a later
# trip, initial_value tying the best candidate and losing to it, two chains tied) hold for about one seed in some thousands at M = 65
TIES_SEEDS = {(3, 2): 6, (70, 2): 14144, (3, 64): 21, (70, 64): 2, (3, 65): 752, (70, 65): 129, (3, 128): 21, (70, 128): 109, (3, 129): 16,
              (70, 129): 114, (3, 200): 12, (70, 200): 109, (3, 1000): 8, (20, 6): 14, (64, 9): 6}
TIES_CASES = [(N, M) for M in (2, 64, 65, 128, 129, 200) for N in (3, 70)] + [(3, 1000)]
# the shapes of the user layout: name -> (N, M).  theta[0]'s draw does not depend on np, so the value table is the same at any (np, nm)
TIES_SHAPE_CASES = {"5x3": (20, 6), "1x2": (20, 6), "lanes": (20, 6), "shard": (64, 9)}
TIES_SHAPES = {"5x3": dict(npar=5, nm=3), "1x2": dict(npar=1, nm=2), "lanes": dict(npar=3, nm=2, units=7), "shard": dict(npar=5, nm=3)}
LANES = dict(n_sums=2, lanes=64)      # the map-reduce form of TIES_LANES_SOURCE

# (M, init_kind) -> (pv, N, opts.seed): the share of status >= 1 falls with M, so that chains without a valid candidate remain
SPECIAL_N = 70
SPECIAL_PV = {1: 0.5, 2: 0.5, 129: 0.03}
SPECIAL_SEEDS = {(1, "fail"): 22, (2, "fail"): 24}      # (the others: 21)
SPECIAL_CASES = [(M, kind) for M in (1, 2, 129) for kind in (("zero" if M == 1 else "valid"), "nan", "fail")]


def ties_case(S, oid, N, M, **kw):
    return ties_problem(S, oid, M, N, T_TIES, TIES_SEEDS[(N, M)], **kw)


def special_case(S, oid, M, kind):
    return special_problem(S, oid, kind, SPECIAL_PV[M], SPECIAL_N, SPECIAL_SEEDS.get((M, kind), 21))


# ---- the premises, from the reference's value / status tables [N][M] --------------------------------------------------------------------
def ties_facts(v, pick_keep, init_value):
    """per-chain facts of a TIES case: which chains tie at their minimum, tie across the lane trips (m < 64 and m >= 64), win from a later
    trip, and how initial_value stands against the best candidate"""
    best = v.min(axis=1)
    at_min = v == best[:, None]
    first = at_min.argmax(axis=1)
    lo, hi = at_min[:, :64].any(axis=1), at_min[:, 64:].any(axis=1)
    return dict(tied=np.flatnonzero(at_min.sum(axis=1) >= 2), across=np.flatnonzero(lo & hi), late=np.flatnonzero(first >= 64),
                init_ties=np.flatnonzero((best == init_value) & (pick_keep == -1)), init_worse=np.flatnonzero(best < init_value))


def value_class(v):
    """the class 0 .. 6 of every value (CLASSES)"""
    v = np.asarray(v)
    with np.errstate(invalid="ignore"):
        return np.select([np.isnan(v), v == np.inf, v == -1.0, (v == 0) & ~np.signbit(v), (v == 0) & np.signbit(v), v == SUBNORMAL],
                         [4, 5, 6, 1, 2, 3], 0)


def special_facts(v, st, ok):
    """per-chain facts of a SPECIAL case (ok: population_ref.valid of the tables)"""
    cls = value_class(v)
    raw = np.where(np.isnan(v), np.inf, v).argmin(axis=1)           # the lowest value whatever its validity
    zero_p, zero_m = (ok & (cls == 1)).any(axis=1), (ok & (cls == 2)).any(axis=1)
    return dict(cls=cls, none_valid=np.flatnonzero(~ok.any(axis=1)), raw_invalid=np.flatnonzero(~ok[np.arange(len(raw)), raw]),
                zero_tie=np.flatnonzero(zero_p & zero_m), minus_zero_only=np.flatnonzero(zero_m & ~zero_p))
