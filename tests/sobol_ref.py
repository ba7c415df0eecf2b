"""smm_sens_sobol's numerical contract (include/smmhip.h) in numpy: the Sobol' first-order (Saltelli et al. 2010) and total-order (Jansen
1999) indices of the objective value and of every simulated moment over a box, from an injected `evaluator(P [np][n]) -> (value [n], simM
[nm][n], status [n])`.  Built only from what the tests already use: the oracle's Philox for the uniforms.  The points, the validity rule,
the pilot's centre, the blocked sum T and the estimators are stated here.  One evaluator call for the pilot and one per batch of base
points, evaluation m * nb + jj of a batch being matrix m at its base point jj: also the host loop the library offered before the device call
(tools/sens_sobol_time.py).  Beyond the contract it keeps what the tests assert on the restatement alone (`complete`, `yA`, and, with
centre0=True, the estimator without the centre)."""
import numpy as np

STREAM_GSA = 9
T_BLOCK = 256
PILOT = 256
DBL_MAX = np.finfo(np.float64).max
TABLES = ("first", "total", "v_first", "v_total", "se_first", "se_total")
FIELDS = ("mean", "var", "centre") + TABLES
SCALARS = ("n_complete", "n_invalid", "evaluated")


def key_of(seed):
    return [seed & 0xffffffff, ((seed >> 32) ^ (STREAM_GSA * 0x9E3779B9)) & 0xffffffff]


def u53(hi, lo):
    return float(((hi << 32) | lo) >> 11) * 2.0 ** -53


def base_u(O, seed, npar, N, which):
    """u [np][N] of matrix A (which = 0) or B (1): base point j, parameter k from the block at counter {j, which, k >> 1, 0}"""
    key = key_of(seed)
    u = np.empty((npar, N))
    for j in range(N):
        for q in range((npar + 1) // 2):
            x = O.philox([j, which, q, 0], key)
            u[2 * q, j] = u53(x[0], x[1])
            if 2 * q + 1 < npar:
                u[2 * q + 1, j] = u53(x[2], x[3])
    return u


def to_theta(u, lo, hi):
    """u * (hi - lo) + lo, each operation rounded"""
    lo, hi = np.asarray(lo, float)[:, None], np.asarray(hi, float)[:, None]
    return u * (hi - lo) + lo


def batch_points(thA, thB, j0, nb):
    """P [np][(np + 2) nb]: matrix 0 is A, 1 is B, 2 + i is A with coordinate i from B, at base points [j0, j0 + nb)"""
    npar = thA.shape[0]
    a, b = thA[:, j0:j0 + nb], thB[:, j0:j0 + nb]
    mats = [a, b]
    for i in range(npar):
        ab = a.copy()
        ab[i] = b[i]
        mats.append(ab)
    return np.ascontiguousarray(np.concatenate(mats, 1))


def outputs(evaluator, P, nm):
    """(y [F][n], valid [n]): output 0 the value, 1 + f moment f; valid: status >= 1 and every output finite"""
    v, sm, st = evaluator(P)
    y = np.concatenate([np.asarray(v, float)[None, :], np.asarray(sm, float).reshape(nm, -1)], 0)
    with np.errstate(invalid="ignore"):
        valid = (np.asarray(st) >= 1) & (np.abs(y) <= DBL_MAX).all(0)
    return y, valid


def T(x, ok):
    """the blocked sum over the last axis in j order: blocks of 256 from 0, each from 0.0 left to right skipping the points that are not
    ok, the block sums from 0.0 left to right"""
    x = np.asarray(x, float)
    N = x.shape[-1]
    total = np.zeros(x.shape[:-1])
    with np.errstate(all="ignore"):
        for b0 in range(0, N, T_BLOCK):
            blk = np.zeros(x.shape[:-1])
            for j in range(b0, min(b0 + T_BLOCK, N)):
                if ok[j]:
                    blk = blk + x[..., j]
            total = total + blk
    return total


def sens_sobol(O, evaluator, seed, lb, ub, nm, N, lo=None, hi=None, batch=None, centre0=False):
    lb, ub = np.asarray(lb, float), np.asarray(ub, float)
    lo = lb if lo is None else np.asarray(lo, float)
    hi = ub if hi is None else np.asarray(hi, float)
    npar, F = len(lb), nm + 1
    assert 1 <= N <= 2 ** 20 and ((lb <= lo) & (lo <= hi) & (hi <= ub)).all()
    thA, thB = to_theta(base_u(O, seed, npar, N, 0), lo, hi), to_theta(base_u(O, seed, npar, N, 1), lo, hi)
    # the pilot
    n_pilot = min(N, PILOT)
    yp, okp = outputs(evaluator, np.ascontiguousarray(thA[:, :n_pilot]), nm)
    cnt = int(okp.sum())
    centre = T(yp, okp) / np.float64(cnt) if cnt else np.zeros(F)
    if centre0:
        centre = np.zeros(F)
    # the batches
    nb_max = N if batch is None else max(1, min(N, int(batch)))
    yA, yB, yAB = np.empty((F, N)), np.empty((F, N)), np.empty((npar, F, N))
    complete = np.empty(N, bool)
    n_invalid = 0
    for j0 in range(0, N, nb_max):
        nb = min(nb_max, N - j0)
        y, valid = outputs(evaluator, batch_points(thA, thB, j0, nb), nm)
        y, valid = y.reshape(F, npar + 2, nb), valid.reshape(npar + 2, nb)
        n_invalid += int((~valid).sum())
        complete[j0:j0 + nb] = valid.all(0)
        yA[:, j0:j0 + nb], yB[:, j0:j0 + nb] = y[:, 0], y[:, 1]
        yAB[:, :, j0:j0 + nb] = np.moveaxis(y[:, 2:], 1, 0)
    n = np.float64(int(complete.sum()))
    with np.errstate(all="ignore"):
        mean = T(yA, complete) / n
        d = yA - mean[:, None]
        var = T(d * d, complete) / n
        p = (yB - centre[:, None])[None] * (yAB - yA[None])            # [np][F][N]
        e = yA[None] - yAB
        q = e * e
        h = 0.5 * q
        v_first = T(p, complete) / n
        v_total = T(q, complete) / (2.0 * n)
        rf = T(p * p, complete) / n - v_first * v_first
        rt = T(h * h, complete) / n - v_total * v_total
        rf, rt = np.where(rf < 0.0, 0.0, rf), np.where(rt < 0.0, 0.0, rt)
        v = var[None, :]
        out = dict(first=v_first / v, total=v_total / v, v_first=v_first, v_total=v_total, se_first=np.sqrt(rf / n) / v, se_total=np.sqrt(rt / n) / v)
    out = {f: np.ascontiguousarray(a.T) for f, a in out.items()}          # [F][np]
    out.update(mean=mean, var=var, centre=centre, n_complete=int(n), n_invalid=n_invalid, evaluated=N * (npar + 2) + n_pilot, complete=complete, yA=yA)
    return out


def assert_equal(got, want):
    """every output field bit for bit (NaN equal to NaN; a zero's sign counts), and the scalars"""
    for f in FIELDS:
        a, b = np.asarray(got[f]), np.asarray(want[f])
        assert a.shape == b.shape, (f, a.shape, b.shape)
        assert np.array_equal(a, b, equal_nan=True), (f, a, b)
        num = ~(np.isnan(a) | np.isnan(b))
        assert np.array_equal(np.signbit(a)[num], np.signbit(b)[num]), (f, a, b)
    for f in SCALARS:
        assert got[f] == want[f], (f, got[f], want[f])
