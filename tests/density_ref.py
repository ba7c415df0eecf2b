"""The numerical contract of smm_get_density (include/smmhip.h) restated in numpy: each group's pooled column is hist_ref.columns'
(the selection and pooling of smm_get_histogram); on it the shortest window over the totally ordered column (chain_stats_ref.total_sort)
for the HDI and the half-sample mode, R's bw.nrd0 from chain_stats_ref.mean / quantile and the chain-stats sum chain_diag_ref.S, numpy's
linspace (hist_ref.linspace) and the Gaussian kernel sum, term by term, added by S.  exp and log are parameters: by default the
contract's own functions (oracle.contract_math, smm_oracle.c).  tests/test_density.py holds it against brute force and plain formulas;
the GPU tests hold the device against it, over the history downloaded with smm_get_history."""
import numpy as np

import chain_diag_ref as D
import chain_stats_ref as CS
import hist_ref as HR

SQRT_2PI = 2.5066282746310002


def contract(what):
    """the contract's exp or log over an array (the oracle's restatement in C)"""
    from oracle import oracle
    return lambda x: oracle.contract_math(what, np.asarray(x, np.float64))


def hdi_span(p, m):
    """k of the HDI of mass p over m >= 1 draws: floor of one rounded product, at most m - 1"""
    return min(int(np.floor(np.float64(p) * np.float64(m))), m - 1)


def hdi(s, p):
    """(lo, hi, first row) of the shortest window of hdi_span(p, m) + 1 sorted draws"""
    m = len(s)
    k = hdi_span(p, m)
    with np.errstate(over="ignore"):
        w = s[k:] - s[: m - k]
    i = int(np.argmin(w))
    return s[i], s[i + k], i


def half_sample_mode(s, trail=None):
    """Bickel & Fruehwirth's half-sample mode of the sorted draws s (m >= 1); trail (a list) receives (lo, n) of every level and the
    name of the ending taken"""
    lo, n = 0, len(s)
    while n > 3:
        h = (n + 1) // 2
        with np.errstate(over="ignore"):
            w = s[lo + h - 1: lo + n] - s[lo: lo + n - h + 1]
        if trail is not None:
            trail.append((lo, n))
        lo, n = lo + int(np.argmin(w)), h
    if n == 1:
        end, v = "one", s[lo]
    elif n == 2:
        end, v = "two", (s[lo] + s[lo + 1]) / 2
    else:
        a, b = s[lo + 1] - s[lo], s[lo + 2] - s[lo + 1]
        if a < b:
            end, v = "left", (s[lo] + s[lo + 1]) / 2
        elif b < a:
            end, v = "right", (s[lo + 1] + s[lo + 2]) / 2
        else:
            end, v = "middle", s[lo + 1]
    if trail is not None:
        trail.append(end)
    return v


def var(x):
    """smm_get_trace's variance: S((x - mu) (x - mu)) / (m - 1), mu the chain-stats mean"""
    m = len(x)
    if m < 2:
        return np.nan
    e = x - CS.mean(x)
    return D.S(e * e) / (m - 1)


def bw_nrd0(x, s, exp=None, log=None, trail=None):
    """R's bw.nrd0 by the contract; trail (a list) receives the name of the spread taken: "sd", "iqr", "sd0" (IQR 0), "first" (a
    constant column), "one" (a constant zero column)"""
    exp, log = exp or contract("exp"), log or contract("log")
    m = len(x)
    sl = [float(v) for v in s]
    with np.errstate(invalid="ignore"):
        sd = float(np.sqrt(var(x)))
    a = (CS.quantile(sl, 0.75) - CS.quantile(sl, 0.25)) / 1.34
    l, took = (sd, "sd") if sd < a else (a, "iqr")
    if l == 0:
        l, took = sd, "sd0"
    if l == 0:
        l, took = abs(float(x[0])), "first"
    if l == 0:
        l, took = 1.0, "one"
    if trail is not None:
        trail.append(took)
    return (0.9 * l) * float(exp(-0.2 * log(np.array([float(m)])))[0])


def kernel_terms(x, g, h, exp=None):
    """e [n_grid][m]: the terms of the density's sums"""
    exp = exp or contract("exp")
    rh = 1.0 / h
    with np.errstate(over="ignore", invalid="ignore"):
        u = (g[:, None] - x[None, :]) * rh
        return exp(-0.5 * (u * u)).reshape(len(g), len(x))


def density(x, g, h, exp=None):
    """the density on the grid g: each grid point's terms added by S (row-wise np.sum of the contiguous terms, which test_density.py
    holds against chain_diag_ref.S)"""
    e = np.ascontiguousarray(kernel_terms(x, g, h, exp))
    with np.errstate(invalid="ignore"):
        return (D.rowsum(e) / float(len(x))) / (h * SQRT_2PI)


def column(x, mass, n_grid, rng=None, bw=None, exp=None, log=None):
    """every output of one pooled column x: a dict of status, hdi_lo / hdi_hi [n_mass], mode, bw, kde_status, grid, density, kde_mode"""
    nan = np.nan
    x = np.asarray(x, np.float64)
    m = len(x)
    out = dict(status=0, hdi_lo=np.full(len(mass), nan), hdi_hi=np.full(len(mass), nan), mode=nan, bw=nan, kde_status=1,
               grid=np.full(n_grid, nan), density=np.full(n_grid, nan), kde_mode=nan)
    if m == 0 or not np.isfinite(x).all():
        out["status"] = 2 if m == 0 else 1
        return out
    s = CS.total_sort(x)
    for p, ms in enumerate(mass):
        out["hdi_lo"][p], out["hdi_hi"][p], _ = hdi(s, ms)
    out["mode"] = half_sample_mode(s)
    h = float(bw) if bw is not None else bw_nrd0(x, s, exp, log)
    out["bw"] = h
    if not (np.isfinite(h) and h > 0):
        return out
    lo, hi = (float(rng[0]), float(rng[1])) if rng is not None else (float(s[0]) - 3.0 * h, float(s[-1]) + 3.0 * h)
    with np.errstate(over="ignore"):
        if not np.isfinite(hi - lo):
            out["kde_status"] = 2
            return out
    out["kde_status"] = 0
    if n_grid > 0:
        g = HR.linspace(lo, hi, n_grid - 1)
        d = density(x, g, h, exp)
        out["grid"], out["density"], out["kde_mode"] = g, d, g[int(np.argmax(d))]
    return out


FIELDS = ("status", "hdi_lo", "hdi_hi", "mode", "bw", "kde_status", "grid", "density", "kde_mode")


def density_from_history(h, t0, t1, select, groups, mass=(0.94,), n_grid=128, range=None, bw=None, n_groups=None, exp=None, log=None):
    """what smm_get_density returns (BGPContext.density's dict), from a HistoryBuffers of iterations [0, >= t1); groups None: every
    chain in group 0"""
    N, npar = h.params.shape[2], h.params.shape[1]
    select = HR.SELECT[select] if isinstance(select, str) else int(select)
    groups = np.zeros(N, np.int32) if groups is None else np.asarray(groups, np.int32)
    G = (int(groups.max()) + 1 if len(groups) else 0) if n_groups is None else int(n_groups)
    mass = [float(p) for p in mass]
    exp, log = exp or contract("exp"), log or contract("log")
    cols = HR.columns(h, t0, t1, select, groups, G)
    out = dict(count=np.array([x.shape[1] for x in cols], np.int64), status=np.zeros((G, npar), np.int32), mode=np.empty((G, npar)),
               bw=np.empty((G, npar)), kde_status=np.zeros((G, npar), np.int32))
    if mass:
        out.update(hdi_lo=np.empty((len(mass), G, npar)), hdi_hi=np.empty((len(mass), G, npar)))
    if n_grid:
        out.update(kde_mode=np.empty((G, npar)), grid=np.empty((G, npar, n_grid)), density=np.empty((G, npar, n_grid)))
    for g, x in enumerate(cols):
        for k in np.arange(npar):
            c = column(x[k], mass, n_grid, None if range is None else range[k], None if bw is None else bw[k], exp, log)
            for f in FIELDS:
                if f in out:
                    if f in ("hdi_lo", "hdi_hi"):
                        out[f][:, g, k] = c[f]
                    else:
                        out[f][g, k] = c[f]
    return out


def assert_density_equal(got, want, fields=None):
    """every field bit for bit: NaN equal to NaN, the sign of a zero compared"""
    for f in fields or want:
        a, b = np.asarray(got[f]), np.asarray(want[f])
        assert a.shape == b.shape, (f, a.shape, b.shape)
        if a.dtype.kind == "f":
            same = ((a == b) & (np.signbit(a) == np.signbit(b))) | (np.isnan(a) & np.isnan(b))
        else:
            same = a == b
        assert same.all(), (f, np.argwhere(~same)[:5], a[~same][:5], b[~same][:5])
