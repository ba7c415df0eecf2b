"""A user objective in the form include/smmhip.h prescribes — an AR(1) simulation with three moments.  The same text
is compiled by hiprtc for the device and by gcc for the oracle (tests only); it is pure arithmetic, so both agree to
the bit."""

AR1_SOURCE = r"""
SMM_USER_OBJECTIVE(const double* theta, int np, const double* mom, const double* w, int nm,
                   const double* udata, int n_udata, double* sim_moments, double* value, int* status)
{
    /* y_t = rho y_{t-1} + sigma e_t with a fixed shock stream; moments: mean(y), mean(y^2), mean(y_t y_{t-1}) */
    const double rho = theta[0], sig = theta[1];
    const int T = (int)udata[0];
    unsigned long long st = 12345ull;
    double y = 0.0, yp = 0.0, s1 = 0.0, s2 = 0.0, s12 = 0.0;
    for (int t = 0; t < T; ++t) {
        st = st * 6364136223846793005ull + 1442695040888963407ull;
        const double u = (double)(st >> 11) * (1.0 / 9007199254740992.0) - 0.5;
        yp = y;
        y = rho * y + sig * u;
        s1 += y; s2 += y * y; s12 += y * yp;
    }
    sim_moments[0] = s1 / T;
    if (nm > 1) sim_moments[1] = s2 / T;
    if (nm > 2) sim_moments[2] = s12 / T;
    if (n_udata > 1 && theta[0] > udata[1]) { *status = -2; *value = -1.0; return; }   /* the model "fails" here */
    double v = 0.0;
    for (int k = 0; k < nm; ++k) { const double d = (sim_moments[k] - mom[k]) / w[k]; v += d * d; }
    *value = v / nm;
    *status = 1;
}
"""


def ar1_numpy(theta, mom, w, udata):
    """independent restatement for the CPU-only test"""
    import numpy as np
    rho, sig = float(theta[0]), float(theta[1])
    T = int(udata[0])
    st = 12345
    y = 0.0; s1 = s2 = s12 = 0.0
    for _ in range(T):
        st = (st * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        u = float(st >> 11) * (1.0 / 9007199254740992.0) - 0.5
        yp = y
        y = rho * y + sig * u
        s1 += y; s2 += y * y; s12 += y * yp
    sm = np.array([s1 / T, s2 / T, s12 / T])[:len(mom)]
    if len(udata) > 1 and rho > udata[1]:
        return sm, -1.0, -2
    d = (sm - np.asarray(mom)) / np.asarray(w)
    return sm, float((d * d).sum() / len(mom)), 1


# The map-reduce form: a panel of AR(1) agents; lane l simulates agents l, l + n_lanes, ...; three sums.
PANEL_SOURCE = r"""
SMM_USER_PARTIAL(const double* theta, int np, const double* udata, int n_udata, int lane, int n_lanes, double* partial)
{
    const double rho = theta[0], sig = theta[1];
    const int T = (int)udata[0], A = (int)udata[1];
    for (int a = lane; a < A; a += n_lanes) {
        unsigned long long st = 12345ull + 7919ull * (unsigned long long)a;
        double y = 0.0, yp = 0.0;
        for (int t = 0; t < T; ++t) {
            st = st * 6364136223846793005ull + 1442695040888963407ull;
            const double u = (double)(st >> 11) * (1.0 / 9007199254740992.0) - 0.5;
            yp = y;
            y = rho * y + sig * u;
            partial[0] += y; partial[1] += y * y; partial[2] += y * yp;
        }
    }
}

SMM_USER_FINISH(const double* theta, int np, const double* totals, int n_sums, const double* mom, const double* w, int nm,
                const double* udata, int n_udata, double* sim_moments, double* value, int* status)
{
    const double n = udata[0] * udata[1];
    double v = 0.0;
    for (int k = 0; k < nm; ++k) {
        sim_moments[k] = totals[k] / n;
        const double d = (sim_moments[k] - mom[k]) / w[k];
        v += d * d;
    }
    *value = v / nm;
    *status = (n_udata > 2 && theta[0] > udata[2]) ? -2 : 1;
    if (*status < 0) *value = -1.0;
}
"""


# A generic objective whose shape is set by the problem: any np, nm (<= 64) and number of sums (<= 64: SMM_NSUMS in the
# map-reduce form, udata[2] in the one-thread form).  udata = [A units, fail above this last parameter, sums (one-thread form)].
# Sum i over units a: theta[i % np] * c(a, i) + d(a, i), c a small integer, d a small multiple of 1/4 — with theta on a dyadic grid
# (multiples of 2^-10 in [-1, 1]) every term and every partial sum is exact, so the order of the sums does not matter.
# Moment k reads sum k % n_sums and parameter 5k % np.  A failing evaluation writes NaN to its last moment.
_GEN_TERM = "theta[i % np] * (double)((a + 3 * i) % 7 - 3) + 0.25 * (double)((5 * a + i) % 9 - 4)"
_GEN_FINISH = r"""
    for (int k = 0; k < nm; ++k) sim_moments[k] = TOT[k % NS] / A + 0.5 * theta[(5 * k) % np];
    if (theta[np - 1] > udata[1]) { sim_moments[nm - 1] = __builtin_nan(""); *value = -1.0; *status = -2; return; }
    double v = 0.0;
    for (int k = 0; k < nm; ++k) { const double d = (sim_moments[k] - mom[k]) / w[k]; v += d * d; }
    *value = v / nm;
    *status = 1;
}
"""


def _one_thread(rng):
    head = ("SMM_USER_OBJECTIVE_RNG(const double* theta, int np, const double* mom, const double* w, int nm,\n"
            "                       const double* udata, int n_udata, smm_rng_t rng, double* sim_moments, double* value, int* status)\n"
            if rng else
            "SMM_USER_OBJECTIVE(const double* theta, int np, const double* mom, const double* w, int nm,\n"
            "                   const double* udata, int n_udata, double* sim_moments, double* value, int* status)\n")
    return head + r"""{
    const int A = (int)udata[0], ns = (int)udata[2];
    double tot[64];
    for (int i = 0; i < ns; ++i) tot[i] = 0.0;
    for (int a = 0; a < A; ++a)
        for (int i = 0; i < ns; ++i) tot[i] += TERM;
""".replace("TERM", _GEN_TERM + (" + 0.25 * smm_normal(rng, (uint64_t)a * 64u + (uint64_t)i)" if rng else "")) + \
        _GEN_FINISH.replace("TOT", "tot").replace("NS", "ns")


def _map_reduce(rng):
    head = ("SMM_USER_PARTIAL_RNG(const double* theta, int np, const double* udata, int n_udata, smm_rng_t rng, int lane, int n_lanes,\n"
            "                     double* partial)\n"
            if rng else
            "SMM_USER_PARTIAL(const double* theta, int np, const double* udata, int n_udata, int lane, int n_lanes, double* partial)\n")
    return head + r"""{
    const int A = (int)udata[0];
    for (int a = lane; a < A; a += n_lanes)
        for (int i = 0; i < SMM_NSUMS; ++i) partial[i] += TERM;
}

SMM_USER_FINISH(const double* theta, int np, const double* totals, int n_sums, const double* mom, const double* w, int nm,
                const double* udata, int n_udata, double* sim_moments, double* value, int* status)
{
    const int A = (int)udata[0];""".replace("TERM", _GEN_TERM + (" + 0.25 * smm_normal(rng, (uint64_t)a * 64u + (uint64_t)i)" if rng else "")) + \
        _GEN_FINISH.replace("TOT", "totals").replace("NS", "n_sums")


GENERIC_SOURCE = _one_thread(False)
GENERIC_LANES_SOURCE = _map_reduce(False)
GENERIC_RNG_SOURCE = _one_thread(True)
GENERIC_LANES_RNG_SOURCE = _map_reduce(True)


def generic_numpy(theta, mom, w, udata, n_sums):
    """restatement of GENERIC_SOURCE (n_sums = udata[2]) and GENERIC_LANES_SOURCE (n_sums = SMM_NSUMS) over the columns of theta
    [np][M], in the sources' order of operations; the sums are exact at dyadic theta, so it equals either form to the bit there.
    -> (value [M], sim_moments [nm][M], status [M])"""
    import numpy as np
    theta = np.asarray(theta, np.float64)
    np_, M = theta.shape
    nm = len(mom)
    A = int(udata[0])
    a = np.arange(A)[:, None]
    tot = np.empty((n_sums, M))
    for i in range(n_sums):
        c = ((a + 3 * i) % 7 - 3).astype(np.float64)
        d = ((5 * a + i) % 9 - 4).astype(np.float64)
        tot[i] = (theta[i % np_][None, :] * c + 0.25 * d).sum(axis=0)
    sm = np.empty((nm, M))
    for k in range(nm):
        sm[k] = tot[k % n_sums] / float(A) + 0.5 * theta[(5 * k) % np_]
    fail = theta[np_ - 1] > udata[1]
    v = np.zeros(M)
    for k in range(nm):
        dk = (sm[k] - mom[k]) / w[k]
        v = v + dk * dk
    v = v / nm
    sm[nm - 1, fail] = np.nan
    return np.where(fail, -1.0, v), sm, np.where(fail, -2, 1).astype(np.int8)


def generic_moments(nm):
    """targets and weights of the generic objective: mom_k != w_k, both varying with k"""
    import numpy as np
    k = np.arange(nm)
    return 0.125 * ((3 * k) % 11) - 0.5, 1.0 + 0.25 * (k % 5)


def dyadic_thetas(np_, M, seed, last_above=None):
    """M points of [-1, 1]^np on multiples of 2^-10 (columns); every third point's last parameter above `last_above` if given"""
    import numpy as np
    rng = np.random.default_rng(seed)
    th = rng.integers(-1024, 1025, (np_, M)) / 1024.0
    if last_above is not None:
        th[np_ - 1, ::3] = np.maximum(th[np_ - 1, ::3], last_above + 1.0 / 1024.0)
    return th
