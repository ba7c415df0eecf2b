"""User objectives that draw from the library's generator (include/smmhip.h: SMM_USER_OBJECTIVE_RNG, SMM_USER_PARTIAL_RNG,
smm_normal / smm_normal2 / smm_uniform), and their CPU build: gcc compiles the same text together with a small C restatement of
the stream (`build_shim`) on the oracle's Philox4x32-10 and contract functions (orc_philox4x32_10, orc_math)."""
import ctypes as C
import os
import subprocess
import tempfile

# draws chosen by udata: moment k is normal udata[k] for k < n_udata / 2, uniform udata[k] after that
PROBE_SOURCE = r"""
SMM_USER_OBJECTIVE_RNG(const double* theta, int np, const double* mom, const double* w, int nm,
                       const double* udata, int n_udata, smm_rng_t rng, double* sim_moments, double* value, int* status)
{
    for (int k = 0; k < nm; ++k) {
        const uint64_t i = (uint64_t)udata[k];
        sim_moments[k] = 2 * k < nm ? smm_normal(rng, i) : smm_uniform(rng, i);
    }
    *value = 0.0;
    *status = 1;
}
"""

# AR(1) with Gaussian shocks: y_t = rho y_{t-1} + sigma e_t, e_{2q}, e_{2q+1} = smm_normal2(rng, q); udata = [T (even), fail above rho]
AR1_RNG_SOURCE = r"""
SMM_USER_OBJECTIVE_RNG(const double* theta, int np, const double* mom, const double* w, int nm,
                       const double* udata, int n_udata, smm_rng_t rng, double* sim_moments, double* value, int* status)
{
    const double rho = theta[0], sig = theta[1];
    const int T = (int)udata[0];
    double y = 0.0, yp = 0.0, s1 = 0.0, s2 = 0.0, s12 = 0.0;
    for (int t = 0; t < T; t += 2) {
        double e[2];
        smm_normal2(rng, (uint64_t)(t >> 1), &e[0], &e[1]);
        for (int h = 0; h < 2; ++h) {
            yp = y;
            y = rho * y + sig * e[h];
            s1 += y; s2 += y * y; s12 += y * yp;
        }
    }
    sim_moments[0] = s1 / T;
    if (nm > 1) sim_moments[1] = s2 / T;
    if (nm > 2) sim_moments[2] = s12 / T;
    if (n_udata > 1 && theta[0] > udata[1]) { *status = -2; *value = -1.0; return; }
    double v = 0.0;
    for (int k = 0; k < nm; ++k) { const double d = (sim_moments[k] - mom[k]) / w[k]; v += d * d; }
    *value = v / nm;
    *status = 1;
}
"""

# PANEL_SOURCE (user_objective_src.py) with Gaussian shocks: agent a's shocks of periods 2q, 2q+1 are block a * T / 2 + q
# (T even); udata = [T, agents, fail above rho]
PANEL_RNG_SOURCE = r"""
SMM_USER_PARTIAL_RNG(const double* theta, int np, const double* udata, int n_udata, smm_rng_t rng, int lane, int n_lanes,
                     double* partial)
{
    const double rho = theta[0], sig = theta[1];
    const int T = (int)udata[0], A = (int)udata[1];
    for (int a = lane; a < A; a += n_lanes) {
        double y = 0.0, yp = 0.0;
        for (int t = 0; t < T; t += 2) {
            double e[2];
            smm_normal2(rng, (uint64_t)a * (uint64_t)(T / 2) + (uint64_t)(t >> 1), &e[0], &e[1]);
            for (int h = 0; h < 2; ++h) {
                yp = y;
                y = rho * y + sig * e[h];
                partial[0] += y; partial[1] += y * y; partial[2] += y * yp;
            }
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

# distribution check: lane l draws normals and uniforms K l .. K (l + 1) - 1 of evaluation c's block; udata = [K]
MOMENTS_RNG_SOURCE = r"""
SMM_USER_PARTIAL_RNG(const double* theta, int np, const double* udata, int n_udata, smm_rng_t rng, int lane, int n_lanes,
                     double* partial)
{
    const uint64_t K = (uint64_t)udata[0];
    for (uint64_t i = (uint64_t)lane * K; i < (uint64_t)(lane + 1) * K; ++i) {
        const double z = smm_normal(rng, i), u = smm_uniform(rng, i);
        partial[0] += z; partial[1] += z * z; partial[2] += u; partial[3] += u * u;
        partial[4] += (u < 0.0 || u >= 1.0) ? 1.0 : 0.0;
    }
}

SMM_USER_FINISH(const double* theta, int np, const double* totals, int n_sums, const double* mom, const double* w, int nm,
                const double* udata, int n_udata, double* sim_moments, double* value, int* status)
{
    for (int k = 0; k < nm; ++k) sim_moments[k] = totals[k];
    *value = 0.0;
    *status = 1;
}
"""

_SHIM = r"""
#include <math.h>
#include <stddef.h>
#include <stdint.h>
typedef struct { uint64_t seed; } smm_rng_t;
typedef void (*philox_fn)(const uint32_t* ctr, const uint32_t* key, uint32_t* out);
typedef void (*math_fn)(int what, const double* x, double* y, int n);
static philox_fn g_philox;
static math_fn g_math;
static uint64_t g_seed;
void shim_init(void* philox, void* math) { g_philox = (philox_fn)philox; g_math = (math_fn)math; }
void shim_set_seed(uint64_t seed) { g_seed = seed; }
static void shim_block(smm_rng_t r, uint64_t i, uint32_t c2, uint32_t x[4]) {
    const uint32_t ctr[4] = {(uint32_t)i, (uint32_t)(i >> 32), c2, 0u};
    const uint32_t key[2] = {(uint32_t)r.seed, (uint32_t)(r.seed >> 32) ^ (6u * 0x9E3779B9u)};
    g_philox(ctr, key, x);
}
static uint64_t w64(uint32_t hi, uint32_t lo) { return ((uint64_t)hi << 32) | lo; }
double smm_uniform(smm_rng_t r, uint64_t i) {
    uint32_t x[4];
    shim_block(r, i, 1u, x);
    return (double)(w64(x[0], x[1]) >> 11) * 0x1.0p-53;
}
void smm_normal2(smm_rng_t r, uint64_t j, double* z0, double* z1) {
    uint32_t x[4];
    shim_block(r, j, 0u, x);
    const double u1 = (double)((w64(x[0], x[1]) >> 11) + 1) * 0x1.0p-53, u2 = (double)(w64(x[2], x[3]) >> 11) * 0x1.0p-53;
    double l, s, c;
    g_math(0, &u1, &l, 1); g_math(2, &u2, &s, 1); g_math(3, &u2, &c, 1);
    const double rr = sqrt(-2.0 * l);
    *z0 = rr * c;
    *z1 = rr * s;
}
double smm_normal(smm_rng_t r, uint64_t i) {
    double z0, z1;
    smm_normal2(r, i >> 1, &z0, &z1);
    return (i & 1) ? z1 : z0;
}
#define SMM_USER_OBJECTIVE_RNG void smm_user_objective_rng
#define SMM_USER_PARTIAL_RNG void smm_user_partial_rng
#define SMM_USER_FINISH void smm_user_finish
"""

_ONE_THREAD = r"""
void smm_user_objective(const double* theta, int np, const double* mom, const double* w, int nm, const double* udata, int n_udata,
                        double* sim_moments, double* value, int* status) {
    const smm_rng_t r = {g_seed};
    smm_user_objective_rng(theta, np, mom, w, nm, udata, n_udata, r, sim_moments, value, status);
}
"""

_LANES = r"""
void smm_user_partial(const double* theta, int np, const double* udata, int n_udata, int lane, int n_lanes, double* partial) {
    const smm_rng_t r = {g_seed};
    smm_user_partial_rng(theta, np, udata, n_udata, r, lane, n_lanes, partial);
}
"""


class smm_rng_t(C.Structure):
    _fields_ = [("seed", C.c_uint64)]


class Shim:
    """gcc build of a user source (or of the stream alone: source=None) with the stream restated in C.  `seed` is the key of the
    stream the oracle's hooks draw from (the context's opts.seed; base_seed + i for noseed evaluation i)."""

    def __init__(self, O, source=None, n_sums=None, workdir=None):
        d = workdir or tempfile.mkdtemp(prefix="smm_user_rng_")
        src, so = os.path.join(d, "shim.c"), os.path.join(d, "shim.so")
        text = _SHIM + "#define SMM_NSUMS %d\n" % (n_sums or 1)
        if source is not None:
            text += source + (_ONE_THREAD if n_sums is None else _LANES)
        with open(src, "w") as f:
            f.write(text)
        subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-o", so, src, "-lm"])
        self.lib = C.CDLL(so)
        lib = O.load()
        self.lib.shim_init(C.cast(lib.orc_philox4x32_10, C.c_void_p), C.cast(lib.orc_math, C.c_void_p))
        self.lib.shim_set_seed.argtypes = [C.c_uint64]
        self.lib.smm_uniform.argtypes = [smm_rng_t, C.c_uint64]
        self.lib.smm_uniform.restype = C.c_double
        self.lib.smm_normal.argtypes = [smm_rng_t, C.c_uint64]
        self.lib.smm_normal.restype = C.c_double
        self.lib.smm_normal2.argtypes = [smm_rng_t, C.c_uint64, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        self.source, self.n_sums = source, n_sums

    def set_seed(self, seed):
        self.lib.shim_set_seed(int(seed))

    def hook(self, O, objective_id, seed, lanes=256):
        """the oracle evaluates objective_id through this build, its stream keyed by `seed`"""
        self.set_seed(seed)
        if self.n_sums is None:
            rc = O.load().orc_set_user_objective(int(objective_id), C.cast(self.lib.smm_user_objective, C.c_void_p))
        else:
            rc = O.load().orc_set_user_objective_lanes(int(objective_id), C.cast(self.lib.smm_user_partial, C.c_void_p),
                                                       C.cast(self.lib.smm_user_finish, C.c_void_p), int(self.n_sums), int(lanes))
        O.check_user_id(objective_id, rc)

    def uniform(self, seed, i):
        return self.lib.smm_uniform(smm_rng_t(int(seed)), int(i))

    def normal(self, seed, i):
        return self.lib.smm_normal(smm_rng_t(int(seed)), int(i))

    def normal2(self, seed, j):
        a, b = C.c_double(), C.c_double()
        self.lib.smm_normal2(smm_rng_t(int(seed)), int(j), C.byref(a), C.byref(b))
        return a.value, b.value
