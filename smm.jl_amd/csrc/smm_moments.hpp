// simulated moments per group: fit, Jacobian, sensitivity and standard errors (smm_get_moment_stats, include/smmhip.h) — part of libsmmhip
// (included by smmhip.hip inside its anonymous namespace after smm_group.hpp; gfx950 device code).  Reads the history records hrec
// [T][N][HW] (smm_params.hpp: H_*) and nothing else; writes only the scratch and result buffers of the call.  The D = np + nm joint
// columns of a group (the parameters, then the simulated moments stored behind them in the record) are pooled, cut into chunks and
// summed exactly as smm_group.hpp pools the parameters: its kernels, k_group_gather (the three selections, the not-finite flag gbad)
// among them, and k_cov_pairs (smm_cov.hpp) run on them with D columns, so the cov_pp block is smm_get_group_stats' covariance bit for
// bit.  What is the moments' own:
//
//   k_moment_cov_acc : one lane per (group, pair a >= b): the batch's chunk sums of k_cov_pairs added in chunk order onto the group's
//                      running sum, S = S + s_c; across the batches of chunks that is the contract's sum from 0.0.
//   k_moment_solve   : one workgroup of one wave per group, lane = row.  Splits the joint results into the call's blocks (means, medians,
//                      quantiles, cov_pp / cov_pm / cov_mm = S / (m - 1), fit_z) and decides the status; then in LDS (np, nm <= 64:
//                      three matrices of at most 64 x 65 doubles, 97.5 KB of the workgroup's 160 KB): A = cov_pp with the ridge and its
//                      lower Cholesky factor in k_cov_chol's order; J row by row, lane = moment, forward then back substitution; B = J'WJ,
//                      lane = row; its factor; Lambda column by column, lane = moment, over J's rows in place once jac is written; se,
//                      lane = parameter.  Every sum runs in ascending index inside one lane: nothing is reduced across lanes.
#pragma once

constexpr int MOMENT_WG = 64;   // lanes of k_moment_solve: a row of the largest matrix each
static_assert(MAX_DIM <= MOMENT_WG, "k_moment_solve: lane = row");

// csum2 [D][D][nb]: k_cov_pairs' raw sums of the chunks [cb0, cb0 + nb); acc [G][D][D], entry (a, b), a >= b
__global__ void k_moment_cov_acc(const double* __restrict__ csum2, int nb, int cb0, const int* __restrict__ gch0, int G, int D,
                                 double* __restrict__ acc) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x, npp = D * (D + 1) / 2;
    if (e >= G * npp) return;
    const int g = e / npp;
    int q = e - g * npp, a = 0;
    while (q > a) { q -= a + 1; ++a; }
    const int b = q;
    const int lo = max(gch0[g], cb0), hi = min(gch0[g + 1], cb0 + nb);
    if (lo >= hi) return;
    double S = acc[((size_t)g * D + a) * D + b];
    for (int ch = lo; ch < hi; ++ch) S = S + csum2[((size_t)a * D + b) * nb + (ch - cb0)];
    acc[((size_t)g * D + a) * D + b] = S;
}

// the lower Cholesky factor of the n x n matrix M (row stride ld, lower triangle) in place, lane k = row k, in k_cov_chol's order; *bad is
// set for a pivot that is not > 0.  Every lane of the workgroup calls it.
__device__ __forceinline__ void moment_chol(double* __restrict__ M, int n, int ld, int k, int* __restrict__ bad) {
    for (int j = 0; j < n; ++j) {
        if (k == j) {
            double s = M[j * ld + j];
            for (int i = 0; i < j; ++i) {
                const double p = M[j * ld + i] * M[j * ld + i];
                s = s - p;
            }
            if (!(s > 0.0)) *bad = 1;
            M[j * ld + j] = sqrt(s);
        }
        __syncthreads();
        if (k > j && k < n) {
            double s = M[k * ld + j];
            for (int i = 0; i < j; ++i) {
                const double p = M[k * ld + i] * M[j * ld + i];
                s = s - p;
            }
            M[k * ld + j] = s / M[j * ld + j];
        }
        __syncthreads();
    }
}

// x (n entries, in place: the right-hand side on entry) solved against the factor L of moment_chol: forward, then back substitution,
// the sums in ascending index, subtracting term by term.  One lane's own vector.
__device__ __forceinline__ void moment_subst(const double* __restrict__ L, int n, int ld, double* __restrict__ x) {
    for (int i = 0; i < n; ++i) {
        double s = x[i];
        for (int j = 0; j < i; ++j) {
            const double p = L[i * ld + j] * x[j];
            s = s - p;
        }
        x[i] = s / L[i * ld + i];
    }
    for (int i = n - 1; i >= 0; --i) {
        double s = x[i];
        for (int j = i + 1; j < n; ++j) {
            const double p = L[j * ld + i] * x[j];
            s = s - p;
        }
        x[i] = s / L[i * ld + i];
    }
}

struct MomentOut {   // the call's result slices on the device (NULL: not asked for)
    int* status;
    double *p_mean, *m_mean, *m_median, *m_quantile, *cov_pp, *cov_pm, *cov_mm, *fit_z, *jac, *sens, *se;
};

// acc [G][D][D] (a >= b): the groups' sums of centred products (NULL: no covariance asked for); mean, median [G][D], quant [nq][G][D]:
// the joint columns' (median, quant NULL: not computed); solve != 0: status, jac, sens and se are wanted
__global__ __launch_bounds__(MOMENT_WG) void k_moment_solve(const double* __restrict__ acc, const double* __restrict__ mean,
                                                            const double* __restrict__ median, const double* __restrict__ quant,
                                                            const long long* __restrict__ gm, const int* __restrict__ gbad, int G, int np,
                                                            int nm, int nq, double ridge, const double* __restrict__ mom,
                                                            const double* __restrict__ w, int solve, MomentOut o) {
    extern __shared__ __align__(16) double sm[];   // A [np][np + 1], B [np][np + 1], JL [nm][np + 1]
    __shared__ double sW[MAX_DIM], sS2[MAX_DIM];
    __shared__ int bad;
    const int g = blockIdx.x, tid = threadIdx.x, D = np + nm, ld = np + 1;
    double* A = sm;
    double* B = A + (size_t)np * ld;
    double* JL = B + (size_t)np * ld;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    const long long m = gm[g];
    const bool few = m < 2, nonfin = gbad[g] != 0;
    int status = few ? 1 : nonfin ? 2 : 0;
    const bool all_nan = status == 2;
    const double den = (double)(m - 1);
    // cov of the joint columns (a, b)
    auto cv = [&](int a, int b) {
        if (status != 0 || !acc) return qnan;
        const int hi = a >= b ? a : b, lo = a >= b ? b : a;
        return acc[((size_t)g * D + hi) * D + lo] / den;
    };
    if (tid == 0) bad = 0;
    for (int k = tid; k < np; k += MOMENT_WG)
        if (o.p_mean) o.p_mean[(size_t)g * np + k] = all_nan ? qnan : mean[(size_t)g * D + k];
    for (int k = tid; k < nm; k += MOMENT_WG) {
        const double mu = all_nan ? qnan : mean[(size_t)g * D + np + k];
        if (o.m_mean) o.m_mean[(size_t)g * nm + k] = mu;
        if (o.m_median) o.m_median[(size_t)g * nm + k] = all_nan ? qnan : median[(size_t)g * D + np + k];
        for (int p = 0; p < nq; ++p)
            o.m_quantile[((size_t)p * G + g) * nm + k] = all_nan ? qnan : quant[((size_t)p * G + g) * D + np + k];
        if (o.fit_z) {
            const double d = mu - mom[k];
            o.fit_z[(size_t)g * nm + k] = d / sqrt(cv(np + k, np + k));
        }
    }
    if (o.cov_pp)
        for (int e = tid; e < np * np; e += MOMENT_WG) o.cov_pp[(size_t)g * np * np + e] = cv(e / np, e % np);
    if (o.cov_pm)
        for (int e = tid; e < np * nm; e += MOMENT_WG) o.cov_pm[(size_t)g * np * nm + e] = cv(e / nm, np + e % nm);
    if (o.cov_mm)
        for (int e = tid; e < nm * nm; e += MOMENT_WG) o.cov_mm[(size_t)g * nm * nm + e] = cv(np + e / nm, np + e % nm);
    if (!solve) return;
    // what a status leaves undefined: jac from 3 on, sens and se from 4 on (1, 2: all of them)
    auto finish = [&](int st) {
        if (st != 0 && st != 4 && o.jac)
            for (int e = tid; e < nm * np; e += MOMENT_WG) o.jac[(size_t)g * nm * np + e] = qnan;
        if (st != 0) {
            if (o.sens)
                for (int e = tid; e < np * nm; e += MOMENT_WG) o.sens[(size_t)g * np * nm + e] = qnan;
            if (o.se)
                for (int e = tid; e < np; e += MOMENT_WG) o.se[(size_t)g * np + e] = qnan;
        }
        if (tid == 0 && o.status) o.status[g] = st;
    };
    if (status != 0) { finish(status); return; }
    const int k = tid;
    if (k < np)
        for (int j = 0; j <= k; ++j) {
            double v = cv(k, j);
            if (j == k) {
                const double p = ridge * v;
                v = v + p;
            }
            A[k * ld + j] = v;
        }
    if (k < nm) {
        const double wk = w[k];
        const double s = (isfinite(wk) && wk != 0.0) ? wk : 1.0;
        const double s2 = s * s;
        sS2[k] = s2;
        sW[k] = 1.0 / s2;
    }
    __syncthreads();
    moment_chol(A, np, ld, k, &bad);
    if (bad) { finish(3); return; }
    if (k < nm) {   // J's row k: A x = cov_pm's column k
        double* x = JL + (size_t)k * ld;
        for (int i = 0; i < np; ++i) x[i] = cv(i, np + k);
        moment_subst(A, np, ld, x);
        if (o.jac)
            for (int i = 0; i < np; ++i) o.jac[((size_t)g * nm + k) * np + i] = x[i];
    }
    __syncthreads();
    if (k < np)
        for (int j = 0; j <= k; ++j) {
            double S = 0.0;
            for (int q = 0; q < nm; ++q) {
                double t = JL[q * ld + k] * sW[q];
                t = t * JL[q * ld + j];
                S = S + t;
            }
            B[k * ld + j] = S;
        }
    __syncthreads();
    moment_chol(B, np, ld, k, &bad);
    if (bad) { finish(4); return; }
    if (k < nm) {   // Lambda's column k over J's row k: B x = -(J'W)'s column k
        double* x = JL + (size_t)k * ld;
        for (int i = 0; i < np; ++i) {
            const double t = x[i] * sW[k];
            x[i] = -t;
        }
        moment_subst(B, np, ld, x);
        if (o.sens)
            for (int i = 0; i < np; ++i) o.sens[((size_t)g * np + i) * nm + k] = x[i];
    }
    __syncthreads();
    if (k < np && o.se) {
        double S = 0.0;
        for (int q = 0; q < nm; ++q) {
            double t = JL[q * ld + k] * JL[q * ld + k];
            t = t * sS2[q];
            S = S + t;
        }
        o.se[(size_t)g * np + k] = sqrt(S);
    }
    finish(0);
}
