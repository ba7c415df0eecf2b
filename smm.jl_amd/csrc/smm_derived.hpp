// the posterior of user functions of each draw on the device (smm_get_derived, include/smmhip.h) — part of libsmmhip (included by smmhip.hip
// inside its anonymous namespace after smm_group.hpp; gfx950 device code).  Reads the history records hrec [T][N][HW] (smm_params.hpp: H_*)
// and nothing else; writes only the scratch of the call.  The pooled rows are smm_get_group_stats' (smm_group.hpp): group g's members in
// ascending local index from G0[g] of the pooled index space, each member from off[c] in iteration order.
//
//   k_derived_rows : one workgroup per chain walks the chain's window as k_group_gather does (block_rank for select 0 / 1, state_walk for
//                    select 2; both smm_window.hpp) and writes, for the pooled rows [p0, p1) of a batch, which history row each of them
//                    is: ridx[pos - p0] = t N + c (the row's index in hrec, in rows of HW doubles), or -1 for a state row with no a(t).
//
// The kernel that reads these rows, runs the user's function on them and writes the packed columns is compiled by hiprtc with the user's
// source inlined (smm_user_transform_kernel: its text is USER_KERNEL_TRANSFORM of smm_user_host.hpp); from the packed columns on the call
// is smm_get_group_stats' own sequence (k_group_chunk_sum, k_group_mean, pool_order, k_cov_pairs, k_group_cov).
#pragma once

__global__ __launch_bounds__(WINDOW_WG) void k_derived_rows(const double* __restrict__ hrec, int N, int HW, int t0, int n, int sel,
                                                            const int* __restrict__ gid, const long long* __restrict__ off,
                                                            const int* __restrict__ count, long long p0, long long p1,
                                                            long long* __restrict__ ridx) {
    __shared__ int wtot[WINDOW_WG / 64];
    const int c = xcd_chain(blockIdx.x, gridDim.x), tid = threadIdx.x;
    if (gid[c] < 0 || count[c] == 0) return;
    const long long o = off[c];
    if (o >= p1 || o + count[c] <= p0) return;   // (no row of the chain in the batch)
    auto put = [&](long long pos, long long row) {
        if (pos >= p0 && pos < p1) ridx[pos - p0] = row;
    };
    if (sel == 2) {
        state_walk(hrec, N, HW, c, t0, n, wtot, [&](int r, int a, bool) { put(o + r, a < 0 ? -1ll : (long long)a * N + c); });
        return;
    }
    long long base = 0;
    for (int r0 = 0; r0 < n; r0 += WINDOW_WG) {
        const int r = r0 + tid;
        const bool valid = r < n;
        const long long row = (long long)(t0 + (valid ? r : 0)) * N + c;
        const bool take = valid && (sel == 0 || hrec[(size_t)row * HW + H_ACC] != 0.0);
        const long long pos = o + block_rank(take, wtot, base);
        if (take) put(pos, row);
    }
}
