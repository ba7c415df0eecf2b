// the walk over one chain's window, shared by the history reducers — part of libsmmhip (included by smmhip.hip inside its anonymous
// namespace ahead of the reducer headers, smm_stats.hpp with its k_stats_gather first; gfx950 device functions only).  A workgroup of
// WINDOW_WG lanes takes WINDOW_WG rows at a time, lane = row (an iteration of the window, or a member of a group in smm_trace.hpp), and
// answers "which history row does this lane contribute, and where does it go?" in one of two forms:
//
//   the rank form  (select 0 / 1) : block_rank: the lane's position among the selected lanes so far — a ballot per wave, the wave totals
//                                   through LDS, a running base advanced by the block's total.
//   the state form (select 2)     : state_walk: a(t), the last accepted row at or before row t (-1: none yet).  state_before finds
//                                   a(t0 - 1) by looking back from t0 as far as row 0, a block at a time (block_max of accepted ? row : -1,
//                                   stopping at the first block that holds one); state_scan then gives a block of the window its a(t):
//                                   the inclusive max-scan of accepted ? t : -1 across the lanes and the waves, on top of the carry from
//                                   the blocks before, which it advances.
//
// and the block reductions that go with them (block_max, block_sum, block_best).  Every thread of the workgroup calls these functions
// together: they hold barriers.  The LDS they are handed (WINDOW_WG / 64 entries per array) is free again when they return.
#pragma once

constexpr int WINDOW_WG = 256;   // (that every calling kernel's workgroup is this: the static_assert of smm_reducers_host.hpp)

__device__ __forceinline__ int block_max(int v, int* wred) {   // every lane gets the block's max of v
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    if (lane == 0) wred[w] = v;
    __syncthreads();
    int r = wred[0];
    for (int q = 1; q < WINDOW_WG / 64; ++q) r = max(r, wred[q]);
    __syncthreads();
    return r;
}

__device__ __forceinline__ int block_sum(int v, int* wred) {   // every lane gets the block's sum of v (wred may be in use on entry)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if (lane == 0) wred[w] = v;
    __syncthreads();
    int r = 0;
    for (int q = 0; q < WINDOW_WG / 64; ++q) r += wred[q];
    __syncthreads();
    return r;
}

// lane 0 of the block gets the block's best (bv, bi) by better(v, i, bv, bi) (the callers': stats_better, smm_stats.hpp); the other
// lanes' are left partly reduced
template <class Better>
__device__ __forceinline__ void block_best(double& bv, int& bi, double* wbv, int* wbi, Better better) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) { wbv[w] = bv; wbi[w] = bi; }
    __syncthreads();
    if (tid == 0)
        for (int q = 1; q < WINDOW_WG / 64; ++q)
            if (better(wbv[q], wbi[q], bv, bi)) { bv = wbv[q]; bi = wbi[q]; }
}

// the rank form, F flags in one barrier pair: pos[f] = base[f] + the lanes before this one whose flag f is set, and base[f] advanced by
// the block's count of them.  CLOSE = false leaves the second barrier to the caller, who passes one before wtot is written again.
template <int F, class T, bool CLOSE = true>
__device__ __forceinline__ void block_rank(const bool (&flag)[F], int (*wtot)[WINDOW_WG / 64], T (&base)[F], T (&pos)[F]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned long long ms[F];
    for (int f = 0; f < F; ++f) {
        ms[f] = __ballot(flag[f]);
        if (lane == 0) wtot[f][w] = __popcll(ms[f]);
    }
    __syncthreads();
    for (int f = 0; f < F; ++f) {
        T off = base[f];
        for (int q = 0; q < WINDOW_WG / 64; ++q) {
            if (q < w) off += wtot[f][q];
            base[f] += wtot[f][q];
        }
        pos[f] = off + __popcll(ms[f] & ((1ull << lane) - 1ull));
    }
    if (CLOSE) __syncthreads();
}
template <class T, bool CLOSE = true>
__device__ __forceinline__ T block_rank(bool flag, int* wtot, T& base) {   // one flag: returns its pos
    const bool f[1] = {flag};
    T b[1] = {base}, p[1];
    block_rank<1, T, CLOSE>(f, (int (*)[WINDOW_WG / 64])wtot, b, p);
    base = b[0];
    return p[0];
}

// a(t0 - 1) of chain c: every lane gets it
__device__ __forceinline__ int state_before(const double* __restrict__ hrec, int N, int HW, int c, int t0, int* wred) {
    int carry = -1;
    for (int r1 = t0; r1 > 0 && carry < 0; r1 -= WINDOW_WG) {
        const int r = r1 - WINDOW_WG + (int)threadIdx.x;
        carry = block_max((r >= 0 && hrec[((size_t)r * N + c) * HW + H_ACC] != 0.0) ? r : -1, wred);
    }
    return carry;
}

// one block of the window: a = this lane's row t where it is accepted, else -1 (a lane past the window: -1); returns the lane's a(t) and
// leaves in carry the a(t) of the block's last row
__device__ __forceinline__ int state_scan(int a, int& carry, int* wred) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int o = 1; o < 64; o <<= 1) {   // inclusive max-scan across the wave
        const int y = __shfl_up(a, o, 64);
        if (lane >= o) a = max(a, y);
    }
    if (lane == 63) wred[w] = a;
    __syncthreads();
    int pre = carry, all = carry;
    for (int q = 0; q < WINDOW_WG / 64; ++q) {
        if (q < w) pre = max(pre, wred[q]);
        all = max(all, wred[q]);
    }
    __syncthreads();
    carry = all;
    return max(a, pre);
}

// the state rows of chain c over the window [t0, t0 + n): emit(r, a, acc) for every window position r, from the lane that holds it, with
// a = a(t0 + r) and acc = whether row t0 + r itself is accepted.  ALSO >= 0: word ALSO of row t0 + r is loaded beside its H_ACC, ahead of
// the scan's barriers, and handed on as emit(r, a, acc, word).  emit runs on the window's lanes only: no barrier in it.
template <int ALSO = -1, class Emit>
__device__ __forceinline__ void state_walk(const double* __restrict__ hrec, int N, int HW, int c, int t0, int n, int* wred, Emit emit) {
    int carry = state_before(hrec, N, HW, c, t0, wred);
    for (int r0 = 0; r0 < n; r0 += WINDOW_WG) {
        const int r = r0 + (int)threadIdx.x, t = t0 + r;
        double acc_w = 0.0, also = 0.0;
        if (r < n) {   // (one guarded block: neighbouring words come in one load)
            const double* h = hrec + ((size_t)t * N + c) * HW;
            acc_w = h[H_ACC];
            if constexpr (ALSO >= 0) also = h[ALSO];
        }
        const bool acc = acc_w != 0.0;
        const int a = state_scan(acc ? t : -1, carry, wred);
        if (r >= n) continue;
        if constexpr (ALSO >= 0) emit(r, a, acc, also);
        else emit(r, a, acc);
    }
}
