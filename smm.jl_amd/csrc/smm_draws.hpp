// thinned posterior draws of groups of chains, exported row by row (smm_get_draws, include/smmhip.h) — part of libsmmhip (included by
// smmhip.hip inside its anonymous namespace after smm_rank.hpp; gfx950 device code).  Reads the history records hrec [T][N][HW]
// (smm_params.hpp: H_*) and nothing else; writes only the scratch and result buffers of the call.  Nothing is computed on a value: every
// double written is a record's double (or the quiet NaN of a state row that does not exist yet).  No list of the selected iterations is
// built: a chain's selection is a bit vector with a running popcount (rank / select), 12 bytes per 64 iterations.
//
//   k_draws_mask    : a tile of 64 chains per workgroup, lane = chain, so that the lanes of a load read the accepted flags of neighbouring
//                     records (HW doubles apart: the history is an array of records, a flag per record is the closest it gets to
//                     coalesced).  The tile's W words are split in four runs, one per wave; a thread builds each word of its run from 64
//                     flags, writes it and the count of set bits before it in the run, then adds the runs before its own (the totals
//                     through LDS).  Word w of a chain covers iterations tb + 64 w .. tb + 64 w + 63 below t1: tb = t0 for select 1 (the
//                     window), 0 for select 2 (the look-back reaches row 0).  Also writes m_c, the chain's set bits (select 1's count).
//   k_draws_offsets : one workgroup per group: the exclusive scan of the members' kept rows m'_c = ceil(m_c / thin) in chunks of the
//                     workgroup (a shuffle scan per wave, the wave totals through LDS, a 64-bit carry from chunk to chunk), then m_g and
//                     min(m_g, K).  The scan across groups that gives row0 is the host's, on the 16 bytes per group it downloads anyway.
//   k_draws_gather  : 256 output rows per workgroup.  First one row per lane: the row's group (binary search of row0), its pooled position
//                     (j, or floor(j m_g / K)), its member (binary search of the group's prefix), its rank in the chain's selection
//                     (times thin) and from the rank the iteration: t0 + i (select 0, 2), or the i-th set bit (a binary search of the
//                     running popcounts, then a descent by halves through the word); select 2 then walks back to the highest set bit
//                     at or below it.  The (chain, source row) pairs go to LDS.  Then the workgroup's threads copy the rows as (row,
//                     field) pairs, the fields consecutive across lanes: a record's parameters and moments are contiguous and so is a
//                     row of params [R][np] / sim_moments [R][nm], so the stores fill whole lines without a transpose.  The reads are
//                     one short run per distinct (iteration, chain) record: scattered by nature.
#pragma once

constexpr int DRAWS_WG = STATS_WG;   // lanes of every kernel; also the output rows of one k_draws_gather workgroup

// grid (ceil(nb / 64)).  Chains [c0, c0 + nb) of the N local ones; mask, pre [nb][W]; o_mc [N] (indexed by local chain)
__global__ __launch_bounds__(DRAWS_WG) void k_draws_mask(const double* __restrict__ hrec, int N, int HW, int tb, int t1, int c0, int nb, int W,
                                                         unsigned long long* __restrict__ mask, unsigned* __restrict__ pre,
                                                         int* __restrict__ o_mc) {
    __shared__ unsigned tot[DRAWS_WG / 64][64];
    const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
    const int cl = blockIdx.x * 64 + lane;
    const bool valid = cl < nb;
    const int Wq = (W + DRAWS_WG / 64 - 1) / (DRAWS_WG / 64), w0 = min(W, q * Wq), w1 = min(W, w0 + Wq);
    unsigned run = 0;
    if (valid) {
        const double* h = hrec + (size_t)(c0 + cl) * HW + H_ACC;
        for (int w = w0; w < w1; ++w) {
            const int ta = tb + 64 * w, nbit = min(64, t1 - ta);
            unsigned long long m = 0;
#pragma unroll 8
            for (int b = 0; b < nbit; ++b)
                if (h[(size_t)(ta + b) * N * HW] != 0.0) m |= 1ull << b;
            mask[(size_t)cl * W + w] = m;
            pre[(size_t)cl * W + w] = run;
            run += (unsigned)__popcll(m);
        }
    }
    tot[q][lane] = run;
    __syncthreads();
    unsigned base = 0, all = 0;
    for (int k = 0; k < DRAWS_WG / 64; ++k) {
        if (k < q) base += tot[k][lane];
        all += tot[k][lane];
    }
    if (!valid) return;
    if (base)
        for (int w = w0; w < w1; ++w) pre[(size_t)cl * W + w] += base;
    if (q == 0) o_mc[c0 + cl] = (int)all;
}

// grid (G).  mc [N]: the chains' selected rows (NULL: n each); prefix [M] (by position in mem), gm, take [G]
__global__ __launch_bounds__(DRAWS_WG) void k_draws_offsets(const int* __restrict__ mem, const int* __restrict__ gmem0, const int* __restrict__ mc,
                                                            int n, int thin, long long K, long long* __restrict__ prefix,
                                                            long long* __restrict__ gm, long long* __restrict__ take) {
    __shared__ long long wtot[DRAWS_WG / 64];
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int m0 = gmem0[g], mg = gmem0[g + 1] - m0;
    long long carry = 0;
    for (int j0 = 0; j0 < mg; j0 += DRAWS_WG) {
        const int j = j0 + tid;
        long long v = 0;
        if (j < mg) {
            const long long m = mc ? mc[mem[m0 + j]] : n;
            v = (m + thin - 1) / thin;
        }
        long long s = v;   // inclusive scan across the wave
        for (int o = 1; o < 64; o <<= 1) {
            const long long y = __shfl_up(s, o, 64);
            if (lane >= o) s += y;
        }
        if (lane == 63) wtot[w] = s;
        __syncthreads();
        long long before = carry, all = carry;
        for (int k = 0; k < DRAWS_WG / 64; ++k) {
            if (k < w) before += wtot[k];
            all += wtot[k];
        }
        __syncthreads();
        if (j < mg) prefix[m0 + j] = before + s - v;
        carry = all;
    }
    if (tid == 0) {
        gm[g] = carry;
        take[g] = carry < K ? carry : K;
    }
}

// the position of the r-th set bit of x (r < popcount(x)), by halves
__device__ __forceinline__ int draws_select_bit(unsigned long long x, int r) {
    int pos = 0;
    for (int s = 32; s > 0; s >>= 1) {
        const int cnt = __popcll(x & ((1ull << s) - 1ull));
        if (r >= cnt) { r -= cnt; x >>= s; pos += s; }
    }
    return pos;
}

// grid (ceil(rn / DRAWS_WG)).  Output rows [r0, r0 + rn) of the call, written at [0, rn) of the batch's arrays (any may be NULL); only rows
// of the chains [c0, c0 + nb), whose masks (tb as in k_draws_mask) the scratch holds.  row0 [G + 1], prefix [M], gm [G] as above
__global__ __launch_bounds__(DRAWS_WG) void k_draws_gather(const double* __restrict__ hrec, int N, int HW, int np, int nm, int t0, int sel,
                                                           int thin, const int* __restrict__ mem, const int* __restrict__ gmem0, int G,
                                                           const long long* __restrict__ row0, const long long* __restrict__ prefix,
                                                           const long long* __restrict__ gm, int c0, int nb, int W, int tb,
                                                           const unsigned long long* __restrict__ mask, const unsigned* __restrict__ pre,
                                                           int chain0, long long r0, int rn, double* __restrict__ o_params,
                                                           double* __restrict__ o_value, double* __restrict__ o_mom, int* __restrict__ o_chain,
                                                           int* __restrict__ o_iter, int* __restrict__ o_src) {
    __shared__ int s_chain[DRAWS_WG], s_src[DRAWS_WG];   // the block's rows: local chain (-1: not of this batch), source row (-1: none)
    const int tid = threadIdx.x, b0 = blockIdx.x * DRAWS_WG, rl = b0 + tid;
    int c = -1, src = -1;
    if (rl < rn) {
        const long long q = r0 + rl;
        int a = 0, b = G;   // the last g with row0[g] <= q: its rows hold q, the empty groups before it skipped
        while (b - a > 1) {
            const int m = (a + b) >> 1;
            if (row0[m] <= q) a = m;
            else b = m;
        }
        const int g = a;
        const long long j = q - row0[g], K = row0[g + 1] - row0[g], m = gm[g];
        const long long p = m <= K ? j : (j * m) / K;
        const int m0 = gmem0[g];
        a = 0, b = gmem0[g + 1] - m0;   // the last member with prefix <= p: the one whose kept rows hold p
        while (b - a > 1) {
            const int k = (a + b) >> 1;
            if (prefix[m0 + k] <= p) a = k;
            else b = k;
        }
        const int cc = mem[m0 + a];
        if (sel == 0 || (cc >= c0 && cc < c0 + nb)) {
            c = cc;
            const long long i = (p - prefix[m0 + a]) * thin;   // the rank in the chain's selection: below m_c <= n
            int t;
            if (sel != 1) {
                t = t0 + (int)i;
                src = t;
            } else {
                const unsigned* pr = pre + (size_t)(c - c0) * W;
                int wa = 0, wb = W;   // the last word with pre <= i (a word without a set bit is never the last)
                while (wb - wa > 1) {
                    const int k = (wa + wb) >> 1;
                    if ((long long)pr[k] <= i) wa = k;
                    else wb = k;
                }
                t = tb + 64 * wa + draws_select_bit(mask[(size_t)(c - c0) * W + wa], (int)(i - pr[wa]));
                src = t;
            }
            if (sel == 2) {   // a(t): the highest set bit at or below t, back over the words without one (tb == 0)
                const unsigned long long* mk = mask + (size_t)(c - c0) * W;
                int wi = t >> 6;
                const int bit = t & 63;
                unsigned long long x = mk[wi] & (bit == 63 ? ~0ull : (1ull << (bit + 1)) - 1ull);
                while (x == 0 && wi > 0) x = mk[--wi];
                src = x ? 64 * wi + 63 - __clzll((long long)x) : -1;
            }
            if (o_chain) o_chain[rl] = chain0 + c + 1;
            if (o_iter) o_iter[rl] = t + 1;
            if (o_src) o_src[rl] = src + 1;
        }
    }
    s_chain[tid] = c;
    s_src[tid] = src;
    __syncthreads();
    const int rows = min(DRAWS_WG, rn - b0), F = np + nm + 1;   // a row's fields: the parameters, the moments, the value
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    for (int e = tid; e < rows * F; e += DRAWS_WG) {
        const int r = e / F, f = e - r * F;
        const int rc = s_chain[r], rs = s_src[r];
        if (rc < 0) continue;
        double* o = f < np ? o_params : f < np + nm ? o_mom : o_value;
        if (!o) continue;
        const int field = f < np + nm ? H_PARAMS + f : H_VALUE;
        const double v = rs < 0 ? qnan : hrec[((size_t)rs * N + rc) * HW + field];
        const size_t at = f < np ? (size_t)(b0 + r) * np + f : f < np + nm ? (size_t)(b0 + r) * nm + (f - np) : (size_t)(b0 + r);
        o[at] = v;
    }
}
