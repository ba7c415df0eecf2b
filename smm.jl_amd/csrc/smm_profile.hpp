// the objective and the simulated moments binned along parameters (smm_get_profile, include/smmhip.h) — part of libsmmhip (included by
// smmhip.hip inside its anonymous namespace after smm_hist.hpp; gfx950 device code).  Reads the history records hrec [T][N][HW]
// (smm_params.hpp: H_*) and nothing else; writes only the scratch and the result buffer of the call.  An *axis* is a parameter (1-D,
// nseg = bins segments) or a pair (2-D, nseg = bins2 bins2 cells); a batch is the members of some groups x some axes.  Counts and minima
// are integers reduced with integer atomics, so they do not depend on the order of additions; the means do, so every segment's scored
// rows are compacted in pooled order first and reduced by the chunked pairwise core (stats_pw) afterwards.
//
//   k_prof_rows    : one workgroup per member chain, once per batch of groups: hist_rows' selection written out, tab [mb][n] = the
//                    history row a pooled row reads (-1: a NaN row of the state series, -2: not selected) and val [mb][n] = its value.
//   k_prof_count   : one workgroup per (member, axis): the bin (hist_bin) or cell (hist_axis twice) of every pooled row, kept in code
//                    [an][mb][n] (-1 none, else 2 seg + scored); u32 counters [2][nseg] in LDS (rows, scored rows), flushed to the
//                    segment's u64 count (one atomic per non-zero segment) and to the member's row of table [an][mb][nseg]; past
//                    PROF_LDS_SEGS segments the lanes add into both directly.  The smallest order key of a scored value per segment:
//                    a 64-bit atomicMin, skipped where the key read back is already smaller.
//   k_prof_scan    : one thread per segment: the exclusive prefix of table over the group's members (the member's first slot inside the
//                    segment) and the segment's scored count.
//   k_prof_scatter : one workgroup per (member, axis), 256 rows at a time in iteration order: a scored row's slot = the segment's start +
//                    the member's prefix + its rank among the member's rows of the segment (a running cursor per segment, in LDS or in
//                    the member's table row, + the rank inside the block from the block's keys in LDS); list [an][mb n] gets the pooled
//                    position.  The rows whose key equals the segment's minimum reduce their pooled position with a 32-bit atomicMin:
//                    the earliest row wins.
//   k_prof_chunk   : one workgroup per (chunk of <= 8192 slots of a segment, column): the value (from val) or one simulated moment
//                    (gathered from the record, lane = row) staged in LDS, then stats_pw.
//   k_prof_finish  : one thread per segment: the chunk sums added in order and divided; the winning row's value, ids and parameters.
#pragma once

constexpr int PROF_WG = HIST_WG;
constexpr int PROF_LDS_SEGS = 4096;   // segments counted in LDS: 2 x 4 bytes each (k_prof_count), 4 bytes (k_prof_scatter)

struct ProfBatch {
    const double* hrec; int N, HW, np, nm, t0, n, offset;
    const int* mem; const int* gmem0; const int* gid; int m0, mb, g0, gn;
    int two, a0, an, nseg, B, lds;             // B: bins (1-D) or bins2 (2-D)
    const int* pairs; const int* st; const double* lo; const double* hi; const double* edges;   // edges [gn][np][B + 1] of the batch
    int* tab; double* val; int* code; unsigned* table; unsigned* list;
    unsigned long long* cnt; unsigned long long* nsc; unsigned long long* minkey; unsigned* minpos;
    const unsigned* segstart; const int* segch0; const unsigned long long* cst; const int* clen; double* csum; int ncol;
    double* vmin; int* chain; int* iter; double* theta; double* vmean; double* mmean;
};

// the order key of a scored value: -0 and +0 the same key
__device__ __forceinline__ unsigned long long prof_key(double v) { return stats_key(v == 0.0 ? 0.0 : v); }

// grid (members of the batch)
__global__ __launch_bounds__(PROF_WG) void k_prof_rows(const double* __restrict__ hrec, int N, int HW, int t0, int n, int sel,
                                                       const int* __restrict__ mem, int m0, int* __restrict__ tab, double* __restrict__ val) {
    __shared__ int rows[HIST_WG];
    __shared__ int wred[HIST_WG / 64];
    const int mi = blockIdx.x, c = mem[m0 + mi], tid = threadIdx.x;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    int r0 = 0;
    hist_rows(hrec, N, HW, c, t0, n, sel, rows, wred, [&](int nb) {
        if (tid < nb) {
            const int src = rows[tid];
            const size_t pos = (size_t)mi * n + r0 + tid;
            tab[pos] = src;
            val[pos] = src >= 0 ? hrec[((size_t)src * N + c) * HW + H_VALUE] : qnan;
        }
        r0 += HIST_WG;
    });
}

// grid (members of the batch, axes of the batch); dynamic LDS 8 nseg bytes with b.lds.  cnt zeroed, minkey all ones, table zeroed
// without b.lds
__global__ __launch_bounds__(PROF_WG) void k_prof_count(const ProfBatch b) {
    extern __shared__ __align__(16) unsigned prof_lds[];   // [nseg] rows, then [nseg] scored rows
    const int mi = blockIdx.x, al = blockIdx.y, a = b.a0 + al, tid = threadIdx.x;
    const int c = b.mem[b.m0 + mi], gl = b.gid[c] - b.g0, n = b.n, nseg = b.nseg, B = b.B;
    const size_t sb = ((size_t)gl * b.an + al) * nseg;
    unsigned* trow = b.table + ((size_t)al * b.mb + mi) * nseg;
    int* code = b.code + (size_t)al * b.mb * n + (size_t)mi * n;
    unsigned *cn = prof_lds, *cs = prof_lds + nseg;
    const size_t at = (size_t)(b.g0 + gl) * b.np;
    int ka, kb = 0;
    bool ok;
    if (!b.two) { ka = a; ok = b.st[at + ka] == 0; }
    else {
        ka = b.pairs[2 * a]; kb = b.pairs[2 * a + 1];
        ok = (b.st[at + ka] == 0 || b.st[at + ka] == 3) && (b.st[at + kb] == 0 || b.st[at + kb] == 3);
    }
    const double lo = b.lo[at + ka], delta = b.hi[at + ka] - lo;
    const double* ea = b.edges + ((size_t)gl * b.np + ka) * (B + 1);
    const double* eb = b.edges + ((size_t)gl * b.np + kb) * (B + 1);
    if (b.lds) {
        for (int i = tid; i < 2 * nseg; i += PROF_WG) prof_lds[i] = 0u;
        __syncthreads();
    }
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    for (int r = tid; r < n; r += PROF_WG) {
        const size_t pos = (size_t)mi * n + r;
        const int src = b.tab[pos];
        int s = -1;
        if (ok && src != -2) {
            const double* h = src >= 0 ? b.hrec + ((size_t)src * b.N + c) * b.HW + H_PARAMS : nullptr;
            if (!b.two) s = hist_bin(h ? h[ka] : qnan, lo, delta, B, ea);
            else if (h) {
                const int i = hist_axis(h[ka], ea, B);
                const int j = i >= 0 ? hist_axis(h[kb], eb, B) : -1;
                if (j >= 0) s = i * B + j;
            }
        }
        int cd = -1;
        if (s >= 0) {
            const double v = b.val[pos];
            const int sc = hist_finite(v);
            cd = 2 * s + sc;
            if (b.lds) {
                atomicAdd(&cn[s], 1u);
                if (sc) atomicAdd(&cs[s], 1u);
            } else {
                atomicAdd(&b.cnt[sb + s], 1ull);
                if (sc) atomicAdd(&trow[s], 1u);
            }
            if (sc) {
                const unsigned long long key = prof_key(v);
                if (key < b.minkey[sb + s]) atomicMin(&b.minkey[sb + s], key);
            }
        }
        code[r] = cd;
    }
    if (!b.lds) return;
    __syncthreads();
    for (int i = tid; i < nseg; i += PROF_WG) {
        const unsigned v = cn[i];
        if (v) atomicAdd(&b.cnt[sb + i], (unsigned long long)v);
        trow[i] = cs[i];
    }
}

// one thread per segment of the batch
__global__ __launch_bounds__(256) void k_prof_scan(const ProfBatch b) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)b.gn * b.an * b.nseg) return;
    const int seg = (int)(e % b.nseg), al = (int)((e / b.nseg) % b.an), gl = (int)(e / ((long long)b.nseg * b.an));
    const int i0 = b.gmem0[b.g0 + gl] - b.m0, i1 = b.gmem0[b.g0 + gl + 1] - b.m0;
    unsigned long long run = 0;
    for (int mi = i0; mi < i1; ++mi) {
        unsigned* p = b.table + ((size_t)al * b.mb + mi) * b.nseg + seg;
        const unsigned v = *p;
        *p = (unsigned)run;
        run += v;
    }
    b.nsc[e] = run;
}

// grid (members of the batch, axes of the batch); dynamic LDS 4 nseg bytes with b.lds.  want_list == 0: the minima's positions only
__global__ __launch_bounds__(PROF_WG) void k_prof_scatter(const ProfBatch b, int want_list) {
    extern __shared__ __align__(16) unsigned prof_lds[];   // [nseg] the member's next slot in every segment
    __shared__ int sk[PROF_WG];
    const int mi = blockIdx.x, al = blockIdx.y, tid = threadIdx.x;
    const int c = b.mem[b.m0 + mi], gl = b.gid[c] - b.g0, n = b.n, nseg = b.nseg;
    const size_t sb = ((size_t)gl * b.an + al) * nseg;
    unsigned* trow = b.table + ((size_t)al * b.mb + mi) * nseg;
    const int* code = b.code + (size_t)al * b.mb * n + (size_t)mi * n;
    unsigned* list = b.list + (size_t)al * b.mb * n;
    unsigned* cur = b.lds ? prof_lds : trow;
    if (want_list) {
        for (int i = tid; i < nseg; i += PROF_WG) cur[i] = b.segstart[sb + i] + trow[i];
        __syncthreads();
    }
    for (int r0 = 0; r0 < n; r0 += PROF_WG) {
        const int r = r0 + tid;
        const int cd = r < n ? code[r] : -1;
        const bool sc = cd >= 0 && (cd & 1);
        const int s = sc ? cd >> 1 : -1;
        const unsigned pos = (unsigned)((size_t)mi * n + r);
        if (sc && prof_key(b.val[pos]) == b.minkey[sb + s] && pos < b.minpos[sb + s]) atomicMin(&b.minpos[sb + s], pos);
        if (!want_list) continue;
        sk[tid] = s;
        __syncthreads();
        int before = 0, after = 0;
        unsigned dest = 0;
        if (sc) {
            for (int j = 0; j < PROF_WG; ++j) {
                const int same = sk[j] == s;
                before += same & (j < tid);
                after |= same & (j > tid);
            }
            dest = cur[s] + (unsigned)before;
            list[dest] = pos;
        }
        __syncthreads();
        if (sc && !after) cur[s] = dest + 1u;   // the segment's last row of the block moves the cursor
        __syncthreads();
    }
}

// grid (chunks, columns); dynamic LDS 8 x the longest chunk
__global__ __launch_bounds__(STATS_WG) void k_prof_chunk(const ProfBatch b) {
    extern __shared__ __align__(16) double prof_sx[];
    __shared__ PwTree pt;
    const int ch = blockIdx.x, col = blockIdx.y, tid = threadIdx.x, len = b.clen[ch];
    const unsigned* L = b.list + b.cst[ch];
    for (int i = tid; i < len; i += STATS_WG) {
        const unsigned pos = L[i];
        double x;
        if (col == 0) x = b.val[pos];
        else {
            const int c = b.mem[b.m0 + (int)(pos / (unsigned)b.n)];
            x = b.hrec[((size_t)b.tab[pos] * b.N + c) * b.HW + H_PARAMS + b.np + col - 1];
        }
        prof_sx[i] = x;
    }
    __syncthreads();
    const double s = stats_pw(prof_sx, len, pt);
    if (tid == 0) b.csum[(size_t)ch * b.ncol + col] = s;
}

// one thread per segment of the batch; any output NULL: not written
__global__ __launch_bounds__(256) void k_prof_finish(const ProfBatch b) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)b.gn * b.an * b.nseg) return;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    const unsigned long long m = b.nsc[e];
    if (b.vmin || b.chain || b.iter || b.theta) {
        double v = qnan;
        int ch = 0, it = 0;
        const double* h = nullptr;
        if (m > 0) {
            const unsigned pos = b.minpos[e];
            const int mi = (int)(pos / (unsigned)b.n), r = (int)(pos - (unsigned)mi * (unsigned)b.n), c = b.mem[b.m0 + mi];
            v = b.val[pos];
            ch = b.offset + c + 1;
            it = b.t0 + r + 1;
            h = b.hrec + ((size_t)b.tab[pos] * b.N + c) * b.HW + H_PARAMS;
        }
        if (b.vmin) b.vmin[e] = v;
        if (b.chain) b.chain[e] = ch;
        if (b.iter) b.iter[e] = it;
        if (b.theta)
            for (int k = 0; k < b.np; ++k) b.theta[e * b.np + k] = h ? h[k] : qnan;
    }
    if (!b.vmean && !b.mmean) return;
    for (int col = 0; col < b.ncol; ++col) {
        double S = 0.0;
        for (int ch = b.segch0[e]; ch < b.segch0[e + 1]; ++ch) S = S + b.csum[(size_t)ch * b.ncol + col];
        const double mu = m == 0 ? qnan : S / (double)m;
        if (col == 0) { if (b.vmean) b.vmean[e] = mu; }
        else if (b.mmean) b.mmean[e * b.nm + col - 1] = mu;
    }
}
