// user objectives: their registration and their persistent forms, compiled with hiprtc (loaded lazily, the library does not link against
// it) — part of libsmmhip (included once by smmhip.hip, ahead of smm_forms_host.hpp; hiprtc never sees it).  What is stated here once:
// the way through hiprtc (rtc_compile), the texts around a user's source (the preludes, the evaluation kernels and the map-reduce
// reduction they share), the device headers a persistent form is made of (PERSIST_HEADERS and each form's tail), one record per
// persistent form (UserCode, by UserForm), which of them a context wants (user_form_wanted) and how it is compiled (user_form_compile).
// User transforms (smm_register_user_transform: functions of one history row for smm_get_derived) are registered here too, in a
// registry of their own, with the text of the kernel that runs them (USER_KERNEL_TRANSFORM; launched by smm_reducers_host.hpp).
#pragma once

namespace {

// the persistent kernels with a user's objective inside: k_chain_persist_gen (one thread per chain: smm_chain_persist_gen.hpp, SMM_GEN_USER),
// k_chain_persist_tile with the map-reduce form (smm_chain_persist_tile.hpp, SMM_TILE_USER), its form for a SHARD (SMM_TILE_SH as well) and
// its form for proposals with a Cholesky factor (SMM_TILE_CHOL as well; never a shard's): each compiled only when a context first wants it
enum UserForm { UF_GEN, UF_TILE, UF_TILE_SHARD, UF_TILE_CHOL, UF_COUNT };
struct UserCode {
    std::vector<char> code;
    int state = 0;     // 0: not tried yet, 1: code stands, -1: not available (log says why)
    std::string log;
};
struct UserObjective {
    std::vector<char> code; int lanes = 0; /* 0: one thread per chain; else lanes per chain (map-reduce form) */
    std::string source;                    // the user's text: compiled once more INTO the persistent kernels on demand
    int n_sums = 1;                        // map-reduce form: partial sums per lane
    bool rng = false;                      // SMM_USER_OBJECTIVE_RNG / SMM_USER_PARTIAL_RNG: takes the library's stream (smm_register_user_objective_rng)
    UserCode form[UF_COUNT];
};
// the device headers the persistent kernels are made of, as text: hiprtc compiles them together with the user's source
struct EmbeddedSource { const char* name; const char* text; };
const EmbeddedSource g_embedded[] = {
#include "smm_embedded.inc"
};
std::vector<UserObjective> g_user_objectives;
std::mutex g_user_mutex;

const char* USER_PRELUDE =
    "#define SMM_USER_OBJECTIVE extern \"C\" __device__ void smm_user_objective\n"
    "extern \"C\" __device__ void smm_user_objective(const double* theta, int np, const double* mom, const double* w, int nm,\n"
    "                                              const double* udata, int n_udata, double* sim_moments, double* value, int* status);\n";
// (the same declaration as the persistent gen form has always been given it, its last line indented otherwise: the code hiprtc returns for
// that form changes with the indentation — same size, other bytes —, and a refactor holds every form's code byte for byte)
const char* USER_PRELUDE_GEN =
    "#define SMM_USER_OBJECTIVE extern \"C\" __device__ void smm_user_objective\n"
    "extern \"C\" __device__ void smm_user_objective(const double* theta, int np, const double* mom, const double* w, int nm,\n"
    "        const double* udata, int n_udata, double* sim_moments, double* value, int* status);\n";
const char* USER_KERNEL =
    "\nextern \"C\" __global__ void smm_user_eval_kernel(const double* theta, int N, int np, const double* mom, const double* w, int nm,\n"
    "        const double* udata, int n_udata, double* simM, double* value, int* status) {\n"
    "    const int c = blockIdx.x * blockDim.x + threadIdx.x;\n"
    "    if (c >= N) return;\n"
    "    int st = 1; double v = 0.0;\n"
    "    smm_user_objective(theta + (size_t)c * np, np, mom, w, nm, udata, n_udata, simM + (size_t)c * nm, &v, &st);\n"
    "    value[c] = v; status[c] = st;\n"
    "}\n";

const char* USER_PRELUDE_LANES =
    "#define SMM_USER_PARTIAL extern \"C\" __device__ void smm_user_partial\n"
    "#define SMM_USER_FINISH extern \"C\" __device__ void smm_user_finish\n"
    "extern \"C\" __device__ void smm_user_partial(const double* theta, int np, const double* udata, int n_udata, int lane, int n_lanes,\n"
    "                                            double* partial);\n"
    "extern \"C\" __device__ void smm_user_finish(const double* theta, int np, const double* totals, int n_sums, const double* mom,\n"
    "                                           const double* w, int nm, const double* udata, int n_udata, double* sim_moments,\n"
    "                                           double* value, int* status);\n";
// the map-reduce kernels' reduction of the lanes' partial sums (part) and what follows it, the text both of them end with.  Its numerical
// contract: inside a wave the 64 partials are combined by the halving tree (offsets 32,16,...,1), the wave totals are added left to right.
#define USER_REDUCE_LANES \
    "    for (int i = 0; i < SMM_NSUMS; ++i) {\n" \
    "        double a = part[i];\n" \
    "        for (int off = 32; off >= 1; off >>= 1) a = a + __shfl_xor(a, off, 64);\n" \
    "        if ((lane & 63) == 0) wsum[lane >> 6][i] = a;\n" \
    "    }\n" \
    "    __syncthreads();\n" \
    "    if (lane == 0) {\n" \
    "        double tot[SMM_NSUMS];\n" \
    "        for (int i = 0; i < SMM_NSUMS; ++i) { double a = wsum[0][i]; for (int wv = 1; wv < nl / 64; ++wv) a = a + wsum[wv][i]; tot[i] = a; }\n" \
    "        int st = 1; double v = 0.0;\n" \
    "        smm_user_finish(theta + (size_t)c * np, np, tot, SMM_NSUMS, mom, w, nm, udata, n_udata, simM + (size_t)c * nm, &v, &st);\n" \
    "        value[c] = v; status[c] = st;\n" \
    "    }\n" \
    "}\n"
// one workgroup of n_lanes threads per evaluation
const char* USER_KERNEL_LANES =
    "\nextern \"C\" __global__ void smm_user_eval_kernel(const double* theta, int N, int np, const double* mom, const double* w, int nm,\n"
    "        const double* udata, int n_udata, double* simM, double* value, int* status) {\n"
    "    __shared__ double wsum[16][SMM_NSUMS];\n"
    "    const int c = blockIdx.x, lane = threadIdx.x, nl = blockDim.x;\n"
    "    double part[SMM_NSUMS];\n"
    "    for (int i = 0; i < SMM_NSUMS; ++i) part[i] = 0.0;\n"
    "    smm_user_partial(theta + (size_t)c * np, np, udata, n_udata, lane, nl, part);\n"
    USER_REDUCE_LANES;

// user objectives that draw from the library's generator (smm_register_user_objective_rng): the stream handle and its draws
// (include/smmhip.h), on smm_rng.hpp's Philox4x32-10 and Box-Muller — compiled with the library's own headers (g_embedded)
const char* USER_RNG_API =
    "#include <stdint.h>\n#include \"smm_rng.hpp\"\n"
    "typedef struct { uint64_t seed; } smm_rng_t;\n"
    "__device__ inline double smm_uniform(smm_rng_t r, uint64_t i) { return smm::user_uniform(r.seed, i); }\n"
    "__device__ inline void smm_normal2(smm_rng_t r, uint64_t j, double* z0, double* z1) { smm::user_normal2(r.seed, j, *z0, *z1); }\n"
    "__device__ inline double smm_normal(smm_rng_t r, uint64_t i) {\n"
    "    double z0, z1;\n"
    "    smm::user_normal2(r.seed, i >> 1, z0, z1);\n"
    "    return (i & 1) ? z1 : z0;\n"
    "}\n";
const char* USER_PRELUDE_RNG =
    "#define SMM_USER_OBJECTIVE_RNG extern \"C\" __device__ void smm_user_objective_rng\n"
    "extern \"C\" __device__ void smm_user_objective_rng(const double* theta, int np, const double* mom, const double* w, int nm,\n"
    "                                                  const double* udata, int n_udata, smm_rng_t rng, double* sim_moments,\n"
    "                                                  double* value, int* status);\n";
// two kernels: keyed by the context's seed (BGP steps, smm_eval_batch), and evaluation c keyed by base_seed + c (smm_eval_batch_noseed)
const char* USER_KERNEL_RNG =
    "\n__device__ inline void smm_user_eval_one(const double* theta, int c, int np, const double* mom, const double* w, int nm,\n"
    "        const double* udata, int n_udata, double* simM, double* value, int* status, uint64_t seed) {\n"
    "    int st = 1; double v = 0.0;\n"
    "    smm_user_objective_rng(theta + (size_t)c * np, np, mom, w, nm, udata, n_udata, smm_rng_t{seed}, simM + (size_t)c * nm, &v, &st);\n"
    "    value[c] = v; status[c] = st;\n"
    "}\n"
    "extern \"C\" __global__ void smm_user_eval_kernel(const double* theta, int N, int np, const double* mom, const double* w, int nm,\n"
    "        const double* udata, int n_udata, double* simM, double* value, int* status, uint64_t seed) {\n"
    "    const int c = blockIdx.x * blockDim.x + threadIdx.x;\n"
    "    if (c < N) smm_user_eval_one(theta, c, np, mom, w, nm, udata, n_udata, simM, value, status, seed);\n"
    "}\n"
    "extern \"C\" __global__ void smm_user_eval_noseed_kernel(const double* theta, int N, int np, const double* mom, const double* w, int nm,\n"
    "        const double* udata, int n_udata, double* simM, double* value, int* status, uint64_t base_seed) {\n"
    "    const int c = blockIdx.x * blockDim.x + threadIdx.x;\n"
    "    if (c < N) smm_user_eval_one(theta, c, np, mom, w, nm, udata, n_udata, simM, value, status, base_seed + (uint64_t)c);\n"
    "}\n";

const char* USER_PRELUDE_LANES_RNG =
    "#define SMM_USER_PARTIAL_RNG extern \"C\" __device__ void smm_user_partial_rng\n"
    "#define SMM_USER_FINISH extern \"C\" __device__ void smm_user_finish\n"
    "extern \"C\" __device__ void smm_user_partial_rng(const double* theta, int np, const double* udata, int n_udata, smm_rng_t rng,\n"
    "                                                int lane, int n_lanes, double* partial);\n"
    "extern \"C\" __device__ void smm_user_finish(const double* theta, int np, const double* totals, int n_sums, const double* mom,\n"
    "                                           const double* w, int nm, const double* udata, int n_udata, double* sim_moments,\n"
    "                                           double* value, int* status);\n";
// the map-reduce kernel of USER_KERNEL_LANES with the stream handle passed to the partial sums: the same reduction
const char* USER_KERNEL_LANES_RNG =
    "\n__device__ inline void smm_user_eval_lanes(const double* theta, int c, int np, const double* mom, const double* w, int nm,\n"
    "        const double* udata, int n_udata, double* simM, double* value, int* status, uint64_t seed) {\n"
    "    __shared__ double wsum[16][SMM_NSUMS];\n"
    "    const int lane = threadIdx.x, nl = blockDim.x;\n"
    "    double part[SMM_NSUMS];\n"
    "    for (int i = 0; i < SMM_NSUMS; ++i) part[i] = 0.0;\n"
    "    smm_user_partial_rng(theta + (size_t)c * np, np, udata, n_udata, smm_rng_t{seed}, lane, nl, part);\n"
    USER_REDUCE_LANES
    "extern \"C\" __global__ void smm_user_eval_kernel(const double* theta, int N, int np, const double* mom, const double* w, int nm,\n"
    "        const double* udata, int n_udata, double* simM, double* value, int* status, uint64_t seed) {\n"
    "    smm_user_eval_lanes(theta, blockIdx.x, np, mom, w, nm, udata, n_udata, simM, value, status, seed);\n"
    "}\n"
    "extern \"C\" __global__ void smm_user_eval_noseed_kernel(const double* theta, int N, int np, const double* mom, const double* w, int nm,\n"
    "        const double* udata, int n_udata, double* simM, double* value, int* status, uint64_t base_seed) {\n"
    "    smm_user_eval_lanes(theta, blockIdx.x, np, mom, w, nm, udata, n_udata, simM, value, status, base_seed + (uint64_t)blockIdx.x);\n"
    "}\n";
#undef USER_REDUCE_LANES

// user transforms (smm_register_user_transform, smm_get_derived): a function of one history row, with the contract's exponential and
// logarithm at global scope — compiled with the library's own headers (g_embedded)
struct UserTransform { std::vector<char> code; int n_out = 0; };
std::vector<UserTransform> g_user_transforms;   // (handle = index: a range of its own, not the objectives')
const char* USER_PRELUDE_TRANSFORM =
    "#include <stdint.h>\n#include \"smm_rng.hpp\"\n"
    "__device__ inline double smm_exp(double x) { return smm::smm_exp(x); }\n"
    "__device__ inline double smm_log(double x) { return smm::smm_log(x); }\n"
    "#define SMM_USER_TRANSFORM extern \"C\" __device__ void smm_user_transform\n"
    "extern \"C\" __device__ void smm_user_transform(const double* theta, int np, const double* sim_moments, int nm, double value,\n"
    "                                              const double* mom, const double* w, const double* udata, int n_udata,\n"
    "                                              const double* tdata, int n_tdata, double* out, int n_out);\n";
// The rows of a batch through the user's function (SMM_NOUT = n_out, SMM_H_PARAMS / SMM_H_VALUE = the record's H_PARAMS / H_VALUE).
// Workgroup (blockIdx.x, blockIdx.y) takes rows [R blockIdx.x, R blockIdx.x + R) of chunk cb0 + blockIdx.y (clen rows from pooled row
// cst, all of group cgrp); ridx [pooled row - p0] is a row's index in hrec, -1: none (every output stays NaN).  The rows are read two
// words per lane, consecutive lanes consecutive words, and staged in LDS at a stride of HW + 1 doubles (HW is even: odd, so that the
// lanes' reads of one word of their own rows fall into different banks), the R row indexes behind them; then one lane per row.
// Packed form (chunked == 0): outputs [q0, q0 + qb) to col [qb][cstride] at the pooled row, and the rows that are not finite counted
// into nnf [G][SMM_NOUT] (a wave's count by its first active lane).  Chunked form: every output, centred by its group's mean gmean
// [G][SMM_NOUT], to col [SMM_NOUT][nbc][cstride] at (chunk - cb0, row in chunk), as k_group_gather's chunked form lays them out.
const char* USER_KERNEL_TRANSFORM =
    "\nextern \"C\" __global__ __launch_bounds__(256) void smm_user_transform_kernel(const double* __restrict__ hrec, int HW, int np, int nm,\n"
    "        const long long* __restrict__ ridx, long long p0, const long long* __restrict__ cst, const int* __restrict__ clen,\n"
    "        const int* __restrict__ cgrp, int cb0, int R, const double* mom, const double* w, const double* udata, int n_udata,\n"
    "        const double* tdata, int n_tdata, int q0, int qb, long long cstride, int chunked, int nbc, const double* __restrict__ gmean,\n"
    "        double* __restrict__ col, unsigned long long* __restrict__ nnf) {\n"
    "    extern __shared__ double smm_rows[];\n"
    "    const int ch = cb0 + (int)blockIdx.y, tid = (int)threadIdx.x, i0 = (int)blockIdx.x * R, len = clen[ch];\n"
    "    if (i0 >= len) return;\n"
    "    const int nr = min(R, len - i0), S = HW + 1, h2 = HW >> 1;\n"
    "    const long long pos0 = cst[ch] + i0;\n"
    "    long long* rix = (long long*)(smm_rows + (size_t)R * S);\n"
    "    for (int r = tid; r < nr; r += 256) rix[r] = ridx[pos0 - p0 + r];\n"
    "    __syncthreads();\n"
    "    for (int e = tid; e < nr * h2; e += 256) {\n"
    "        const int r = e / h2, j = e - r * h2;\n"
    "        const long long ri = rix[r];\n"
    "        if (ri < 0) continue;\n"
    "        const double2 v = ((const double2*)(hrec + (size_t)ri * HW))[j];\n"
    "        smm_rows[r * S + 2 * j] = v.x;\n"
    "        smm_rows[r * S + 2 * j + 1] = v.y;\n"
    "    }\n"
    "    __syncthreads();\n"
    "    if (tid >= nr) return;\n"
    "    double out[SMM_NOUT];\n"
    "#pragma unroll\n"
    "    for (int q = 0; q < SMM_NOUT; ++q) out[q] = __longlong_as_double(0x7ff8000000000000ll);\n"
    "    const double* row = smm_rows + tid * S;\n"
    "    if (rix[tid] >= 0)\n"
    "        smm_user_transform(row + SMM_H_PARAMS, np, row + SMM_H_PARAMS + np, nm, row[SMM_H_VALUE], mom, w, udata, n_udata, tdata, n_tdata,\n"
    "                           out, SMM_NOUT);\n"
    "    const int g = cgrp[ch];\n"
    "    const int first = __ffsll((long long)__ballot(1)) - 1;\n"
    "#pragma unroll\n"
    "    for (int q = 0; q < SMM_NOUT; ++q) {\n"
    "        if (q < q0 || q >= q0 + qb) continue;\n"
    "        const double v = out[q];\n"
    "        if (chunked) {\n"
    "            col[((size_t)q * nbc + (size_t)blockIdx.y) * cstride + i0 + tid] = v - gmean[(size_t)g * SMM_NOUT + q];\n"
    "            continue;\n"
    "        }\n"
    "        col[(size_t)(q - q0) * cstride + pos0 + tid] = v;\n"
    "        const bool bad = (__double_as_longlong(v) & 0x7ff0000000000000ll) == 0x7ff0000000000000ll;\n"
    "        const unsigned long long m = __ballot(bad);\n"
    "        if (m != 0ull && (tid & 63) == first) atomicAdd(&nnf[(size_t)g * SMM_NOUT + q], (unsigned long long)__popcll(m));\n"
    "    }\n"
    "}\n";

// what a persistent form's translation unit includes behind the user's source: these, then its own kernel's headers (every one of them,
// and what they include in turn, must be among the Makefile's EMBED: tests/test_user_objective.py compiles each form without a device)
const char* const PERSIST_HEADERS[] = {"smm_params.hpp", "smm_walk_lean.hpp", "smm_propose.hpp", "smm_chain.hpp", "smm_p2p.hpp", "smm_chain_norm.hpp", "smm_chain_persist.hpp"};
const char* const PERSIST_HEADERS_GEN[] = {"smm_chain_persist_gen.hpp"};
const char* const PERSIST_HEADERS_TILE[] = {"smm_chain_persist_loc.hpp", "smm_chain_persist_tile.hpp"};

struct Hiprtc {
    void* lib = nullptr;
    decltype(&hiprtcCreateProgram) create = nullptr;
    decltype(&hiprtcCompileProgram) compile = nullptr;
    decltype(&hiprtcGetProgramLogSize) log_size = nullptr;
    decltype(&hiprtcGetProgramLog) log = nullptr;
    decltype(&hiprtcGetCodeSize) code_size = nullptr;
    decltype(&hiprtcGetCode) code = nullptr;
    decltype(&hiprtcDestroyProgram) destroy = nullptr;
    bool load(std::string& err) {
        if (lib) return true;
        lib = dlopen("libhiprtc.so", RTLD_NOW | RTLD_LOCAL);
        if (!lib) lib = dlopen("/opt/rocm/lib/libhiprtc.so", RTLD_NOW | RTLD_LOCAL);
        if (!lib) { err = std::string("cannot load libhiprtc.so: ") + dlerror(); return false; }
#define RTC_SYM(f, name) f = (decltype(f))dlsym(lib, name); if (!f) { err = std::string("libhiprtc.so lacks ") + name; return false; }
        RTC_SYM(create, "hiprtcCreateProgram") RTC_SYM(compile, "hiprtcCompileProgram") RTC_SYM(log_size, "hiprtcGetProgramLogSize")
        RTC_SYM(log, "hiprtcGetProgramLog") RTC_SYM(code_size, "hiprtcGetCodeSize") RTC_SYM(code, "hiprtcGetCode")
        RTC_SYM(destroy, "hiprtcDestroyProgram")
#undef RTC_SYM
        return true;
    }
};
Hiprtc g_rtc;

// One translation unit through hiprtc (g_user_mutex held): 1 with its code; 0 where the text does not compile, with the compiler's log; -1
// where there is no compiler to ask, with the reason in log.  headers: hiprtc is given the library's device headers for #include (g_embedded)
// and stand-ins for what they ask of the host's toolchain (hiprtc brings its own runtime header and has no system headers to lean on).
int rtc_compile(const std::string& tu, const char* name, bool headers, const std::vector<const char*>& opts, std::vector<char>& code, std::string& log) {
    if (!g_rtc.load(log)) return -1;
    std::vector<const char*> names, texts;
    if (headers) {
        for (const EmbeddedSource& e : g_embedded) { names.push_back(e.name); texts.push_back(e.text); }
        static const char* stub_stdint = "typedef unsigned int uint32_t; typedef unsigned long uint64_t; typedef int int32_t; typedef long int64_t;\n"
                                         "typedef unsigned short uint16_t; typedef unsigned char uint8_t; typedef signed char int8_t; typedef short int16_t;\n";
        static const char* stub_math = "#ifndef INFINITY\n#define INFINITY __builtin_huge_val()\n#endif\n#ifndef NAN\n#define NAN __builtin_nan(\"\")\n#endif\n";
        names.push_back("hip/hip_runtime.h"); texts.push_back("\n");
        names.push_back("stdint.h"); texts.push_back(stub_stdint);
        names.push_back("math.h"); texts.push_back(stub_math);
    }
    hiprtcProgram prog = nullptr;
    if (g_rtc.create(&prog, tu.c_str(), name, (int)names.size(), texts.data(), names.data()) != HIPRTC_SUCCESS) {
        log = "hiprtcCreateProgram failed";
        return -1;
    }
    const bool ok = g_rtc.compile(prog, (int)opts.size(), const_cast<const char**>(opts.data())) == HIPRTC_SUCCESS;
    size_t n = 0;
    if (ok) {
        g_rtc.code_size(prog, &n);
        code.resize(n);
        g_rtc.code(prog, code.data());
    } else {
        g_rtc.log_size(prog, &n);
        log.assign(n, ' ');
        if (n) g_rtc.log(prog, &log[0]);
    }
    g_rtc.destroy(&prog);
    return ok ? 1 : 0;
}

// which persistent form of its user objective a context of these forms launches (select_forms gives a shard with a factor no persistent form)
UserForm user_form_wanted(const Forms& F, bool has_chol) {
    return F.persist != PERSIST_TILE ? UF_GEN : F.persist_sh ? UF_TILE_SHARD : has_chol ? UF_TILE_CHOL : UF_TILE;
}
const char* user_form_kernel(UserForm form) { return form == UF_GEN ? "smm_user_persist_kernel" : "smm_user_persist_tile_kernel"; }

// A persistent kernel with the user's objective inside: the library's own device headers (embedded as text) + the user's source through
// hiprtc, once per registered objective and form, on demand (the first context that qualifies for the form: ~1.5 s).  false: the form is
// not available for this objective (u.form[form].log says why); the per-iteration launches serve it as before.
bool user_form_compile(UserObjective& u, UserForm form) {   // (g_user_mutex held)
    UserCode& F = u.form[form];
    if (F.state != 0) return F.state > 0;
    F.state = -1;
    const bool tile = form != UF_GEN;
    if (u.source.empty() || (u.lanes != 0) != tile) { F.log = tile ? "not the map-reduce form" : "not the one-thread-per-chain form"; return false; }
    std::string tu = "#include <type_traits>\n#include <stdint.h>\n#include <math.h>\n";
    if (u.rng) tu += std::string(USER_RNG_API) + (tile ? USER_PRELUDE_LANES_RNG : USER_PRELUDE_RNG) + "#define SMM_USER_RNG 1\n";
    else tu += tile ? USER_PRELUDE_LANES : USER_PRELUDE_GEN;
    tu += u.source;
    if (form == UF_TILE_SHARD) tu += "\n#define SMM_TILE_SH 1";
    if (form == UF_TILE_CHOL) tu += "\n#define SMM_TILE_CHOL 1";
    tu += tile ? "\n#define SMM_TILE_USER 1\n" : "\n#define SMM_GEN_USER 1\n";
    tu += "#include \"smmhip.h\"\n#include \"smm_rng.hpp\"\nusing namespace smm;\n";
    auto include = [&tu](const char* h) { tu += std::string("#include \"") + h + "\"\n"; };
    for (const char* h : PERSIST_HEADERS) include(h);
    if (tile) for (const char* h : PERSIST_HEADERS_TILE) include(h);
    else for (const char* h : PERSIST_HEADERS_GEN) include(h);
    const std::string nsd = "-DSMM_NSUMS=" + std::to_string(u.n_sums);
    std::vector<const char*> opts = {"--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fno-fast-math", "-std=c++17"};
    if (tile) opts.push_back(nsd.c_str());
    if (rtc_compile(tu, tile ? "smm_user_persist_tile.hip" : "smm_user_persist.hip", true, opts, F.code, F.log) > 0) F.state = 1;
    return F.state > 0;
}

// a user's text between its prelude and its evaluation kernel, compiled and entered in the registry (user_text: kept for the persistent forms)
int register_user_source(const std::string& src, int n_sums, int lanes, int32_t* objective_id_out, const char* user_text, bool rng = false) {
    std::lock_guard<std::mutex> lock(g_user_mutex);
    UserObjective u;
    u.lanes = lanes;
    u.n_sums = n_sums > 0 ? n_sums : 1;
    u.rng = rng;
    u.source = user_text;
    const std::string nsd = "-DSMM_NSUMS=" + std::to_string(u.n_sums);
    // (rng: the stream's draws need smm_rng.hpp)
    std::string log;
    const int rc = rtc_compile(src, "smm_user_objective.hip", rng, {"--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", nsd.c_str()}, u.code, log);
    if (rc < 0) { g_create_err = log; return SMM_ERR_HIP; }
    if (rc == 0) { g_create_err = "user objective does not compile:\n" + log; return SMM_ERR_INVALID_ARG; }
    g_user_objectives.push_back(std::move(u));
    *objective_id_out = SMM_OBJ_USER_BASE + (int32_t)g_user_objectives.size() - 1;
    return SMM_OK;
}

// a registered transform's outputs, and its code where the caller still has to load it (code != NULL); false: no such handle
bool user_transform_get(int32_t transform_id, int* n_out, std::vector<char>* code) {
    std::lock_guard<std::mutex> lock(g_user_mutex);
    if (transform_id < 0 || transform_id >= (int32_t)g_user_transforms.size()) return false;
    const UserTransform& u = g_user_transforms[transform_id];
    *n_out = u.n_out;
    if (code) *code = u.code;
    return true;
}

}  // namespace

extern "C" {

int smm_register_user_transform(const char* hip_source, int32_t n_out, int32_t* transform_id_out) {
    if (!hip_source || !transform_id_out) { g_create_err = "smm_register_user_transform: null argument"; return SMM_ERR_INVALID_ARG; }
    if (n_out < 1 || n_out > 64) { g_create_err = "smm_register_user_transform: need 1 <= n_out <= 64"; return SMM_ERR_INVALID_ARG; }
    std::lock_guard<std::mutex> lock(g_user_mutex);
    UserTransform u;
    u.n_out = n_out;
    const std::string nout = "-DSMM_NOUT=" + std::to_string(n_out), hp = "-DSMM_H_PARAMS=" + std::to_string((int)H_PARAMS),
                      hv = "-DSMM_H_VALUE=" + std::to_string((int)H_VALUE);
    std::string log;
    const int rc = rtc_compile(std::string(USER_PRELUDE_TRANSFORM) + hip_source + USER_KERNEL_TRANSFORM, "smm_user_transform.hip", true,
                               {"--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fno-fast-math", "-std=c++17", nout.c_str(), hp.c_str(),
                                hv.c_str()},
                               u.code, log);
    if (rc < 0) { g_create_err = log; return SMM_ERR_HIP; }
    if (rc == 0) { g_create_err = "user transform does not compile:\n" + log; return SMM_ERR_INVALID_ARG; }
    g_user_transforms.push_back(std::move(u));
    *transform_id_out = (int32_t)g_user_transforms.size() - 1;
    return SMM_OK;
}

int smm_register_user_objective(const char* hip_source, int32_t* objective_id_out) {
    if (!hip_source || !objective_id_out) { g_create_err = "smm_register_user_objective: null argument"; return SMM_ERR_INVALID_ARG; }
    return register_user_source(std::string(USER_PRELUDE) + hip_source + USER_KERNEL, 1, 0, objective_id_out, hip_source);
}

int smm_register_user_objective_lanes(const char* hip_source, int32_t n_sums, int32_t lanes, int32_t* objective_id_out) {
    if (!hip_source || !objective_id_out) { g_create_err = "smm_register_user_objective_lanes: null argument"; return SMM_ERR_INVALID_ARG; }
    if (n_sums < 1 || n_sums > 64 || lanes < 64 || lanes > 1024 || lanes % 64 != 0) {
        g_create_err = "smm_register_user_objective_lanes: need 1 <= n_sums <= 64 and lanes a multiple of 64 in [64, 1024]";
        return SMM_ERR_INVALID_ARG;
    }
    return register_user_source(std::string(USER_PRELUDE_LANES) + hip_source + USER_KERNEL_LANES, n_sums, lanes, objective_id_out, hip_source);
}

int smm_register_user_objective_rng(const char* hip_source, int32_t n_sums, int32_t lanes, int32_t* objective_id_out) {
    if (!hip_source || !objective_id_out) { g_create_err = "smm_register_user_objective_rng: null argument"; return SMM_ERR_INVALID_ARG; }
    if (n_sums < 0 || n_sums > 64 || (n_sums > 0 && (lanes < 64 || lanes > 1024 || lanes % 64 != 0))) {
        g_create_err = "smm_register_user_objective_rng: need n_sums = 0 (one thread per evaluation) or 1 <= n_sums <= 64 with lanes a multiple "
                       "of 64 in [64, 1024]";
        return SMM_ERR_INVALID_ARG;
    }
    if (n_sums == 0)
        return register_user_source(std::string(USER_RNG_API) + USER_PRELUDE_RNG + hip_source + USER_KERNEL_RNG, 1, 0, objective_id_out, hip_source, true);
    return register_user_source(std::string(USER_RNG_API) + USER_PRELUDE_LANES_RNG + hip_source + USER_KERNEL_LANES_RNG, n_sums, lanes, objective_id_out,
                                hip_source, true);
}

#ifdef SMM_TEST_HOOKS
// debug (test build only, not part of the public header), touching no device: size and FNV-1a of the code hiprtc gave for a registered
// objective.  form 0: its evaluation kernels (made at registration); 1 .. 4: its persistent forms gen, tile, tile_shard, tile_chol, compiled now
// (user_form_compile) unless they stand already.  1: the form is available; 0: it is refused or does not compile (log says why); < 0: a bad id or form
int smm_debug_user_form(int32_t objective_id, int form, unsigned long long* size, unsigned long long* fnv1a, char* log, int cap) {
    std::lock_guard<std::mutex> lock(g_user_mutex);
    const int k = objective_id - SMM_OBJ_USER_BASE;
    if (k < 0 || k >= (int)g_user_objectives.size() || form < 0 || form > UF_COUNT) return SMM_ERR_INVALID_ARG;
    UserObjective& u = g_user_objectives[k];
    const bool ok = form == 0 || user_form_compile(u, (UserForm)(form - 1));
    const std::vector<char>& code = form == 0 ? u.code : u.form[form - 1].code;
    unsigned long long h = 14695981039346656037ull;
    for (const char ch : code) h = (h ^ (unsigned char)ch) * 1099511628211ull;
    if (size) *size = ok ? code.size() : 0;
    if (fnv1a) *fnv1a = ok ? h : 0;
    if (log && cap > 0) snprintf(log, (size_t)cap, "%s", form == 0 ? "" : u.form[form - 1].log.c_str());
    return ok ? 1 : 0;
}
#endif

}  // extern "C"
