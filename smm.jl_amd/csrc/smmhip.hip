// smmhip.hip — libsmmhip.so: hand-written HIP (gfx950 / MI355X) implementation of the BGP
// parallel-tempering iteration of floswald/SMM.jl behind the C ABI of include/smmhip.h.
//
// One iteration of computeNextIteration!(algo::MAlgoBGP) (src/mopt/AlgoBGP.jl:589-640) is ONE launch on a single
// shard (two when sharded or above 4096 chains):
//   k_chain_iter      : exchangeMoves! of the previous iteration (:647-716; the level walk of
//                       exchange_walk_tile, executed by every workgroup) and next_eval for every chain at once —
//                       materialise that exchange (swap_ev_ij! :734-749), proposal (:424-471), objective
//                       (mprob.jl:175-188 -> ObjExamples.jl:59-116), doAcceptReject! (:324-392),
//                       set_eval! (:220-245).  A 512-lane tile owns CT chains, the ns simulated draws are
//                       spread over the lanes, every shock z is re-used CT times from a register, moments
//                       are reduced by a transposed wave reduction and combined through LDS.
//   k_exch_resolve_*  : the same exchange resolution as a kernel of one workgroup (sharded path, larger
//                       populations, and whenever the result is needed before the next chain kernel).
// Files: smm_params.hpp (parameter block, layouts), smm_accept.hpp (the accept step's rules, written once for every kernel), smm_chain.hpp (chain kernel and its parts), smm_lookahead.hpp (k_pregen_rng,
// k_exch_plan), smm_exchange.hpp (stand-alone exchange kernels), this file (host: the types, user objectives, launch helpers, choosers, windows, the call frame), smm_forms_host.hpp (which forms a context runs and the LDS they take: select_forms), smm_create_host.hpp (context creation, step by step), smm_run_host.hpp (the run's host side:
// stepping, settling, the sharded protocol), smm_reducers_host.hpp (the history reducers' host side), smm_population_host.hpp (the starting population's).
// Everything that does not depend on the chains' state is produced ahead of the dependent loop by
// wide, latency-tolerant kernels, one window of iterations at a time:
//   k_pregen_rng      : proposal normals (first tries) and the MH uniforms (probs_acc, :85)
//   k_exch_plan       : the exchange pair list of every iteration and each pair's rank among the
//                       pairs of its two chains (the dependency structure of the sequential walk)
//
// Data layout in HBM (FP64 throughout): everything a chain needs per iteration sits in a few
// 16-byte aligned per-chain blocks (array-of-structures), so that the 64 lanes of a tile's
// control wave move a whole tile's state with a handful of dwordx4 instructions:
//   cs   [N][16]          chain state block (sigma, accept-rate counters, best/bestp, acc_tuner)
//   rec  [2][N][RW]       last accepted record: value, prob, status, params[np], simM[nm]
//   rb   [W][N][RBW]      randomness block of one iteration: u, normals[tries][np]
//   hrec [T][N][HW]       history record: value, prob, curr, best, best_id, exch, acc, status,
//                         params[np], simM[nm]   (transposed to the ABI's SoA on download)
//   xres [Ng]             exchange result: src | partner<<32
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <hip/hiprtc.h>
#include <dlfcn.h>
#include <chrono>
#include <mutex>
#include <thread>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <math.h>
#include <algorithm>
#include <string>
#include <vector>
#include <type_traits>

#include "../../include/smmhip.h"
#include "smm_rng.hpp"

namespace {

using namespace smm;

#include "smm_params.hpp"
#include "smm_walk_lean.hpp"
#include "smm_propose.hpp"
#include "smm_chain.hpp"
#include "smm_p2p.hpp"
#include "smm_chain_norm.hpp"
#include "smm_chain_persist.hpp"
#include "smm_chain_persist_gen.hpp"
#include "smm_chain_persist_loc.hpp"
#include "smm_chain_persist_tile.hpp"
#include "smm_lookahead.hpp"
#include "smm_exchange.hpp"
#include "smm_cone_big.hpp"
#include "smm_window.hpp"
#include "smm_stats.hpp"
#include "smm_cov.hpp"
#include "smm_diag.hpp"
#include "smm_group.hpp"
#include "smm_moments.hpp"
#include "smm_adjust.hpp"
#include "smm_hist.hpp"
#include "smm_profile.hpp"
#include "smm_trace.hpp"
#include "smm_rank.hpp"
#include "smm_draws.hpp"
#include "smm_population.hpp"

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
thread_local std::string g_create_err;

// Test seams.  The shipped library (libsmmhip.so) reads two environment variables, both diagnostics: SMMHIP_TS (phase stamps for
// tools/) and SMMHIP_DBG (timing experiments; results invalid).  Everything that changes which kernel runs or how much it may
// hold — forcing an exchange kernel, switching a fast path off, a tiny capacity, poisoned allocations — exists only in the build
// the tests load next to it (libsmmhip_hooks.so, -DSMM_TEST_HOOKS): a stray variable cannot change what production runs.
#ifdef SMM_TEST_HOOKS
#define SMM_HOOK(name) getenv(name)
#else
#define SMM_HOOK(name) ((const char*)nullptr)
#endif

// ------------------------------------------------------------------------------------------
// user objectives: compiled with hiprtc (loaded lazily, the library does not link against it)
// ------------------------------------------------------------------------------------------
struct UserObjective {
    std::vector<char> code; int lanes = 0; /* 0: one thread per chain; else lanes per chain (map-reduce form) */
    std::string source;                    // the user's text (one thread per chain form): compiled once more INTO the persistent kernel on demand
    std::vector<char> persist_code;        // k_chain_persist_gen with the user's objective inside (smm_chain_persist_gen.hpp, SMM_GEN_USER)
    int persist_state = 0;                 // 0: not tried yet, 1: persist_code stands, -1: did not compile (persist_log)
    std::string persist_log;
    int n_sums = 1;                        // map-reduce form: partial sums per lane
    std::vector<char> tile_code;           // k_chain_persist_tile with the user's map-reduce objective inside (smm_chain_persist_tile.hpp, SMM_TILE_USER)
    int tile_state = 0;                    // 0: not tried yet, 1: tile_code stands, -1: did not compile (tile_log)
    std::string tile_log;
    std::vector<char> tile_sh_code;        // ... its form for a SHARD (SMM_TILE_SH as well): compiled only when a sharded context first wants it
    int tile_sh_state = 0;
    std::string tile_sh_log;
    std::vector<char> tile_chol_code;      // ... its form for proposals with a Cholesky factor (SMM_TILE_CHOL as well): compiled only when a context with a factor first wants it
    int tile_chol_state = 0;
    std::string tile_chol_log;
    bool rng = false;                      // SMM_USER_OBJECTIVE_RNG / SMM_USER_PARTIAL_RNG: takes the library's stream (smm_register_user_objective_rng)
};
// the device headers the persistent kernel is made of, as text: hiprtc compiles them together with the user's source
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
// one workgroup of n_lanes threads per evaluation.  Numerical contract of the reduction: inside a
// wave the 64 partials are combined by the halving tree (offsets 32,16,...,1), the wave totals are added left to right.
const char* USER_KERNEL_LANES =
    "\nextern \"C\" __global__ void smm_user_eval_kernel(const double* theta, int N, int np, const double* mom, const double* w, int nm,\n"
    "        const double* udata, int n_udata, double* simM, double* value, int* status) {\n"
    "    __shared__ double wsum[16][SMM_NSUMS];\n"
    "    const int c = blockIdx.x, lane = threadIdx.x, nl = blockDim.x;\n"
    "    double part[SMM_NSUMS];\n"
    "    for (int i = 0; i < SMM_NSUMS; ++i) part[i] = 0.0;\n"
    "    smm_user_partial(theta + (size_t)c * np, np, udata, n_udata, lane, nl, part);\n"
    "    for (int i = 0; i < SMM_NSUMS; ++i) {\n"
    "        double a = part[i];\n"
    "        for (int off = 32; off >= 1; off >>= 1) a = a + __shfl_xor(a, off, 64);\n"
    "        if ((lane & 63) == 0) wsum[lane >> 6][i] = a;\n"
    "    }\n"
    "    __syncthreads();\n"
    "    if (lane == 0) {\n"
    "        double tot[SMM_NSUMS];\n"
    "        for (int i = 0; i < SMM_NSUMS; ++i) { double a = wsum[0][i]; for (int wv = 1; wv < nl / 64; ++wv) a = a + wsum[wv][i]; tot[i] = a; }\n"
    "        int st = 1; double v = 0.0;\n"
    "        smm_user_finish(theta + (size_t)c * np, np, tot, SMM_NSUMS, mom, w, nm, udata, n_udata, simM + (size_t)c * nm, &v, &st);\n"
    "        value[c] = v; status[c] = st;\n"
    "    }\n"
    "}\n";

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
// the map-reduce kernel of USER_KERNEL_LANES with the stream handle passed to the partial sums: the same reduction order
const char* USER_KERNEL_LANES_RNG =
    "\n__device__ inline void smm_user_eval_lanes(const double* theta, int c, int np, const double* mom, const double* w, int nm,\n"
    "        const double* udata, int n_udata, double* simM, double* value, int* status, uint64_t seed) {\n"
    "    __shared__ double wsum[16][SMM_NSUMS];\n"
    "    const int lane = threadIdx.x, nl = blockDim.x;\n"
    "    double part[SMM_NSUMS];\n"
    "    for (int i = 0; i < SMM_NSUMS; ++i) part[i] = 0.0;\n"
    "    smm_user_partial_rng(theta + (size_t)c * np, np, udata, n_udata, smm_rng_t{seed}, lane, nl, part);\n"
    "    for (int i = 0; i < SMM_NSUMS; ++i) {\n"
    "        double a = part[i];\n"
    "        for (int off = 32; off >= 1; off >>= 1) a = a + __shfl_xor(a, off, 64);\n"
    "        if ((lane & 63) == 0) wsum[lane >> 6][i] = a;\n"
    "    }\n"
    "    __syncthreads();\n"
    "    if (lane == 0) {\n"
    "        double tot[SMM_NSUMS];\n"
    "        for (int i = 0; i < SMM_NSUMS; ++i) { double a = wsum[0][i]; for (int wv = 1; wv < nl / 64; ++wv) a = a + wsum[wv][i]; tot[i] = a; }\n"
    "        int st = 1; double v = 0.0;\n"
    "        smm_user_finish(theta + (size_t)c * np, np, tot, SMM_NSUMS, mom, w, nm, udata, n_udata, simM + (size_t)c * nm, &v, &st);\n"
    "        value[c] = v; status[c] = st;\n"
    "    }\n"
    "}\n"
    "extern \"C\" __global__ void smm_user_eval_kernel(const double* theta, int N, int np, const double* mom, const double* w, int nm,\n"
    "        const double* udata, int n_udata, double* simM, double* value, int* status, uint64_t seed) {\n"
    "    smm_user_eval_lanes(theta, blockIdx.x, np, mom, w, nm, udata, n_udata, simM, value, status, seed);\n"
    "}\n"
    "extern \"C\" __global__ void smm_user_eval_noseed_kernel(const double* theta, int N, int np, const double* mom, const double* w, int nm,\n"
    "        const double* udata, int n_udata, double* simM, double* value, int* status, uint64_t base_seed) {\n"
    "    smm_user_eval_lanes(theta, blockIdx.x, np, mom, w, nm, udata, n_udata, simM, value, status, base_seed + (uint64_t)blockIdx.x);\n"
    "}\n";

// what hiprtc is given for #include: the library's device headers (g_embedded) and stand-ins for what they ask of the host's toolchain
// (hiprtc brings its own runtime header and has no system headers to lean on)
void rtc_headers(std::vector<const char*>& names, std::vector<const char*>& texts) {
    for (const EmbeddedSource& e : g_embedded) { names.push_back(e.name); texts.push_back(e.text); }
    static const char* stub_stdint = "typedef unsigned int uint32_t; typedef unsigned long uint64_t; typedef int int32_t; typedef long int64_t;\n"
                                     "typedef unsigned short uint16_t; typedef unsigned char uint8_t; typedef signed char int8_t; typedef short int16_t;\n";
    static const char* stub_math = "#ifndef INFINITY\n#define INFINITY __builtin_huge_val()\n#endif\n#ifndef NAN\n#define NAN __builtin_nan(\"\")\n#endif\n";
    names.push_back("hip/hip_runtime.h"); texts.push_back("\n");
    names.push_back("stdint.h"); texts.push_back(stub_stdint);
    names.push_back("math.h"); texts.push_back(stub_math);
}

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

// k_chain_persist_gen with a user objective inside: the library's own device headers (embedded as text) + the user's source through
// hiprtc, once per registered objective and on demand (the first context that qualifies for the persistent form: ~1.5 s).  false: the
// form is not available for this objective (u.persist_log says why); the per-iteration launches serve it as before.
bool user_persist_compile(UserObjective& u) {   // (g_user_mutex held)
    if (u.persist_state != 0) return u.persist_state > 0;
    u.persist_state = -1;
    if (u.source.empty() || u.lanes != 0) { u.persist_log = "not the one-thread-per-chain form"; return false; }
    std::string err;
    if (!g_rtc.load(err)) { u.persist_log = err; return false; }
    std::string tu = "#include <type_traits>\n#include <stdint.h>\n#include <math.h>\n";
    if (u.rng)
        tu += std::string(USER_RNG_API) + USER_PRELUDE_RNG + "#define SMM_USER_RNG 1\n";
    else
        tu += "#define SMM_USER_OBJECTIVE extern \"C\" __device__ void smm_user_objective\n"
              "extern \"C\" __device__ void smm_user_objective(const double* theta, int np, const double* mom, const double* w, int nm,\n"
              "        const double* udata, int n_udata, double* sim_moments, double* value, int* status);\n";
    tu += u.source;
    tu += "\n#define SMM_GEN_USER 1\n#include \"smmhip.h\"\n#include \"smm_rng.hpp\"\nusing namespace smm;\n#include \"smm_params.hpp\"\n"
          "#include \"smm_walk_lean.hpp\"\n#include \"smm_propose.hpp\"\n#include \"smm_chain.hpp\"\n#include \"smm_p2p.hpp\"\n#include \"smm_chain_norm.hpp\"\n"
          "#include \"smm_chain_persist.hpp\"\n#include \"smm_chain_persist_gen.hpp\"\n";
    std::vector<const char*> names, texts;
    rtc_headers(names, texts);
    hiprtcProgram prog = nullptr;
    if (g_rtc.create(&prog, tu.c_str(), "smm_user_persist.hip", (int)names.size(), texts.data(), names.data()) != HIPRTC_SUCCESS) {
        u.persist_log = "hiprtcCreateProgram failed";
        return false;
    }
    const char* opts[] = {"--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fno-fast-math", "-std=c++17"};
    const hiprtcResult rc = g_rtc.compile(prog, 5, opts);
    if (rc != HIPRTC_SUCCESS) {
        size_t n = 0;
        g_rtc.log_size(prog, &n);
        std::string log(n, ' ');
        if (n) g_rtc.log(prog, &log[0]);
        u.persist_log = log;
        g_rtc.destroy(&prog);
        return false;
    }
    size_t cs = 0;
    g_rtc.code_size(prog, &cs);
    u.persist_code.resize(cs);
    g_rtc.code(prog, u.persist_code.data());
    g_rtc.destroy(&prog);
    u.persist_state = 1;
    return true;
}

// k_chain_persist_tile with a user objective in its MAP-REDUCE form inside (smm_register_user_objective_lanes; SMM_TILE_USER in
// smm_chain_persist_tile.hpp): the same recipe, on demand, once per registered objective — and once more as a shard's form (sh: SMM_TILE_SH),
// only when a sharded context wants it, and as the form for a Cholesky factor (chol: SMM_TILE_CHOL; never a shard's), only when a context
// with a factor wants it
bool user_tile_compile(UserObjective& u, const bool sh = false, const bool chol = false) {   // (g_user_mutex held)
    int& state = chol ? u.tile_chol_state : sh ? u.tile_sh_state : u.tile_state;
    std::string& tlog = chol ? u.tile_chol_log : sh ? u.tile_sh_log : u.tile_log;
    std::vector<char>& code = chol ? u.tile_chol_code : sh ? u.tile_sh_code : u.tile_code;
    if (state != 0) return state > 0;
    state = -1;
    if (u.source.empty() || u.lanes == 0) { tlog = "not the map-reduce form"; return false; }
    std::string err;
    if (!g_rtc.load(err)) { tlog = err; return false; }
    std::string tu = "#include <type_traits>\n#include <stdint.h>\n#include <math.h>\n";
    if (u.rng)
        tu += std::string(USER_RNG_API) + USER_PRELUDE_LANES_RNG + "#define SMM_USER_RNG 1\n";
    else
        tu += USER_PRELUDE_LANES;
    tu += u.source;
    if (sh) tu += "\n#define SMM_TILE_SH 1";
    if (chol) tu += "\n#define SMM_TILE_CHOL 1";
    tu += "\n#define SMM_TILE_USER 1\n#include \"smmhip.h\"\n#include \"smm_rng.hpp\"\nusing namespace smm;\n#include \"smm_params.hpp\"\n"
          "#include \"smm_walk_lean.hpp\"\n#include \"smm_propose.hpp\"\n#include \"smm_chain.hpp\"\n#include \"smm_p2p.hpp\"\n#include \"smm_chain_norm.hpp\"\n"
          "#include \"smm_chain_persist.hpp\"\n#include \"smm_chain_persist_loc.hpp\"\n#include \"smm_chain_persist_tile.hpp\"\n";
    std::vector<const char*> names, texts;
    rtc_headers(names, texts);
    hiprtcProgram prog = nullptr;
    if (g_rtc.create(&prog, tu.c_str(), "smm_user_persist_tile.hip", (int)names.size(), texts.data(), names.data()) != HIPRTC_SUCCESS) {
        tlog = "hiprtcCreateProgram failed";
        return false;
    }
    const std::string nsd = "-DSMM_NSUMS=" + std::to_string(u.n_sums);
    const char* opts[] = {"--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fno-fast-math", "-std=c++17", nsd.c_str()};
    const hiprtcResult rc = g_rtc.compile(prog, 6, opts);
    if (rc != HIPRTC_SUCCESS) {
        size_t n = 0;
        g_rtc.log_size(prog, &n);
        std::string log(n, ' ');
        if (n) g_rtc.log(prog, &log[0]);
        tlog = log;
        g_rtc.destroy(&prog);
        return false;
    }
    size_t cs = 0;
    g_rtc.code_size(prog, &cs);
    code.resize(cs);
    g_rtc.code(prog, code.data());
    g_rtc.destroy(&prog);
    state = 1;
    return true;
}

// Test hooks, read once at the top of smm_ctx_create (SMM_HOOK: nothing of them in the shipped library; read_hooks names the
// variables).  Every field holds the value that applies when its variable is not set.
struct Hooks {
    int fill = -1;                 // every allocation starts as this byte (reads of memory nobody wrote show up)
    bool any_exchange = false;     // the any-size resolution kernel
    bool dataflow = false;         // the ticket (data-flow) resolution kernel
    bool big_exchange = false;     // the global-memory level kernels
    bool key_exchange_off = false; // the global-memory walk instead of the key kernels
    bool key_walk_off = false;     // no lean plan, no rows resolution (k_exch_resolve_key, 16-byte / split slots)
    bool inline_walk_off = false;
    bool norm_fast_off = false;    // the general kernel for objfunc_norm
    int norm_narrow = -1;          // 0 never, 1 always
    int tpw = 0;                   // 1 one tile per workgroup, 2 two at any size
    bool dense_keys_off = false;   // the dense objective keeps the stand-alone resolution
    bool no_cone = false;          // every workgroup walks the whole list
    bool persist_off = false, persist_loc_off = false, persist_tile_off = false;   // the persistent forms: none, not the local, not the tile form
    bool cone_big_off = false;     // k_exch_resolve_rows between the launches
    bool plan_ahead_off = false;   // each window planned on the main stream when it is entered
    int plan_cap = 1 << 30;        // short plan windows
    int lvl_wg = 1024;             // tuning: the workgroup of k_exch_resolve_lvl
    int scout_after = SMM_SCOUT_AFTER, scout_gl = 16;   // the scouting form of mysample's late tries
    int a2a_cap = 0;               // a small capacity of the values form (0: a2a_capacity)
    int pr_ring_k = PR_K, pr_slow_tile = -1, pr_slow_ticks = 0;   // the persistent kernels' ring depth, a tile made slow by so many ticks
    int pr_slow_read = 0;   // ... k_chain_persist_tile's shard form: slow while it still reads the ring's last entry (a donor's remote granules), not before its publication
    bool rows_win_check = false;   // the p2p rows resolution checked against the plain kernels
    size_t stats_scratch = 0;      // the reducers' scratch cap instead of REDUCER_BATCH_CAP (0: that cap; reducer_batch_cap): batches of chains and parameters at small sizes
    int stats_mode_bins = STATS_MODE_BINS;   // partner ids per pass of k_stats_mode (1 .. STATS_MODE_BINS): several passes at small populations
    long long group_wide_min = STATS_LDS_N + 1;   // pooled columns of at least so many draws take the grid-wide select (1 .. STATS_LDS_N + 1)
    int hist_lds_bins = 1 << 30;   // bins (1-D) and bins2 (2-D) above this count into global memory, not LDS (1 ..)
    size_t pop_scratch = 0;        // the candidate scratch cap of smm_scatter_population instead of POP_SCRATCH_CAP (0: that cap): several batches of chains at small sizes
};
Hooks read_hooks() {
    Hooks H;
    auto is = [](const char* v, char ch) { return v && v[0] == ch; };
    if (const char* v = SMM_HOOK("SMMHIP_FILL")) H.fill = atoi(v);
    H.any_exchange = is(SMM_HOOK("SMMHIP_ANY_EXCHANGE"), '1');
    H.dataflow = is(SMM_HOOK("SMMHIP_DATAFLOW_EXCHANGE"), '1');
    H.big_exchange = is(SMM_HOOK("SMMHIP_BIG_EXCHANGE"), '1');
    H.key_exchange_off = is(SMM_HOOK("SMMHIP_KEY_EXCHANGE"), '0');
    H.key_walk_off = is(SMM_HOOK("SMMHIP_KEY_WALK"), '0');
    H.inline_walk_off = is(SMM_HOOK("SMMHIP_INLINE_WALK"), '0');
    H.norm_fast_off = is(SMM_HOOK("SMMHIP_NORM_FAST"), '0');
    if (const char* v = SMM_HOOK("SMMHIP_NORM_NARROW")) H.norm_narrow = v[0] == '0' ? 0 : v[0] == '1' ? 1 : -1;
    if (const char* v = SMM_HOOK("SMMHIP_TPW")) H.tpw = v[0] == '1' ? 1 : v[0] == '2' ? 2 : 0;
    H.dense_keys_off = is(SMM_HOOK("SMMHIP_DENSE_KEYS"), '0');
    H.no_cone = is(SMM_HOOK("SMMHIP_NO_CONE"), '1');
    H.persist_off = is(SMM_HOOK("SMMHIP_PERSIST"), '0');
    H.persist_loc_off = is(SMM_HOOK("SMMHIP_PERSIST_LOC"), '0');
    H.persist_tile_off = is(SMM_HOOK("SMMHIP_PERSIST_TILE"), '0');
    H.cone_big_off = is(SMM_HOOK("SMMHIP_CONE_BIG"), '0');
    H.plan_ahead_off = is(SMM_HOOK("SMMHIP_PLAN_AHEAD"), '0');
    if (const char* v = SMM_HOOK("SMMHIP_PLAN_CAP")) H.plan_cap = atoi(v);
    if (const char* v = SMM_HOOK("SMMHIP_LVL_WG")) H.lvl_wg = atoi(v);
    if (const char* v = SMM_HOOK("SMMHIP_SCOUT_AFTER")) H.scout_after = atoi(v);
    if (const char* v = SMM_HOOK("SMMHIP_SCOUT_GL")) H.scout_gl = atoi(v) == 8 ? 8 : 16;
    if (const char* v = SMM_HOOK("SMMHIP_A2A_CAP")) H.a2a_cap = std::max(1, atoi(v));
    if (const char* v = SMM_HOOK("SMMHIP_PR_RING")) { const int k = atoi(v); if (k == 2 || k == 4) H.pr_ring_k = k; }
    if (const char* v = SMM_HOOK("SMMHIP_PR_SLOW_TILE")) H.pr_slow_tile = atoi(v);
    if (const char* v = SMM_HOOK("SMMHIP_PR_SLOW_US")) H.pr_slow_ticks = 100 * atoi(v);
    H.pr_slow_read = is(SMM_HOOK("SMMHIP_PR_SLOW_READ"), '1');
    H.rows_win_check = SMM_HOOK("SMMHIP_ROWS_WIN_CHECK") != nullptr;
    if (const char* v = SMM_HOOK("SMMHIP_STATS_SCRATCH")) H.stats_scratch = (size_t)strtoull(v, nullptr, 10);
    if (const char* v = SMM_HOOK("SMMHIP_STATS_MODE_BINS")) H.stats_mode_bins = std::min(STATS_MODE_BINS, std::max(1, atoi(v)));
    if (const char* v = SMM_HOOK("SMMHIP_GROUP_WIDE_MIN")) H.group_wide_min = std::min((long long)STATS_LDS_N + 1, std::max(1ll, atoll(v)));
    if (const char* v = SMM_HOOK("SMMHIP_HIST_LDS_BINS")) H.hist_lds_bins = std::max(1, atoi(v));
    if (const char* v = SMM_HOOK("SMMHIP_POP_SCRATCH")) H.pop_scratch = (size_t)strtoull(v, nullptr, 10);
    return H;
}
// which stand-alone resolution of exchangeMoves! (AlgoBGP.jl:647-716) a context takes: decided once (select_forms); the kernels: exch_instance's table
enum ExchKernel { XK_LEAN, XK_LVL, XK_LVL_SOA, XK_TICKETS, XK_ROWS, XK_KEY, XK_LVL_BIG, XK_ANY };
// The forms a context runs, chosen once at creation from the problem, the device and the hooks (select_forms) and not changed after.
enum PlanKind { PLAN_NONE, PLAN_LDS, PLAN_BIG };   // the look-ahead exchange plans: none (one chain), k_exch_plan, k_exch_plan_big
enum PersistKind { PERSIST_NONE, PERSIST_GEN, PERSIST_LOC, PERSIST_TILE };   // the persistent chain kernel (smm_chain_persist*.hpp)
struct Forms {
    // the exchange
    PlanKind plan = PLAN_NONE;
    ExchKernel xk = XK_ANY;      // the stand-alone resolution (the table above)
    int rows_cap = 0;            // XK_ROWS: rows of XWG pairs per iteration of the plan
    bool lean_plan = false;      // the padded lean plan (smm_walk_lean.hpp) is made behind the level plan
    bool lean_wide = false;      // ... on 16-byte units (one min_improve > 0, or thresholds by chain)
    bool plan_ahead = false;     // big plans: the windows are planned ahead on a second stream into two sets of tables (PlanSet)
    int win_cap = 0;             // iterations per window of pre-generated randomness
    int plan_cap = 0;            // iterations per window of exchange plans
    // the chain kernel
    int ct = 8;                  // chains per simulation tile (4 and 16 were measured and rejected: more shock traffic / spills)
    bool norm_fast = false;      // objfunc_norm with np == nm <= 4 and one proposal batch: k_chain_iter_norm (16-chain tiles)
    bool norm_narrow = false;    // k_chain_iter_norm_narrow instead of k_chain_iter_norm<., false>: shards of more than one round of tiles
    int tpw = 1;                 // tiles per workgroup of k_chain_iter (2 with the inline walk: one walk per CU)
    int tile_off = 0;            // KParams::tile_off: doubles of LDS in front of the tile (the inline walk's slots)
    // the inline exchange walk: in the prologue of the next chain kernel
    bool inline_walk = false;
    bool gen_lean = false;       // k_chain_iter walks inline on the lean form (16-byte slots) when the plan fits it
    bool gen_keys = false;       // ... on the lean KEY form (8-byte slots): single shards of 4096 < N <= 8192 chains without a simulation (two 16-chain tiles per workgroup)
    bool dense_keys = false;     // ... and the dense objective's tiles (one 16-chain tile per workgroup, N <= 4096): the walk's slots and lists UNDER the tile's blocks
    bool cone = false;           // the key form of k_chain_iter walks its workgroups' cones (smm_cone.hpp)
    bool cone_big = false;       // large single shards of objfunc_norm (8192 < N <= 32768): the narrow chain kernel's tiles walk their own, locally numbered cones (smm_cone_big.hpp)
    bool walk_slots = false;     // the accept step writes the lean key walk's 8-byte slots (slot8_buf, walk_flags)
    int cone_tiles = 0, cone_ct = 0;   // the cone tables: tiles and chains per tile (0 tiles: none)
    bool cone_gather = false;    // ... with the tiles' gather lists (the persistent forms, the local cones)
    // the persistent chain kernel: one launch for a run of iterations
    PersistKind persist = PERSIST_NONE;
    bool persist_wide = false;   // ... its 16-byte slots: one min_improve > 0 (or NaN) for all chains
    bool persist_sh = false;     // ... as a SHARD of a sharded run: the ring lives in every rank's p2p window (smm_bgp_p2p_step)
    bool persist_sh_big = false; // ... of a population past 8192 chains: k_exch_plan_big + k_cone_chains + k_cone_tiles list its tiles' cones (locally numbered)
    bool persist_user = false;   // PERSIST_GEN launches pfn (the user's objective inside)
    int max_tiles = 0;           // tiles of the persistent kernel this device holds at once (occupancy x compute units)
    bool defer_resolve = false;  // the exchange of an iteration is left unresolved until somebody needs it (the next launch may be the persistent kernel's)
};

// the device for select_forms: its compute units, and the candidate persistent kernel's resident workgroups per CU (-1: not asked yet; 0: not available)
struct DeviceFacts { int n_cus = 256; int per_cu = -1; };
// what a chooser hands a launcher (name: what smm_describe says; block: lanes of a workgroup; ct: chains per tile; tpw: tiles per workgroup)
struct ChainKernel { const void* fn; const char* name; unsigned block; int ct, tpw; };
struct PersistKernel { const void* fn; hipFunction_t mfn; dim3 grid, block; size_t smem; const char* name; };
// a row of exch_instance's table (cap: the dynamic LDS limit raised at creation where the context's forms include the row's group, 0: the default
// will do; stamped: takes the dispatch's own stamps in profiling mode 2), and a chooser's pick for one launch (the row, this launch's dynamic LDS)
enum ExchId { XI_CONE_CHAINS, XI_CONE_TILES, XI_PLAN_BIG, XI_PLAN, XI_LEAN, XI_LVL_256, XI_LVL_512, XI_LVL, XI_LVL_SOA, XI_TICKETS, XI_KEYS, XI_ROWS_PLDS,
              XI_ROWS, XI_KEY_PLDS, XI_KEY, XI_LVL_BIG, XI_ANY, XI_ROWS_WIN_OWN, XI_ROWS_WIN_PLDS, XI_ROWS_WIN, XI_APPLY, XI_COUNT };
enum ExchGroup { XG_BIG, XG_KEYS, XG_LDS, XG_CONE_BIG };
struct ExchInstance { const void* fn; unsigned block; size_t cap; ExchGroup group; const char* name; bool stamped; };
struct ExchLaunch { int id; size_t smem; };
// one set of the plan window's tables: the levels' pairs, thresholds and offsets, the rows of k_exch_resolve_rows, the tiles' cones
struct LevelTables {
    uint32_t *lv_pairs = nullptr, *lv_off = nullptr, *lv_rows = nullptr, *lv_rowinfo = nullptr, *cone_ok = nullptr, *cone_hdr = nullptr, *cone_pairs = nullptr;
    double* lv_mi = nullptr; uint16_t* cone_gather = nullptr;
};
// Where the run stands, as the host keeps it: what persist_snapshot saves and persist_repair puts back, whole
struct Run {
    int iter = 0;
    int cur = 0;               // rec[cur] holds the records after the last accept step
    int slots_iter = -1;       // single shard, rows exchange: the accept step of this iteration wrote the resolution's initial slots (no pre-pass)
    bool pending = false;      // exchange of iteration `iter` resolved but not applied
    bool prev_open = false;    // accept-rate counters of iteration `iter` not closed yet
    bool unresolved = false;   // exchangeMoves! of iteration `iter` is still to be resolved (inline, or by resolve_now)
    bool exch_done = false;    // the three-phase / values forms: exchangeMoves! of iteration `iter` has been applied (cleared by the next local step)
};

struct Ctx {
    KParams P{};
    Hooks H;                   // read once at creation
    Forms F;                   // chosen once at creation (select_forms)
    DeviceFacts dev;           // ... with these
    // what will be uploaded, known before it is (create_facts; select_forms reads these, not the pointers): a factor, the 256 x 256 stage, injected normals / uniforms
    bool has_chol = false, dense2 = false, has_ntab = false, has_utab = false;
    int obj = 0, device = 0, exchange_from = 2;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::vector<void*> allocs;
    std::string err;
    int u_lanes = 0;                // user objective: lanes per evaluation (0 = one thread per chain)
    int n_objp = 0;                 // doubles in P.objp
    hipModule_t umod = nullptr;     // user objective: this context's module and kernel
    hipFunction_t ufn = nullptr;
    hipFunction_t ufn_noseed = nullptr;   // ... an objective with the library's stream: its noseed kernel (evaluation i keyed by base_seed + i)
    bool u_rng = false;
    hipModule_t pmod = nullptr;     // ... and the persistent kernel compiled with it inside: k_chain_persist_gen (SMM_GEN_USER), or
    hipFunction_t pfn = nullptr;    //     k_chain_persist_tile with its map-reduce form (SMM_TILE_USER)
    int u_nsums = 1;                // ... its partial sums per lane
    int pop_kind = 0, pop_M = 0; // the starting population installed on this context: 0 none, 1 smm_set_population, 2 smm_scatter_population (smm_describe)
    double pop_spread = 0.0;

    // ---- run state ----
    Run run;
    // (a shard's flags: not part of what persist_snapshot saves — persist_repair sets them itself)
    bool rec_external = false;  // the records after the last accept step were written to the caller's gather buffer (sharded_step)
    bool pending_ext = false;   // sharded_step: the exchange of iteration `run.iter` is still to be resolved from the gathered records
    bool a2a_open = false;
    bool p2p_current = false;                  // the windows hold the records after iteration `run.iter`
    bool p2p_unwaited = false;                 // nobody has waited for the arrivals of the last push yet
    int failed = 0;             // a hard device error (AlgoBGP.jl:341,409) stopped the run at iteration `run.iter`: sticky until smm_set_state
    bool failed_told = false;   // `failed` has been returned to the caller by some entry point
    // double-buffered last-accepted records [N][RW]
    double* rec[2] = {nullptr, nullptr};
    double* vals_buf[2] = {nullptr, nullptr};   // KParams::vals / vals_out, by iteration parity (point_values)
    uint2* slot8_buf[2] = {nullptr, nullptr};
    bool deep_plan = false;      // an injected pair list has an iteration of more than LV_MAXLEV dependency levels
    bool nan_values = false;     // the uploaded state holds NaN values (smm_set_state)
    // (set for one launch: ExternalRecords, smm_run_host.hpp)
    const double* ext_rec_in = nullptr;   // sharded_step: donor records come from / results go to the caller's gather buffers
    double* ext_rec_out = nullptr;
    double* ext_vals_out = nullptr;            // p2p generic form: the accept step's values go into the window

    // ---- look-ahead windows ----
    double* win_rb = nullptr;
    unsigned long long* win_plan = nullptr;
    double* win_plan_mi = nullptr;
    LevelTables win;              // the plan window's own set of tables
    uint32_t *win_lv_pairs_p = nullptr, *win_lv_offp = nullptr, *slots17 = nullptr, *nan_flags = nullptr;
    uint32_t* big_scratch = nullptr;
    int rng_t0 = 0, rng_w = 0;    // window currently held: iterations [t0, t0+w)
    int plan_t0 = 0, plan_w = 0;
    uint32_t* cb_scratch = nullptr;
    std::vector<uint32_t> cone_big_ok;   // per iteration of the plan window: its cones fit their caps
    // ... their windows are planned AHEAD: the plan of a window depends on (seed, iteration) only, so while the chain kernels of one
    // window run, the three plan kernels of the next run beside them on a second stream into the other of two sets of tables
    struct PlanSet : LevelTables {
        uint32_t* ok_host = nullptr;   // (pinned) cone_ok as the host reads it
        hipEvent_t done = nullptr;
        int t0 = 0, w = 0;             // iterations [t0, t0 + w) are (being) planned into this set
    } ps[2];
    int ps_act = 0;                      // the set the chain kernels read
    hipStream_t pstream = nullptr;
    hipEvent_t ev_free = nullptr;        // main stream: every launch that reads the set about to be planned into has been enqueued before it (plan_window_into)

    // ---- the values form of the sharded exchange ----
    int32_t *a2a_send_idx = nullptr, *a2a_send_cnt = nullptr, *a2a_rowidx = nullptr;
    int a2a_cap = 0, a2a_G = 0;

    // ---- the p2p form of the sharded iteration (smm_p2p.hpp) ----
    unsigned char* p2p_mine = nullptr;         // this rank's window (null: smm_bgp_p2p_init not called)
    void* p2p_opened[P2P_MAXG] = {};           // peers' windows opened through HIP IPC (closed with the context)
    unsigned p2p_attached = 0;                 // bit r: rank r's window is known
    unsigned long long p2p_seq = 0;            // pushes so far (every rank counts the same)
    bool p2p_inline = false;                   // the inline form is available: k_chain_iter_norm_p2p walks inline and pushes from its epilogue
    bool p2p_rows = false;                     // the same kernel without the walk + k_exch_resolve_rows<., true> on the window's slots
    bool p2p_mode_inline = false;              // ... and is what the windows currently hold (decided at every publication)
    int p2p_ranks_here = 1;                    // ranks whose windows live on THIS device (this one included): their tiles must all be resident together

    // ---- the persistent chain kernel (smm_chain_persist.hpp): one launch for a run of iterations ----
    unsigned char* prw = nullptr;              // persist_loc: the ring's window (pr_win_layout) — a single shard's own allocation, a shard's: inside its p2p window
    size_t prw_off = 0;                        // persist_sh: offset of the ring's window inside the p2p window
    bool persist_proven = false;               // a launch of the persistent form has come through: its spins may last P2P_TIMEOUT_TICKS from now on
    int persist_strikes = 0;                   // time-outs so far (two: the form is off for the context)
    int persist_on = 1;                        // smm_set_persistent
    bool persist_broken = false;               // a launch gave up waiting (tiles not resident together?): the form is off for this context
    uint32_t pr_epoch = 0;                     // launches so far
    int persist_launches = 0, persist_repairs = 0;
    int pregen_seen_launches = 0;              // persist_launches when the last window of randomness blocks was made (ensure_windows)
    bool in_repair = false;
    // ... and what persist_repair restores when a launch of it ends with the error word set: the state before the FIRST such launch
    // since the last check of the error word
    bool snap_valid = false;
    Run snap;
    double *snap_cs = nullptr, *snap_rec = nullptr, *snap_vals[2] = {nullptr, nullptr}, *hist_fill = nullptr;
    uint2* snap_slot8[2] = {nullptr, nullptr};
    unsigned long long* snap_xres = nullptr;

    // ---- the history reducers (smm_get_chain_stats / _cov / _diag, smm_adapt_proposal) ----
    // their shared scratch for the compacted columns (reducer_scratch) and the results of a call (reducer_result: grown to the largest
    // call's), both in smm_reducers_host.hpp
    void* st_scr = nullptr;
    size_t st_scr_bytes = 0;
    void* red_res = nullptr;
    size_t red_res_bytes = 0;

    // ---- profiling ----
    smm_timing_t timing{};
    bool pending_timing = false;
    int profiling = 0;   // 1: event brackets around the kernels; 2: the kernels' own begin/end timestamps (launch_fn)
    hipEvent_t kev0 = nullptr, kev1 = nullptr;   // mode 2: start/stop events of the next launch (set for that launch: KernelEvents, smm_run_host.hpp)
    std::vector<char> pev_exch;
    std::vector<hipEvent_t> pev;  // profiling events: 4 per iteration (the last two bracket nothing: the event overhead)
    int pev_iters = 0;
};

#define HIPCHK(call)                                                                                  \
    do {                                                                                              \
        hipError_t e_ = (call);                                                                       \
        if (e_ != hipSuccess) {                                                                       \
            char b_[512];                                                                             \
            snprintf(b_, sizeof b_, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            throw std::string(b_);                                                                    \
        }                                                                                             \
    } while (0)

template <class T>
T* dalloc(Ctx* c, size_t n) {
    void* p = nullptr;
    HIPCHK(hipMalloc(&p, (n ? n : 1) * sizeof(T)));
    c->allocs.push_back(p);
    if (c->H.fill >= 0) HIPCHK(hipMemset(p, c->H.fill, (n ? n : 1) * sizeof(T)));   // (test hook SMMHIP_FILL)
    return (T*)p;
}
template <class T>
T* dupload(Ctx* c, const T* h, size_t n) {
    T* d = dalloc<T>(c, n);
    if (h && n) HIPCHK(hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice));
    return d;
}

// a kernel known by its address (the choosers' tables) onto a stream, the launch's result checked here; in profiling mode 2 (kev0 set: a KernelEvents
// scope) a launch on the context's own stream that takes them (stamped) carries the begin/end of its dispatch as the command processor stamps them
void launch_fn(Ctx* c, const void* fn, dim3 grid, dim3 block, size_t smem, hipStream_t st, void** args, bool stamped = true) {
    if (stamped && c->kev0 && st == c->stream) HIPCHK(hipExtLaunchKernel(fn, grid, block, args, smem, st, c->kev0, c->kev1, 0));
    else HIPCHK(hipLaunchKernel(fn, grid, block, args, smem, st));
}

bool is_sim(int obj) { return obj == SMM_OBJ_NORM || obj == SMM_OBJ_NORM_FAILBOX; }
int obj_kind(int obj) { return is_sim(obj) ? 1 : obj == SMM_OBJ_DENSE ? 2 : 0; }
// the two value arrays (and slot arrays) alternate by iteration: reads of iteration t_read's values, writes of iteration t_write's
void point_values(const Ctx* c, KParams& P, int t_read, int t_write) {
    P.vals = c->vals_buf[t_read & 1]; P.vals_out = c->vals_buf[t_write & 1];
    P.slot8 = c->slot8_buf[t_read & 1]; P.slot8_out = c->slot8_buf[t_write & 1];
}

}  // namespace

#include "smm_forms_host.hpp"

namespace {

int exchange_K(const Ctx* c) { return c->P.n_pairs_tab > 0 ? c->P.n_pairs_tab : n_exchange_pairs(c->P.Ng); }   // (an injected pair list: its length)
bool exchange_active(const Ctx* c, int t) { return t >= c->exchange_from && c->P.Ng > 1; }  // AlgoBGP.jl:637

ExchInstance exch_instance(int id, int Ng = 0);   // (the table stands behind the chain kernels': the kernels are emitted in the order in which they are named)
// row `id` of that table onto stream st: every launch of the exchange family (args: exactly the kernel's parameter types — they travel as addresses)
template <class... Args>
void launch_exch(Ctx* c, int id, dim3 grid, size_t smem, hipStream_t st, const Args&... args) {
    const ExchInstance I = exch_instance(id);
    if (!I.fn) throw std::string("exchange kernel ") + I.name + " is not part of this build";
    void* a[] = {(void*)&args...};
    launch_fn(c, I.fn, grid, dim3(I.block), smem, st, a, I.stamped);
}
size_t plan_smem(int Ng, int K, bool cones) { return cones ? std::max(plan_lds_bytes(Ng, K), plan_cone_bytes()) : plan_lds_bytes(Ng, K); }   // k_exch_plan's dynamic LDS (cones: it lists the tiles' cones too)
// the big plan of W iterations from t on into the tables L on stream st; cones: and the tiles' locally numbered cones, from the plan's scratch (pairs in list order, their levels)
void launch_plan_big(Ctx* c, const KParams& P, int t, int W, const LevelTables& L, hipStream_t st, bool cones) {
    launch_exch(c, XI_PLAN_BIG, dim3(W), plan_big_lds_bytes(P.Ng), st, P, t, c->big_scratch, L.lv_pairs, L.lv_mi, L.lv_off, L.lv_rows, L.lv_rowinfo);
    if (!cones) return;
    launch_exch(c, XI_CONE_CHAINS, dim3(W), cone_chains_lds_bytes(P.Ng), st, P, (const uint32_t*)L.lv_pairs, (const uint32_t*)L.lv_off, c->cb_scratch);
    const unsigned blocks = ((P.cone_tiles + CONEB_WAVES - 1) / CONEB_WAVES) * ((W + 7) & ~7);
    launch_exch(c, XI_CONE_TILES, dim3(blocks), cone_tiles_lds_bytes(P.plan_K), st, P, W, (const uint32_t*)c->cb_scratch);
}
// the plan window starting at iteration t into set k, on the plan stream (the kernels' scratch is theirs alone: one window at a time
// there) — behind every launch enqueued on the main stream so far: the ones that read set k are all among them (k is not the active set)
void plan_window_into(Ctx* c, int k, int t) {
    Ctx::PlanSet& S = c->ps[k];
    KParams Pw = c->P;
    HIPCHK(hipEventRecord(c->ev_free, c->stream));
    HIPCHK(hipStreamWaitEvent(c->pstream, c->ev_free, 0));
    Pw.cone_ok = S.cone_ok; Pw.cone_hdr = S.cone_hdr; Pw.cone_pairs = S.cone_pairs; Pw.cone_gather = S.cone_gather;
    const int W = std::min(c->F.plan_cap, Pw.T - t + 1);
    launch_plan_big(c, Pw, t, W, S, c->pstream, true);
    HIPCHK(hipMemcpyAsync(S.ok_host, S.cone_ok, (size_t)W * 4, hipMemcpyDeviceToHost, c->pstream));
    HIPCHK(hipEventRecord(S.done, c->pstream));
    S.t0 = t; S.w = W;
}

// iteration t lies behind the plan window, the exchange of t - 1 is still to be walked: does the window planned ahead hold both?
bool plan_ahead_covers(const Ctx* c, int t) {
    const Ctx::PlanSet& S = c->ps[c->ps_act ^ 1];
    return c->F.plan_ahead && S.w >= 2 && S.t0 == t - 1;
}

// make the look-ahead tables cover iteration t (1-based): a new window simply starts at t
void ensure_windows(Ctx* c, int t, bool rng = true) {
    KParams& P = c->P;
    // (k_chain_iter_norm generates its randomness itself unless tables are injected: no randomness blocks)
    const bool pregen = rng && !(c->F.norm_fast && !P.user_ntab && !P.user_utab);
    if (pregen && !(t >= c->rng_t0 && t < c->rng_t0 + c->rng_w)) {
        int W = std::min(c->F.win_cap, P.T - t + 1);
        // (k_chain_persist_gen draws in the kernel too: blocks only for the iterations between its launches)
        // — and only where such launches are really being made: a caller that steps one iteration at a time (the reference's run! loop
        // over computeNextIteration!, AlgoAbstract.jl:38-45) never takes the persistent form and keeps its full windows
        if ((c->F.persist == PERSIST_GEN || c->F.persist == PERSIST_TILE) && c->persist_on && !c->persist_broken && !c->in_repair && !P.user_ntab && !P.user_utab &&
            c->persist_launches != c->pregen_seen_launches) W = std::min(W, 2);
        c->pregen_seen_launches = c->persist_launches;
        const size_t Q = (size_t)(P.np + 1) / 2;
        const size_t per_iter = (size_t)P.rb_tries * Q * P.N;   // (< 2^31: checked at creation)
        hipLaunchKernelGGL(k_pregen_rng, dim3((unsigned)((per_iter + 255) / 256), (unsigned)W), dim3(256), 0, c->stream, P, t, W, c->win_rb);
        c->rng_t0 = t; c->rng_w = W;
        P.rb = c->win_rb; P.rb_t0 = t;
    }
    if (c->F.plan_ahead && !(t >= c->plan_t0 && t < c->plan_t0 + c->plan_w)) {
        const int nx = c->ps_act ^ 1;
        Ctx::PlanSet& S = c->ps[nx];
        // (the window planned ahead starts with the LAST iteration of the one before it, so that an exchange of that iteration still
        // to be walked by this launch's tiles finds its cones in the new window: plan_ahead_covers)
        if (!(S.w > 0 && (S.t0 == t || (S.t0 == t - 1 && S.w >= 2)))) plan_window_into(c, nx, t);   // (the first window, a jump: not the window planned ahead)
        HIPCHK(hipEventSynchronize(S.done));                         // the host reads the window's flags (long there when planned ahead)
        HIPCHK(hipStreamWaitEvent(c->stream, S.done, 0));
        c->ps_act = nx; c->plan_t0 = S.t0; c->plan_w = S.w;
        P.plan_t0 = S.t0;
        P.lv_rows = S.lv_rows; P.lv_rowinfo = S.lv_rowinfo; P.lv_pairs = S.lv_pairs; P.lv_mi = S.lv_mi; P.lv_off = S.lv_off;
        P.cone_ok = S.cone_ok; P.cone_hdr = S.cone_hdr; P.cone_pairs = S.cone_pairs; P.cone_gather = S.cone_gather;
        c->cone_big_ok.assign(S.ok_host, S.ok_host + S.w);
        // the next window, into the set the launches enqueued so far read
        c->ps[nx ^ 1].w = 0;
        if (S.t0 + S.w <= P.T) plan_window_into(c, nx ^ 1, S.t0 + S.w - (S.w >= 2 && c->F.plan_cap >= 2 ? 1 : 0));
    }
    if (c->F.plan == PLAN_BIG && !c->F.plan_ahead && !(t >= c->plan_t0 && t < c->plan_t0 + c->plan_w)) {
        const int W = std::min(c->F.plan_cap, P.T - t + 1);
        launch_plan_big(c, P, t, W, c->win, c->stream, c->F.cone_big || c->F.persist_sh_big);
        c->plan_t0 = t; c->plan_w = W;
        P.plan_t0 = t;
        if (c->F.cone_big) {   // (the persistent kernel of a shard looks at the window's flags itself: no synchronisation)
            // a cone that does not fit its caps (a pair list of very deep dependency chains: the user's, or an unlucky sample) sends its
            // iteration to the stand-alone resolution: the host looks at the window's flags once (one synchronisation per window)
            c->cone_big_ok.resize((size_t)W);
            HIPCHK(hipMemcpyAsync(c->cone_big_ok.data(), P.cone_ok, (size_t)W * 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
        }
        P.lv_rows = c->win.lv_rows; P.lv_rowinfo = c->win.lv_rowinfo;
        P.lv_pairs = c->win.lv_pairs; P.lv_mi = c->win.lv_mi; P.lv_off = c->win.lv_off;
    }
    if (c->F.plan == PLAN_LDS && P.Ng > 1 && !(t >= c->plan_t0 && t < c->plan_t0 + c->plan_w)) {
        const int W = std::min(c->F.plan_cap, P.T - t + 1);
        launch_exch(c, XI_PLAN, dim3(W), plan_smem(P.Ng, P.plan_K, c->F.cone || c->F.persist != PERSIST_NONE), c->stream, P, t, c->win_plan, c->win_plan_mi,
                    c->win.lv_pairs, c->win.lv_mi, c->win.lv_off, c->win_lv_pairs_p, c->win_lv_offp);
        c->plan_t0 = t; c->plan_w = W;
        P.plan = c->win_plan; P.plan_mi = c->win_plan_mi; P.plan_t0 = t;
        P.lv_pairs = c->win.lv_pairs; P.lv_mi = c->win.lv_mi; P.lv_off = c->win.lv_off;
        P.lv_pairs_p = c->win_lv_pairs_p; P.lv_offp = c->win_lv_offp;
    }
}

// ---- which per-iteration chain kernel (smm_chain.hpp, smm_chain_norm.hpp) ----
// Every instantiation of the chain kernels' templates that a launch can take is named in chain_instance() and nowhere else: chain_kernel()
// and chain_kernel_p2p() pick one for a launch, smm_ctx_create raises the dynamic LDS limit of every one of them, smm_describe prints the
// pick's name.  A new instantiation is one line in chain_instance() (a new family: one more name in ChainFamily).
enum ChainFamily {
    CF_SIM, CF_SIM_2, CF_DENSE, CF_GEN_KEYS, CF_GEN_64, CF_GEN_2, CF_GEN,   // k_chain_iter<KIND, CT, TPW, b>: b = compiled with the inline walk
    CF_NORM_NARROW_CONE, CF_NORM_ANY, CF_NORM_WIDE, CF_NORM_NARROW,        // k_chain_iter_norm_*<np>
    CF_NORM,                                                               // k_chain_iter_norm<np, b>: b = this launch walks
    CF_P2P_ROWS_NARROW, CF_P2P_ROWS,                                       // k_chain_iter_norm_p2p_rows*<np>
    CF_P2P,                                                                // k_chain_iter_norm_p2p<np, b>: b = staging loops for more than XLVL_MAX chains or pairs
    CF_COUNT
};
// f(std::integral_constant<int, np>) for a parameter count known at run time: 1 .. 4, as the norm kernels are instantiated
template <class F>
const void* by_np(int np, F f) {
    switch (np) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        default: return f(std::integral_constant<int, 4>{});
    }
}
// (np counts for the norm and p2p families only.  The order in which the kernels are named here is the order in which the compiler emits
// them, and the register numbering of a few of them follows it: kept as the launchers named them before there was this table)
ChainKernel chain_instance(int family, int np, bool b) {
#define ITER(KIND, CT, TPW, NAME) \
    ChainKernel{b ? (const void*)k_chain_iter<KIND, CT, TPW, true> : (const void*)k_chain_iter<KIND, CT, TPW, false>, NAME, WG * TPW, CT, TPW}
#define NORM(KERN, NAME, BLOCK) ChainKernel{by_np(np, [](auto NP) { return (const void*)KERN<decltype(NP)::value>; }), NAME, BLOCK, NORM_CT, 1}
#define NORM_B(KERN, NAME) \
    ChainKernel{by_np(np, [b](auto NP) { return !b ? (const void*)KERN<decltype(NP)::value, false> : (const void*)KERN<decltype(NP)::value, true>; }), NAME, NORM_WG, NORM_CT, 1}
    switch (family) {
        case CF_SIM: return ITER(1, 8, 1, "iter<sim,8>");
        case CF_SIM_2: return ITER(1, 8, 2, "iter<sim,8,2>");
        case CF_DENSE: return ITER(2, 16, 1, "iter<dense,16>");
        case CF_GEN_KEYS: return ITER(0, 16, 2, "iter<gen,16,2>");
        case CF_GEN_64: return ITER(0, 64, 1, "iter<gen,8>");   // (smm_describe has always filed the 64-chain tile under the 8-chain tile's name)
        case CF_GEN_2: return ITER(0, 8, 2, "iter<gen,8,2>");
        case CF_GEN: return ITER(0, 8, 1, "iter<gen,8>");
        case CF_NORM_NARROW_CONE: return NORM(k_chain_iter_norm_narrow_cone, "iter_norm_narrow_cone", NORM_WG / 2);
        case CF_NORM_ANY: return NORM(k_chain_iter_norm_any, "iter_norm_any", NORM_WG);
        case CF_NORM_WIDE: return NORM(k_chain_iter_norm_wide, "iter_norm_wide", NORM_WG);
        case CF_NORM_NARROW: return NORM(k_chain_iter_norm_narrow, "iter_norm_narrow", NORM_WG / 2);
        case CF_NORM: return NORM_B(k_chain_iter_norm, "iter_norm");
        case CF_P2P_ROWS_NARROW: return NORM(k_chain_iter_norm_p2p_rows_narrow, "iter_norm_p2p_rows_narrow", NORM_WG / 2);
        case CF_P2P_ROWS: return NORM(k_chain_iter_norm_p2p_rows, "iter_norm_p2p_rows", NORM_WG);
        default: return NORM_B(k_chain_iter_norm_p2p, "iter_norm_p2p");
    }
#undef ITER
#undef NORM
#undef NORM_B
}
// what launch_chain_iter launches for this context as it stands now; flags & F_WALK_INLINE: the launch walks the previous iteration's
// exchange.  Decides only: allocates nothing, launches nothing.
ChainKernel chain_kernel(const Ctx* c, int flags) {
    const KParams& P = c->P;
    const Forms& F = c->F;
    const bool walk = (flags & F_WALK_INLINE) != 0, user = c->obj == SMM_OBJ_USER;
    if (F.norm_fast && !user) {   // k_chain_iter_norm and its variants: one 16-chain tile per workgroup
        // large single shards: every tile walks its own, locally numbered cone (smm_cone_big.hpp)
        if (walk && F.cone_big) return chain_instance(CF_NORM_NARROW_CONE, P.np, false);
        // the lean walks need a padded plan of at most 31 levels and values without NaN: where that is not given — per-chain or
        // negative thresholds (no padded plan), an injected pair list that goes deeper, an uploaded state with NaN values — the
        // kernel with the walk on 16-byte slots {value, src, partner} runs
        // (mi_pct: the lean plan stands for the persistent launches only)
        if (walk && (!F.lean_plan || c->deep_plan || c->nan_values || P.mi_pct)) return chain_instance(CF_NORM_ANY, P.np, false);
        if (walk && P.lean_wide) return chain_instance(CF_NORM_WIDE, P.np, false);   // one min_improve > 0 for all chains: the lean walk on 16-byte slots
        // more than one round of tiles: two half-size workgroups per CU (k_chain_iter_norm_narrow)
        if (!walk && F.norm_narrow) return chain_instance(CF_NORM_NARROW, P.np, false);
        return chain_instance(CF_NORM, P.np, walk);
    }
    // the general kernel (contexts that never walk inline run it compiled without the walk).  Objectives without a simulation take tiles
    // of 64 chains where such a tile's LDS fits in 60 KB — a user objective's three launches per iteration wherever it does, ct says which
    const bool fits64 = tile_smem_base(c, 64) <= (size_t)60 * 1024;
    const int family = is_sim(c->obj) ? (F.tpw == 2 ? CF_SIM_2 : CF_SIM) : c->obj == SMM_OBJ_DENSE ? CF_DENSE : user ? (fits64 ? CF_GEN_64 : CF_GEN)
                     : F.gen_keys ? CF_GEN_KEYS : (fits64 && !F.inline_walk) ? CF_GEN_64 : F.tpw == 2 ? CF_GEN_2 : CF_GEN;
    ChainKernel K = chain_instance(family, P.np, F.inline_walk);
    if (user) K.name = c->u_lanes ? "user_lanes_3launches" : "user_3launches";
    if (c->obj == SMM_OBJ_DENSE && c->dense2) K.name = "iter<dense2,16>";
    // an objective without a simulation (banana, user objectives) has work for the tile's control wave only: unless the exchange
    // walk runs inline (all lanes stage its inputs) the tile is launched as that one wave, so that every tile of a large
    // population is resident at once instead of queueing behind 448 idle lanes each
    if (obj_kind(c->obj) == 0 && K.tpw == 1 && !walk && !F.inline_walk) K.block = 64;
    return K;
}
// ... and launch_chain_iter_norm_p2p (smm_p2p.hpp)
ChainKernel chain_kernel_p2p(const Ctx* c) {
    const KParams& P = c->P;
    // the kernel without a walk, whose accept step stores the 4-byte slots of k_exch_resolve_rows<., true>: on half-size workgroups for a
    // shard of more than one round of tiles
    if (c->p2p_rows) return chain_instance(c->F.norm_narrow ? CF_P2P_ROWS_NARROW : CF_P2P_ROWS, P.np, false);
    // (BIG: staging loops for up to 8192 chains — two shards of 4096; the small form serves populations up to 4096)
    return chain_instance(CF_P2P, P.np, P.Ng > XLVL_MAX || P.plan_K > XLVL_MAX);
}
// K over the chains of P onto the context's stream, with `smem` bytes of dynamic LDS: every kernel of these families takes (P, t, rec_in, rec_out, flags)
void launch_chain_kernel(Ctx* c, const ChainKernel& K, size_t smem, const KParams& P, int t, const double* rec_in, double* rec_out, int flags) {
    const dim3 grid((unsigned)(((P.N + K.ct - 1) / K.ct + K.tpw - 1) / K.tpw)), block(K.block);
    void* args[] = {(void*)&P, (void*)&t, (void*)&rec_in, (void*)&rec_out, (void*)&flags};
    launch_fn(c, K.fn, grid, block, smem, c->stream, args);
}

// one thread per evaluation: theta [n][np] -> simM [n][nm], value [n], status [n].  An objective with the library's stream draws from
// the context's seed, or with base_seed (smm_eval_batch_noseed) evaluation i from base_seed + i
void launch_user_kernel(Ctx* c, const double* theta, int n, double* simM, double* value, int* status, const uint64_t* base_seed = nullptr) {
    const KParams& P = c->P;
    int np = P.np, nm = P.nm, nud = c->n_objp;
    const double *mom = P.mom, *w = P.w, *ud = P.objp;
    uint64_t seed = base_seed ? *base_seed : P.seed;
    void* args[] = {(void*)&theta, (void*)&n, (void*)&np, (void*)&mom, (void*)&w, (void*)&nm, (void*)&ud, (void*)&nud,
                    (void*)&simM, (void*)&value, (void*)&status, (void*)&seed};
    const hipFunction_t fn = base_seed ? c->ufn_noseed : c->ufn;
    if (c->u_lanes > 0)   // map-reduce form: one workgroup of u_lanes threads per evaluation
        HIPCHK(hipModuleLaunchKernel(fn, (unsigned)n, 1, 1, (unsigned)c->u_lanes, 1, 1, 0, c->stream, args, nullptr));
    else
        HIPCHK(hipModuleLaunchKernel(fn, (unsigned)((n + 127) / 128), 1, 1, 128, 1, 1, 0, c->stream, args, nullptr));
}

// n evaluations on device pointers, onto the context's stream (smm_eval_batch and the starting population share it): the built-in objectives read
// params [np][n] and write simM [nm][n] and status as int8; a user objective's kernel (launch_user_kernel) reads theta [n][np] and writes
// simM [n][nm] and status as int
void launch_eval_dev(Ctx* c, const double* params, int n, double* value, double* simM, void* status) {
    const KParams& P = c->P;
    if (c->obj == SMM_OBJ_USER) {
        launch_user_kernel(c, params, n, simM, value, (int*)status);
        return;
    }
    constexpr int CT = 8;
    if (is_sim(c->obj))
        hipLaunchKernelGGL((k_eval_batch<1, CT>), dim3((n + CT - 1) / CT), dim3(WG), tile_smem_base(c, CT), c->stream, P, params, n, value, simM, (int8_t*)status);
    else if (c->obj == SMM_OBJ_DENSE)
        hipLaunchKernelGGL((k_eval_batch<2, 16>), dim3((n + 15) / 16), dim3(WG), tile_smem_base(c, 16), c->stream, P, params, n, value, simM, (int8_t*)status);
    else
        hipLaunchKernelGGL((k_eval_batch<0, CT>), dim3((n + CT - 1) / CT), dim3(WG), tile_smem_base(c, CT), c->stream, P, params, n, value, simM, (int8_t*)status);
    HIPCHK(hipGetLastError());
}

void launch_chain_iter(Ctx* c, int t, int flags) {
    point_values(c, c->P, t - 1, t);   // the inline walk reads what the accept step of t-1 wrote; this accept step writes the other array
    if (c->ext_vals_out) { c->P.vals_out = c->ext_vals_out; c->P.slot8_out = nullptr; }
    // large single shards (k_exch_resolve_rows): the accept step writes the resolution's initial slots itself
    const bool own_slots = c->F.xk == XK_ROWS && c->P.N == c->P.Ng && !c->ext_rec_out && !c->ext_vals_out && c->obj != SMM_OBJ_USER;
    c->P.slots17_out = own_slots ? c->slots17 : nullptr;
    c->P.nan_flags_out = own_slots ? c->nan_flags + (t & 1) : nullptr;
    if (own_slots) c->run.slots_iter = t;
    const ChainKernel K = chain_kernel(c, flags);
    const size_t smem = tile_smem(c, c->F, K.ct, K.tpw);
    const double* rin = c->ext_rec_in ? c->ext_rec_in : (const double*)c->rec[c->run.cur];
    double* rout = c->ext_rec_out ? c->ext_rec_out : c->rec[c->run.cur ^ 1];
    if (c->obj == SMM_OBJ_USER) {
        // proposal launch (stores nothing but the proposals) -> the user's kernel -> accept launch (repeats the
        // deterministic prologue, takes value / moments / status from the user's kernel)
        const KParams& P = c->P;
        launch_chain_kernel(c, K, smem, P, t, rin, rout, flags | F_PROPOSE_ONLY);
        launch_user_kernel(c, P.u_theta, P.N, P.u_simM, P.u_value, P.u_status);
    }
    launch_chain_kernel(c, K, smem, c->P, t, rin, rout, flags);
    if (!c->ext_rec_out) c->run.cur ^= 1;
}

// ---- the stand-alone kernels of the exchange (smm_lookahead.hpp, smm_exchange.hpp, smm_cone_big.hpp) ----
// Every instantiation of them that a launch can take is named in exch_instance() and nowhere else: launch_exch launches a row, resolve_kernel()
// and resolve_rows_window_kernel() pick the resolution's, lds_limits raises every row's dynamic LDS limit, smm_describe prints the pick's name.
// A new instantiation is one row here and one name in ExchId.  What resolves exchangeMoves! (F.xk: select_forms):
//   N_global        min_improve                      dist_fun   F.xk        rows                slots / where
//   <= 8192 (~7400) one value >= 0 for all chains    -          XK_LEAN     lean                8-byte keys (0) or 16-byte values (> 0), LDS
//   <= 4096         anything else                    any        XK_LVL      lvl<1024>           16-byte slots, LDS
//   <= 8192         anything else                    any        XK_LVL_SOA  lvl_soa             split slots, LDS
//   <= 32768        0 for all chains                 -          XK_ROWS     keys + rows<PLDS>   4-byte slots (17-bit keys), rows of 1024 pairs, LDS
//   <= 32768        anything else                    -          XK_KEY      keys + key<PLDS>    4-byte slots (16-bit keys, intervals), LDS
//   <= 65535        anything else / other dist_fun   any        XK_LVL_BIG  lvl_big             16-byte slots, global memory
//   above, or K > N_global                           any        XK_ANY      any                 barrier rounds, global atomics
// (PLDS: the partners in LDS up to XKEY_PARTNER_MAX chains, else the ballot replay.  The p2p form of a sharded run launches the rows kernel itself
//  where this table says XK_ROWS — resolve_rows_window_kernel: <., true> reads the tagged slots of its window instead of a key pre-pass, <false,
//  true, true> keeps the partners of the rank's own chains only; every other p2p population resolves from the window's plain values through this
//  table.  Single shards of objfunc_norm up to 4096 chains do not get here in steady state: their chain kernel walks inline.  The test build can
//  force an entry (SMM_TEST_HOOKS: Hooks) and adds the ticket kernel and two workgroups of lvl.  The rows stand in the order in which the host code
//  named these kernels before there was this table, behind chain_instance's: kernels are emitted, and a few numbered, in that order.  Ng: for k_cone_chains' cap.)
constexpr size_t ROWS_OWN_MAX = (size_t)158 * 1024;   // <false, true, true>: the slots, the rows and the own chains' partners of one workgroup
ExchInstance exch_instance(int id, int Ng) {
    const size_t rows_all = resolve_rows_bytes(XKEY_MAX, XKEY_MAX, XROWS_MAX), rows_part = resolve_rows_bytes(XKEY_PARTNER_MAX, XKEY_PARTNER_MAX, XROWS_MAX),
                 lvl = resolve_lvl_bytes(XLVL_MAX, XLVL_MAX);
    switch (id) {
        case XI_CONE_CHAINS: return {(const void*)k_cone_chains, XWG, cone_chains_lds_bytes(Ng), XG_CONE_BIG, "cone_chains", false};
        case XI_CONE_TILES: return {(const void*)k_cone_tiles, 64 * CONEB_WAVES, 0, XG_CONE_BIG, "cone_tiles", false};
        case XI_PLAN_BIG: return {(const void*)k_exch_plan_big, XWG, plan_big_lds_bytes(65535), XG_BIG, "plan_big", false};
        case XI_PLAN: return {(const void*)k_exch_plan, XWG, plan_smem(XLDS_MAX, XLDS_MAX, true), XG_LDS, "plan", false};
        case XI_LEAN: return {(const void*)k_exch_resolve_lean, XWG, LDS_CU, XG_LDS, "lean", true};
#ifdef SMM_TEST_HOOKS
        case XI_LVL_256: return {(const void*)k_exch_resolve_lvl<256>, 256, lvl, XG_LDS, "lvl", false};
        case XI_LVL_512: return {(const void*)k_exch_resolve_lvl<512>, 512, lvl, XG_LDS, "lvl", false};
        case XI_TICKETS: return {(const void*)k_exch_resolve_lds, XWG, resolve_lds_bytes(XLDS_MAX), XG_LDS, "tickets", false};
#endif
        case XI_LVL: return {(const void*)k_exch_resolve_lvl<1024>, 1024, lvl, XG_LDS, "lvl", true};
        case XI_LVL_SOA: return {(const void*)k_exch_resolve_lvl_soa<1024>, 1024, resolve_lvl_soa_bytes(XLDS_MAX, XLDS_MAX), XG_LDS, "lvl_soa", false};
        case XI_KEYS: return {(const void*)k_exch_keys, 256, 0, XG_KEYS, "keys", false};   // (values and initial slots: the pre-pass of rows and key)
        case XI_ROWS_PLDS: return {(const void*)k_exch_resolve_rows<true>, XWG, rows_part, XG_KEYS, "rows", false};
        case XI_ROWS: return {(const void*)k_exch_resolve_rows<false>, XWG, rows_all, XG_KEYS, "rows", false};
        case XI_KEY_PLDS: return {(const void*)k_exch_resolve_key<true>, XWG, resolve_key_bytes(XKEY_PARTNER_MAX, XKEY_PARTNER_MAX), XG_KEYS, "key", false};
        case XI_KEY: return {(const void*)k_exch_resolve_key<false>, XWG, resolve_key_bytes(XKEY_MAX, XKEY_MAX), XG_KEYS, "key", false};
        case XI_LVL_BIG: return {(const void*)k_exch_resolve_lvl_big, XWG, 0, XG_BIG, "lvl_big", false};
        case XI_ANY: return {(const void*)k_exch_resolve_any, XWG, 0, XG_BIG, "any", false};
        case XI_ROWS_WIN_OWN: return {(const void*)k_exch_resolve_rows<false, true, true>, XWG, ROWS_OWN_MAX, XG_KEYS, "rows_window_own", true};
        case XI_ROWS_WIN_PLDS: return {(const void*)k_exch_resolve_rows<true, true>, XWG, rows_part, XG_KEYS, "rows_window", true};
        case XI_ROWS_WIN: return {(const void*)k_exch_resolve_rows<false, true>, XWG, rows_all, XG_KEYS, "rows_window", true};
        case XI_APPLY: return {(const void*)k_exch_apply, 256, 0, XG_BIG, "apply", false};   // (the three-phase calls: the resolved swaps into the records)
        default: return {nullptr, 0, 0, XG_LDS, id == XI_TICKETS ? "tickets" : "lvl", false};   // (a row of the test build)
    }
}
// what launch_resolve_p launches for this context as it stands (P: its parameters or the caller's copy): F.xk, the partners-in-LDS split, the hooks' workgroup of lvl.  Decides only.
ExchLaunch resolve_kernel(const Ctx* c, const KParams& P) {
    const bool plds = P.Ng <= XKEY_PARTNER_MAX;   // partners in LDS, else the ballot replay
    switch (c->F.xk) {
        case XK_LEAN: return {XI_LEAN, resolve_lean_bytes(P.Ng, P.plan_K, P.lean_wide != 0)};
        case XK_LVL: return {c->H.lvl_wg == 256 ? XI_LVL_256 : c->H.lvl_wg == 512 ? XI_LVL_512 : XI_LVL, resolve_lvl_bytes(P.Ng, P.plan_K)};
        case XK_LVL_SOA: return {XI_LVL_SOA, resolve_lvl_soa_bytes(P.Ng, P.plan_K)};
        case XK_TICKETS: return {XI_TICKETS, resolve_lds_bytes(P.Ng)};
        case XK_ROWS: return {plds ? XI_ROWS_PLDS : XI_ROWS, resolve_rows_bytes(P.Ng, P.plan_K, P.rows_cap)};
        case XK_KEY: return {plds ? XI_KEY_PLDS : XI_KEY, resolve_key_bytes(P.Ng, P.plan_K)};
        case XK_LVL_BIG: return {XI_LVL_BIG, 0};
        default: return {XI_ANY, 0};
    }
}
// ... and launch_resolve_rows_window.  A shard of a population past XKEY_PARTNER_MAX keeps its own chains' partners only (written by the swaps), where that fits
ExchLaunch resolve_rows_window_kernel(const Ctx* c) {
    const KParams& P = c->P;
    const size_t own = resolve_rows_bytes(P.Ng, P.plan_K, P.rows_cap, P.N);
    if (P.Ng > XKEY_PARTNER_MAX && P.N < P.Ng && own <= ROWS_OWN_MAX) return {XI_ROWS_WIN_OWN, own};
    return {P.Ng <= XKEY_PARTNER_MAX ? XI_ROWS_WIN_PLDS : XI_ROWS_WIN, resolve_rows_bytes(P.Ng, P.plan_K, P.rows_cap)};
}
// Profiling mode 2, stated once: does the resolution take the dispatch's own stamps (a KernelEvents scope around its launch, pev_exch set), or do
// event brackets stand around the iteration and the exchange reports 0?  Only `stamped` rows ever do; a single shard's steps also ask for a population
// of the level walk (its chain kernel is stamped under the same condition), a shard's stamp the lean kernel only (the cases: DESIGN.md section 3)
bool resolve_stamped(const Ctx* c, bool shard) {
    const int id = resolve_kernel(c, c->P).id;
    return exch_instance(id).stamped && (shard ? id == XI_LEAN : c->P.Ng <= XLVL_MAX && !c->H.dataflow && c->H.lvl_wg == 1024);
}

// (P: the context's parameters, or a copy whose RW is the stride of the value column in `gathered`)
void launch_resolve_p(Ctx* c, const KParams& P_in, int t, const double* gathered) {
    KParams P = P_in;
    point_values(c, P, t, t);   // (single shard: the values the accept step of iteration t wrote)
    const ExchLaunch L = resolve_kernel(c, P);
    if (c->F.xk != XK_ROWS && c->F.xk != XK_KEY) return launch_exch(c, L.id, dim3(1), L.smem, c->stream, P, t, gathered);
    // values and initial slots by the whole chip (gathered records: their value column; single shard: the compact array)
    const bool prepass = gathered || c->run.slots_iter != t;   // (a single shard's accept step of iteration t has made the slots already)
    const double* vals = gathered ? P.xval : P.vals;
    const uint32_t *slots16 = prepass ? (const uint32_t*)P.xsrc : nullptr, *slots17 = c->slots17;
    if (prepass)
        launch_exch(c, XI_KEYS, dim3((P.Ng + 255) / 256), 0, c->stream, gathered ? gathered : (const double*)P.vals, gathered ? P.RW : 1, P.Ng, (double*)vals, (uint32_t*)P.xsrc,
                    c->F.xk == XK_ROWS ? c->slots17 : (uint32_t*)nullptr, c->nan_flags, t);
    if (c->F.xk == XK_ROWS) launch_exch(c, L.id, dim3(1), L.smem, c->stream, P, t, vals, slots16, slots17, c->nan_flags);
    else launch_exch(c, L.id, dim3(1), L.smem, c->stream, P, t, vals, (const uint32_t*)P.xsrc);
}
void launch_resolve(Ctx* c, int t, const double* gathered) { launch_resolve_p(c, c->P, t, gathered); }

int fail(Ctx* c, int code, const std::string& m) {
    if (c) c->err = m;
    else g_create_err = m;
    return code;
}

// the frame of every entry point that takes a context and can throw: body(c) returns SMM_OK or what fail() (or an early return) gave;
// its checks that do not throw stand inside it, in their order
template <class Body>
int api_call(void* ctx, bool args_given, Body body) {
    Ctx* c = (Ctx*)ctx;
    if (!c || !args_given) return SMM_ERR_INVALID_ARG;
    try {
        return body(c);
    } catch (const std::string& m) {
        return fail(c, SMM_ERR_HIP, m);
    }
}

// temporary device buffer of one call (freed on every exit path)
template <class T>
struct DevBuf {
    T* p = nullptr;
    explicit DevBuf(size_t n) { HIPCHK(hipMalloc((void**)&p, (n ? n : 1) * sizeof(T))); }
    ~DevBuf() { if (p) (void)hipFree(p); }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
};


// ---- the p2p form of the sharded iteration (smm_p2p.hpp, include/smmhip.h) ----
size_t p2p_walk_bytes(const Ctx* c) { return (lean_walk_bytes(c->P.Ng, c->P.plan_K) + 15) & ~(size_t)15; }
void launch_chain_iter_norm_p2p(Ctx* c, int t, int flags) {
    KParams P = c->P;
    point_values(c, P, t - 1, t);
    const bool walk = (flags & F_WALK_INLINE) != 0;
    P.tile_off = walk ? (int)(p2p_walk_bytes(c) / sizeof(double)) : 0;
    const size_t smem = (size_t)P.tile_off * sizeof(double) + norm_tile_doubles(P.np) * sizeof(double);
    launch_chain_kernel(c, chain_kernel_p2p(c), smem, P, t, nullptr, nullptr, flags);
}
// this rank's slice after iteration t -> every rank's window (parity t & 1); rec_src: out of the context's own record array (a
// publication), else out of its own window (generic form, after a chain kernel); ll: the self-validating form of the inline kernels
void launch_p2p_push(Ctx* c, int t, const double* rec_src, bool ll) {
    KParams P = c->P;
    const dim3 grid(p2p_units(P.N)), block(256);
    if (ll) hipLaunchKernelGGL((k_p2p_push<true, true>), grid, block, 0, c->stream, P, t, rec_src);
    else if (rec_src) hipLaunchKernelGGL((k_p2p_push<true, false>), grid, block, 0, c->stream, P, t, rec_src);
    else hipLaunchKernelGGL((k_p2p_push<false, false>), grid, block, 0, c->stream, P, t, (const double*)nullptr);
    if (!ll) { c->p2p_seq += 1; c->p2p_unwaited = true; }
}
void launch_p2p_wait(Ctx* c) {
    KParams P = c->P;
    P.p2p_want = (unsigned long long)p2p_units(P.N) * c->p2p_seq;
    hipLaunchKernelGGL(k_p2p_wait, dim3(1), dim3(64), 0, c->stream, P, c->run.iter);
    c->p2p_unwaited = false;
}
// inline form: everybody's records and values after iteration t, out of their self-validating form into this rank's plain arrays
void launch_p2p_unpack(Ctx* c, int t) {
    hipLaunchKernelGGL(k_p2p_unpack, dim3((c->P.Ng + 255) / 256), dim3(256), 0, c->stream, c->P, t);
}
// exchangeMoves! of iteration t from the values in this rank's window (complete: somebody has waited for the arrivals)
void launch_resolve_window(Ctx* c, int t) {
    const P2PLayout L = p2p_layout(c->P.Ng, c->P.RW);
    KParams P1 = c->P;
    P1.RW = 1;   // (the resolve kernels read value s at gathered[s * RW])
    launch_resolve_p(c, P1, t, (const double*)(c->p2p_mine + L.val[t & 1]));
}
// the same straight from the window's tagged slots and self-validating values (p2p form of large norm populations): no wait, no unpacking, no key pre-pass
void launch_resolve_rows_window(Ctx* c, int t) {
    const ExchLaunch L = resolve_rows_window_kernel(c);
    launch_exch(c, L.id, dim3(1), L.smem, c->stream, c->P, t, (const double*)nullptr, (const uint32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr);
}
// ---- the persistent chain kernels (smm_chain_persist*.hpp) ----
// what launches F's persistent kernel: a kernel of the library (fn) or of a user objective's module (mfn: loaded by persist_occupancy),
// its grid, block and dynamic LDS.  persist_occupancy sets its LDS attribute and asks for its occupancy, launch_chain_persist launches it,
// smm_describe prints its name.
PersistKernel persist_kernel(const Ctx* c, const Forms& F) {
    const KParams& P = c->P;
    PersistKernel K{nullptr, nullptr, dim3(persist_tiles_rank(F, P.N)), dim3(1), 0, "none"};
    if (F.persist == PERSIST_GEN) {
        K.block = dim3(1024);
        K.smem = persist_gen_smem(c, F.persist_user);
        K.name = F.persist_user ? "gen_user" : "gen";
        if (F.persist_user) K.mfn = c->pfn;   // (the same kernel, compiled with the user's objective inside: user_persist_compile)
        else K.fn = (const void*)k_chain_persist_gen;
    } else if (F.persist == PERSIST_LOC) {
        const bool one = P.np == 1, wd = F.persist_wide, sh = F.persist_sh;
        K.block = dim3(NORM_WG);
        K.smem = persist_loc_smem_bytes(P.np);
        K.name = sh ? (F.persist_sh_big ? (wd ? "loc_wide_shard_bigplan" : "loc_shard_bigplan") : (wd ? "loc_wide_shard" : "loc_shard")) : (wd ? "loc_wide" : "loc");
        if (P.mi_pct) K.fn = one ? (const void*)k_chain_persist_loc<1, true, false, true> : (const void*)k_chain_persist_loc<2, true, false, true>;
        else if (one) K.fn = wd ? (sh ? (const void*)k_chain_persist_loc<1, true, true> : (const void*)k_chain_persist_loc<1, true, false>)
                                : (sh ? (const void*)k_chain_persist_loc<1, false, true> : (const void*)k_chain_persist_loc<1, false, false>);
        else K.fn = wd ? (sh ? (const void*)k_chain_persist_loc<2, true, true> : (const void*)k_chain_persist_loc<2, true, false>)
                       : (sh ? (const void*)k_chain_persist_loc<2, false, true> : (const void*)k_chain_persist_loc<2, false, false>);
    } else if (F.persist == PERSIST_TILE) {
        const bool dense = obj_kind(c->obj) == 2;
        K.block = dim3(WG);
        K.smem = persist_tile_smem(c);
        K.name = c->obj == SMM_OBJ_USER ? (F.persist_sh ? "tile_user_shard" : "tile_user") : !dense ? (F.persist_sh ? "tile_sim_shard" : "tile_sim")
               : c->dense2 ? (F.persist_sh ? "tile_dense2_shard" : "tile_dense2") : (F.persist_sh ? "tile_dense_shard" : "tile_dense");
        if (c->obj == SMM_OBJ_USER) K.mfn = c->pfn;   // (the same kernel, compiled with the user's map-reduce objective inside: user_tile_compile)
        else if (F.persist_sh) K.fn = dense ? (const void*)k_chain_persist_tile<2, false, true> : (const void*)k_chain_persist_tile<1, false, true>;
        else if (c->has_chol && P.mi_pct) K.fn = dense ? (const void*)k_chain_persist_tile<2, true, false, true> : (const void*)k_chain_persist_tile<1, true, false, true>;
        else if (c->has_chol) K.fn = dense ? (const void*)k_chain_persist_tile<2, false, false, true> : (const void*)k_chain_persist_tile<1, false, false, true>;
        else if (P.mi_pct) K.fn = dense ? (const void*)k_chain_persist_tile<2, true> : (const void*)k_chain_persist_tile<1, true>;
        else K.fn = dense ? (const void*)k_chain_persist_tile<2> : (const void*)k_chain_persist_tile<1>;
    }
    return K;
}
// K onto the context's stream with the argument block A; in profiling mode 2 with the begin/end of this dispatch as the command processor stamps them
void launch_persist(Ctx* c, const PersistKernel& K, PersistArgs A) {
    void* args[] = {(void*)&A};
    if (K.mfn && c->kev0)
        HIPCHK(hipExtModuleLaunchKernel(K.mfn, K.grid.x * K.block.x, 1, 1, K.block.x, 1, 1, K.smem, c->stream, args, nullptr, c->kev0, c->kev1, 0));
    else if (K.mfn) HIPCHK(hipModuleLaunchKernel(K.mfn, K.grid.x, 1, 1, K.block.x, 1, 1, (unsigned)K.smem, c->stream, args, nullptr));
    else launch_fn(c, K.fn, K.grid, K.block, K.smem, c->stream, args);
}

}  // namespace

#include "smm_run_host.hpp"

namespace {

// --- the history readers (smm_get_history, smm_get_state); the reducers built on these two are in smm_reducers_host.hpp ----------------

// a reader's prelude: the iterations enqueued so far settled (a repair may move c->run.iter), flushed and finished
void reader_prelude(Ctx* c) {
    HIPCHK(hipSetDevice(c->device));
    settle_persist(c);
    flush(c);
    HIPCHK(hipStreamSynchronize(c->stream));
}

// a reducer's window [t0, t1), checked after the prelude
int check_window(Ctx* c, int t0, int t1) {
    if (t0 < 0 || t1 < t0 || t1 > c->run.iter) return fail(c, SMM_ERR_INVALID_ARG, "window must satisfy 0 <= t0 <= t1 <= completed iterations");
    return SMM_OK;
}

}  // namespace

#include "smm_reducers_host.hpp"
#include "smm_population_host.hpp"
#include "smm_create_host.hpp"

extern "C" {

int smm_abi_version(void) { return SMMHIP_ABI_VERSION; }

// 1 in the build the tests load for their seams (libsmmhip_hooks.so), 0 in the shipped library (not part of the public header)
int smm_debug_has_test_hooks(void) {
#ifdef SMM_TEST_HOOKS
    return 1;
#else
    return 0;
#endif
}

static int register_user_source(const std::string& src, int n_sums, int lanes, int32_t* objective_id_out, const char* user_text = nullptr,
                                bool rng = false) {
    std::lock_guard<std::mutex> lock(g_user_mutex);
    std::string err;
    if (!g_rtc.load(err)) { g_create_err = err; return SMM_ERR_HIP; }
    hiprtcProgram prog = nullptr;
    std::vector<const char*> names, texts;
    if (rng) rtc_headers(names, texts);   // (the stream's draws: smm_rng.hpp)
    if (g_rtc.create(&prog, src.c_str(), "smm_user_objective.hip", (int)names.size(), texts.data(), names.data()) != HIPRTC_SUCCESS) {
        g_create_err = "hiprtcCreateProgram failed";
        return SMM_ERR_HIP;
    }
    const std::string nsd = "-DSMM_NSUMS=" + std::to_string(n_sums > 0 ? n_sums : 1);
    const char* opts[] = {"--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", nsd.c_str()};
    const hiprtcResult rc = g_rtc.compile(prog, 5, opts);
    if (rc != HIPRTC_SUCCESS) {
        size_t n = 0;
        g_rtc.log_size(prog, &n);
        std::string log(n, ' ');
        if (n) g_rtc.log(prog, &log[0]);
        g_create_err = "user objective does not compile:\n" + log;
        g_rtc.destroy(&prog);
        return SMM_ERR_INVALID_ARG;
    }
    size_t cs = 0;
    g_rtc.code_size(prog, &cs);
    UserObjective u;
    u.code.resize(cs);
    u.lanes = lanes;
    u.n_sums = n_sums > 0 ? n_sums : 1;
    u.rng = rng;
    if (user_text) u.source = user_text;
    g_rtc.code(prog, u.code.data());
    g_rtc.destroy(&prog);
    g_user_objectives.push_back(std::move(u));
    *objective_id_out = SMM_OBJ_USER_BASE + (int32_t)g_user_objectives.size() - 1;
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

int smm_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* smm_last_error(void* ctx) { return ctx ? ((Ctx*)ctx)->err.c_str() : g_create_err.c_str(); }

void* smm_stream(void* ctx) { return ctx ? (void*)((Ctx*)ctx)->stream : nullptr; }

// a user objective's evaluations (smm_eval_batch; with base_seed, smm_eval_batch_noseed): its kernel wants [M][np] / [M][nm], transposed on the host
static void user_eval_batch(Ctx* c, const double* params, int32_t M, double* value, double* sim_moments, int8_t* status, const uint64_t* base_seed) {
    const KParams& P = c->P;
    DevBuf<double> dp((size_t)P.np * M), dv((size_t)M), dm((size_t)P.nm * M);
    std::vector<double> tp((size_t)M * P.np), tm((size_t)M * P.nm);
    std::vector<int> ts((size_t)M);
    for (int i = 0; i < M; ++i)
        for (int k = 0; k < P.np; ++k) tp[(size_t)i * P.np + k] = params[(size_t)k * M + i];
    DevBuf<int> dsi((size_t)M);
    HIPCHK(hipMemcpyAsync(dp.p, tp.data(), tp.size() * 8, hipMemcpyHostToDevice, c->stream));
    if (base_seed) launch_user_kernel(c, dp.p, M, dm.p, dv.p, dsi.p, base_seed);
    else launch_eval_dev(c, dp.p, M, dv.p, dm.p, dsi.p);
    HIPCHK(hipMemcpyAsync(value, dv.p, (size_t)M * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(tm.data(), dm.p, tm.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(ts.data(), dsi.p, ts.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int i = 0; i < M; ++i) {
        status[i] = (int8_t)ts[i];
        for (int k = 0; k < P.nm; ++k) sim_moments[(size_t)k * M + i] = tm[(size_t)i * P.nm + k];
    }
}

int smm_eval_batch(void* ctx, const double* params, int32_t M, double* value, double* sim_moments, int8_t* status) {
    return api_call(ctx, params && M >= 0 && value && sim_moments && status, [&](Ctx* c) -> int {
        if (M == 0) return SMM_OK;
        HIPCHK(hipSetDevice(c->device));
        const KParams& P = c->P;
        if (c->obj == SMM_OBJ_USER) {
            user_eval_batch(c, params, M, value, sim_moments, status, nullptr);
            return SMM_OK;
        }
        DevBuf<double> dp((size_t)P.np * M), dv((size_t)M), dm((size_t)P.nm * M);
        DevBuf<int8_t> ds((size_t)M);
        HIPCHK(hipMemcpyAsync(dp.p, params, (size_t)P.np * M * 8, hipMemcpyHostToDevice, c->stream));
        launch_eval_dev(c, dp.p, M, dv.p, dm.p, ds.p);
        HIPCHK(hipMemcpyAsync(value, dv.p, (size_t)M * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(sim_moments, dm.p, (size_t)P.nm * M * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(status, ds.p, (size_t)M, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return SMM_OK;
    });
}

int smm_eval_batch_noseed(void* ctx, const double* params, int32_t M, uint64_t base_seed, double* value, double* sim_moments, int8_t* status) {
    return api_call(ctx, params && M >= 0 && value && sim_moments && status, [&](Ctx* c) -> int {
        const bool user_rng = c->obj == SMM_OBJ_USER && c->u_rng;
        if (!is_sim(c->obj) && !user_rng)
            return fail(c, SMM_ERR_INVALID_ARG, "noseed evaluations exist for objfunc_norm and for user objectives that draw from the library's "
                                                "stream (smm_register_user_objective_rng) only");
        if (M == 0) return SMM_OK;
        HIPCHK(hipSetDevice(c->device));
        if (user_rng) {
            const uint64_t bs = base_seed;
            user_eval_batch(c, params, M, value, sim_moments, status, &bs);
            return SMM_OK;
        }
        const KParams& P = c->P;
        DevBuf<double> dp((size_t)P.np * M), dv((size_t)M), dm((size_t)P.nm * M);
        DevBuf<int8_t> ds((size_t)M);
        HIPCHK(hipMemcpyAsync(dp.p, params, (size_t)P.np * M * 8, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_eval_batch_noseed, dim3(M), dim3(WG), (size_t)(WG / 64) * P.nm * 8, c->stream, P, (const double*)dp.p, M,
                           (uint64_t)base_seed, dv.p, dm.p, ds.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(value, dv.p, (size_t)M * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(sim_moments, dm.p, (size_t)P.nm * M * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(status, ds.p, (size_t)M, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return SMM_OK;
    });
}

// history(c) (AlgoBGP.jl:138-160): download iterations t0..t1-1 and transpose the per-chain history
// records into the ABI's structure-of-arrays buffers.
int smm_get_history(void* ctx, int32_t t0, int32_t t1, smm_history_t* out) {
    return api_call(ctx, out && t0 >= 0 && t1 >= t0, [&](Ctx* c) -> int {
        if (t1 > c->P.T) return SMM_ERR_INVALID_ARG;
        reader_prelude(c);
        const KParams& P = c->P;
        const size_t N = P.N, HW = P.HW, np = P.np, nm = P.nm;
        std::vector<double> row(N * HW);
        for (int t = t0; t < t1; ++t) {
            HIPCHK(hipMemcpy(row.data(), P.hrec + (size_t)t * N * HW, row.size() * 8, hipMemcpyDeviceToHost));
            const size_t o = (size_t)(t - t0) * N;
            for (size_t i = 0; i < N; ++i) {
                const double* h = row.data() + i * HW;
                if (out->value) out->value[o + i] = h[H_VALUE];
                if (out->prob) out->prob[o + i] = h[H_PROB];
                if (out->curr_val) out->curr_val[o + i] = h[H_CURR];
                if (out->best_val) out->best_val[o + i] = h[H_BEST];
                if (out->best_id) out->best_id[o + i] = (int32_t)h[H_BESTID];
                if (out->exchanged) out->exchanged[o + i] = (int32_t)h[H_EXCH];
                if (out->accepted) out->accepted[o + i] = (uint8_t)h[H_ACC];
                if (out->status) out->status[o + i] = (int8_t)h[H_STATUS];
                if (out->params)
                    for (size_t k = 0; k < np; ++k) out->params[((size_t)(t - t0) * np + k) * N + i] = h[H_PARAMS + k];
                if (out->sim_moments)
                    for (size_t k = 0; k < nm; ++k) out->sim_moments[((size_t)(t - t0) * nm + k) * N + i] = h[H_PARAMS + np + k];
            }
        }
        return SMM_OK;
    });
}

int smm_get_state(void* ctx, smm_state_t* s) {
    return api_call(ctx, s != nullptr, [&](Ctx* c) -> int {
        reader_prelude(c);
        const KParams& P = c->P;
        const size_t N = P.N, RW = P.RW, np = P.np, nm = P.nm;
        std::vector<double> cs(N * CSW), rec(N * RW);
        HIPCHK(hipMemcpy(cs.data(), P.cs, cs.size() * 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(rec.data(), c->rec[c->run.cur], rec.size() * 8, hipMemcpyDeviceToHost));
        s->iter = c->run.iter;
        for (size_t i = 0; i < N; ++i) {
            const double* b = cs.data() + i * CSW;
            const double* r = rec.data() + i * RW;
            if (s->sigma) s->sigma[i] = b[CS_SIGMA];
            if (s->accept_rate) s->accept_rate[i] = b[CS_RATE];
            if (s->n_noex) s->n_noex[i] = (int32_t)b[CS_NNOEX];
            if (s->n_acc_noex) s->n_acc_noex[i] = (int32_t)b[CS_NACC];
            if (s->best_val) s->best_val[i] = b[CS_BEST];
            if (s->best_id) s->best_id[i] = (int32_t)b[CS_BESTID];
            if (s->la_value) s->la_value[i] = r[0];
            if (s->la_prob) s->la_prob[i] = r[1];
            if (s->la_status) s->la_status[i] = (int8_t)r[2];
            if (s->la_params)
                for (size_t k = 0; k < np; ++k) s->la_params[k * N + i] = r[3 + k];
            if (s->la_sim_moments)
                for (size_t k = 0; k < nm; ++k) s->la_sim_moments[k * N + i] = r[3 + np + k];
        }
        return SMM_OK;
    });
}

// restart! (AlgoBGP.jl:804-884) with clean resume semantics: continue at iteration iter+1
int smm_set_state(void* ctx, const smm_state_t* s, const smm_history_t* h) {
    return api_call(ctx, s && s->iter >= 0, [&](Ctx* c) -> int {
        if (s->iter > c->P.T) return SMM_ERR_INVALID_ARG;
        if (s->iter > 0 && !h) return fail(c, SMM_ERR_INVALID_ARG, "history of iterations 0..iter-1 required");
        if (!s->sigma || !s->accept_rate || !s->n_noex || !s->n_acc_noex || !s->best_val || !s->best_id || !s->la_value ||
            !s->la_prob || !s->la_status || !s->la_params || !s->la_sim_moments)
            return fail(c, SMM_ERR_INVALID_ARG, "smm_set_state needs every field of smm_state_t");
        if (s->iter > 0 && (!h->value || !h->prob || !h->curr_val || !h->best_val || !h->params || !h->sim_moments ||
                            !h->best_id || !h->exchanged || !h->accepted || !h->status))
            return fail(c, SMM_ERR_INVALID_ARG, "smm_set_state needs every field of smm_history_t");
        HIPCHK(hipSetDevice(c->device));
        settle_persist(c);
        HIPCHK(hipStreamSynchronize(c->stream));
        // a hard error nobody has been TOLD of yet (raised on the device by steps this caller enqueued and never synchronised; the state readers
        // do not raise): this call is the recovery from a failure, it must not be the place where one disappears — it reports it, once, and uploads
        // nothing; the caller's next smm_set_state goes through (tests/test_gpu_error_enumeration.py: every `... step ss` sequence lost its error here)
        (void)check_device_error(c);
        if (c->failed && !c->failed_told) { c->failed_told = true; return c->failed; }
        KParams& P = c->P;
        const size_t N = P.N, RW = P.RW, HW = P.HW, np = P.np, nm = P.nm;
        std::vector<double> cs(N * CSW), rec(N * RW, 0.0);
        HIPCHK(hipMemcpy(cs.data(), P.cs, cs.size() * 8, hipMemcpyDeviceToHost));  // keeps acc_tuner
        bool nan_seen = false;   // (NaN orders under no key: the lean walks are not launched from such a state, launch_chain_iter_norm)
        for (size_t i = 0; i < N; ++i) {
            double* b = cs.data() + i * CSW;
            double* r = rec.data() + i * RW;
            b[CS_SIGMA] = s->sigma[i]; b[CS_RATE] = s->accept_rate[i];
            b[CS_NNOEX] = (double)s->n_noex[i]; b[CS_NACC] = (double)s->n_acc_noex[i];
            b[CS_LACC] = 0.0; b[CS_WASX] = 0.0;
            b[CS_BEST] = s->best_val[i]; b[CS_BESTID] = (double)s->best_id[i];
            b[CS_BESTP] = s->best_val[i]; b[CS_BESTPID] = (double)s->best_id[i];
            r[0] = s->la_value[i]; r[1] = s->la_prob[i]; r[2] = (double)s->la_status[i];
            if (s->la_value[i] != s->la_value[i]) nan_seen = true;
            for (size_t k = 0; k < np; ++k) r[3 + k] = s->la_params[k * N + i];
            for (size_t k = 0; k < nm; ++k) r[3 + np + k] = s->la_sim_moments[k * N + i];
        }
        c->nan_values = nan_seen;
        HIPCHK(hipMemcpy(P.cs, cs.data(), cs.size() * 8, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(c->rec[c->run.cur], rec.data(), rec.size() * 8, hipMemcpyHostToDevice));
        std::vector<double> row(N * HW, 0.0);
        for (int t = 0; t < s->iter; ++t) {
            const size_t o = (size_t)t * N;
            for (size_t i = 0; i < N; ++i) {
                double* hr = row.data() + i * HW;
                history_head(hr, h->value[o + i], h->prob[o + i], h->curr_val[o + i], h->best_val[o + i], (double)h->best_id[o + i],
                             (double)h->exchanged[o + i], (double)h->accepted[o + i], (double)h->status[o + i]);
                for (size_t k = 0; k < np; ++k) hr[H_PARAMS + k] = h->params[((size_t)t * np + k) * N + i];
                for (size_t k = 0; k < nm; ++k) hr[H_PARAMS + np + k] = h->sim_moments[((size_t)t * nm + k) * N + i];
            }
            HIPCHK(hipMemcpy(P.hrec + (size_t)t * N * HW, row.data(), row.size() * 8, hipMemcpyHostToDevice));
        }
        c->run.iter = s->iter;
        if (c->failed) {   // a state from before the failure: the run may go on
            const unsigned long long e = ERR_NONE;
            HIPCHK(hipMemcpy(P.err, &e, 8, hipMemcpyHostToDevice));
            c->failed = 0; c->failed_told = false;
        }
        c->rec_external = false; c->pending_ext = false; c->run.unresolved = false;
        c->run.pending = false;
        c->run.prev_open = false;
        c->a2a_open = false;
        c->p2p_current = false;   // (the next smm_bgp_p2p_step publishes the uploaded state)
        c->run.exch_done = false;
        c->run.slots_iter = -1;
        if (P.walk_flags) HIPCHK(hipMemset(P.walk_flags, 0, 16));   // (the values the next exchange sees are written by the next accept step)
        return SMM_OK;
    });
}

int smm_get_timing(void* ctx, smm_timing_t* out) {
    Ctx* c = (Ctx*)ctx;
    if (!c || !out) return SMM_ERR_INVALID_ARG;
    *out = c->timing;
    return SMM_OK;
}

int smm_set_persistent(void* ctx, int32_t on) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return SMM_ERR_INVALID_ARG;
    c->persist_on = on ? 1 : 0;
    return SMM_OK;
}

int smm_get_persistent(void* ctx, int32_t* available, int32_t* launches, int32_t* repairs) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return SMM_ERR_INVALID_ARG;
    if (available) *available = (c->F.persist != PERSIST_NONE && c->persist_on && !c->persist_broken) ? 1 : 0;
    if (launches) *launches = c->persist_launches;
    if (repairs) *repairs = c->persist_repairs;
    return SMM_OK;
}

int smm_set_profiling(void* ctx, int32_t on) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return SMM_ERR_INVALID_ARG;
    c->profiling = on < 0 ? 0 : (on > 2 ? 2 : on);
    return SMM_OK;
}

// debug (not part of the public header): per-workgroup wall_clock64 stamps of the last k_chain_iter
int smm_debug_ts(void* ctx, unsigned long long* out, int n_wg) {
    Ctx* c = (Ctx*)ctx;
    if (!c || !c->P.ts) return SMM_ERR_INVALID_ARG;
    if (n_wg == -2) {  // k_chain_persist_loc's counts of the tiles that entered persist_late_tries, by iteration mod PL_LATE_N (PL_LATE_N words;
                       // never reset, not even at allocation: take differences — tools/late_tries_time.py)
        if (hipMemcpy(out, c->P.ts + PL_LATE_BASE, (size_t)PL_LATE_N * 8, hipMemcpyDeviceToHost) != hipSuccess) return SMM_ERR_HIP;
        return SMM_OK;
    }
    if (n_wg < 0) {  // the exchange kernel's stamps
        if (hipMemcpy(out, c->P.ts + (size_t)8 * 60000, 8 * 100, hipMemcpyDeviceToHost) != hipSuccess) return SMM_ERR_HIP;
        return SMM_OK;
    }
    if (hipMemcpy(out, c->P.ts, (size_t)n_wg * 8 * 8, hipMemcpyDeviceToHost) != hipSuccess) return SMM_ERR_HIP;
    return SMM_OK;
}
// debug (not part of the public header): k_chain_persist_loc's per-wave stamps of the simulation phase, [n_wg][16][PL_TSW] (tools/persist_waves.py)
int smm_debug_ts_waves(void* ctx, unsigned long long* out, int n_wg) {
    Ctx* c = (Ctx*)ctx;
    if (!c || !c->P.ts || n_wg < 0 || n_wg > PL_TSW_TILES) return SMM_ERR_INVALID_ARG;
    const size_t words = (size_t)n_wg * (NORM_WG / 64) * PL_TSW;
    if (hipMemcpy(out, c->P.ts + PL_TSW_BASE, words * 8, hipMemcpyDeviceToHost) != hipSuccess) return SMM_ERR_HIP;
    return SMM_OK;
}

#ifdef SMM_TEST_HOOKS
// debug (test build only, not part of the public header): the look-ahead window starting at iteration t, planned now; milliseconds of its
// kernels on the stream (tools/exp/shard_plan_time.py: what a shard of 8 x 4096 spends on its plan per window)
int smm_debug_plan_window(void* ctx, int t, double* ms_out, int* window_out) {
    return api_call(ctx, ms_out != nullptr, [&](Ctx* c) -> int {
        HIPCHK(hipSetDevice(c->device));
        hipEvent_t e0, e1;
        HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
        c->plan_w = 0;
        HIPCHK(hipEventRecord(e0, c->stream));
        ensure_windows(c, t, false);
        HIPCHK(hipEventRecord(e1, c->stream));
        HIPCHK(hipEventSynchronize(e1));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e0, e1));
        *ms_out = ms;
        if (window_out) *window_out = c->plan_w;
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
        return SMM_OK;
    });
}
// debug (test build only, not part of the public header): the cone of one tile in iteration plan_t0 + w of the current plan window
int smm_debug_cone(void* ctx, int w, int tile, uint32_t* hdr, uint32_t* pairs, uint16_t* gather, int32_t* info) {
    Ctx* c = (Ctx*)ctx;
    if (!c || !c->P.cone_hdr) return SMM_ERR_INVALID_ARG;
    const KParams& P = c->P;
    if (hipStreamSynchronize(c->stream) != hipSuccess) return SMM_ERR_HIP;
    if (hipMemcpy(hdr, P.cone_hdr + ((size_t)w * P.cone_tiles + tile) * CONE_HDRW, CONE_HDRW * 4, hipMemcpyDeviceToHost) != hipSuccess) return SMM_ERR_HIP;
    if (hipMemcpy(pairs, P.cone_pairs + ((size_t)w * P.cone_tiles + tile) * (CONE_LEVELS * 64), CONE_LEVELS * 64 * 4, hipMemcpyDeviceToHost) != hipSuccess) return SMM_ERR_HIP;
    if (P.cone_gather && hipMemcpy(gather, P.cone_gather + ((size_t)w * P.cone_tiles + tile) * CONE_GCAP, CONE_GCAP * 2, hipMemcpyDeviceToHost) != hipSuccess) return SMM_ERR_HIP;
    uint32_t ok = 0;
    if (hipMemcpy(&ok, P.cone_ok + w, 4, hipMemcpyDeviceToHost) != hipSuccess) return SMM_ERR_HIP;
    info[0] = c->plan_t0; info[1] = c->plan_w; info[2] = (int32_t)ok; info[3] = P.cone_ct;
    return SMM_OK;
}
#endif

int smm_get_Z(void* ctx, double* Z) {
    return api_call(ctx, Z != nullptr, [&](Ctx* c) -> int {
        HIPCHK(hipSetDevice(c->device));
        for (int k = 0; k < c->P.nm; ++k)
            HIPCHK(hipMemcpy(Z + (size_t)k * c->P.ns, c->P.Z + (size_t)k * c->P.zstride, (size_t)c->P.ns * sizeof(double),
                             hipMemcpyDeviceToHost));
        return SMM_OK;
    });
}

}  // extern "C"
