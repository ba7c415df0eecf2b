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
// k_exch_plan), smm_exchange.hpp (stand-alone exchange kernels), this file (host: contexts, forms, choosers, windows, the call frame), smm_run_host.hpp (the run's host side:
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
// Which stand-alone kernel resolves exchangeMoves! (AlgoBGP.jl:647-716) — ONE decision, taken once per context (select_forms),
// from the population, the thresholds and dist_fun:
//
//   N_global        min_improve                      dist_fun   kernel                       slots / where
//   <= 8192 (~7400) one value >= 0 for all chains    -          k_exch_resolve_lean          8-byte keys (0) or 16-byte values (> 0), LDS
//   <= 4096         anything else                    any        k_exch_resolve_lvl<1024>     16-byte slots, LDS
//   <= 8192         anything else                    any        k_exch_resolve_lvl_soa       split slots, LDS
//   <= 32768        0 for all chains                 -          k_exch_keys + _rows          4-byte slots (17-bit keys), rows of 1024 pairs, LDS
//   <= 32768        anything else                    -          k_exch_keys + _key           4-byte slots (16-bit keys, intervals), LDS
//   <= 65535        anything else / other dist_fun   any        k_exch_resolve_lvl_big       16-byte slots, global memory
//   above, or K > N_global                           any        k_exch_resolve_any           barrier rounds, global atomics
//
// (the p2p form of a sharded run launches k_exch_resolve_rows itself where this table says _rows — launch_resolve_rows_window:
//  <., true> reads the tagged slots of its window instead of a key pre-pass, <false, true, true> keeps the partners of the rank's
//  own chains only; every other p2p population resolves from the window's plain values through this table.)
// (single shards of objfunc_norm up to 4096 chains do not get here in steady state: their chain kernel walks inline.)  The test
// build can force an entry (SMM_TEST_HOOKS: Hooks) and adds the ticket kernel k_exch_resolve_lds.
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
    uint32_t *win_lv_pairs = nullptr, *win_lv_off = nullptr, *win_lv_pairs_p = nullptr, *win_lv_offp = nullptr;
    uint32_t *win_lv_rows = nullptr, *win_lv_rowinfo = nullptr, *slots17 = nullptr, *nan_flags = nullptr;
    double* win_lv_mi = nullptr;
    uint32_t* big_scratch = nullptr;
    int rng_t0 = 0, rng_w = 0;    // window currently held: iterations [t0, t0+w)
    int plan_t0 = 0, plan_w = 0;
    uint32_t* cb_scratch = nullptr;
    std::vector<uint32_t> cone_big_ok;   // per iteration of the plan window: its cones fit their caps
    // ... their windows are planned AHEAD: the plan of a window depends on (seed, iteration) only, so while the chain kernels of one
    // window run, the three plan kernels of the next run beside them on a second stream into the other of two sets of tables
    struct PlanSet {
        uint32_t *lv_pairs = nullptr, *lv_off = nullptr, *lv_rows = nullptr, *lv_rowinfo = nullptr, *cone_ok = nullptr, *cone_hdr = nullptr, *cone_pairs = nullptr;
        double* lv_mi = nullptr;
        uint16_t* cone_gather = nullptr;
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
    int profiling = 0;   // 1: event brackets around the kernels; 2: the kernels' own begin/end timestamps (launch)
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

// a kernel onto the context's stream; in profiling mode 2 with the begin/end of this dispatch as the command processor stamps them
template <class Kern, class... Args>
void launch(Ctx* c, Kern kern, dim3 grid, dim3 block, size_t smem, const Args&... args) {
    if (c->kev0) hipExtLaunchKernelGGL(kern, grid, block, smem, c->stream, c->kev0, c->kev1, 0, args...);
    else hipLaunchKernelGGL(kern, grid, block, smem, c->stream, args...);
}

bool is_sim(int obj) { return obj == SMM_OBJ_NORM || obj == SMM_OBJ_NORM_FAILBOX; }
int obj_kind(int obj) { return is_sim(obj) ? 1 : obj == SMM_OBJ_DENSE ? 2 : 0; }
// ... as the LDS layouts see it: 3 = the dense objective's spec v2 (SMM_OBJ_DENSE2: internally SMM_OBJ_DENSE with the 256 x 256 stage's
// operand set; its first hidden layer is staged in the partial sums' region)
int lay_kind(const Ctx* c);

// the two value arrays (and slot arrays) alternate by iteration: reads of iteration t_read's values, writes of iteration t_write's
void point_values(const Ctx* c, KParams& P, int t_read, int t_write) {
    P.vals = c->vals_buf[t_read & 1]; P.vals_out = c->vals_buf[t_write & 1];
    P.slot8 = c->slot8_buf[t_read & 1]; P.slot8_out = c->slot8_buf[t_write & 1];
}

size_t tile_smem_base(const Ctx* c, int ct) {
    const KParams& P = c->P;
    return tile_smem_doubles(ct, P.np, P.nm, P.RW, P.HW, P.RBW, lay_kind(c)) * sizeof(double);
}
int lay_kind(const Ctx* c) { const int k = obj_kind(c->obj); return k == 2 && c->P.dense_A2f ? 3 : (c->obj == SMM_OBJ_USER && c->u_lanes > 0) ? 4 : k; }
// dynamic LDS of k_chain_persist_tile for this context (a user objective's wave totals: 16 chains x lanes / 64 groups x its sums)
size_t persist_tile_smem(const Ctx* c) {
    const KParams& P = c->P;
    return pt_layout(P.np, P.nm, P.RW, P.HW, P.RBW, lay_kind(c), P.dense_nOt, PT_CT * (c->u_lanes / 64) * c->u_nsums).total;
}
// tiles (workgroups) of one rank's launch of F's persistent kernel: k_chain_persist_gen has PG_CT chains per tile (whole tiles),
// k_chain_persist_loc NORM_CT, k_chain_persist_tile PT_CT
int persist_tiles_rank(const Forms& F, int N) {
    if (F.persist == PERSIST_GEN) return N / PG_CT;
    const int ct = F.persist == PERSIST_TILE ? PT_CT : NORM_CT;
    return (N + ct - 1) / ct;
}
size_t norm_smem(const Ctx* c) {   // k_chain_iter_norm: [walk: chain slots | pair list] theta, partial sums, parked state
    const size_t b = (size_t)c->P.tile_off * sizeof(double) + norm_tile_doubles(c->P.np) * sizeof(double);
    return c->F.cone_big ? std::max(b, cone_local_lds_bytes()) : b;   // (the local cone walk lies UNDER the tile's blocks)
}
size_t tile_smem(const Ctx* c, int ct, int tpw = 1) {   // dynamic LDS of k_chain_iter: tpw tiles; with the inline exchange
    if (c->F.norm_fast) return norm_smem(c);
    const size_t base = tile_smem_base(c, ct);           // walk its chain slots in front and its pair list under the tiles
    const size_t tiles = (size_t)tpw * ((base + 15) & ~(size_t)15);
    if (!c->F.inline_walk) return tiles;
    if (c->F.dense_keys) return std::max(tiles, (size_t)(((c->P.Ng + 3) & ~3) + 4) * 8 + std::max((size_t)CONE_LEVELS * 64 * 4, (size_t)lean_walk_Kp(c->P.plan_K) * 4));
    if (c->F.gen_keys) return (size_t)(((c->P.Ng + 3) & ~3) + 4) * 8 + std::max(tiles, (size_t)lean_walk_Kp(c->P.plan_K) * 4);
    return c->F.gen_lean ? tile_lean_slot_bytes(c->P.Ng) + std::max(tiles, (size_t)lean_walk_Kp(c->P.plan_K) * 4)
                       : walk_slot_bytes(c->P.Ng) + std::max(tiles, (size_t)c->P.plan_K * 4);
}
size_t plan_lds_bytes(int Ng, int K) { return (size_t)(Ng + 2) * 4 + (size_t)K * 8 + (size_t)K * 4 + 128 + 16; }
#ifdef SMM_TEST_HOOKS
size_t resolve_lds_bytes(int Ng) { return (size_t)Ng * 16 + 16; }
#endif
size_t resolve_lvl_soa_bytes(int Ng, int K) { return (size_t)Ng * 12 + (size_t)K * 4 + 16; }
size_t resolve_lvl_bytes(int Ng, int K) { return (size_t)Ng * 16 + (size_t)K * 12 + 64 * 8 + 64; }

int exchange_K(const Ctx* c) { return c->P.pairtab ? c->P.n_pairs_tab : n_exchange_pairs(c->P.Ng); }
bool exchange_active(const Ctx* c, int t) { return t >= c->exchange_from && c->P.Ng > 1; }  // AlgoBGP.jl:637

void launch_cone_big(Ctx* c, const KParams& Pw, int W, const uint32_t* lv_pairs, const uint32_t* lv_off, hipStream_t st) {
    hipLaunchKernelGGL(k_cone_chains, dim3(W), dim3(XWG), (size_t)Pw.Ng * 4, st, Pw, lv_pairs, lv_off, c->cb_scratch);
    hipLaunchKernelGGL(k_cone_tiles, dim3((unsigned)(((Pw.cone_tiles + CONEB_WAVES - 1) / CONEB_WAVES) * ((W + 7) & ~7))), dim3(64 * CONEB_WAVES), cone_tiles_lds_bytes(Pw.plan_K),
                       st, Pw, W, (const uint32_t*)c->cb_scratch);
    HIPCHK(hipGetLastError());
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
    hipLaunchKernelGGL(k_exch_plan_big, dim3(W), dim3(XWG), plan_big_lds_bytes(Pw.Ng), c->pstream, Pw, t, c->big_scratch, S.lv_pairs, S.lv_mi, S.lv_off, S.lv_rows, S.lv_rowinfo);
    launch_cone_big(c, Pw, W, S.lv_pairs, S.lv_off, c->pstream);
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
        hipLaunchKernelGGL(k_exch_plan_big, dim3(W), dim3(XWG), plan_big_lds_bytes(P.Ng), c->stream, P, t, c->big_scratch, c->win_lv_pairs, c->win_lv_mi,
                           c->win_lv_off, c->win_lv_rows, c->win_lv_rowinfo);
        c->plan_t0 = t; c->plan_w = W;
        P.plan_t0 = t;
        if (c->F.cone_big) {   // the tiles' locally numbered cones, from the plan's scratch (pairs in list order, their levels)
            launch_cone_big(c, P, W, c->win_lv_pairs, c->win_lv_off, c->stream);
            // a cone that does not fit its caps (a pair list of very deep dependency chains: the user's, or an unlucky sample) sends its
            // iteration to the stand-alone resolution: the host looks at the window's flags once (one synchronisation per window)
            c->cone_big_ok.resize((size_t)W);
            HIPCHK(hipMemcpyAsync(c->cone_big_ok.data(), P.cone_ok, (size_t)W * 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
        } else if (c->F.persist_sh_big) {   // (the persistent kernel looks at the window's flags itself: no synchronisation)
            launch_cone_big(c, P, W, c->win_lv_pairs, c->win_lv_off, c->stream);
        }
        P.lv_rows = c->win_lv_rows; P.lv_rowinfo = c->win_lv_rowinfo;
        P.lv_pairs = c->win_lv_pairs; P.lv_mi = c->win_lv_mi; P.lv_off = c->win_lv_off;
    }
    if (c->F.plan == PLAN_LDS && P.Ng > 1 && !(t >= c->plan_t0 && t < c->plan_t0 + c->plan_w)) {
        const int W = std::min(c->F.plan_cap, P.T - t + 1);
        hipLaunchKernelGGL(k_exch_plan, dim3(W), dim3(XWG), (c->F.cone || c->F.persist != PERSIST_NONE) ? std::max(plan_lds_bytes(P.Ng, P.plan_K), plan_cone_bytes()) : plan_lds_bytes(P.Ng, P.plan_K), c->stream, P, t, c->win_plan,
                           c->win_plan_mi, c->win_lv_pairs, c->win_lv_mi, c->win_lv_off, c->win_lv_pairs_p, c->win_lv_offp);
        c->plan_t0 = t; c->plan_w = W;
        P.plan = c->win_plan; P.plan_mi = c->win_plan_mi; P.plan_t0 = t;
        P.lv_pairs = c->win_lv_pairs; P.lv_mi = c->win_lv_mi; P.lv_off = c->win_lv_off;
        P.lv_pairs_p = c->win_lv_pairs_p; P.lv_offp = c->win_lv_offp;
    }
}

// ---- which per-iteration chain kernel (smm_chain.hpp, smm_chain_norm.hpp) ----
// Every instantiation of the chain kernels' templates that a launch can take is named in chain_instance() and nowhere else: chain_kernel()
// and chain_kernel_p2p() pick one for a launch, smm_ctx_create raises the dynamic LDS limit of every one of them, smm_describe prints the
// pick's name.  A new instantiation is one line in chain_instance() (a new family: one more name in ChainFamily).
// (name: what smm_describe's chain= says; block: lanes of a workgroup; ct: chains per tile; tpw: tiles per workgroup)
struct ChainKernel { const void* fn; const char* name; unsigned block; int ct, tpw; };
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
    if (c->obj == SMM_OBJ_DENSE && P.dense_A2f) K.name = "iter<dense2,16>";
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
// K over the chains of P onto the context's stream, with `smem` bytes of dynamic LDS: every kernel of these families takes (P, t, rec_in,
// rec_out, flags); in profiling mode 2 with the begin/end of this dispatch as the command processor stamps them
void launch_chain_kernel(Ctx* c, const ChainKernel& K, size_t smem, const KParams& P, int t, const double* rec_in, double* rec_out, int flags) {
    const dim3 grid((unsigned)(((P.N + K.ct - 1) / K.ct + K.tpw - 1) / K.tpw)), block(K.block);
    void* args[] = {(void*)&P, (void*)&t, (void*)&rec_in, (void*)&rec_out, (void*)&flags};
    if (c->kev0) HIPCHK(hipExtLaunchKernel(K.fn, grid, block, args, smem, c->stream, c->kev0, c->kev1, 0));
    else HIPCHK(hipLaunchKernel(K.fn, grid, block, args, smem, c->stream));
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
    const size_t smem = tile_smem(c, K.ct, K.tpw);
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

size_t resolve_lean_bytes(int Ng, int K, bool wide) { return std::max(wide ? lean_wide_bytes(Ng, K) : lean_walk_bytes(Ng, K), resolve_lvl_soa_bytes(Ng, K)); }

void launch_resolve_p(Ctx* c, const KParams& P, int t, const double* gathered);
void launch_resolve(Ctx* c, int t, const double* gathered) { launch_resolve_p(c, c->P, t, gathered); }
// (P: the context's parameters, or a copy whose RW is the stride of the value column in `gathered`)
void launch_resolve_p(Ctx* c, const KParams& P_in, int t, const double* gathered) {
    KParams P = P_in;
    point_values(c, P, t, t);   // (single shard: the values the accept step of iteration t wrote)
    switch ((ExchKernel)c->F.xk) {
    case XK_LEAN:
        launch(c, k_exch_resolve_lean, dim3(1), dim3(XWG), resolve_lean_bytes(P.Ng, P.plan_K, P.lean_wide != 0), P, t, gathered);
        break;
    case XK_LVL:
#ifdef SMM_TEST_HOOKS
        if (c->H.lvl_wg == 256) { hipLaunchKernelGGL(k_exch_resolve_lvl<256>, dim3(1), dim3(256), resolve_lvl_bytes(P.Ng, P.plan_K), c->stream, P, t, gathered); break; }
        if (c->H.lvl_wg == 512) { hipLaunchKernelGGL(k_exch_resolve_lvl<512>, dim3(1), dim3(512), resolve_lvl_bytes(P.Ng, P.plan_K), c->stream, P, t, gathered); break; }
#endif
        launch(c, k_exch_resolve_lvl<1024>, dim3(1), dim3(1024), resolve_lvl_bytes(P.Ng, P.plan_K), P, t, gathered);
        break;
    case XK_LVL_SOA:
        hipLaunchKernelGGL(k_exch_resolve_lvl_soa<1024>, dim3(1), dim3(1024), resolve_lvl_soa_bytes(P.Ng, P.plan_K), c->stream, P, t, gathered);
        break;
    case XK_TICKETS:
#ifdef SMM_TEST_HOOKS
        hipLaunchKernelGGL(k_exch_resolve_lds, dim3(1), dim3(XWG), resolve_lds_bytes(P.Ng), c->stream, P, t, gathered);
#endif
        break;
    case XK_ROWS:
    case XK_KEY: {
        // values and initial slots by the whole chip (gathered records: their value column; single shard: the compact array)
        const double* src = gathered ? gathered : (const double*)P.vals;
        double* vals = gathered ? P.xval : P.vals;
        if (gathered || c->run.slots_iter != t)   // (a single shard's accept step of iteration t has made the slots already)
            hipLaunchKernelGGL(k_exch_keys, dim3((P.Ng + 255) / 256), dim3(256), 0, c->stream, src, gathered ? P.RW : 1, P.Ng, vals,
                               (uint32_t*)P.xsrc, c->F.xk == XK_ROWS ? c->slots17 : (uint32_t*)nullptr, c->nan_flags, t);
        const bool plds = P.Ng <= XKEY_PARTNER_MAX;   // partners in LDS, else the ballot replay
        const uint32_t* slots16 = (gathered || c->run.slots_iter != t) ? (const uint32_t*)P.xsrc : (const uint32_t*)nullptr;
        if (c->F.xk == XK_ROWS && plds)
            hipLaunchKernelGGL(k_exch_resolve_rows<true>, dim3(1), dim3(XWG), resolve_rows_bytes(P.Ng, P.plan_K, P.rows_cap), c->stream, P, t,
                               (const double*)vals, slots16, (const uint32_t*)c->slots17, c->nan_flags);
        else if (c->F.xk == XK_ROWS)
            hipLaunchKernelGGL(k_exch_resolve_rows<false>, dim3(1), dim3(XWG), resolve_rows_bytes(P.Ng, P.plan_K, P.rows_cap), c->stream, P, t,
                               (const double*)vals, slots16, (const uint32_t*)c->slots17, c->nan_flags);
        else if (plds)
            hipLaunchKernelGGL(k_exch_resolve_key<true>, dim3(1), dim3(XWG), resolve_key_bytes(P.Ng, P.plan_K), c->stream, P, t,
                               (const double*)vals, (const uint32_t*)P.xsrc);
        else
            hipLaunchKernelGGL(k_exch_resolve_key<false>, dim3(1), dim3(XWG), resolve_key_bytes(P.Ng, P.plan_K), c->stream, P, t,
                               (const double*)vals, (const uint32_t*)P.xsrc);
        break;
    }
    case XK_LVL_BIG:
        hipLaunchKernelGGL(k_exch_resolve_lvl_big, dim3(1), dim3(XWG), 0, c->stream, P, t, gathered);
        break;
    case XK_ANY:
        hipLaunchKernelGGL(k_exch_resolve_any, dim3(1), dim3(XWG), 0, c->stream, P, t, gathered);
        break;
    }
}

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
// the same straight from the tagged slots and self-validating values of the window (p2p form of large norm populations): no wait,
// no unpacking, no key pre-pass in front of k_exch_resolve_rows
void launch_resolve_rows_window(Ctx* c, int t) {
    const KParams& P = c->P;
    // a shard of a population past XKEY_PARTNER_MAX: partners of its own chains only, written by the swaps (no second pass over the rows)
    const bool own = P.Ng > XKEY_PARTNER_MAX && P.N < P.Ng && resolve_rows_bytes(P.Ng, P.plan_K, P.rows_cap, P.N) <= (size_t)158 * 1024;
    if (own) {
        const size_t sm = resolve_rows_bytes(P.Ng, P.plan_K, P.rows_cap, P.N);
        launch(c, k_exch_resolve_rows<false, true, true>, dim3(1), dim3(XWG), sm, P, t, (const double*)nullptr, (const uint32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr);
        return;
    }
    const size_t smem = resolve_rows_bytes(P.Ng, P.plan_K, P.rows_cap);
    if (P.Ng <= XKEY_PARTNER_MAX) {
        launch(c, k_exch_resolve_rows<true, true>, dim3(1), dim3(XWG), smem, P, t, (const double*)nullptr, (const uint32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr);
    } else {
        launch(c, k_exch_resolve_rows<false, true>, dim3(1), dim3(XWG), smem, P, t, (const double*)nullptr, (const uint32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr);
    }
}
// ---- the persistent chain kernels (smm_chain_persist*.hpp) ----
// what launches F's persistent kernel: a kernel of the library (fn) or of a user objective's module (mfn: loaded by persist_occupancy),
// its grid, block and dynamic LDS.  persist_occupancy sets its LDS attribute and asks for its occupancy, launch_chain_persist launches it,
// smm_describe prints its name.
struct PersistKernel { const void* fn; hipFunction_t mfn; dim3 grid, block; size_t smem; const char* name; };
PersistKernel persist_kernel(const Ctx* c, const Forms& F) {
    const KParams& P = c->P;
    PersistKernel K{nullptr, nullptr, dim3(persist_tiles_rank(F, P.N)), dim3(1), 0, "none"};
    if (F.persist == PERSIST_GEN) {
        K.block = dim3(1024);
        K.smem = persist_gen_smem_bytes(P.Ng, P.np, P.RW, P.HW) + (F.persist_user ? persist_gen_user_bytes() : 0);
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
               : P.dense_A2f ? (F.persist_sh ? "tile_dense2_shard" : "tile_dense2") : (F.persist_sh ? "tile_dense_shard" : "tile_dense");
        if (c->obj == SMM_OBJ_USER) K.mfn = c->pfn;   // (the same kernel, compiled with the user's map-reduce objective inside: user_tile_compile)
        else if (F.persist_sh) K.fn = dense ? (const void*)k_chain_persist_tile<2, false, true> : (const void*)k_chain_persist_tile<1, false, true>;
        else if (P.chol_L && P.mi_pct) K.fn = dense ? (const void*)k_chain_persist_tile<2, true, false, true> : (const void*)k_chain_persist_tile<1, true, false, true>;
        else if (P.chol_L) K.fn = dense ? (const void*)k_chain_persist_tile<2, false, false, true> : (const void*)k_chain_persist_tile<1, false, false, true>;
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
    else if (c->kev0) HIPCHK(hipExtLaunchKernel(K.fn, K.grid, K.block, args, K.smem, c->stream, c->kev0, c->kev1, 0));
    else HIPCHK(hipLaunchKernel(K.fn, K.grid, K.block, args, K.smem, c->stream));
}

// ---- the forms of a context (smm_ctx_create) ----
// what the device says about a context's forms: its compute units, and the resident workgroups per CU of the one persistent kernel
// that is the candidate (-1: not asked yet — select_forms then names the candidate; 0: it is not available, its user kernel did not compile)
struct DeviceFacts { int n_cus = 256; int per_cu = -1; };

// Every form a context runs, from the problem (c->P, c->obj, the user objective's lanes, the injected tables), the hooks and the device.
// Decides and allocates nothing.  The order of preference between the persistent forms: gen -> gen_user -> gen_small / user -> loc /
// shard -> tile, each only where none before it was taken.
Forms select_forms(const Ctx* c, const Hooks& H, const DeviceFacts& dev) {
    const KParams& P = c->P;
    const int np = P.np, nm = P.nm, ns = P.ns, N = P.N, Ng = P.Ng, K = P.plan_K, n_cus = dev.n_cus;
    const bool user_obj = c->obj == SMM_OBJ_USER, minus = P.dist_fun == SMM_DIST_MINUS, chol = P.chol_L != nullptr;
    const bool mi0 = P.mi_uniform && P.mi_value == 0.0;   // one threshold 0 for all chains
    Forms F;
    // the level plan in LDS, or in global memory
    bool lds = Ng > 1 && Ng <= XLDS_MAX && K >= 1 && K <= Ng && !H.any_exchange;
    bool lvl = lds && Ng <= XLVL_MAX && !H.dataflow;
    bool lvl_soa = lds && !lvl && !H.dataflow;
    // (... and a SHARD whose population is past what the lean plan's 16-byte walk holds in LDS — one min_improve > 0 for all chains of
    // 7400 < N_global <= 8192, e.g. 2 x 4096 with the reference's default threshold —: the global-memory plan lists its tiles' cones,
    // locally numbered, so that the shard can still take the persistent form)
    const bool shard_wide_big = N < Ng && lds && P.mi_uniform && P.mi_value != 0.0 && !(P.mi_value < 0.0) && minus &&
                                resolve_lean_bytes(Ng, K, true) > (size_t)160 * 1024;
    const bool big = Ng > 1 && Ng <= 65535 && K >= 1 && K <= Ng && !H.any_exchange && (H.big_exchange || shard_wide_big || !lds);
    if (big) lds = lvl = lvl_soa = false;
    const bool key = big && Ng <= XKEY_MAX && K <= XKEY_MAX && !H.key_exchange_off && minus;   // (the keys order value_i - value_j)
    F.plan = big ? PLAN_BIG : lds ? PLAN_LDS : PLAN_NONE;
    // inline exchange walk: single shard, level plan available, and two tiles must still share a CU's 160 KB LDS
    const int tile_ct = is_sim(c->obj) ? F.ct : (c->obj == SMM_OBJ_DENSE ? 16 : 8);
    const size_t tile_b = (tile_smem_base(c, tile_ct) + 15) & ~(size_t)15;
    F.norm_fast = is_sim(c->obj) && np == nm && np <= 4 && P.batch_size == np && P.dbg == 0 && !chol && !H.norm_fast_off;
    // more tiles than CUs: the walk-free kernel on half-size workgroups, two to a CU (k_chain_iter_norm_narrow)
    F.norm_narrow = F.norm_fast && ((N + NORM_CT - 1) / NORM_CT > n_cus || H.norm_narrow == 1) && H.norm_narrow != 0;
    // k_chain_iter_norm: pair list NOT overlaid; room for either walk (16-byte slots, 4-byte slots + value table)
    const bool wide_form = P.mi_uniform && P.mi_value != 0.0 && !(P.mi_value < 0.0);   // (the lean walk on 16-byte slots, below)
    const size_t walk_b = std::max(walk_slot_bytes(Ng) + (((size_t)K * 4 + 15) & ~(size_t)15),
                                   ((wide_form ? lean_wide_bytes(Ng, K) : lean_walk_bytes(Ng, K)) + 15) & ~(size_t)15);
    F.inline_walk = !H.inline_walk_off && lvl && N == Ng && !user_obj &&
                    (!F.norm_fast || minus) &&   // (k_chain_iter_norm's walks are for `-`)
                    (F.norm_fast ? walk_b + norm_tile_doubles(np) * 8 <= (size_t)160 * 1024
                                 : walk_slot_bytes(Ng) + std::max(tile_b, (size_t)K * 4) <= (size_t)80 * 1024);
    F.tile_off = F.inline_walk ? (int)((F.norm_fast ? walk_b : walk_slot_bytes(Ng)) / sizeof(double)) : 0;
    // (the lean plan: the same conditions as below)
    const bool lean_plan = P.mi_uniform && !(P.mi_value < 0.0) && minus && K <= XLDS_MAX && !H.key_walk_off &&
                           (P.mi_value == 0.0 || resolve_lean_bytes(Ng, K, true) <= (size_t)160 * 1024);
    // two tiles per workgroup share one walk (the 2p/2m-style simulation tile of 8 chains only) — worth it only when two tiles would
    // share a CU anyway (more tiles than CUs)
    F.tpw = (F.inline_walk && !F.norm_fast && (is_sim(c->obj) ? F.ct == 8 : c->obj != SMM_OBJ_DENSE) && ((N + 7) / 8 > n_cus || H.tpw == 2) &&
             H.tpw != 1 && walk_slot_bytes(Ng) + std::max(2 * tile_b, (size_t)K * 4) <= (size_t)160 * 1024) ? 2 : 1;
    // k_chain_iter on the lean walk (16-byte slots, padded pair list): where its somewhat larger LDS keeps the same budget
    F.gen_lean = F.inline_walk && !F.norm_fast && lean_plan &&
                 tile_lean_slot_bytes(Ng) + std::max((size_t)F.tpw * tile_b, (size_t)lean_walk_Kp(K) * 4) <= (size_t)(F.tpw == 2 ? 160 : 80) * 1024;
    if (F.gen_lean) F.tile_off = (int)(tile_lean_slot_bytes(Ng) / sizeof(double));
    // single shards of 4096 < N <= 8192 chains without a simulation (banana, BASELINE config 4): the key walk inline, two
    // 16-chain tiles per workgroup of 1024 lanes (256 workgroups at 8192 chains: one per CU, one launch per iteration)
    const size_t tile16 = (tile_smem_base(c, 16) + 15) & ~(size_t)15;
    const size_t slots = (size_t)(((Ng + 3) & ~3) + 4) * 8;
    F.gen_keys = !F.inline_walk && !H.inline_walk_off && obj_kind(c->obj) == 0 && !user_obj && N == Ng && Ng > XLVL_MAX &&
                 Ng <= XLDS_MAX && K <= XLDS_MAX && lds && mi0 && minus && !H.key_walk_off &&
                 slots + std::max(2 * tile16, (size_t)lean_walk_Kp(K) * 4) <= (size_t)160 * 1024;
    if (F.gen_keys) { F.inline_walk = true; F.tpw = 2; F.tile_off = (int)(slots / sizeof(double)); }
    // the dense objective (BASELINE config 5): its tile fills a CU's LDS (143 KB at 50 parameters / 50 moments), so the key
    // walk's slots and lists lie UNDER the tile's blocks — the walk is over before anything of the tile is written
    F.dense_keys = !F.inline_walk && !H.inline_walk_off && !H.dense_keys_off && c->obj == SMM_OBJ_DENSE && N == Ng &&
                   Ng >= 2 && Ng <= XLVL_MAX && K <= XLVL_MAX && lds && mi0 && minus && !H.key_walk_off && lean_walk_unit(Ng) == 8 &&
                   std::max(tile16, slots + std::max((size_t)CONE_LEVELS * 64 * 4, (size_t)lean_walk_Kp(K) * 4)) <= (size_t)160 * 1024;
    if (F.dense_keys) { F.gen_keys = true; F.inline_walk = true; F.tpw = 1; F.tile_off = 0; }

    // the candidates for the persistent chain kernel and the cone tables behind the plan
    // the workgroups' cones of the inline key walk (smm_cone.hpp): where k_chain_iter walks 8192 chains' keys in every workgroup
    const bool want_cone = F.gen_keys && !H.no_cone && (F.dense_keys ? (N % 16 == 0 && N / 16 <= 256) : (F.tpw == 2 && N % 32 == 0 && N / 32 <= 256));
    const int cone_ct = F.dense_keys ? 16 : 32;
    const bool gen_ok = np <= PG_MAXP && nm <= PG_MAXP && P.batch_size == np && !chol && N == Ng && !c->deep_plan && P.dbg == 0 && !H.persist_off;
    const bool gen_fits = persist_gen_smem_bytes(Ng, np, P.RW, P.HW) <= (size_t)160 * 1024;
    // k_chain_persist_gen (smm_chain_persist_gen.hpp), objectives without a simulation: where k_chain_iter walks its workgroups'
    // cones inline (4096 < N <= 8192 in whole workgroups of 32 chains, one per CU), one proposal batch, isotropic proposals
    const bool want_gen = want_cone && !F.dense_keys && c->obj == SMM_OBJ_BANANA && gen_ok && N / PG_CT <= n_cus && gen_fits;
    // ... and for the smaller populations of the same objective (up to 4096 chains in whole groups of 32: VERDICT r4 "banana at 2048
    // chains takes the per-iteration path"): the same kernel — the cones are listed behind the lean plan whether or not the
    // per-iteration kernel walks them
    const bool gen_small_ok = gen_ok && N % PG_CT == 0 && N / PG_CT >= 1 && N / PG_CT <= n_cus && lds && mi0 && minus && K <= XLDS_MAX;
    const bool want_gen_small = !want_cone && c->obj == SMM_OBJ_BANANA && F.inline_walk && gen_small_ok && gen_fits;
    // ... and a USER objective (one thread per evaluation) in the same loop: the kernel compiled with the user's source inside
    // (user_persist_compile)
    const bool want_user = user_obj && c->u_lanes == 0 && gen_small_ok &&
                           persist_gen_smem_bytes(Ng, np, P.RW, P.HW) + persist_gen_user_bytes() <= (size_t)160 * 1024;
    // ... and on LOCALLY NUMBERED cones (smm_chain_persist_loc.hpp): the same objective with one threshold >= 0 (or NaN: nothing
    // ever swaps) for all chains — min_improve > 0 is the reference's default (AlgoBGP.jl:522) —, whatever the population's size
    // does to the tile's LDS
    const bool mi_ok = (P.mi_uniform && !(P.mi_value < 0.0)) || P.mi_pct;   // one threshold >= 0 (or NaN) for all chains, or one per chain, each >= 0 (or NaN)
    const bool loc_ok = F.norm_fast && np <= 2 && ns <= WG * PR_ZR && minus && !c->deep_plan && P.dbg == 0 && !H.persist_off && !H.persist_loc_off;
    const bool want_loc = loc_ok && N == Ng && Ng >= 2 && F.inline_walk && mi_ok && K <= XLDS_MAX && Ng <= XLDS_MAX && (N + NORM_CT - 1) / NORM_CT <= n_cus;
    // ... and as a shard of a sharded run (one process per GPU: smm_bgp_p2p_step): the same kernel, the ring in the ranks' windows
    const bool want_sh = loc_ok && N < Ng && N > 0 && Ng % N == 0 && P.offset % N == 0 && Ng / N <= P2P_MAXG && N % NORM_CT == 0 &&
                         P.mi_uniform && !(P.mi_value < 0.0) && N / NORM_CT <= n_cus &&
                         (lds ? K <= XLDS_MAX : (big && Ng <= 32768 && K <= 65535 && (size_t)Ng * 4 <= (size_t)160 * 1024));
    // ... and for the objectives a whole tile evaluates (smm_chain_persist_tile.hpp): objfunc_norm with any number of parameters — the
    // reference's larger examples have 6 and 18, Examples.jl:210-230, 232-319 — and the dense simulation (BASELINE config 5); one
    // threshold >= 0 (or NaN) for all chains, isotropic proposals or a Cholesky factor (the kernel's CH form: no LDS of its own), one 16-chain
    // tile per workgroup, all of them resident
    const int tile_kind = obj_kind(c->obj);
    // ... and a USER objective in its map-reduce form (smm_register_user_objective_lanes) whose lanes are a whole share of the tile's 512
    const bool user_tile = user_obj && c->u_lanes > 0 && c->u_lanes <= WG && WG % c->u_lanes == 0 && PT_CT % (WG / c->u_lanes) == 0 && !P.mi_pct;   // (compiled for ONE threshold)
    const bool want_tile = (tile_kind == 1 || tile_kind == 2 || user_tile) && !(F.norm_fast && np <= 2 && ns <= WG * PR_ZR) && N == Ng && Ng >= 2 && lds &&
                           mi_ok && minus && K <= XLDS_MAX && Ng <= XLDS_MAX && !c->deep_plan && P.dbg == 0 && !H.persist_off &&
                           !H.persist_tile_off && P.RW <= PT_LPC * PT_NJ && (tile_kind != 2 || N % PT_CT == 0) && (N + PT_CT - 1) / PT_CT <= 2 * n_cus &&
                           persist_tile_smem(c) <= (size_t)160 * 1024;
    // ... and as a shard of a sharded run (smm_bgp_p2p_step; SH of smm_chain_persist_tile.hpp): equal shards of whole tiles, the LDS plan
    // (N_global <= 8192: every rank's progress words fit wave 2's 512 lanes' worth), one threshold >= 0 (or NaN) for all chains
    const bool want_tile_sh = (tile_kind == 1 || tile_kind == 2 || user_tile) && !(F.norm_fast && np <= 2 && ns <= WG * PR_ZR) &&
                              N < Ng && N > 0 && Ng % N == 0 && P.offset % N == 0 && Ng / N <= P2P_MAXG && N % PT_CT == 0 && lds &&
                              Ng <= XLDS_MAX && K <= XLDS_MAX && P.mi_uniform && !(P.mi_value < 0.0) && !P.mi_pct && minus && !c->deep_plan && !chol &&
                              P.dbg == 0 && !H.persist_off && !H.persist_tile_off && P.RW <= PT_LPC * PT_NJ && N / PT_CT <= 2 * n_cus &&
                              persist_tile_smem(c) <= (size_t)160 * 1024;
    const size_t persist_tiles = (want_gen || want_gen_small || want_user) ? (size_t)N / PG_CT : (size_t)(N + NORM_CT - 1) / NORM_CT;
    // large single shards of objfunc_norm (C3 on one GPU): the narrow chain kernel's tiles walk their own, locally numbered cones
    // (smm_cone_big.hpp) instead of waiting for the one-workgroup resolution between two launches
    const bool rows = key && mi0 && !H.key_walk_off;
    const bool want_cone_big = big && rows && F.norm_fast && F.norm_narrow && N == Ng && N % NORM_CT == 0 && Ng <= 32768 && K <= 65535 &&
                               P.dbg == 0 && !H.cone_big_off && (size_t)Ng * 4 <= (size_t)160 * 1024;

    // look-ahead windows.  Two with budgets of their own (288 GB of HBM: a few hundred MiB of look-ahead tables are nothing), at most 256
    // iterations each.  The plan kernels are launched with one workgroup per iteration of the window: a short window leaves
    // the chip idle while they run — at 32768 chains k_exch_plan_big needs 1.7 ms per launch, which with the 26 iterations the
    // former common budget of 192 MiB allowed was 63 us per iteration, more than the exchange itself (round 3, rocprofv3).
    // (the plan's budget counts the tables of every candidate, taken or not)
    const bool pregen = !(F.norm_fast && !P.user_ntab && !P.user_utab);   // (k_chain_iter_norm draws in the kernel)
    const size_t rb_iter = (size_t)P.RBW * N * 8;
    const size_t cone_iter = (size_t)(CONE_LEVELS * 64 + CONE_HDRW) * 4;   // one tile's header and sub-levels
    const size_t plan_iter = (want_cone_big ? (size_t)(N / NORM_CT) * (cone_iter + CONE_GCAP * 2) + cone_big_scratch_words(Ng, K) * 4 : 0) + (size_t)K * 36 +
                             (big ? BigPlanScratch::words(Ng, K) * 4 + (size_t)(XROWS_MAX + 1) * XWG * 4 : 0) +
                             (size_t)lean_walk_Kp(K) * 4 + 1024 + (want_cone ? (size_t)(N / cone_ct) * cone_iter + 4 : 0) +
                             ((want_loc || want_sh || want_tile || want_tile_sh) ? persist_tiles * (cone_iter + CONE_GCAP * 2) + 4 : 0) +
                             ((want_sh && big) ? cone_big_scratch_words(Ng, K) * 4 : 0) +
                             (want_gen ? persist_tiles * (CONE_GCAP * 2) : 0) +
                             ((want_gen_small || want_user) ? persist_tiles * (cone_iter + CONE_GCAP * 2) + 4 : 0);
    F.win_cap = pregen ? (int)std::max<size_t>(1, std::min<size_t>(256, ((size_t)768 << 20) / rb_iter)) : 1;
    F.win_cap = std::min(F.win_cap, P.T);
    F.plan_cap = (int)std::max<size_t>(1, std::min<size_t>(256, ((size_t)1536 << 20) / plan_iter));
    F.plan_cap = std::max(1, std::min(std::min(F.plan_cap, P.T), H.plan_cap));

    // the exchange: the big plan's forms
    if (big && rows) {
        F.rows_cap = std::min(XROWS_MAX, (K + XWG - 1) / XWG + LV_MAXLEV);
        if (want_cone_big) { F.cone_big = true; F.plan_ahead = !H.plan_ahead_off; F.walk_slots = true; }
    }
    if (big && want_sh) {   // a shard of a large population: its own tiles' cones, locally numbered (smm_cone_big.hpp)
        F.persist = PERSIST_LOC; F.persist_wide = P.mi_value != 0.0; F.persist_sh = true; F.persist_sh_big = true;
    }
    // ... the lean walk (smm_walk_lean.hpp) behind the LDS plan: one min_improve for every chain — 0: 8-byte slots of order keys; > 0 (or
    // NaN: nothing ever swaps): 16-byte slots of values, as far as the 160 KB of LDS reach (~7400 chains)
    // (thresholds by chain: the lean PLAN — padded levels on 16-byte units, the tiles' cones behind it — is made for the persistent launches; the
    // stand-alone lean resolution and the inline lean walks, which test ONE threshold, stay off: XK_LEAN below, launch_chain_iter_norm)
    const bool wide = P.mi_uniform && !mi0 && !(P.mi_value < 0.0) && resolve_lean_bytes(Ng, K, true) <= (size_t)160 * 1024;
    const bool pct = P.mi_pct != 0 && (want_loc || want_tile);
    F.lean_plan = lds && (mi0 || wide || pct) && K <= XLDS_MAX && !H.key_walk_off && minus;
    F.lean_wide = F.lean_plan && (wide || pct);
    if (F.lean_plan) {
        // ... walked in the prologue of k_chain_iter_norm, or of k_chain_iter (key form)
        if (mi0 && ((F.norm_fast && F.inline_walk && Ng <= XLVL_MAX && K <= XLVL_MAX) || F.gen_keys)) {
            F.walk_slots = true;
            F.cone = want_cone;
            if (want_gen) F.persist = PERSIST_GEN;
        }
        const bool user_ok = want_user && mi0 && F.persist == PERSIST_NONE;
        if ((want_gen_small || user_ok) && mi0 && F.persist == PERSIST_NONE) {
            F.persist = PERSIST_GEN; F.persist_user = user_ok; F.defer_resolve = user_ok;
        }
        if ((want_loc || want_sh) && F.persist == PERSIST_NONE && F.norm_fast) {   // (k_exch_plan lists the tiles' cones behind the lean plan)
            F.persist = PERSIST_LOC; F.persist_wide = wide || pct; F.persist_sh = want_sh;
        }
        // (the dense tiles of the per-iteration kernel walk the same cones: want_cone above)
        if (want_tile && F.persist == PERSIST_NONE &&
            (!F.cone || (cone_ct == PT_CT && (size_t)(N / cone_ct) == (size_t)(N + PT_CT - 1) / PT_CT))) {
            F.persist = PERSIST_TILE; F.persist_wide = true;
            F.defer_resolve = !F.inline_walk;   // (the exchange of an iteration is left to the next launch: it may be this kernel's)
        }
        if (want_tile_sh && F.persist == PERSIST_NONE) { F.persist = PERSIST_TILE; F.persist_wide = true; F.persist_sh = true; }
    }
    // ... all of its tiles resident at once, or it is not taken (per_cu 0 also where a user objective's kernel did not compile)
    if (F.persist != PERSIST_NONE && dev.per_cu >= 0) {
        const int tiles = persist_tiles_rank(F, N);
        if (F.persist != PERSIST_GEN) F.max_tiles = dev.per_cu * n_cus;
        if (tiles > dev.per_cu * n_cus) {
            F.persist = PERSIST_NONE;
            F.persist_wide = F.persist_sh = F.persist_sh_big = F.persist_user = F.defer_resolve = false;
        }
    }
    // the cone tables: the persistent form's (with gather lists), the local cones', or the inline key walk's
    if (F.cone_big) { F.cone_tiles = N / NORM_CT; F.cone_ct = NORM_CT; F.cone_gather = true; }
    else if (F.persist == PERSIST_GEN) { F.cone_tiles = N / PG_CT; F.cone_ct = PG_CT; F.cone_gather = true; }
    else if (F.persist == PERSIST_LOC) { F.cone_tiles = (int)persist_tiles; F.cone_ct = NORM_CT; F.cone_gather = true; }
    else if (F.persist == PERSIST_TILE) { F.cone_tiles = (N + PT_CT - 1) / PT_CT; F.cone_ct = PT_CT; F.cone_gather = true; }
    else if (F.cone) { F.cone_tiles = N / cone_ct; F.cone_ct = cone_ct; }

    // the stand-alone resolution
    F.xk = (F.lean_plan && !pct) ? XK_LEAN : lvl ? XK_LVL : lvl_soa ? XK_LVL_SOA : lds ? XK_TICKETS   // (XK_TICKETS: test build only, SMMHIP_DATAFLOW_EXCHANGE)
         : key ? (rows ? XK_ROWS : XK_KEY) : big ? XK_LVL_BIG : XK_ANY;
    return F;
}

// the persistent kernel that is the candidate of F, asked how many of its workgroups a CU holds — with its dynamic LDS set first, as the
// launches want it; a user objective's kernel is compiled (once per registered objective) and loaded here.  0: not available
int persist_occupancy(Ctx* c, const Forms& F, int objective_id) {
    if (F.persist_user || (F.persist == PERSIST_TILE && c->obj == SMM_OBJ_USER)) {   // (user_persist_compile / user_tile_compile)
        const bool tile = F.persist == PERSIST_TILE;
        {
            std::lock_guard<std::mutex> lock(g_user_mutex);
            UserObjective& u = g_user_objectives[objective_id - SMM_OBJ_USER_BASE];
            const bool chol = tile && !F.persist_sh && c->P.chol_L != nullptr;   // (select_forms gives a shard with a factor no persistent form)
            if (!(tile ? user_tile_compile(u, F.persist_sh, chol) : user_persist_compile(u))) {
                if (getenv("SMMHIP_VERBOSE"))
                    fprintf(stderr, "libsmmhip: the persistent form of this user objective is not available:\n%s\n",
                            (tile ? (chol ? u.tile_chol_log : F.persist_sh ? u.tile_sh_log : u.tile_log) : u.persist_log).c_str());
                return 0;
            }
            HIPCHK(hipModuleLoadData(&c->pmod, (tile ? (chol ? u.tile_chol_code : F.persist_sh ? u.tile_sh_code : u.tile_code) : u.persist_code).data()));
        }
        HIPCHK(hipModuleGetFunction(&c->pfn, c->pmod, tile ? "smm_user_persist_tile_kernel" : "smm_user_persist_kernel"));
    }
    const PersistKernel K = persist_kernel(c, F);
    int per_cu = 0;
    if (K.mfn) {
        // (a module's function: not every runtime takes the attribute this way; the launch asks for what it needs)
        (void)hipFuncSetAttribute((const void*)K.mfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)K.smem);
        (void)hipGetLastError();
        HIPCHK(hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, K.mfn, K.block.x, K.smem));
    } else {
        HIPCHK(hipFuncSetAttribute(K.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)K.smem));
        HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, K.fn, K.block.x, K.smem));
    }
    return per_cu;
}

// one set of cone tables for the plan window (KParams or a PlanSet): tiles x CONE_HDRW header words, tiles x the sub-levels' pairs and,
// with_gather, tiles x the gather lists, per iteration; cone_ok zeroed
template <class Tables>
void alloc_cones(Ctx* c, Tables& P, size_t tiles, bool with_gather) {
    const size_t W = (size_t)c->F.plan_cap;
    P.cone_ok = dalloc<uint32_t>(c, W);
    P.cone_hdr = dalloc<uint32_t>(c, W * tiles * CONE_HDRW);
    P.cone_pairs = dalloc<uint32_t>(c, W * tiles * (CONE_LEVELS * 64) + 1024);   // (+: whole 1 KB pieces are fetched)
    P.cone_gather = with_gather ? dalloc<uint16_t>(c, W * tiles * CONE_GCAP + 512) : nullptr;
    HIPCHK(hipMemset((void*)P.cone_ok, 0, W * 4));
}

// the persistent form's ring — one window (pr_win_layout; a shard's lives in its p2p window: smm_bgp_p2p_init) — and the state
// persist_repair rolls back to (after the history's fill: hist_fill is a row of it)
void alloc_persist(Ctx* c) {
    KParams& P = c->P;
    const size_t N = P.N;
    if (!c->F.persist_sh) {
        const PrWin WL = pr_win_layout(P.Ng, P.RW, 1, persist_tiles_rank(c->F, P.N));
        c->prw = dalloc<unsigned char>(c, WL.total);
        HIPCHK(hipMemset(c->prw, 0, WL.total));
    }
    c->snap_cs = dalloc<double>(c, N * CSW);
    c->snap_rec = dalloc<double>(c, N * P.RW);
    for (int b = 0; b < 2; ++b) { c->snap_vals[b] = dalloc<double>(c, N + 4); c->snap_slot8[b] = dalloc<uint2>(c, N + 4 + 128); }
    c->snap_xres = dalloc<unsigned long long>(c, P.Ng);
    c->hist_fill = dalloc<double>(c, N * P.HW);
    HIPCHK(hipMemcpy(c->hist_fill, P.hrec, N * P.HW * 8, hipMemcpyDeviceToDevice));   // (a row of the constructor's fill)
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

void smm_ctx_destroy(void* ctx) {
    Ctx* c = (Ctx*)ctx;
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->pstream) { (void)hipStreamSynchronize(c->pstream); (void)hipStreamDestroy(c->pstream); }
    if (c->ev_free) (void)hipEventDestroy(c->ev_free);
    for (Ctx::PlanSet& S : c->ps) { if (S.done) (void)hipEventDestroy(S.done); if (S.ok_host) (void)hipHostFree(S.ok_host); }
    for (void* p : c->allocs) (void)hipFree(p);
    for (void* w : c->p2p_opened) if (w) (void)hipIpcCloseMemHandle(w);
    if (c->p2p_mine) (void)hipFree(c->p2p_mine);
    if (c->st_scr) (void)hipFree(c->st_scr);
    if (c->red_res) (void)hipFree(c->red_res);
    if (c->umod) (void)hipModuleUnload(c->umod);
    if (c->pmod) (void)hipModuleUnload(c->pmod);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    for (hipEvent_t e : c->pev) (void)hipEventDestroy(e);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int smm_ctx_create(const smm_problem_t* prob, const smm_bgp_opts_t* opts, const smm_tables_t* tab, void** out) {
    if (!prob || !opts || !out) return fail(nullptr, SMM_ERR_INVALID_ARG, "null argument");
    const int np = prob->np, nm = prob->nm, ns = prob->ns, N = opts->N, T = opts->maxiter, Ng = opts->N_global;
    if (np < 1 || nm < 1 || ns < 1 || np > MAX_DIM || nm > MAX_DIM)
        return fail(nullptr, SMM_ERR_INVALID_ARG, "need 1 <= np,nm <= 64 and ns >= 1");
    if (N < 1 || T < 1 || Ng < N || opts->chain_offset < 0 || opts->chain_offset + N > Ng || (Ng % N) != 0)
        return fail(nullptr, SMM_ERR_INVALID_ARG, "bad N / N_global / chain_offset / maxiter");
    const bool user_obj = prob->objective_id >= SMM_OBJ_USER_BASE;
    if (user_obj) {
        std::lock_guard<std::mutex> lock(g_user_mutex);
        if (prob->objective_id - SMM_OBJ_USER_BASE >= (int)g_user_objectives.size())
            return fail(nullptr, SMM_ERR_INVALID_ARG, "unknown user objective handle");
    } else if (prob->objective_id < 0 || (prob->objective_id > SMM_OBJ_DENSE && prob->objective_id != SMM_OBJ_DENSE2))
        return fail(nullptr, SMM_ERR_INVALID_ARG, "unknown objective_id");
    if (is_sim(prob->objective_id) && np != nm)
        return fail(nullptr, SMM_ERR_INVALID_ARG, "objfunc_norm needs one moment per parameter (ObjExamples.jl:66-78)");
    if (opts->batch_size < 1 || opts->batch_size > np || (np % opts->batch_size) != 0)
        return fail(nullptr, SMM_ERR_BAD_BATCH, "batch_size must divide the number of parameters (AlgoBGP.jl:95-103)");
    if (opts->sigma_update_steps < 1) return fail(nullptr, SMM_ERR_INVALID_ARG, "sigma_update_steps < 1");
    if (opts->smpl_iters < 1) return fail(nullptr, SMM_ERR_INVALID_ARG, "smpl_iters < 1 (AlgoBGP.jl:521: at least one proposal try)");
    // the exchange of iteration t reads the history of iteration t-1: the reference starts at algo.i >= 2 (AlgoBGP.jl:637)
    if (opts->exchange_from_iter < 2) return fail(nullptr, SMM_ERR_INVALID_ARG, "exchange_from_iter < 2 (AlgoBGP.jl:637)");
    if (!prob->init || !prob->lb || !prob->ub || !prob->mom || !prob->w)
        return fail(nullptr, SMM_ERR_INVALID_ARG, "smm_problem_t: init / lb / ub / mom / w must not be NULL");
    if (!opts->sigma || !opts->acc_tuner || !opts->min_improve)
        return fail(nullptr, SMM_ERR_INVALID_ARG, "smm_bgp_opts_t: sigma / acc_tuner / min_improve must not be NULL (length N_global)");
    if (prob->n_obj_params > 0 && !prob->obj_params) return fail(nullptr, SMM_ERR_INVALID_ARG, "n_obj_params > 0 but obj_params is NULL");
    if (tab && tab->pairs && tab->n_pairs > 0) {   // injected pair lists: 0 <= i < j < N_global (16-bit packing in the plans)
        for (size_t q = 0; q < (size_t)T * tab->n_pairs; ++q) {
            const int32_t i = tab->pairs[2 * q], j = tab->pairs[2 * q + 1];
            if (i < 0 || j <= i || j >= Ng) return fail(nullptr, SMM_ERR_INVALID_ARG, "smm_tables_t.pairs: need 0 <= i < j < N_global");
        }
    }
    if (tab && tab->prop_normals && tab->prop_tries < 1) return fail(nullptr, SMM_ERR_INVALID_ARG, "prop_normals given but prop_tries < 1");
    if (opts->dist_fun < SMM_DIST_MINUS || opts->dist_fun > SMM_DIST_RELDIFF)
        return fail(nullptr, SMM_ERR_INVALID_ARG, "smm_bgp_opts_t.dist_fun: SMM_DIST_MINUS, SMM_DIST_ABSDIFF or SMM_DIST_RELDIFF");
    if (opts->chol_L && opts->batch_size != np)
        return fail(nullptr, SMM_ERR_BAD_BATCH, "Cholesky proposals (chol_L) draw all parameters in one batch: batch_size must equal np");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(nullptr, SMM_ERR_NO_DEVICE, "no HIP device available: libsmmhip has no CPU fallback");
    if (opts->device < 0 || opts->device >= ndev) return fail(nullptr, SMM_ERR_INVALID_ARG, "bad device ordinal");
    Ctx* c = new Ctx();
    try {
        c->H = read_hooks();
        c->device = opts->device;
        HIPCHK(hipSetDevice(c->device));
        HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        HIPCHK(hipEventCreate(&c->ev0));
        HIPCHK(hipEventCreate(&c->ev1));
        KParams& P = c->P;
        c->obj = user_obj ? SMM_OBJ_USER : prob->objective_id == SMM_OBJ_DENSE2 ? SMM_OBJ_DENSE : prob->objective_id;   // (spec v2: the dense kind with P.dense_A2f set)
        c->exchange_from = opts->exchange_from_iter;
        P.exch_from = opts->exchange_from_iter;
        {
            const char* d = getenv("SMMHIP_DBG");
            P.dbg = d ? atoi(d) : 0;
            P.scout_after = c->H.scout_after;
            P.scout_gl = c->H.scout_gl;
            const char* tsv = getenv("SMMHIP_TS");
            if (tsv && (tsv[0] == '1' || tsv[0] == '2')) P.ts = dalloc<unsigned long long>(c, (size_t)8 * 65536);
            P.ts_levels = tsv && tsv[0] == '2';   // also a stamp per level of the inline walk (the stamps stretch the levels: not with '1')
        }
        P.np = np; P.nm = nm; P.ns = ns; P.obj = c->obj;
        P.init = dupload(c, prob->init, np); P.lb = dupload(c, prob->lb, np); P.ub = dupload(c, prob->ub, np);
        P.mom = dupload(c, prob->mom, nm); P.w = dupload(c, prob->w, nm);
        P.objp = prob->n_obj_params > 0 ? dupload(c, prob->obj_params, prob->n_obj_params) : nullptr;
        c->n_objp = prob->n_obj_params > 0 ? prob->n_obj_params : 0;
        if (user_obj) {
            {
                std::lock_guard<std::mutex> lock(g_user_mutex);
                const UserObjective& u = g_user_objectives[prob->objective_id - SMM_OBJ_USER_BASE];
                HIPCHK(hipModuleLoadData(&c->umod, u.code.data()));
                c->u_lanes = u.lanes; c->u_nsums = u.n_sums; c->u_rng = u.rng;
            }
            HIPCHK(hipModuleGetFunction(&c->ufn, c->umod, "smm_user_eval_kernel"));
            if (c->u_rng) HIPCHK(hipModuleGetFunction(&c->ufn_noseed, c->umod, "smm_user_eval_noseed_kernel"));
            P.u_theta = dalloc<double>(c, (size_t)N * np);
            P.u_simM = dalloc<double>(c, (size_t)N * nm);
            P.u_value = dalloc<double>(c, N);
            P.u_status = dalloc<int>(c, N);
        }
        if (prob->objective_id == SMM_OBJ_DENSE || prob->objective_id == SMM_OBJ_DENSE2) {
            const bool v2 = prob->objective_id == SMM_OBJ_DENSE2;   // [B, A2, A]: with the 256 x 256 stage
            const size_t nB = (size_t)DENSE_D * np, n2 = v2 ? (size_t)DENSE_D * DENSE_D : 0, nA = (size_t)nm * DENSE_D;
            if (prob->n_obj_params != 0 && (size_t)prob->n_obj_params != nB + n2 + nA)
                throw std::string(v2 ? "SMM_OBJ_DENSE2: obj_params must hold B (256 x np), A2 (256 x 256) and A (nm x 256), or be empty"
                                     : "SMM_OBJ_DENSE: obj_params must hold B (256 x np) and A (nm x 256), or be empty");
            std::vector<double> M(nB + n2 + nA);
            if (prob->n_obj_params) memcpy(M.data(), prob->obj_params, M.size() * 8);
            else {  // N(0,1)/sqrt(fan-in) from the counter RNG, stream 5
                for (size_t i = 0; i < M.size(); i += 2) {
                    double z0, z1;
                    box_muller(philox_stream(opts->seed, 5, (uint32_t)(i >> 1), (uint32_t)((i >> 1) >> 32), 0, 0), z0, z1);
                    M[i] = z0 / sqrt(i < nB ? (double)np : (double)DENSE_D);
                    if (i + 1 < M.size()) M[i + 1] = z1 / sqrt(i + 1 < nB ? (double)np : (double)DENSE_D);
                }
            }
            const int nPs = (np + 3) / 4, nOt = (nm + 15) / 16;
            std::vector<double> Bf((size_t)(DENSE_D / 16) * nPs * 64, 0.0), Af((size_t)nOt * (DENSE_D / 16) * 4 * 64, 0.0);
            for (int T = 0; T < DENSE_D / 16; ++T)
                for (int s = 0; s < nPs; ++s)
                    for (int l = 0; l < 64; ++l) {
                        const int d = 16 * T + (l & 15), p = 4 * s + (l >> 4);
                        if (p < np) Bf[((size_t)T * nPs + s) * 64 + l] = M[(size_t)d * np + p];
                    }
            for (int o = 0; o < nOt; ++o)
                for (int T = 0; T < DENSE_D / 16; ++T)
                    for (int s = 0; s < 4; ++s)
                        for (int l = 0; l < 64; ++l) {
                            const int k = 16 * o + (l & 15), d = 16 * T + 4 * s + (l >> 4);
                            if (k < nm) Af[(((size_t)o * (DENSE_D / 16) + T) * 4 + s) * 64 + l] = M[nB + n2 + (size_t)k * DENSE_D + d];
                        }
            P.dense_Bf = dupload(c, Bf.data(), Bf.size());
            P.dense_Af = dupload(c, Af.data(), Af.size());
            P.dense_nOt = nOt;
            if (v2) {   // A2 in fragment order [wave][k-step][lane][the wave's two row tiles] (smm_chain.hpp: dense2_tile_n)
                std::vector<double> A2f((size_t)DENSE_D * DENSE_D);
                for (int wv = 0; wv < 8; ++wv)
                    for (int s = 0; s < DENSE_D / 4; ++s)
                        for (int l = 0; l < 64; ++l)
                            for (int tt = 0; tt < 2; ++tt) {
                                const int j = 16 * (2 * wv + tt) + (l & 15), d = 4 * s + (l >> 4);
                                A2f[(((size_t)wv * (DENSE_D / 4) + s) * 64 + l) * 2 + tt] = M[nB + (size_t)j * DENSE_D + d];
                            }
                P.dense_A2f = dupload(c, A2f.data(), A2f.size());
            }
        }
        {
            const int rows = (ns + WG - 1) / WG;
            P.zstride = ((rows + ZU) / ZU) * ZU * WG;  // at least one chunk beyond the last full one
            std::vector<double> Z((size_t)nm * P.zstride, 0.0);
            for (int k = 0; k < nm; ++k)
                for (int s = 0; s < ns; ++s)
                    Z[(size_t)k * P.zstride + s] = (tab && tab->Z) ? tab->Z[(size_t)k * ns + s] : rng_Z(opts->seed, (uint32_t)k, (uint32_t)s);
            P.Z = dupload(c, Z.data(), Z.size());
        }
        P.N = N; P.Ng = Ng; P.offset = opts->chain_offset; P.T = T;
        P.sigma_update_steps = opts->sigma_update_steps; P.smpl_iters = opts->smpl_iters;
        P.batch_size = opts->batch_size; P.sigma_adjust_by = opts->sigma_adjust_by; P.seed = opts->seed;
        P.min_improve_g = dupload(c, opts->min_improve, Ng);
        if (opts->chol_L) {
            P.chol_per_chain = opts->chol_per_chain ? 1 : 0;
            P.chol_L = dupload(c, opts->chol_L, (size_t)(P.chol_per_chain ? Ng : 1) * np * np);
        }
        P.dist_fun = opts->dist_fun;
        P.mi_uniform = 1; P.mi_value = opts->min_improve[0];
        for (int i = 1; i < Ng; ++i)
            if (!(opts->min_improve[i] == P.mi_value || (opts->min_improve[i] != opts->min_improve[i] && P.mi_value != P.mi_value))) P.mi_uniform = 0;   // (NaN everywhere is one threshold too: nothing ever swaps)
        // per-chain thresholds (what the reference's API takes: opts["min_improve"] is a vector, AlgoBGP.jl:522): the persistent forms walk them too
        // (a threshold per slot position, smm_walk_lean.hpp PCT) while this context's single iterations keep the forms they had (the level walk on any
        // thresholds): every threshold >= 0 or NaN (the dummy pair's 0 - 0 must not exceed it), dist_fun = `-`
        P.mi_pct = 0;
        if (!P.mi_uniform && opts->dist_fun == SMM_DIST_MINUS) {
            P.mi_pct = 1;
            for (int i = 0; i < Ng; ++i) if (opts->min_improve[i] < 0.0) P.mi_pct = 0;
        }
        const size_t TN = (size_t)T * N;
        if (tab && tab->probs_acc) P.user_utab = dupload(c, tab->probs_acc, TN);
        if (tab && tab->prop_normals && tab->prop_tries > 0) {
            P.rb_tries = tab->prop_tries; P.user_n = 1;
            P.user_ntab = dupload(c, tab->prop_normals, TN * (size_t)tab->prop_tries * np);
        } else {
            // tries of mysample whose normals are made ahead of time (k_pregen_rng); later ones come from the generator inside the chain
            // kernel, ~1.4 us per try and tile.  Past 8 parameters: two (C4, 10 parameters: four cost 9 % — 398 -> 433 M chain-evals/s
            // with two, 447 with one; a first try outside the support is rare, a second one rarer)
            P.rb_tries = np <= 8 ? 8 : 2;
        }
        if ((size_t)P.rb_tries * (size_t)((np + 1) / 2) * (size_t)N >= ((size_t)1 << 31))   // (k_pregen_rng indexes one iteration's pieces in 32 bits)
            throw std::string("injected proposal normals: tries x parameters x chains of one iteration must stay below 2^31 pieces");
        if (tab && tab->pairs && tab->n_pairs > 0) {
            P.n_pairs_tab = tab->n_pairs;
            P.pairtab = dupload(c, tab->pairs, (size_t)T * tab->n_pairs * 2);
            {   // dependency depth of the injected lists (pairs sharing a chain keep their order): the lean walks hold LV_MAXLEV levels
                std::vector<int> last((size_t)Ng);
                for (int it = 0; it < T && !c->deep_plan; ++it) {
                    std::fill(last.begin(), last.end(), 0);
                    for (int q = 0; q < tab->n_pairs; ++q) {
                        const int32_t i = tab->pairs[2 * ((size_t)it * tab->n_pairs + q)], j = tab->pairs[2 * ((size_t)it * tab->n_pairs + q) + 1];
                        const int lv = std::max(last[i], last[j]) + 1;
                        last[i] = last[j] = lv;
                        if (lv > LV_MAXLEV) { c->deep_plan = true; break; }
                    }
                }
            }
        }
        P.RW = even_up(3 + np + nm);
        P.HW = even_up(H_PARAMS + np + nm);
        P.RBW = even_up(1 + P.rb_tries * np);
        const int K = exchange_K(c);
        P.plan_K = K;
        // the forms: the device's compute units, then the candidate persistent kernel's occupancy, then the choice
        DeviceFacts dev;
        (void)hipDeviceGetAttribute(&dev.n_cus, hipDeviceAttributeMultiprocessorCount, c->device);
        c->F = select_forms(c, c->H, dev);
        if (c->F.persist != PERSIST_NONE) {
            dev.per_cu = persist_occupancy(c, c->F, prob->objective_id);
            c->F = select_forms(c, c->H, dev);
        }
        const Forms& F = c->F;
        P.tile_off = F.tile_off;
        P.gen_lean = F.gen_keys ? 2 : F.gen_lean ? 1 : 0;
        P.rows_cap = F.rows_cap;
        // the look-ahead tables
        c->win_rb = dalloc<double>(c, (size_t)F.win_cap * N * P.RBW);
        HIPCHK(hipMemset(c->win_rb, 0, (size_t)F.win_cap * N * P.RBW * 8));
        const size_t W = (size_t)F.plan_cap;
        if (F.plan != PLAN_NONE) {
            c->win_lv_pairs = dalloc<uint32_t>(c, W * K);
            c->win_lv_mi = dalloc<double>(c, W * K);
            c->win_lv_off = dalloc<uint32_t>(c, W * (K + 2));
        }
        if (F.plan == PLAN_BIG) c->big_scratch = dalloc<uint32_t>(c, W * BigPlanScratch::words(Ng, K));
        if (F.xk == XK_ROWS) {
            c->win_lv_rows = dalloc<uint32_t>(c, W * P.rows_cap * XWG);
            c->win_lv_rowinfo = dalloc<uint32_t>(c, W * 4);
            c->slots17 = dalloc<uint32_t>(c, (size_t)Ng + 4);
            c->nan_flags = dalloc<uint32_t>(c, 4);
            HIPCHK(hipMemset(c->nan_flags, 0, 16));
        }
        if (F.plan == PLAN_LDS) {
            c->win_plan = dalloc<unsigned long long>(c, W * K);
            c->win_plan_mi = dalloc<double>(c, W * K);
        }
        if (F.lean_plan) {
            P.lean_wide = F.lean_wide ? 1 : 0;
            P.plan_Kp = lean_walk_Kp(K);
            P.lean_unit = F.lean_wide ? lean_wide_unit(Ng) : lean_walk_unit(Ng);
            c->win_lv_pairs_p = dalloc<uint32_t>(c, W * P.plan_Kp + 512);   // (+512: whole 1 KB pieces may be read past the last iteration's words)
            c->win_lv_offp = dalloc<uint32_t>(c, W * LV_OFFP);
        }
        if (F.walk_slots) {   // the lean key walk's slots, written by the accept step
            for (int b = 0; b < 2; ++b) c->slot8_buf[b] = dalloc<uint2>(c, (size_t)N + 4 + 128);
            P.slot8 = c->slot8_buf[0];
            P.walk_flags = dalloc<uint32_t>(c, 4);
            HIPCHK(hipMemset(P.walk_flags, 0, 16));
        }
        if (F.cone_tiles) {
            P.cone_tiles = F.cone_tiles; P.cone_ct = F.cone_ct;
            alloc_cones(c, P, (size_t)F.cone_tiles, F.cone_gather);
        }
        if (F.cone_big || F.persist_sh_big) c->cb_scratch = dalloc<uint32_t>(c, W * cone_big_scratch_words(Ng, K));
        if (F.plan_ahead) {   // the big plan's second set of tables (the first: the window's own)
            HIPCHK(hipStreamCreateWithFlags(&c->pstream, hipStreamNonBlocking));
            HIPCHK(hipEventCreateWithFlags(&c->ev_free, hipEventDisableTiming));
            Ctx::PlanSet& S0 = c->ps[0];
            S0.lv_pairs = c->win_lv_pairs; S0.lv_mi = c->win_lv_mi; S0.lv_off = c->win_lv_off; S0.lv_rows = c->win_lv_rows; S0.lv_rowinfo = c->win_lv_rowinfo;
            S0.cone_ok = (uint32_t*)P.cone_ok; S0.cone_hdr = (uint32_t*)P.cone_hdr; S0.cone_pairs = (uint32_t*)P.cone_pairs; S0.cone_gather = P.cone_gather;
            Ctx::PlanSet& S1 = c->ps[1];
            S1.lv_pairs = dalloc<uint32_t>(c, W * K);
            S1.lv_mi = dalloc<double>(c, W * K);
            S1.lv_off = dalloc<uint32_t>(c, W * (K + 2));
            S1.lv_rows = dalloc<uint32_t>(c, W * P.rows_cap * XWG);
            S1.lv_rowinfo = dalloc<uint32_t>(c, W * 4);
            alloc_cones(c, S1, (size_t)F.cone_tiles, true);
            for (Ctx::PlanSet& S : c->ps) {
                HIPCHK(hipHostMalloc((void**)&S.ok_host, W * 4, hipHostMallocDefault));
                HIPCHK(hipEventCreateWithFlags(&S.done, hipEventDisableTiming));
            }
        }
        {   // chain state blocks and records (BGPChain ctor, AlgoBGP.jl:78-109: best = Inf, best_id = -1, ...)
            std::vector<double> cs((size_t)N * CSW, 0.0);
            for (int i = 0; i < N; ++i) {
                double* b = cs.data() + (size_t)i * CSW;
                b[CS_SIGMA] = opts->sigma[opts->chain_offset + i];
                b[CS_BEST] = INFINITY; b[CS_BESTID] = -1.0; b[CS_BESTP] = INFINITY; b[CS_BESTPID] = -1.0;
                b[CS_ATUN] = opts->acc_tuner[opts->chain_offset + i];
            }
            P.cs = dupload(c, cs.data(), cs.size());
            std::vector<double> rec((size_t)N * P.RW, 0.0);
            for (int i = 0; i < N; ++i) rec[(size_t)i * P.RW] = INFINITY;  // value: Inf until the first accept
            for (int b = 0; b < 2; ++b) c->rec[b] = dupload(c, rec.data(), rec.size());
        }
        P.xres = dalloc<unsigned long long>(c, Ng);
        if (N > 0 && Ng % N == 0 && opts->chain_offset % N == 0) {   // equal shards: the values form of the sharded exchange is available
            c->a2a_G = Ng / N;
            c->a2a_cap = c->H.a2a_cap ? c->H.a2a_cap : a2a_capacity(N, c->a2a_G);
            c->a2a_send_idx = dalloc<int32_t>(c, (size_t)c->a2a_G * c->a2a_cap);
            c->a2a_send_cnt = dalloc<int32_t>(c, (size_t)c->a2a_G);
            c->a2a_rowidx = dalloc<int32_t>(c, (size_t)N);
        }
        for (int b = 0; b < 2; ++b) c->vals_buf[b] = dalloc<double>(c, (size_t)N + 4);   // (+4: read as 16-byte pieces)
        P.vals = c->vals_buf[0];
        if (F.plan != PLAN_LDS) {
            const int Kmax = std::max(K, 1);
            P.xval = dalloc<double>(c, Ng); P.xnext = dalloc<int32_t>(c, Ng); P.xpairs = dalloc<int32_t>(c, (size_t)Kmax * 2);
            P.xsrc = dalloc<int32_t>(c, Ng); P.xpartner = dalloc<int32_t>(c, Ng);
            P.xslot = dalloc<double>(c, (size_t)Ng * 2);
        }
        {   // history: NaN values, curr/best = Inf, best_id = -1, exchanged = accepted = status = 0
            std::vector<double> row((size_t)N * P.HW, NAN);
            for (int i = 0; i < N; ++i) history_head(row.data() + (size_t)i * P.HW, NAN, NAN, INFINITY, INFINITY, -1.0, 0.0, 0.0, 0.0);
            P.hrec = dalloc<double>(c, TN * P.HW);
            // (one row from the host, then doubling copies on the device: a long history — bench.py's repetitions hold 50 000 iterations — is filled
            // at HBM speed instead of row by row over PCIe)
            HIPCHK(hipMemcpy(P.hrec, row.data(), row.size() * 8, hipMemcpyHostToDevice));
            for (size_t have = 1; have < (size_t)T; have *= 2) {
                const size_t n = std::min(have, (size_t)T - have);
                HIPCHK(hipMemcpy(P.hrec + have * N * P.HW, P.hrec, n * N * P.HW * 8, hipMemcpyDeviceToDevice));
            }
        }
        P.err = dalloc<unsigned long long>(c, 1);
        {
            const unsigned long long e = ERR_NONE;
            HIPCHK(hipMemcpy(P.err, &e, 8, hipMemcpyHostToDevice));
        }
        if (F.persist != PERSIST_NONE) alloc_persist(c);
        if (F.plan == PLAN_BIG)
            HIPCHK(hipFuncSetAttribute((const void*)k_exch_plan_big, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan_big_lds_bytes(65535)));
        if (F.xk == XK_ROWS || F.xk == XK_KEY) {
            HIPCHK(hipFuncSetAttribute((const void*)k_exch_resolve_key<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)resolve_key_bytes(XKEY_MAX, XKEY_MAX)));
            HIPCHK(hipFuncSetAttribute((const void*)k_exch_resolve_key<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)resolve_key_bytes(XKEY_PARTNER_MAX, XKEY_PARTNER_MAX)));
            HIPCHK(hipFuncSetAttribute((const void*)k_exch_resolve_rows<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)resolve_rows_bytes(XKEY_MAX, XKEY_MAX, XROWS_MAX)));
            HIPCHK(hipFuncSetAttribute((const void*)k_exch_resolve_rows<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)resolve_rows_bytes(XKEY_PARTNER_MAX, XKEY_PARTNER_MAX, XROWS_MAX)));
            HIPCHK(hipFuncSetAttribute((const void*)k_exch_resolve_rows<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)resolve_rows_bytes(XKEY_MAX, XKEY_MAX, XROWS_MAX)));
            HIPCHK(hipFuncSetAttribute((const void*)k_exch_resolve_rows<false, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 158 * 1024));
            HIPCHK(hipFuncSetAttribute((const void*)k_exch_resolve_rows<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)resolve_rows_bytes(XKEY_PARTNER_MAX, XKEY_PARTNER_MAX, XROWS_MAX)));
        }
        if (F.plan == PLAN_LDS) {
#ifdef SMM_TEST_HOOKS
            HIPCHK(hipFuncSetAttribute((const void*)k_exch_resolve_lds, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)resolve_lds_bytes(XLDS_MAX)));
#endif
            HIPCHK(hipFuncSetAttribute((const void*)k_exch_plan, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)std::max(plan_lds_bytes(XLDS_MAX, XLDS_MAX), plan_cone_bytes())));
#ifdef SMM_TEST_HOOKS
            HIPCHK(hipFuncSetAttribute((const void*)k_exch_resolve_lvl<256>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)resolve_lvl_bytes(XLVL_MAX, XLVL_MAX)));
            HIPCHK(hipFuncSetAttribute((const void*)k_exch_resolve_lvl<512>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)resolve_lvl_bytes(XLVL_MAX, XLVL_MAX)));
#endif
            HIPCHK(hipFuncSetAttribute((const void*)k_exch_resolve_lvl_soa<1024>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)resolve_lvl_soa_bytes(XLDS_MAX, XLDS_MAX)));
            HIPCHK(hipFuncSetAttribute((const void*)k_exch_resolve_lvl<1024>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)resolve_lvl_bytes(XLVL_MAX, XLVL_MAX)));
            HIPCHK(hipFuncSetAttribute((const void*)k_exch_resolve_lean, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       160 * 1024));
        }
        {   // tiles of problems with many parameters need more than the default 64 KiB of dynamic LDS
            const int lim = 160 * 1024;
            // (every kernel chain_kernel / chain_kernel_p2p can pick: what chain_instance names)
            for (int family = 0; family < CF_COUNT; ++family)
                for (int np = 1; np <= 4; ++np)
                    for (int b = 0; b < 2; ++b) HIPCHK(hipFuncSetAttribute(chain_instance(family, np, b != 0).fn, hipFuncAttributeMaxDynamicSharedMemorySize, lim));
            if (F.cone_big) HIPCHK(hipFuncSetAttribute((const void*)k_cone_chains, hipFuncAttributeMaxDynamicSharedMemorySize, Ng * 4));
            HIPCHK(hipFuncSetAttribute((const void*)k_eval_batch<1, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, lim));
            HIPCHK(hipFuncSetAttribute((const void*)k_eval_batch<2, 16>, hipFuncAttributeMaxDynamicSharedMemorySize, lim));
            HIPCHK(hipFuncSetAttribute((const void*)k_eval_batch<0, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, lim));
            if (tile_smem(c, is_sim(c->obj) ? F.ct : (c->obj == SMM_OBJ_DENSE ? 16 : 8)) > (size_t)lim)
                throw std::string("tile does not fit the 160 KiB LDS");
        }
        reducer_kernel_attributes();
        HIPCHK(hipDeviceSynchronize());
    } catch (const std::string& m) {
        g_create_err = m;
        smm_ctx_destroy(c);
        return SMM_ERR_HIP;
    }
    *out = c;
    return SMM_OK;
}

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

// which forms this context was given at creation (one line; tests/test_gpu_forms.py pins the table)
int smm_describe(void* ctx, char* out, int32_t cap) {
    Ctx* c = (Ctx*)ctx;
    if (!c || !out || cap < 1) return SMM_ERR_INVALID_ARG;
    const KParams& P = c->P;
    // the kernel of the iterations that walk the previous exchange inline, where the context has such iterations and a kernel made for
    // them (narrow_cone, any, wide); else the kernel of the others (k_chain_iter_norm<np, true> is "iter_norm" like <np, false>, and where
    // the walk-free iterations take the narrow kernel that one is named)
    const bool walks = c->F.inline_walk || c->F.cone_big;
    ChainKernel chain = chain_kernel(c, walks ? F_WALK_INLINE : 0);
    if (walks && !strcmp(chain.name, "iter_norm")) chain = chain_kernel(c, 0);
    static const char* xk[] = {"lean", "lvl", "lvl_soa", "tickets", "rows", "key", "lvl_big", "any"};
    const char* walk = c->F.cone_big ? "cone_local" : !c->F.inline_walk ? "standalone" : c->F.dense_keys ? "inline_keys_under_tile" : c->F.gen_keys ? (c->F.cone ? "inline_keys_cone" : "inline_keys")
                     : c->F.norm_fast ? ((P.lean_wide && !P.mi_pct) ? "inline_lean_wide" : (c->F.lean_plan && !P.mi_pct) ? "inline_lean" : "inline_slots") : c->F.gen_lean ? "inline_lean16" : "inline_slots";
    const int n = snprintf(out, (size_t)cap, "chain=%s walk=%s exchange=%s persistent=%s plan=%s window=%d", chain.name, walk, xk[c->F.xk], persist_kernel(c, c->F).name,
                           c->F.plan == PLAN_BIG ? (c->F.plan_ahead ? "big_ahead" : "big") : c->F.plan == PLAN_LDS ? "lds" : "none", c->F.plan_cap);
    int n2 = n;
    if (c->obj == SMM_OBJ_USER && n >= 0 && n < cap) n2 = n + snprintf(out + n, (size_t)(cap - n), " ct=%d", chain.ct);   // (the three launches' tile width)
    // (only once a starting population has been installed: smm_set_population / smm_scatter_population)
    if (c->pop_kind == 1 && n2 >= 0 && n2 < cap) snprintf(out + n2, (size_t)(cap - n2), " population=set");
    if (c->pop_kind == 2 && n2 >= 0 && n2 < cap) snprintf(out + n2, (size_t)(cap - n2), " population=scatter pop_M=%d pop_spread=%.17g", c->pop_M, c->pop_spread);
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
