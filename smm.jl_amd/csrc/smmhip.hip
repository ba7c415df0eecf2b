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
// k_exch_plan), smm_exchange.hpp (stand-alone exchange kernels), this file (host: the types, the call frame, the reader prelude, the plain entry points), smm_user_host.hpp (user objectives: registration and their persistent forms, one way through hiprtc), smm_forms_host.hpp (which forms a context runs and the LDS they take: select_forms),
// smm_launch_host.hpp (the look-ahead windows, the four tables of kernel instantiations, the choosers, the launchers), smm_create_host.hpp (context creation, step by step), smm_run_host.hpp (the run's host side:
// stepping, settling, the sharded protocol), smm_reducers_host.hpp (the history reducers' host side), smm_estimate_host.hpp (the frame of the estimators that evaluate points off the chains; device side: smm_evalscratch.hpp), smm_population_host.hpp (the starting population's), smm_optslices_host.hpp (smm_opt_slices: the coordinate searches' loop), smm_optsimplex_host.hpp (smm_opt_simplex: the simplex searches' loop), smm_optlm_host.hpp (smm_opt_lm: the Levenberg–Marquardt searches' loop), smm_pmc_host.hpp (smm_abc_pmc: the sampler's generations), smm_sobol_host.hpp (smm_sens_sobol: the batches of base points).
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
#include "smm_reweight.hpp"
#include "smm_hist.hpp"
#include "smm_profile.hpp"
#include "smm_trace.hpp"
#include "smm_rank.hpp"
#include "smm_density.hpp"
#include "smm_derived.hpp"
#include "smm_draws.hpp"
#include "smm_evalscratch.hpp"
#include "smm_population.hpp"
#include "smm_optslices.hpp"
#include "smm_optsimplex.hpp"
#include "smm_optlm.hpp"
#include "smm_pmc.hpp"
#include "smm_sobol.hpp"

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
    size_t opt_scratch = 0;        // the scratch cap of smm_opt_slices, smm_opt_simplex and smm_opt_lm instead of OPT_SCRATCH_CAP (0: that cap): several batches of searches at small sizes
    bool opt_materialise = false;  // smm_opt_slices writes the built-in objectives' candidates out too and evaluates them with k_eval_batch (tools/opt_slices_time.py)
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
    if (const char* v = SMM_HOOK("SMMHIP_OPT_SCRATCH")) H.opt_scratch = (size_t)strtoull(v, nullptr, 10);
    H.opt_materialise = is(SMM_HOOK("SMMHIP_OPT_MATERIALISE"), '1');
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
struct PersistKernel { const void* fn; hipFunction_t mfn; dim3 grid, block; size_t smem; std::string name; };   // (name: the row's of persist_instance, and the forms' suffixes)
// a row of exch_instance's table (cap: the dynamic LDS limit raised at creation where the context's forms include the row's group, 0: the default
// will do; stamped: takes the dispatch's own stamps in profiling mode 2), and a chooser's pick for one launch (the row, this launch's dynamic LDS)
enum ExchId { XI_CONE_CHAINS, XI_CONE_TILES, XI_PLAN_BIG, XI_PLAN, XI_LEAN, XI_LVL_256, XI_LVL_512, XI_LVL, XI_LVL_SOA, XI_TICKETS, XI_KEYS, XI_ROWS_PLDS,
              XI_ROWS, XI_KEY_PLDS, XI_KEY, XI_LVL_BIG, XI_ANY, XI_ROWS_WIN_OWN, XI_ROWS_WIN_PLDS, XI_ROWS_WIN, XI_APPLY, XI_PLAN_BG, XI_COUNT };
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
    std::vector<std::pair<int32_t, hipModule_t>> tmods;   // user transforms (smm_get_derived): the modules this context has loaded, by handle
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
        // (plan_beside: the LDS plan's own tables of the set — the ranked pair list, its thresholds, the lean walk's padded list)
        unsigned long long* plan = nullptr;
        double* plan_mi = nullptr;
        uint32_t *lv_pairs_p = nullptr, *lv_offp = nullptr;
    } ps[2];
    // ... and so are the LDS plan's of a single shard on k_chain_persist_loc whose plan fits k_exch_plan_bg (plan_bg_fits): that kernel runs
    // BESIDE the chain kernel, in the registers and the LDS it leaves (choose_plan_beside); the host waits for nothing.  Not a field of
    // Forms: what select_forms decides is what it decided before there was this path
    bool plan_beside = false;
    int windows_beside = 0, windows_instream = 0;   // plan windows entered so far: planned beside the chain kernel / on the main stream (smm_get_plan_beside)
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

}  // namespace

#include "smm_user_host.hpp"
#include "smm_forms_host.hpp"
#include "smm_launch_host.hpp"
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

// the round trip of M evaluations (smm_eval_batch, smm_eval_batch_noseed): the parameters up, launch(params, value, moments, status) on the
// context's stream, the three results down, finished.  Moments and parameters travel as they lie (a user objective's: user_eval_batch).
template <class Status, class Launch>
void eval_round_trip(Ctx* c, const double* params, int32_t M, double* value, double* sim_moments, Status* status, Launch launch) {
    const size_t np = (size_t)c->P.np * M, nm = (size_t)c->P.nm * M;
    DevBuf<double> dp(np), dv((size_t)M), dm(nm);
    DevBuf<Status> ds((size_t)M);
    HIPCHK(hipMemcpyAsync(dp.p, params, np * 8, hipMemcpyHostToDevice, c->stream));
    launch(dp.p, dv.p, dm.p, ds.p);
    HIPCHK(hipMemcpyAsync(value, dv.p, (size_t)M * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(sim_moments, dm.p, nm * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(status, ds.p, (size_t)M * sizeof(Status), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
}

}  // namespace

#include "smm_reducers_host.hpp"
#include "smm_estimate_host.hpp"
#include "smm_population_host.hpp"
#include "smm_optslices_host.hpp"
#include "smm_optsimplex_host.hpp"
#include "smm_optlm_host.hpp"
#include "smm_pmc_host.hpp"
#include "smm_sobol_host.hpp"
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
    std::vector<double> tp((size_t)M * P.np), tm((size_t)M * P.nm);
    std::vector<int> ts((size_t)M);
    for (int i = 0; i < M; ++i)
        for (int k = 0; k < P.np; ++k) tp[(size_t)i * P.np + k] = params[(size_t)k * M + i];
    eval_round_trip(c, tp.data(), M, value, tm.data(), ts.data(), [&](const double* dp, double* dv, double* dm, int* ds) {
        if (base_seed) launch_user_kernel(c, dp, M, dm, dv, ds, base_seed);
        else launch_eval_dev(c, dp, M, dv, dm, ds);
    });
    for (int i = 0; i < M; ++i) {
        status[i] = (int8_t)ts[i];
        for (int k = 0; k < P.nm; ++k) sim_moments[(size_t)k * M + i] = tm[(size_t)i * P.nm + k];
    }
}

int smm_eval_batch(void* ctx, const double* params, int32_t M, double* value, double* sim_moments, int8_t* status) {
    return api_call(ctx, params && M >= 0 && value && sim_moments && status, [&](Ctx* c) -> int {
        if (M == 0) return SMM_OK;
        HIPCHK(hipSetDevice(c->device));
        if (c->obj == SMM_OBJ_USER) user_eval_batch(c, params, M, value, sim_moments, status, nullptr);
        else eval_round_trip(c, params, M, value, sim_moments, status, [&](const double* dp, double* dv, double* dm, int8_t* ds) { launch_eval_dev(c, dp, M, dv, dm, ds); });
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
        eval_round_trip(c, params, M, value, sim_moments, status, [&](const double* dp, double* dv, double* dm, int8_t* ds) {
            hipLaunchKernelGGL(k_eval_batch_noseed, dim3(M), dim3(WG), (size_t)(WG / 64) * P.nm * 8, c->stream, P, dp, M, (uint64_t)base_seed, dv, dm, ds);
            HIPCHK(hipGetLastError());
        });
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
        if (const int rc = estimate_enter(c)) return rc;   // (an untold failure is reported here, once: smm_estimate_host.hpp)
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

int smm_get_plan_beside(void* ctx, int32_t* beside, int32_t* windows_beside, int32_t* windows_instream) {
    return api_call(ctx, true, [&](Ctx* c) -> int {
        if (beside) *beside = c->plan_beside ? 1 : 0;
        if (windows_beside) *windows_beside = c->windows_beside;
        if (windows_instream) *windows_instream = c->windows_instream;
        return SMM_OK;
    });
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
// debug (test build only, not part of the public header; touches no device): the sizes the residency of k_exch_plan_bg beside k_chain_persist_loc
// is argued from — out[0] persist_loc_smem_bytes(np), [1] the background kernel's LDS request, [2] the LDS of a compute unit, [3] the allocation
// granule, [4] / [5] the largest population (pairs = chains) the background form takes / 1 if it takes (Ng, K), [6] the static LDS the residency allows the compiler to add
int smm_debug_plan_beside_budget(int np, int Ng, int K, long long* out) {
    if (!out || np < 1 || np > 2) return SMM_ERR_INVALID_ARG;
    out[0] = (long long)persist_loc_smem_bytes(np); out[1] = (long long)PBG_LDS; out[2] = (long long)LDS_CU; out[3] = (long long)LDS_GRANULE;
    int n = 0;
    while (plan_bg_fits(n + 1, n + 1)) ++n;
    out[4] = n; out[5] = plan_bg_fits(Ng, K) && plan_beside_resident(np) ? 1 : 0; out[6] = (long long)PBG_LDS_STATIC;
    return SMM_OK;
}
// (the two seams below on a context of the LDS plan that does NOT plan beside — a population past the persistent form's 4096 chains —: the two sets are
// made on first use, with cone tables of 16-chain tiles, so that k_exch_plan_bg can be held against k_exch_plan up to the last population its LDS takes,
// which no context reaches on a device of 256 compute units.  Returns the tiles of the sets' cone tables, 0: not a context of the LDS plan)
static int debug_plan_sets(Ctx* c) {
    if (c->plan_beside) return c->P.cone_tiles;
    if (c->F.plan != PLAN_LDS || !c->F.lean_plan || c->F.plan_ahead) return 0;
    const int tiles = (c->P.N + NORM_CT - 1) / NORM_CT;
    if (!c->ps[0].plan) {
        const size_t W = (size_t)c->F.plan_cap, K = (size_t)c->P.plan_K;
        for (Ctx::PlanSet& S : c->ps) {
            alloc_level_tables(c, S, false, (size_t)tiles, true);
            S.plan = dalloc<unsigned long long>(c, W * K); S.plan_mi = dalloc<double>(c, W * K);
            S.lv_pairs_p = dalloc<uint32_t>(c, W * c->P.plan_Kp + 512); S.lv_offp = dalloc<uint32_t>(c, W * LV_OFFP);
        }
    }
    return tiles;
}
// debug (test build only): the tables of the plan set `which` (0 / 1: by index; -1: the active one) for iteration S.t0 + w, copied out after both streams
// have drained — info: t0, w of the set, nlev, cone_ok, K, tiles; plan [K] words, lv_pairs [K], lv_off [K + 2], offp [LV_OFFP], pairs_p [plan_Kp],
// hdr [tiles][CONE_HDRW], cone pairs [tiles][CONE_LEVELS * 64], gather [tiles][CONE_GCAP] (tests/test_gpu_plan_beside.py: k_exch_plan_bg's against k_exch_plan's)
int smm_debug_plan_tables(void* ctx, int which, int w, int32_t* info, unsigned long long* plan, uint32_t* lv_pairs, uint32_t* lv_off, uint32_t* offp, uint32_t* pairs_p,
                          uint32_t* hdr, uint32_t* cpairs, uint16_t* gather) {
    return api_call(ctx, info != nullptr, [&](Ctx* c) -> int {
        HIPCHK(hipSetDevice(c->device));
        const size_t tiles = (size_t)debug_plan_sets(c);
        if (!tiles) return SMM_ERR_INVALID_ARG;
        HIPCHK(hipStreamSynchronize(c->stream));
        if (c->pstream) HIPCHK(hipStreamSynchronize(c->pstream));
        const Ctx::PlanSet& S = c->ps[which < 0 ? c->ps_act : (which & 1)];
        const KParams& P = c->P;
        const size_t K = (size_t)P.plan_K;
        uint32_t ok = 0, nlev = 0;
        HIPCHK(hipMemcpy(&ok, S.cone_ok + w, 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(&nlev, S.lv_off + (size_t)w * (K + 2) + K + 1, 4, hipMemcpyDeviceToHost));
        info[0] = S.t0; info[1] = S.w; info[2] = (int32_t)nlev; info[3] = (int32_t)ok; info[4] = (int32_t)K; info[5] = (int32_t)tiles; info[6] = P.plan_Kp; info[7] = S.lv_pairs_p ? 1 : 0;
        if (plan) HIPCHK(hipMemcpy(plan, S.plan + (size_t)w * K, K * 8, hipMemcpyDeviceToHost));
        if (lv_pairs) HIPCHK(hipMemcpy(lv_pairs, S.lv_pairs + (size_t)w * K, K * 4, hipMemcpyDeviceToHost));
        if (lv_off) HIPCHK(hipMemcpy(lv_off, S.lv_off + (size_t)w * (K + 2), (K + 2) * 4, hipMemcpyDeviceToHost));
        if (offp && S.lv_offp) HIPCHK(hipMemcpy(offp, S.lv_offp + (size_t)w * LV_OFFP, LV_OFFP * 4, hipMemcpyDeviceToHost));
        if (pairs_p && S.lv_pairs_p) HIPCHK(hipMemcpy(pairs_p, S.lv_pairs_p + (size_t)w * P.plan_Kp, (size_t)P.plan_Kp * 4, hipMemcpyDeviceToHost));
        if (hdr) HIPCHK(hipMemcpy(hdr, S.cone_hdr + (size_t)w * tiles * CONE_HDRW, tiles * CONE_HDRW * 4, hipMemcpyDeviceToHost));
        if (cpairs) HIPCHK(hipMemcpy(cpairs, S.cone_pairs + (size_t)w * tiles * (CONE_LEVELS * 64), tiles * CONE_LEVELS * 64 * 4, hipMemcpyDeviceToHost));
        if (gather && S.cone_gather) HIPCHK(hipMemcpy(gather, S.cone_gather + (size_t)w * tiles * CONE_GCAP, tiles * CONE_GCAP * 2, hipMemcpyDeviceToHost));
        return SMM_OK;
    });
}
// debug (test build only): the plan window from iteration t on by k_exch_plan_bg (bg != 0) or k_exch_plan into plan set `which`, on the main stream
int smm_debug_plan_into(void* ctx, int which, int t, int bg) {
    return api_call(ctx, true, [&](Ctx* c) -> int {
        if (t < 1 || t > c->P.T || (bg && !plan_bg_fits(c->P.Ng, c->P.plan_K))) return SMM_ERR_INVALID_ARG;
        HIPCHK(hipSetDevice(c->device));
        const int tiles = debug_plan_sets(c);
        if (!tiles) return SMM_ERR_INVALID_ARG;
        if (c->pstream) HIPCHK(hipStreamSynchronize(c->pstream));
        Ctx::PlanSet& S = c->ps[which & 1];
        KParams Pw = c->P;
        point_tables(Pw, S);
        if (!c->plan_beside) { Pw.cone_tiles = tiles; Pw.cone_ct = NORM_CT; }
        const int W = std::min(c->F.plan_cap, Pw.T - t + 1);
        launch_exch(c, bg ? XI_PLAN_BG : XI_PLAN, dim3(W), bg ? PBG_LDS : plan_smem(Pw.Ng, Pw.plan_K, true), c->stream, Pw, t, S.plan, S.plan_mi, S.lv_pairs, S.lv_mi, S.lv_off,
                    S.lv_pairs_p, S.lv_offp);
        HIPCHK(hipStreamSynchronize(c->stream));
        S.t0 = t; S.w = W;
        if (c->plan_beside && (which & 1) == c->ps_act) { c->plan_t0 = t; c->plan_w = W; c->P.plan_t0 = t; }
        return SMM_OK;
    });
}
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
