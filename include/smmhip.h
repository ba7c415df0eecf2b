/*
 * smmhip.h — C ABI of libsmmhip.so: the MI355X (gfx950) backend for the BGP
 * parallel-tempering hot path of floswald/SMM.jl.
 *
 * The reference has no FFI; its two seams are Julia dynamic dispatch:
 *   (1) computeNextIteration!(algo::MAlgoBGP)      src/mopt/AlgoBGP.jl:589-640
 *       (called once per iteration from run!       src/mopt/AlgoAbstract.jl:38-45)
 *   (2) the objective contract f(ev::Eval)::Eval   src/mopt/mprob.jl:175-205
 * A Julia maintainer binds the functions below with `ccall`;
 * the Python host layer in smm.jl_amd/ binds them with ctypes.
 *
 * Conventions
 *   - every entry point returns 0 on success, <0 = smm_status_t error code;
 *     smm_last_error(ctx) returns a human readable message (ctx may be NULL for
 *     errors raised by smm_ctx_create).
 *   - all pointers are HOST pointers unless the name ends in `_dev`.
 *   - host buffers are borrowed for the duration of the call only.
 *   - chain ids and iteration numbers in *downloaded* data are 1-based exactly
 *     as in the reference (BGPChain.id, BGPChain.exchanged, BGPChain.best_id;
 *     AlgoBGP.jl:42-110): exchanged==0 means "no exchange", best_id==-1 "unset".
 *   - all floating point data is IEEE double (the reference is Float64 throughout).
 *   - a ctx is single-threaded (one caller thread), like the reference's master task.
 */
#ifndef SMMHIP_H
#define SMMHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMMHIP_ABI_VERSION 3

/* Numerical contract shared with the oracle (oracle/smm_oracle.c):
 * the ns simulated draws of one moment are summed as SMM_REDUCE_LANES lane-strided
 * sequential partial sums (lane l takes draws l, l+512, l+1024, ...), each group of 64
 * partials is combined by a halving tree (offsets 32,16,8,4,2,1) and the 8 group
 * totals are added left to right.  Replaces mean(X,dims=2), ObjExamples.jl:79.
 * The elementary functions of the path are part of the contract too: the logarithm and the sine / cosine of the generator's
 * Box-Muller transform and the exponential of the acceptance probability (AlgoBGP.jl:344) are fixed sequences of correctly
 * rounded operations (smm.jl_amd/csrc/smm_rng.hpp: smm_log, smm_sincos2pi — after fdlibm —, smm_exp; each within 1 ulp), the
 * dense objective's tanh likewise (below).  Consequence: a run is reproduced BIT FOR BIT by any implementation of the contract —
 * every floating-point field of the history, not only the bookkeeping. */
#define SMM_REDUCE_LANES 512

typedef enum {
    SMM_OK = 0,
    SMM_ERR_INVALID_ARG = -1,
    SMM_ERR_NO_DEVICE = -2,          /* no HIP device / HIP runtime failure          */
    SMM_ERR_NEGATIVE_OBJECTIVE = -3, /* objective value <0 or NaN: AlgoBGP.jl:341     */
    SMM_ERR_NO_DRAW_IN_SUPPORT = -4, /* mysample exhausted smpl_iters: AlgoBGP.jl:409 */
    SMM_ERR_BAD_BATCH = -5,          /* batch_size not a divisor of np: AlgoBGP.jl:95-103 (quirk not replicated) */
    SMM_ERR_MAXITER = -6,            /* step beyond opts.maxiter (history capacity)   */
    SMM_ERR_HIP = -7,
    SMM_ERR_STATE = -8,
    SMM_ERR_EXCHANGE_CAPACITY = -9   /* values form of the sharded exchange: a (source, destination) block overflowed */
} smm_status_t;

/* objective_id: device objectives replacing MProb.objfunc (mprob.jl:159,182) */
typedef enum {
    SMM_OBJ_NORM = 0,   /* objfunc_norm, ObjExamples.jl:59-116 (requires np==nm)          */
    SMM_OBJ_BANANA = 1, /* banana, ObjExamples.jl:251-265, generalised to np dims        */
    SMM_OBJ_NORM_FAILBOX = 2, /* objfunc_norm that "throws" (status=-2, mprob.jl:183-186)
                                when obj_params[0] <= theta_0 <= obj_params[1]; the role of
                                Testobj_fails, ObjExamples.jl:27-32 */
    SMM_OBJ_DENSE = 3,  /* synthetic dense simulation (BASELINE config 5, no reference counterpart):
                           x = B*theta (B: SMM_DENSE_D x np), h = tanh(x), y = A*h (A: nm x SMM_DENSE_D),
                           simM = y, value = mean(((simM-mom)/w)^2).  obj_params = [B row-major, A row-major]
                           (SMM_DENSE_D*np + nm*SMM_DENSE_D doubles) or empty = generated from the seed.
                           Summation order (numerical contract): x_d = fma chain over p; y_k = 8 fma chains
                           over d in [32w, 32w+32), added left to right.  FP64 MFMA on the device.
                           tanh (numerical contract, at most 3 ulp from the true value): with z = 2|x|, n = rint(z log2 e),
                           r = z - n ln2 (two fma), p = expm1(r) by its Taylor series to r^13 (Horner, fma):
                           tanh|x| = fma(2^n, p, 2^n - 1) / fma(2^n, p, 2^n + 1), 1 from |x| = 19.0625 on. */
    /* (4 is SMM_OBJ_USER, the internal kind of every user objective) */
    SMM_OBJ_DENSE2 = 5  /* BASELINE config 5 AS WORDED — "256x256 matvec per eval" (spec v2 of the synthetic dense simulation; SMM_OBJ_DENSE
                           keeps its id and its goldens):
                               x = B*theta (B: 256 x np), h1 = tanh(x), g = A2*h1 (A2: 256 x 256), h2 = tanh(g), y = A*h2 (A: nm x 256),
                           simM = y, value = mean(((simM-mom)/w)^2): 2*256*np + 2*256*256 + 2*nm*256 flop per evaluation (1.8e5 at
                           np = nm = 50).  obj_params = [B row-major, A2 row-major, A row-major] (256*np + 65536 + nm*256 doubles) or
                           empty = generated from the seed (N(0,1)/sqrt(fan-in), counter stream 5, in that order).
                           Summation order (numerical contract): x_d = fma chain over p; g_j = ONE fma chain over d = 0..255 (the
                           accumulator of a row tile's 64 v_mfma_f64_16x16x4); y_k = 8 fma chains over d in [32w, 32w+32), added
                           left to right; the tanh above.  The plugin seam it exercises: MProb.objfunc, mprob.jl:159,182. */
} smm_objective_t;
#define SMM_DENSE_D 256

/* User objectives — the reference's "bring your own objfunc" (MProb.objfunc, mprob.jl:159,182) on the device.
 * objective_id >= SMM_OBJ_USER_BASE is a handle returned by smm_register_user_objective.  The source is HIP/C++
 * text defining ONE function with this exact signature (SMM_USER_OBJECTIVE expands to the required linkage):
 *
 *   SMM_USER_OBJECTIVE(const double* theta, int np, const double* mom, const double* w, int nm,
 *                      const double* udata, int n_udata, double* sim_moments, double* value, int* status)
 *
 * It must fill sim_moments[0..nm), *value (>= 0, AlgoBGP.jl:341) and *status (1 = ok; < 0 = failed, the record is
 * rejected like an objective that threw, mprob.jl:183-186).  It must be a deterministic function of its inputs
 * (a simulation seeds its own generator, as objfunc_norm does with Random.seed!(1234)); udata = obj_params.
 * It is compiled at registration (hiprtc, -ffp-contract=off) and evaluated for all chains of an iteration by one
 * kernel launch, one thread per chain, between the proposal and the accept step.
 *
 * Map-reduce form for simulations that are sums over many independent units (agents, draws, paths) —
 * smm_register_user_objective_lanes(source, n_sums, lanes, &id): `lanes` threads (a multiple of 64, <= 1024)
 * evaluate one chain.  The source defines TWO functions:
 *
 *   SMM_USER_PARTIAL(const double* theta, int np, const double* udata, int n_udata, int lane, int n_lanes,
 *                    double* partial)          lane's partial sums, partial[0..n_sums) (zero on entry);
 *                                              by convention lane l works on units l, l + n_lanes, ...
 *   SMM_USER_FINISH (const double* theta, int np, const double* totals, int n_sums, const double* mom,
 *                    const double* w, int nm, const double* udata, int n_udata, double* sim_moments,
 *                    double* value, int* status)   from the totals to moments, objective value, status.
 *
 * The library reduces the partials in a fixed order (numerical contract): inside each group of 64 lanes the
 * halving tree (offsets 32,16,..,1), then the group totals left to right.
 *
 * Objectives that draw from the library's generator — smm_register_user_objective_rng(source, n_sums, lanes, &id):
 * n_sums == 0 is the one-thread form (lanes ignored), n_sums >= 1 the map-reduce form (limits as for _lanes).  The source
 * defines the same functions with a stream handle as one more argument:
 *
 *   SMM_USER_OBJECTIVE_RNG(const double* theta, int np, const double* mom, const double* w, int nm,
 *                          const double* udata, int n_udata, smm_rng_t rng, double* sim_moments, double* value, int* status)
 *   SMM_USER_PARTIAL_RNG(const double* theta, int np, const double* udata, int n_udata, smm_rng_t rng,
 *                        int lane, int n_lanes, double* partial)          (+ SMM_USER_FINISH as above, without a stream)
 *
 * and may call, from any lane:
 *   double smm_uniform(smm_rng_t r, uint64_t i)                          draw i of the stream, in [0, 1)
 *   void   smm_normal2(smm_rng_t r, uint64_t j, double* z0, double* z1)  both standard normals of Philox block j
 *   double smm_normal(smm_rng_t r, uint64_t i)                           normal i = component i & 1 of smm_normal2(r, i >> 1)
 * Numerical contract: Philox4x32-10 with the key (k0, k1) = (lo32(seed), hi32(seed) ^ (6 * 0x9E3779B9)) (stream 6 of the
 * library's generator).  smm_normal2: counter {lo32(j), hi32(j), 0, 0} -> x, u1 = ((x0:x1 >> 11) + 1) * 2^-53,
 * u2 = (x2:x3 >> 11) * 2^-53 (x0:x1 = the 64-bit word x0 * 2^32 + x1), r = sqrt(-2 log u1), z0 = r cos(2 pi u2), z1 = r sin(2 pi u2)
 * with the contract's log / sine / cosine (above).  smm_uniform: counter {lo32(i), hi32(i), 1, 0} -> (x0:x1 >> 11) * 2^-53.
 * The seed: opts.seed in BGP steps and smm_eval_batch — the SAME stream for every chain, shard and iteration (common random
 * numbers, as objfunc_norm's shocks; the role of Random.seed!(1234), ObjExamples.jl:74) —, base_seed + i for evaluation i of
 * smm_eval_batch_noseed (fresh shocks per repetition: getSigma, econometrics.jl:125-145).  Both forms run in every kernel form
 * the same objective without a stream runs in (the persistent ones included). */
#define SMM_OBJ_USER_BASE 1000
#define SMM_OBJ_USER 4   /* internal kind of every user objective */

/* MProb (mprob.jl:29-53) flattened: parameters to sample with bounds and start
 * values (addSampledParam!, mprob.jl:81-98), data moments and weights
 * (addMoment!, mprob.jl:123-155). */
typedef struct {
    int32_t np;              /* number of sampled parameters                              */
    int32_t nm;              /* number of moments                                         */
    int32_t ns;              /* simulated draws per moment (10000 in ObjExamples.jl:76)   */
    int32_t objective_id;    /* smm_objective_t                                           */
    const double* init;      /* [np] MProb.initial_value                                  */
    const double* lb;        /* [np]                                                      */
    const double* ub;        /* [np]                                                      */
    const double* mom;       /* [nm] data moments                                         */
    const double* w;         /* [nm] weights; NaN = no weight (ObjExamples.jl:96-97)      */
    const double* obj_params;/* objective specific blob, may be NULL                      */
    int32_t n_obj_params;
    int32_t reserved;
} smm_problem_t;

/* opts["dist_fun"] (AlgoBGP.jl:494,537): the reference takes any Julia function of two objective values; the device offers a
 * menu.  value_i belongs to the colder chain i < j of the pair; the pair swaps when the distance exceeds min_improve_i. */
typedef enum {
    SMM_DIST_MINUS   = 0,    /* value_i - value_j            (the default `-`: j is better by more than min_improve_i)      */
    SMM_DIST_ABSDIFF = 1,    /* |value_i - value_j|          (swap whenever the two differ by more than min_improve_i)      */
    SMM_DIST_RELDIFF = 2     /* (value_i - value_j)/|value_i| (j is better by more than the fraction min_improve_i)         */
} smm_dist_fun_t;

/* opts Dict of MAlgoBGP (AlgoBGP.jl:505-537) flattened; per-chain vectors are
 * supplied already expanded (sigma[i] = opts["sigma"]*temps[i], AlgoBGP.jl:508,518) and
 * GLOBAL (length N_global); the context uses entries [chain_offset, chain_offset+N). */
typedef struct {
    int32_t N;               /* chains owned by THIS context (local shard)                */
    int32_t maxiter;         /* history capacity T (BGPChain(n), AlgoBGP.jl:78)           */
    const double* sigma;     /* [N_global] initial proposal std-dev in [0,1]-space        */
    const double* acc_tuner; /* [N_global] AlgoBGP.jl:523                                 */
    const double* min_improve;/* [N_global] AlgoBGP.jl:522 (the exchange test of pair (i,j)
                                 reads chain i's threshold on every shard, :688)          */
    int32_t sigma_update_steps; /* AlgoBGP.jl:519                                         */
    int32_t smpl_iters;         /* AlgoBGP.jl:521                                         */
    double  sigma_adjust_by;    /* AlgoBGP.jl:520                                         */
    int32_t batch_size;         /* AlgoBGP.jl:524; must divide np                         */
    int32_t exchange_from_iter; /* 2 in the reference (AlgoBGP.jl:637)                    */
    uint64_t seed;
    int32_t chain_offset;    /* global id (0-based) of local chain 0                      */
    int32_t N_global;        /* total chains over all shards (== N on one GPU)            */
    int32_t device;          /* HIP device ordinal                                        */
    int32_t chol_per_chain;  /* 0: chol_L is one [np][np] factor shared by all chains; 1: [N_global][np][np] */
    const double* chol_L;    /* General Gaussian proposals ("Cholesky apply"): NULL = the reference's isotropic kernel
                                MvNormal(mu01, sigma) (AlgoBGP.jl:442).  Otherwise a lower-triangular factor L (row-major,
                                entries above the diagonal ignored) of the proposal's shape in [0,1]-space:
                                    x = mu01 + sigma_c * (L z),   z ~ N(0, I)      i.e. covariance sigma_c^2 L L'
                                with the chain's adaptive scalar sigma_c (AlgoBGP.jl:381-390) as the scale; L = diag(s)
                                is the per-parameter sigma vector hinted at AlgoBGP.jl:218.  Requires one proposal batch
                                (batch_size == np).  Numerical contract: (L z)_k = sum_{j<=k} L[k][j]*z[j], products
                                rounded, added left to right (no fma). */
    int32_t dist_fun;        /* smm_dist_fun_t: opts["dist_fun"], AlgoBGP.jl:537 — the exchange test of pair (i, j) is
                                dist_fun(value_i, value_j) > min_improve_i (:688).  0 = the reference's default `-`.           */
    int32_t reserved;
} smm_bgp_opts_t;

/* Injected randomness ("parity mode").  Any pointer may be NULL = use the built-in
 * counter-based generator (Philox4x32-10 + Box-Muller, documented in DESIGN.md).
 * Tables cover the LOCAL shard's chains, except `pairs` which is global. */
typedef struct {
    const double* probs_acc;   /* [T][N]  the MH uniforms, BGPChain.probs_acc AlgoBGP.jl:85    */
    const double* prop_normals;/* [T][K][np][N] standard normals for try k of mysample         */
    int32_t prop_tries;        /* K; tries beyond K raise SMM_ERR_NO_DRAW_IN_SUPPORT           */
    int32_t n_pairs;           /* pairs per iteration in `pairs` (N_global, or N_global-1 <3)  */
    const int32_t* pairs;      /* [T][n_pairs][2] 0-based global chain ids i<j, AlgoBGP.jl:656 */
    const double* Z;           /* [nm][ns] shock matrix of objfunc_norm (seed-1234 draws)      */
} smm_tables_t;

/* Caller-allocated SoA download buffers for iterations t0..t1-1 (0-based t = iter-1).
 * nt = t1-t0.  Any pointer may be NULL (skipped).  Mirrors history(c) AlgoBGP.jl:138-160
 * plus the Eval fields read by params()/allAccepted() (:117-131). */
typedef struct {
    double* value;      /* [nt][N]      evals[t].value                         */
    double* prob;       /* [nt][N]      evals[t].prob                          */
    double* curr_val;   /* [nt][N]                                              */
    double* best_val;   /* [nt][N]                                              */
    double* params;     /* [nt][np][N]                                          */
    double* sim_moments;/* [nt][nm][N]                                          */
    int32_t* best_id;   /* [nt][N]      1-based iteration                      */
    int32_t* exchanged; /* [nt][N]      1-based partner id, 0 none             */
    uint8_t* accepted;  /* [nt][N]                                              */
    int8_t*  status;    /* [nt][N]      evals[t].status                        */
} smm_history_t;

/* Per-chain scalar state (what save/readMalgo/restart! need besides history;
 * AlgoAbstract.jl:83-102, AlgoBGP.jl:759-884). Caller-allocated, any may be NULL. */
typedef struct {
    int32_t iter;        /* out/in: completed iterations                        */
    int32_t reserved;
    double* sigma;       /* [N]                                                  */
    double* accept_rate; /* [N]                                                  */
    double* la_value;    /* [N] last accepted record (getLastAccepted :217)      */
    double* la_prob;     /* [N]                                                  */
    double* la_params;   /* [np][N]                                              */
    double* la_sim_moments; /* [nm][N]                                           */
    int8_t* la_status;   /* [N]                                                  */
    int32_t* n_noex;     /* [N] iterations with exchanged==0 (set_acceptRate! :253-257) */
    int32_t* n_acc_noex; /* [N] accepted among those                             */
    double* best_val;    /* [N]                                                  */
    int32_t* best_id;    /* [N]                                                  */
} smm_state_t;

typedef struct {
    double step_ms;       /* device time of the last smm_bgp_step (hipEvent)           */
    double iter_kernel_ms;/* summed device time of the per-iteration chain kernel       */
    double exch_kernel_ms;/* summed device time of the exchange kernels                 */
    int64_t chain_evals;  /* chain evaluations performed by the last smm_bgp_step      */
    int32_t iters;
    int32_t reserved;
    double null_bracket_ms;/* summed device time of event pairs that bracket nothing: the per-bracket
                              overhead contained in iter_kernel_ms / exch_kernel_ms            */
} smm_timing_t;

int  smm_abi_version(void);
/* compile a user objective; errors (with the compiler log) through smm_last_error(NULL) */
int  smm_register_user_objective(const char* hip_source, int32_t* objective_id_out);
int  smm_register_user_objective_lanes(const char* hip_source, int32_t n_sums, int32_t lanes, int32_t* objective_id_out);
int  smm_register_user_objective_rng(const char* hip_source, int32_t n_sums, int32_t lanes, int32_t* objective_id_out);
int  smm_device_count(void);

/* MAlgoBGP(m,opts) constructor, AlgoBGP.jl:505-537 + BGPChain ctor :78-109 */
int  smm_ctx_create(const smm_problem_t* prob, const smm_bgp_opts_t* opts,
                    const smm_tables_t* tables /* may be NULL */, void** ctx_out);
void smm_ctx_destroy(void* ctx);
const char* smm_last_error(void* ctx);

/* n_iters x computeNextIteration! (AlgoBGP.jl:589-640) incl. exchangeMoves!
 * (:647-716); single shard only (N_global == N). Blocks until the device is done. */
int  smm_bgp_step(void* ctx, int32_t n_iters);
/* same, but returns after enqueueing; smm_sync waits and reports device errors. */
int  smm_bgp_step_async(void* ctx, int32_t n_iters);
int  smm_sync(void* ctx);

/* Sharded form (one ctx per GPU), the three phases of one iteration:
 *   smm_bgp_local_step : next_eval for the local chains (AlgoBGP.jl:272-294)
 *   smm_bgp_export_records_dev : copy the last-accepted records of the local chains into
 *        rec_dev [N][RW] doubles, RW = smm_bgp_record_doubles(ctx) (value, prob, status,
 *        params[np], simM[nm], zero padded to an even count) — the RCCL all-gather payload
 *   smm_bgp_exchange_dev : exchangeMoves! over all N_global chains given the gathered
 *        records [N_global][RW] in global chain order (identical on every rank), applied
 *        to the local chains */
int  smm_bgp_local_step(void* ctx);
int  smm_bgp_record_doubles(void* ctx);
int  smm_bgp_export_records_dev(void* ctx, void* rec_dev);
int  smm_bgp_exchange_dev(void* ctx, const void* gathered_dev);
/* The values form of the exchange phase, for long records: instead of every record, only every chain's
 * VALUE goes to every rank, and the record a chain continues from goes to that chain's owner alone.  Ranks own equal
 * blocks of N chains (G = N_global / N ranks).  After smm_bgp_local_step:
 *   smm_bgp_export_values_dev(ctx, vals [N])              the local chains' last accepted values -> all-gather to [N_global]
 *   smm_bgp_a2a_pack_dev(ctx, vals_all [N_global], send)  resolves exchangeMoves! from the values and fills this rank's
 *        send buffer [G][cap][RW]: block b holds, in the order of the receiving chains, the records that chains of rank b
 *        continue from (cap = smm_bgp_a2a_capacity(ctx) records per block; the block to itself included)
 *   -> one all-to-all of equal blocks (RCCL: ncclAllToAll / all_to_all_single of cap * RW doubles per pair)
 *   smm_bgp_a2a_apply_dev(ctx, recv [G][cap][RW])         applies the swaps to the local chains
 * Same result as smm_bgp_export_records_dev + all-gather + smm_bgp_exchange_dev.  A block that would need more than cap
 * records raises SMM_ERR_EXCHANGE_CAPACITY at the next smm_sync (cap = min(N, 2 N / G + 64): about four times the expected
 * count for the reference's pair sampling). */
int  smm_bgp_a2a_capacity(void* ctx);
int  smm_bgp_export_values_dev(void* ctx, void* vals_dev);
int  smm_bgp_a2a_pack_dev(void* ctx, const void* vals_all_dev, void* send_dev);
int  smm_bgp_a2a_apply_dev(void* ctx, const void* recv_dev);
/* The same iteration in two enqueues instead of five.  Both buffers are [N_global][RW] in global chain order:
 *   smm_bgp_sharded_step(ctx, gathered_prev, gathered_next): resolves exchangeMoves! of the previous iteration
 *        from gathered_prev (the all-gathered records after that iteration's accept step; may be NULL before
 *        the first sharded step), runs next_eval for the local chains — every chain continues from its own or
 *        its donor's record taken straight from gathered_prev — and writes the new last-accepted records into
 *        THIS shard's slice of gathered_next (rows chain_offset .. chain_offset+N).  The caller then all-gathers
 *        gathered_next in place (RCCL: ncclAllGather with sendbuff = recvbuff + rank*N*RW) and passes it as
 *        gathered_prev of the next call; two buffers alternate.
 *   smm_bgp_sharded_finish(ctx, gathered): settles the last sharded step (its exchange, history, counters) into
 *        the context; required before smm_get_history / smm_get_state / the three-phase calls. */
int  smm_bgp_sharded_step(void* ctx, const void* gathered_prev_dev, void* gathered_next_dev);
int  smm_bgp_sharded_finish(void* ctx, const void* gathered_dev);
/* The p2p form of the sharded iteration: NO collective call at all.  The xGMI fabric of an MI355X node is point-to-point, so
 * the all-gather of the last-accepted records is done by the chains' accept step itself: every rank owns a WINDOW of device
 * memory that all other ranks map (HIP IPC between processes; plain device pointers between contexts of one process), a
 * chain's accept step stores its record, value and walk slot into every rank's window, and the next iteration's kernel reads
 * its own window.  Where the single shard needs one launch per iteration so does a shard (objfunc_norm, np == nm <= 4,
 * min_improve == 0, N_global <= 8192): every word in a window carries the iteration it belongs to, a reader that finds an older
 * one looks again (nobody waits for an acknowledgement, nothing is counted); the same objectives at 8192 < N_global <= 32768 (four
 * and eight shards of 4096): two launches, the exchange resolution reading the tagged words of its window itself and the chain kernel
 * pushing from its accept step; everywhere else: chain kernel + push kernel (stores, then one arrival count per 16 chains and rank)
 * + wait + resolve kernel.  The host enqueues nothing else.  Same results as every other form (bit-identical to the single shard).
 * smm.jl_amd/csrc/smm_p2p.hpp has the protocol.
 *   smm_bgp_p2p_init(ctx, handle_out, window_out): allocates this rank's window (rank = chain_offset / N, equal shards, at most
 *        8 ranks); handle_out (SMM_P2P_HANDLE_BYTES bytes, may be NULL) receives its hipIpcMemHandle_t for the other
 *        PROCESSES, window_out (may be NULL) its device pointer for other contexts of THIS process.
 *   smm_bgp_p2p_attach(ctx, rank, handle, window): rank's window, by IPC handle or by device pointer (exactly one non-NULL).
 *   smm_bgp_p2p_step(ctx, n): enqueues n iterations and returns (smm_sync waits).  All ranks call it with the same n, in the
 *        same order relative to each other's p2p calls (publications and pushes are counted).  A rank whose peers' stores never
 *        arrive gives up after ~4 s and reports SMM_ERR_HIP at the next smm_sync.  Where the context qualifies (smm_set_persistent,
 *        below) n >= 2 iterations behind a completed one are ONE launch per look-ahead window and rank; smm_sync of such steps is a
 *        rendezvous of the ranks (their error words travel through the windows): every rank must reach it.
 *   smm_bgp_p2p_finish(ctx): settles the last iteration into the context (required before smm_get_history / smm_get_state /
 *        the other stepping forms).  Callers must not destroy a context while a peer may still be stepping.
 *        A BARRIER ACROSS THE RANKS belongs between smm_bgp_p2p_finish (+ smm_sync) and the next smm_bgp_p2p_step: that step's
 *        first publication rewrites the windows with a new epoch, and a rank still in its finish would find the words of the
 *        last iteration replaced (a time-out in the tagged forms, other records without notice in the generic one).
 *        smm.jl_amd/dist.py::ShardedBGP.sync does it.
 *   Which of the forms a context steps in is decided from what every rank knows (population, objective, thresholds),
 *   never from a shard's own values.  A NaN value in an uploaded state (smm_set_state) reaches every window with the first
 *   publication: the rows form resolves such iterations on the exact values, the one-launch form (N_global <= 8192) has no
 *   second walk and reports SMM_ERR_HIP on every rank in the same iteration — step such a state once with smm_bgp_sharded_step
 *   (or as a single shard) first.  The persistent form reports it from inside its launch; the ranks agree on that at their
 *   rendezvous and replay the step on the forms above.
 *   What a shard in the persistent form sends per chain, iteration and PEER: the parameters and the value of its last accepted
 *   record as self-validating granules — (np + 1) x 16 bytes, 48 at two parameters; the rest of a record (prob, status, simulated
 *   moments) stays in the owner's window and is fetched by the one chain that continues from it (swap_ev_ij!, AlgoBGP.jl:734-749).
 *   The same holds for the shards of the objectives a whole tile evaluates (objfunc_norm with more than two parameters, SMM_OBJ_DENSE,
 *   SMM_OBJ_DENSE2, a map-reduce user objective; below): 816 bytes per chain, iteration and peer at np = 50 (BASELINE config 5), the
 *   donor's other granules read from its owner's window behind the objective.  The ring part of the window holds the context's own
 *   records: PR_K x N_global x RW x 16 bytes (RW = 104 at np = nm = 50: 13.6 MB at 4096 chains). */
#define SMM_P2P_HANDLE_BYTES 64
int  smm_bgp_p2p_init(void* ctx, void* ipc_handle_out, void** window_dev_out);
int  smm_bgp_p2p_attach(void* ctx, int32_t rank, const void* ipc_handle, void* window_dev);
int  smm_bgp_p2p_step(void* ctx, int32_t n_iters);
int  smm_bgp_p2p_finish(void* ctx);
/* the HIP stream all of the ctx's work is enqueued on (hipStream_t as void*).  (Large single shards, 8192 < N <= 32768, also own a
 * private second stream on which the NEXT window's exchange plan is computed ahead; the work on smm_stream waits for it through
 * events, so everything a caller can observe is ordered by smm_stream alone; smm_ctx_destroy drains both.) */
void* smm_stream(void* ctx);

/* batched evaluateObjective(m,p) (mprob.jl:175-188) for M parameter vectors
 * params [np][M] -> value[M], sim_moments[nm][M], status[M].  Used by tests and by
 * the other callers of evaluateObjective (slices.jl:153, econometrics.jl:42). */
int  smm_eval_batch(void* ctx, const double* params, int32_t M,
                    double* value, double* sim_moments, int8_t* status);
/* the same for objfunc_norm with options[:noseed] = true (ObjExamples.jl:71-75): evaluation i draws its own
 * shocks (generator keyed by base_seed + i) instead of the fixed seed-1234 matrix — the repetitions of
 * getSigma (econometrics.jl:125-145).  Also for user objectives registered with smm_register_user_objective_rng
 * (their stream keyed by base_seed + i); other objectives have no stream to re-key: SMM_ERR_INVALID_ARG. */
int  smm_eval_batch_noseed(void* ctx, const double* params, int32_t M, uint64_t base_seed,
                           double* value, double* sim_moments, int8_t* status);

int  smm_get_history(void* ctx, int32_t t0, int32_t t1, smm_history_t* out);

/* Chain summaries computed on the device from the history it holds: params / mean / median / CI / best / summary of the reference
 * (AlgoBGP.jl:117-206, 541-550) for every LOCAL chain of the context (a shard reports its own N chains; partner ids are global),
 * over the 0-based iterations [t0, t1), 0 <= t0 <= t1 <= completed iterations.  accepted_only != 0 selects the iterations with
 * accepted != 0 (params(c), AlgoBGP.jl:120-131), otherwise every iteration of the window.  Caller-allocated; any pointer may be NULL
 * (not returned; mean, median and quantile all NULL: no column is compacted).  The call is read-only (it settles, flushes and
 * synchronises like smm_get_history, and changes no state, history or generator).  Scratch: allocated by the first call, kept in the
 * ctx, freed with it — min(N x maxiter x (8 np + 4), max(256 MiB, 12 x maxiter)) bytes (a context holding more is reduced in
 * batches of chains and, past that, of parameters, each batch reading the window once more), plus the call's results
 * ((N + n_probs + (2 + n_probs) np N) x 8 + 16 N bytes, grown to the largest call's).  SMM_ERR_INVALID_ARG: NULL ctx or out, a bad
 * window, n_probs < 0, probs NULL with n_probs > 0, a prob outside [0, 1] or NaN, quantile without probs.
 *
 * Numerical contract — NumPy's readers (np.mean, np.median, np.quantile(method="linear"), np.argmin, np.bincount(...).argmax() on
 * the compacted column, as the Python host layer computes them), NOT Julia's Statistics, which sums differently.  Every operation
 * rounded on its own (no fma).  x = the selected draws of one parameter in iteration order, m = count, s = x sorted by the IEEE
 * total order (-0 before +0):
 *   pw(x, lo, n): n < 8: r = 0.0, r = r + x[lo+i] for i = 0..n-1;  n <= 128: r[k] = x[lo+k] (k < 8), r[k] = r[k] + x[lo+i+k] for
 *                 i = 8, 16, .. < n - n%8; s = ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then s = s + x[lo+i] for the n%8 last;
 *                 otherwise n2 = n/2 - (n/2)%8: pw(x, lo, n2) + pw(x, lo+n2, n-n2)          (numpy's pairwise sum)
 *   mean       = S / m with S = 0.0, S = S + pw(x, c, min(8192, m-c)) for c = 0, 8192, ..
 *   median     = the mean above of the middle draw(s): (0.0 + s[m/2]) / 1 for odd m, ((0.0 + s[m/2-1]) + s[m/2]) / 2 for even m
 *   quantile p = h = (m-1) p; h >= m-1: a = b = s[m-1], g = h + 1;  else j = floor(h), a = s[j], b = s[j+1], g = h - j;
 *                d = b - a; g >= 0.5 ? b - d (1 - g) : a + d g                              (numpy's _lerp, indexes clipped as numpy)
 *   a NaN among the selected draws: mean, median and every quantile NaN (count still reported); m == 0: NaN.
 *   best       = the first NaN value of the window if any, else its first minimum (over EVERY iteration of the window, as best(c));
 *                best_iter its 1-based iteration (t + 1); an empty window: NaN and 0.
 *   most_exchanged_with = the most frequent non-zero partner of the window, ties to the smallest id; 0 = no exchange.
 * numpy selects order statistics with a partition that does not order -0 and +0: its results and these can differ in the sign of
 * a zero, nowhere else. */
typedef struct {            /* caller-allocated; any pointer may be NULL = not computed                                        */
    int32_t* count;         /* [N]            draws selected in the window                                                     */
    double*  mean;          /* [np][N]                                                                                         */
    double*  median;        /* [np][N]                                                                                         */
    double*  quantile;      /* [n_probs][np][N]                                                                                */
    double*  best_value;    /* [N]   findmin of value over the window (all iterations, as best(c))                             */
    int32_t* best_iter;     /* [N]   1-based iteration of it                                                                   */
    int32_t* n_exchanged;   /* [N]   iterations with exchanged != 0                                                            */
    int32_t* most_exchanged_with; /* [N] mode of the non-zero partners (1-based global id), 0 = none                           */
} smm_chain_stats_t;
int  smm_get_chain_stats(void* ctx, int32_t t0, int32_t t1, int32_t accepted_only,
                         const double* probs, int32_t n_probs, smm_chain_stats_t* out);

/* Convergence diagnostics computed on the device from the history it holds: each LOCAL chain's accept rate, and for each of its
 * S = np + 1 series (s < np: parameter s; s = np: the objective value) the autocorrelation, the effective sample size by Geyer's initial
 * monotone sequence, and the split R-hat of groups of local chains, over the 0-based iterations [t0, t1), n = t1 - t0 (a shard reports
 * its own N chains; a group is made of local chains only).  Caller-allocated; any pointer may be NULL (not returned).  Read-only and
 * ordered like smm_get_chain_stats (it settles, flushes and synchronises, and changes no state, history or generator), and uses its
 * scratch, grown where needed to one chain's maxiter x 8 S bytes (a context holding more is reduced in batches of chains), plus
 * ((5 + n_acf) S + 2) N x 8 bytes of results.  group [N]: the chain's group in [0, n_groups), or -1 for none.  SMM_ERR_INVALID_ARG:
 * NULL ctx or out, t0 < 0, t1 > completed iterations, n < 4, max_lag outside [1, n - 1], n_acf outside [0, max_lag + 1],
 * n_groups < 0, group NULL with n_groups > 0, a group id outside [-1, n_groups), rhat with n_groups == 0.
 *
 * Numerical contract (every operation rounded on its own, no fma).  S(.) = the chain-stats chunked pairwise sum (bit for bit np.sum of
 * a contiguous float64 array), mean(.) = the chain-stats mean:
 *   series    : a(t) = the last row r <= t with accepted[r] != 0, looking back before t0 as far as row 0 (swapped rows have accepted = 1,
 *               AlgoBGP.jl:734-749, so a(t) is the chain's state, lastAccepted, AlgoBGP.jl:209-215); x_s(t) = params[a(t)][s] for
 *               s < np, x_np(t) = value[a(t)] (= curr_val[t] for every history the library writes).  No such row: non-finite.
 *   accept    : (double)A / (double)E, E = window iterations with exchanged == 0, A = those of them with accepted != 0 (NaN when
 *               E == 0; set_acceptRate!, AlgoBGP.jl:253-257, restricted to the window)
 *   acov_k    = S(d[0:n-k] * d[k:n]) / n with d = x - mean(x): np.sum(d[:n-k] * d[k:]) / n;  rho_k = acov_k / acov_0
 *   ESS       : P_j = rho_2j + rho_2j+1 while 2j + 1 <= max_lag; J = the smallest j >= 1 with !(P_j > 0), else the number of pairs
 *               (status 1); Q_0 = P_0, Q_j = P_j < Q_j-1 ? P_j : Q_j-1 (j < J); T = ((0.0 + Q_0) + Q_1) + .. + Q_J-1;
 *               tau = -1.0 + 2.0 T; ess = n / tau
 *   status    : first match wins: 3 a non-finite entry in the series (ess and every acf entry NaN); 2 acov_0 == 0 or !(tau > 0) (ess NaN,
 *               acf as the arithmetic gives); 1 max_lag reached before truncation (ess as above: it overstates); 0 otherwise.  A
 *               negative ESS is never reported.
 *   split R-hat of group g, series s: h = n / 2 (integer); the members of g in ascending local index each give x[0:h] then x[n-h:n];
 *               each half y: mu = mean(y), var = S((y - mu) * (y - mu)) / (h - 1) (np.var(y, ddof=1)).  Over the 2k halves:
 *               W = mean(vars), v = S((mu_i - mean(mus)) * (mu_i - mean(mus))) / (2k - 1), var_plus = ((h - 1.0) / h) W + v,
 *               rhat = sqrt(var_plus / W).  NaN when g is empty or a member's series has status 3; otherwise the arithmetic decides.
 * The device stops computing lags once the sequence is truncated and every requested acf lag is done: the results are those of
 * computing every lag up to max_lag. */
typedef struct {            /* caller-allocated; any pointer may be NULL = not computed; S = np + 1 series                       */
    double*  accept_rate;   /* [N]               accepted among the window's non-exchanged iterations                         */
    double*  ess;           /* [S][N]            series s < np: parameter s; s = np: the objective value                      */
    int32_t* status;        /* [S][N]            0 ok, 1 max_lag reached first, 2 undefined, 3 non-finite series             */
    double*  acf;           /* [n_acf][S][N]     rho_k, k = 0 .. n_acf - 1                                                    */
    double*  rhat;          /* [n_groups][S]     split R-hat of each group                                                    */
} smm_chain_diag_t;
int  smm_get_chain_diag(void* ctx, int32_t t0, int32_t t1, int32_t max_lag, int32_t n_acf,
                        const int32_t* group /* [N] or NULL */, int32_t n_groups, smm_chain_diag_t* out);

/* Pooled summaries of groups of chains computed on the device from the history it holds: the posterior of a group's pooled draws (mean,
 * median, quantiles, covariance over every member's draws), over the 0-based iterations [t0, t1).  Group g is made of the LOCAL chains
 * with group[c] == g (-1: in no group; a shard reports its own groups of local chains), in ascending local index; group NULL with
 * n_groups == 1: every local chain in group 0.  Pooled column of group g, parameter k: the concatenation over the members in that order of
 * each member's selected draws of the window in iteration order, selected exactly as smm_get_chain_stats selects them (accepted_only) —
 * bit for bit np.concatenate([params(c, accepted_only)[k] for c in members]).  Caller-allocated; any pointer may be NULL (not returned).
 * Read-only and ordered like smm_get_chain_stats (it settles, flushes and synchronises, and changes no state, history or generator).  It
 * uses smm_get_chain_stats' scratch, grown where needed to N x maxiter x 8 bytes (one parameter's pooled columns) and, for cov, to
 * np x 8192 x 8 bytes (every parameter of one chunk); pooled columns that do not fit are reduced in batches of parameters, and the
 * covariance in batches of chunks, each batch reading the window once more.  Results: ((2 + n_probs) np + np np) n_groups x 8 bytes and
 * the plan's tables (chunk sums, ranks, up to 32 MiB of histograms).  SMM_ERR_INVALID_ARG: NULL ctx or out, a bad window, n_groups < 0,
 * group NULL with n_groups != 1, a group id outside [-1, n_groups), n_probs < 0, probs NULL with n_probs > 0, a prob outside [0, 1] or
 * NaN, quantile without probs.
 *
 * Numerical contract: smm_get_chain_stats' and smm_get_chain_cov's, on the pooled column x of m = count draws (every operation rounded on
 * its own, no fma; ranks and counts 64-bit):
 *   mean       = the chain-stats mean: S / m, S = S + pw(x, c, min(8192, m-c)) for c = 0, 8192, .. (chunks from the group's first draw,
 *                straddling the members' boundaries)
 *   median, quantile p = the chain-stats order statistics of x (numpy's _lerp); the -0/+0 caveat of smm_get_chain_stats holds
 *   cov_jk     = S(d_j * d_k) / (m - 1), d_j = x_j - mean_j, S the same chunked pairwise sum; cov_kj the same value
 *   a NaN among the group's draws: mean, median and every quantile NaN (and it propagates into cov); m == 0: NaN everywhere, count 0;
 *   m < 2: cov NaN. */
typedef struct {            /* caller-allocated; any pointer may be NULL = not computed                                        */
    int64_t* count;         /* [n_groups]                 selected draws pooled in the group                                   */
    int32_t* n_chains;      /* [n_groups]                 member chains                                                        */
    double*  mean;          /* [n_groups][np]                                                                                  */
    double*  median;        /* [n_groups][np]                                                                                  */
    double*  quantile;      /* [n_probs][n_groups][np]                                                                         */
    double*  cov;           /* [n_groups][np][np]  both triangles                                                              */
} smm_group_stats_t;
int  smm_get_group_stats(void* ctx, int32_t t0, int32_t t1, int32_t accepted_only,
                         const int32_t* group /* [N] or NULL */, int32_t n_groups,
                         const double* probs, int32_t n_probs, smm_group_stats_t* out);

/* Histograms of the draws of groups of chains computed on the device from the history it holds, over the 0-based iterations [t0, t1):
 * for each group and parameter numpy's np.histogram(x, bins, range), and for each pair (j, k) of parameters np.histogram2d(x_j, x_k,
 * bins2), bit for bit.  Groups as in smm_get_group_stats (group[c] in [-1, n_groups), -1: in no group; group NULL with n_groups == 1:
 * every local chain in group 0; a shard reports its own local chains; per-chain histograms: group = 0 .. N-1).  Column x of group g,
 * parameter k: the members' selected rows in ascending local index, each in iteration order:
 *   select 0: every row of the window;  1: the rows with accepted != 0 (bit for bit np.concatenate([params(c, accepted_only)[k] for c in
 *   members]), smm_get_chain_stats' selection);  2: the state series x(t) = params[a(t)] of smm_get_chain_diag (a(t) looks back before
 *   t0; a row with no such a(t) is NaN) — the MCMC marginal, weighted by holding time.  count[g]: the selected rows of the members.
 * Caller-allocated; any pointer may be NULL (not returned).  Read-only and ordered like smm_get_chain_stats (it settles, flushes and
 * synchronises, and changes no state, history or generator).  Device memory (the reducers' result buffer): N x (12 + 20 np) bytes of
 * per-chain ranges and lists plus the tables of a batch of groups, each group taking np ((bins + 1) + bins + (bins2 + 1)) x 8 + n_pairs bins2
 * bins2 x 8 bytes; a batch holds as many groups as fit 256 MiB (at least one), and larger results are produced and copied out batch by
 * batch.  Counts are integers added with integer atomics: they do not depend on the order of additions, and counts over a shared given
 * range add across shards.  SMM_ERR_INVALID_ARG: NULL ctx or out, a bad window, select outside [0, 2], n_groups < 0, group NULL with
 * n_groups != 1, a group id outside [-1, n_groups), bins outside [1, 65536], a range row not finite or with lo > hi, n_pairs outside
 * [0, np np], pairs NULL with n_pairs > 0, a pair entry outside [0, np), bins2 outside [1, 512] with n_pairs > 0, hist2 or edges2
 * requested with n_pairs == 0.
 *
 * Numerical contract (every operation rounded on its own, no fma):
 *   outer edges : range given: (lo, hi) = range[k] for every group;  else the min and max of the column, (0, 1) for an empty column, and
 *                 status 1 for a NaN or +-inf in it (numpy raises): lo, hi, edges NaN.  Then lo == hi: lo = lo - 0.5, hi = hi + 0.5.
 *                 hi - lo not finite: status 2, edges NaN (numpy's index arithmetic is undefined there; the one stated departure).
 *                 Autodetected lo, hi and edges may differ from numpy's in the sign of a zero; counts never do.
 *   edges       : numpy's linspace(lo, hi, b + 1): delta = hi - lo, step = delta / b; step != 0: e[i] = i step + lo, else
 *                 e[i] = (i / b) delta + lo; e[b] = hi.  (b = bins for edges, bins2 for edges2.)
 *   1-D         : numpy's uniform-bins path.  Edges not strictly increasing (a narrow range at a large magnitude): status 3 (numpy raises
 *                 "Too many bins"), 1-D counts 0, edges as computed.  Otherwise, for each x: kept only if x >= lo && x <= hi (NaN
 *                 dropped); f = ((x - lo) / delta) * bins, i = (int64)f; i == bins: i = bins - 1; x < e[i]: i = i - 1; then
 *                 x >= e[i + 1] && i != bins - 1: i = i + 1; hist[i] += 1.
 *   2-D         : numpy's histogramdd, per axis over edges2 of that parameter's outer edges: i = searchsorted(e, x, side='right') (exact
 *                 for repeated edges; NaN sorts last); x == e[bins2]: i = i - 1; counted in cell (i_j - 1, i_k - 1) only when both axes
 *                 land in [1, bins2].  A pair with status 1 or 2 on either axis: counts 0 (status 3 does not apply to the 2-D axes).
 * Counts are np.histogram's and np.histogram2d's (as int64): density and any weighting are the caller's. */
typedef struct {            /* caller-allocated; any pointer may be NULL = not returned                                        */
    int64_t* count;         /* [G]                     rows selected for the group (NaN / outliers included)                   */
    int32_t* status;        /* [G][np]                 0 ok, 1 autodetected range not finite, 2 width not finite, 3 1-D edges repeat */
    double*  lo;            /* [G][np]                 outer edges actually used (after numpy's +-0.5)                         */
    double*  hi;            /* [G][np]                                                                                         */
    double*  edges;         /* [G][np][bins + 1]       numpy's linspace(lo, hi, bins + 1)                                      */
    int64_t* hist;          /* [G][np][bins]           np.histogram counts                                                     */
    double*  edges2;        /* [G][np][bins2 + 1]      linspace(lo, hi, bins2 + 1), the 2-D axes                               */
    int64_t* hist2;         /* [G][n_pairs][bins2][bins2]  np.histogram2d counts, rows = the pair's first parameter            */
} smm_histogram_t;
int  smm_get_histogram(void* ctx, int32_t t0, int32_t t1, int32_t select, const int32_t* group /* [N] or NULL */, int32_t n_groups,
                       int32_t bins, const double* range /* [np][2] or NULL */, const int32_t* pairs /* [n_pairs][2] */,
                       int32_t n_pairs, int32_t bins2, smm_histogram_t* out);

/* The population per iteration computed on the device from the history it holds: for each kept iteration of the 0-based window
 * [t0, t1) and each group of chains, the across-chain mean, variance, median and quantiles of every series, the members' accept,
 * exchange and failure counts, and the best value among them — the readers above collapse the iterations of a window per chain or
 * group; this one collapses the member chains of a group per iteration.  Row i is iteration t0 + i stride, i < nt =
 * ceil((t1 - t0) / stride) (0 for an empty window).  Groups as in smm_get_group_stats / smm_get_histogram (group[c] in [-1, n_groups),
 * -1: in no group; group NULL with n_groups == 1: every local chain in group 0; a shard reports its own local chains; per-chain
 * traces: group = 0 .. N-1), members in ascending local index.  S = np + 1 series, or np + 1 + nm with moments != 0: s < np parameter s,
 * s == np the objective value, s = np + 1 + k simulated moment k.  Column x of (row i, group g, series s), t = t0 + i stride:
 *   select 0: every member's row t itself — params[t], value[t], sim_moments[t] (what params(c, accepted_only = false) plots);
 *   1: the same of the members with accepted[t] != 0 only, so count varies with t;
 *   2: the state series of smm_get_chain_diag — every member's row a(t), the last row r <= t with accepted[r] != 0, looking back
 *      before t0 as far as row 0; that row supplies parameters, value and moments alike; a member with no such row contributes NaN.
 * Caller-allocated; any pointer may be NULL (not returned; mean, var, median and quantile all NULL: no column is gathered).  Read-only
 * and ordered like smm_get_chain_stats (it settles, flushes and synchronises, and changes no state, history or generator).  Device
 * memory is bounded: the kept iterations go in batches.  A kept iteration takes M x (8 S + 4) bytes (+ 4) of smm_get_chain_stats'
 * scratch (M <= N member chains: the columns and the state table; the scratch is grown where needed to one series of one iteration,
 * at most 12 N + 4 bytes, and an iteration whose columns do not fit goes in batches of series, each reading its rows once more) and
 * n_groups x ((3 + n_probs) S x 8 + 28) bytes of the result buffer; a batch holds as many kept iterations as fit the scratch and
 * 256 MiB of results (at least one), and results are produced and copied out batch by batch, so nt x n_groups x S may be gigabytes
 * of host memory (per-chain groups) without being so on the device.  Plus 4 (n_groups + 1 + M) + 8 n_probs bytes of lists.
 * SMM_ERR_INVALID_ARG: NULL ctx or out, a bad window, stride < 1, select outside [0, 2], n_groups < 0, group NULL with n_groups != 1,
 * a group id outside [-1, n_groups), n_probs < 0, probs NULL with n_probs > 0, a prob outside [0, 1] or NaN, quantile without probs.
 *
 * Numerical contract: numpy's on the contiguous column x of the m = count selected members in ascending local index (every operation
 * rounded on its own, no fma):
 *   mean       = the chain-stats mean (the pw sum in chunks of 8192, divided by m): np.mean(x)
 *   var        = S((x - mu) * (x - mu)) / (m - 1), mu = mean(x), S the same chunked pairwise sum (smm_get_chain_diag's half variance):
 *                np.var(x, ddof = 1); m < 2: NaN
 *   median, quantile p = the chain-stats order statistics of x (numpy's _lerp); the -0/+0 caveat of smm_get_chain_stats holds
 *   a NaN in the column: mean, var, median and every quantile NaN (count still reported); m == 0: NaN
 *   best       = the first NaN of value[t] over the group's members if any, else its first minimum, in ascending local index
 *                (np.argmin; EVERY member, whatever select); best_chain its 1-based GLOBAL chain id; an empty group: NaN and 0. */
typedef struct {            /* caller-allocated; any pointer may be NULL = not returned; S = np + 1 (+ nm with moments != 0)          */
    int32_t* iter;          /* [nt]                  the 0-based iteration of row i: t0 + i * stride                                   */
    int32_t* n_chains;      /* [G]                   member chains                                                                      */
    int32_t* count;         /* [nt][G]               members selected at that iteration (= n_chains for select 0 and 2)                 */
    int32_t* n_accepted;    /* [nt][G]               members with accepted != 0 and exchanged == 0                                      */
    int32_t* n_exchanged;   /* [nt][G]               members with exchanged != 0                                                        */
    int32_t* n_failed;      /* [nt][G]               members with status < 0                                                            */
    double*  mean;          /* [nt][G][S]                                                                                               */
    double*  var;           /* [nt][G][S]            np.var(x, ddof = 1)                                                                */
    double*  median;        /* [nt][G][S]                                                                                               */
    double*  quantile;      /* [n_probs][nt][G][S]                                                                                      */
    double*  best_value;    /* [nt][G]               np.argmin order over the members' value[t] (every member, whatever select)         */
    int32_t* best_chain;    /* [nt][G]               1-based GLOBAL chain id of it; 0 for an empty group                                */
} smm_trace_t;
int  smm_get_trace(void* ctx, int32_t t0, int32_t t1, int32_t stride, int32_t select, int32_t moments,
                   const int32_t* group /* [N] or NULL */, int32_t n_groups,
                   const double* probs, int32_t n_probs, smm_trace_t* out);

/* Rank-normalised convergence diagnostics of groups of chains computed on the device from the history it holds (Vehtari, Gelman, Simpson,
 * Carpenter, Buerkner 2021): the rank-normalised split R-hat (bulk, folded, and their maximum), the multi-chain bulk, tail and mean ESS,
 * and every chain's rank histogram (the rank plot), for each group g and each of smm_get_chain_diag's S = np + 1 state series, over the
 * 0-based iterations [t0, t1), n = t1 - t0.  Group g is made of the LOCAL chains with group[c] == g (-1: in no group; a shard reports its
 * own chains and its own groups), in ascending local index; group NULL with n_groups == 1: every local chain in group 0.
 * Caller-allocated; any pointer may be NULL (not returned).  Read-only and ordered like smm_get_chain_stats (it settles, flushes and
 * synchronises, and changes no state, history or generator; it can sit between smm_bgp_step_async calls).  It uses smm_get_chain_stats'
 * scratch, grown where needed to one series of the largest group: 72 bytes per pooled value (values, keys, indices, ranks, scores) and
 * (80 + 32 min(256, max_lag + 1)) bytes per split chain, 256 KB more for a column above 8192 values; what does not fit is reduced in
 * batches of series and, where one series of every group does not fit, of groups, each batch reading the window once more.  Results:
 * 31 S n_groups x 8 bytes and, with rank_hist, n_bins S N x 8.  SMM_ERR_INVALID_ARG: NULL ctx or out, t0 < 0, t1 > completed iterations,
 * n < 8, max_lag outside [1, h - 1] (h = n / 2), n_bins < 0, rank_hist with n_bins == 0, n_groups < 1, group NULL with n_groups != 1, a
 * group id outside [-1, n_groups), a group whose pooled column would hold more than 2^31 - 1 values; the outputs are then untouched.
 *
 * Numerical contract (every operation rounded on its own, no fma; counts and ranks are 64-bit).  S(.), mean(.), the median and the
 * quantile are the chain-stats ones; x_s(t) is smm_get_chain_diag's state series:
 *   split chains : h = n / 2; the k members of g in ascending local index each give x[0:h] then x[n-h:n]: m = 2 k chains of length h,
 *                  pooled in that order into M = m h values.
 *   rank2_i      = 2 L + E + 1, L the number of pooled values strictly less than x_i, E the number equal to it, itself included (twice the
 *                  average rank); -0.0 and +0.0 are equal.
 *   z_i          = ndtri(((double)rank2_i * 0.5 - 0.375) / ((double)M + 0.25)), ndtri = Wichura's AS 241 PPND16 with its operations in
 *                  their order, the logarithm smm_log, the square root IEEE's.
 *   R-hat of m chains y_j: mu_j = mean(y_j), var_j = S((y_j - mu_j) (y_j - mu_j)) / (h - 1), W = mean(var), v = S((mu_j - mean(mu))
 *                  (mu_j - mean(mu))) / (m - 1), var_plus = ((h - 1.0) / h) W + v, rhat = sqrt(var_plus / W): smm_get_chain_diag's
 *                  arithmetic on the chains as they stand.  rhat_bulk: of the z chains.  rhat_folded: of the normal scores of
 *                  f_i = |x_i - med|, med the median of the M pooled values (taken with -0.0 as +0.0).  rhat_rank = rhat_bulk >
 *                  rhat_folded ? rhat_bulk : rhat_folded, NaN if either is.
 *   ESS of m chains y_j: d_j = y_j - mu_j, acov_{j,t} = S(d_j[0:h-t] d_j[t:h]) / h, A_t = mean_j(acov_{j,t}), rho_0 = 1.0,
 *                  rho_t = 1.0 - (W - A_t) / var_plus; P_j, J, Q_j, T and tau = -1.0 + 2.0 T from the rho exactly as in
 *                  smm_get_chain_diag; ess = (double)M / tau.  This is the library's Geyer truncation (initial positive, monotone
 *                  sequence) applied to the combined autocorrelation: Stan's estimator without its extra odd-lag term and without its
 *                  M log10 M cap.  ess_bulk: of the z chains; ess_mean: of the x chains; ess_tail: the smaller of the ESS of the
 *                  indicator chains (x <= q05 ? 1.0 : 0.0) and (x <= q95 ? 1.0 : 0.0), q the quantiles 0.05 and 0.95 of the pooled
 *                  values, NaN if either is.
 *   status       : [0] bulk, [3] mean: 2 when W == 0, var_plus == 0 or !(tau > 0) (ess NaN), else 1 when max_lag came before the
 *                  truncation, else 0; [2] tail: the larger of its two chains' statuses; [1] folded: 2 when W == 0 or var_plus == 0,
 *                  else 0.  A non-finite pooled value: 3 in all four, every statistic of the cell NaN and no count in rank_hist from
 *                  it.  A group without members: 2 and NaN.
 *   rank_hist    : a value of rank rank2 falls in bin ((rank2 - 1) n_bins) / (2 M) (64-bit integer division); chain c collects its 2 h
 *                  values of series s in rank_hist[.][s][c]; a chain in no group gets zeros.
 * The device stops computing the lags of a cell once its sequence is truncated: the results are those of computing every lag up to
 * max_lag. */
typedef struct {               /* caller-allocated; any pointer may be NULL; S = np + 1 series as in smm_chain_diag_t */
    double*  rhat_rank;        /* [n_groups][S]  max(bulk, folded) rank-normalised split R-hat            */
    double*  rhat_bulk;        /* [n_groups][S]                                                            */
    double*  rhat_folded;      /* [n_groups][S]                                                            */
    double*  ess_bulk;         /* [n_groups][S]  multi-chain ESS of the rank-normalised split chains       */
    double*  ess_tail;         /* [n_groups][S]  min of the ESS of I(x <= q05) and of I(x <= q95)          */
    double*  ess_mean;         /* [n_groups][S]  multi-chain ESS of the raw split chains                   */
    int32_t* status;           /* [4][n_groups][S]  for bulk, folded, tail, mean: 0 ok, 1 max_lag first, 2 undefined, 3 non-finite */
    int64_t* rank_hist;        /* [n_bins][S][N] each chain's pooled ranks, binned: the rank plot          */
} smm_rank_diag_t;
int  smm_get_rank_diag(void* ctx, int32_t t0, int32_t t1, int32_t max_lag, int32_t n_bins,
                       const int32_t* group /* [N] or NULL */, int32_t n_groups, smm_rank_diag_t* out);

/* The posterior sample itself: thinned draws of groups of chains, exported row by row from the history the device holds — parameters,
 * value, simulated moments and where each row comes from (chain and iteration) — without downloading the history.  Window, groups and
 * select as in smm_get_histogram and smm_get_trace: the 0-based iterations [t0, t1), n = t1 - t0; group g is made of the LOCAL chains
 * with group[c] == g (-1: in no group; a shard reports its own chains), in ascending local index; group NULL with n_groups == 1: every
 * local chain in group 0.  select 0: all rows; 1: the rows with accepted != 0; 2: the state series, row a(t) = the last accepted row
 * r <= t, looking back before t0 (a t without one gives a row of quiet NaNs with src_iter 0).
 * Read-only and ordered like smm_get_chain_stats (it settles, flushes and synchronises, and changes no state, history or generator; it
 * can sit between smm_bgp_step_async calls).
 *
 * Selection contract (integers only):
 *   per chain : chain c's selected rows of the window in iteration order are s_c[0 .. m_c) (select 0, 2: m_c = n, s_c[i] = t0 + i).
 *               Thinning keeps s_c[i] with i % thin == 0: m'_c = ceil(m_c / thin) rows.
 *   pool      : group g's pooled sequence is the members' kept rows, member after member in ascending local index; its length m_g is
 *               count[g].
 *   cap       : K = max_rows.  m_g <= K: every pooled row is written.  Otherwise exactly K rows: row j is pooled position
 *               floor(j m_g / K), in 64-bit integers (strictly increasing, as m_g > K): systematic thinning, spread evenly over the
 *               members' series.
 *   packing   : the groups in order, row0[g + 1] = row0[g] + min(m_g, K); a group without members or without rows writes none.
 *   bits      : every double written is the history's double, bit for bit, NaNs included; nothing is computed on a value.
 * Sizing call: with params, value, sim_moments, chain, iter and src_iter all NULL the call fills count, n_chains and row0 only and
 * ignores rows_cap; the caller sizes its arrays by row0[n_groups] = R.  Row call: the arrays hold rows_cap rows; R > rows_cap is
 * SMM_ERR_INVALID_ARG with R in the message.  SMM_ERR_INVALID_ARG also for: NULL ctx or out, t0 < 0, t1 < t0, t1 > completed iterations,
 * select outside [0, 2], n_groups < 0, group NULL with n_groups != 1, a group id outside [-1, n_groups), thin < 1, max_rows outside
 * [1, 1 << 24] (j m_g then stays below 2^63 at any population and capacity), rows_cap < 0 in a row call.  On an error nothing is written.
 * Device memory: no list of selected iterations is built.  Select 1 and 2 keep one 64-bit mask word and one 32-bit running count per
 * chain and 64 iterations (of the window; of [0, t1) for select 2) in smm_get_chain_stats' scratch, in batches of chains where they do
 * not fit; the rows are produced and copied out in batches of at most 256 MB at 8 (np + 1 + nm) + 12 bytes a row. */
typedef struct {            /* caller-allocated; any pointer may be NULL = not returned                          */
    int64_t* count;         /* [G]      draws of the group after per-chain thinning, before the cap (m_g)       */
    int32_t* n_chains;      /* [G]      member chains                                                            */
    int64_t* row0;          /* [G + 1]  group g's rows are [row0[g], row0[g + 1]); row0[G] = R, the rows written */
    double*  params;        /* [R][np]  ROW-major: one draw per row                                              */
    double*  value;         /* [R]                                                                               */
    double*  sim_moments;   /* [R][nm]                                                                           */
    int32_t* chain;         /* [R]      1-based GLOBAL chain id (as smm_get_trace's best_chain)                  */
    int32_t* iter;          /* [R]      1-based iteration t + 1 the draw stands for                              */
    int32_t* src_iter;      /* [R]      1-based iteration of the row that supplied it (= iter for select 0, 1;
                                        a(t) + 1 for select 2, 0 where there is none)                            */
} smm_draws_t;
int  smm_get_draws(void* ctx, int32_t t0, int32_t t1, int32_t select, const int32_t* group /* [N] or NULL */,
                   int32_t n_groups, int32_t thin, int32_t max_rows, int64_t rows_cap, smm_draws_t* out);

/* The simulated moments of groups of chains computed on the device from the history it holds: the first table of an SMM paper (the data
 * moments next to the simulated moments at the estimate), and from the same pooled draws the Jacobian dm/dtheta linearised over the
 * posterior (the regression of the simulated moments on the parameters over a group's draws), the sensitivity matrix of Andrews,
 * Gentzkow & Shapiro (2017) and sandwich standard errors — no further evaluation of the objective and no finite-difference step.
 * Window and groups as in smm_get_group_stats: the 0-based iterations [t0, t1); group g is made of the LOCAL chains with group[c] == g
 * (-1: in no group; a shard reports its own chains), in ascending local index; group NULL with n_groups == 1: every local chain in
 * group 0.  select as in smm_get_histogram: 0 every row of the window; 1 the rows with accepted != 0; 2 the state series, row a(t) of
 * smm_get_chain_diag supplying the parameters and the simulated moments alike (a(t) looks back before t0; a row with no a(t) is NaN) —
 * the MCMC posterior itself, weighted by holding time.  Caller-allocated; any pointer may be NULL (not computed).  Read-only and ordered
 * like smm_get_chain_stats (it settles, flushes and synchronises, and changes no state, history or generator).  It uses
 * smm_get_chain_stats' scratch, grown where needed to N x maxiter x 8 bytes (one pooled column) and, for the covariances, to
 * (np + nm) x 8192 x 8 bytes (every joint column of one chunk); pooled columns that do not fit are reduced in batches of columns, and
 * the covariance in batches of chunks (whose (np + nm)^2 pair sums per chunk stay under 256 MiB of the result buffer), each batch
 * reading the window once more.  SMM_ERR_INVALID_ARG: NULL ctx or out, a bad window, select outside [0, 2], n_groups < 0, group NULL
 * with n_groups != 1, a group id outside [-1, n_groups), n_probs < 0, probs NULL with n_probs > 0, a prob outside [0, 1] or NaN,
 * m_quantile without probs, ridge negative or not finite; nothing is written then.
 *
 * Numerical contract (every operation rounded on its own, no fma; counts and ranks 64-bit):
 *   pooled columns : the members' selected rows in member order, then iteration order, m = count of them.  Joint column k < np is the
 *                parameter k of the row; column np + k is the simulated moment k stored behind the parameters in the same record;
 *                D = np + nm.
 *   mean, median, quantile p = the chain-stats ones on the pooled column (chunks of 8192 counted from the group's first row, pw,
 *                numpy's _lerp; the -0/+0 caveat of smm_get_chain_stats holds).
 *   cov_ab     = S(d_a * d_b) / (m - 1), d centred by the column's own mean above, S the chunked pairwise sum: smm_get_group_stats'
 *                covariance over the D joint columns.  cov_pp = the block a, b < np (bit for bit smm_get_group_stats' cov on select
 *                1), cov_pm[j][k] = cov_{j, np + k}, cov_mm[k][l] = cov_{np + k, np + l}; mirrored entries hold the same value.
 *   fit_z_k    = (m_mean_k - mom_k) / sqrt(cov_mm_kk): the data moment's distance from the posterior predictive, in its standard
 *                deviations.
 *   Cholesky   : A = cov_pp with A_jj = C_jj + ridge * C_jj.  For k = 0..np-1, j = 0..k: s = A_kj; s = s - L_ki * L_ji for i = 0..j-1
 *                in that order; j == k: L_kk = sqrt(s), status 3 when !(s > 0); otherwise L_kj = s / L_jj (smm_adapt_proposal's order).
 *   solve(L, b): y_i = (b_i - L_i0 y_0 - .. - L_i,i-1 y_i-1) / L_ii for i = 0..np-1, then x_i = (y_i - L_i+1,i x_i+1 - .. -
 *                L_np-1,i x_np-1) / L_ii for i = np-1..0; the products subtracted one by one in ascending index.
 *   jac        : J = Cov(m, theta) Cov(theta, theta)^-1, row k = solve(L, column k of cov_pm).
 *   weights    : s_k = w_k if it is finite and not zero, else 1.0; W_k = 1.0 / (s_k * s_k) — objfunc_norm's reading of the weights,
 *                ((sim - mom) / w)^2; a NaN weight means no weight.
 *   sens       : Lambda = -(J'WJ)^-1 J'W.  B_ij = ((J_0i * W_0) * J_0j + (J_1i * W_1) * J_1j) + .., from 0.0 over k ascending; its
 *                lower Cholesky factor as above without a ridge, status 4 when a pivot is not > 0; column k of Lambda =
 *                solve(L_B, b) with b_i = -(J_ki * W_k).
 *   se_j       = sqrt(S), S = 0.0, S = S + (Lambda_jk * Lambda_jk) * (s_k * s_k) over k ascending; sqrt and / are IEEE.  se takes the
 *                weights as the data moments' standard deviations, Lambda diag(s^2) Lambda'; a caller with a full covariance Sigma
 *                of the data moments computes Lambda Sigma Lambda' from sens.
 *   status     : the first that applies: 1 count < 2 (the covariances and everything derived from them NaN); 2 a non-finite value
 *                among the selected parameters or moments (everything but count and n_chains NaN); 3 a pivot of the factor of A is
 *                not > 0 (jac, sens, se NaN); 4 a pivot of the factor of J'WJ is not > 0 (sens, se NaN); 0 otherwise. */
typedef struct {            /* caller-allocated; any pointer may be NULL = not computed; G = n_groups                          */
    int64_t* count;         /* [G]               selected rows pooled in the group                                             */
    int32_t* n_chains;      /* [G]               member chains                                                                 */
    int32_t* status;        /* [G]               0 ok, 1 fewer than 2 rows, 2 non-finite value, 3 Cov(theta) not PD, 4 J'WJ not PD */
    double*  p_mean;        /* [G][np]           pooled parameter mean                                                         */
    double*  m_mean;        /* [G][nm]           pooled simulated-moment mean                                                  */
    double*  m_median;      /* [G][nm]                                                                                         */
    double*  m_quantile;    /* [n_probs][G][nm]                                                                                */
    double*  cov_pp;        /* [G][np][np]       parameter covariance                                                          */
    double*  cov_pm;        /* [G][np][nm]       parameter-moment covariance                                                   */
    double*  cov_mm;        /* [G][nm][nm]       moment covariance                                                             */
    double*  fit_z;         /* [G][nm]           (m_mean - mom) / sqrt(diag cov_mm)                                            */
    double*  jac;           /* [G][nm][np]       J = Cov(m, theta) Cov(theta, theta)^-1                                        */
    double*  sens;          /* [G][np][nm]       Lambda = -(J'WJ)^-1 J'W                                                       */
    double*  se;            /* [G][np]           sqrt(diag(Lambda diag(s^2) Lambda'))                                          */
} smm_moment_stats_t;
int  smm_get_moment_stats(void* ctx, int32_t t0, int32_t t1, int32_t select, const int32_t* group /* [N] or NULL */,
                          int32_t n_groups, const double* probs, int32_t n_probs, double ridge, smm_moment_stats_t* out);

/* The regression-adjusted posterior of groups of chains, computed on the device from the history it holds: the local-linear adjustment
 * of Beaumont, Zhang & Balding (2002).  A chain keeps a draw whose simulated moments lie near the data moments, not at them, so every
 * posterior over the history is an ABC posterior at a non-zero tolerance; here the draws of a group are weighted by how close their
 * simulated moments are to the data, the parameters are regressed on the moment discrepancy, and every draw is moved to where it would
 * lie at zero discrepancy, theta* = theta - beta'(s - s_obs).  No further evaluation of the objective.  Window, groups and select are
 * exactly those of smm_get_moment_stats (select 0 all rows, 1 the accepted rows, 2 the state series through a(t); a shard reports its own
 * local chains; group NULL with n_groups == 1: every local chain in group 0).  tol is the accepted fraction, in (0, 1]; kernel 0 is the
 * uniform kernel, 1 Epanechnikov's; scale NULL or nm values, each finite and > 0 (the usual per-moment standard deviation is sqrt(diag
 * cov_mm) of smm_get_moment_stats); ridge finite and >= 0.  Caller-allocated; any pointer may be NULL (not computed).  Read-only and
 * ordered like smm_get_chain_stats (it settles, flushes and synchronises, and changes no state, history or generator).  Device memory:
 * smm_get_chain_stats' scratch, grown where needed to 2 x N x maxiter x 8 bytes (the distance column, later the integer weights, and one
 * column of adjusted parameters) plus (np + nm + 2) x 8192 x 8 bytes (every joint column of one chunk, the weight and its square); the
 * rows are taken in batches of chunks (whose (np + nm)^2 pair sums per chunk stay under 256 MiB of the result buffer) and the adjusted
 * parameters in batches of columns, each batch reading the window once more.  SMM_ERR_INVALID_ARG: NULL ctx or out, a bad window,
 * select outside [0, 2], n_groups < 0, group NULL with n_groups != 1, a group id outside [-1, n_groups), n_probs < 0, probs NULL with
 * n_probs > 0, a prob outside [0, 1] or NaN, adj_quantile without probs, tol outside (0, 1] or NaN, kernel not 0 or 1, a scale not
 * finite or not > 0, ridge negative or not finite; nothing is written then.
 *
 * Numerical contract (every operation rounded on its own, no fma; counts and integer weights 64-bit):
 *   pooled rows: smm_get_moment_stats' rows: the members in ascending local index, each in iteration order; m = count.  Row i has the
 *                parameters theta_ij (j < np) and the simulated moments s_ik (k < nm).
 *   scale      : sc_k = scale[k] when given, else smm_get_moment_stats' s_k (w_k if it is finite and not zero, else 1.0).
 *   discrepancy: x_ik = (s_ik - mom_k) / sc_k.
 *   distance   : d2_i = 0.0, d2_i = d2_i + x_ik * x_ik over k ascending.
 *   bandwidth  : delta2 = the chain-stats quantile tol of the pooled column d2 (numpy's _lerp; chunks and order as smm_get_group_stats).
 *   weight     : kernel 0: w_i = d2_i <= delta2 ? 1.0 : 0.0; kernel 1: w_i = d2_i < delta2 ? 1.0 - d2_i / delta2 : 0.0; r_i = sqrt(w_i).
 *   n_kept     : the rows with w_i > 0.
 *   sum_w, ess : sum_w = S(w_i), S the chunked pairwise sum of the pooled column (chunks of 8192 counted from the group's first row);
 *                sum_w2 = S(w_i * w_i); ess = (sum_w * sum_w) / sum_w2.
 *   joint columns: D = nm + np; column c < nm is x_.c, column nm + j is theta_.j.
 *   means      : mu_c = S(w_i * v_ic) / sum_w; x_mean the first nm of them, raw_mean the rest.
 *   e_ic       = r_i * (v_ic - mu_c) over all m rows (a row with w = 0 contributes zeros).
 *   pair sums  : C_ab = S(e_ia * e_ib): smm_get_chain_cov's pair sums over chunks of 8192, the chunks' sums added in order from 0.0 as
 *                smm_get_moment_stats adds them; mirrored entries hold the same value.
 *   factor     : A = C_xx (a, b < nm) with A_kk = C_kk + ridge * C_kk; its lower Cholesky factor in smm_get_moment_stats' order.
 *   beta       : column j = solve(L, b) of smm_get_moment_stats with b_k = C_{k, nm + j}; stored [nm][np].
 *   adj_mean_j = mu_{nm + j} - t, t = 0.0, t = t + mu_k * beta_kj over k ascending (the data sit at x = 0).
 *   adj_sd_j   = sqrt((C_{nm + j, nm + j} - u) / sum_w), u = 0.0, u = u + beta_kj * C_{k, nm + j} over k ascending; a negative radicand
 *                gives NaN as IEEE sqrt does.
 *   adjusted draw: for the rows with w_i > 0, theta*_ij = theta_ij - t, t = 0.0, t = t + x_ik * beta_kj over k ascending.
 *   n_outside_j: the kept rows with theta*_ij < lb_j or theta*_ij > ub_j (nothing is clamped).
 *   adj_quantile: integer weights, so that no sum depends on an order: q_i = (int64) ceil(w_i * 1048576.0), exact and at least 1 for a
 *                kept row; Q = the sum of them (below 2^51 with fewer than 2^31 rows, so (double) Q is exact); for prob p, target =
 *                max(1, (int64) ceil(p * (double) Q)); the quantile is the smallest v among the kept theta*_.j for which the q of the
 *                rows with theta* <= v add up to at least target: the inverted weighted CDF, without interpolation.  Doubles are
 *                ordered by smm_get_chain_stats' sort keys, the IEEE total order (-0.0 before +0.0), and the result is one of the
 *                kept theta*, never interpolated: a quantile that is a zero carries the sign of the row it is.
 *   status     : the first that applies: 1 m < 2; 2 a non-finite value among the selected parameters or moments (1, 2: everything but
 *                count and n_chains NaN, the integers 0); 3 kernel 1 with !(delta2 > 0), or n_kept < nm + 2; 4 a pivot of the factor
 *                of A is not > 0 (3, 4: bandwidth, n_kept, sum_w, ess, x_mean and raw_mean keep the values defined above, beta and
 *                adj_* are NaN, n_outside 0); 0 otherwise.  An empty window or a group without rows: status 1. */
typedef struct {             /* caller-allocated; any pointer may be NULL = not computed; G = n_groups                          */
    int64_t* count;          /* [G]              selected rows pooled in the group                                               */
    int32_t* n_chains;       /* [G]              member chains                                                                   */
    int32_t* status;         /* [G]              0 ok, 1 fewer than 2 rows, 2 non-finite value, 3 nothing to regress on, 4 not PD */
    int64_t* n_kept;         /* [G]              rows with weight > 0                                                            */
    double*  bandwidth;      /* [G]              delta2: the squared distance at which the weight reaches 0                      */
    double*  sum_w;          /* [G]                                                                                              */
    double*  ess;            /* [G]              sum_w^2 / sum of w^2 (Kish)                                                     */
    double*  x_mean;         /* [G][nm]          weighted mean discrepancy of the kept draws                                     */
    double*  raw_mean;       /* [G][np]          weighted parameter mean: the unadjusted (rejection) estimate                    */
    double*  beta;           /* [G][nm][np]      regression of the parameters on the discrepancy                                 */
    double*  adj_mean;       /* [G][np]          the intercept: E[theta | s = s_obs]                                             */
    double*  adj_sd;         /* [G][np]          weighted residual standard deviation                                            */
    double*  adj_quantile;   /* [n_probs][G][np] weighted quantiles of the adjusted draws                                        */
    int64_t* n_outside;      /* [G][np]          kept rows whose adjusted value leaves [lb, ub] (nothing is clamped)             */
} smm_adjustment_t;
int  smm_get_adjustment(void* ctx, int32_t t0, int32_t t1, int32_t select, const int32_t* group /* [N] or NULL */, int32_t n_groups,
                        double tol, int32_t kernel, const double* scale /* [nm] or NULL */, double ridge, const double* probs,
                        int32_t n_probs, smm_adjustment_t* out);

/* The target posterior from every temperature, computed on the device from the history it holds.  Chain c accepts with
 * exp(acc_tuner[c] (v_old - v_new)) (AlgoBGP.jl:344), so its state series samples the density proportional to exp(-acc_tuner[c] v(theta))
 * on the box.  Every scored row of chain c is importance-reweighted from the chain's own temperature to the target a* = targets[r] by
 * exp((acc_tuner[c] - a*) v); each chain is self-normalised, so the unknown normalisers drop out, and the chains of a group are combined
 * by their effective sample sizes.  The one statistical assumption: each chain's state series targets exp(-acc_tuner v); BGP's exchange
 * moves respect this only approximately.  select 2 (the state series through a(t)) is the selection the theory is about; 0 (all rows)
 * and 1 (the accepted rows) are offered as the other group readers offer them.  Window, groups and select are exactly those of
 * smm_get_moment_stats (a shard reports its own local chains; group NULL with n_groups == 1: every local chain in group 0); acc_tuner is
 * the chain's own, indexed by its global id.  Caller-allocated; any pointer may be NULL (not computed).  Read-only and ordered like
 * smm_get_chain_stats (it settles, flushes and synchronises, and changes no state, history or generator).  Device memory:
 * smm_get_chain_stats' scratch, grown where needed to 5 x N x maxiter x 8 bytes (per scored row its history row and chain, its value, its
 * weight, its integer weight, and one column of parameters) plus (np + nm + 3) x 8192 x 8 bytes (the columns of one chunk) plus at most
 * 256 MiB (further chunks and parameter columns, no more than the context's capacity can fill); the rows are
 * taken in batches of chunks (whose np^2 pair sums per chunk stay under 256 MiB of the result buffer) and the select's parameters in
 * batches of columns; the targets run one after another over the same packed columns.  SMM_ERR_INVALID_ARG: NULL ctx or out, a bad
 * window, select outside [0, 2], n_groups < 0, group NULL with n_groups != 1, a group id outside [-1, n_groups), n_targets outside
 * [1, 64], targets NULL, a target that is not finite or < 0, n_probs < 0, probs NULL with n_probs > 0, a prob outside [0, 1] or NaN,
 * quantile without probs; nothing is written then.  R = n_targets, G = n_groups, N the local chains.
 *
 * Numerical contract (every operation rounded on its own, no fma outside smm_exp / smm_log; counts and integer weights 64-bit):
 *   scored row : a selected row whose value has |v| <= DBL_MAX; a select-2 row with no a(t) is not scored.  count includes the unscored
 *                rows, nothing else does.
 *   per member chain c and target r, over the chain's scored rows in iteration order (n_c of them) as one contiguous column:
 *     d = acc_tuner[c] - targets[r]; lw_i = d * v_i; L = max_i lw_i; w_i = smm_exp(lw_i - L), 0.0 where lw_i - L is -inf (smm_exp(0.0) is
 *     exactly 1.0: k = 0, r = 0, p = 0, ldexp(1.0 + 0.0, 0); the row that attains L has w = 1).
 *     sw = S_c(w_i), sw2 = S_c(w_i * w_i), S_c the chain-stats pairwise sum (chunks of 8192 from the chain's first scored row).
 *     chain_ess = (sw * sw) / sw2; chain_logz = L + smm_log(sw / (double) n_c), the log normaliser ratio log Z(a*) / Z(a_c);
 *     f_c = sw / sw2.  n_c == 0, or a chain in no group: chain_ess 0, chain_logz NaN, and the chain contributes no row.
 *   row weight : u_i = w_i * f_c: every chain is self-normalised and enters with its own effective sample size (the u of chain c add up
 *                to chain_ess up to rounding).
 *   group      : over the members' scored rows in pooled order (members in ascending local index, each in iteration order, packed);
 *                S the chunked pairwise sum of smm_get_group_stats, chunks of 8192 counted from the group's first scored row.
 *     sum_u = S(u_i); ess = (sum_u * sum_u) / S(u_i * u_i).
 *     mean_j = S(u_i * theta_ij) / sum_u; value_mean and m_mean_k the same with v_i and s_ik in place of theta_ij.
 *     e_ij = sqrt(u_i) * (theta_ij - mean_j); cov_jk = C_jk / sum_u, C smm_get_adjustment's pair sums (smm_get_chain_cov's per chunk,
 *     the chunks' sums added in order from 0.0): the weighted population form, without a Bessel factor; mirrored entries hold the same
 *     value.
 *     n_kept: the rows with u_i > 0.
 *     quantile: F = the largest f_c among the members with n_c > 0; q_i = (int64) ceil((u_i / F) * 1048576.0), at least 1 for a kept
 *     row and at most 2^20 (u_i <= f_c <= F); Q = the sum of them; from there smm_get_adjustment's rule: target = max(1, (int64)
 *     ceil(p * (double) Q)); the quantile is the smallest theta_.j among the kept rows for which the q of the rows with theta <= it add
 *     up to at least target: the inverted weighted CDF over the IEEE total order (-0.0 before +0.0), one of the rows' own doubles.
 *   status per (r, g), the first that applies: 1 fewer than 2 scored rows; 2 a non-finite parameter in a scored row; 3 a member's L, or
 *                sum_u, is not finite (d * v overflowed); 0 otherwise.  For 1 to 3 every double of (r, g) is NaN and n_kept 0; the
 *                per-chain outputs keep the values defined above.  A NaN simulated moment in a scored row propagates into that moment's
 *                mean only. */
typedef struct {             /* caller-allocated; any pointer may be NULL = not computed                                        */
    int64_t* count;          /* [G]                   rows selected                                                             */
    int64_t* n_scored;       /* [G]                   rows that carry a weight                                                  */
    int32_t* n_chains;       /* [G]                   member chains                                                             */
    int32_t* status;         /* [R][G]                0 ok, 1 fewer than 2 scored rows, 2 non-finite parameter, 3 overflow      */
    int32_t* chain_n;        /* [N]                   a chain's scored rows; 0 for a chain in no group                          */
    double*  chain_ess;      /* [R][N]                per-chain effective sample size                                           */
    double*  chain_logz;     /* [R][N]                per-chain log normaliser ratio log Z(a*) / Z(a_c)                         */
    int64_t* n_kept;         /* [R][G]                rows with u > 0                                                           */
    double*  sum_u;          /* [R][G]                sum of the row weights                                                    */
    double*  ess;            /* [R][G]                effective sample size of the group (Kish)                                 */
    double*  mean;           /* [R][G][np]            weighted parameter mean                                                   */
    double*  cov;            /* [R][G][np][np]        weighted population covariance, both triangles                            */
    double*  value_mean;     /* [R][G]                weighted mean of the objective value                                      */
    double*  m_mean;         /* [R][G][nm]            weighted mean of each simulated moment                                    */
    double*  quantile;       /* [n_probs][R][G][np]   weighted quantiles of the parameters                                      */
} smm_reweighted_t;
int  smm_get_reweighted(void* ctx, int32_t t0, int32_t t1, int32_t select, const int32_t* group /* [N] or NULL */, int32_t n_groups,
                        const double* targets, int32_t n_targets, const double* probs, int32_t n_probs, smm_reweighted_t* out);

/* The objective and the simulated moments binned along parameters, computed on the device from the history it holds: for each group of
 * chains and each parameter, over smm_get_histogram's bins of that parameter, the profile of the objective (the smallest value among the
 * rows of the bin and the row that attains it, with its full parameter vector: the lower envelope a slice plot draws, over everywhere the
 * chains went), the mean value and the mean of every simulated moment; and for each pair of parameters the same minima and means over
 * smm_get_histogram's 2-D cells (the objective surface for a contour plot).  No further evaluation of the objective.  The window, the
 * groups and select (0 all rows, 1 accepted rows, 2 the state series through a(t)) are exactly those of smm_get_histogram; a shard
 * reports its own local chains.  For select 2, row a(t) supplies the parameters, the value and the moments alike, as in
 * smm_get_moment_stats; min_iter is the window iteration t of the pooled row, not a(t).  Caller-allocated; any pointer may be NULL (not
 * computed).  Read-only and ordered like smm_get_chain_stats (it settles, flushes and synchronises, and changes no state, history or
 * generator).  Device memory: the reducers' scratch and result buffer, in batches of groups and of axes (an axis: a parameter with
 * nseg = bins segments, or a pair with nseg = bins2 bins2).  A batch of mb member chains and an axes takes mb n 12 + an mb (8 n + 4 nseg)
 * bytes of the scratch (n = t1 - t0: each pooled row's source row and value; per axis its segment, its slot in the compacted list and
 * the per-member segment counts) and, for its gn groups, gn an nseg (60 + 8 np + 8 nm) bytes of results plus 12 + 8 (1 + nm) bytes per
 * chunk of 8192 scored rows, N x (12 + 20 np) bytes of per-chain ranges and lists and smm_get_histogram's edge tables.  Groups are taken
 * while one axis of them fits the scratch (256 MiB unless the whole history's columns are smaller) and 256 MiB of results, then as many
 * axes as fit; the scratch is grown where needed to one axis of the largest group.  SMM_ERR_INVALID_ARG: NULL ctx or out, a bad window,
 * select outside [0, 2], n_groups < 0, group NULL with n_groups != 1, a group id outside [-1, n_groups), bins outside [1, 4096], a range
 * row not finite or with lo > hi, n_pairs outside [0, np np], pairs NULL with n_pairs > 0, a pair entry outside [0, np), bins2 outside
 * [1, 256] with n_pairs > 0, a 2-D output requested with n_pairs == 0, a group whose pooled rows would number more than 2^31 - 1;
 * nothing is written then.
 *
 * Numerical contract (every operation rounded on its own, no fma; ranks and counts 64-bit):
 *   axes       : smm_get_histogram's 1-D and 2-D rules bit for bit: the outer edges, edges, edges2, status, the bin of a row and the
 *                cell of a row.  A row that numpy drops is dropped here (outside [lo, hi], NaN, or a 2-D axis out of range).  An axis
 *                with status 1-3 (a pair with status 1 or 2 on either axis) has n = 0 and every double NaN.  n and n2 equal hist and
 *                hist2 of smm_get_histogram called with the same arguments.
 *   segment    : the rows of a bin or cell in pooled order: the members in ascending local index, each in iteration order.  A row is
 *                scored when |value| <= DBL_MAX; failed evaluations and NaN values count in n but in nothing else.
 *   v_mean, v_mean2, m_mean[..][k] : the chain-stats mean of the segment's m = n_scored scored rows as a contiguous column: S / m,
 *                S = S + pw(x, c, min(8192, m - c)) for c = 0, 8192, .. counted from the segment's first scored row: np.mean(col[idx]).
 *                m == 0: NaN.  A moment that is NaN in a scored row propagates into that moment's mean only.
 *   v_min      : the first minimum of the scored column in pooled order; ties go to the earliest row, -0 and +0 compare equal (the
 *                earlier one is reported, with its sign).  min_chain: that row's 1-based GLOBAL chain id, min_iter: its 1-based
 *                iteration t + 1 (smm_get_draws' chain and iter), theta_at_min: its np parameters bit for bit.  m == 0: v_min NaN,
 *                min_chain and min_iter 0, theta_at_min NaN. */
typedef struct {            /* caller-allocated; any pointer may be NULL = not computed; G = n_groups, B = bins, B2 = bins2 */
    int64_t* count;         /* [G]                      rows selected for the group                                  */
    int32_t* status;        /* [G][np]                  smm_get_histogram's status of the axis                        */
    double*  edges;         /* [G][np][B + 1]                                                                          */
    int64_t* n;             /* [G][np][B]               rows in the bin (== smm_get_histogram's hist)                  */
    int64_t* n_scored;      /* [G][np][B]               of them, rows with a finite value                              */
    double*  v_min;         /* [G][np][B]               profile: smallest value among the scored rows                  */
    int32_t* min_chain;     /* [G][np][B]               the row that attains it: chain and iteration, numbered as      */
    int32_t* min_iter;      /* [G][np][B]               smm_get_draws numbers a row's chain and iteration; 0 = none    */
    double*  theta_at_min;  /* [G][np][B][np]           that row's parameters (the profile path)                       */
    double*  v_mean;        /* [G][np][B]               mean value over the scored rows                                */
    double*  m_mean;        /* [G][np][B][nm]           mean simulated moment over the scored rows                     */
    double*  edges2;        /* [G][np][B2 + 1]                                                                         */
    int64_t* n2;            /* [G][n_pairs][B2][B2]     (== smm_get_histogram's hist2)                                 */
    int64_t* n_scored2;     /* [G][n_pairs][B2][B2]                                                                    */
    double*  v_min2;        /* [G][n_pairs][B2][B2]                                                                    */
    int32_t* min_chain2;    /* [G][n_pairs][B2][B2]                                                                    */
    int32_t* min_iter2;     /* [G][n_pairs][B2][B2]                                                                    */
    double*  v_mean2;       /* [G][n_pairs][B2][B2]                                                                    */
} smm_profile_t;
int  smm_get_profile(void* ctx, int32_t t0, int32_t t1, int32_t select, const int32_t* group /* [N] or NULL */, int32_t n_groups,
                     int32_t bins, const double* range /* [np][2] or NULL */, const int32_t* pairs /* [n_pairs][2] */,
                     int32_t n_pairs, int32_t bins2, smm_profile_t* out);

/* Highest-density intervals, half-sample modes and Gaussian kernel densities of the draws of groups of chains, computed on the device from
 * the history it holds, over the 0-based iterations [t0, t1): for each group and parameter the shortest interval holding a given mass of
 * the pooled draws (ArviZ's hdi of a unimodal sample; smm_get_chain_stats' and every quantile's intervals are equal-tailed), the
 * half-sample mode (Bickel & Fruehwirth 2006: the marginal mode, which best — the argmin of the objective — is not), and the kernel
 * density on a grid of n_grid points with its bandwidth and its highest grid point.  Groups, select (0 all rows, 1 accepted rows, 2 the
 * state series through a(t)), the window and the pooled column x of (group g, parameter k) are exactly smm_get_histogram's: the members
 * in ascending local index, each in iteration order; per-chain results: group = 0 .. N-1; group NULL with n_groups == 1: every local
 * chain in group 0; a shard reports its own local chains.  Caller-allocated; any pointer may be NULL (not computed).  Read-only and
 * ordered like smm_get_chain_stats (it settles, flushes and synchronises, and changes no state, history or generator).  Device memory:
 * the reducers' scratch and result buffer.  A parameter takes 16 bytes per pooled row of the scratch (the packed column and its sorted
 * keys; 32 and the digit tables of smm_get_rank_diag's sort where a column has 8193 rows or more) and goes with as many other
 * parameters as fit (the scratch is grown where needed to one parameter); [G][np] and [n_mass][G][np] results stay on the device for the
 * call, the curves are produced and copied out in batches of groups that fit 256 MiB (at least one group; a group takes n_grid x 8 x
 * (2 + its chunks of 8192 rows) bytes per parameter of the batch).  SMM_ERR_INVALID_ARG: NULL ctx or out, a bad window, select outside
 * [0, 2], n_groups < 0, group NULL with n_groups != 1, a group id outside [-1, n_groups), n_mass < 0, mass NULL with n_mass > 0, a mass
 * outside (0, 1] or NaN, hdi_lo or hdi_hi requested with n_mass == 0, n_grid neither 0 nor in [2, 4096], grid, density or kde_mode
 * requested with n_grid == 0, a range row not finite or with lo > hi, a bw entry not finite or not > 0, a group whose pooled rows
 * would number more than 2^31 - 1; nothing is written then.
 *
 * Numerical contract (every operation rounded on its own, no fma outside smm_exp; counts and indexes 64-bit).  m = count; s = x sorted
 * by the IEEE total order (-0 before +0); S(.) the chain-stats sum (pw over chunks of 8192 from the group's first draw), mean, quantile
 * the chain-stats ones on the pooled column, var smm_get_trace's (ddof 1):
 *   status     : 1: a NaN or +-inf in the column: every double output of (g, k) NaN, kde_status 1, count still reported.
 *                2: m == 0: every double output NaN, kde_status 1.
 *   HDI of mass p : k = min((int64)floor(p * (double)m), m - 1) (one rounded product); w_i = s[i + k] - s[i], i in [0, m - k);
 *                i* the first minimum of w (np.argmin); hdi_lo = s[i*], hdi_hi = s[i* + k].
 *   mode       : lo = 0, n = m; while n > 3: h = (n + 1) / 2, w_i = s[lo + i + h - 1] - s[lo + i] for i in [0, n - h + 1), lo += the first
 *                argmin, n = h.  n == 1: s[lo]; n == 2: (s[lo] + s[lo + 1]) / 2; n == 3: a = s[lo + 1] - s[lo], b = s[lo + 2] - s[lo + 1]:
 *                a < b: (s[lo] + s[lo + 1]) / 2; b < a: (s[lo + 1] + s[lo + 2]) / 2; else s[lo + 1].
 *   bandwidth  : h = bw[k] where given; else R's bw.nrd0: sd = sqrt(var(x)) (NaN for m < 2), a = (quantile(0.75) - quantile(0.25)) / 1.34,
 *                l = sd < a ? sd : a; l == 0: l = sd; still 0: l = |x[0]| (the first pooled draw); still 0: l = 1.0;
 *                h = (0.9 * l) * smm_exp(-0.2 * smm_log((double)m)).  h not finite or not > 0: kde_status 1, bw as computed, grid,
 *                density and kde_mode NaN.
 *   grid       : (lo, hi) = range[k] where given, else lo = s[0] - 3.0 * h, hi = s[m - 1] + 3.0 * h; hi - lo not finite: kde_status 2,
 *                grid, density and kde_mode NaN.  Else smm_get_histogram's linspace with b = n_grid - 1: delta = hi - lo,
 *                step = delta / b; step != 0: g[j] = j step + lo, else g[j] = (j / b) delta + lo; g[b] = hi.
 *   density    : rh = 1.0 / h; u = (g[j] - x[i]) * rh; e_ij = smm_exp(-0.5 * (u * u)); D_j = S(e_.j) over i in pooled order;
 *                density[j] = (D_j / (double)m) / (h * 2.5066282746310002).
 *   kde_mode   : g[first argmax of density] (np.argmax: the first NaN where there is one). */
typedef struct {            /* caller-allocated; any pointer may be NULL = not computed */
    int64_t* count;         /* [G]              rows selected for the group                                   */
    int32_t* status;        /* [G][np]          0 ok, 1 a non-finite draw in the column, 2 empty column       */
    double*  hdi_lo;        /* [n_mass][G][np]                                                                */
    double*  hdi_hi;        /* [n_mass][G][np]                                                                */
    double*  mode;          /* [G][np]          half-sample mode                                              */
    double*  bw;            /* [G][np]          bandwidth used                                                */
    int32_t* kde_status;    /* [G][np]          0 ok, 1 no usable bandwidth, 2 grid width not finite          */
    double*  grid;          /* [G][np][n_grid]                                                                */
    double*  density;       /* [G][np][n_grid]                                                                */
    double*  kde_mode;      /* [G][np]          grid point of the first maximum of density                    */
} smm_density_t;
int  smm_get_density(void* ctx, int32_t t0, int32_t t1, int32_t select, const int32_t* group /* [N] or NULL */, int32_t n_groups,
                     const double* mass, int32_t n_mass, int32_t n_grid, const double* range /* [np][2] or NULL */,
                     const double* bw /* [np] or NULL */, smm_density_t* out);

/* The posterior of user functions of each draw — Stan's "generated quantities": an elasticity, a ratio of two parameters, a welfare
 * number, an untargeted statistic built from the simulated moments, each with its interval, computed on the device from the history it
 * holds without downloading it (the delta method on smm_get_moment_stats' Jacobian is a linearisation that the draws make unnecessary).
 *
 * smm_register_user_transform(source, n_out, &id): the source is HIP/C++ text defining ONE function with this exact signature
 * (SMM_USER_TRANSFORM expands to the required linkage):
 *
 *   SMM_USER_TRANSFORM(const double* theta, int np, const double* sim_moments, int nm, double value,
 *                      const double* mom, const double* w, const double* udata, int n_udata,
 *                      const double* tdata, int n_tdata, double* out, int n_out)
 *
 * It must be a deterministic function of its arguments: theta, sim_moments and value of one history row exactly as smm_get_history
 * returns them, the context's mom, w and udata = obj_params, and tdata, a vector given per call (the policy values of a counterfactual,
 * say).  out[0..n_out) holds NaN on entry; an output left unwritten stays NaN.  It may call smm_exp(double) and smm_log(double), the
 * contract's functions (above), at global scope.  1 <= n_out <= 64.  Compiled at registration with the user objectives' options
 * (hiprtc, --offload-arch=gfx950 -O3 -ffp-contract=off -fno-fast-math -std=c++17), which make + - * /, sqrt, smm_exp and smm_log
 * reproducible bit for bit.  The handles are a range of their own (from 0), not the objectives'.  SMM_ERR_INVALID_ARG: a NULL argument,
 * n_out outside [1, 64], or a source that does not compile (the compiler's log in smm_last_error(NULL)); SMM_ERR_HIP: no hiprtc.
 *
 * smm_get_derived(ctx, id, ...), with Q = the transform's n_out: group g's pooled rows are those of smm_get_histogram — the members in
 * ascending local index, each in iteration order; select 0 all rows of [t0, t1), 1 the rows with accepted != 0, 2 the state series, row
 * a(t) looking back before t0; groups, group NULL with n_groups == 1 and shards as in smm_get_group_stats (a shard reports its own
 * local chains).  The derived column q of a group is y_q[i] = output q of the function on pooled row i; for a select 2 row with no a(t)
 * the function is not called and every output of the row is NaN.  Caller-allocated; any pointer may be NULL (not computed).  Read-only
 * and ordered like smm_get_chain_stats (it settles, flushes and synchronises, and changes no state, history or generator).  Device
 * memory: the reducers' scratch and result buffer.  An output takes 8 bytes per pooled row of the scratch and goes with as many other
 * outputs as fit beside the row indexes of one chunk of 8192 rows (the scratch is grown, up to 256 MiB, to every output and row index
 * of the context's capacity, and beyond that where needed to one output); the rows go through the function in batches of chunks,
 * every batch of outputs runs the function on every row again, and so does cov, which takes one chunk of every output at a time or
 * more.  SMM_ERR_INVALID_ARG: NULL ctx or out, an unknown transform_id, a bad window,
 * select outside [0, 2], n_groups < 0, group NULL with n_groups != 1, a group id outside [-1, n_groups), n_probs < 0, probs NULL with
 * n_probs > 0, a prob outside [0, 1], quantile requested without probs, n_tdata < 0 or > 4096, tdata NULL with n_tdata > 0; nothing is
 * written then.
 *
 * Numerical contract: mean, median, quantile and cov are smm_get_group_stats' on the columns y_q in place of the parameter columns
 * (the chunked pairwise sum over chunks of 8192 rows from the group's first row, numpy's _lerp order statistics on the IEEE total
 * order, cov = S(d_j d_k) / (m - 1) with d = y - mean); NaN propagates as it does there; m == 0: NaN everywhere; m < 2: cov NaN.
 * Values that are not finite are not dropped: n_nonfinite counts the rows of each column that are NaN or +-inf. */
typedef struct {            /* caller-allocated; any pointer may be NULL = not computed */
    int64_t* count;         /* [G]        selected rows pooled in the group                   */
    int32_t* n_chains;      /* [G]                                                            */
    int64_t* n_nonfinite;   /* [G][Q]     rows whose output q is NaN or +-inf                 */
    double*  mean;          /* [G][Q]                                                         */
    double*  median;        /* [G][Q]                                                         */
    double*  quantile;      /* [n_probs][G][Q]                                                */
    double*  cov;           /* [G][Q][Q]  both triangles                                      */
} smm_derived_t;
int  smm_register_user_transform(const char* hip_source, int32_t n_out, int32_t* transform_id_out);
int  smm_get_derived(void* ctx, int32_t transform_id, int32_t t0, int32_t t1, int32_t select, const int32_t* group /* [N] or NULL */,
                     int32_t n_groups, const double* tdata, int32_t n_tdata, const double* probs, int32_t n_probs, smm_derived_t* out);

/* Covariances of the chains' draws and the proposal factor between steps — adaptive Metropolis (Haario et al.) on top of chol_L: a
 * pilot run, then each chain's proposal shaped by the covariance of its own draws, without leaving the device.
 *
 * smm_get_chain_cov: the covariance of every LOCAL chain's selected draws over the 0-based iterations [t0, t1), selected exactly as
 * smm_get_chain_stats selects them (accepted_only != 0: params(c), AlgoBGP.jl:120-131).  unit_space != 0: the draws mapped to [0, 1]
 * first, u = (x - lb) / (ub - lb) (mapto_01, mprob.jl:248, the kernels' own arithmetic) — the space the proposal lives in; 0: the
 * parameters themselves.  count [N], mean [np][N], cov [np][np][N] (both triangles); any output may be NULL.  Works on any context;
 * read-only: it settles, flushes and synchronises like smm_get_chain_stats and changes no state, history or generator.  It uses
 * smm_get_chain_stats' scratch, grown where needed to one chain's maxiter x (8 np + 4) bytes, plus ((np + 1) np + 1) N x 8 + 16 N bytes
 * of results.  SMM_ERR_INVALID_ARG: NULL ctx, a bad window (0 <= t0 <= t1 <= completed iterations).
 *
 * Numerical contract (every operation rounded on its own, no fma).  u = the compacted column (mapped when unit_space != 0), m = count:
 *   mean_j  = the chain-stats mean of column j (the pw sum in chunks of 8192, divided by m)
 *   d_j[i]  = u_j[i] - mean_j
 *   cov_jk  = S(d_j[i] * d_k[i]) / (m - 1), S = the chain-stats chunked pairwise sum over i: bit for bit np.sum(dj * dk) / (m - 1) on
 *             contiguous float64 columns; cov_kj is the same value.  m < 2: NaN.  A NaN among the draws propagates.
 *   tau     = (((0 + C_00) + C_11) + ...) / np
 *   chol    : for k = 0..np-1, j = 0..k: s = A_kj; s = s - L_ki * L_ji for i = 0..j-1 in that order; j == k: L_kk = sqrt(s), failing
 *             when !(s > 0); otherwise L_kj = s / L_jj.
 *
 * The three proposal calls need a context created with chol_L (otherwise SMM_ERR_INVALID_ARG).  The factor(s) are [np][np] for a shared
 * factor, [N][np][np] for per-chain factors (the LOCAL chains, global rows chain_offset .. chain_offset + N - 1: a shard reads and writes
 * only its own chains' rows, the only rows its kernels read), row-major.  A context's forms do not change (smm_describe is the same):
 * installing a factor overwrites the device buffer the chain kernels read — the per-iteration ones and the persistent tile form, which
 * reads the factor at every iteration — on the context's stream.
 *
 * smm_get_proposal: the installed factor(s), zeros above the diagonal.
 * smm_set_proposal: install factor(s) between steps (the matrix form of set_sigma!, AlgoBGP.jl:218-219); entries above the diagonal are
 *   ignored.  SMM_ERR_INVALID_ARG (nothing installed): a non-finite entry on or below the diagonal, a diagonal entry not > 0.  On a
 *   sharded context with a shared factor every rank must install the same factor.
 * smm_adapt_proposal: per-chain contexts only (chol_per_chain = 1; a shared factor has no single history to take it from): for every
 *   local chain C = smm_get_chain_cov(..., unit_space = 1) of the window, A = C / tau (normalize != 0) or A = C, A_kk = A_kk + ridge,
 *   L = chol(A), installed where the chain's status is 0.  status [N] (may be NULL): 0 installed; 1 fewer than min_draws selected
 *   draws; 2 a non-finite entry in C; 3 not positive definite (a pivot !(s > 0)).  A chain with a non-zero status keeps its factor.
 *   SMM_ERR_INVALID_ARG: a bad window, min_draws < 2, ridge < 0 or not finite.
 *
 * Ordering and failures: smm_set_proposal and smm_adapt_proposal settle, flush and synchronise before they act, so an smm_bgp_step_async
 * in flight is ordered before them.  A hard error standing on the context (AlgoBGP.jl:341,409) — reported before or not — is returned
 * by them and nothing is installed; it counts as told, so the smm_set_state that recovers from it goes through at its first call. */
int  smm_get_chain_cov(void* ctx, int32_t t0, int32_t t1, int32_t accepted_only, int32_t unit_space,
                       int32_t* count /* [N] */, double* mean /* [np][N] */, double* cov /* [np][np][N] */);
int  smm_get_proposal(void* ctx, double* L);
int  smm_set_proposal(void* ctx, const double* L);
int  smm_adapt_proposal(void* ctx, int32_t t0, int32_t t1, int32_t accepted_only, int32_t min_draws,
                        int32_t normalize, double ridge, int32_t* status /* [N] */);

int  smm_get_state(void* ctx, smm_state_t* out);
/* smm_set_state is also the recovery from a hard error (AlgoBGP.jl:341,409): the context steps again from the uploaded state.  A failure that
 * no entry point has handed to the caller yet — raised on the device by asynchronous steps nobody synchronised; the state readers do not
 * raise — is returned by THIS call, once, and nothing is uploaded: an error never disappears into a recovery the caller did not know it was
 * making.  The next smm_set_state goes through. */
int  smm_set_state(void* ctx, const smm_state_t* in, const smm_history_t* hist /* iterations 0..iter-1 */);

/* The starting population: every chain from its own point, installed on the device as the chain's COMPLETED iteration 1.  The reference
 * starts all chains at MProb.initial_value (iteration 1 of every chain proposes it, AlgoBGP.jl:426-427); the search over a space-filling set
 * of points in the box is the role of its sobolsearch.jl.  Both calls are valid only on a context that has completed no iteration (iter == 0;
 * later: SMM_ERR_STATE); after success iter == 1 and stepping continues at iteration 2 in whatever form the context has chosen.
 *
 * Install contract: for every chain the device holds exactly what a fresh context would hold after smm_bgp_step(ctx, 1) if that chain's
 * initial_value were its start (as smm_get_history / smm_get_state report it): history row 0 — params = the start, value and sim_moments
 * = its evaluation, status = 1 and prob = 1 (doAcceptReject! at iteration 1 accepts whatever the objective returned, AlgoBGP.jl:326-332),
 * accepted = 1, curr_val = best_val = value, best_id = 1, exchanged = 0 —, the last-accepted record (the same evaluation), and the chain
 * state: accept_rate = 1, n_noex = n_acc_noex = 1, best = (value, 1), sigma untouched.  The context's bookkeeping is what smm_set_state
 * leaves for iter == 1 (no exchange pending; a NaN value among the installed ones is remembered as there).  No exchange belongs to
 * iteration 1 (exchange_from_iter >= 2).
 *
 * smm_set_population: the caller supplies the starts, [np][N] for the LOCAL chains; each is evaluated once (evaluated = N) and installed
 *   whatever its evaluation says; pick = 0 for every chain.  A start outside [lb, ub], or a NaN: SMM_ERR_INVALID_ARG with the (1-based global)
 *   chain and the parameter in the message, nothing installed.  Scratch: N x ((np + nm + 1) x 8 + 4) bytes, one batch.
 * smm_scatter_population: for each chain M >= 1 candidates are generated, evaluated and reduced on the device; initial_value is evaluated once
 *   (evaluated = N x M + 1).
 *   Candidates (numerical contract; every operation rounded on its own, no fma).  Candidate m of global chain g = chain_offset + i,
 *   parameter k: the Philox4x32-10 block x = philox(counter {g, m, k >> 1, 0}, key (lo32(seed), hi32(seed) ^ (7 * 0x9E3779B9))) (stream 7 of the
 *   library's generator, smm.jl_amd/csrc/smm_rng.hpp: STREAM_POP); u = (x0:x1 >> 11) * 2^-53 for even k, (x2:x3 >> 11) * 2^-53 for odd k; with
 *   c = (init_k - lb_k) / (ub_k - lb_k) (mapto_01, mprob.jl:248) and 0 < spread <= 1: lo = max(0, c - spread / 2), hi = min(1, c + spread / 2),
 *   x01 = lo + u * (hi - lo), theta_k = x01 * (ub_k - lb_k) + lb_k (mapto_ab, mprob.jl:271, as the proposal computes it).  spread == 1 around a
 *   centred init covers the whole box.  The key is the GLOBAL chain id: a shard generates exactly the candidates the single-shard run
 *   generates for its chains.
 *   Selection: a candidate is valid when its status >= 1 and its value is finite and >= 0; invalid ones are skipped (in a search they are not
 *   a hard error).  The valid candidate with the lowest value wins, ties to the lowest m.  With keep_init != 0 initial_value competes as
 *   candidate -1 and wins ties; when no candidate is valid it is the start whatever keep_init says (pick = -1).  The winner's evaluation is
 *   installed as computed (value, sim_moments); it is not evaluated a second time.  A user objective with a stream draws from opts.seed, as in
 *   BGP steps (common random numbers).
 *   SMM_ERR_INVALID_ARG: M < 1, spread outside (0, 1] or NaN, (int64)M * N_global >= 2^31.
 *   Scratch: chains go in batches whose candidates and results — M x ((np + nm + 1) x 8 + 4) bytes per chain — stay under 64 MiB (at least one
 *   chain per batch); freed before the call returns.
 * Both: out may be NULL, and so may any pointer in it.  Ordered on smm_stream behind everything enqueued before (a persistent launch is
 * settled first, as smm_set_state does) and synchronised before they return.  A hard error nobody has been told of yet is returned once, and
 * nothing is installed.  SMM_ERR_MAXITER on a context without room for one iteration.  smm_describe then ends in "population=set" or
 * "population=scatter pop_M=.. pop_spread=..". */
typedef struct {            /* caller-allocated, any pointer may be NULL */
    double*  start;         /* [np][N] the point each chain starts from            */
    double*  value;         /* [N]     its objective value                          */
    int32_t* pick;          /* [N]     index of the chosen candidate, -1 = initial_value */
    int64_t  evaluated;     /* out: objective evaluations performed                 */
} smm_population_t;
int  smm_set_population(void* ctx, const double* starts /* [np][N], host */, smm_population_t* out);
int  smm_scatter_population(void* ctx, int32_t M, double spread, int32_t keep_init, smm_population_t* out);

/* The estimate: K cyclic coordinate searches on grids, advancing together on the device (the reference's optSlices, slices.jl:114-242, from
 * many starts: every chain's or every temperature group's best point, say).  Valid on any context at any iteration; it never changes the
 * chains, the history, the generator's position or which kernel form the next step takes.  A stream objective draws from opts.seed, as
 * smm_eval_batch does (common random numbers).  Ordered on smm_stream behind everything enqueued before (a persistent launch is settled
 * first) and synchronised before it returns; a hard error nobody has been told of yet is returned once, and nothing runs.
 *
 * Numerical contract (every operation rounded on its own, no fma), per search s, independent of every other search; G = npoints:
 *   Ranges: [lo_k, hi_k] start at [lb_k, ub_k]; bestp = the start, which must lie inside and must not be NaN (else SMM_ERR_INVALID_ARG with
 *   the 1-based search and parameter in the message; nothing runs).
 *   Grid of step (cycle, k) — numpy's linspace(lo_k, hi_k, G): with d = hi - lo and step = d / (G - 1), x_g = g * step + lo for g < G - 1 and
 *   x_(G-1) = hi; if step == 0, x_g = (g / (G - 1)) * d + lo.  Candidate g is bestp with coordinate k replaced by x_g.
 *   Select: the candidate with the smallest FINITE value wins — strict <, the lowest g wins ties, the status is not consulted (slices.jl:181).
 *   The winner becomes bestp, its value and moments the search's, as evaluated (never evaluated again) — even when it is worse than the
 *   previous value: the reference's behaviour.  With no finite value bestp stays.  dvec_k = old_k - new_k.
 *   End of cycle: if update is not NaN, for every k: r = (hi - lo) / 2, lo = max(bestp_k - update * r, lo), hi = min(bestp_k + update * r, hi)
 *   (both from the old lo and hi).  delta = sqrt(sum_k dvec_k^2): squares rounded, added left to right from k = 0, correctly rounded
 *   square root.  The search stops converged when delta <= tol, unconverged after max_cycles cycles; a search that stopped costs nothing more.
 *   evaluated: the sum of G over every step of every search still running.
 * It differs from the reference only where that is undefined: a cap on the cycles, and a result (+inf, NaN moments) before the first finite value.
 *   SMM_ERR_INVALID_ARG: K < 1, npoints < 2, (int64)K * npoints >= 2^31, tol negative or NaN, update not NaN and <= 0, max_cycles < 1, starts NULL.
 *   Scratch: values, moments and status of a step take G x ((nm + 1) x 8 + 4) bytes per search (a user objective's candidates G x np x 8 more;
 *   the built-in objectives' candidates are never written: their evaluation kernel builds each from bestp and the one replaced coordinate);
 *   the running searches go in batches under 64 MiB (at least one search per batch); freed before the call returns.  The host reads 4
 *   bytes per cycle — the number of searches that go on. */
typedef struct {             /* caller-allocated; any pointer may be NULL = not returned */
    double*  best;           /* [np][K]  the point each search ended at                      */
    double*  value;          /* [K]      objective there; +inf while no finite grid value was ever seen */
    double*  sim_moments;    /* [nm][K]  simulated moments there; NaN in that case           */
    double*  lo;             /* [np][K]  final search ranges                                 */
    double*  hi;             /* [np][K]                                                      */
    double*  delta;          /* [K]      norm of the last cycle's moves                      */
    double*  cycle_value;    /* [max_cycles][K] value after each cycle; NaN past a search's last cycle */
    int32_t* cycles;         /* [K]      cycles run                                          */
    int32_t* converged;      /* [K]      1: delta <= tol; 0: stopped by max_cycles           */
    int64_t  evaluated;      /* out: objective evaluations performed                         */
} smm_opt_slices_t;
int  smm_opt_slices(void* ctx, const double* starts /* [np][K], host */, int32_t K, int32_t npoints,
                    double tol, double update /* NaN = ranges never shrink */, int32_t max_cycles, smm_opt_slices_t* out);

/* The estimate, second optimiser: K Nelder–Mead (simplex) searches inside the box [lb, ub], advancing together on the device — for curved or
 * rotated valleys, which a coordinate search cannot follow.  Valid on any context at any iteration; it never changes the chains, the history,
 * the generator's position or which kernel form the next step takes.  A stream objective draws from opts.seed, as smm_eval_batch does.
 * Ordered on smm_stream behind everything enqueued before (a persistent launch is settled first) and synchronised before it returns; a
 * hard error nobody has been told of yet is returned once, and nothing runs.
 *
 * Numerical contract: scipy's _minimize_neldermead with bounds and a given initial_simplex, made exact — every operation rounded on its own,
 * no fma; per search, independent of every other search.  N = np, vertices sim[0..N], values fsim[0..N].
 *   Coefficients, computed once in double on the host as Python computes them: rho = 1; chi = 2, psi = 0.5, sigma = 0.5, or with adaptive != 0
 *   chi = 1 + 2/N, psi = 0.75 - 1/(2N), sigma = 1 - 1/N.  The products (1 + rho), (1 + rho chi), rho chi, (1 + psi rho), psi rho and (1 - psi)
 *   are formed on the host too and reach the kernels as doubles.
 *   Initial simplex: sim[0] = the start, which must lie inside the box and must not be NaN (else SMM_ERR_INVALID_ARG with the 1-based search
 *   and parameter in the message; nothing runs); sim[k + 1] = the start with coordinate k replaced by y = x_k + step * (ub_k - lb_k); if
 *   y > ub_k then y = 2 * ub_k - y; then y = min(max(y, lb_k), ub_k).  All N + 1 vertices are evaluated.
 *   Sort, after the initial evaluation and at the end of every iteration: stable, ascending in fsim, NaN last, +inf just before NaN; equal
 *   values keep their current order (np.argsort(kind="stable")).
 *   No finite value (departure 1 from scipy, which would shrink until maxiter): after any sort, if fsim[0] is not finite the search stops with
 *   status 2.
 *   The loop, while fewer than max_iter iterations have run (else the search stops with status 0):
 *   Convergence: size_x = max |sim[j][k] - sim[0][k]| over j >= 1 and all k, size_f = max |fsim[0] - fsim[j]| over j >= 1; the search stops
 *   converged, status 1, when size_x <= xatol && size_f <= fatol; a NaN in either maximum (size_f is then NaN) makes the test false.  size_x
 *   and size_f are NaN for a search that stopped before its first test.
 *   Centroid and reflection: xbar_k = (sim[0][k] + sim[1][k] + ... + sim[N-1][k]) / N, added left to right; xr = clip((1 + rho) * xbar -
 *   rho * sim[N]); fxr its value.  clip(x) = min(max(x, lb), ub) per coordinate.
 *   Branches, scipy's comparisons literally (a NaN fails every <):
 *     fxr < fsim[0]:        xe = clip((1 + rho chi) * xbar - rho chi * sim[N]); take xe if fxe < fxr (expansion), else take xr (reflection);
 *     else fxr < fsim[N-1]: take xr (reflection);
 *     else fxr < fsim[N]:   xc = clip((1 + psi rho) * xbar - psi rho * sim[N]); take xc if fxc <= fxr (outside contraction), else shrink;
 *     else:                 xcc = clip((1 - psi) * xbar + psi * sim[N]); take xcc if fxcc < fsim[N] (inside contraction), else shrink.
 *   "Take" replaces sim[N], its value and its moments — as evaluated, never evaluated again.
 *   Shrink: sim[j] = clip(sim[0] + sigma * (sim[j] - sim[0])) for j = 1 .. N, each evaluated.
 *   The objective's status is not consulted (as in smm_opt_slices).  value = fsim[0] of the final sort (departure 2: scipy reports
 *   np.min(fsim), NaN whenever a vertex's value is; value is what best was evaluated to).  n_eval counts exactly the evaluations above; evaluated is their sum over the searches (evaluations that pad a launch are never counted).
 *   SMM_ERR_INVALID_ARG: starts NULL, K < 1, (int64)K * (np + 1) >= 2^31, step outside (0, 1] or NaN, xatol or fatol negative or NaN,
 *   max_iter < 1.
 *   Scratch: a search takes (np + 2) ((np + nm + 1) x 8 + 4) + (2 np + nm + 1) x 8 + 20 bytes — per vertex its coordinates, moments,
 *   value and place in the order, once more for an evaluation launch (no launch evaluates more than one point per search: the initial
 *   simplex and a shrink go vertex by vertex), and the iteration's points and lists; the searches go in batches under smm_opt_slices'
 *   64 MiB (at least one search per batch), one batch after another; freed before the call returns.  The host reads three 4-byte counts
 *   per iteration: the searches that need a second point, that shrink, that go on. */
typedef struct {             /* caller-allocated; any pointer may be NULL = not returned */
    double*  best;           /* [np][K]        vertex 0 of the final simplex                 */
    double*  value;          /* [K]            its objective value                           */
    double*  sim_moments;    /* [nm][K]        moments as evaluated at that vertex           */
    double*  simplex;        /* [np+1][np][K]  the final simplex                             */
    double*  simplex_value;  /* [np+1][K]      its values, in final sorted order             */
    double*  size_x;         /* [K]            the two quantities of the last convergence test */
    double*  size_f;         /* [K]                                                          */
    int32_t* iterations;     /* [K]            iterations run                                */
    int32_t* status;         /* [K]            1 converged, 0 stopped by max_iter, 2 no finite value */
    int32_t* moves;          /* [5][K]         iterations that ended in reflection, expansion, outside contraction, inside contraction, shrink */
    int32_t* n_eval;         /* [K]            evaluations of this search                    */
    int64_t  evaluated;      /* out: objective evaluations performed                         */
} smm_opt_simplex_t;
int  smm_opt_simplex(void* ctx, const double* starts /* [np][K], host */, int32_t K, double step, int32_t adaptive, double xatol, double fatol,
                     int32_t max_iter, smm_opt_simplex_t* out);

/* The estimate, third optimiser: K Levenberg–Marquardt searches inside the box [lb, ub], advancing together on the device — the first that
 * uses what an SMM objective is: a weighted sum of squared moment discrepancies, whose simulated moments every evaluation returns beside the
 * value.  An iteration costs np + 1 evaluations and up (a forward-difference Jacobian of the moments, then tries), and a search tens of
 * iterations.  Valid on any context at any iteration; it never changes the chains, the history, the generator's position or which kernel
 * form the next step takes.  A stream objective draws from opts.seed, as smm_eval_batch does (common random numbers: the differences of
 * the Jacobian are differences in the parameters alone).  Ordered on smm_stream behind everything enqueued before (a persistent launch is
 * settled first) and synchronised before it returns; a hard error nobody has been told of yet is returned once, and nothing runs.
 *
 * Numerical contract (every operation rounded on its own, no fma), per search, independent of every other search:
 *   Weights: s_j = w_j if it is finite and not zero, else 1.0 (smm_get_moment_stats' rule).
 *   Residual: r_j = (sim_j - mom_j) / s_j.  F = 0.0 + r_0^2 + r_1^2 + ...: squares rounded, added in ascending j.  The search minimises F, not
 *   the objective's value: for objfunc_norm, dense_sim and dense_sim2 value is F / nm up to rounding; the banana's value is not its moment
 *   distance (its moments are constant: every search ends with status 4), and a user objective's value is whatever its source makes it.
 *   value is reported as evaluated and never consulted, and neither is the objective's status (as in the other two searches).
 *   Start: x = the start, which must lie inside the box and must not be NaN (else SMM_ERR_INVALID_ARG with the 1-based search and parameter in
 *   the message; nothing runs).  It is evaluated; if any r_j is not finite the search stops with status 2.  lambda = lambda0.
 *   An iteration, while fewer than max_iter have run:
 *   Jacobian: h_k = fd_step * (ub_k - lb_k); y = x_k + h_k, and if y > ub_k then y = x_k - h_k; d_k = y - x_k as rounded; point k is x with
 *   coordinate k replaced by y; all np points are evaluated; J_jk = (r_j(point k) - r_j) / d_k.  A J_jk that is not finite: status 2.
 *   Normal equations: g_k = 0.0 + J_0k r_0 + J_1k r_1 + ...; A_kl = 0.0 + J_0k J_0l + J_1k J_1l + ... for l <= k, mirrored; products rounded,
 *   added in ascending j.
 *   Active set: coordinate k is active when (x_k == lb_k && g_k > 0) || (x_k == ub_k && g_k < 0), free otherwise.  Then, in this order:
 *   if a free k has A_kk == 0, no moment moves with that parameter and the search stops with status 4; if |g_k| <= gtol for every free k
 *   (max |g_k| over the free k <= gtol), or no k is free, the search stops with status 1.  For an active k row and column k of A become 0,
 *   A_kk = 1 and g_k = 0 (grad reports g before that).
 *   Tries, at most max_tries per iteration: B = A with B_kk = A_kk + lambda * A_kk; L = B's lower Cholesky factor and delta = the solution
 *   of L L' delta = -g by forward, then back substitution, both in smm_get_moment_stats' order; x_new = min(max(x + delta, lb), ub) per
 *   coordinate, which is evaluated.  A pivot that is not > 0 is a failed try without an evaluation.  The try is accepted when r_new is all
 *   finite and F_new < F; a failed try gives lambda = lambda * lambda_up.
 *   On acceptance x, r, F, value and the moments are replaced, as evaluated (never evaluated again); step = max_k |x_new,k - x_k|, dF = F -
 *   F_new, lambda = max(lambda / lambda_down, 1e-300); if step <= xtol || dF <= ftol * F_new the search stops with status 1; after max_iter
 *   iterations it stops with status 0; else the next iteration begins.
 *   If lambda is no longer finite after a failed try, or max_tries tries of an iteration failed, the search stops with status 3: no descent
 *   was found — at a minimum, the normal ending.
 *   Counts: iterations counts Jacobians, tries every try (a failed pivot too), n_eval exactly the evaluations above: 1, np per iteration and
 *   one per try with a factor; evaluated is their sum over the searches.  Evaluations that pad a launch are never counted: a round of tries
 *   is one launch of one point per search in it, in which a search without a factor — and, in an iteration's first round, one that stopped
 *   at its normal equations — has x evaluated and the result ignored.
 *   Results of a search that stopped before its first Jacobian: grad and jac NaN, active 0; step and dF are NaN before the first accepted try.
 *   SMM_ERR_INVALID_ARG: starts NULL, K < 1, (int64)K * np >= 2^31, fd_step outside (0, 0.5] or NaN, lambda0 <= 0 or not finite,
 *   lambda_up <= 1, lambda_down < 1 (or NaN), xtol, ftol or gtol negative or NaN, max_iter < 1, max_tries < 1.
 *   Scratch: a search takes np ((nm + 1) x 8 + 4) + np x 8 + (nm + np^2 + np) x 8 + 32 bytes — moments, value and status of the Jacobian
 *   launch's np evaluations, a trial point, its residuals, A, x_new, flags and list entries; a user objective's Jacobian points are written
 *   out, np^2 x 8 instead of np x 8 (the built-in objectives' are never written: their evaluation kernel builds each from x and the one
 *   shifted coordinate) —; the searches go in batches under smm_opt_slices' 64 MiB (at least one search per batch), one batch after
 *   another; freed before the call returns.  The results' K x (3 np + nm + 9) x 8 bytes or so (and jac's K nm np x 8 when it is asked for)
 *   hold x, F and lambda of the running searches and are not part of that.  The host reads one 4-byte count per round of tries — the
 *   searches that try again — and one per iteration — the searches that go on. */
typedef struct {             /* caller-allocated; any pointer may be NULL = not returned */
    double*  best;           /* [np][K]      the point each search ended at                  */
    double*  value;          /* [K]          objective value there, as evaluated             */
    double*  sim_moments;    /* [nm][K]      simulated moments there, as evaluated           */
    double*  ssr;            /* [K]          F, the sum of squared residuals, there          */
    double*  grad;           /* [np][K]      the last g, before the active set zeroes it     */
    double*  jac;            /* [nm][np][K]  the last Jacobian of the residuals              */
    double*  lambda;         /* [K]          the final lambda                                */
    double*  step;           /* [K]          step and dF of the last accepted try; NaN before one */
    double*  dF;             /* [K]                                                          */
    int32_t* active;         /* [np][K]      the last active set, 1 = active                 */
    int32_t* iterations;     /* [K]          iterations run                                  */
    int32_t* tries;          /* [K]          tries made                                      */
    int32_t* n_eval;         /* [K]          evaluations of this search                      */
    int32_t* status;         /* [K]          1 converged, 0 stopped by max_iter, 2 a residual or Jacobian entry not finite, 3 no descent found, 4 a parameter moves no moment */
    int64_t  evaluated;      /* out: objective evaluations performed, the sum of n_eval      */
} smm_opt_lm_t;
int  smm_opt_lm(void* ctx, const double* starts /* [np][K], host */, int32_t K, double fd_step, double lambda0, double lambda_up,
                double lambda_down, double xtol, double ftol, double gtol, int32_t max_iter, int32_t max_tries, smm_opt_lm_t* out);

/* Sample without chains: the adaptive population Monte Carlo ABC sampler of Lenormand, Jabot & Deffuant (2013), the whole loop on the
 * device.  The algorithm is likelihood-free, so a posterior read off a history is an ABC posterior (smm_get_adjustment); the standard
 * sampler for ABC is not MCMC but population Monte Carlo: P particles per generation, evaluated independently — no accept step, no
 * exchange, no serial dependence; a generation is one batched evaluation plus reductions.  The prior is uniform on the box [lb, ub]; the
 * context's objective value is the distance.  P = n_particles, A = n_keep; scale 2.0 is the paper's kernel.  Valid on any context at any
 * iteration; it never changes the chains, the history, the generator's position or which kernel form the next step takes.  A stream
 * objective draws from opts.seed, as smm_eval_batch does.  Ordered on smm_stream behind everything enqueued before (a persistent launch is
 * settled first) and synchronised before it returns; a hard error nobody has been told of yet is returned once, and nothing runs.
 *
 * Numerical contract (every operation rounded on its own, no fma outside smm_exp; integers 64-bit).  All particle arithmetic is in unit
 * space, u = (theta - lb) / (ub - lb), where the prior density is 1; theta_k = u_k * (ub_k - lb_k) + lb_k, as mapto_ab and the proposal
 * compute it.  Philox blocks are philox_stream(opts.seed, STREAM_PMC = 8, counter) of smm_rng.hpp; u53 its uniform in [0, 1).
 *   Generation 0: particle j in [0, P), parameter k: the block at counter {j, 0, k >> 1, 0}; u = u53(x0, x1) for even k, u53(x2, x3) for odd k.
 *     All P particles are evaluated; lw_j = 0.0.
 *   Distance: rho = value where status >= 1 and |value| <= DBL_MAX; otherwise rho = +inf and the particle is counted in n_invalid (the
 *     status is consulted here, unlike in the optimisers: a failed simulation is not a posterior draw).
 *   Select, after every generation: the candidates are the kept particles in stored order, then the new ones in j order.  A' = min(A,
 *     candidates with finite rho); the A' candidates with the smallest rho are kept — ordered by smm_get_chain_stats' sort keys, the IEEE
 *     total order (-0.0 before +0.0), ties to the earlier candidate — and stored in candidate order (a stable compaction).  eps_g = the
 *     largest kept rho (NaN when A' = 0); n_new_kept_g = the new ones among the kept.  A' < 2: the run stops with status 2.
 *   Sampling weights of the kept: M = max lw; w_i = smm_exp(lw_i - M); q_i = (int64) ceil(w_i * 1048576.0), at least 1; Q = sum q_i;
 *     wn_i = (double) q_i / (double) Q; ess_g = ((double) Q * (double) Q) / (double) sum q_i^2.  Integer sums: none depends on an order.
 *     A' = 0: ess_g NaN.
 *   Stop, after the select and the weights of generation g, the first that applies: A' < 2: status 2; g >= 1 and p_acc_g <= p_acc_min:
 *     status 1; g == max_gen: status 0.  p_acc_g = (double)(new particles of g with rho < eps_(g-1)) / (double)(P - A'), A' the previous
 *     generation's, rho as it stands after the underflow rule below; p_acc_0 NaN.  eps never increases: the kept set is always the best
 *     of a superset.
 *   Kernel covariance (when the run goes on): mean_k = S(wn_i * u_ik); C_kl = S(e_ik * e_il), e_ik = sqrt(wn_i) * (u_ik - mean_k) —
 *     smm_get_reweighted's pair sums; S the chunked pairwise sum of smm_get_group_stats, chunks of 8192 from the first kept particle.
 *     Sigma_kl = scale * C_kl, then Sigma_kk = Sigma_kk + ridge.  L = chol(Sigma) by smm_adapt_proposal's rule; a pivot with !(s > 0) stops
 *     the run with status 3, and the kept set is the result.  logc = -((double) np * 0.9189385332046727) - t, t = 0.0, t = t + smm_log(L_kk)
 *     over k ascending.
 *   Whitening: z = L^-1 u by forward substitution: s = u_k, then s = s - L_km * z_m for m = 0 .. k-1 in that order, z_k = s / L_kk.
 *   New particle j in [0, P - A'), generation g >= 1.  Parent: v = u53(x0, x1) of the block at counter {j, g, 0, 1}; r = min((int64)(v *
 *     (double) Q), Q - 1); the parent is the kept i with prefix_i <= r < prefix_i + q_i, prefix the exclusive integer prefix of q in stored
 *     order.  Normals: n_2m and n_2m+1 are box_muller of the block at counter {j, g, m, 2}.  Step: y_k = L_k0 * n_0, then + L_km * n_m left
 *     to right up to m = k, exactly as the Cholesky step of smm_propose.hpp; u_k = u_parent,k + y_k.  The particle is inside when
 *     0 <= u_k <= 1 for every k (inclusive; a NaN fails).  An outside particle is not evaluated: rho = +inf, counted in n_outside.
 *   Importance weight of a new particle with a finite rho (weights of particles that cannot be kept are never reported, so the others are
 *     not computed), over the previous generation's kept i in stored order: d2 = (z_0 - z_i0)^2, then + (z_k - z_ik)^2 left to right;
 *     t_i = wn_i * smm_exp(-0.5 * d2).  D = T(t): blocks of 256 consecutive kept particles from the first; each block's terms added left to
 *     right from 0.0; the block sums added left to right from 0.0 — never a function of grid or scheduling.  lw = -(smm_log(D) + logc).
 *     D < DBL_MIN: rho = +inf, counted in n_underflow.
 *   Summary of the final kept set, in parameter space: mean_k = S(wn_i * theta_ik); cov_kl = S(e_ik * e_il) with e on theta, without scale or
 *     ridge (the weighted population form; both triangles hold the same value); quantile p: smm_get_adjustment's integer rule on the q_i:
 *     target = max(1, (int64) ceil(p * (double) Q)), the smallest kept theta_.k at which the q of the rows with theta <= it reach the
 *     target, over the IEEE total order, one of the rows' own doubles.  ess = the last generation's ess_g.  n_kept = 0: all NaN.
 *   Rows past n_kept are NaN (born: -1); entries of generations past the last are NaN or -1.  evaluated = P + the inside particles of every
 *     later generation.
 *   SMM_ERR_INVALID_ARG: n_particles > 2^22 (so that sum q^2 fits 63 bits), n_keep < 2 or >= n_particles, max_gen < 0, p_acc_min outside
 *     [0, 1) or NaN, scale not > 0, ridge negative or not finite, n_probs < 0, probs NULL with n_probs > 0, a prob outside [0, 1] or NaN;
 *     nothing runs then.
 *   Scratch: the particles stay resident — u, z, theta, moments, rho, lw for P new particles and twice for A kept ones, q, its prefix, wn and a
 *     second copy of z by particle (up to 512 bytes each) for the kept — plus 64 block sums of T per new particle (512 P bytes) and one evaluation launch's parameters, moments, value and
 *     status ((np + nm + 1) x 8 + 4 bytes an evaluation), the inside particles going in batches under smm_opt_slices' 64 MiB; freed before
 *     the call returns.  The host reads two small counts per generation: the particles inside, then A' and whether the run goes on. */
typedef struct {              /* caller-allocated; any pointer may be NULL = not returned; G1 = max_gen + 1 */
    double*  theta;           /* [np][A]     the kept particles, in stored order                   */
    double*  value;           /* [A]         their distances                                       */
    double*  sim_moments;     /* [nm][A]     their moments as evaluated                            */
    double*  weight;          /* [A]         wn: the normalised sampling weights                   */
    double*  logw;            /* [A]         lw                                                    */
    int32_t* born;            /* [A]         the generation each was proposed in                   */
    double*  eps;             /* [G1]        the largest kept distance after each generation       */
    double*  p_acc;           /* [G1]        NaN at generation 0                                   */
    double*  gen_ess;         /* [G1]                                                              */
    int32_t* n_outside;       /* [G1]        new particles outside the box                         */
    int32_t* n_invalid;       /* [G1]        evaluated particles without a valid finite value      */
    int32_t* n_underflow;     /* [G1]        new particles whose kernel mixture underflowed        */
    int32_t* n_new_kept;      /* [G1]        new particles among the kept                          */
    double*  mean;            /* [np]                                                              */
    double*  cov;             /* [np][np]                                                          */
    double*  quantile;        /* [n_probs][np]                                                     */
    double   ess;             /* out: the last generation's ess                                    */
    int32_t  n_kept;          /* out: A' of the last generation                                    */
    int32_t  generations;     /* out: the last generation run                                      */
    int32_t  status;          /* out: 0 max_gen, 1 p_acc <= p_acc_min, 2 fewer than 2 finite particles, 3 kernel covariance not PD */
    int32_t  reserved;
    int64_t  evaluated;       /* out: objective evaluations performed                              */
} smm_abc_pmc_t;
int  smm_abc_pmc(void* ctx, int32_t n_particles /* P */, int32_t n_keep /* A */, int32_t max_gen, double p_acc_min, double scale /* 2.0 is the paper's */,
                 double ridge, const double* probs, int32_t n_probs, smm_abc_pmc_t* out);

/* Identify: variance-based global sensitivity over a box — the Sobol' first-order and total-order indices of the objective value and of
 * every simulated moment with respect to every parameter: which parameters move which moments, and how much of that is interaction
 * (total - first).  smm_get_moment_stats answers locally and linearly, where the chains went; smm_opt_lm's status 4 at one point; this over
 * the whole box [lo, hi] (NULL, NULL: the context's [lb, ub]) under the uniform distribution.  N = n_base base points need N (np + 2)
 * independent evaluations: no accept step, no exchange, no serial dependence.  F = nm + 1 outputs: output 0 is the objective value, output
 * 1 + f simulated moment f.  Valid on any context at any iteration; it never changes the chains, the history, the generator's position or
 * which kernel form the next step takes.  A stream objective draws from opts.seed, as smm_eval_batch does.  Ordered on smm_stream behind
 * everything enqueued before (a persistent launch is settled first) and synchronised before it returns; a hard error nobody has been told
 * of yet is returned once, and nothing runs.
 *
 * Numerical contract (every operation rounded on its own, no fma).
 *   Points: Philox blocks are philox_stream(opts.seed, STREAM_GSA = 9, counter) of smm_rng.hpp; u53 its uniform in [0, 1).  Base point j in
 *     [0, N), parameter k: a_jk = u53(x0, x1) for even k, u53(x2, x3) for odd k, of the block at counter {j, 0, k >> 1, 0}; b_jk the same at
 *     counter {j, 1, k >> 1, 0}.  theta = u * (hi_k - lo_k) + lo_k.  Matrix m = 0 is A, m = 1 is B, m = 2 + i is A with coordinate i taken
 *     from B: yA_j, yB_j and yABi_j are the outputs at base point j.
 *   Validity: an evaluation is valid when status >= 1 and all F of its outputs are finite (|y| <= DBL_MAX); the others of the N (np + 2)
 *     are counted in n_invalid.  Base point j is complete when all np + 2 of its evaluations are valid; an incomplete one adds no term
 *     anywhere (skipped, not zero-filled).  n = n_complete, as a double in every division.
 *   Centre: a pilot evaluates a_j for j < min(N, 256) once more; centre_f = T(y_f over the pilot's valid evaluations) / (double) their
 *     number, 0.0 without one.  The pilot's invalid evaluations are not counted in n_invalid.  The first-order estimator is unbiased under
 *     any constant shift of yB; the centre removes the variance a large mean adds; being a pilot it does not depend on the batch size.
 *   T, the sum over base points in j order: blocks of 256 consecutive j from 0; a block's terms added left to right from 0.0, skipping
 *     incomplete points; the block sums added left to right from 0.0 — never a function of grid, batch size or scheduling.
 *   Per output f: mean = T(yA) / n; var = T(d * d) / n, d = yA - mean: a second pass.
 *   Per (f, i): p_j = (yB_j - centre_f) * (yABi_j - yA_j); q_j = e * e, e = yA_j - yABi_j; h_j = 0.5 * q_j.
 *     v_first = T(p) / n (Saltelli et al. 2010); v_total = T(q) / (2.0 * n) (Jansen 1999); first = v_first / var; total = v_total / var.
 *     se_first = sqrt(r / n) / var, r = T(p * p) / n - v_first * v_first, a negative r replaced by 0.0; se_total the same with
 *     r = T(h * h) / n - v_total * v_total: what is summed for it is the square of half of q.  The standard errors are those of the
 *     numerators alone: they ignore var's own sampling error.  The square root is IEEE's.
 *   Divisions are plain IEEE (0 / 0 gives NaN): a constant output has numerators of exactly 0.0 and a var of 0.0 or of the rounding of a
 *     mean of equal values, so its indices are 0.0 or NaN; n = 0 gives NaN everywhere but in centre.  lo_k == hi_k is allowed: the
 *     parameter is frozen, and its indices are 0 or NaN as the arithmetic gives.
 *   evaluated = N (np + 2) + min(N, 256).
 *   SMM_ERR_INVALID_ARG: n_base < 1 or > 2^20, exactly one of lo and hi NULL, any !(lb_k <= lo_k <= hi_k <= ub_k) (a NaN too); nothing
 *     runs then.
 *   Scratch: resident are yA [F][N], a flag per base point, the block sums — 4 x F x np doubles per block of T for the pairs, F for yA — and
 *     the pilot's launch (at most 256 evaluations); one evaluation launch's parameters, moments, value and status ((np + nm + 1) x 8 + 4
 *     bytes an evaluation, np + 2 evaluations a base point), the base points going in batches under smm_opt_slices' 64 MiB (at least one
 *     base point per batch; a block of T that spans batches goes on from its partial sums); the built-in objectives' points are never
 *     written.  Freed before the call returns.  The host reads nothing per batch. */
typedef struct {              /* caller-allocated; any pointer may be NULL = not returned; F = nm + 1 */
    double*  mean;            /* [F]                                                               */
    double*  var;             /* [F]                                                               */
    double*  centre;          /* [F]                                                               */
    double*  first;           /* [F][np]     S1                                                    */
    double*  total;           /* [F][np]     ST                                                    */
    double*  v_first;         /* [F][np]     the numerators                                        */
    double*  v_total;         /* [F][np]                                                           */
    double*  se_first;        /* [F][np]                                                           */
    double*  se_total;        /* [F][np]                                                           */
    int64_t  n_complete;      /* out: base points with np + 2 valid evaluations                    */
    int64_t  n_invalid;       /* out: invalid evaluations among the N (np + 2)                     */
    int64_t  evaluated;       /* out: objective evaluations performed                              */
} smm_sens_sobol_t;
int  smm_sens_sobol(void* ctx, int32_t n_base /* N */, const double* lo, const double* hi /* [np] host, NULL = lb / ub */, smm_sens_sobol_t* out);
int  smm_get_timing(void* ctx, smm_timing_t* out);
/* on = 1: bracket every kernel of smm_bgp_step with hipEvents on the ctx stream so that
 * smm_get_timing reports iter_kernel_ms / exch_kernel_ms (sums over the last step; each bracket
 * contains the event overhead reported as null_bracket_ms).
 * on = 2: the kernels carry their own start/stop events (hipExtLaunchKernelGGL): the sums are the
 * dispatch-begin to dispatch-end durations the command processor stamps, i.e. what rocprofv3
 * --kernel-trace reports; null_bracket_ms = 0.   on = 0: off. */
int  smm_set_profiling(void* ctx, int32_t on);
/* The persistent form of smm_bgp_step and smm_bgp_p2p_step (smm.jl_amd/csrc/smm_chain_persist_loc.hpp, smm_chain_persist_gen.hpp, smm_chain_persist_tile.hpp;
 * replaces the loop of run!, AlgoAbstract.jl:38-45, over computeNextIteration!, AlgoBGP.jl:589-640): where a context qualifies a step of
 * n >= 2 iterations is ONE kernel launch per look-ahead window (<= 256 iterations) instead of one per iteration.  Results are
 * bit-identical.  A context qualifies with
 *   - objfunc_norm with at most two parameters / moments and ns <= 10240, one proposal batch, isotropic proposals, dist_fun = `-`, ONE
 *     min_improve >= 0 (or NaN) for all chains — 0, or the reference's default 0.5 (AlgoBGP.jl:522); a single shard also one PER chain,
 *     below —, at most one 16-chain tile per
 *     compute unit: a single shard of up to 4096 chains (smm_bgp_step), or a SHARD of a sharded run (smm_bgp_p2p_step: N a multiple
 *     of 16, N <= 4096 per rank, N_global <= 32768; the ring of tagged words then lives in every rank's window, a hard error inside
 *     such a launch is agreed upon by the ranks at their next smm_sync / smm_bgp_p2p_finish and replayed by every rank up to the
 *     failing iteration);
 *   - the banana objective, or a USER objective in the one-thread-per-evaluation form (smm_register_user_objective: the library compiles
 *     the persistent kernel once more with the user's source inside, through hiprtc, when the first such context is created: ~1.5 s),
 *     with at most 16 parameters / moments (one proposal batch, isotropic, min_improve == 0) on a single shard of up to 8192 chains in
 *     whole groups of 32;
 *   - objfunc_norm with MORE than two parameters (the reference's own larger examples have 6 and 18, Examples.jl:210-230, 232-319; with a
 *     Cholesky factor: any number), the
 *     dense objectives (SMM_OBJ_DENSE, SMM_OBJ_DENSE2), or a USER objective in its MAP-REDUCE form (smm_register_user_objective_lanes with
 *     64, 128, 256 or 512 lanes per evaluation: the library compiles the persistent tile kernel once more with the user's source inside,
 *     through hiprtc, when the first such context is created; a tile's 512 lanes then evaluate 512 / lanes chains at a time with the
 *     stand-alone kernel's reduction order — the same bits; it pays while an evaluation is short beside the ~40 us of three launches per
 *     iteration: a long simulation fills the device better from its own launches, smm_set_persistent(ctx, 0)):
 *     one proposal batch or several, isotropic proposals or — single shards only — a Cholesky factor (chol_L, shared or per chain; a
 *     map-reduce user objective's form for a factor is a further hiprtc module, compiled only when a context with a factor first wants
 *     it), dist_fun = `-`, ONE min_improve >= 0 (or NaN) for all chains, a single shard of
 *     at most two 16-chain tiles per compute unit whose blocks fit the LDS (np = nm = 50: yes; 64 + 64: no) — or a SHARD of a sharded run
 *     (smm_bgp_p2p_step; smm_chain_persist_tile.hpp, SH) with the same conditions and: equal shards of whole tiles (N a multiple of 16,
 *     chain_offset a multiple of N, at most 8 ranks), N_global <= 8192 (the LDS plan), min_improve the same for every chain.  A
 *     map-reduce user objective's shard form is a second hiprtc module, compiled only when a sharded context first wants it.
 *   - (round 6) min_improve BY CHAIN, what the reference's API takes (a vector, AlgoBGP.jl:522; the pair (i, j) is tested against chain i's,
 *     :688): single shards of the objfunc_norm and tile forms above walk one threshold per chain, every one >= 0 or NaN; a context's single
 *     iterations keep the per-iteration kernels' walk on any thresholds.
 * A negative threshold, other dist_fun, Cholesky proposals of the banana or a one-thread user objective,
 * user objectives with 1024 lanes; as shards: Cholesky proposals, thresholds by chain, N_global past
 * 8192 for anything but objfunc_norm with at most two parameters (bench.py --gpus 8 --workload c5's weak-scaling 32768 chains among them),
 * the banana and one-thread user objectives: the per-iteration kernels.
 * on = 0 keeps the one-launch-per-iteration kernels (default: on).  A hard error of the algorithm inside such a launch is found at
 * the next call that checks (smm_sync, smm_bgp_step, the state readers): the library then repeats those iterations from the state
 * it saved on the one-launch-per-iteration path, so that the context stands at the failing iteration exactly as documented above.
 * All tiles of such a launch must be resident together; on a device that shows the process fewer compute units than it reports (a CU
 * mask, a partition) the first launch gives up after 0.4 s, the step is replayed on the per-iteration kernels, and after the second
 * such time-out the form is off for the context (smm_get_persistent says so).
 * smm_get_persistent: whether the next step would take this form; launches of it so far; repairs so far. */
int  smm_set_persistent(void* ctx, int32_t on);
int  smm_get_persistent(void* ctx, int32_t* available, int32_t* launches, int32_t* repairs);
/* The exchange plan of a window of iterations depends on (seed, iteration) alone.  A single shard on the locally numbered persistent form
 * (persistent=loc) of up to some 4390 chains has the NEXT window's plan made beside the chain kernel — a small kernel on a second stream,
 * in the registers and the LDS the chain kernel leaves on every compute unit — instead of ahead of it on the main stream; the first
 * window, and one a jump (smm_set_state) or a step pattern asks for that is not the one planned ahead, are planned on the main stream
 * as ever.  Results are the same to the bit; the host waits for nothing more.  beside: whether this context plans that way; the plan
 * windows entered so far that were planned beside / on the main stream.  Any pointer may be NULL. */
int  smm_get_plan_beside(void* ctx, int32_t* beside, int32_t* windows_beside, int32_t* windows_instream);
/* one line naming the forms this context was given at creation — per-iteration chain kernel, where the exchange is walked, the stand-alone
 * resolution, the persistent form, the look-ahead plan and its window: "chain=iter_norm walk=inline_lean exchange=lean persistent=loc
 * plan=lds window=256" (diagnostic; tests/test_gpu_forms.py holds the table of what is chosen when) */
int  smm_describe(void* ctx, char* out, int32_t cap);
/* copy of the shock matrix actually used, [nm][ns] */
int  smm_get_Z(void* ctx, double* Z);

#ifdef __cplusplus
}
#endif
#endif /* SMMHIP_H */
