# SMMHip.jl — raw Julia binding of libsmmhip.so (the C ABI of include/smmhip.h, ABI version 2).
#
# Stdlib only (Libdl): loads without a package registry and without SMM.jl.  The drop-in layer for SMM.jl itself —
# `MAlgoBGPHip <: SMM.MAlgo`, `computeNextIteration!`, real `SMM.BGPChain` objects filled from the device, `save`,
# `restart!` — is julia/SMMHipBackend.jl, built on the functions of this file.
#
# NOT EXECUTED IN THIS REPOSITORY'S CI: the build image has no `julia` binary.  What CAN be checked without one is:
# tests/test_julia_layer.py parses the `struct` blocks below and compares field order, types, offsets and sizes
# with the C header (through a compiled probe), checks that every `ccall` names an exported symbol with the header's
# argument count, and that the glue defines the methods the reference dispatches on.  The same ABI is exercised
# end to end through the ctypes binding (smm.jl_amd/_abi.py, tests/).
module SMMHip

using Libdl

export HipBGP, hip_create, hip_destroy!, hip_step!, hip_iter, hip_history, hip_state, hip_set_state!, hip_eval_batch,
       hip_register_objective, hip_register_objective_rng, hip_record_doubles
export hip_eval_batch_noseed, hip_stream, hip_sync, hip_local_step!, hip_export_records!, hip_exchange!, hip_sharded_step!, hip_sharded_finish!,
       hip_a2a_capacity, hip_export_values!, hip_a2a_pack!, hip_a2a_apply!, hip_record_doubles
export hip_chain_stats, hip_chain_cov, hip_chain_diag, hip_rank_diag, hip_get_draws, hip_moment_stats, hip_adjustment, hip_reweighted, hip_profile, hip_density, hip_register_transform, hip_derived, hip_group_stats, hip_histogram, hip_trace, hip_get_proposal, hip_set_proposal!, hip_adapt_proposal!
export hip_set_population!, hip_scatter_population!, hip_opt_slices, hip_opt_simplex, hip_opt_lm, hip_abc_pmc, hip_sens_sobol
export hip_step_async!, hip_p2p_init, hip_p2p_attach!, hip_p2p_step!, hip_p2p_finish!, hip_set_persistent!, hip_persistent_info, P2P_HANDLE_BYTES

const ABI_VERSION = 3
const LIB = Ref{Ptr{Cvoid}}(C_NULL)

"path of the library: ENV[\"SMMHIP_LIBRARY\"] or the in-tree build"
libpath() = get(ENV, "SMMHIP_LIBRARY", joinpath(@__DIR__, "..", "smm.jl_amd", "csrc", "libsmmhip.so"))

function __init__()
    LIB[] = Libdl.dlopen(libpath())          # throws if the library is missing: there is no CPU fallback
    v = ccall(Libdl.dlsym(LIB[], :smm_abi_version), Cint, ())
    v == ABI_VERSION || error("libsmmhip ABI version $v, this binding is written for $ABI_VERSION")
end

sym(s::Symbol) = Libdl.dlsym(LIB[], s)

# ---- mirror of include/smmhip.h (field for field; tests/test_julia_layer.py checks offsets and sizes) -----------
struct SmmProblem
    np::Cint
    nm::Cint
    ns::Cint
    objective_id::Cint
    init::Ptr{Cdouble}
    lb::Ptr{Cdouble}
    ub::Ptr{Cdouble}
    mom::Ptr{Cdouble}
    w::Ptr{Cdouble}
    obj_params::Ptr{Cdouble}
    n_obj_params::Cint
    reserved::Cint
end

struct SmmBgpOpts
    N::Cint
    maxiter::Cint
    sigma::Ptr{Cdouble}
    acc_tuner::Ptr{Cdouble}
    min_improve::Ptr{Cdouble}
    sigma_update_steps::Cint
    smpl_iters::Cint
    sigma_adjust_by::Cdouble
    batch_size::Cint
    exchange_from_iter::Cint
    seed::UInt64
    chain_offset::Cint
    N_global::Cint
    device::Cint
    chol_per_chain::Cint
    chol_L::Ptr{Cdouble}
    dist_fun::Cint
    reserved::Cint
end

struct SmmTables
    probs_acc::Ptr{Cdouble}
    prop_normals::Ptr{Cdouble}
    prop_tries::Cint
    n_pairs::Cint
    pairs::Ptr{Int32}
    Z::Ptr{Cdouble}
end

struct SmmHistory
    value::Ptr{Cdouble}
    prob::Ptr{Cdouble}
    curr_val::Ptr{Cdouble}
    best_val::Ptr{Cdouble}
    params::Ptr{Cdouble}
    sim_moments::Ptr{Cdouble}
    best_id::Ptr{Int32}
    exchanged::Ptr{Int32}
    accepted::Ptr{UInt8}
    status::Ptr{Int8}
end

struct SmmChainStats
    count::Ptr{Int32}
    mean::Ptr{Cdouble}
    median::Ptr{Cdouble}
    quantile::Ptr{Cdouble}
    best_value::Ptr{Cdouble}
    best_iter::Ptr{Int32}
    n_exchanged::Ptr{Int32}
    most_exchanged_with::Ptr{Int32}
end

struct SmmChainDiag
    accept_rate::Ptr{Cdouble}
    ess::Ptr{Cdouble}
    status::Ptr{Int32}
    acf::Ptr{Cdouble}
    rhat::Ptr{Cdouble}
end

struct SmmRankDiag
    rhat_rank::Ptr{Cdouble}
    rhat_bulk::Ptr{Cdouble}
    rhat_folded::Ptr{Cdouble}
    ess_bulk::Ptr{Cdouble}
    ess_tail::Ptr{Cdouble}
    ess_mean::Ptr{Cdouble}
    status::Ptr{Int32}
    rank_hist::Ptr{Int64}
end

struct SmmDraws
    count::Ptr{Int64}
    n_chains::Ptr{Int32}
    row0::Ptr{Int64}
    params::Ptr{Cdouble}
    value::Ptr{Cdouble}
    sim_moments::Ptr{Cdouble}
    chain::Ptr{Int32}
    iter::Ptr{Int32}
    src_iter::Ptr{Int32}
end

struct SmmAdjustment
    count::Ptr{Int64}
    n_chains::Ptr{Int32}
    status::Ptr{Int32}
    n_kept::Ptr{Int64}
    bandwidth::Ptr{Cdouble}
    sum_w::Ptr{Cdouble}
    ess::Ptr{Cdouble}
    x_mean::Ptr{Cdouble}
    raw_mean::Ptr{Cdouble}
    beta::Ptr{Cdouble}
    adj_mean::Ptr{Cdouble}
    adj_sd::Ptr{Cdouble}
    adj_quantile::Ptr{Cdouble}
    n_outside::Ptr{Int64}
end

struct SmmReweighted
    count::Ptr{Int64}
    n_scored::Ptr{Int64}
    n_chains::Ptr{Int32}
    status::Ptr{Int32}
    chain_n::Ptr{Int32}
    chain_ess::Ptr{Cdouble}
    chain_logz::Ptr{Cdouble}
    n_kept::Ptr{Int64}
    sum_u::Ptr{Cdouble}
    ess::Ptr{Cdouble}
    mean::Ptr{Cdouble}
    cov::Ptr{Cdouble}
    value_mean::Ptr{Cdouble}
    m_mean::Ptr{Cdouble}
    quantile::Ptr{Cdouble}
end

struct SmmMomentStats
    count::Ptr{Int64}
    n_chains::Ptr{Int32}
    status::Ptr{Int32}
    p_mean::Ptr{Cdouble}
    m_mean::Ptr{Cdouble}
    m_median::Ptr{Cdouble}
    m_quantile::Ptr{Cdouble}
    cov_pp::Ptr{Cdouble}
    cov_pm::Ptr{Cdouble}
    cov_mm::Ptr{Cdouble}
    fit_z::Ptr{Cdouble}
    jac::Ptr{Cdouble}
    sens::Ptr{Cdouble}
    se::Ptr{Cdouble}
end

struct SmmProfile
    count::Ptr{Int64}
    status::Ptr{Int32}
    edges::Ptr{Cdouble}
    n::Ptr{Int64}
    n_scored::Ptr{Int64}
    v_min::Ptr{Cdouble}
    min_chain::Ptr{Int32}
    min_iter::Ptr{Int32}
    theta_at_min::Ptr{Cdouble}
    v_mean::Ptr{Cdouble}
    m_mean::Ptr{Cdouble}
    edges2::Ptr{Cdouble}
    n2::Ptr{Int64}
    n_scored2::Ptr{Int64}
    v_min2::Ptr{Cdouble}
    min_chain2::Ptr{Int32}
    min_iter2::Ptr{Int32}
    v_mean2::Ptr{Cdouble}
end

struct SmmDensity
    count::Ptr{Int64}
    status::Ptr{Int32}
    hdi_lo::Ptr{Cdouble}
    hdi_hi::Ptr{Cdouble}
    mode::Ptr{Cdouble}
    bw::Ptr{Cdouble}
    kde_status::Ptr{Int32}
    grid::Ptr{Cdouble}
    density::Ptr{Cdouble}
    kde_mode::Ptr{Cdouble}
end

struct SmmDerived
    count::Ptr{Int64}
    n_chains::Ptr{Int32}
    n_nonfinite::Ptr{Int64}
    mean::Ptr{Cdouble}
    median::Ptr{Cdouble}
    quantile::Ptr{Cdouble}
    cov::Ptr{Cdouble}
end

struct SmmGroupStats
    count::Ptr{Int64}
    n_chains::Ptr{Int32}
    mean::Ptr{Cdouble}
    median::Ptr{Cdouble}
    quantile::Ptr{Cdouble}
    cov::Ptr{Cdouble}
end

struct SmmHistogram
    count::Ptr{Int64}
    status::Ptr{Int32}
    lo::Ptr{Cdouble}
    hi::Ptr{Cdouble}
    edges::Ptr{Cdouble}
    hist::Ptr{Int64}
    edges2::Ptr{Cdouble}
    hist2::Ptr{Int64}
end

struct SmmTrace
    iter::Ptr{Int32}
    n_chains::Ptr{Int32}
    count::Ptr{Int32}
    n_accepted::Ptr{Int32}
    n_exchanged::Ptr{Int32}
    n_failed::Ptr{Int32}
    mean::Ptr{Cdouble}
    var::Ptr{Cdouble}
    median::Ptr{Cdouble}
    quantile::Ptr{Cdouble}
    best_value::Ptr{Cdouble}
    best_chain::Ptr{Int32}
end

struct SmmPopulation
    start::Ptr{Cdouble}
    value::Ptr{Cdouble}
    pick::Ptr{Int32}
    evaluated::Int64
end

struct SmmOptSlices
    best::Ptr{Cdouble}
    value::Ptr{Cdouble}
    sim_moments::Ptr{Cdouble}
    lo::Ptr{Cdouble}
    hi::Ptr{Cdouble}
    delta::Ptr{Cdouble}
    cycle_value::Ptr{Cdouble}
    cycles::Ptr{Int32}
    converged::Ptr{Int32}
    evaluated::Int64
end

struct SmmOptSimplex
    best::Ptr{Cdouble}
    value::Ptr{Cdouble}
    sim_moments::Ptr{Cdouble}
    simplex::Ptr{Cdouble}
    simplex_value::Ptr{Cdouble}
    size_x::Ptr{Cdouble}
    size_f::Ptr{Cdouble}
    iterations::Ptr{Int32}
    status::Ptr{Int32}
    moves::Ptr{Int32}
    n_eval::Ptr{Int32}
    evaluated::Int64
end

struct SmmOptLM
    best::Ptr{Cdouble}
    value::Ptr{Cdouble}
    sim_moments::Ptr{Cdouble}
    ssr::Ptr{Cdouble}
    grad::Ptr{Cdouble}
    jac::Ptr{Cdouble}
    lambda::Ptr{Cdouble}
    step::Ptr{Cdouble}
    dF::Ptr{Cdouble}
    active::Ptr{Int32}
    iterations::Ptr{Int32}
    tries::Ptr{Int32}
    n_eval::Ptr{Int32}
    status::Ptr{Int32}
    evaluated::Int64
end

struct SmmAbcPmc
    theta::Ptr{Cdouble}
    value::Ptr{Cdouble}
    sim_moments::Ptr{Cdouble}
    weight::Ptr{Cdouble}
    logw::Ptr{Cdouble}
    born::Ptr{Int32}
    eps::Ptr{Cdouble}
    p_acc::Ptr{Cdouble}
    gen_ess::Ptr{Cdouble}
    n_outside::Ptr{Int32}
    n_invalid::Ptr{Int32}
    n_underflow::Ptr{Int32}
    n_new_kept::Ptr{Int32}
    mean::Ptr{Cdouble}
    cov::Ptr{Cdouble}
    quantile::Ptr{Cdouble}
    ess::Cdouble
    n_kept::Int32
    generations::Int32
    status::Int32
    reserved::Int32
    evaluated::Int64
end

struct SmmSensSobol
    mean::Ptr{Cdouble}
    var::Ptr{Cdouble}
    centre::Ptr{Cdouble}
    first::Ptr{Cdouble}
    total::Ptr{Cdouble}
    v_first::Ptr{Cdouble}
    v_total::Ptr{Cdouble}
    se_first::Ptr{Cdouble}
    se_total::Ptr{Cdouble}
    n_complete::Int64
    n_invalid::Int64
    evaluated::Int64
end

struct SmmState
    iter::Cint
    reserved::Cint
    sigma::Ptr{Cdouble}
    accept_rate::Ptr{Cdouble}
    la_value::Ptr{Cdouble}
    la_prob::Ptr{Cdouble}
    la_params::Ptr{Cdouble}
    la_sim_moments::Ptr{Cdouble}
    la_status::Ptr{Int8}
    n_noex::Ptr{Int32}
    n_acc_noex::Ptr{Int32}
    best_val::Ptr{Cdouble}
    best_id::Ptr{Int32}
end

struct SmmTiming
    step_ms::Cdouble
    iter_kernel_ms::Cdouble
    exch_kernel_ms::Cdouble
    chain_evals::Int64
    iters::Cint
    reserved::Cint
    null_bracket_ms::Cdouble
end

# smm_objective_t
const OBJ_NORM = Cint(0)
const OBJ_BANANA = Cint(1)
const OBJ_NORM_FAILBOX = Cint(2)
const OBJ_DENSE = Cint(3)
const OBJ_DENSE2 = Cint(5)      # the dense simulation with its 256 x 256 stage: BASELINE config 5 as worded
const OBJ_USER_BASE = Cint(1000)
# smm_dist_fun_t (opts["dist_fun"], AlgoBGP.jl:537)
const DIST_MINUS = Cint(0)
const DIST_ABSDIFF = Cint(1)
const DIST_RELDIFF = Cint(2)

struct SMMHipError <: Exception
    code::Int
    msg::String
end
Base.showerror(io::IO, e::SMMHipError) = print(io, "smmhip error ", e.code, ": ", e.msg)

last_error(ctx::Ptr{Cvoid}) = unsafe_string(ccall(sym(:smm_last_error), Cstring, (Ptr{Cvoid},), ctx))
check(ctx::Ptr{Cvoid}, rc::Integer) = rc == 0 ? nothing : throw(SMMHipError(Int(rc), last_error(ctx)))

# ---- one device context = the chains of one MAlgoBGP (shard) ----------------------------------------------------
"""
    HipBGP

Handle of one device context (`smm_ctx_create`): the chains of one `MAlgoBGP` on one GPU.  `N`, `np`, `nm`, `maxiter`
are kept for buffer sizes.  Destroyed by `hip_destroy!` or the finalizer (whichever comes first; never twice).
"""
mutable struct HipBGP
    ctx::Ptr{Cvoid}
    N::Int
    np::Int
    nm::Int
    maxiter::Int
    chol::Int        # the proposal factor: 0 none (isotropic), 1 shared, 2 per chain
end

function hip_destroy!(h::HipBGP)
    if h.ctx != C_NULL
        ccall(sym(:smm_ctx_destroy), Cvoid, (Ptr{Cvoid},), h.ctx)
        h.ctx = C_NULL                      # the finalizer (or a second call) finds nothing to free
    end
    return nothing
end

"""
    hip_create(init, lb, ub, mom, w, sigma, acc_tuner, min_improve; maxiter, ns = 10000, objective_id = OBJ_NORM, ...)

`MAlgoBGP(m, opts)` + the `BGPChain` constructors (AlgoBGP.jl:505-537, :78-109) as one device context.  The per-chain
vectors `sigma`, `acc_tuner`, `min_improve` are GLOBAL (length `N_global`, default `N = length(sigma)`): the reference's
default 3-entry lists must be expanded by the caller (the glue does); shorter vectors are an error here, not a read
past the end of a Julia array inside the library.
"""
function hip_create(init::Vector{Float64}, lb::Vector{Float64}, ub::Vector{Float64}, mom::Vector{Float64}, w::Vector{Float64},
                    sigma::Vector{Float64}, acc_tuner::Vector{Float64}, min_improve::Vector{Float64};
                    maxiter::Integer, ns::Integer = 10000, objective_id::Integer = OBJ_NORM,
                    obj_params::Vector{Float64} = Float64[], N::Integer = length(sigma), N_global::Integer = length(sigma),
                    chain_offset::Integer = 0, sigma_update_steps::Integer = 10, sigma_adjust_by::Real = 0.01,
                    smpl_iters::Integer = 1000, batch_size::Integer = length(init), seed::Integer = 12, device::Integer = 0,
                    chol_L::Union{Nothing,Array{Float64}} = nothing, dist_fun::Integer = DIST_MINUS)
    np, nm = length(init), length(mom)
    length(lb) == np && length(ub) == np || throw(ArgumentError("lb / ub need one entry per parameter"))
    length(w) == nm || throw(ArgumentError("w needs one entry per moment"))
    (length(sigma) >= N_global && length(acc_tuner) >= N_global && length(min_improve) >= N_global) ||
        throw(ArgumentError("sigma / acc_tuner / min_improve need N_global = $N_global entries (AlgoBGP.jl:518-523)"))
    per_chain = 0
    Lrow = Float64[]
    if chol_L !== nothing
        # row-major [np][np] (shared) or [N_global][np][np]: Julia arrays are column-major, so L[k, j] of a Matrix is
        # transposed into the row-major order the header asks for
        if ndims(chol_L) == 2
            size(chol_L) == (np, np) || throw(ArgumentError("chol_L must be np x np"))
            Lrow = vec(permutedims(chol_L, (2, 1)))
        else
            size(chol_L) == (np, np, N_global) || throw(ArgumentError("per-chain chol_L must be np x np x N_global (L[:, :, c])"))
            Lrow = vec(permutedims(chol_L, (2, 1, 3)))
            per_chain = 1
        end
    end
    ctx = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve init lb ub mom w sigma acc_tuner min_improve obj_params Lrow begin
        p = SmmProblem(np, nm, ns, objective_id, pointer(init), pointer(lb), pointer(ub), pointer(mom), pointer(w),
                       isempty(obj_params) ? Ptr{Cdouble}(C_NULL) : pointer(obj_params), length(obj_params), 0)
        o = SmmBgpOpts(N, maxiter, pointer(sigma), pointer(acc_tuner), pointer(min_improve), sigma_update_steps, smpl_iters,
                       Float64(sigma_adjust_by), batch_size, 2, UInt64(seed), chain_offset, N_global, device, per_chain,
                       isempty(Lrow) ? Ptr{Cdouble}(C_NULL) : pointer(Lrow), dist_fun, 0)
        rc = ccall(sym(:smm_ctx_create), Cint, (Ref{SmmProblem}, Ref{SmmBgpOpts}, Ptr{SmmTables}, Ref{Ptr{Cvoid}}),
                   p, o, C_NULL, ctx)
        rc == 0 || throw(SMMHipError(Int(rc), last_error(Ptr{Cvoid}(C_NULL))))
    end
    h = HipBGP(ctx[], Int(N), np, nm, Int(maxiter), chol_L === nothing ? 0 : per_chain == 1 ? 2 : 1)
    finalizer(hip_destroy!, h)
    return h
end

"`n` x `computeNextIteration!` (AlgoBGP.jl:589-640, incl. `exchangeMoves!` :647-716) in one enqueue; blocks"
function hip_step!(h::HipBGP, n::Integer = 1)
    check(h.ctx, ccall(sym(:smm_bgp_step), Cint, (Ptr{Cvoid}, Cint), h.ctx, n))
    return h
end

"""
    hip_step_async!(h, n)

The same, enqueued only: returns at once, `hip_sync(h)` waits (and reports a hard error of the reference, AlgoBGP.jl:341,409).
Steps of n >= 2 iterations take the persistent form where the context qualifies (include/smmhip.h, smm_set_persistent).
"""
function hip_step_async!(h::HipBGP, n::Integer = 1)
    check(h.ctx, ccall(sym(:smm_bgp_step_async), Cint, (Ptr{Cvoid}, Cint), h.ctx, n))
    return h
end

"the persistent form of `hip_step!` (include/smmhip.h): on by default where the context qualifies"
hip_set_persistent!(h::HipBGP, on::Bool) = (check(h.ctx, ccall(sym(:smm_set_persistent), Cint, (Ptr{Cvoid}, Cint), h.ctx, on ? 1 : 0)); h)
"(would the next step take the persistent form, launches of it so far, repairs so far)"
function hip_persistent_info(h::HipBGP)
    a = Ref{Int32}(0); l = Ref{Int32}(0); r = Ref{Int32}(0)
    check(h.ctx, ccall(sym(:smm_get_persistent), Cint, (Ptr{Cvoid}, Ref{Int32}, Ref{Int32}, Ref{Int32}), h.ctx, a, l, r))
    return (a[] != 0, Int(l[]), Int(r[]))
end

"completed iterations (after a hard error: the failing iteration, see include/smmhip.h)"
hip_iter(h::HipBGP) = hip_state(h).iter

hip_record_doubles(h::HipBGP) = Int(ccall(sym(:smm_bgp_record_doubles), Cint, (Ptr{Cvoid},), h.ctx))

# The sharded forms (one HipBGP per GPU and process; device pointers of the caller's communication library, e.g. the
# buffers of an MPI.jl / RCCL wrapper; everything is enqueued on hip_stream(h)).  include/smmhip.h describes the protocols.
hip_stream(h::HipBGP) = ccall(sym(:smm_stream), Ptr{Cvoid}, (Ptr{Cvoid},), h.ctx)
hip_sync(h::HipBGP) = (check(h.ctx, ccall(sym(:smm_sync), Cint, (Ptr{Cvoid},), h.ctx)); h)
hip_local_step!(h::HipBGP) = (check(h.ctx, ccall(sym(:smm_bgp_local_step), Cint, (Ptr{Cvoid},), h.ctx)); h)
hip_export_records!(h::HipBGP, rec::Ptr{Cvoid}) = (check(h.ctx, ccall(sym(:smm_bgp_export_records_dev), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), h.ctx, rec)); h)
hip_exchange!(h::HipBGP, gathered::Ptr{Cvoid}) = (check(h.ctx, ccall(sym(:smm_bgp_exchange_dev), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), h.ctx, gathered)); h)
hip_sharded_step!(h::HipBGP, prev::Ptr{Cvoid}, next::Ptr{Cvoid}) =
    (check(h.ctx, ccall(sym(:smm_bgp_sharded_step), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), h.ctx, prev, next)); h)
hip_sharded_finish!(h::HipBGP, gathered::Ptr{Cvoid}) =
    (check(h.ctx, ccall(sym(:smm_bgp_sharded_finish), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), h.ctx, gathered)); h)
# the values form for long records: all-gather of N doubles per rank, then one all-to-all of hip_a2a_capacity(h) * RW doubles per pair
hip_a2a_capacity(h::HipBGP) = Int(ccall(sym(:smm_bgp_a2a_capacity), Cint, (Ptr{Cvoid},), h.ctx))
hip_export_values!(h::HipBGP, vals::Ptr{Cvoid}) = (check(h.ctx, ccall(sym(:smm_bgp_export_values_dev), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), h.ctx, vals)); h)
hip_a2a_pack!(h::HipBGP, vals_all::Ptr{Cvoid}, send::Ptr{Cvoid}) =
    (check(h.ctx, ccall(sym(:smm_bgp_a2a_pack_dev), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), h.ctx, vals_all, send)); h)
hip_a2a_apply!(h::HipBGP, recv::Ptr{Cvoid}) = (check(h.ctx, ccall(sym(:smm_bgp_a2a_apply_dev), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), h.ctx, recv)); h)

# The p2p form (no collective at all: every rank owns a window that the others map through HIP IPC; include/smmhip.h).  The handles
# are 64 plain bytes: any transport hands them round once — julia/SMMHipSharded.jl does it with Distributed alone.
const P2P_HANDLE_BYTES = 64
"this rank's window: returns its IPC handle (for the other PROCESSES) as a Vector{UInt8}"
function hip_p2p_init(h::HipBGP)
    handle = zeros(UInt8, P2P_HANDLE_BYTES)
    win = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve handle check(h.ctx, ccall(sym(:smm_bgp_p2p_init), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Ref{Ptr{Cvoid}}), h.ctx, pointer(handle), win))
    return handle
end
"rank `rank`'s window by its IPC handle (ranks are 0-based: chain_offset / N)"
function hip_p2p_attach!(h::HipBGP, rank::Integer, handle::Vector{UInt8})
    length(handle) == P2P_HANDLE_BYTES || throw(ArgumentError("an IPC handle is $P2P_HANDLE_BYTES bytes"))
    GC.@preserve handle check(h.ctx, ccall(sym(:smm_bgp_p2p_attach), Cint, (Ptr{Cvoid}, Cint, Ptr{UInt8}, Ptr{Cvoid}), h.ctx, rank, pointer(handle), C_NULL))
    return h
end
"n iterations of this shard, enqueued (every rank calls it with the same n); `hip_sync` waits"
hip_p2p_step!(h::HipBGP, n::Integer) = (check(h.ctx, ccall(sym(:smm_bgp_p2p_step), Cint, (Ptr{Cvoid}, Cint), h.ctx, n)); h)
"settle the last iteration into the context (before history / state are read); every rank calls it"
hip_p2p_finish!(h::HipBGP) = (check(h.ctx, ccall(sym(:smm_bgp_p2p_finish), Cint, (Ptr{Cvoid},), h.ctx)); h)

"""
    hip_history(h, t0, t1) -> NamedTuple

Iterations `t0+1 .. t1` (0-based half-open `[t0, t1)` as in the ABI).  The ABI's buffers are iteration-major
(`[t][chain]`, params `[t][k][chain]`); in Julia's column-major terms `value[chain, t]`, `params[chain, k, t]`.
`exchanged`, `best_id` are 1-based exactly as in `BGPChain` (AlgoBGP.jl:42-110): 0 = no exchange, -1 = unset.
"""
function hip_history(h::HipBGP, t0::Integer, t1::Integer)
    N, T, np, nm = h.N, t1 - t0, h.np, h.nm
    value = Matrix{Float64}(undef, N, T); prob = similar(value); curr = similar(value); best = similar(value)
    pars = Array{Float64}(undef, N, np, T); simm = Array{Float64}(undef, N, nm, T)
    bid = Matrix{Int32}(undef, N, T); exch = similar(bid); acc = Matrix{UInt8}(undef, N, T); st = Matrix{Int8}(undef, N, T)
    GC.@preserve value prob curr best pars simm bid exch acc st begin
        hs = SmmHistory(pointer(value), pointer(prob), pointer(curr), pointer(best), pointer(pars), pointer(simm),
                        pointer(bid), pointer(exch), pointer(acc), pointer(st))
        check(h.ctx, ccall(sym(:smm_get_history), Cint, (Ptr{Cvoid}, Cint, Cint, Ref{SmmHistory}), h.ctx, t0, t1, hs))
    end
    return (value = value, prob = prob, curr_val = curr, best_val = best, params = pars, sim_moments = simm,
            best_id = bid, exchanged = exch, accepted = acc, status = st)
end

"""
    hip_chain_stats(h, t0, t1; accepted_only = true, probs = Float64[]) -> NamedTuple

Summaries of every chain of the context over iterations `t0+1 .. t1`, reduced on the device without downloading the history
(`smm_get_chain_stats`): `count[chain]`, `mean[chain, k]`, `median[chain, k]`, `quantile[chain, k, p]`, `best_value[chain]`,
`best_iter[chain]` (1-based iteration), `n_exchanged[chain]`, `most_exchanged_with[chain]` (1-based global id, 0 = none).
`accepted_only` selects the accepted draws, as `params(c)`.  The numbers are NumPy's (include/smmhip.h), not `Statistics`'.
"""
function hip_chain_stats(h::HipBGP, t0::Integer, t1::Integer; accepted_only::Bool = true, probs::Vector{Float64} = Float64[])
    N, np, nq = h.N, h.np, length(probs)
    count = Vector{Int32}(undef, N); mean = Matrix{Float64}(undef, N, np); median = similar(mean)
    quant = Array{Float64}(undef, N, np, nq); bestv = Vector{Float64}(undef, N); besti = Vector{Int32}(undef, N)
    nex = Vector{Int32}(undef, N); most = Vector{Int32}(undef, N)
    GC.@preserve count mean median quant bestv besti nex most probs begin
        cs = SmmChainStats(pointer(count), pointer(mean), pointer(median), nq > 0 ? pointer(quant) : Ptr{Cdouble}(C_NULL),
                           pointer(bestv), pointer(besti), pointer(nex), pointer(most))
        check(h.ctx, ccall(sym(:smm_get_chain_stats), Cint, (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cdouble}, Cint, Ref{SmmChainStats}),
                           h.ctx, t0, t1, accepted_only ? 1 : 0, nq > 0 ? pointer(probs) : Ptr{Cdouble}(C_NULL), nq, cs))
    end
    return (count = count, mean = mean, median = median, quantile = quant, best_value = bestv, best_iter = besti,
            n_exchanged = nex, most_exchanged_with = most)
end

"""
    hip_chain_cov(h, t0, t1; accepted_only = true, unit_space = false) -> NamedTuple

Covariance of every chain's selected draws over iterations `t0+1 .. t1`, on the device (`smm_get_chain_cov`): `count[chain]`,
`mean[chain, k]`, `cov[chain, j, k]`.  `unit_space` maps the draws to [0, 1] first (`mapto_01`, the space of the proposal).
NumPy's summation (include/smmhip.h).
"""
function hip_chain_cov(h::HipBGP, t0::Integer, t1::Integer; accepted_only::Bool = true, unit_space::Bool = false)
    N, np = h.N, h.np
    count = Vector{Int32}(undef, N); mean = Matrix{Float64}(undef, N, np); cov = Array{Float64}(undef, N, np, np)
    GC.@preserve count mean cov begin
        check(h.ctx, ccall(sym(:smm_get_chain_cov), Cint, (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Ptr{Int32}, Ptr{Cdouble}, Ptr{Cdouble}),
                           h.ctx, t0, t1, accepted_only ? 1 : 0, unit_space ? 1 : 0, pointer(count), pointer(mean), pointer(cov)))
    end
    return (count = count, mean = mean, cov = cov)   # (the header's [np][N] / [np][np][N] row-major = these column-major arrays)
end

"""
    hip_chain_diag(h, t0, t1; max_lag = t1 - t0 - 1, n_acf = 0, groups = nothing) -> NamedTuple

Convergence diagnostics of every chain over iterations `t0+1 .. t1`, on the device (`smm_get_chain_diag`): `accept_rate[chain]`,
and per series s (the parameters, then the objective value, `np + 1` of them) `ess[chain, s]`, `status[chain, s]` (0 ok, 1 `max_lag`
reached first, 2 undefined, 3 non-finite series), `acf[chain, s, k + 1]` (rho_k, k < `n_acf`) and, when `groups[chain]` (0-based group
ids, -1 = none) is given, `rhat[s, g + 1]`: the split R-hat of each group.  NumPy's summation (include/smmhip.h).
"""
function hip_chain_diag(h::HipBGP, t0::Integer, t1::Integer; max_lag::Integer = t1 - t0 - 1, n_acf::Integer = 0,
                        groups::Union{Nothing,AbstractVector{<:Integer}} = nothing)
    N, S = h.N, h.np + 1
    g = groups === nothing ? Int32[] : Vector{Int32}(groups)
    groups === nothing || length(g) == N || throw(ArgumentError("groups needs one entry per chain"))
    ng = isempty(g) ? 0 : Int(maximum(g)) + 1
    rate = Vector{Float64}(undef, N); ess = Matrix{Float64}(undef, N, S); st = Matrix{Int32}(undef, N, S)
    acf = Array{Float64}(undef, N, S, n_acf); rhat = Matrix{Float64}(undef, S, ng)
    GC.@preserve g rate ess st acf rhat begin
        cd = SmmChainDiag(pointer(rate), pointer(ess), pointer(st), n_acf > 0 ? pointer(acf) : Ptr{Cdouble}(C_NULL),
                          ng > 0 ? pointer(rhat) : Ptr{Cdouble}(C_NULL))
        check(h.ctx, ccall(sym(:smm_get_chain_diag), Cint, (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Ptr{Int32}, Cint, Ref{SmmChainDiag}),
                           h.ctx, t0, t1, max_lag, n_acf, ng > 0 ? pointer(g) : Ptr{Int32}(C_NULL), ng, cd))
    end
    return (accept_rate = rate, ess = ess, status = st, acf = acf, rhat = rhat)   # (the header's row-major = these column-major arrays)
end

"""
    hip_rank_diag(h, t0, t1; max_lag = (t1 - t0) ÷ 2 - 1, n_bins = 20, groups = nothing) -> NamedTuple

Rank-normalised diagnostics of groups of chains over iterations `t0+1 .. t1`, on the device (`smm_get_rank_diag`; Vehtari et al.
2021): per series s (the parameters, then the objective value, `np + 1` of them) and group g `rhat_rank[s, g]` (the larger of
`rhat_bulk` and `rhat_folded`), `ess_bulk[s, g]`, `ess_tail[s, g]`, `ess_mean[s, g]`, `status[s, g, 1:4]` (bulk, folded, tail, mean:
0 ok, 1 `max_lag` reached first, 2 undefined, 3 non-finite) and `rank_hist[chain, s, bin]`, each chain's ranks in its group's pooled
sample, binned (the rank plot).  `groups[chain]` holds 0-based group ids (-1 = none); `nothing`: every chain in one group.
"""
function hip_rank_diag(h::HipBGP, t0::Integer, t1::Integer; max_lag::Integer = (t1 - t0) ÷ 2 - 1, n_bins::Integer = 20,
                       groups::Union{Nothing,AbstractVector{<:Integer}} = nothing)
    N, S = h.N, h.np + 1
    g = groups === nothing ? Int32[] : Vector{Int32}(groups)
    groups === nothing || length(g) == N || throw(ArgumentError("groups needs one entry per chain"))
    ng = groups === nothing ? 1 : (isempty(g) ? 0 : Int(maximum(g)) + 1)
    rr = Matrix{Float64}(undef, S, ng); rb = Matrix{Float64}(undef, S, ng); rf = Matrix{Float64}(undef, S, ng)
    eb = Matrix{Float64}(undef, S, ng); et = Matrix{Float64}(undef, S, ng); em = Matrix{Float64}(undef, S, ng)
    st = Array{Int32}(undef, S, ng, 4); rh = Array{Int64}(undef, N, S, n_bins)
    GC.@preserve g rr rb rf eb et em st rh begin
        rd = SmmRankDiag(pointer(rr), pointer(rb), pointer(rf), pointer(eb), pointer(et), pointer(em), pointer(st),
                         n_bins > 0 ? pointer(rh) : Ptr{Int64}(C_NULL))
        check(h.ctx, ccall(sym(:smm_get_rank_diag), Cint, (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Ptr{Int32}, Cint, Ref{SmmRankDiag}),
                           h.ctx, t0, t1, max_lag, n_bins, groups === nothing ? Ptr{Int32}(C_NULL) : pointer(g), ng, rd))
    end
    return (rhat_rank = rr, rhat_bulk = rb, rhat_folded = rf, ess_bulk = eb, ess_tail = et, ess_mean = em, status = st,
            rank_hist = rh)   # (the header's row-major = these column-major arrays)
end

"""
    hip_group_stats(h, t0, t1; accepted_only = true, groups = nothing, probs = Float64[]) -> NamedTuple

The posterior of each group's pooled draws over iterations `t0+1 .. t1`, on the device (`smm_get_group_stats`): a group's pooled
column is the concatenation of its members' selected draws, members in ascending chain order.  `groups[chain]` holds 0-based group
ids (-1 = none); `nothing`: every chain in one group.  Returns `count[g]`, `n_chains[g]`, `mean[k, g]`, `median[k, g]`,
`quantile[k, g, p]` and `cov[j, k, g]`.  NumPy's summation and order statistics (include/smmhip.h).
"""
function hip_group_stats(h::HipBGP, t0::Integer, t1::Integer; accepted_only::Bool = true,
                         groups::Union{Nothing,AbstractVector{<:Integer}} = nothing, probs::AbstractVector{<:Real} = Float64[])
    N, np = h.N, h.np
    g = groups === nothing ? Int32[] : Vector{Int32}(groups)
    groups === nothing || length(g) == N || throw(ArgumentError("groups needs one entry per chain"))
    ng = groups === nothing ? 1 : (isempty(g) ? 0 : Int(maximum(g)) + 1)
    p = Vector{Float64}(probs); nq = length(p)
    count = Vector{Int64}(undef, ng); nch = Vector{Int32}(undef, ng)
    mean = Matrix{Float64}(undef, np, ng); med = Matrix{Float64}(undef, np, ng)
    quant = Array{Float64}(undef, np, ng, nq); cov = Array{Float64}(undef, np, np, ng)
    GC.@preserve g p count nch mean med quant cov begin
        gs = SmmGroupStats(pointer(count), pointer(nch), pointer(mean), pointer(med), nq > 0 ? pointer(quant) : Ptr{Cdouble}(C_NULL),
                           pointer(cov))
        check(h.ctx, ccall(sym(:smm_get_group_stats), Cint,
                           (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Int32}, Cint, Ptr{Cdouble}, Cint, Ref{SmmGroupStats}),
                           h.ctx, t0, t1, accepted_only ? 1 : 0, groups === nothing ? Ptr{Int32}(C_NULL) : pointer(g), ng,
                           nq > 0 ? pointer(p) : Ptr{Cdouble}(C_NULL), nq, gs))
    end
    return (count = count, n_chains = nch, mean = mean, median = med, quantile = quant, cov = cov)   # (the header's row-major arrays)
end

const HIST_SELECT = Dict(:all => 0, :accepted => 1, :state => 2)

"""
    hip_histogram(h, t0, t1; select = :accepted, groups = nothing, bins = 10, range = nothing, pairs = Tuple{Int,Int}[],
                  bins2 = bins) -> NamedTuple

Histograms of the draws of groups of chains over iterations `t0+1 .. t1`, counted on the device (`smm_get_histogram`) without
downloading the history.  `select`: `:all` rows, `:accepted` rows (`params(c)`), or `:state`, the chain's state series (weighted by
holding time).  `groups[chain]` holds 0-based group ids (-1 = none); `nothing`: every chain in one group.  `range`: an `np x 2`
matrix of given outer edges, `nothing`: each group's own min and max.  `pairs`: 1-based parameter indexes `(j, k)` of 2-D histograms.
Returns `count[g]`, `status[k, g]`, `lo[k, g]`, `hi[k, g]`, `edges[:, k, g]`, `hist[:, k, g]` and, with pairs, `edges2[:, k, g]`,
`hist2[k_bin, j_bin, p, g]` (the header's row-major arrays).  Bins follow numpy's `histogram` (the last bin is closed: `x == hi`
counts in it), not `StatsBase.fit(Histogram)`'s right-open bins.
"""
function hip_histogram(h::HipBGP, t0::Integer, t1::Integer; select::Symbol = :accepted,
                       groups::Union{Nothing,AbstractVector{<:Integer}} = nothing, bins::Integer = 10,
                       range::Union{Nothing,AbstractMatrix{<:Real}} = nothing, pairs = Tuple{Int,Int}[], bins2::Integer = bins)
    N, np = h.N, h.np
    g = groups === nothing ? Int32[] : Vector{Int32}(groups)
    groups === nothing || length(g) == N || throw(ArgumentError("groups needs one entry per chain"))
    ng = groups === nothing ? 1 : (isempty(g) ? 0 : Int(maximum(g)) + 1)
    rg = range === nothing ? Float64[] : vec(Matrix{Float64}(permutedims(range)))   # row k = (lo, hi)
    pr = Int32[v - 1 for p in pairs for v in p]
    npr = length(pairs)
    b2 = npr > 0 ? Int(bins2) : 0
    count = Vector{Int64}(undef, ng); st = Matrix{Int32}(undef, np, ng)
    lo = Matrix{Float64}(undef, np, ng); hi = Matrix{Float64}(undef, np, ng)
    edges = Array{Float64}(undef, bins + 1, np, ng); hist = Array{Int64}(undef, bins, np, ng)
    edges2 = Array{Float64}(undef, b2 + 1, np, ng); hist2 = Array{Int64}(undef, b2, b2, npr, ng)
    GC.@preserve g rg pr count st lo hi edges hist edges2 hist2 begin
        hs = SmmHistogram(pointer(count), pointer(st), pointer(lo), pointer(hi), pointer(edges), pointer(hist),
                          npr > 0 ? pointer(edges2) : Ptr{Cdouble}(C_NULL), npr > 0 ? pointer(hist2) : Ptr{Int64}(C_NULL))
        check(h.ctx, ccall(sym(:smm_get_histogram), Cint,
                           (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Int32}, Cint, Cint, Ptr{Cdouble}, Ptr{Int32}, Cint, Cint, Ref{SmmHistogram}),
                           h.ctx, t0, t1, HIST_SELECT[select], groups === nothing ? Ptr{Int32}(C_NULL) : pointer(g), ng, bins,
                           range === nothing ? Ptr{Cdouble}(C_NULL) : pointer(rg), npr > 0 ? pointer(pr) : Ptr{Int32}(C_NULL), npr,
                           max(b2, 1), hs))
    end
    return (count = count, status = st, lo = lo, hi = hi, edges = edges, hist = hist, edges2 = edges2, hist2 = hist2)
end

"""
    hip_profile(h, t0, t1; select = :accepted, groups = nothing, bins = 20, range = nothing, pairs = Tuple{Int,Int}[],
                bins2 = bins, moments = true) -> NamedTuple

The objective and the simulated moments binned along parameters over iterations `t0+1 .. t1`, on the device (`smm_get_profile`)
without downloading the history: per group, parameter and `hip_histogram` bin the rows `n`, the scored rows `n_scored` (finite value),
the smallest value `v_min` with the row that attains it (`min_chain`, `min_iter`, 1-based, 0 = none; `theta_at_min[:, b, k, g]`), the
mean value `v_mean` and, with `moments`, the mean simulated moments `m_mean[:, b, k, g]`; with `pairs` the same over the 2-D cells
(`n2`, `n_scored2`, `v_min2`, `min_chain2`, `min_iter2`, `v_mean2`, each `[k_bin, j_bin, p, g]`).  Arguments as `hip_histogram`.
Arrays are the header's row-major ones.
"""
function hip_profile(h::HipBGP, t0::Integer, t1::Integer; select::Symbol = :accepted,
                     groups::Union{Nothing,AbstractVector{<:Integer}} = nothing, bins::Integer = 20,
                     range::Union{Nothing,AbstractMatrix{<:Real}} = nothing, pairs = Tuple{Int,Int}[], bins2::Integer = bins,
                     moments::Bool = true)
    N, np, nm = h.N, h.np, h.nm
    g = groups === nothing ? Int32[] : Vector{Int32}(groups)
    groups === nothing || length(g) == N || throw(ArgumentError("groups needs one entry per chain"))
    ng = groups === nothing ? 1 : (isempty(g) ? 0 : Int(maximum(g)) + 1)
    rg = range === nothing ? Float64[] : vec(Matrix{Float64}(permutedims(range)))   # row k = (lo, hi)
    pr = Int32[v - 1 for p in pairs for v in p]
    npr = length(pairs)
    b2 = npr > 0 ? Int(bins2) : 0
    count = Vector{Int64}(undef, ng); st = Matrix{Int32}(undef, np, ng); edges = Array{Float64}(undef, bins + 1, np, ng)
    n = Array{Int64}(undef, bins, np, ng); nsc = Array{Int64}(undef, bins, np, ng); vmin = Array{Float64}(undef, bins, np, ng)
    mch = Array{Int32}(undef, bins, np, ng); mit = Array{Int32}(undef, bins, np, ng); theta = Array{Float64}(undef, np, bins, np, ng)
    vmean = Array{Float64}(undef, bins, np, ng); mmean = Array{Float64}(undef, moments ? nm : 0, bins, np, ng)
    edges2 = Array{Float64}(undef, b2 + 1, np, ng); n2 = Array{Int64}(undef, b2, b2, npr, ng); nsc2 = Array{Int64}(undef, b2, b2, npr, ng)
    vmin2 = Array{Float64}(undef, b2, b2, npr, ng); mch2 = Array{Int32}(undef, b2, b2, npr, ng); mit2 = Array{Int32}(undef, b2, b2, npr, ng)
    vmean2 = Array{Float64}(undef, b2, b2, npr, ng)
    two(a, T) = npr > 0 ? pointer(a) : Ptr{T}(C_NULL)
    GC.@preserve g rg pr count st edges n nsc vmin mch mit theta vmean mmean edges2 n2 nsc2 vmin2 mch2 mit2 vmean2 begin
        ps = SmmProfile(pointer(count), pointer(st), pointer(edges), pointer(n), pointer(nsc), pointer(vmin), pointer(mch), pointer(mit),
                        pointer(theta), pointer(vmean), moments ? pointer(mmean) : Ptr{Cdouble}(C_NULL), two(edges2, Cdouble),
                        two(n2, Int64), two(nsc2, Int64), two(vmin2, Cdouble), two(mch2, Int32), two(mit2, Int32), two(vmean2, Cdouble))
        check(h.ctx, ccall(sym(:smm_get_profile), Cint,
                           (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Int32}, Cint, Cint, Ptr{Cdouble}, Ptr{Int32}, Cint, Cint, Ref{SmmProfile}),
                           h.ctx, t0, t1, HIST_SELECT[select], groups === nothing ? Ptr{Int32}(C_NULL) : pointer(g), ng, bins,
                           range === nothing ? Ptr{Cdouble}(C_NULL) : pointer(rg), npr > 0 ? pointer(pr) : Ptr{Int32}(C_NULL), npr,
                           max(b2, 1), ps))
    end
    return (count = count, status = st, edges = edges, n = n, n_scored = nsc, v_min = vmin, min_chain = mch, min_iter = mit,
            theta_at_min = theta, v_mean = vmean, m_mean = mmean, edges2 = edges2, n2 = n2, n_scored2 = nsc2, v_min2 = vmin2,
            min_chain2 = mch2, min_iter2 = mit2, v_mean2 = vmean2)
end

"""
    hip_density(h, t0, t1; select = :accepted, groups = nothing, mass = [0.94], n_grid = 128, range = nothing, bw = nothing) -> NamedTuple

Highest-density intervals, half-sample modes and Gaussian kernel densities of the draws of groups of chains over iterations
`t0+1 .. t1`, on the device (`smm_get_density`) without downloading the history.  `select`, `groups` and `range` as `hip_histogram`;
`mass`: the intervals' masses in (0, 1]; `n_grid`: grid points of the density (0: none); `bw`: a bandwidth per parameter, `nothing`:
R's `bw.nrd0` of each column; `range = nothing`: three bandwidths past each column's extremes.  Returns `count[g]`, `status[k, g]`
(0 ok, 1 a non-finite draw, 2 no draw), `hdi_lo[k, g, p]`, `hdi_hi[k, g, p]`, `mode[k, g]`, `bw[k, g]`, `kde_status[k, g]`,
`grid[:, k, g]`, `density[:, k, g]`, `kde_mode[k, g]` (the header's row-major arrays).
"""
function hip_density(h::HipBGP, t0::Integer, t1::Integer; select::Symbol = :accepted,
                     groups::Union{Nothing,AbstractVector{<:Integer}} = nothing, mass::AbstractVector{<:Real} = [0.94],
                     n_grid::Integer = 128, range::Union{Nothing,AbstractMatrix{<:Real}} = nothing,
                     bw::Union{Nothing,AbstractVector{<:Real}} = nothing)
    N, np = h.N, h.np
    g = groups === nothing ? Int32[] : Vector{Int32}(groups)
    groups === nothing || length(g) == N || throw(ArgumentError("groups needs one entry per chain"))
    ng = groups === nothing ? 1 : (isempty(g) ? 0 : Int(maximum(g)) + 1)
    rg = range === nothing ? Float64[] : vec(Matrix{Float64}(permutedims(range)))   # row k = (lo, hi)
    bv = bw === nothing ? Float64[] : Vector{Float64}(bw)
    bw === nothing || length(bv) == np || throw(ArgumentError("bw needs one entry per parameter"))
    ms = Vector{Float64}(mass)
    nms, ngr = length(ms), Int(n_grid)
    count = Vector{Int64}(undef, ng); st = Matrix{Int32}(undef, np, ng)
    hlo = Array{Float64}(undef, np, ng, nms); hhi = Array{Float64}(undef, np, ng, nms)
    md = Matrix{Float64}(undef, np, ng); obw = Matrix{Float64}(undef, np, ng); kst = Matrix{Int32}(undef, np, ng)
    grid = Array{Float64}(undef, ngr, np, ng); dens = Array{Float64}(undef, ngr, np, ng); kmode = Matrix{Float64}(undef, np, ng)
    opt(a, T, on) = on ? pointer(a) : Ptr{T}(C_NULL)
    GC.@preserve g rg bv ms count st hlo hhi md obw kst grid dens kmode begin
        ds = SmmDensity(pointer(count), pointer(st), opt(hlo, Cdouble, nms > 0), opt(hhi, Cdouble, nms > 0), pointer(md), pointer(obw),
                        pointer(kst), opt(grid, Cdouble, ngr > 0), opt(dens, Cdouble, ngr > 0), opt(kmode, Cdouble, ngr > 0))
        check(h.ctx, ccall(sym(:smm_get_density), Cint,
                           (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Int32}, Cint, Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ref{SmmDensity}),
                           h.ctx, t0, t1, HIST_SELECT[select], groups === nothing ? Ptr{Int32}(C_NULL) : pointer(g), ng,
                           opt(ms, Cdouble, nms > 0), nms, ngr, opt(rg, Cdouble, range !== nothing), opt(bv, Cdouble, bw !== nothing), ds))
    end
    return (count = count, status = st, hdi_lo = hlo, hdi_hi = hhi, mode = md, bw = obw, kde_status = kst, grid = grid, density = dens,
            kde_mode = kmode)
end

"""
    hip_register_transform(src, n_out) -> transform id

A user function of one history row for `hip_derived` (include/smmhip.h): `src` defines
`SMM_USER_TRANSFORM(theta, np, sim_moments, nm, value, mom, w, udata, n_udata, tdata, n_tdata, out, n_out)`, a deterministic function
writing `out[0 .. n_out)` (NaN on entry), `1 <= n_out <= 64`; it may call `smm_exp` and `smm_log`.  Throws with the compiler's log if
the source does not compile.
"""
function hip_register_transform(src::AbstractString, n_out::Integer)
    id = Ref{Int32}(-1)
    rc = ccall(sym(:smm_register_user_transform), Cint, (Cstring, Int32, Ref{Int32}), src, Int32(n_out), id)
    rc == 0 || throw(SMMHipError(Int(rc), last_error(Ptr{Cvoid}(C_NULL))))
    return Int(id[])
end

"""
    hip_derived(h, transform, n_out, t0, t1; select = :accepted, groups = nothing, probs = Float64[], tdata = Float64[]) -> NamedTuple

The posterior of a user function of each draw (Stan's generated quantities) over the pooled rows of groups of chains over iterations
`t0+1 .. t1`, evaluated and summarised on the device (`smm_get_derived`) without downloading the history.  `transform`, `n_out`: the
handle of `hip_register_transform` and its outputs; `select` and `groups` as `hip_histogram`; `tdata`: the vector the function
receives as `tdata`.  Returns `count[g]`, `n_chains[g]`, `n_nonfinite[q, g]`, `mean[q, g]`, `median[q, g]`, `quantile[q, g, p]`,
`cov[q, q2, g]` (the header's row-major arrays).
"""
function hip_derived(h::HipBGP, transform::Integer, n_out::Integer, t0::Integer, t1::Integer; select::Symbol = :accepted,
                     groups::Union{Nothing,AbstractVector{<:Integer}} = nothing, probs::AbstractVector{<:Real} = Float64[],
                     tdata::AbstractVector{<:Real} = Float64[])
    N, Q = h.N, Int(n_out)
    g = groups === nothing ? Int32[] : Vector{Int32}(groups)
    groups === nothing || length(g) == N || throw(ArgumentError("groups needs one entry per chain"))
    ng = groups === nothing ? 1 : (isempty(g) ? 0 : Int(maximum(g)) + 1)
    pr = Vector{Float64}(probs); td = Vector{Float64}(tdata)
    npr, ntd = length(pr), length(td)
    count = Vector{Int64}(undef, ng); nch = Vector{Int32}(undef, ng); nnf = Matrix{Int64}(undef, Q, ng)
    mean = Matrix{Float64}(undef, Q, ng); med = Matrix{Float64}(undef, Q, ng); quant = Array{Float64}(undef, Q, ng, npr)
    cov = Array{Float64}(undef, Q, Q, ng)
    opt(a, T, on) = on ? pointer(a) : Ptr{T}(C_NULL)
    GC.@preserve g pr td count nch nnf mean med quant cov begin
        ds = SmmDerived(pointer(count), pointer(nch), pointer(nnf), pointer(mean), pointer(med), opt(quant, Cdouble, npr > 0), pointer(cov))
        check(h.ctx, ccall(sym(:smm_get_derived), Cint,
                           (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Ptr{Int32}, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cint, Ref{SmmDerived}),
                           h.ctx, transform, t0, t1, HIST_SELECT[select], groups === nothing ? Ptr{Int32}(C_NULL) : pointer(g), ng,
                           opt(td, Cdouble, ntd > 0), ntd, opt(pr, Cdouble, npr > 0), npr, ds))
    end
    return (count = count, n_chains = nch, n_nonfinite = nnf, mean = mean, median = med, quantile = quant, cov = cov)
end

"""
    hip_trace(h, t0, t1; stride = 1, select = :state, moments = false, groups = nothing, probs = Float64[]) -> NamedTuple

The population per iteration over the kept iterations `t0+1, t0+1+stride, .. <= t1`, reduced across the chains of each group on the
device (`smm_get_trace`) without downloading the history.  `select`: `:all` (every member's row itself), `:accepted` (the members
accepted at that iteration) or `:state` (every member's last accepted row).  `groups[chain]` holds 0-based group ids (-1 = none);
`nothing`: every chain in one group.  The `S` series are the parameters, the objective value and, with `moments`, the simulated
moments.  Returns `iter[i]` (0-based), `n_chains[g]`, `count[g, i]`, `n_accepted[g, i]`, `n_exchanged[g, i]`, `n_failed[g, i]`,
`best_value[g, i]`, `best_chain[g, i]` (1-based global id), `mean[s, g, i]`, `var[s, g, i]`, `median[s, g, i]` and
`quantile[s, g, i, p]` (the header's row-major arrays).  NumPy's summation and order statistics (include/smmhip.h).
"""
function hip_trace(h::HipBGP, t0::Integer, t1::Integer; stride::Integer = 1, select::Symbol = :state, moments::Bool = false,
                   groups::Union{Nothing,AbstractVector{<:Integer}} = nothing, probs::AbstractVector{<:Real} = Float64[])
    N = h.N
    S = h.np + 1 + (moments ? h.nm : 0)
    stride >= 1 || throw(ArgumentError("stride must be at least 1"))
    g = groups === nothing ? Int32[] : Vector{Int32}(groups)
    groups === nothing || length(g) == N || throw(ArgumentError("groups needs one entry per chain"))
    ng = groups === nothing ? 1 : (isempty(g) ? 0 : Int(maximum(g)) + 1)
    p = Vector{Float64}(probs); nq = length(p)
    nt = max(0, cld(t1 - t0, stride))
    iter = Vector{Int32}(undef, nt); nch = Vector{Int32}(undef, ng)
    count = Matrix{Int32}(undef, ng, nt); nacc = Matrix{Int32}(undef, ng, nt); nex = Matrix{Int32}(undef, ng, nt)
    nfail = Matrix{Int32}(undef, ng, nt); bestv = Matrix{Float64}(undef, ng, nt); bestc = Matrix{Int32}(undef, ng, nt)
    mean = Array{Float64}(undef, S, ng, nt); var = Array{Float64}(undef, S, ng, nt); med = Array{Float64}(undef, S, ng, nt)
    quant = Array{Float64}(undef, S, ng, nt, nq)
    GC.@preserve g p iter nch count nacc nex nfail bestv bestc mean var med quant begin
        tr = SmmTrace(pointer(iter), pointer(nch), pointer(count), pointer(nacc), pointer(nex), pointer(nfail), pointer(mean), pointer(var),
                      pointer(med), nq > 0 ? pointer(quant) : Ptr{Cdouble}(C_NULL), pointer(bestv), pointer(bestc))
        check(h.ctx, ccall(sym(:smm_get_trace), Cint,
                           (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Cint, Ptr{Int32}, Cint, Ptr{Cdouble}, Cint, Ref{SmmTrace}),
                           h.ctx, t0, t1, stride, HIST_SELECT[select], moments ? 1 : 0, groups === nothing ? Ptr{Int32}(C_NULL) : pointer(g), ng,
                           nq > 0 ? pointer(p) : Ptr{Cdouble}(C_NULL), nq, tr))
    end
    return (iter = iter, n_chains = nch, count = count, n_accepted = nacc, n_exchanged = nex, n_failed = nfail, mean = mean, var = var,
            median = med, quantile = quant, best_value = bestv, best_chain = bestc)
end

"""
    hip_get_draws(h, t0, t1; select = :accepted, groups = nothing, thin = 1, max_rows = 10000, moments = true) -> NamedTuple

The posterior sample itself: thinned draws of groups of chains over iterations `t0+1 .. t1`, gathered on the device (`smm_get_draws`)
without downloading the history.  `select`: `:all`, `:accepted` or `:state` (each chain's last accepted row, looking back before the
window).  Every `thin`-th selected row of a chain is kept; a group with more than `max_rows` kept rows is thinned systematically to
`max_rows`.  `groups[chain]` holds 0-based group ids (-1 = none); `nothing`: every chain in one group.  Returns `count[g]` (kept rows
before the cap), `n_chains[g]`, `row0[g]` (0-based: group g's rows are `row0[g]+1 : row0[g+1]`), `params[k, r]`, `value[r]`,
`sim_moments[k, r]` (empty without `moments`), `chain[r]` (1-based global id), `iter[r]` and `src_iter[r]` (1-based; 0: a state row
that does not exist yet, a NaN row).  A sizing call, then the row call.
"""
function hip_get_draws(h::HipBGP, t0::Integer, t1::Integer; select::Symbol = :accepted,
                       groups::Union{Nothing,AbstractVector{<:Integer}} = nothing, thin::Integer = 1, max_rows::Integer = 10000,
                       moments::Bool = true)
    N = h.N
    g = groups === nothing ? Int32[] : Vector{Int32}(groups)
    groups === nothing || length(g) == N || throw(ArgumentError("groups needs one entry per chain"))
    ng = groups === nothing ? 1 : (isempty(g) ? 0 : Int(maximum(g)) + 1)
    gp = groups === nothing ? Ptr{Int32}(C_NULL) : pointer(g)
    count = Vector{Int64}(undef, ng); nch = Vector{Int32}(undef, ng); row0 = zeros(Int64, ng + 1)
    GC.@preserve g count nch row0 begin
        sz = SmmDraws(pointer(count), pointer(nch), pointer(row0), Ptr{Cdouble}(C_NULL), Ptr{Cdouble}(C_NULL), Ptr{Cdouble}(C_NULL),
                      Ptr{Int32}(C_NULL), Ptr{Int32}(C_NULL), Ptr{Int32}(C_NULL))
        check(h.ctx, ccall(sym(:smm_get_draws), Cint, (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Int32}, Cint, Cint, Cint, Int64, Ref{SmmDraws}),
                           h.ctx, t0, t1, HIST_SELECT[select], gp, ng, thin, max_rows, 0, sz))
    end
    R = Int(row0[ng + 1])
    params = Matrix{Float64}(undef, h.np, R); value = Vector{Float64}(undef, R); mom = Matrix{Float64}(undef, h.nm, moments ? R : 0)
    chain = Vector{Int32}(undef, R); iter = Vector{Int32}(undef, R); src = Vector{Int32}(undef, R)
    GC.@preserve g count nch row0 params value mom chain iter src begin
        dr = SmmDraws(pointer(count), pointer(nch), pointer(row0), pointer(params), pointer(value),
                      moments ? pointer(mom) : Ptr{Cdouble}(C_NULL), pointer(chain), pointer(iter), pointer(src))
        check(h.ctx, ccall(sym(:smm_get_draws), Cint, (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Int32}, Cint, Cint, Cint, Int64, Ref{SmmDraws}),
                           h.ctx, t0, t1, HIST_SELECT[select], gp, ng, thin, max_rows, R, dr))
    end
    return (count = count, n_chains = nch, row0 = row0, params = params, value = value, sim_moments = mom, chain = chain, iter = iter,
            src_iter = src)   # (the header's row-major [R][np] = these column-major [np, R] arrays)
end

"""
    hip_moment_stats(h, t0, t1; select = :state, groups = nothing, probs = Float64[], ridge = 0.0) -> NamedTuple

The simulated moments of groups of chains over iterations `t0+1 .. t1`, on the device (`smm_get_moment_stats`) without downloading the
history: their pooled mean, median and quantiles next to the data moments (`fit_z`), the joint covariance of parameters and moments,
the Jacobian `jac` (the regression of the simulated moments on the parameters over the pooled draws), the sensitivity `sens` of
Andrews, Gentzkow & Shapiro (2017) and the sandwich standard errors `se` (the weights read as the data moments' standard deviations).
`select`: `:all`, `:accepted` or `:state`.  `groups[chain]` holds 0-based group ids (-1 = none); `nothing`: every chain in one group.
Returns `count[g]`, `n_chains[g]`, `status[g]` (0 ok, 1 fewer than 2 rows, 2 a non-finite value, 3 / 4 the parameter covariance /
J'WJ not positive definite), `p_mean[k, g]`, `m_mean[k, g]`, `m_median[k, g]`, `m_quantile[k, g, p]`, `cov_pp[k, j, g]`,
`cov_pm[m, k, g]`, `cov_mm[l, k, g]`, `fit_z[k, g]`, `jac[k, m, g]`, `sens[m, k, g]`, `se[k, g]` (the header's row-major arrays).
"""
function hip_moment_stats(h::HipBGP, t0::Integer, t1::Integer; select::Symbol = :state,
                          groups::Union{Nothing,AbstractVector{<:Integer}} = nothing, probs::AbstractVector{<:Real} = Float64[],
                          ridge::Real = 0.0)
    N, np, nm = h.N, h.np, h.nm
    g = groups === nothing ? Int32[] : Vector{Int32}(groups)
    groups === nothing || length(g) == N || throw(ArgumentError("groups needs one entry per chain"))
    ng = groups === nothing ? 1 : (isempty(g) ? 0 : Int(maximum(g)) + 1)
    p = Vector{Float64}(probs); nq = length(p)
    count = Vector{Int64}(undef, ng); nch = Vector{Int32}(undef, ng); st = Vector{Int32}(undef, ng)
    pmean = Matrix{Float64}(undef, np, ng); mmean = Matrix{Float64}(undef, nm, ng); mmed = Matrix{Float64}(undef, nm, ng)
    mq = Array{Float64}(undef, nm, ng, nq); cpp = Array{Float64}(undef, np, np, ng); cpm = Array{Float64}(undef, nm, np, ng)
    cmm = Array{Float64}(undef, nm, nm, ng); z = Matrix{Float64}(undef, nm, ng); jac = Array{Float64}(undef, np, nm, ng)
    sens = Array{Float64}(undef, nm, np, ng); se = Matrix{Float64}(undef, np, ng)
    GC.@preserve g p count nch st pmean mmean mmed mq cpp cpm cmm z jac sens se begin
        ms = SmmMomentStats(pointer(count), pointer(nch), pointer(st), pointer(pmean), pointer(mmean), pointer(mmed),
                            nq > 0 ? pointer(mq) : Ptr{Cdouble}(C_NULL), pointer(cpp), pointer(cpm), pointer(cmm), pointer(z), pointer(jac),
                            pointer(sens), pointer(se))
        check(h.ctx, ccall(sym(:smm_get_moment_stats), Cint,
                           (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Int32}, Cint, Ptr{Cdouble}, Cint, Cdouble, Ref{SmmMomentStats}),
                           h.ctx, t0, t1, HIST_SELECT[select], groups === nothing ? Ptr{Int32}(C_NULL) : pointer(g), ng,
                           nq > 0 ? pointer(p) : Ptr{Cdouble}(C_NULL), nq, Float64(ridge), ms))
    end
    return (count = count, n_chains = nch, status = st, p_mean = pmean, m_mean = mmean, m_median = mmed, m_quantile = mq, cov_pp = cpp,
            cov_pm = cpm, cov_mm = cmm, fit_z = z, jac = jac, sens = sens, se = se)
end

const ADJUST_KERNEL = Dict(:uniform => 0, :epanechnikov => 1)

"""
    hip_adjustment(h, t0, t1; select = :state, groups = nothing, tol = 0.2, kernel = :epanechnikov, scale = nothing, ridge = 0.0,
                   probs = Float64[]) -> NamedTuple

The regression-adjusted posterior of groups of chains over iterations `t0+1 .. t1`, on the device (`smm_get_adjustment`) without
downloading the history: the local-linear adjustment of Beaumont, Zhang & Balding (2002).  The fraction `tol` of a group's pooled rows
whose simulated moments lie nearest the data moments is kept and weighted by `kernel` (`:uniform` or `:epanechnikov`), the parameters
are regressed on the moment discrepancy `(s - mom) / scale` (`scale = nothing`: the moments' weights), and every kept draw is moved to
zero discrepancy.  `select`: `:all`, `:accepted` or `:state`.  `groups[chain]` holds 0-based group ids (-1 = none); `nothing`: every
chain in one group.  Returns `count[g]`, `n_chains[g]`, `status[g]` (0 ok, 1 fewer than 2 rows, 2 a non-finite value, 3 nothing to
regress on, 4 the moments' weighted covariance not positive definite), `n_kept[g]`, `bandwidth[g]`, `sum_w[g]`, `ess[g]`,
`x_mean[m, g]`, `raw_mean[k, g]`, `beta[k, m, g]`, `adj_mean[k, g]`, `adj_sd[k, g]`, `adj_quantile[k, g, p]` and `n_outside[k, g]`
(the header's row-major arrays).
"""
function hip_adjustment(h::HipBGP, t0::Integer, t1::Integer; select::Symbol = :state,
                        groups::Union{Nothing,AbstractVector{<:Integer}} = nothing, tol::Real = 0.2, kernel::Symbol = :epanechnikov,
                        scale::Union{Nothing,AbstractVector{<:Real}} = nothing, ridge::Real = 0.0,
                        probs::AbstractVector{<:Real} = Float64[])
    N, np, nm = h.N, h.np, h.nm
    g = groups === nothing ? Int32[] : Vector{Int32}(groups)
    groups === nothing || length(g) == N || throw(ArgumentError("groups needs one entry per chain"))
    ng = groups === nothing ? 1 : (isempty(g) ? 0 : Int(maximum(g)) + 1)
    sc = scale === nothing ? Float64[] : Vector{Float64}(scale)
    scale === nothing || length(sc) == nm || throw(ArgumentError("scale needs one entry per moment"))
    p = Vector{Float64}(probs); nq = length(p)
    count = Vector{Int64}(undef, ng); nch = Vector{Int32}(undef, ng); st = Vector{Int32}(undef, ng); kept = Vector{Int64}(undef, ng)
    bw = Vector{Float64}(undef, ng); sw = Vector{Float64}(undef, ng); ess = Vector{Float64}(undef, ng)
    xmean = Matrix{Float64}(undef, nm, ng); rmean = Matrix{Float64}(undef, np, ng); beta = Array{Float64}(undef, np, nm, ng)
    amean = Matrix{Float64}(undef, np, ng); asd = Matrix{Float64}(undef, np, ng); aq = Array{Float64}(undef, np, ng, nq)
    nout = Matrix{Int64}(undef, np, ng)
    GC.@preserve g sc p count nch st kept bw sw ess xmean rmean beta amean asd aq nout begin
        ad = SmmAdjustment(pointer(count), pointer(nch), pointer(st), pointer(kept), pointer(bw), pointer(sw), pointer(ess), pointer(xmean),
                           pointer(rmean), pointer(beta), pointer(amean), pointer(asd), nq > 0 ? pointer(aq) : Ptr{Cdouble}(C_NULL),
                           pointer(nout))
        check(h.ctx, ccall(sym(:smm_get_adjustment), Cint,
                           (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Int32}, Cint, Cdouble, Cint, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Cint,
                            Ref{SmmAdjustment}),
                           h.ctx, t0, t1, HIST_SELECT[select], groups === nothing ? Ptr{Int32}(C_NULL) : pointer(g), ng, Float64(tol),
                           ADJUST_KERNEL[kernel], scale === nothing ? Ptr{Cdouble}(C_NULL) : pointer(sc), Float64(ridge),
                           nq > 0 ? pointer(p) : Ptr{Cdouble}(C_NULL), nq, ad))
    end
    return (count = count, n_chains = nch, status = st, n_kept = kept, bandwidth = bw, sum_w = sw, ess = ess, x_mean = xmean,
            raw_mean = rmean, beta = beta, adj_mean = amean, adj_sd = asd, adj_quantile = aq, n_outside = nout)
end

"""
    hip_reweighted(h, t0, t1; select = :state, groups = nothing, targets = [1.0], probs = Float64[]) -> NamedTuple

The target posterior from every temperature over iterations `t0+1 .. t1`, on the device (`smm_get_reweighted`) without downloading the
history: every scored row of a chain is importance-reweighted from the chain's own `acc_tuner` to each of `targets` (1 to 64 finite
values >= 0), each chain self-normalised, the chains of a group combined by their effective sample sizes.  It assumes that each chain's
state series targets `exp(-acc_tuner * v)`; BGP's exchange moves respect this only approximately.  `select`: `:all`, `:accepted` or
`:state` (the selection the theory is about).  `groups[chain]` holds 0-based group ids (-1 = none); `nothing`: every chain in one
group.  Returns `count[g]`, `n_scored[g]`, `n_chains[g]`, `chain_n[c]`, `status[g, r]` (0 ok, 1 fewer than 2 scored rows, 2 a
non-finite parameter, 3 the weights overflowed), `chain_ess[c, r]`, `chain_logz[c, r]`, `n_kept[g, r]`, `sum_u[g, r]`, `ess[g, r]`,
`mean[k, g, r]`, `cov[k, j, g, r]`, `value_mean[g, r]`, `m_mean[m, g, r]` and `quantile[k, g, r, p]` (the header's row-major arrays).
"""
function hip_reweighted(h::HipBGP, t0::Integer, t1::Integer; select::Symbol = :state,
                        groups::Union{Nothing,AbstractVector{<:Integer}} = nothing, targets::AbstractVector{<:Real} = [1.0],
                        probs::AbstractVector{<:Real} = Float64[])
    N, np, nm = h.N, h.np, h.nm
    g = groups === nothing ? Int32[] : Vector{Int32}(groups)
    groups === nothing || length(g) == N || throw(ArgumentError("groups needs one entry per chain"))
    ng = groups === nothing ? 1 : (isempty(g) ? 0 : Int(maximum(g)) + 1)
    tg = Vector{Float64}(targets); R = length(tg)
    1 <= R <= 64 || throw(ArgumentError("targets needs 1 to 64 entries"))
    p = Vector{Float64}(probs); nq = length(p)
    count = Vector{Int64}(undef, ng); nsc = Vector{Int64}(undef, ng); nch = Vector{Int32}(undef, ng); st = Matrix{Int32}(undef, ng, R)
    cn = Vector{Int32}(undef, N); cess = Matrix{Float64}(undef, N, R); clz = Matrix{Float64}(undef, N, R)
    kept = Matrix{Int64}(undef, ng, R); su = Matrix{Float64}(undef, ng, R); ess = Matrix{Float64}(undef, ng, R)
    mean = Array{Float64}(undef, np, ng, R); cov = Array{Float64}(undef, np, np, ng, R); vm = Matrix{Float64}(undef, ng, R)
    mm = Array{Float64}(undef, nm, ng, R); q = Array{Float64}(undef, np, ng, R, nq)
    GC.@preserve g tg p count nsc nch st cn cess clz kept su ess mean cov vm mm q begin
        rw = SmmReweighted(pointer(count), pointer(nsc), pointer(nch), pointer(st), pointer(cn), pointer(cess), pointer(clz),
                           pointer(kept), pointer(su), pointer(ess), pointer(mean), pointer(cov), pointer(vm), pointer(mm),
                           nq > 0 ? pointer(q) : Ptr{Cdouble}(C_NULL))
        check(h.ctx, ccall(sym(:smm_get_reweighted), Cint,
                           (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Int32}, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cint, Ref{SmmReweighted}),
                           h.ctx, t0, t1, HIST_SELECT[select], groups === nothing ? Ptr{Int32}(C_NULL) : pointer(g), ng, pointer(tg), R,
                           nq > 0 ? pointer(p) : Ptr{Cdouble}(C_NULL), nq, rw))
    end
    return (count = count, n_scored = nsc, n_chains = nch, status = st, chain_n = cn, chain_ess = cess, chain_logz = clz, n_kept = kept,
            sum_u = su, ess = ess, mean = mean, cov = cov, value_mean = vm, m_mean = mm, quantile = q)
end

# the factor(s) between the header's row-major [np][np] / [N][np][np] and Julia's L[k, j] / L[k, j, c]
proposal_length(h::HipBGP) = (h.chol == 2 ? h.N : 1) * h.np * h.np

"""
    hip_get_proposal(h) -> Array

The installed proposal factor(s) (`smm_get_proposal`): `L[k, j]` (shared) or `L[k, j, c]` (per chain, the context's chains).
"""
function hip_get_proposal(h::HipBGP)
    h.chol == 0 && throw(ArgumentError("the context has no proposal factor: create it with chol_L"))
    buf = Vector{Float64}(undef, proposal_length(h))
    GC.@preserve buf check(h.ctx, ccall(sym(:smm_get_proposal), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), h.ctx, pointer(buf)))
    return h.chol == 2 ? permutedims(reshape(buf, h.np, h.np, h.N), (2, 1, 3)) : permutedims(reshape(buf, h.np, h.np), (2, 1))
end

"""
    hip_set_proposal!(h, L)

Install proposal factor(s) between steps (`smm_set_proposal`, the matrix form of `set_sigma!`): `L[k, j]` (shared; the same on
every shard) or `L[k, j, c]` (per chain).  Entries above the diagonal are ignored.
"""
function hip_set_proposal!(h::HipBGP, L::Array{Float64})
    want = h.chol == 2 ? (h.np, h.np, h.N) : (h.np, h.np)
    size(L) == want || throw(ArgumentError("the factor must be $(want)"))
    Lrow = ndims(L) == 3 ? vec(permutedims(L, (2, 1, 3))) : vec(permutedims(L, (2, 1)))
    GC.@preserve Lrow check(h.ctx, ccall(sym(:smm_set_proposal), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), h.ctx, pointer(Lrow)))
    return nothing
end

"""
    hip_adapt_proposal!(h, t0, t1; accepted_only = true, min_draws = np + 1, normalize = true, ridge = 1e-8) -> Vector{Int32}

Every chain's factor from the covariance of its own draws of iterations `t0+1 .. t1` in [0, 1]-space (`smm_adapt_proposal`,
per-chain factors only): the status of each chain — 0 installed, 1 fewer than `min_draws` draws, 2 a non-finite covariance,
3 not positive definite (the chain keeps its factor).
"""
function hip_adapt_proposal!(h::HipBGP, t0::Integer, t1::Integer; accepted_only::Bool = true, min_draws::Integer = h.np + 1,
                             normalize::Bool = true, ridge::Real = 1e-8)
    status = Vector{Int32}(undef, h.N)
    GC.@preserve status check(h.ctx, ccall(sym(:smm_adapt_proposal), Cint, (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Cint, Cdouble, Ptr{Int32}),
                                           h.ctx, t0, t1, accepted_only ? 1 : 0, min_draws, normalize ? 1 : 0, Float64(ridge), pointer(status)))
    return status
end

# the starting population (include/smmhip.h): both calls fill (start [N, np], value [N], pick [N], evaluated)
function population_call(h::HipBGP, call)
    start = Matrix{Float64}(undef, h.N, h.np); value = Vector{Float64}(undef, h.N); pick = Vector{Int32}(undef, h.N)
    evaluated = 0
    GC.@preserve start value pick begin
        out = Ref(SmmPopulation(pointer(start), pointer(value), pointer(pick), 0))
        check(h.ctx, call(out))
        evaluated = Int(out[].evaluated)
    end
    return (start = start, value = value, pick = pick, evaluated = evaluated)
end

"""
    hip_set_population!(h, starts) -> (start, value, pick, evaluated)

Every chain from its own point: `starts[c, k]` (chain, parameter), installed on the device as each chain's completed iteration 1
(`smm_set_population`).  Only on a context that has not stepped; afterwards `hip_iter(h) == 1`.
"""
function hip_set_population!(h::HipBGP, starts::Matrix{Float64})
    size(starts) == (h.N, h.np) || throw(ArgumentError("starts must be (N, np) = $((h.N, h.np))"))
    return GC.@preserve starts population_call(h, out -> ccall(sym(:smm_set_population), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{SmmPopulation}),
                                                                 h.ctx, pointer(starts), out))
end

"""
    hip_scatter_population!(h, M; spread = 1.0, keep_init = true) -> (start, value, pick, evaluated)

Scatter search on the device (`smm_scatter_population`, the role of the reference's sobolsearch.jl): `M` candidates per chain in the box
of width `spread` (in [0, 1]-space) around the initial value, the best valid one installed as the chain's completed iteration 1;
`pick[c] == -1`: chain `c` starts from the initial value.  Only on a context that has not stepped.
"""
function hip_scatter_population!(h::HipBGP, M::Integer; spread::Real = 1.0, keep_init::Bool = true)
    return population_call(h, out -> ccall(sym(:smm_scatter_population), Cint, (Ptr{Cvoid}, Cint, Cdouble, Cint, Ptr{SmmPopulation}),
                                           h.ctx, M, Float64(spread), keep_init ? 1 : 0, out))
end

"""
    hip_opt_slices(h, starts, npoints; tol = 1e-5, update = nothing, max_cycles = 1000)
        -> (best, value, sim_moments, lo, hi, delta, cycle_value, cycles, converged, evaluated)

`K = size(starts, 1)` cyclic coordinate searches on grids of `npoints` values (optSlices, slices.jl:114-242), `starts[s, k]` (search,
parameter), advancing together on the device (`smm_opt_slices`): one evaluation launch per coordinate step for all running searches, 4
bytes read back per cycle.  The chains of the context are not touched.  `update = nothing`: the ranges never shrink.  `best`, `lo`, `hi`
are `(K, np)`, `sim_moments` `(K, nm)`, `cycle_value` `(K, max_cycles)` (NaN past a search's last cycle); `value[s] == Inf` while
search `s` never saw a finite value.
"""
function hip_opt_slices(h::HipBGP, starts::Matrix{Float64}, npoints::Integer; tol::Real = 1e-5, update::Union{Nothing, Real} = nothing,
                        max_cycles::Integer = 1000)
    size(starts, 2) == h.np || throw(ArgumentError("starts must be (K, np) with np = $(h.np)"))
    K = size(starts, 1)
    mc = max(Int(max_cycles), 0)
    best = Matrix{Float64}(undef, K, h.np); lo = similar(best); hi = similar(best)
    value = Vector{Float64}(undef, K); delta = similar(value)
    simm = Matrix{Float64}(undef, K, h.nm); cycle_value = Matrix{Float64}(undef, K, mc)
    cycles = Vector{Int32}(undef, K); converged = Vector{Int32}(undef, K)
    evaluated = 0
    GC.@preserve starts best lo hi value delta simm cycle_value cycles converged begin
        out = Ref(SmmOptSlices(pointer(best), pointer(value), pointer(simm), pointer(lo), pointer(hi), pointer(delta), pointer(cycle_value),
                               pointer(cycles), pointer(converged), 0))
        check(h.ctx, ccall(sym(:smm_opt_slices), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Cint, Cdouble, Cdouble, Cint, Ptr{SmmOptSlices}),
                           h.ctx, pointer(starts), K, npoints, Float64(tol), update === nothing ? NaN : Float64(update), max_cycles, out))
        evaluated = Int(out[].evaluated)
    end
    return (best = best, value = value, sim_moments = simm, lo = lo, hi = hi, delta = delta, cycle_value = cycle_value, cycles = cycles,
            converged = converged .!= 0, evaluated = evaluated)
end

"""
    hip_opt_simplex(h, starts; step = 0.05, adaptive = false, xatol = 1e-4, fatol = 1e-4, max_iter = nothing)
        -> (best, value, sim_moments, simplex, simplex_value, size_x, size_f, iterations, status, moves, n_eval, evaluated)

`K = size(starts, 1)` Nelder–Mead searches inside the parameter box, `starts[s, k]` (search, parameter), advancing together on the device
(`smm_opt_simplex`: scipy's bounded Nelder–Mead made exact; the initial simplex is `step` of each parameter's range wide): three 4-byte
counts read back per iteration.  The chains of the context are not touched.  `max_iter = nothing`: 200 per parameter.  `best` is
`(K, np)`, `sim_moments` `(K, nm)`, `simplex` `(K, np, np + 1)` (search, parameter, vertex), `simplex_value` `(K, np + 1)`, `moves` `(K, 5)`:
iterations that ended in reflection, expansion, outside contraction, inside contraction, shrink; `status[s]`: 1 converged, 0 stopped by
`max_iter`, 2 no finite value at any vertex.
"""
function hip_opt_simplex(h::HipBGP, starts::Matrix{Float64}; step::Real = 0.05, adaptive::Bool = false, xatol::Real = 1e-4, fatol::Real = 1e-4,
                         max_iter::Union{Nothing, Integer} = nothing)
    size(starts, 2) == h.np || throw(ArgumentError("starts must be (K, np) with np = $(h.np)"))
    K = size(starts, 1)
    mi = max_iter === nothing ? 200 * h.np : Int(max_iter)
    best = Matrix{Float64}(undef, K, h.np); simm = Matrix{Float64}(undef, K, h.nm)
    simplex = Array{Float64, 3}(undef, K, h.np, h.np + 1); simplex_value = Matrix{Float64}(undef, K, h.np + 1)
    value = Vector{Float64}(undef, K); size_x = similar(value); size_f = similar(value)
    iterations = Vector{Int32}(undef, K); status = similar(iterations); n_eval = similar(iterations)
    moves = Matrix{Int32}(undef, K, 5)
    evaluated = 0
    GC.@preserve starts best simm simplex simplex_value value size_x size_f iterations status n_eval moves begin
        out = Ref(SmmOptSimplex(pointer(best), pointer(value), pointer(simm), pointer(simplex), pointer(simplex_value), pointer(size_x),
                                pointer(size_f), pointer(iterations), pointer(status), pointer(moves), pointer(n_eval), 0))
        check(h.ctx, ccall(sym(:smm_opt_simplex), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Cdouble, Cint, Cdouble, Cdouble, Cint, Ptr{SmmOptSimplex}),
                           h.ctx, pointer(starts), K, Float64(step), adaptive ? 1 : 0, Float64(xatol), Float64(fatol), mi, out))
        evaluated = Int(out[].evaluated)
    end
    return (best = best, value = value, sim_moments = simm, simplex = simplex, simplex_value = simplex_value, size_x = size_x, size_f = size_f,
            iterations = iterations, status = status, moves = moves, n_eval = n_eval, evaluated = evaluated)
end

"""
    hip_opt_lm(h, starts; fd_step = 1e-4, lambda0 = 1e-3, lambda_up = 10, lambda_down = 10, xtol = 1e-8, ftol = 1e-12, gtol = 0.0,
               max_iter = 100, max_tries = 12)
        -> (best, value, sim_moments, ssr, grad, jac, lambda, step, dF, active, iterations, tries, n_eval, status, evaluated)

`K = size(starts, 1)` Levenberg–Marquardt searches inside the parameter box, `starts[s, k]` (search, parameter), advancing together on the
device (`smm_opt_lm`: least squares on the moments' residuals `(sim - mom) / s` with forward-difference Jacobians, `fd_step` of each
parameter's range wide): one 4-byte count read back per round of tries and one per iteration.  The chains of the context are not touched.
`best` and `grad` are `(K, np)`, `sim_moments` `(K, nm)`, `jac` `(K, np, nm)` (search, parameter, moment), `active` `(K, np)`; `ssr` is
the sum of squared residuals, which the search minimises; `status[s]`: 1 converged, 0 stopped by `max_iter`, 2 a residual or Jacobian
entry not finite, 3 no descent found, 4 a parameter moves no moment.
"""
function hip_opt_lm(h::HipBGP, starts::Matrix{Float64}; fd_step::Real = 1e-4, lambda0::Real = 1e-3, lambda_up::Real = 10, lambda_down::Real = 10,
                    xtol::Real = 1e-8, ftol::Real = 1e-12, gtol::Real = 0.0, max_iter::Integer = 100, max_tries::Integer = 12)
    size(starts, 2) == h.np || throw(ArgumentError("starts must be (K, np) with np = $(h.np)"))
    K = size(starts, 1)
    best = Matrix{Float64}(undef, K, h.np); grad = similar(best); simm = Matrix{Float64}(undef, K, h.nm)
    jac = Array{Float64, 3}(undef, K, h.np, h.nm)
    value = Vector{Float64}(undef, K); ssr = similar(value); lambda = similar(value); step = similar(value); dF = similar(value)
    active = Matrix{Int32}(undef, K, h.np)
    iterations = Vector{Int32}(undef, K); tries = similar(iterations); n_eval = similar(iterations); status = similar(iterations)
    evaluated = 0
    GC.@preserve starts best grad simm jac value ssr lambda step dF active iterations tries n_eval status begin
        out = Ref(SmmOptLM(pointer(best), pointer(value), pointer(simm), pointer(ssr), pointer(grad), pointer(jac), pointer(lambda),
                           pointer(step), pointer(dF), pointer(active), pointer(iterations), pointer(tries), pointer(n_eval), pointer(status), 0))
        check(h.ctx, ccall(sym(:smm_opt_lm), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Cdouble, Cdouble, Cdouble, Cdouble, Cdouble, Cdouble, Cdouble,
                                                    Cint, Cint, Ptr{SmmOptLM}),
                           h.ctx, pointer(starts), K, Float64(fd_step), Float64(lambda0), Float64(lambda_up), Float64(lambda_down), Float64(xtol),
                           Float64(ftol), Float64(gtol), Int(max_iter), Int(max_tries), out))
        evaluated = Int(out[].evaluated)
    end
    return (best = best, value = value, sim_moments = simm, ssr = ssr, grad = grad, jac = jac, lambda = lambda, step = step, dF = dF,
            active = active .!= 0, iterations = iterations, tries = tries, n_eval = n_eval, status = status, evaluated = evaluated)
end

"""
    hip_abc_pmc(h, n_particles, n_keep; max_gen = 20, p_acc_min = 0.05, scale = 2.0, ridge = 0.0, probs = Float64[])
        -> (theta, value, sim_moments, weight, logw, born, eps, p_acc, gen_ess, n_outside, n_invalid, n_underflow, n_new_kept, mean, cov,
            quantile, ess, n_kept, generations, status, evaluated)

Sample without chains: the adaptive population Monte Carlo ABC sampler of Lenormand, Jabot & Deffuant (2013) on the device (`smm_abc_pmc`):
a uniform prior on the box, the objective value as the distance, `n_particles` particles a generation of which the best `n_keep` are kept.
The chains of the context are not touched.  `theta` is `(n_keep, np)`, `sim_moments` `(n_keep, nm)`, rows past `n_kept` NaN; the
per-generation vectors have `max_gen + 1` entries, NaN or -1 past the last generation; `quantile` is `(np, length(probs))`.  `status`: 0
stopped by `max_gen`, 1 `p_acc <= p_acc_min`, 2 fewer than 2 finite particles, 3 kernel covariance not positive definite.
"""
function hip_abc_pmc(h::HipBGP, n_particles::Integer, n_keep::Integer; max_gen::Integer = 20, p_acc_min::Real = 0.05, scale::Real = 2.0,
                     ridge::Real = 0.0, probs::Vector{Float64} = Float64[])
    A = max(Int(n_keep), 0); G1 = max(Int(max_gen), 0) + 1; nq = length(probs)
    theta = Matrix{Float64}(undef, A, h.np); simm = Matrix{Float64}(undef, A, h.nm)
    value = Vector{Float64}(undef, A); weight = similar(value); logw = similar(value); born = Vector{Int32}(undef, A)
    eps = Vector{Float64}(undef, G1); p_acc = similar(eps); gen_ess = similar(eps)
    n_outside = Vector{Int32}(undef, G1); n_invalid = similar(n_outside); n_underflow = similar(n_outside); n_new_kept = similar(n_outside)
    mean = Vector{Float64}(undef, h.np); cov = Matrix{Float64}(undef, h.np, h.np); quantile = Matrix{Float64}(undef, h.np, nq)
    res = nothing
    GC.@preserve probs theta simm value weight logw born eps p_acc gen_ess n_outside n_invalid n_underflow n_new_kept mean cov quantile begin
        out = Ref(SmmAbcPmc(pointer(theta), pointer(value), pointer(simm), pointer(weight), pointer(logw), pointer(born), pointer(eps),
                            pointer(p_acc), pointer(gen_ess), pointer(n_outside), pointer(n_invalid), pointer(n_underflow), pointer(n_new_kept),
                            pointer(mean), pointer(cov), pointer(quantile), 0.0, 0, 0, 0, 0, 0))
        check(h.ctx, ccall(sym(:smm_abc_pmc), Cint, (Ptr{Cvoid}, Cint, Cint, Cint, Cdouble, Cdouble, Cdouble, Ptr{Cdouble}, Cint, Ptr{SmmAbcPmc}),
                           h.ctx, n_particles, n_keep, max_gen, Float64(p_acc_min), Float64(scale), Float64(ridge),
                           nq > 0 ? pointer(probs) : Ptr{Cdouble}(C_NULL), nq, out))
        res = out[]
    end
    return (theta = theta, value = value, sim_moments = simm, weight = weight, logw = logw, born = born, eps = eps, p_acc = p_acc,
            gen_ess = gen_ess, n_outside = n_outside, n_invalid = n_invalid, n_underflow = n_underflow, n_new_kept = n_new_kept, mean = mean,
            cov = cov, quantile = quantile, ess = res.ess, n_kept = Int(res.n_kept), generations = Int(res.generations), status = Int(res.status),
            evaluated = Int(res.evaluated))
end

"""
    hip_sens_sobol(h, n_base; lo = nothing, hi = nothing)
        -> (mean, var, centre, first, total, v_first, v_total, se_first, se_total, n_complete, n_invalid, evaluated)

Identify: variance-based global sensitivity on the device (`smm_sens_sobol`): the Sobol' first-order and total-order indices of the objective
value and of every simulated moment with respect to every parameter, from `n_base * (np + 2)` evaluations over the box `[lo, hi]` (both
`nothing`: the context's bounds).  The chains of the context are not touched.  The tables are `(np, nm + 1)`: column 1 is the value,
column `1 + f` moment `f`; `mean`, `var` and `centre` have `nm + 1` entries.
"""
function hip_sens_sobol(h::HipBGP, n_base::Integer; lo::Union{Nothing,Vector{Float64}} = nothing, hi::Union{Nothing,Vector{Float64}} = nothing)
    F = h.nm + 1
    mean = Vector{Float64}(undef, F); var = similar(mean); centre = similar(mean)
    first = Matrix{Float64}(undef, h.np, F); total = similar(first); v_first = similar(first); v_total = similar(first)
    se_first = similar(first); se_total = similar(first)
    lo === nothing || length(lo) == h.np || error("hip_sens_sobol: lo takes one entry per parameter")
    hi === nothing || length(hi) == h.np || error("hip_sens_sobol: hi takes one entry per parameter")
    res = nothing
    GC.@preserve lo hi mean var centre first total v_first v_total se_first se_total begin
        out = Ref(SmmSensSobol(pointer(mean), pointer(var), pointer(centre), pointer(first), pointer(total), pointer(v_first), pointer(v_total),
                               pointer(se_first), pointer(se_total), 0, 0, 0))
        check(h.ctx, ccall(sym(:smm_sens_sobol), Cint, (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{SmmSensSobol}), h.ctx, n_base,
                           lo === nothing ? Ptr{Cdouble}(C_NULL) : pointer(lo), hi === nothing ? Ptr{Cdouble}(C_NULL) : pointer(hi), out))
        res = out[]
    end
    return (mean = mean, var = var, centre = centre, first = first, total = total, v_first = v_first, v_total = v_total, se_first = se_first,
            se_total = se_total, n_complete = Int(res.n_complete), n_invalid = Int(res.n_invalid), evaluated = Int(res.evaluated))
end

"per-chain state: what `save` / `readMalgo` / `restart!` need besides the history (AlgoAbstract.jl:83-102)"
function hip_state(h::HipBGP)
    N, np, nm = h.N, h.np, h.nm
    sigma = Vector{Float64}(undef, N); rate = similar(sigma); lav = similar(sigma); lap = similar(sigma)
    lapar = Matrix{Float64}(undef, N, np); lasm = Matrix{Float64}(undef, N, nm)
    last = Vector{Int8}(undef, N); nno = Vector{Int32}(undef, N); nac = similar(nno)
    bv = similar(sigma); bi = Vector{Int32}(undef, N)
    it = 0
    GC.@preserve sigma rate lav lap lapar lasm last nno nac bv bi begin
        s = Ref(SmmState(0, 0, pointer(sigma), pointer(rate), pointer(lav), pointer(lap), pointer(lapar), pointer(lasm),
                         pointer(last), pointer(nno), pointer(nac), pointer(bv), pointer(bi)))
        check(h.ctx, ccall(sym(:smm_get_state), Cint, (Ptr{Cvoid}, Ref{SmmState}), h.ctx, s))
        it = Int(s[].iter)
    end
    return (iter = it, sigma = sigma, accept_rate = rate, la_value = lav, la_prob = lap, la_params = lapar,
            la_sim_moments = lasm, la_status = last, n_noex = nno, n_acc_noex = nac, best_val = bv, best_id = bi)
end

"""
    hip_set_state!(h, state, history)

`restart!` (AlgoBGP.jl:804-884) with clean resume semantics: upload a state (as returned by `hip_state`, `iter` completed
iterations) and the history of iterations `1 .. iter` (as returned by `hip_history(h, 0, iter)`); stepping continues at
`iter + 1`.  Also clears a sticky hard error.
"""
function hip_set_state!(h::HipBGP, s::NamedTuple, hist::NamedTuple)
    GC.@preserve s hist begin
        st = SmmState(s.iter, 0, pointer(s.sigma), pointer(s.accept_rate), pointer(s.la_value), pointer(s.la_prob),
                      pointer(s.la_params), pointer(s.la_sim_moments), pointer(s.la_status), pointer(s.n_noex),
                      pointer(s.n_acc_noex), pointer(s.best_val), pointer(s.best_id))
        hs = SmmHistory(pointer(hist.value), pointer(hist.prob), pointer(hist.curr_val), pointer(hist.best_val),
                        pointer(hist.params), pointer(hist.sim_moments), pointer(hist.best_id), pointer(hist.exchanged),
                        pointer(hist.accepted), pointer(hist.status))
        check(h.ctx, ccall(sym(:smm_set_state), Cint, (Ptr{Cvoid}, Ref{SmmState}, Ref{SmmHistory}), h.ctx, st, hs))
    end
    return h
end

"""
    hip_eval_batch(h, params) -> (value, sim_moments, status)

Batched `evaluateObjective(m, p)` (mprob.jl:175-188): `params` is M x np, one row per point (the ABI wants `[np][M]`,
which is this matrix in column-major order).  Serves `doSlices` (slices.jl:153) and `FD_gradient` (econometrics.jl:42).
"""
function hip_eval_batch(h::HipBGP, params::Matrix{Float64})
    M = size(params, 1)
    size(params, 2) == h.np || throw(ArgumentError("params must be M x np"))
    value = Vector{Float64}(undef, M); simm = Matrix{Float64}(undef, M, h.nm); st = Vector{Int8}(undef, M)
    GC.@preserve params value simm st begin
        check(h.ctx, ccall(sym(:smm_eval_batch), Cint,
                           (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int8}),
                           h.ctx, pointer(params), M, pointer(value), pointer(simm), pointer(st)))
    end
    return value, simm, st
end

"""
    hip_eval_batch_noseed(h, params, base_seed) -> (value, sim_moments, status)

The same with `options[:noseed] = true` (ObjExamples.jl:71-75): evaluation i draws its own shocks, keyed by `base_seed + i` —
the repetitions of `getSigma` (econometrics.jl:125-145).
"""
function hip_eval_batch_noseed(h::HipBGP, params::Matrix{Float64}, base_seed::Integer)
    M = size(params, 1)
    size(params, 2) == h.np || throw(ArgumentError("params must be M x np"))
    value = Vector{Float64}(undef, M); simm = Matrix{Float64}(undef, M, h.nm); st = Vector{Int8}(undef, M)
    GC.@preserve params value simm st begin
        check(h.ctx, ccall(sym(:smm_eval_batch_noseed), Cint,
                           (Ptr{Cvoid}, Ptr{Cdouble}, Cint, UInt64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int8}),
                           h.ctx, pointer(params), M, UInt64(base_seed), pointer(value), pointer(simm), pointer(st)))
    end
    return value, simm, st
end

"""
    hip_register_objective(src) -> objective id

Compile a user objective (HIP/C++ text defining `SMM_USER_OBJECTIVE(theta, np, mom, w, nm, udata, n_udata, sim_moments,
value, status)`, see include/smmhip.h) for the device: the counterpart of `addEvalFunc!(m, f)` (mprob.jl:159).
"""
function hip_register_objective(src::AbstractString)
    id = Ref{Int32}(0)
    rc = ccall(sym(:smm_register_user_objective), Cint, (Cstring, Ref{Int32}), src, id)
    rc == 0 || throw(SMMHipError(Int(rc), last_error(Ptr{Cvoid}(C_NULL))))
    return Int(id[])
end

"""
    hip_register_objective_rng(src; n_sums = 0, lanes = 256) -> objective id

A user objective that draws from the library's generator (include/smmhip.h): `n_sums = 0` — `src` defines
`SMM_USER_OBJECTIVE_RNG(theta, np, mom, w, nm, udata, n_udata, rng, sim_moments, value, status)`; `n_sums >= 1` — the map-reduce
form, `SMM_USER_PARTIAL_RNG(theta, np, udata, n_udata, rng, lane, n_lanes, partial)` + `SMM_USER_FINISH(...)` on `lanes` lanes.
The source draws with `smm_normal(rng, i)`, `smm_normal2(rng, j, &z0, &z1)`, `smm_uniform(rng, i)`; such objectives also have
noseed evaluations (`hip_eval_batch_noseed`, `getSigmaHip`).
"""
function hip_register_objective_rng(src::AbstractString; n_sums::Integer = 0, lanes::Integer = 256)
    id = Ref{Int32}(0)
    rc = ccall(sym(:smm_register_user_objective_rng), Cint, (Cstring, Int32, Int32, Ref{Int32}), src, Int32(n_sums), Int32(lanes), id)
    rc == 0 || throw(SMMHipError(Int(rc), last_error(Ptr{Cvoid}(C_NULL))))
    return Int(id[])
end

end # module
