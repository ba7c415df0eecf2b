# SMMHipBackend.jl — the drop-in layer for SMM.jl: the BGP path of floswald/SMM.jl on libsmmhip.so.
#
#     using SMM
#     include("julia/SMMHip.jl"); include("julia/SMMHipBackend.jl"); using .SMMHipBackend
#     MA = MAlgoBGPHip(mprob, opts)        # instead of MAlgoBGP(mprob, opts)          (AlgoBGP.jl:497-539)
#     run!(MA)                              # SMM.run! unchanged: it calls computeNextIteration!(MA) (AlgoAbstract.jl:27-76)
#     summary(MA); history(MA.chains[1]); SMM.params(MA.chains[1]); CI(MA.chains[1])   # the reference's own readers
#     save(MA, "run.jld2"); readMalgo("run.jld2")  # a plain SMM.MAlgoBGP on disk: readable without this layer
#     restart!(MA, 100)                     # more iterations, continuing the same chains
#
# How it stays a drop-in: `MAlgoBGPHip <: SMM.MAlgo` has the fields the reference's generic code touches (`m`, `opts`, `i`,
# `chains`, `anim`, `dist_fun`), and `chains` holds REAL `SMM.BGPChain` objects (built by the reference's own constructor),
# filled from the device history the first time somebody looks at them after a step (`getproperty(algo, :chains)` syncs).
# So `history(c)`, `summary(c)`, `params`, `allAccepted`, `best`, `mean`/`median`/`CI`, the plotting recipes — everything
# the reference defines on `BGPChain` (AlgoBGP.jl:117-206) — runs unmodified on what the GPU computed.
#
# Only the per-iteration work changes: `computeNextIteration!(algo::MAlgoBGPHip)` is one call into the library (proposal,
# objective, accept/reject, set_eval! for all chains and exchangeMoves!, AlgoBGP.jl:589-640) instead of pmap/map over chains.
#
# The objective must be a DEVICE objective: `SMM.objfunc_norm` maps to the built-in one; anything else is given as
# `opts["hip_objective"]` = an id of SMMHip.hip_register_objective(source) (or :banana / :dense / :dense2 — :dense2 is BASELINE config 5 as
# worded, the dense simulation with its 256 x 256 stage —, or the source text itself: registered
# once, with opts["hip_rng"] = true as an objective that draws from the library's stream, SMM_USER_OBJECTIVE_RNG — opts["hip_n_sums"] /
# opts["hip_lanes"] for its map-reduce form), with `opts["hip_ns"]`, `opts["hip_obj_params"]` as needed.  A Julia closure cannot run inside the GPU iteration.
#
# NOT EXECUTED IN THIS REPOSITORY'S CI (no julia binary in the image); see the header of SMMHip.jl for what is checked.
module SMMHipBackend

using SMM
using OrderedCollections: OrderedDict          # (what SMM.jl itself depends on: Project.toml, src/SMM.jl:10)
import SMM: MAlgo, MAlgoBGP, MProb, Eval, BGPChain, Slice, computeNextIteration!, run!, summary, history, save, readMalgo, restart!,
            extendBGPChain!
import Base: getproperty, show
using ..SMMHip

export MAlgoBGPHip, sync_chains!, flush_steps!, chain_stats, chain_diag, rank_diag, posterior_draws, moment_fit, sensitivity, regression_adjust, posterior_tempered, profile_objective, posterior_density, posterior_derived, pooled_summary, chain_histogram, population_trace, adapt_proposal!, scatter_start!, hip_context, serialNormalHip, evaluateObjectivesHip, doSlicesHip, optSlicesHip, optSimplexHip, optLMHip, abcPMCHip, sobolIndicesHip, FD_gradient_hip, getSigmaHip

"""
    MAlgoBGPHip(m::MProb, opts::Dict)

GPU-resident counterpart of `MAlgoBGP(m, opts)` (AlgoBGP.jl:505-537): same `opts` keys (`N`, `maxiter`, `maxtemp`, `sigma`,
`sigma_update_steps`, `sigma_adjust_by`, `smpl_iters`, `min_improve`, `acc_tuners`, `batch_size`, `save_frequency`,
`filename`), plus `seed`, `device`, `chol_L` (general Gaussian proposals) and the `hip_*` keys described above.
"""
mutable struct MAlgoBGPHip <: MAlgo
    m::MProb                      # AlgoBGP.jl:498
    opts::Dict                    # :499
    i::Int                        # :500  iteration (set by run!, AlgoAbstract.jl:42)
    chains::Vector{BGPChain}      # :501  real SMM.BGPChain objects, refreshed from the device on access
    anim::Any                     # :502  (plots of the proposal cloud are not produced by the device path)
    dist_fun::Function            # :503  `-` (:537) or the function of the menu entry chosen (device_dist_fun)
    hip::SMMHip.HipBGP            # the device context
    synced::Int                   # iterations already materialised in `chains`
    stepped::Int                  # iterations enqueued on the device so far (host-side count: asking it needs no device synchronisation)
    deferred::Int                 # single steps of computeNextIteration! counted but not enqueued yet (flush_steps!)
    pnames::Vector{Symbol}        # parameter order on the device = keys(m.params_to_sample)
    mnames::Vector{Symbol}        # moment order on the device = keys(m.moments)
end

# per-chain option vectors as the reference reads them (AlgoBGP.jl:522-523), expanded to exactly N entries
function chain_vector(opts::Dict, key::String, default::Float64, N::Int)
    v = Float64.(get(opts, key, fill(default, N)))
    length(v) >= N || throw(ArgumentError("opts[\"$key\"] needs one entry per chain (N = $N), AlgoBGP.jl:522-523"))
    return v[1:N]
end

# user objectives given as source text in opts["hip_objective"], compiled once per (source, form)
const USER_OBJECTIVES = Dict{Tuple{String,Bool,Int,Int},Cint}()

function register_source(src::AbstractString, opts::Dict)
    rng = Bool(get(opts, "hip_rng", false))             # the _RNG forms: the library's stream (noseed evaluations, getSigmaHip)
    n_sums = Int(get(opts, "hip_n_sums", 0))            # 0: one thread per evaluation; >= 1: the map-reduce form
    lanes = Int(get(opts, "hip_lanes", 256))
    key = (String(src), rng, n_sums, lanes)
    get!(USER_OBJECTIVES, key) do
        rng && return Cint(SMMHip.hip_register_objective_rng(src; n_sums = n_sums, lanes = lanes))
        n_sums == 0 || throw(ArgumentError("the map-reduce form of a source in opts[\"hip_objective\"] needs opts[\"hip_rng\"] = true"))
        return Cint(SMMHip.hip_register_objective(src))
    end
end

function device_objective(m::MProb, opts::Dict)
    if haskey(opts, "hip_objective")
        o = opts["hip_objective"]
        o isa Integer && return Cint(o)
        o isa AbstractString && return register_source(o, opts)
        o == :norm && return SMMHip.OBJ_NORM
        o == :banana && return SMMHip.OBJ_BANANA
        o == :dense && return SMMHip.OBJ_DENSE
        o == :dense2 && return SMMHip.OBJ_DENSE2
        throw(ArgumentError("unknown opts[\"hip_objective\"] = $o"))
    end
    m.objfunc === SMM.objfunc_norm && return SMMHip.OBJ_NORM
    throw(ArgumentError("the objective of this MProb is a Julia function; the GPU iteration needs a device objective: " *
                        "SMM.objfunc_norm, or opts[\"hip_objective\"] = SMMHip.hip_register_objective(source)"))
end

function reference_chains(m::MProb, opts::Dict, N::Int, temps::Vector{Float64}, mi::Vector{Float64}, acc::Vector{Float64})
    # exactly the comprehension of the reference's constructor (AlgoBGP.jl:512-536): every field of BGPChain exists and has
    # the reference's initial value (best_val = Inf, best_id = -1, accepted = false, exchanged = 0, ...)
    return BGPChain[BGPChain(i, opts["maxiter"];
                             m = m,
                             sig = get(opts, "sigma", 0.05) * temps[i],
                             upd = get(opts, "sigma_update_steps", 10),
                             upd_by = get(opts, "sigma_adjust_by", 0.01),
                             smpl_iters = get(opts, "smpl_iters", 1000),
                             min_improve = mi[i],
                             acc_tuner = acc[i],
                             batch_size = get(opts, "batch_size", length(m.params_to_sample))) for i in 1:N]
end

# opts["chol_L"]: nothing, a factor L[k, j] / L[k, j, c], or :identity — one identity factor per chain: the isotropic kernel bit for bit,
# and factors that adapt_proposal! can reshape
chol_opt(L, np::Int, N::Int) = L === :identity ? repeat([Float64(k == j) for k in 1:np, j in 1:np], 1, 1, N) : L

"""
    hip_context(m, opts; N_local, chain_offset, device) -> (hip, N, temps, mi, acc, dist_fun, dist_id, pnames, mnames)

The device context of `MAlgoBGP(m, opts)` (AlgoBGP.jl:505-537): ladder, per-chain vectors, flat problem.  `N_local` / `chain_offset`
make it ONE SHARD of the population `opts["N"]` (julia/SMMHipSharded.jl: one process per GPU); the per-chain vectors stay global.
"""
function hip_context(m::MProb, opts::Dict; N_local::Int = Int(opts["N"]), chain_offset::Int = 0, device::Int = Int(get(opts, "device", 0)))
    N = Int(opts["N"])
    temps = N > 1 ? collect(range(1.0, stop = Float64(opts["maxtemp"]), length = N)) : [1.0]      # AlgoBGP.jl:508
    mi = chain_vector(opts, "min_improve", 0.5, N)                                                  # :522
    acc = chain_vector(opts, "acc_tuners", 2.0, N)                                                  # :523
    dist_fun = get(opts, "hip_dist_fun", get(opts, "dist_fun", -))                                  # :537 (hip_dist_fun: the menu entry of a saved run, as_reference)
    dist_id = device_dist_fun(dist_fun)
    pnames = Symbol[Symbol(k) for k in keys(m.params_to_sample)]
    mnames = Symbol[Symbol(k) for k in keys(m.moments)]
    init = Float64[m.initial_value[k] for k in keys(m.params_to_sample)]
    lb = Float64[v[:lb] for (k, v) in m.params_to_sample]
    ub = Float64[v[:ub] for (k, v) in m.params_to_sample]
    mom = Float64[v[:value] for (k, v) in m.moments]
    w = Float64[v[:weight] for (k, v) in m.moments]
    sigma = get(opts, "sigma", 0.05) .* temps                                                        # :518
    hip = SMMHip.hip_create(init, lb, ub, mom, w, sigma, acc, mi;
                            maxiter = Int(opts["maxiter"]), ns = Int(get(opts, "hip_ns", 10000)),
                            objective_id = device_objective(m, opts),
                            obj_params = Float64.(get(opts, "hip_obj_params", Float64[])),
                            sigma_update_steps = Int(get(opts, "sigma_update_steps", 10)),
                            sigma_adjust_by = Float64(get(opts, "sigma_adjust_by", 0.01)),
                            smpl_iters = Int(get(opts, "smpl_iters", 1000)),
                            batch_size = Int(get(opts, "batch_size", length(init))),
                            seed = Int(get(opts, "seed", 12)), device = device,
                            N = N_local, N_global = N, chain_offset = chain_offset,
                            chol_L = chol_opt(get(opts, "chol_L", nothing), length(init), N), dist_fun = dist_id)
    return hip, N, temps, mi, acc, dist_fun, dist_id, pnames, mnames
end

function MAlgoBGPHip(m::MProb, opts::Dict)
    # opts["animate"] (AlgoBGP.jl:621-624) makes the reference push a plot frame of its chains into algo.anim every iteration:
    # that is a host-side per-iteration hook on objects this backend fills lazily; refused rather than silently ignored
    get(opts, "animate", false) == true &&
        throw(ArgumentError("opts[\"animate\"] is not supported by the GPU backend: run without it and plot the synced chains afterwards"))
    hip, N, temps, mi, acc, dist_fun, dist_id, pnames, mnames = hip_context(m, opts)
    return MAlgoBGPHip(m, opts, 0, reference_chains(m, opts, N, temps, mi, acc), nothing,
                       dist_fun isa Function ? dist_fun : host_dist_fun(dist_id), hip, 0, 0, 0, pnames, mnames)
end

# opts["dist_fun"] (AlgoBGP.jl:494,537) -> smm_dist_fun_t.  The reference takes any function of two objective values; inside the
# exchange kernels only the header's menu runs: `-` (the default), :absdiff (|a - b|), :reldiff ((a - b) / |a|).
function device_dist_fun(f)
    f === (-) && return SMMHip.DIST_MINUS
    f in (:minus, "-", "minus") && return SMMHip.DIST_MINUS
    f in (:absdiff, "absdiff") && return SMMHip.DIST_ABSDIFF
    f in (:reldiff, "reldiff") && return SMMHip.DIST_RELDIFF
    throw(ArgumentError("dist_fun: the device runs `-` (AlgoBGP.jl:537), :absdiff or :reldiff (smm_dist_fun_t), not an arbitrary function"))
end
host_dist_fun(id) = id == SMMHip.DIST_ABSDIFF ? ((a, b) -> abs(a - b)) : id == SMMHip.DIST_RELDIFF ? ((a, b) -> (a - b) / abs(a)) : (-)

# ---- the one method SMM.jl dispatches on (AlgoAbstract.jl:45; README.md:105-107) -------------------------------
"""
    computeNextIteration!(algo::MAlgoBGPHip)

One BGP iteration of all chains on the device: next_eval for every chain (AlgoBGP.jl:272-294) and exchangeMoves!
(:647-716).  `run!` has set `algo.i` (AlgoAbstract.jl:42); a hard error of the reference (negative objective :341, no draw
in support :409) is thrown as `SMMHip.SMMHipError`.
"""
function computeNextIteration!(algo::MAlgoBGPHip)
    # Nothing is enqueued per call, and nobody waits for the device: the reference's unchanged loop (`for i in 1:maxiter ...
    # computeNextIteration!(algo)`, AlgoAbstract.jl:38-45) would otherwise pay a library call and a device synchronisation per
    # iteration and — one iteration at a time — never take the persistent form (include/smmhip.h: steps of n >= 2).  The calls are
    # COUNTED and handed to the library as one asynchronous step when somebody looks (`algo.chains`, `save`, `summary`, ...) or a
    # look-ahead window's worth has come together.  A hard error of the reference (AlgoBGP.jl:341,409) therefore surfaces at that
    # point, naming its iteration, not inside the call of that iteration.
    d = getfield(algo, :deferred) + 1
    setfield!(algo, :deferred, d)
    d >= DEFER_MAX && flush_steps!(algo)
    return nothing
end

const DEFER_MAX = 256            # a look-ahead window of the library

"""
    flush_steps!(algo)

Enqueue the iterations `computeNextIteration!` has counted since the last flush as ONE asynchronous step (no device synchronisation).
"""
function flush_steps!(algo::MAlgoBGPHip)
    d = getfield(algo, :deferred)
    d == 0 && return nothing
    setfield!(algo, :deferred, 0)
    SMMHip.hip_step_async!(getfield(algo, :hip), d)       # (throws before anything is enqueued: a step past maxiter, a failed context)
    setfield!(algo, :stepped, getfield(algo, :stepped) + d)
    return nothing
end

"""
    run!(algo::MAlgoBGPHip)

`SMM.run!` works unchanged (one library call per iteration, with the progress meter).  This method does the same job
without per-iteration host work: all iterations between two save points are enqueued in ONE call (AlgoAbstract.jl:27-76).
"""
function run!(algo::MAlgoBGPHip)
    t0 = time()
    maxiter = Int(algo.opts["maxiter"])
    sf = get(algo.opts, "save_frequency", 0)
    fn = get(algo.opts, "filename", "")
    # (iterations somebody already asked for through computeNextIteration! — enqueued or still counted — are part of the run: `algo.i` alone would
    # step past maxiter when the caller had not advanced it itself, ADVICE r5)
    algo.i = max(algo.i, getfield(algo, :stepped) + getfield(algo, :deferred))
    while algo.i < maxiter
        n = maxiter - algo.i
        if sf > 0 && fn != ""
            n = min(n, sf - (algo.i % sf))
        end
        flush_steps!(algo)
        try
            SMMHip.hip_step!(getfield(algo, :hip), n)
            setfield!(algo, :stepped, getfield(algo, :stepped) + n)
        catch
            # a hard error: the device stands at the failing iteration (include/smmhip.h) — what was completed before it must still
            # reach `algo.chains` (ADVICE r4: the count was only raised behind a successful call)
            setfield!(algo, :stepped, SMMHip.hip_iter(getfield(algo, :hip)))
            rethrow()
        end
        algo.i += n
        if sf > 0 && fn != "" && algo.i % sf == 0
            save(algo, fn)
        end
    end
    algo.opts["time"] = round((time() - t0) / 60, digits = 1)
    if fn != ""
        save(algo, fn)
    end
    return nothing
end

# ---- BGPChain-shaped views --------------------------------------------------------------------------------------
"""
    sync_chains!(algo)

Fill `algo.chains` (real `SMM.BGPChain` objects) with what the device has computed since the last sync: `evals[t]`
(`value`, `params`, `simMoments`, `prob`, `accepted`, `status`), `accepted`, `exchanged`, `best_val`, `best_id`, `curr_val`,
`iter`, `sigma`, `accept_rate` (AlgoBGP.jl:42-110, set_eval! :220-245, set_exchanged! :246-249, set_acceptRate! :253-257).
Called by `getproperty(algo, :chains)`; cheap when nothing new happened.
"""
function sync_chains!(algo::MAlgoBGPHip)
    hip = getfield(algo, :hip)
    chains = getfield(algo, :chains)
    # nothing was stepped since the last sync: the chains are current (no device synchronisation, no download) — `algo.chains` is read
    # by every reader the reference defines, often many times in a row
    flush_steps!(algo)
    getfield(algo, :stepped) == getfield(algo, :synced) && return chains
    try
        SMMHip.hip_sync(hip)          # (the steps were only enqueued; a hard error of the reference is reported here)
    catch
        setfield!(algo, :stepped, SMMHip.hip_iter(hip))    # the failing iteration: everything up to it is materialised by the next read
        rethrow()
    end
    st = SMMHip.hip_state(hip)
    done = st.iter
    first = getfield(algo, :synced)
    # the exchange of iteration t rewrites the records of iteration t (swap_ev_ij!, :734-749) after they were first written:
    # the last synced iteration is downloaded again
    t0 = max(first - 1, 0)
    if done > t0
        h = SMMHip.hip_history(hip, t0, done)
        m = getfield(algo, :m)
        pn, mn = getfield(algo, :pnames), getfield(algo, :mnames)
        for (ci, c) in enumerate(chains)
            for (col, t) in enumerate(t0+1:done)
                ev = Eval(m)                                   # data moments and weights from the MProb (Eval.jl)
                ev.value = h.value[ci, col]
                ev.prob = h.prob[ci, col]
                ev.accepted = h.accepted[ci, col] != 0
                ev.status = Int(h.status[ci, col])
                ev.params = OrderedDict{Symbol,Float64}(pn[k] => h.params[ci, k, col] for k in 1:length(pn))
                ev.simMoments = OrderedDict{Symbol,Float64}(mn[k] => h.sim_moments[ci, k, col] for k in 1:length(mn))
                c.evals[t] = ev
                c.accepted[t] = ev.accepted
                c.exchanged[t] = Int(h.exchanged[ci, col])
                c.best_val[t] = h.best_val[ci, col]
                c.best_id[t] = Int(h.best_id[ci, col])
                c.curr_val[t] = h.curr_val[ci, col]
            end
        end
    end
    for (ci, c) in enumerate(chains)
        c.iter = done
        c.sigma = st.sigma[ci]
        c.accept_rate = st.accept_rate[ci]
    end
    setfield!(algo, :synced, done)
    return chains
end

function getproperty(algo::MAlgoBGPHip, s::Symbol)
    s === :chains && return sync_chains!(algo)
    return getfield(algo, s)
end

"""
    chain_stats(algo; t0 = 0, t1 = nothing, accepted_only = true, probs = Float64[]) -> NamedTuple

Per-chain count, mean, median, quantiles at `probs`, best value and iteration, exchanges and most frequent partner over
iterations `t0+1 .. t1` (default: every completed one), computed on the device from the history it holds — no download, no sync of
the chains (`SMMHip.hip_chain_stats`).  NumPy's summation and quantile rule (include/smmhip.h), so the numbers can differ in the
last bits from `mean`, `median` and `CI` of the synced chains, which stay the reference's (`Statistics`).
"""
function chain_stats(algo::MAlgoBGPHip; t0::Integer = 0, t1 = nothing, accepted_only::Bool = true, probs::Vector{Float64} = Float64[])
    flush_steps!(algo)
    hip = getfield(algo, :hip)
    return SMMHip.hip_chain_stats(hip, t0, t1 === nothing ? SMMHip.hip_iter(hip) : t1; accepted_only = accepted_only, probs = probs)
end

"""
    chain_diag(algo; t0 = 0, t1 = nothing, max_lag = nothing, n_acf = 0, groups = nothing) -> NamedTuple

Per-chain accept rate, autocorrelation, effective sample size (Geyer's initial monotone sequence) and the split R-hat of groups of
chains over iterations `t0+1 .. t1` (default: every completed one), computed on the device from the history it holds
(`SMMHip.hip_chain_diag`).  `max_lag` defaults to `t1 - t0 - 1`; `groups[chain]` holds 0-based group ids (-1 = none).  Not a method
of `SMM`: the reference has no such function.
"""
function chain_diag(algo::MAlgoBGPHip; t0::Integer = 0, t1 = nothing, max_lag = nothing, n_acf::Integer = 0, groups = nothing)
    flush_steps!(algo)
    hip = getfield(algo, :hip)
    t1 = t1 === nothing ? SMMHip.hip_iter(hip) : t1
    return SMMHip.hip_chain_diag(hip, t0, t1; max_lag = max_lag === nothing ? t1 - t0 - 1 : max_lag, n_acf = n_acf, groups = groups)
end

"""
    rank_diag(algo; t0 = 0, t1 = nothing, max_lag = nothing, n_bins = 20, groups = nothing) -> NamedTuple

The rank-normalised split R-hat, the multi-chain bulk, tail and mean ESS and the rank plot of groups of chains over iterations
`t0+1 .. t1` (default: every completed one), computed on the device from the history it holds (`SMMHip.hip_rank_diag`).  `max_lag`
defaults to `(t1 - t0) ÷ 2 - 1`; `groups[chain]` holds 0-based group ids (-1 = none), `nothing`: every chain in one group.  Not a
method of `SMM`: the reference has no such function.
"""
function rank_diag(algo::MAlgoBGPHip; t0::Integer = 0, t1 = nothing, max_lag = nothing, n_bins::Integer = 20, groups = nothing)
    flush_steps!(algo)
    hip = getfield(algo, :hip)
    t1 = t1 === nothing ? SMMHip.hip_iter(hip) : t1
    return SMMHip.hip_rank_diag(hip, t0, t1; max_lag = max_lag === nothing ? (t1 - t0) ÷ 2 - 1 : max_lag, n_bins = n_bins, groups = groups)
end

"""
    pooled_summary(algo; groups = nothing, window = nothing, level = 0.95, accepted_only = true) -> NamedTuple

The posterior of each group's pooled draws, computed on the device from the history it holds (`SMMHip.hip_group_stats`): `count`,
`n_chains`, `mean[k, g]`, `median[k, g]`, `CI[k, g, 1:2]` (the `level` credible interval) and `cov[j, k, g]`.  `groups[chain]` holds
0-based group ids (-1 = none); by default the chains with equal `acc_tuners` entries, numbered in order of first appearance.
`window = (t0, t1)` defaults to every completed iteration.  Not a method of `SMM`: the reference has no such function.
"""
function pooled_summary(algo::MAlgoBGPHip; groups = nothing, window = nothing, level::Real = 0.95, accepted_only::Bool = true)
    flush_steps!(algo)
    hip = getfield(algo, :hip)
    t0, t1 = window === nothing ? (0, SMMHip.hip_iter(hip)) : window
    if groups === nothing   # (MAlgoBGPHip holds every chain of the population: the context's N)
        ids = Dict{Float64,Int32}()
        opts = getfield(algo, :opts)
        groups = [get!(ids, a, Int32(length(ids))) for a in chain_vector(opts, "acc_tuners", 2.0, Int(opts["N"]))]
    end
    q = ((1 - level) / 2, 1 - (1 - level) / 2)
    r = SMMHip.hip_group_stats(hip, t0, t1; accepted_only = accepted_only, groups = groups, probs = collect(Float64, q))
    return (count = r.count, n_chains = r.n_chains, mean = r.mean, median = r.median, CI = r.quantile, cov = r.cov)
end

"""
    chain_histogram(algo; window = nothing, select = :accepted, groups = nothing, bins = 10, range = nothing,
                    pairs = Tuple{Int,Int}[], bins2 = bins) -> NamedTuple

The histograms a plot of the posterior needs, counted on the device from the history it holds (`SMMHip.hip_histogram`), without
`sync_chains!`: per parameter `hist[:, k, g]` over `edges[:, k, g]` and, for each pair `(j, k)` of 1-based parameter indexes,
`hist2[:, :, p, g]` over `edges2`.  `groups[chain]` holds 0-based group ids (-1 = none); by default the chains with equal `acc_tuners`
entries, as `pooled_summary`; `0:N-1` gives one histogram per chain.  Bins follow numpy's rule: equal widths from the group's min to
its max (or the given `range`, an `np x 2` matrix), the last bin closed; this is not `StatsBase.fit(Histogram)`, whose bins are
right-open and whose edges are rounded to nice numbers.  `status[k, g]` != 0 where numpy would raise (a non-finite draw with an
autodetected range, too many bins for the range).  Not a method of `SMM`: the reference plots `params(c)` through its recipe.
"""
function chain_histogram(algo::MAlgoBGPHip; window = nothing, select::Symbol = :accepted, groups = nothing, bins::Integer = 10,
                         range = nothing, pairs = Tuple{Int,Int}[], bins2::Integer = bins)
    flush_steps!(algo)
    hip = getfield(algo, :hip)
    t0, t1 = window === nothing ? (0, SMMHip.hip_iter(hip)) : window
    if groups === nothing
        ids = Dict{Float64,Int32}()
        opts = getfield(algo, :opts)
        groups = [get!(ids, a, Int32(length(ids))) for a in chain_vector(opts, "acc_tuners", 2.0, Int(opts["N"]))]
    end
    return SMMHip.hip_histogram(hip, t0, t1; select = select, groups = groups, bins = bins, range = range, pairs = pairs, bins2 = bins2)
end

"""
    profile_objective(algo; window = nothing, select = :accepted, groups = nothing, bins = 20, range = nothing,
                      pairs = Tuple{Int,Int}[], bins2 = bins, moments = true) -> NamedTuple

What `doSlices` draws, read from the run itself: the objective value and every simulated moment against each parameter, binned on the
device over every row the chains evaluated (`SMMHip.hip_profile`), without `sync_chains!` and without a further evaluation.  Per
group, parameter and bin: `v_min` (the profile, the lower envelope of the value) with `theta_at_min`, `min_chain`, `min_iter`;
`v_mean`; `m_mean`; the counts `n` and `n_scored`; with `pairs` the surface `v_min2` / `v_mean2` over the 2-D cells.  Groups, window,
range and bins as `chain_histogram`.  Not a method of `SMM`: the reference evaluates `np x npoints` new points along the axes.
"""
function profile_objective(algo::MAlgoBGPHip; window = nothing, select::Symbol = :accepted, groups = nothing, bins::Integer = 20,
                           range = nothing, pairs = Tuple{Int,Int}[], bins2::Integer = bins, moments::Bool = true)
    flush_steps!(algo)
    hip = getfield(algo, :hip)
    t0, t1 = window === nothing ? (0, SMMHip.hip_iter(hip)) : window
    if groups === nothing
        ids = Dict{Float64,Int32}()
        opts = getfield(algo, :opts)
        groups = [get!(ids, a, Int32(length(ids))) for a in chain_vector(opts, "acc_tuners", 2.0, Int(opts["N"]))]
    end
    return SMMHip.hip_profile(hip, t0, t1; select = select, groups = groups, bins = bins, range = range, pairs = pairs, bins2 = bins2,
                              moments = moments)
end

"""
    posterior_density(algo; window = nothing, select = :accepted, groups = nothing, mass = [0.94], n_grid = 128, range = nothing,
                      bw = nothing) -> NamedTuple

The intervals, modes and density curves of a posterior report, computed on the device from the history it holds
(`SMMHip.hip_density`), without `sync_chains!`: per group and parameter the highest-density interval of each `mass`
(`hdi_lo[k, g, p]`, `hdi_hi[k, g, p]`: the shortest interval holding that share of the draws, where `CI` and the quantiles are
equal-tailed), the half-sample `mode[k, g]` of the marginal (which `best`, the argmin of the objective, is not), and the Gaussian kernel
density `density[:, k, g]` on `grid[:, k, g]` with its bandwidth `bw[k, g]` (R's `bw.nrd0` unless given) and its highest grid point
`kde_mode[k, g]`.  Groups and window as `chain_histogram`.  `status[k, g]` != 0: a non-finite draw in the column (1) or no draw (2);
`kde_status[k, g]` != 0: no usable bandwidth (1: fewer than two draws) or a grid whose width is not finite (2).  Not a method of `SMM`.
"""
function posterior_density(algo::MAlgoBGPHip; window = nothing, select::Symbol = :accepted, groups = nothing,
                           mass::AbstractVector{<:Real} = [0.94], n_grid::Integer = 128, range = nothing, bw = nothing)
    flush_steps!(algo)
    hip = getfield(algo, :hip)
    t0, t1 = window === nothing ? (0, SMMHip.hip_iter(hip)) : window
    if groups === nothing
        ids = Dict{Float64,Int32}()
        opts = getfield(algo, :opts)
        groups = [get!(ids, a, Int32(length(ids))) for a in chain_vector(opts, "acc_tuners", 2.0, Int(opts["N"]))]
    end
    return SMMHip.hip_density(hip, t0, t1; select = select, groups = groups, mass = mass, n_grid = n_grid, range = range, bw = bw)
end

"""
    posterior_derived(algo, source, n_out; window = nothing, select = :accepted, groups = nothing, probs = [0.025, 0.975],
                      tdata = Float64[]) -> NamedTuple

The posterior of a function of the parameters and the simulated moments (Stan's generated quantities: an elasticity, a ratio of two
parameters, a welfare number, an untargeted statistic), evaluated on every pooled draw and summarised on the device from the history
it holds (`SMMHip.hip_derived`), without `sync_chains!` and without the delta method's linearisation.  `source`: HIP text defining
`SMM_USER_TRANSFORM(theta, np, sim_moments, nm, value, mom, w, udata, n_udata, tdata, n_tdata, out, n_out)` (include/smmhip.h), or the
handle `SMMHip.hip_register_transform` gave for it; `tdata`: the vector it receives as `tdata`.  Per group and output `mean[q, g]`,
`median[q, g]`, `quantile[q, g, p]`, `cov[q, q2, g]` and `n_nonfinite[q, g]`, the rows whose output is NaN or infinite (they are not
dropped).  Groups and window as `chain_histogram`.  Not a method of `SMM`.
"""
function posterior_derived(algo::MAlgoBGPHip, source, n_out::Integer; window = nothing, select::Symbol = :accepted, groups = nothing,
                           probs::AbstractVector{<:Real} = [0.025, 0.975], tdata::AbstractVector{<:Real} = Float64[])
    flush_steps!(algo)
    hip = getfield(algo, :hip)
    t0, t1 = window === nothing ? (0, SMMHip.hip_iter(hip)) : window
    if groups === nothing
        ids = Dict{Float64,Int32}()
        opts = getfield(algo, :opts)
        groups = [get!(ids, a, Int32(length(ids))) for a in chain_vector(opts, "acc_tuners", 2.0, Int(opts["N"]))]
    end
    id = source isa Integer ? Int(source) : SMMHip.hip_register_transform(source, n_out)
    return SMMHip.hip_derived(hip, id, n_out, t0, t1; select = select, groups = groups, probs = probs, tdata = tdata)
end

"""
    population_trace(algo; window = nothing, stride = 1, select = :state, moments = false, groups = nothing,
                     probs = [0.025, 0.5, 0.975]) -> NamedTuple

The trace a convergence plot needs, reduced across the chains of each group on the device from the history it holds
(`SMMHip.hip_trace`), without `sync_chains!`: for every `stride`-th iteration of the window the across-chain `mean[s, g, i]`,
`var[s, g, i]`, `median[s, g, i]` and `quantile[s, g, i, p]` of each parameter, of the objective value and, with `moments`, of each
simulated moment, the members' `n_accepted[g, i]`, `n_exchanged[g, i]` and `n_failed[g, i]`, and `best_value[g, i]` with its
`best_chain[g, i]`.  `groups[chain]` holds 0-based group ids (-1 = none); by default the chains with equal `acc_tuners` entries, as
`pooled_summary`.  `select = :state` follows each chain's current state (its last accepted row), `:all` the rows themselves, as the
reference's chain plot draws them.  Not a method of `SMM`: the reference plots one line per chain through its recipe.
"""
function population_trace(algo::MAlgoBGPHip; window = nothing, stride::Integer = 1, select::Symbol = :state, moments::Bool = false,
                          groups = nothing, probs = [0.025, 0.5, 0.975])
    flush_steps!(algo)
    hip = getfield(algo, :hip)
    t0, t1 = window === nothing ? (0, SMMHip.hip_iter(hip)) : window
    if groups === nothing
        ids = Dict{Float64,Int32}()
        opts = getfield(algo, :opts)
        groups = [get!(ids, a, Int32(length(ids))) for a in chain_vector(opts, "acc_tuners", 2.0, Int(opts["N"]))]
    end
    return SMMHip.hip_trace(hip, t0, t1; stride = stride, select = select, moments = moments, groups = groups, probs = collect(Float64, probs))
end

"""
    posterior_draws(algo; window = nothing, select = :accepted, groups = nothing, thin = 1, max_rows = 10000, moments = false) -> NamedTuple

The posterior sample itself, gathered on the device from the history it holds (`SMMHip.hip_get_draws`), without `sync_chains!`: for
each group of chains every `thin`-th selected draw of its members, thinned systematically to at most `max_rows` rows, with
`params[k, r]`, `value[r]`, `sim_moments[k, r]` (with `moments`), `chain[r]` and `iter[r]`; group g's rows are
`row0[g]+1 : row0[g+1]`.  `groups[chain]` holds 0-based group ids (-1 = none); by default the chains with equal `acc_tuners`
entries, as `pooled_summary`.  What a corner plot, a posterior-predictive check or a DataFrame needs.  Not a method of `SMM`: the
reference reads `params(chain)` of every chain.
"""
function posterior_draws(algo::MAlgoBGPHip; window = nothing, select::Symbol = :accepted, groups = nothing, thin::Integer = 1,
                         max_rows::Integer = 10000, moments::Bool = false)
    flush_steps!(algo)
    hip = getfield(algo, :hip)
    t0, t1 = window === nothing ? (0, SMMHip.hip_iter(hip)) : window
    if groups === nothing
        ids = Dict{Float64,Int32}()
        opts = getfield(algo, :opts)
        groups = [get!(ids, a, Int32(length(ids))) for a in chain_vector(opts, "acc_tuners", 2.0, Int(opts["N"]))]
    end
    return SMMHip.hip_get_draws(hip, t0, t1; select = select, groups = groups, thin = thin, max_rows = max_rows, moments = moments)
end

# the device's moment statistics of algo's groups (by default the chains with equal `acc_tuners` entries, as `pooled_summary`)
function moment_stats(algo::MAlgoBGPHip, window, select::Symbol, groups, probs, ridge)
    flush_steps!(algo)
    hip = getfield(algo, :hip)
    t0, t1 = window === nothing ? (0, SMMHip.hip_iter(hip)) : window
    if groups === nothing
        ids = Dict{Float64,Int32}()
        opts = getfield(algo, :opts)
        groups = [get!(ids, a, Int32(length(ids))) for a in chain_vector(opts, "acc_tuners", 2.0, Int(opts["N"]))]
    end
    return SMMHip.hip_moment_stats(hip, t0, t1; select = select, groups = groups, probs = collect(Float64, probs), ridge = ridge)
end

"""
    moment_fit(algo; window = nothing, select = :state, groups = nothing, level = 0.95) -> NamedTuple

The first table of an SMM paper, computed on the device from the history it holds (`SMMHip.hip_moment_stats`), without
`sync_chains!`: for each group of chains `count[g]`, `n_chains[g]`, `status[g]`, and of the simulated moments over the group's pooled
draws `mean[k, g]`, `median[k, g]`, `band[k, g, 1:2]` (the quantiles at `level`) and `z[k, g]`, the data moment's distance from the
posterior predictive in its standard deviations.  `select = :state`: the chains' state series, the MCMC posterior itself.  Not a
method of `SMM`: the reference has no such table.
"""
function moment_fit(algo::MAlgoBGPHip; window = nothing, select::Symbol = :state, groups = nothing, level::Real = 0.95)
    r = moment_stats(algo, window, select, groups, ((1 - level) / 2, 1 - (1 - level) / 2), 0.0)
    return (count = r.count, n_chains = r.n_chains, status = r.status, mean = r.m_mean, median = r.m_median, band = r.m_quantile, z = r.fit_z)
end

"""
    sensitivity(algo; window = nothing, select = :state, groups = nothing, ridge = 0.0) -> NamedTuple

Identification and standard errors from the pooled draws, on the device (`SMMHip.hip_moment_stats`): `jac[k, m, g]` (dm/dtheta, the
regression of the simulated moments on the parameters), `sens[m, k, g]` (Andrews, Gentzkow & Shapiro 2017), `se[k, g]` (the sandwich
standard errors, the weights read as the data moments' standard deviations) and `status[g]`.  No further evaluation of the objective
and no finite-difference step, unlike `get_stdErrors`.
"""
function sensitivity(algo::MAlgoBGPHip; window = nothing, select::Symbol = :state, groups = nothing, ridge::Real = 0.0)
    r = moment_stats(algo, window, select, groups, Float64[], ridge)
    return (count = r.count, n_chains = r.n_chains, status = r.status, jac = r.jac, sens = r.sens, se = r.se)
end

"""
    regression_adjust(algo; window = nothing, select = :state, groups = nothing, tol = 0.2, kernel = :epanechnikov, scale = nothing,
                      ridge = 0.0, level = 0.95) -> NamedTuple

The posterior at zero tolerance, on the device (`SMMHip.hip_adjustment`): the local-linear regression adjustment of Beaumont, Zhang &
Balding (2002) over each group's pooled draws.  `raw_mean[k, g]` is the weighted (rejection) estimate, `adj_mean[k, g]` and
`adj_sd[k, g]` the adjusted one, `band[k, g, 1:2]` the weighted quantiles of the adjusted draws at `level`, with `n_kept[g]`,
`ess[g]`, `n_outside[k, g]` (adjusted draws that leave the parameter's bounds; nothing is clamped) and `status[g]`.  `scale = :sd`
scales the discrepancy by the moments' pooled standard deviations (`sqrt(diag cov_mm)` of `SMMHip.hip_moment_stats`, which must be
the same for every group: pass one group, or a vector).  Not a method of `SMM`: the reference has no such function.
"""
function regression_adjust(algo::MAlgoBGPHip; window = nothing, select::Symbol = :state, groups = nothing, tol::Real = 0.2,
                           kernel::Symbol = :epanechnikov, scale = nothing, ridge::Real = 0.0, level::Real = 0.95)
    flush_steps!(algo)
    hip = getfield(algo, :hip)
    t0, t1 = window === nothing ? (0, SMMHip.hip_iter(hip)) : window
    if groups === nothing
        ids = Dict{Float64,Int32}()
        opts = getfield(algo, :opts)
        groups = [get!(ids, a, Int32(length(ids))) for a in chain_vector(opts, "acc_tuners", 2.0, Int(opts["N"]))]
    end
    if scale === :sd
        ms = SMMHip.hip_moment_stats(hip, t0, t1; select = select, groups = zeros(Int32, length(groups)))
        scale = [sqrt(ms.cov_mm[k, k, 1]) for k in 1:size(ms.cov_mm, 1)]
    end
    r = SMMHip.hip_adjustment(hip, t0, t1; select = select, groups = groups, tol = tol, kernel = kernel, scale = scale, ridge = ridge,
                              probs = [(1 - level) / 2, 1 - (1 - level) / 2])
    return (count = r.count, n_chains = r.n_chains, status = r.status, n_kept = r.n_kept, ess = r.ess, raw_mean = r.raw_mean,
            adj_mean = r.adj_mean, adj_sd = r.adj_sd, band = r.adj_quantile, n_outside = r.n_outside)
end

"""
    posterior_tempered(algo; target = nothing, window = nothing, select = :state, groups = nothing, level = 0.95) -> NamedTuple

The target posterior from every temperature, on the device (`SMMHip.hip_reweighted`): every chain's draws importance-reweighted from its
own `acc_tuners` entry to `target` (default: the largest entry, the coldest chain's), each chain self-normalised and entering with its
own effective sample size, so the warmer chains' evaluations are not thrown away.  It assumes that each chain's state series targets
`exp(-acc_tuner * v)`; BGP's exchange moves respect this only approximately.  `groups`: 0-based ids per chain (-1 = none), by default
every chain in one group.  Returns `target`, `count[g]`, `n_scored[g]`, `n_chains[g]`, `status[g]`, `n_kept[g]`, `ess[g]`,
`mean[k, g]`, `cov[k, j, g]`, `value_mean[g]`, `m_mean[m, g]`, `band[k, g, 1:2]` (the weighted quantiles at `level`), `chain_ess[c]`
and `chain_logz[c]`.  Not a method of `SMM`: the reference has no such function.
"""
function posterior_tempered(algo::MAlgoBGPHip; target = nothing, window = nothing, select::Symbol = :state, groups = nothing,
                            level::Real = 0.95)
    flush_steps!(algo)
    hip = getfield(algo, :hip)
    t0, t1 = window === nothing ? (0, SMMHip.hip_iter(hip)) : window
    opts = getfield(algo, :opts)
    a = target === nothing ? maximum(chain_vector(opts, "acc_tuners", 2.0, Int(opts["N"]))) : Float64(target)
    r = SMMHip.hip_reweighted(hip, t0, t1; select = select, groups = groups, targets = [a],
                              probs = [(1 - level) / 2, 1 - (1 - level) / 2])
    return (target = a, count = r.count, n_scored = r.n_scored, n_chains = r.n_chains, status = r.status[:, 1], n_kept = r.n_kept[:, 1],
            ess = r.ess[:, 1], mean = r.mean[:, :, 1], cov = r.cov[:, :, :, 1], value_mean = r.value_mean[:, 1], m_mean = r.m_mean[:, :, 1],
            band = r.quantile[:, :, 1, :], chain_ess = r.chain_ess[:, 1], chain_logz = r.chain_logz[:, 1])
end

"""
    adapt_proposal!(algo; t0 = 0, t1 = nothing, accepted_only = true, min_draws = np + 1, normalize = true, ridge = 1e-8)

Adaptive Metropolis between runs: each chain's proposal factor from the covariance of its own draws of iterations `t0+1 .. t1`
(default: every completed one), computed and installed on the device (`SMMHip.hip_adapt_proposal!`).  Needs per-chain factors
(`opts["chol_L"] = :identity` or `L[k, j, c]`).  Returns the per-chain status (0 installed).  Not a method of `SMM`: the reference
has no such function.
"""
function adapt_proposal!(algo::MAlgoBGPHip; t0::Integer = 0, t1 = nothing, accepted_only::Bool = true, min_draws = nothing,
                         normalize::Bool = true, ridge::Real = 1e-8)
    flush_steps!(algo)
    hip = getfield(algo, :hip)
    return SMMHip.hip_adapt_proposal!(hip, t0, t1 === nothing ? SMMHip.hip_iter(hip) : t1; accepted_only = accepted_only,
                                      min_draws = min_draws === nothing ? hip.np + 1 : min_draws, normalize = normalize, ridge = ridge)
end

"""
    scatter_start!(algo; M = 64, spread = 1.0, keep_init = true) -> (start, value, pick, evaluated)

Scatter search for every chain's start on the device (`SMMHip.hip_scatter_population!`; the role of the reference's sobolsearch.jl):
only on an algorithm that has not stepped.  Afterwards `algo.i == 1` and the chains hold their first iteration, as after one
`computeNextIteration!`.  Not a method of `SMM`: the reference starts every chain at the initial value.
"""
function scatter_start!(algo::MAlgoBGPHip; M::Integer = 64, spread::Real = 1.0, keep_init::Bool = true)
    (getfield(algo, :stepped) == 0 && getfield(algo, :deferred) == 0) || error("scatter_start!: the algorithm has stepped already")
    r = SMMHip.hip_scatter_population!(getfield(algo, :hip), M; spread = spread, keep_init = keep_init)
    setfield!(algo, :stepped, 1)
    setfield!(algo, :i, 1)
    return r
end

"`summary(m::MAlgoBGP)` (AlgoBGP.jl:541-550) on the synced chains"
summary(algo::MAlgoBGPHip) = vcat([summary(c) for c in algo.chains]...)

function show(io::IO, algo::MAlgoBGPHip)
    print(io, "\nBGP Algorithm with $(length(getfield(algo, :chains))) chains on libsmmhip (MI355X)\n")
    print(io, "============================\n\n")
    print(io, "Algorithm\n---------\n")
    print(io, "Current iteration: $(algo.i)\n")
    print(io, "Number of params to estimate: $(length(algo.m.params_to_sample))\n")
    print(io, "Number of moments to match: $(length(algo.m.moments))\n\n")
end

# ---- save / readMalgo / restart! --------------------------------------------------------------------------------
"""
    as_reference(algo::MAlgoBGPHip) -> SMM.MAlgoBGP

The run as a plain `SMM.MAlgoBGP` (same MProb, opts, iteration and the synced chains): what is written to disk, so that a
file saved from the GPU path is read by the reference's own `readMalgo` (AlgoAbstract.jl:95-102) on any machine.
"""
function as_reference(algo::MAlgoBGPHip)
    # the reference stores opts["dist_fun"] in a field typed ::Function (AlgoBGP.jl:503,537): a menu entry (:absdiff, "reldiff", ...)
    # would throw there, so the plain algo gets the host function and the menu entry moves to "hip_dist_fun" (read back on resume)
    opts = copy(algo.opts)
    if haskey(opts, "dist_fun") && !(opts["dist_fun"] isa Function)
        opts["hip_dist_fun"] = opts["dist_fun"]
        opts["dist_fun"] = getfield(algo, :dist_fun)
    end
    ref = MAlgoBGP(algo.m, opts)
    ref.chains = algo.chains
    ref.i = algo.i
    return ref
end

"`save(algo, filename)` (AlgoAbstract.jl:83-88): JLD2 file holding an `SMM.MAlgoBGP` named `algo`"
save(algo::MAlgoBGPHip, filename::AbstractString) = save(as_reference(algo), filename)

# number of iterations a chain counts towards its accept rate / how many of them accepted (set_acceptRate!, :253-257)
noex_counts(c::BGPChain) = (count(c.exchanged[1:c.iter] .== 0), count(c.accepted[1:c.iter] .& (c.exchanged[1:c.iter] .== 0)))

"""
    MAlgoBGPHip(ref::MAlgoBGP; extra_iter = 0)

Continue a run of the reference (for example one read back by `readMalgo`) on the GPU: a device context with
`maxiter + extra_iter` iterations of history, loaded with the chains' state after iteration `ref.i`.
"""
function MAlgoBGPHip(ref::MAlgoBGP; extra_iter::Int = 0)
    opts = copy(ref.opts)
    done = ref.chains[1].iter
    opts["maxiter"] = Int(ref.opts["maxiter"]) + extra_iter
    algo = MAlgoBGPHip(ref.m, opts)
    hip = getfield(algo, :hip)
    N, np, nm = hip.N, hip.np, hip.nm
    pn, mn = getfield(algo, :pnames), getfield(algo, :mnames)
    if done > 0
        value = Matrix{Float64}(undef, N, done); prob = similar(value); curr = similar(value); best = similar(value)
        pars = Array{Float64}(undef, N, np, done); simm = fill(NaN, N, nm, done)
        bid = Matrix{Int32}(undef, N, done); exch = similar(bid); accd = Matrix{UInt8}(undef, N, done); stt = Matrix{Int8}(undef, N, done)
        sigma = Vector{Float64}(undef, N); rate = similar(sigma); lav = similar(sigma); lap = similar(sigma)
        lapar = Matrix{Float64}(undef, N, np); lasm = fill(NaN, N, nm); last = Vector{Int8}(undef, N)
        nno = Vector{Int32}(undef, N); nac = similar(nno); bv = similar(sigma); bi = Vector{Int32}(undef, N)
        for (ci, c) in enumerate(ref.chains)
            for t in 1:done
                ev = c.evals[t]
                value[ci, t] = ev.value; prob[ci, t] = ev.prob; curr[ci, t] = c.curr_val[t]; best[ci, t] = c.best_val[t]
                bid[ci, t] = c.best_id[t]; exch[ci, t] = c.exchanged[t]; accd[ci, t] = c.accepted[t] ? 1 : 0; stt[ci, t] = ev.status
                for k in 1:np
                    pars[ci, k, t] = ev.params[pn[k]]
                end
                for k in 1:nm
                    simm[ci, k, t] = get(ev.simMoments, mn[k], NaN)
                end
            end
            la = SMM.getLastAccepted(c)                       # AlgoBGP.jl:209-217
            sigma[ci] = c.sigma; rate[ci] = c.accept_rate
            lav[ci] = la.value; lap[ci] = la.prob; last[ci] = la.status
            for k in 1:np
                lapar[ci, k] = la.params[pn[k]]
            end
            for k in 1:nm
                lasm[ci, k] = get(la.simMoments, mn[k], NaN)
            end
            nno[ci], nac[ci] = noex_counts(c)
            bv[ci] = c.best_val[done]; bi[ci] = c.best_id[done]
        end
        s = (iter = done, sigma = sigma, accept_rate = rate, la_value = lav, la_prob = lap, la_params = lapar,
             la_sim_moments = lasm, la_status = last, n_noex = nno, n_acc_noex = nac, best_val = bv, best_id = bi)
        h = (value = value, prob = prob, curr_val = curr, best_val = best, params = pars, sim_moments = simm,
             best_id = bid, exchanged = exch, accepted = accd, status = stt)
        SMMHip.hip_set_state!(hip, s, h)
    end
    setfield!(algo, :stepped, done)
    algo.i = done
    return algo
end

"""
    restart!(algo::MAlgoBGPHip, extraIter)

`restart!(algo, extraIter)` (AlgoBGP.jl:804-884): `extraIter` more iterations of the same chains.  The reference re-runs
iteration `algo.i` after extending (its loop starts at the old `maxiter`); here stepping continues at `algo.i + 1`.
"""
function restart!(algo::MAlgoBGPHip, extraIter::Int)
    ext = MAlgoBGPHip(as_reference(algo); extra_iter = extraIter)     # a new device context: the history capacity is fixed at creation
    SMMHip.hip_destroy!(getfield(algo, :hip))
    setfield!(algo, :hip, getfield(ext, :hip))                        # `algo` stays the object the caller holds, as in the reference
    setfield!(algo, :chains, getfield(ext, :chains))
    setfield!(algo, :opts, getfield(ext, :opts))
    setfield!(algo, :synced, 0)
    setfield!(algo, :stepped, getfield(ext, :stepped))
    setfield!(algo, :deferred, 0)
    run!(algo)
    return nothing
end

# ---- Examples.jl:118-153 ------------------------------------------------------------------------------------------
"`SMM.serialNormal(npars, niter)` on the device (2 parameters / 2 moments, 3 chains)"
function serialNormalHip(niter::Int = 200; nchains::Int = 3, acc_tuners = [20.0, 2.0, 1.0])
    pb = OrderedDict("p1" => [0.2, -3, 3], "p2" => [-0.2, -20, 20])
    moms = SMM.DataFrame(name = ["mu1", "mu2"], value = [-1.0, 10.0], weight = ones(2))
    mprob = MProb()
    SMM.addSampledParam!(mprob, pb)
    SMM.addMoment!(mprob, moms)
    SMM.addEvalFunc!(mprob, SMM.objfunc_norm)
    opts = Dict("N" => nchains, "maxiter" => niter, "maxtemp" => 5, "coverage" => 0.02, "smpl_iters" => 1000,
                "parallel" => false, "min_improve" => zeros(nchains), "acc_tuners" => Float64.(acc_tuners), "animate" => false)
    MA = MAlgoBGPHip(mprob, opts)
    run!(MA)
    return MA
end

# ------------------------------------------------------------------------------------------
# The other callers of evaluateObjective (slices.jl, econometrics.jl), as batches on the device: where the reference maps
# evaluateObjective over a grid (pmap / map), the whole grid is ONE call of smm_eval_batch.  (smm.jl_amd/callers.py is the
# tested mirror of the same drivers, tests/test_callers.py.)
# ------------------------------------------------------------------------------------------
"a one-chain context that only evaluates: `opts` as for MAlgoBGPHip (hip_objective, hip_ns, hip_obj_params, device)"
function eval_context(m::MProb, opts::Dict = Dict())
    init = Float64[m.initial_value[k] for k in keys(m.params_to_sample)]
    lb = Float64[v[:lb] for (k, v) in m.params_to_sample]
    ub = Float64[v[:ub] for (k, v) in m.params_to_sample]
    mom = Float64[v[:value] for (k, v) in m.moments]
    w = Float64[v[:weight] for (k, v) in m.moments]
    return SMMHip.hip_create(init, lb, ub, mom, w, [0.05], [1.0], [0.0]; maxiter = 1, ns = Int(get(opts, "hip_ns", 10000)),
                             objective_id = device_objective(m, opts), obj_params = Float64.(get(opts, "hip_obj_params", Float64[])),
                             device = Int(get(opts, "device", 0)))
end

"""
    evaluateObjectivesHip(m, ps; opts = Dict(), noseed_base = nothing) -> Vector{Eval}

`evaluateObjective(m, p)` (mprob.jl:175-205) for every parameter dict of `ps`, as one batch on the device.
"""
function evaluateObjectivesHip(m::MProb, ps::Vector; opts::Dict = Dict(), noseed_base = nothing)
    h = eval_context(m, opts)
    pk = collect(keys(m.params_to_sample))
    mk = collect(keys(m.moments))
    P = Float64[p[k] for p in ps, k in pk]                      # M x np
    value, simm, st = noseed_base === nothing ? SMMHip.hip_eval_batch(h, P) : SMMHip.hip_eval_batch_noseed(h, P, noseed_base)
    SMMHip.hip_destroy!(h)
    evs = Eval[]
    for (i, p) in enumerate(ps)
        ev = Eval(m, p)
        ev.value = value[i]
        ev.status = Int(st[i])
        for (j, k) in enumerate(mk)
            ev.simMoments[k] = simm[i, j]
        end
        push!(evs, ev)
    end
    return evs
end

"`doSlices(m, npoints)` (slices.jl:250-290): all np * npoints evaluations in one batch"
function doSlicesHip(m::MProb, npoints::Int; opts::Dict = Dict())
    res = Slice(m.initial_value, m.moments)
    ps = Any[]
    tags = Symbol[]
    for (pp, bb) in m.params_to_sample
        for pval in range(bb[:lb], stop = bb[:ub], length = npoints)
            p = deepcopy(m.initial_value)
            p[pp] = pval
            push!(ps, p)
            push!(tags, pp)
        end
    end
    for (pp, ev) in zip(tags, evaluateObjectivesHip(m, ps; opts = opts))
        SMM.add!(res, pp, ev)
    end
    return res
end

"""
    optSlicesHip(m, npoints; starts = nothing, tol = 1e-5, update = nothing, max_cycles = 1000, opts = Dict()) -> Vector{Dict}

`optSlices(m, npoints)` (slices.jl:114-242) from many starts, the whole search on the device (`SMMHip.hip_opt_slices`): the searches advance
together, one evaluation launch per coordinate step, 4 bytes read back per cycle.  `starts`: a vector of parameter dicts (`nothing`: the
initial value).  Per start the reference's `Dict(:best => Dict(:p => ..., :value => ...), :iterations => n, :converged => Bool)`; a start
that never saw a finite value keeps its point and has value `Inf`.  (No `:history`: the evaluations never visit the host.)
"""
function optSlicesHip(m::MProb, npoints::Int; starts = nothing, tol::Real = 1e-5, update = nothing, max_cycles::Int = 1000, opts::Dict = Dict())
    ps = starts === nothing ? Any[m.initial_value] : starts
    pk = collect(keys(m.params_to_sample))
    P = Float64[p[k] for p in ps, k in pk]                      # K x np
    h = eval_context(m, opts)
    r = SMMHip.hip_opt_slices(h, P, npoints; tol = tol, update = update, max_cycles = max_cycles)
    SMMHip.hip_destroy!(h)
    out = Dict[]
    for (s, p0) in enumerate(ps)
        p = deepcopy(p0)
        for (j, k) in enumerate(pk)
            p[k] = r.best[s, j]
        end
        push!(out, Dict(:best => Dict(:p => p, :value => r.value[s]), :iterations => Int(r.cycles[s]), :converged => r.converged[s]))
    end
    return out
end

"""
    optSimplexHip(m; starts = nothing, step = 0.05, adaptive = false, xatol = 1e-4, fatol = 1e-4, max_iter = nothing, opts = Dict()) -> Vector{Dict}

Nelder–Mead inside the parameter box from many starts, the whole search on the device (`SMMHip.hip_opt_simplex`): for valleys that do not
run along the axes, which `optSlicesHip` cannot follow.  `starts`: a vector of parameter dicts (`nothing`: the initial value).  Per start
`Dict(:best => Dict(:p => ..., :value => ...), :iterations => n, :converged => Bool, :status => 0 | 1 | 2, :n_eval => n, :moves => [5])`;
status 2: no vertex of the simplex had a finite value.
"""
function optSimplexHip(m::MProb; starts = nothing, step::Real = 0.05, adaptive::Bool = false, xatol::Real = 1e-4, fatol::Real = 1e-4,
                       max_iter = nothing, opts::Dict = Dict())
    ps = starts === nothing ? Any[m.initial_value] : starts
    pk = collect(keys(m.params_to_sample))
    P = Float64[p[k] for p in ps, k in pk]                      # K x np
    h = eval_context(m, opts)
    r = SMMHip.hip_opt_simplex(h, P; step = step, adaptive = adaptive, xatol = xatol, fatol = fatol, max_iter = max_iter)
    SMMHip.hip_destroy!(h)
    out = Dict[]
    for (s, p0) in enumerate(ps)
        p = deepcopy(p0)
        for (j, k) in enumerate(pk)
            p[k] = r.best[s, j]
        end
        push!(out, Dict(:best => Dict(:p => p, :value => r.value[s]), :iterations => Int(r.iterations[s]), :converged => r.status[s] == 1,
                        :status => Int(r.status[s]), :n_eval => Int(r.n_eval[s]), :moves => Int.(r.moves[s, :])))
    end
    return out
end

"""
    optLMHip(m; starts = nothing, fd_step = 1e-4, lambda0 = 1e-3, lambda_up = 10, lambda_down = 10, xtol = 1e-8, ftol = 1e-12, gtol = 0.0,
             max_iter = 100, max_tries = 12, opts = Dict()) -> Vector{Dict}

Levenberg–Marquardt inside the parameter box from many starts, the whole search on the device (`SMMHip.hip_opt_lm`): least squares on the
moments' residuals, the one optimiser here that follows the gradient of the moments.  `starts`: a vector of parameter dicts (`nothing`:
the initial value).  Per start `Dict(:best => Dict(:p => ..., :value => ...), :iterations => n, :converged => Bool, :status => 0 .. 4,
:n_eval => n, :tries => n, :ssr => F, :lambda => lambda)`; status 3: no descent found (at a minimum, the normal ending); 4: a parameter
moves no moment.
"""
function optLMHip(m::MProb; starts = nothing, fd_step::Real = 1e-4, lambda0::Real = 1e-3, lambda_up::Real = 10, lambda_down::Real = 10,
                  xtol::Real = 1e-8, ftol::Real = 1e-12, gtol::Real = 0.0, max_iter::Integer = 100, max_tries::Integer = 12, opts::Dict = Dict())
    ps = starts === nothing ? Any[m.initial_value] : starts
    pk = collect(keys(m.params_to_sample))
    P = Float64[p[k] for p in ps, k in pk]                      # K x np
    h = eval_context(m, opts)
    r = SMMHip.hip_opt_lm(h, P; fd_step = fd_step, lambda0 = lambda0, lambda_up = lambda_up, lambda_down = lambda_down, xtol = xtol, ftol = ftol,
                          gtol = gtol, max_iter = max_iter, max_tries = max_tries)
    SMMHip.hip_destroy!(h)
    out = Dict[]
    for (s, p0) in enumerate(ps)
        p = deepcopy(p0)
        for (j, k) in enumerate(pk)
            p[k] = r.best[s, j]
        end
        push!(out, Dict(:best => Dict(:p => p, :value => r.value[s]), :iterations => Int(r.iterations[s]), :converged => r.status[s] == 1,
                        :status => Int(r.status[s]), :n_eval => Int(r.n_eval[s]), :tries => Int(r.tries[s]), :ssr => r.ssr[s],
                        :lambda => r.lambda[s]))
    end
    return out
end

"""
    abcPMCHip(m, n_particles; keep = 0.5, max_gen = 20, p_acc_min = 0.05, scale = 2.0, ridge = 0.0, probs = [0.025, 0.5, 0.975], opts = Dict()) -> Dict

Sample without chains (`SMMHip.hip_abc_pmc`): the population Monte Carlo ABC sampler over the box of `m` with its objective value as the
distance; `keep`: the kept fraction of the particles (or, `>= 2`, their number).  `Dict(:mean => Dict(name => value), :cov => Matrix,
:quantile => Dict(name => [per prob]), :draws => (theta (n_kept, np), weight), :eps, :p_acc, :status, :ess, :generations, :evaluated)`.
"""
function abcPMCHip(m::MProb, n_particles::Integer; keep::Real = 0.5, max_gen::Integer = 20, p_acc_min::Real = 0.05, scale::Real = 2.0,
                   ridge::Real = 0.0, probs::Vector{Float64} = [0.025, 0.5, 0.975], opts::Dict = Dict())
    A = keep >= 2 ? Int(keep) : Int(floor(keep * n_particles))
    pk = collect(keys(m.params_to_sample))
    h = eval_context(m, opts)
    r = SMMHip.hip_abc_pmc(h, n_particles, A; max_gen = max_gen, p_acc_min = p_acc_min, scale = scale, ridge = ridge, probs = probs)
    SMMHip.hip_destroy!(h)
    n, g = r.n_kept, r.generations
    return Dict(:mean => Dict(k => r.mean[j] for (j, k) in enumerate(pk)), :cov => r.cov,
                :quantile => Dict(k => r.quantile[j, :] for (j, k) in enumerate(pk)), :draws => (r.theta[1:n, :], r.weight[1:n]),
                :eps => r.eps[1:g + 1], :p_acc => r.p_acc[1:g + 1], :status => r.status, :ess => r.ess, :generations => g, :evaluated => r.evaluated)
end

"""
    sobolIndicesHip(m, n_base = 4096; box = nothing, opts = Dict()) -> Dict

Identify (`SMMHip.hip_sens_sobol`): the Sobol' first-order and total-order indices of the objective value and of every moment of `m` with
respect to every sampled parameter, over its box or over a sub-box `box = Dict(name => (lo, hi))`.  `Dict(:first, :total, :interaction,
:se_first, :se_total => Dict(output => Dict(name => index)), :mean, :var => Dict(output => value), :n_complete, :n_invalid, :evaluated)`,
the outputs being `:value` and the moments' names.
"""
function sobolIndicesHip(m::MProb, n_base::Integer = 4096; box = nothing, opts::Dict = Dict())
    pk = collect(keys(m.params_to_sample))
    outs = vcat(Any[:value], collect(keys(m.moments)))
    lo = hi = nothing
    if box !== nothing
        lo = Float64[haskey(box, k) ? box[k][1] : m.params_to_sample[k][:lb] for k in pk]
        hi = Float64[haskey(box, k) ? box[k][2] : m.params_to_sample[k][:ub] for k in pk]
    end
    h = eval_context(m, opts)
    r = SMMHip.hip_sens_sobol(h, n_base; lo = lo, hi = hi)
    SMMHip.hip_destroy!(h)
    table(a) = Dict(o => Dict(k => a[j, f] for (j, k) in enumerate(pk)) for (f, o) in enumerate(outs))
    return Dict(:first => table(r.first), :total => table(r.total), :interaction => table(r.total .- r.first), :se_first => table(r.se_first),
                :se_total => table(r.se_total), :mean => Dict(o => r.mean[f] for (f, o) in enumerate(outs)),
                :var => Dict(o => r.var[f] for (f, o) in enumerate(outs)), :n_complete => r.n_complete, :n_invalid => r.n_invalid,
                :evaluated => r.evaluated)
end

"`FD_gradient(m, p)` (econometrics.jl:29-85): the 1 + k (forward) or 2k (central) evaluations in one batch; rows in the order of `p`"
function FD_gradient_hip(m::MProb, p::Union{Dict,OrderedDict}; step_perc = 0.01, diff_method = :forward, use_range = true, opts::Dict = Dict())
    diff_method in (:forward, :central) || error("only :central and :foward implemented")
    rs = SMM.range_length(m)
    ks = collect(keys(p))
    hs = Float64[(use_range ? rs[k] : p[k]) * step_perc for k in ks]
    ps = Any[deepcopy(p)]
    for (k, h) in zip(ks, hs)
        if diff_method == :forward
            q = deepcopy(p); q[k] = p[k] + h; push!(ps, q)
        else
            q = deepcopy(p); q[k] = p[k] + 0.5 * h; push!(ps, q)
            q = deepcopy(p); q[k] = p[k] - 0.5 * h; push!(ps, q)
        end
    end
    evs = evaluateObjectivesHip(m, ps; opts = opts)
    mk = collect(keys(m.moments))
    g(ev) = Float64[ev.simMoments[k] for k in mk]
    gp = g(evs[1])
    D = zeros(length(ks), length(mk))
    for (i, h) in enumerate(hs)
        D[i, :] = diff_method == :forward ? (g(evs[1 + i]) .- gp) ./ h : (g(evs[2 * i]) .- g(evs[2 * i + 1])) ./ h
    end
    return D
end

"`getSigma(m, p, reps)` (econometrics.jl:125-145): `reps` evaluations with their own shock sequences (seed + i) in one batch"
function getSigmaHip(m::MProb, p::Union{Dict,OrderedDict}, reps::Int; seed::Integer = 0, opts::Dict = Dict())
    evs = evaluateObjectivesHip(m, Any[deepcopy(p) for i in 1:reps]; opts = opts, noseed_base = seed)
    mk = collect(keys(m.moments))
    X = Float64[ev.simMoments[k] for ev in evs, k in mk]
    mu = sum(X, dims = 1) ./ reps
    Xc = X .- mu
    return (Xc' * Xc) ./ (reps - 1)
end

end # module
