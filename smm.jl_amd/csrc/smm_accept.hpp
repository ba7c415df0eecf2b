// smm_accept.hpp — what a chain does at the end of an iteration, written once: the numerical contract shared by the five chain kernels
// (k_chain_iter, k_chain_iter_norm*, k_chain_persist_loc, k_chain_persist_gen, k_chain_persist_tile), the kernels that rewrite an exchanged
// row (k_flush, k_exch_apply, k_a2a_apply) and the install of a population (k_pop_select).  Host + gfx950 device code, included by
// smm_params.hpp (so ahead of smm_chain.hpp and of every other user, in smmhip.hip, in the hiprtc builds and in tools/).  Scalars, and pointers or arrays the caller hands in (registers or LDS): nothing here knows of parameter blocks, lanes
// or tiles.  WHEN a rule is evaluated, which lane evaluates it and how an error is reported stay with each kernel.
//   doAcceptReject!                 src/mopt/AlgoBGP.jl:324-392  -> accept_decide
//   set_acceptRate!                 src/mopt/AlgoBGP.jl:253-257  -> accept_rate
//   the sigma update                src/mopt/AlgoBGP.jl:381-390  -> sigma_next
//   set_eval!                       src/mopt/AlgoBGP.jl:220-245  -> best_of, history_head, record_head
//   swap_ev_ij!'s set_eval!(ci, ej) src/mopt/AlgoBGP.jl:231-243, 734-749 -> swapped_head
//   objfunc_norm's moments          src/mopt/ObjExamples.jl:79-110 -> moment_sq, sum_in_order; banana :251-265 -> banana_value
//   a failing evaluation            src/mopt/mprob.jl:183-186    -> in_failbox
#pragma once

#define SMM_RULE __host__ __device__ __forceinline__

// history record: its head (the parameters and the simulated moments follow from H_PARAMS on)
enum : int { H_VALUE = 0, H_PROB, H_CURR, H_BEST, H_BESTID, H_EXCH, H_ACC, H_STATUS, H_PARAMS };

// doAcceptReject!.  first: iteration 1, accepted whatever the evaluation said (:326-332).  exp_fn: the contract exponential (smm_rng.hpp:
// smm_exp, or a kernel's out-of-line copy of it).  negative: the value was not >= 0 (:341) — a hard error, reported by the caller.
struct AcceptDecision {
    double prob;
    bool acc;
    int status;
    bool negative;
};
template <class ExpFn>
SMM_RULE AcceptDecision accept_decide(const bool first, const int status, const double value, const double old, const double atun,
                                      const double u, ExpFn exp_fn) {
    if (first) return {1.0, true, 1, false};
    if (status < 0) return {0.0, false, status, false};   // :336-338
    const bool negative = !(value >= 0.0);
    const double e = exp_fn(atun * (old - value));
    const double prob = (e != e) ? e : (e < 1.0 ? e : 1.0);   // minimum([1.0,e]), NaN propagates (:344)
    if (!isfinite(prob)) return {0.0, false, -1, negative};   // :350-353
    if (!isfinite(old)) return {1.0, true, status, negative};   // :355-359
    return {prob, prob > u, 1, negative};                      // strict >, :362-367
}

// set_acceptRate!: na acceptances in nn iterations without an exchange, this one (not exchanged at this point) counted in
SMM_RULE double accept_rate(const int na, const int nn, const bool acc) { return (double)(na + (acc ? 1 : 0)) / (double)(nn + 1); }

// the sigma update of an iteration that is a multiple of sigma_update_steps
SMM_RULE double sigma_next(const double sig, const double rate, const double adjust_by) {
    return (rate > 0.234) ? sig * (1.0 + adjust_by) : sig * (1.0 - adjust_by);
}

// best value and the iteration it was found in, after iteration t (a tie keeps the older one; a NaN never is the best).
// bp: {best, best_id} so far, as they lie in a chain's state block — read when needed, for callers whose block is in memory
struct Best {
    double best, best_id;
};
SMM_RULE Best best_of(const double value, const int t, const double* bp) {
    if (value < bp[0]) return {value, (double)t};
    return {bp[0], bp[1]};
}
// (the same rule for callers that hold the pair in registers; written through the pointer form, not the other way round, so that k_flush
// and the apply kernels read their state block only when needed: 4 VGPRs less there, MEASUREMENTS.md)
SMM_RULE Best best_of(const double value, const int t, const double bp, const double bpid) {
    const double so_far[2] = {bp, bpid};
    return best_of(value, t, so_far);
}

SMM_RULE void history_head(double* h, const double value, const double prob, const double curr, const double best, const double best_id,
                           const double exch, const double acc, const double status) {
    h[H_VALUE] = value; h[H_PROB] = prob; h[H_CURR] = curr; h[H_BEST] = best; h[H_BESTID] = best_id;
    h[H_EXCH] = exch; h[H_ACC] = acc; h[H_STATUS] = status;
}

// the chain's record of the exchanged iteration tp is the donor's last accepted one {value, prob, status, ...}: accepted, the donor's prob
// and status, curr = the donor's value, exchanged = partner, best against the best after iteration tp - 1 (bestp: {best, best_id}).
// (the donor's parameters and moments are copied by the caller)
SMM_RULE void swapped_head(double* h, const double* donor, const int partner, const Best b) {
    const double value = donor[0];
    h[H_VALUE] = value; h[H_PROB] = donor[1]; h[H_CURR] = value; h[H_BEST] = b.best; h[H_BESTID] = b.best_id;
    h[H_EXCH] = (double)partner; h[H_ACC] = 1.0; h[H_STATUS] = donor[2];
}
SMM_RULE Best swapped_head(double* h, const double* donor, const int partner, const int tp, const double* bestp) {
    const Best b = best_of(donor[0], tp, bestp);
    swapped_head(h, donor, partner, b);
    return b;
}

// the head of the chain's last accepted record (lastAccepted, :209-215): this iteration's if accepted, else the one it continued from
SMM_RULE void record_head(double* out, const double* in, const bool acc, const double value, const double prob, const int status) {
    out[0] = acc ? value : in[0]; out[1] = acc ? prob : in[1]; out[2] = acc ? (double)status : in[2];
}

// a moment's term: the deviation of the simulated mean from the data moment, over the weight unless that is NaN, squared
SMM_RULE double moment_sq(const double m, const double mom, const double w) {
    double d = m - mom;
    if (!isnan(w)) d = d / w;
    return d * d;
}

// the terms added in moment order (read eight at a time)
SMM_RULE double sum_in_order(const double* vk, const int n) {
    double vsum = 0.0;
    int k = 0;
    for (; k + 8 <= n; k += 8) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = vk[k + u];
#pragma unroll
        for (int u = 0; u < 8; ++u) vsum = (k + u == 0) ? v[u] : vsum + v[u];
    }
    for (; k < n; ++k) vsum = (k == 0) ? vk[k] : vsum + vk[k];
    return vsum;
}

// the banana in np dimensions, its terms in order
SMM_RULE double banana_value(const double* theta, const int np) {
    double v = 0.0;
    for (int i = 0; i + 1 < np; ++i) {
        const double a = theta[i], b = theta[i + 1];
        const double t1 = b - a * a;
        const double t2 = 1.0 - a;
        const double term = 100.0 * (t1 * t1) + t2 * t2;
        v = (i == 0) ? term : v + term;
    }
    return v;
}

// SMM_OBJ_NORM_FAILBOX's "exception": the first parameter inside box = {lo, hi} (the evaluation then has value -1, Eval.jl:84, status -2
// and NaN moments).  The bounds are read where they lie, hi only if lo passed: with both handed in as loaded values k_chain_persist_loc
// waited for two LDS reads ahead of its accept step and C2 lost 1 % (MEASUREMENTS.md)
SMM_RULE bool in_failbox(const double theta0, const double* box) { return theta0 >= box[0] && theta0 <= box[1]; }

#undef SMM_RULE
