"""Host-side mirror of the reference's API surface for the BGP path (src/SMM.jl:31-57).

The reference is Julia; no julia binary exists in the build image, so the host layer above the C
ABI is written in Python with the reference's names, argument meaning and error behaviour
(`addSampledParam!` -> `addSampledParam`, `run!` -> `run`, ...).  A Julia maintainer binds the
same C ABI with `ccall`.  Everything numerical happens in libsmmhip.so.

  MProb, addParam, addSampledParam, addMoment, addEvalFunc          mprob.jl:29-159
  Eval and its accessors                                            Eval.jl:20-238
  evaluateObjective                                                 mprob.jl:175-205
  objfunc_norm / banana: device objectives                          ObjExamples.jl:59-116, 251-265
  BGPChain (a view on the downloaded history), MAlgoBGP             AlgoBGP.jl:42-110, 497-539
  computeNextIteration, run, restart, history, summary, ...         AlgoBGP.jl:589-640, AlgoAbstract.jl:27-76
"""
import time as _time
from builtins import range as _builtins_range
from collections import OrderedDict

import numpy as np

from . import _abi as A
from .backend import BGPOpts, Problem, Tables, hip_context


# ------------------------------------------------------------------------------------------
# objectives: the reference stores a Julia function in MProb.objfunc (mprob.jl:159) and calls
# it with an Eval (mprob.jl:182).  On the GPU the objective is a device function selected by id.
# ------------------------------------------------------------------------------------------
class DeviceObjective:
    def __init__(self, name, objective_id, ns=10000, needs_square=False):
        self.name, self.objective_id, self.ns, self.needs_square = name, objective_id, ns, needs_square

    def __call__(self, ev, **opts):  # f(ev::Eval; kwargs...)::Eval, evaluated on the device
        return evaluateObjective(ev._mprob, ev) if getattr(ev, "_mprob", None) is not None else _no_mprob()

    def __repr__(self):
        return "<device objective %s>" % self.name


def _no_mprob():
    raise ValueError("a device objective needs an Eval built from an MProb (Eval(mprob, p))")


def user_objective(source, name="user_objective", n_sums=None, lanes=256, rng=False):
    """A user-written device objective (MProb.objfunc of the reference, mprob.jl:159): HIP/C++ text that defines
    SMM_USER_OBJECTIVE(...) — or, with n_sums=k, the map-reduce pair SMM_USER_PARTIAL / SMM_USER_FINISH evaluated by
    `lanes` threads per chain — see include/smmhip.h.  addEvalFunc(m, user_objective(src));
    m.objfunc_opts["obj_params"] = [...] passes udata.  rng=True: the _RNG forms, which draw from the library's generator
    (smm_normal / smm_normal2 / smm_uniform) and so have noseed evaluations: getSigma / get_stdErrors work on them."""
    from .backend import register_user_objective
    return DeviceObjective(name, register_user_objective(source, n_sums, lanes, rng=rng), ns=1)


objfunc_norm = DeviceObjective("objfunc_norm", A.SMM_OBJ_NORM, needs_square=True)   # ObjExamples.jl:59-116
banana = DeviceObjective("banana", A.SMM_OBJ_BANANA, ns=1)                           # ObjExamples.jl:251-265
dense_sim = DeviceObjective("dense_sim", A.SMM_OBJ_DENSE, ns=1)                     # synthetic dense simulation (include/smmhip.h)
dense_sim2 = DeviceObjective("dense_sim2", A.SMM_OBJ_DENSE2, ns=1)                  # ... with the 256 x 256 stage: BASELINE config 5 as worded


class MProb:
    """mprob.jl:29-53"""

    def __init__(self):
        self.initial_value = OrderedDict()
        self.params_to_sample = OrderedDict()
        self.objfunc = None
        self.objfunc_opts = {}
        self.moments = OrderedDict()

    def __repr__(self):
        return "MProb: %d parameters to sample, %d moments, objective %r" % (
            len(self.params_to_sample), len(self.moments), self.objfunc)


def addParam(m, name_or_dict, init=None):
    """addParam!, mprob.jl:60-75"""
    if isinstance(name_or_dict, dict):
        for k, v in name_or_dict.items():
            m.initial_value[str(k)] = v
    else:
        m.initial_value[str(name_or_dict)] = init
    return m


def addSampledParam(m, name_or_dict, init=None, lb=None, ub=None):
    """addSampledParam!, mprob.jl:81-98: a name with (init, lb, ub), or a dict name -> [init, lb, ub]"""
    if isinstance(name_or_dict, dict):
        for k, v in name_or_dict.items():
            addSampledParam(m, k, v[0], v[1], v[2])
        return m
    if not ub > lb:
        raise AssertionError("ub>lb")  # @assert ub>lb, mprob.jl:82
    m.initial_value[str(name_or_dict)] = init
    m.params_to_sample[str(name_or_dict)] = {"lb": lb, "ub": ub}
    return m


def addMoment(m, name, value=None, weight=1.0):
    """addMoment!, mprob.jl:123-155: (name, value[, weight]), a dict name -> {value, weight}, or a
    table with columns name/value/weight (pandas DataFrame or dict of columns)."""
    if hasattr(name, "columns") or (isinstance(name, dict) and "name" in name and "value" in name):
        names, values = list(name["name"]), list(name["value"])
        weights = list(name["weight"]) if "weight" in name else [1.0] * len(names)
        for n, v, w in zip(names, values, weights):
            addMoment(m, n, v, w)
        return m
    if isinstance(name, dict):
        for k, d in name.items():
            addMoment(m, k, d["value"], d["weight"])
        return m
    m.moments[str(name)] = {"value": value, "weight": weight}
    return m


def addEvalFunc(m, f):
    """addEvalFunc!, mprob.jl:159"""
    m.objfunc = f
    return m


def ps_names(m):
    return list(m.initial_value.keys())


def ps2s_names(m):
    return list(m.params_to_sample.keys())


def ms_names(m):
    return list(m.moments.keys())


def _flat_problem(m):
    if not isinstance(m.objfunc, DeviceObjective):
        raise TypeError("MProb.objfunc must be a device objective (objfunc_norm, banana, dense_sim, or user_objective(src) "
                        "for your own): arbitrary host closures cannot run inside the GPU iteration")
    names = ps2s_names(m)
    init = [m.initial_value[k] for k in names]
    lb = [m.params_to_sample[k]["lb"] for k in names]
    ub = [m.params_to_sample[k]["ub"] for k in names]
    mom = [m.moments[k]["value"] for k in ms_names(m)]
    w = [np.nan if m.moments[k]["weight"] is None else m.moments[k]["weight"] for k in ms_names(m)]
    return Problem(init, lb, ub, mom, w, ns=m.objfunc_opts.get("ns", m.objfunc.ns), objective_id=m.objfunc.objective_id,
                   obj_params=m.objfunc_opts.get("obj_params"))


class Eval:
    """Eval.jl:20-155.  Constructors: Eval(), Eval(mprob), Eval(mprob, p), Eval(p, moments_table)."""

    def __init__(self, a=None, b=None):
        self.value = -1.0
        self.time = _time.time()
        self.status = -1
        self.params = OrderedDict()
        self.simMoments = OrderedDict()
        self.dataMoments = OrderedDict()
        self.dataMomentsW = OrderedDict()
        self.prob = 0.0
        self.accepted = False
        self.options = {}
        self._mprob = None
        if isinstance(a, MProb):
            self._mprob = a
            for k, d in a.moments.items():
                self.dataMoments[k] = d["value"]
                self.dataMomentsW[k] = d["weight"]
            p = a.initial_value if b is None else b  # Eval(mprob) uses the initial value, Eval.jl:108-130
            for k, v in p.items():
                self.params[str(k)] = v
        elif a is not None:  # Eval(p::Dict, mom::DataFrame), Eval.jl:48-80
            for col in ("name", "value", "weight"):
                if col not in b:
                    raise ValueError("moment dataframe needs column named `%s`" % col)
            for n, v, w in zip(b["name"], b["value"], b["weight"]):
                self.dataMoments[str(n)] = v
                self.dataMomentsW[str(n)] = w
            for k, v in a.items():
                self.params[str(k)] = v[0] if np.ndim(v) else v

    def __eq__(self, o):  # Eval.jl:157-166
        return (self.value == o.value and self.status == o.status and self.params == o.params and
                self.simMoments == o.simMoments and self.dataMoments == o.dataMoments and self.accepted == o.accepted)


def param(ev, which=None):
    if which is None:
        return np.array(list(ev.params.values()), float)
    if isinstance(which, (list, tuple)):
        return np.array([ev.params[k] for k in which], float)
    return ev.params[which]


def paramd(ev):
    return ev.params


def dataMoment(ev, which=None):
    if which is None:
        return np.array(list(ev.dataMoments.values()), float)
    if isinstance(which, (list, tuple)):
        return np.array([ev.dataMoments[k] for k in which], float)
    return ev.dataMoments[which]


def dataMomentd(ev):
    return ev.dataMoments


def dataMomentW(ev, which=None):
    if which is None:
        return np.array(list(ev.dataMomentsW.values()), float)
    if isinstance(which, (list, tuple)):
        return np.array([ev.dataMomentsW[k] for k in which], float)
    return ev.dataMomentsW[which]


def dataMomentWd(ev):
    return ev.dataMomentsW


def setValue(ev, value):
    ev.value = float(value)


def setMoments(ev, k, value=None):
    if isinstance(k, dict):
        for kk, v in k.items():
            ev.simMoments[str(kk)] = v
    else:
        ev.simMoments[str(k)] = value


def fill(p, ev):
    """fill(p, ev): copy the parameters onto the fields of a user object, Eval.jl:207-211"""
    for k, v in ev.params.items():
        setattr(p, k, v)


def _eval_context(m, prob):
    """the device context behind evaluateObjective, kept on the MProb and rebuilt when anything it holds a device copy
    of changes (dimensions, objective, data moments, weights, objective parameters; byte-wise, so NaN weights compare equal)"""
    op = b"" if prob.obj_params is None else prob.obj_params.tobytes()
    key = (prob.np, prob.nm, prob.ns, prob.objective_id, prob.mom.tobytes(), prob.w.tobytes(), op,
           prob.init.tobytes(), prob.lb.tobytes(), prob.ub.tobytes())
    cached = getattr(m, "_eval_ctx", None)
    if cached is None or cached[0] != key:
        if cached is not None:
            cached[1].close()
        opts = BGPOpts(N=1, maxiter=1, sigma=[0.05], acc_tuner=[1.0], min_improve=[0.0])
        cached = (key, hip_context(prob, opts))
        m._eval_ctx = cached
    return cached[1]


def evaluateObjective(m, p_or_ev):
    """evaluateObjective(m, p) / (m, ev), mprob.jl:175-205, as a batch of one on the device."""
    ev = p_or_ev if isinstance(p_or_ev, Eval) else Eval(m, p_or_ev)
    prob = _flat_problem(m)
    ctx = (None, _eval_context(m, prob))
    names = ps2s_names(m)
    theta = np.array([[ev.params[k]] for k in names], float)
    t0 = _time.time()
    v, sm, st = ctx[1].eval_batch(theta)
    ev.value, ev.status = float(v[0]), int(st[0])
    for k, x in zip(ms_names(m), sm[:, 0]):
        ev.simMoments[k] = float(x)
    ev.time = _time.time() - t0
    return ev


# ------------------------------------------------------------------------------------------
# BGPChain: AlgoBGP.jl:42-110.  The chain's per-iteration arrays are views on the downloaded
# structure-of-arrays history; evals[t] materialises an Eval on demand.
# ------------------------------------------------------------------------------------------
class _Evals:
    def __init__(self, chain):
        self._c = chain

    def __len__(self):
        return self._c._algo.opts["maxiter"]

    def __getitem__(self, t):
        c = self._c
        if isinstance(t, slice):
            return [self[i] for i in range(*t.indices(len(self)))]
        if isinstance(t, (np.ndarray, list)):
            idx = np.flatnonzero(t) if np.asarray(t).dtype == bool else t
            return [self[int(i)] for i in idx]
        h = c._h()
        if t < 0:
            t += h.value.shape[0]
        ev = Eval(c.m, OrderedDict((k, float(h.params[t, i, c._j])) for i, k in enumerate(ps2s_names(c.m))))
        ev.value = float(h.value[t, c._j]); ev.prob = float(h.prob[t, c._j])
        ev.accepted = bool(h.accepted[t, c._j]); ev.status = int(h.status[t, c._j])
        for i, k in enumerate(ms_names(c.m)):
            ev.simMoments[k] = float(h.sim_moments[t, i, c._j])
        return ev


class BGPChain:
    def __init__(self, algo, j):
        self._algo, self._j = algo, j
        self.id = j + 1
        self.m = algo.m
        self.evals = _Evals(self)

    def _h(self):
        return self._algo._history()

    def _col(self, f, fill, dtype):
        h, n = self._h(), self._algo.opts["maxiter"]
        out = np.full(n, fill, dtype)
        out[: h.value.shape[0]] = getattr(h, f)[:, self._j]
        return out

    iter = property(lambda s: s._algo.i)
    accepted = property(lambda s: s._col("accepted", 0, np.uint8).astype(bool))
    exchanged = property(lambda s: s._col("exchanged", 0, np.int64))
    best_val = property(lambda s: s._col("best_val", np.inf, float))
    curr_val = property(lambda s: s._col("curr_val", np.inf, float))
    best_id = property(lambda s: s._col("best_id", -1, np.int64))
    sigma = property(lambda s: float(s._algo._state().sigma[s._j]))
    accept_rate = property(lambda s: float(s._algo._state().accept_rate[s._j]))
    acc_tuner = property(lambda s: float(s._algo._acc_tuner[s._j]))
    min_improve = property(lambda s: float(s._algo._min_improve[s._j]))
    sigma_update_steps = property(lambda s: s._algo._flat["sigma_update_steps"])
    sigma_adjust_by = property(lambda s: s._algo._flat["sigma_adjust_by"])
    smpl_iters = property(lambda s: s._algo._flat["smpl_iters"])


def allAccepted(c):
    """AlgoBGP.jl:117"""
    return c.evals[c.accepted[: c.iter]]


def params(c, accepted_only=True):
    """AlgoBGP.jl:120-131: dict name -> vector of parameter values"""
    h = c._h()
    sel = h.accepted[:, c._j].astype(bool) if accepted_only else np.ones(h.value.shape[0], bool)
    return {k: h.params[sel, i, c._j].copy() for i, k in enumerate(ps2s_names(c.m))}


def history(c):
    """history(c::BGPChain), AlgoBGP.jl:138-160: columns iter, value, accepted, curr_val, best_val, prob,
    exchanged, <params...> (a pandas DataFrame when pandas is importable, else a dict of columns)."""
    h = c._h()
    n = h.value.shape[0]
    cols = OrderedDict()
    cols["iter"] = np.arange(1, n + 1)
    cols["value"] = h.value[:, c._j].copy()
    cols["accepted"] = h.accepted[:, c._j].astype(bool)
    cols["curr_val"] = h.curr_val[:, c._j].copy()
    cols["best_val"] = h.best_val[:, c._j].copy()
    cols["prob"] = h.prob[:, c._j].copy()
    cols["exchanged"] = h.exchanged[:, c._j].astype(np.int64)
    for i, k in enumerate(ps2s_names(c.m)):
        cols[k] = h.params[:, i, c._j].copy()
    try:
        import pandas as pd
        return pd.DataFrame(cols)
    except Exception:  # pragma: no cover
        return cols


def _stats(c, probs=()):
    """the device's summaries of every chain of c's MAlgoBGP over its accepted draws (smm_get_chain_stats), one call per
    (iteration, probs): mean, median, CI, best and summary read them instead of downloading the history"""
    return c._algo._chain_stats(True, tuple(float(p) for p in probs))


def best(c):
    """best(c) -> (val, idx), AlgoBGP.jl:167 (1-based index like findmin)"""
    if c._algo.i == 0:
        np.argmin(np.empty(0))   # raises as findmin of an empty history
    st = _stats(c)
    return float(st["best_value"][c._j]), int(st["best_iter"][c._j])


def _empty_selection(c, st):
    return st["count"][c._j] == 0


def cov(c):
    """the covariance matrix of chain c's accepted draws (np.cov(params(c)), ddof 1), reduced on the device (smm_get_chain_cov)"""
    a = c._algo
    if a._cov is None or a._cov[0] != a.i:
        a._cov = (a.i, a._ctx.chain_cov(0, a.i, True, False))
    return a._cov[1][2][:, :, c._j].copy()


def mean(c):
    st = _stats(c)
    if _empty_selection(c, st):
        return {k: float(np.mean(np.empty(0))) for k in ps2s_names(c.m)}   # numpy's RuntimeWarning and NaN
    return {k: float(st["mean"][i, c._j]) for i, k in enumerate(ps2s_names(c.m))}


def median(c):
    st = _stats(c)
    if _empty_selection(c, st):
        return {k: float(np.median(np.empty(0))) for k in ps2s_names(c.m)}
    return {k: float(st["median"][i, c._j]) for i, k in enumerate(ps2s_names(c.m))}


def CI(c, level=0.95):
    q = ((1 - level) / 2, 1 - (1 - level) / 2)
    st = _stats(c, q)
    if _empty_selection(c, st):
        return {k: np.quantile(np.empty(0), list(q)) for k in ps2s_names(c.m)}   # raises IndexError, as np.quantile of no draw
    return {k: st["quantile"][:, i, c._j].copy() for i, k in enumerate(ps2s_names(c.m))}


def _diag(algo, window, groups):
    """the device's diagnostics of every chain of algo over window = (t0, t1) (default: every completed iteration; smm_get_chain_diag),
    one call per (iteration, window, groups): ess and rhat read them instead of downloading the history"""
    t0, t1 = (0, algo.i) if window is None else (int(window[0]), int(window[1]))
    g = None if groups is None else tuple(int(v) for v in groups)
    key = (algo.i, t0, t1, g)
    if key not in algo._diag:
        algo._diag[key] = algo._ctx.chain_diag(t0, t1, groups=None if g is None else np.asarray(g, np.int32))
    return algo._diag[key]


def ess(c, window=None):
    """the effective sample size of each parameter of chain c over window = (t0, t1) (default: the whole run): Geyer's initial
    monotone sequence on the chain's state, computed on the device (include/smmhip.h: smm_get_chain_diag); NaN where undefined"""
    d = _diag(c._algo, window, None)
    return OrderedDict((k, float(d["ess"][i, c._j])) for i, k in enumerate(ps2s_names(c.m)))


def _default_groups(algo):
    """the chains with equal acc_tuners entries, which share a target density, numbered in order of first appearance"""
    ids = {}
    return [ids.setdefault(float(a), len(ids)) for a in algo._acc_tuner]


def rhat(algo, groups=None, window=None):
    """the split R-hat of each parameter in each group of chains over window = (t0, t1) (default: the whole run), on the device:
    one OrderedDict per group.  groups: a group id per chain (-1 = none); by default the chains with equal acc_tuners entries, which
    share a target density, numbered in order of first appearance"""
    d = _diag(algo, window, _default_groups(algo) if groups is None else groups)
    return [OrderedDict((k, float(d["rhat"][g, i])) for i, k in enumerate(ps2s_names(algo.m))) for g in range(d["rhat"].shape[0])]


def _rank_diag(algo, window, groups, bins):
    """the device's rank-normalised diagnostics of the groups of algo over window = (t0, t1) (default: every completed iteration;
    smm_get_rank_diag), one call per (iteration, window, groups, bins)"""
    t0, t1 = (0, algo.i) if window is None else (int(window[0]), int(window[1]))
    g = tuple(int(v) for v in (_default_groups(algo) if groups is None else groups))
    key = ("rank", algo.i, t0, t1, g, int(bins))
    if key not in algo._diag:
        algo._diag[key] = algo._ctx.rank_diag(t0, t1, n_bins=int(bins), groups=np.asarray(g, np.int32))
    return algo._diag[key]


def _per_group(algo, a):
    return [OrderedDict((k, float(a[g, i])) for i, k in enumerate(ps2s_names(algo.m))) for g in range(a.shape[0])]


def rhat_rank(algo, groups=None, window=None):
    """the rank-normalised split R-hat (the larger of the bulk and the folded statistic; Vehtari et al. 2021) of each parameter in each
    group of chains over window = (t0, t1) (default: the whole run), on the device (include/smmhip.h: smm_get_rank_diag): one
    OrderedDict per group.  groups and window as in rhat"""
    return _per_group(algo, _rank_diag(algo, window, groups, 0)["rhat_rank"])


def ess_bulk(algo, groups=None, window=None):
    """the multi-chain bulk ESS (of the rank-normalised split chains) of each parameter in each group's pooled sample, on the device
    (include/smmhip.h: smm_get_rank_diag): one OrderedDict per group; NaN where undefined.  groups and window as in rhat"""
    return _per_group(algo, _rank_diag(algo, window, groups, 0)["ess_bulk"])


def ess_tail(algo, groups=None, window=None):
    """the multi-chain tail ESS (the smaller of the ESS of the 5 % and of the 95 % quantile indicators) of each parameter in each
    group's pooled sample, on the device (include/smmhip.h: smm_get_rank_diag): one OrderedDict per group; NaN where undefined"""
    return _per_group(algo, _rank_diag(algo, window, groups, 0)["ess_tail"])


def rank_plot(algo, groups=None, window=None, bins=20):
    """the rank plot of every chain: an OrderedDict name -> int64 array [N][bins], chain c's draws of the window counted by the bin of
    their rank in the pooled sample of c's group (uniform when the chains of a group agree), on the device (include/smmhip.h:
    smm_get_rank_diag); zeros for a chain in no group.  groups and window as in rhat"""
    h = _rank_diag(algo, window, groups, bins)["rank_hist"]
    return OrderedDict((k, h[:, i, :].T.copy()) for i, k in enumerate(ps2s_names(algo.m)))


def pooled(algo, groups=None, window=None, accepted_only=True, level=0.95):
    """the posterior of each group's pooled draws over window = (t0, t1) (default: the whole run), summarised on the device
    (include/smmhip.h: smm_get_group_stats): one OrderedDict per group with count, chains, mean / median (name -> value), CI
    (name -> [lo, hi]) and cov (ndarray [np][np]).  groups: a group id per chain (-1 = none); by default those of rhat"""
    t0, t1 = (0, algo.i) if window is None else (int(window[0]), int(window[1]))
    g = tuple(int(v) for v in (_default_groups(algo) if groups is None else groups))
    q = ((1 - level) / 2, 1 - (1 - level) / 2)
    key = (algo.i, t0, t1, g, bool(accepted_only), q)
    if key not in algo._pooled:
        algo._pooled[key] = algo._ctx.group_stats(t0, t1, accepted_only, np.asarray(g, np.int32), q)
    r = algo._pooled[key]
    names = ps2s_names(algo.m)
    return [OrderedDict(count=int(r["count"][j]), chains=int(r["n_chains"][j]),
                        mean=OrderedDict((k, float(r["mean"][j, i])) for i, k in enumerate(names)),
                        median=OrderedDict((k, float(r["median"][j, i])) for i, k in enumerate(names)),
                        CI=OrderedDict((k, r["quantile"][:, j, i].copy()) for i, k in enumerate(names)),
                        cov=r["cov"][j].copy())
            for j in range(r["count"].shape[0])]


def derived(algo, transform, names=None, t0=0, t1=None, select="accepted", groups=None, probs=(0.025, 0.975), tdata=()):
    """the posterior of a user function of each draw (Stan's generated quantities: an elasticity, a ratio of parameters, a statistic of
    the simulated moments) over each group's pooled rows of iterations [t0, t1) (default: the whole run), evaluated and summarised on
    the device (include/smmhip.h: smm_get_derived) without downloading the history: one OrderedDict per group, keyed like pooled()'s —
    count, chains, mean / median (name -> value), CI (name -> the quantiles of probs), cov (ndarray [Q][Q]) — and n_nonfinite
    (name -> rows whose value is NaN or infinite).  transform: what user_transform(source, n_out) returned; names: the Q outputs' names
    (default out0, out1, ..); select: "all", "accepted" or "state"; groups: a group id per chain (-1 = none), by default those of
    rhat; tdata: the vector the function receives as tdata"""
    Q = transform.n_out
    names = ["out%d" % q for q in _builtins_range(Q)] if names is None else list(names)
    if len(names) != Q or len(set(names)) != Q:
        raise ValueError("derived: names must be %d distinct names, one per output" % Q)
    g = np.asarray(_default_groups(algo) if groups is None else groups, np.int32)
    r = algo._ctx.derived(transform, int(t0), algo.i if t1 is None else int(t1), select, g, probs, tdata)
    return [OrderedDict(count=int(r["count"][j]), chains=int(r["n_chains"][j]),
                        n_nonfinite=OrderedDict((k, int(r["n_nonfinite"][j, i])) for i, k in enumerate(names)),
                        mean=OrderedDict((k, float(r["mean"][j, i])) for i, k in enumerate(names)),
                        median=OrderedDict((k, float(r["median"][j, i])) for i, k in enumerate(names)),
                        CI=OrderedDict((k, r["quantile"][:, j, i].copy()) for i, k in enumerate(names)),
                        cov=r["cov"][j].copy())
            for j in _builtins_range(r["count"].shape[0])]


def _hist_call(x, window, accepted_only, state, **kw):
    """(algo, chain index or None, the device's histogram dict) of a chain (alone in group 0) or of the groups of an algo"""
    if isinstance(x, BGPChain):
        algo, j = x._algo, x._j
        g = np.full(algo._ctx.N, -1, np.int32)
        g[j] = 0
        kw["n_groups"] = 1
    else:
        algo, j = x, None
        g = np.asarray(_default_groups(algo) if kw.get("groups") is None else kw["groups"], np.int32)
    kw.pop("groups", None)
    t0, t1 = (0, algo.i) if window is None else (int(window[0]), int(window[1]))
    sel = "state" if state else "accepted" if accepted_only else "all"
    return algo, j, algo._ctx.histogram(t0, t1, sel, g, **kw)


def _hist_range(rng, names):
    """numpy's checks of a given range, then the rows [np][2] of the call (by name or in parameter order)"""
    if rng is None:
        return None
    rows = [rng[k] for k in names] if isinstance(rng, dict) else list(rng)
    for lo, hi in rows:
        if lo > hi:
            raise ValueError("max must be larger than min in range parameter.")
        if not (np.isfinite(lo) and np.isfinite(hi)):
            raise ValueError("supplied range of [{}, {}] is not finite".format(lo, hi))
    return np.asarray(rows, np.float64).reshape(len(names), 2)


def _hist_raise(st, lo, hi, bins, one_d=True):
    """the ValueError numpy raises where the device reports a status (include/smmhip.h: smm_get_histogram)"""
    if st == 1:
        raise ValueError("autodetected range of [{}, {}] is not finite".format(lo, hi))
    if st == 2:
        raise ValueError("range of [{}, {}] has a width that is not finite".format(lo, hi))
    if st == 3 and one_d:
        raise ValueError("Too many bins for data range. Cannot create {} finite-sized bins.".format(bins))


def histogram(x, bins=10, range=None, window=None, accepted_only=True, state=False, density=False, groups=None):
    """np.histogram(params(c, accepted_only)[name], bins, range, density) of every parameter, counted on the device (include/smmhip.h:
    smm_get_histogram) without downloading the history: an OrderedDict name -> (counts, edges) for a chain, a list of them (one per
    group) for an algo, whose groups default to those of rhat / pooled.  window = (t0, t1) (default: the whole run); state: the chain's
    state series (each iteration weighted by holding time) instead of its accepted draws; range: [np][2] or name -> (lo, hi).  Where
    numpy raises (a non-finite autodetected range, a bad range, too many bins for the range), so does this"""
    if int(bins) < 1:
        raise ValueError("`bins` must be positive, when an integer")
    names = ps2s_names(x.m)
    _, j, r = _hist_call(x, window, accepted_only, state, groups=groups, bins=int(bins), range=_hist_range(range, names))
    out = []
    for g in _builtins_range(r["count"].shape[0]):
        d = OrderedDict()
        for i, k in enumerate(names):
            _hist_raise(r["status"][g, i], r["lo"][g, i], r["hi"][g, i], bins)
            n, e = r["hist"][g, i].copy(), r["edges"][g, i].copy()
            if density:
                db = np.diff(e)
                n = n / db / n.sum()
            d[k] = (n, e)
        out.append(d)
    return out[0] if j is not None else out


def histogram2d(x, pair, bins=10, range=None, window=None, accepted_only=True, state=False, density=False, groups=None):
    """np.histogram2d(params(c)[a], params(c)[b], bins, range, density) for pair = (a, b), parameter names, counted on the device:
    (H, xedges, yedges) for a chain, a list of them (one per group) for an algo.  range: numpy's [[xmin, xmax], [ymin, ymax]] or None"""
    if int(bins) < 1:
        raise ValueError("`bins` must be positive, when an integer")
    names = ps2s_names(x.m)
    a, b = names.index(pair[0]), names.index(pair[1])
    rg = None
    if range is not None:
        ax = _hist_range(list(range), [0, 1])
        rg = np.tile([0.0, 1.0], (len(names), 1))
        rg[a], rg[b] = ax[0], ax[1]
    _, j, r = _hist_call(x, window, accepted_only, state, groups=groups, bins=1, range=rg, pairs=[(a, b)], bins2=int(bins))
    out = []
    for g in _builtins_range(r["count"].shape[0]):
        for i in (a, b):
            _hist_raise(r["status"][g, i], r["lo"][g, i], r["hi"][g, i], bins, one_d=False)
        H = r["hist2"][g, 0].astype(float)
        xe, ye = r["edges2"][g, a].copy(), r["edges2"][g, b].copy()
        if density:
            s = H.sum()
            H = H / np.diff(xe).reshape(-1, 1)
            H = H / np.diff(ye).reshape(1, -1)
            H /= s
        out.append((H, xe, ye))
    return out[0] if j is not None else out


def _density_call(x, window, accepted_only, state, **kw):
    """(chain index or None, the device's density dict) of a chain (alone in group 0) or of the groups of an algo"""
    if isinstance(x, BGPChain):
        algo, j = x._algo, x._j
        g = np.full(algo._ctx.N, -1, np.int32)
        g[j] = 0
        kw["n_groups"] = 1
    else:
        algo, j = x, None
        g = np.asarray(_default_groups(algo) if kw.get("groups") is None else kw["groups"], np.int32)
    kw.pop("groups", None)
    t0, t1 = (0, algo.i) if window is None else (int(window[0]), int(window[1]))
    sel = "state" if state else "accepted" if accepted_only else "all"
    return j, algo._ctx.density(t0, t1, sel, g, **kw)


def _density_raise(st):
    """a column the device could not summarise (include/smmhip.h: smm_get_density's status)"""
    if st == 1:
        raise ValueError("a draw of the column is not finite")
    if st == 2:
        raise ValueError("the column holds no draw")


def hdi(x, mass=0.94, window=None, accepted_only=True, state=False, groups=None):
    """the highest-density interval of every parameter: the shortest interval holding `mass` of the draws (ArviZ's hdi of a unimodal
    sample; CI and the quantiles are equal-tailed), found on the device (include/smmhip.h: smm_get_density) without downloading the
    history: an OrderedDict name -> (lo, hi) for a chain, a list of them (one per group) for an algo, whose groups default to those of
    rhat / pooled.  window, accepted_only, state as in histogram()"""
    names = ps2s_names(x.m)
    j, r = _density_call(x, window, accepted_only, state, groups=groups, mass=(float(mass),), n_grid=0)
    out = []
    for g in _builtins_range(r["count"].shape[0]):
        d = OrderedDict()
        for i, k in enumerate(names):
            _density_raise(r["status"][g, i])
            d[k] = (float(r["hdi_lo"][0, g, i]), float(r["hdi_hi"][0, g, i]))
        out.append(d)
    return out[0] if j is not None else out


def mode(x, window=None, accepted_only=True, state=False, groups=None):
    """the half-sample mode of every parameter's draws (Bickel & Fruehwirth 2006: the marginal posterior mode, which `best`, the argmin
    of the objective, is not), found on the device (smm_get_density): an OrderedDict name -> mode for a chain, a list of them (one per
    group) for an algo.  Arguments as hdi()"""
    names = ps2s_names(x.m)
    j, r = _density_call(x, window, accepted_only, state, groups=groups, mass=(), n_grid=0)
    out = []
    for g in _builtins_range(r["count"].shape[0]):
        d = OrderedDict()
        for i, k in enumerate(names):
            _density_raise(r["status"][g, i])
            d[k] = float(r["mode"][g, i])
        out.append(d)
    return out[0] if j is not None else out


def kde(x, n_grid=128, bw=None, range=None, window=None, accepted_only=True, state=False, groups=None):
    """the Gaussian kernel density of every parameter's draws on a grid of n_grid points, summed on the device (smm_get_density) without
    downloading the history: an OrderedDict name -> (grid, density, bandwidth) for a chain, a list of them (one per group) for an algo.
    bw: a bandwidth, one per parameter (in order) or name -> bandwidth, None: R's bw.nrd0 of the column; range: [np][2] or
    name -> (lo, hi), None: three bandwidths past the column's extremes.  A column without a usable bandwidth (fewer than two draws)
    or with a grid whose width is not finite raises"""
    names = ps2s_names(x.m)
    if isinstance(bw, dict):
        bw = [bw[k] for k in names]
    j, r = _density_call(x, window, accepted_only, state, groups=groups, mass=(), n_grid=int(n_grid), bw=bw,
                         range=_hist_range(range, names))
    out = []
    for g in _builtins_range(r["count"].shape[0]):
        d = OrderedDict()
        for i, k in enumerate(names):
            _density_raise(r["status"][g, i])
            if r["kde_status"][g, i] == 1:
                raise ValueError("no usable bandwidth for {} (bw = {})".format(k, r["bw"][g, i]))
            if r["kde_status"][g, i] == 2:
                raise ValueError("the grid of {} has a width that is not finite".format(k))
            d[k] = (r["grid"][g, i].copy(), r["density"][g, i].copy(), float(r["bw"][g, i]))
        out.append(d)
    return out[0] if j is not None else out


def _profile_call(x, window, accepted_only, state, **kw):
    """(chain index or None, the device's profile dict) of a chain (alone in group 0) or of the groups of an algo"""
    if isinstance(x, BGPChain):
        algo, j = x._algo, x._j
        g = np.full(algo._ctx.N, -1, np.int32)
        g[j] = 0
        kw["n_groups"] = 1
    else:
        algo, j = x, None
        g = np.asarray(_default_groups(algo) if kw.get("groups") is None else kw["groups"], np.int32)
    kw.pop("groups", None)
    t0, t1 = (0, algo.i) if window is None else (int(window[0]), int(window[1]))
    sel = "state" if state else "accepted" if accepted_only else "all"
    return j, algo._ctx.profile(t0, t1, sel, g, **kw)


def profile(x, bins=20, range=None, window=None, accepted_only=True, state=False, groups=None, moments=True):
    """what the reference's slices draw (doSlices: the objective value and every simulated moment against one parameter), read from the
    run itself on the device (include/smmhip.h: smm_get_profile) without downloading the history and without a further evaluation: an
    OrderedDict parameter name -> OrderedDict(edges [bins + 1], n, n_scored, v_min (the profile: the smallest value in the bin), min_chain,
    min_iter (1-based, 0 = none), theta_at_min (parameter name -> [bins]), v_mean and, with moments, m_mean (moment name -> [bins])) for a
    chain, a list of them (one per group) for an algo, whose groups default to those of rhat / pooled.  bins, range, window,
    accepted_only and state as in histogram, raising where it raises"""
    if int(bins) < 1:
        raise ValueError("`bins` must be positive, when an integer")
    ps, ms = ps2s_names(x.m), ms_names(x.m)
    j, r = _profile_call(x, window, accepted_only, state, groups=groups, bins=int(bins), range=_hist_range(range, ps), moments=bool(moments))
    out = []
    for g in _builtins_range(r["count"].shape[0]):
        d = OrderedDict()
        for i, k in enumerate(ps):
            lo, hi = (r["edges"][g, i, 0], r["edges"][g, i, -1])
            _hist_raise(r["status"][g, i], lo, hi, bins)
            e = OrderedDict(edges=r["edges"][g, i].copy())
            for f in ("n", "n_scored", "v_min", "min_chain", "min_iter"):
                e[f] = r[f][g, i].copy()
            e["theta_at_min"] = OrderedDict((q, r["theta_at_min"][g, i, :, b].copy()) for b, q in enumerate(ps))
            e["v_mean"] = r["v_mean"][g, i].copy()
            if moments:
                e["m_mean"] = OrderedDict((q, r["m_mean"][g, i, :, b].copy()) for b, q in enumerate(ms))
            d[k] = e
        out.append(d)
    return out[0] if j is not None else out


def profile2d(x, pair, bins=20, range=None, window=None, accepted_only=True, state=False, groups=None):
    """the objective surface over pair = (a, b), parameter names, on np.histogram2d's cells (a contour plot next to histogram2d), from
    the device: an OrderedDict(xedges, yedges, n, n_scored, v_min, min_chain, min_iter, v_mean, each [bins][bins]) for a chain, a list of
    them (one per group) for an algo.  range: numpy's [[xmin, xmax], [ymin, ymax]] or None"""
    if int(bins) < 1:
        raise ValueError("`bins` must be positive, when an integer")
    names = ps2s_names(x.m)
    a, b = names.index(pair[0]), names.index(pair[1])
    rg = None
    if range is not None:
        ax = _hist_range(list(range), [0, 1])
        rg = np.tile([0.0, 1.0], (len(names), 1))
        rg[a], rg[b] = ax[0], ax[1]
    j, r = _profile_call(x, window, accepted_only, state, groups=groups, bins=1, range=rg, pairs=[(a, b)], bins2=int(bins), moments=False)
    out = []
    for g in _builtins_range(r["count"].shape[0]):
        for i in (a, b):
            _hist_raise(r["status"][g, i], r["edges2"][g, i, 0], r["edges2"][g, i, -1], bins, one_d=False)
        d = OrderedDict(xedges=r["edges2"][g, a].copy(), yedges=r["edges2"][g, b].copy())
        for f in ("n", "n_scored", "v_min", "min_chain", "min_iter", "v_mean"):
            d[f] = r[f + "2"][g, 0].copy()
        out.append(d)
    return out[0] if j is not None else out


def trace(algo, groups=None, window=None, stride=1, state=True, moments=False, probs=(0.025, 0.5, 0.975)):
    """the population per iteration, reduced across the chains of each group on the device (include/smmhip.h: smm_get_trace) without
    downloading the history: one OrderedDict per group with iter [nt] (0-based), chains, count / n_accepted / n_exchanged / n_failed /
    best_value / best_chain [nt], and mean / var / median (series name -> [nt]) and quantile (series name -> [len(probs)][nt]) of every
    parameter, of "value" and, with moments, of every simulated moment.  window = (t0, t1) (default: the whole run), every stride-th
    iteration of it; state: the chains' state series (the row last accepted) instead of the rows themselves, as params(c,
    accepted_only=False) holds them; groups: a group id per chain (-1 = none), by default those of rhat / pooled"""
    t0, t1 = (0, algo.i) if window is None else (int(window[0]), int(window[1]))
    g = np.asarray(_default_groups(algo) if groups is None else groups, np.int32)
    r = algo._ctx.trace(t0, t1, int(stride), "state" if state else "all", moments, g, tuple(float(p) for p in probs))
    names = list(ps2s_names(algo.m)) + ["value"] + (list(ms_names(algo.m)) if moments else [])
    out = []
    for j in _builtins_range(r["n_chains"].shape[0]):
        d = OrderedDict(iter=r["iter"].copy(), chains=int(r["n_chains"][j]))
        for f in ("count", "n_accepted", "n_exchanged", "n_failed", "best_value", "best_chain"):
            d[f] = r[f][:, j].copy()
        for f in ("mean", "var", "median"):
            d[f] = OrderedDict((k, r[f][:, j, i].copy()) for i, k in enumerate(names))
        d["quantile"] = OrderedDict((k, r["quantile"][:, :, j, i].copy()) for i, k in enumerate(names))
        out.append(d)
    return out


def draws(x, groups=None, window=None, accepted_only=True, state=False, thin=1, max_rows=10000, moments=False):
    """the posterior sample itself, gathered on the device (include/smmhip.h: smm_get_draws) without downloading the history: one
    table per group (a pandas DataFrame when pandas is importable, else an OrderedDict of columns, as history(c)) with the columns
    chain and iter (1-based), value, every parameter and, with moments, every simulated moment.  Every thin-th selected draw of a chain
    is kept and a group with more than max_rows of them is thinned systematically to max_rows.  window = (t0, t1) (default: the whole
    run); state: the chains' state series instead of their accepted draws; groups: a group id per chain (-1 = none), by default those
    of rhat / pooled.  For a chain: that chain's table (alone in group 0)"""
    if isinstance(x, BGPChain):
        algo, j = x._algo, x._j
        g = np.full(algo._ctx.N, -1, np.int32)
        g[j] = 0
        ng = 1
    else:
        algo, j = x, None
        g = np.asarray(_default_groups(algo) if groups is None else groups, np.int32)
        ng = None
    t0, t1 = (0, algo.i) if window is None else (int(window[0]), int(window[1]))
    sel = "state" if state else "accepted" if accepted_only else "all"
    r = algo._ctx.draws(t0, t1, sel, g, int(thin), int(max_rows), bool(moments), n_groups=ng)
    out = []
    for k in _builtins_range(r["count"].shape[0]):
        a, b = int(r["row0"][k]), int(r["row0"][k + 1])
        cols = OrderedDict(chain=r["chain"][a:b].astype(np.int64), iter=r["iter"][a:b].astype(np.int64), value=r["value"][a:b].copy())
        for i, name in enumerate(ps2s_names(algo.m)):
            cols[name] = r["params"][a:b, i].copy()
        if moments:
            for i, name in enumerate(ms_names(algo.m)):
                cols[name] = r["sim_moments"][a:b, i].copy()
        try:
            import pandas as pd
            cols = pd.DataFrame(cols)
        except Exception:  # pragma: no cover
            pass
        out.append(cols)
    return out[0] if j is not None else out


def _moment_stats(algo, groups, window, state, accepted_only, probs, ridge):
    """the device's moment statistics of the groups of algo (smm_get_moment_stats): window = (t0, t1) (default: the whole run)"""
    t0, t1 = (0, algo.i) if window is None else (int(window[0]), int(window[1]))
    g = np.asarray(_default_groups(algo) if groups is None else groups, np.int32)
    sel = "state" if state else "accepted" if accepted_only else "all"
    return algo._ctx.moment_stats(t0, t1, sel, g, tuple(float(p) for p in probs), float(ridge))


def moment_fit(algo, groups=None, window=None, state=True, level=0.95, accepted_only=True):
    """the first table of an SMM paper, from the device (include/smmhip.h: smm_get_moment_stats) without downloading the history: one
    OrderedDict per group with count, chains, status and, keyed by ms_names, data (the data moment), mean and median (of the simulated
    moments over the group's pooled draws), band ([lo, hi] at `level`) and z (the data moment's distance from the posterior predictive
    in its standard deviations).  state: the chains' state series, the MCMC posterior itself (default), else their accepted draws
    (accepted_only) or every row; groups: a group id per chain (-1 = none), by default those of rhat / pooled"""
    q = ((1 - level) / 2, 1 - (1 - level) / 2)
    r = _moment_stats(algo, groups, window, state, accepted_only, q, 0.0)
    names = ms_names(algo.m)
    return [OrderedDict(count=int(r["count"][j]), chains=int(r["n_chains"][j]), status=int(r["status"][j]),
                        data=OrderedDict((k, float(algo.m.moments[k]["value"])) for k in names),
                        mean=OrderedDict((k, float(r["m_mean"][j, i])) for i, k in enumerate(names)),
                        median=OrderedDict((k, float(r["m_median"][j, i])) for i, k in enumerate(names)),
                        band=OrderedDict((k, r["m_quantile"][:, j, i].copy()) for i, k in enumerate(names)),
                        z=OrderedDict((k, float(r["fit_z"][j, i])) for i, k in enumerate(names)))
            for j in _builtins_range(r["count"].shape[0])]


def sensitivity(algo, groups=None, window=None, state=True, ridge=0.0, accepted_only=True):
    """identification and standard errors from the pooled draws, on the device (include/smmhip.h: smm_get_moment_stats): one OrderedDict
    per group with count, chains, status (0 ok; 1 too few rows; 2 a non-finite value; 3 the parameter covariance, 4 J'WJ not positive
    definite), jac (moment name -> parameter name -> dm/dtheta, the regression of the simulated moments on the parameters), sens
    (parameter name -> moment name -> the sensitivity of Andrews, Gentzkow & Shapiro 2017) and se (parameter name -> the sandwich
    standard error, the moments' weights read as the data moments' standard deviations).  groups, window and state as in moment_fit"""
    r = _moment_stats(algo, groups, window, state, accepted_only, (), ridge)
    ps, ms = ps2s_names(algo.m), ms_names(algo.m)
    return [OrderedDict(count=int(r["count"][j]), chains=int(r["n_chains"][j]), status=int(r["status"][j]),
                        jac=OrderedDict((k, OrderedDict((q, float(r["jac"][j, a, b])) for b, q in enumerate(ps))) for a, k in enumerate(ms)),
                        sens=OrderedDict((q, OrderedDict((k, float(r["sens"][j, b, a])) for a, k in enumerate(ms))) for b, q in enumerate(ps)),
                        se=OrderedDict((q, float(r["se"][j, b])) for b, q in enumerate(ps)))
            for j in _builtins_range(r["count"].shape[0])]


def adjusted(algo, groups=None, window=None, state=True, tol=0.2, kernel="epanechnikov", scale=None, ridge=0.0, level=0.95,
             accepted_only=True):
    """the posterior at zero tolerance, from the device (include/smmhip.h: smm_get_adjustment) without downloading the history: the
    local-linear regression adjustment of Beaumont, Zhang & Balding (2002) over each group's pooled draws.  One OrderedDict per group
    with count, chains, status (0 ok; 1 too few rows; 2 a non-finite value; 3 nothing to regress on; 4 the discrepancies' weighted
    covariance not positive definite), n_kept, ess and, keyed by ps2s_names, raw_mean (the weighted, unadjusted estimate), adj_mean,
    adj_sd, band ([lo, hi]: the weighted quantiles of the adjusted draws at `level`) and n_outside (adjusted draws that leave the
    parameter's bounds; nothing is clamped).  tol: the fraction of a group's rows kept, those whose simulated moments lie nearest the
    data; kernel: "uniform" or "epanechnikov"; scale: None (the moments' weights), nm positive values, or "sd": the simulated moments'
    standard deviations over every chain's rows of the window (sqrt(diag cov_mm) of smm_get_moment_stats, fetched first).  groups,
    window and state as in moment_fit"""
    t0, t1 = (0, algo.i) if window is None else (int(window[0]), int(window[1]))
    g = np.asarray(_default_groups(algo) if groups is None else groups, np.int32)
    sel = "state" if state else "accepted" if accepted_only else "all"
    if isinstance(scale, str):
        if scale != "sd":
            raise ValueError("adjusted: scale is None, 'sd' or one value per moment")
        scale = np.sqrt(np.diagonal(algo._ctx.moment_stats(t0, t1, sel, None, (), 0.0)["cov_mm"][0]))
    q = ((1 - level) / 2, 1 - (1 - level) / 2)
    r = algo._ctx.adjustment(t0, t1, sel, g, float(tol), kernel, scale, float(ridge), q)
    ps = ps2s_names(algo.m)
    per = lambda f, j, cast: OrderedDict((k, cast(r[f][j, i])) for i, k in enumerate(ps))
    return [OrderedDict(count=int(r["count"][j]), chains=int(r["n_chains"][j]), status=int(r["status"][j]), n_kept=int(r["n_kept"][j]),
                        ess=float(r["ess"][j]), raw_mean=per("raw_mean", j, float), adj_mean=per("adj_mean", j, float),
                        adj_sd=per("adj_sd", j, float),
                        band=OrderedDict((k, r["adj_quantile"][:, j, i].copy()) for i, k in enumerate(ps)),
                        n_outside=per("n_outside", j, int))
            for j in _builtins_range(r["count"].shape[0])]


def tempered(algo, target=None, per=None, window=None, state=True, level=0.95, accepted_only=True):
    """the target posterior from every temperature, from the device (include/smmhip.h: smm_get_reweighted) without downloading the
    history: every chain's draws importance-reweighted from its own acc_tuners entry to `target` (default: the largest acc_tuners
    entry, the coldest chain's), each chain self-normalised and entering with its own effective sample size.  It assumes that each
    chain's state series targets exp(-acc_tuner v); BGP's exchange moves respect this only approximately.  One OrderedDict per group
    with target, count, n_scored, chains, status (0 ok; 1 too few rows; 2 a non-finite parameter; 3 the weights overflowed), n_kept,
    ess, value_mean and, keyed by ps2s_names, mean, sd (from the weighted population covariance) and band ([lo, hi]: the weighted
    quantiles at `level`), keyed by ms_names m_mean, and cov [np][np].  per: a group id per chain (-1 = none), by default every chain
    in one group; window and state as in moment_fit"""
    t0, t1 = (0, algo.i) if window is None else (int(window[0]), int(window[1]))
    a = float(np.max(algo._acc_tuner)) if target is None else float(target)
    g = None if per is None else np.asarray(per, np.int32)
    sel = "state" if state else "accepted" if accepted_only else "all"
    q = ((1 - level) / 2, 1 - (1 - level) / 2)
    r = algo._ctx.reweighted(t0, t1, sel, g, (a,), q)
    ps, ms = ps2s_names(algo.m), ms_names(algo.m)
    return [OrderedDict(target=a, count=int(r["count"][j]), n_scored=int(r["n_scored"][j]), chains=int(r["n_chains"][j]),
                        status=int(r["status"][0, j]), n_kept=int(r["n_kept"][0, j]), ess=float(r["ess"][0, j]),
                        value_mean=float(r["value_mean"][0, j]),
                        mean=OrderedDict((k, float(r["mean"][0, j, i])) for i, k in enumerate(ps)),
                        sd=OrderedDict((k, float(np.sqrt(r["cov"][0, j, i, i]))) for i, k in enumerate(ps)),
                        band=OrderedDict((k, r["quantile"][:, 0, j, i].copy()) for i, k in enumerate(ps)),
                        m_mean=OrderedDict((k, float(r["m_mean"][0, j, i])) for i, k in enumerate(ms)),
                        cov=r["cov"][0, j].copy())
            for j in _builtins_range(r["count"].shape[0])]


def ladder_logz(algo, window=None, state=True, accepted_only=True):
    """the log normaliser along the temperature ladder, from the device (smm_get_reweighted's chain_logz): the distinct acc_tuners
    entries in ascending order a_0 < a_1 < ..; step k is the estimate of log Z(a_{k+1}) / Z(a_k) from the chains at a_k reweighted to
    their colder neighbour (the mean of their chain_logz, each chain alone in its estimate), and logz their running sum from 0 at a_0:
    the stepping-stone estimate.  Returns OrderedDict(acc_tuner [K], step [K - 1], logz [K], n_chains [K]); a step whose chains have
    no scored row is NaN.  One call with one target per rung (at most 64 rungs above the first)"""
    t0, t1 = (0, algo.i) if window is None else (int(window[0]), int(window[1]))
    sel = "state" if state else "accepted" if accepted_only else "all"
    acc = np.asarray(algo._acc_tuner, float)
    rungs = np.unique(acc)
    if len(rungs) - 1 > 64:
        raise ValueError("ladder_logz: at most 65 distinct acc_tuners entries")
    step = np.empty(max(len(rungs) - 1, 0))
    if len(step):
        r = algo._ctx.reweighted(t0, t1, sel, None, tuple(rungs[1:]), ())
        for k in _builtins_range(len(step)):
            z = r["chain_logz"][k, acc == rungs[k]]
            z = z[~np.isnan(z)]
            step[k] = z.mean() if len(z) else np.nan
    return OrderedDict(acc_tuner=rungs, step=step, logz=np.concatenate([[0.0], np.cumsum(step)]),
                       n_chains=np.array([(acc == a).sum() for a in rungs], np.int64))


def summary(x):
    """summary(c::BGPChain) AlgoBGP.jl:197-206 / summary(m::MAlgoBGP) :541-550"""
    if isinstance(x, MAlgoBGP):
        rows = [summary(c) for c in x.chains]
        try:
            import pandas as pd
            return pd.DataFrame(rows)
        except Exception:  # pragma: no cover
            return rows
    a, j = x._algo, x._j
    st = _stats(x)
    n = int(a.opts["maxiter"])
    # best_val[-1] of the column padded to maxiter: the padding (inf) until the last iteration is done
    best_last = float(a._last_row().best_val[0, j]) if a.i >= n else np.inf
    return OrderedDict(id=x.id, acc_rate=x.accept_rate, perc_exchanged=100.0 * np.int64(st["n_exchanged"][j]) / n,
                       exchanged_most_with=int(st["most_exchanged_with"][j]), best_val=best_last)


# ------------------------------------------------------------------------------------------
# MAlgoBGP: AlgoBGP.jl:497-539
# ------------------------------------------------------------------------------------------
_DEFAULT_OPTS = {"N": 3, "maxiter": 100, "maxtemp": 2, "sigma": 0.05, "sigma_update_steps": 10, "sigma_adjust_by": 0.01,
                 "smpl_iters": 1000, "parallel": False, "min_improve": [0.0] * 3, "acc_tuners": [2.0] * 3}
_IGNORED_OPTS = ("coverage", "mixprob", "acc_tuner", "maxdists")  # read by nothing in the reference either


def _dist_fun_id(f):
    """opts["dist_fun"] (AlgoBGP.jl:494,537: any Julia function of two objective values, default `-`) -> smm_dist_fun_t.
    The device offers a menu: "-" / operator.sub (default), "absdiff" (|a - b|), "reldiff" ((a - b) / |a|), or the ids
    themselves; an arbitrary host callable cannot run inside the exchange kernels."""
    import operator
    if f is None or f is operator.sub or f in ("-", "minus", "sub", A.SMM_DIST_MINUS):
        return A.SMM_DIST_MINUS
    if f in ("absdiff", "abs", A.SMM_DIST_ABSDIFF):
        return A.SMM_DIST_ABSDIFF
    if f in ("reldiff", "relative", A.SMM_DIST_RELDIFF):
        return A.SMM_DIST_RELDIFF
    raise NotImplementedError("dist_fun: the device runs '-' (AlgoBGP.jl:537), 'absdiff' or 'reldiff' (smm_dist_fun_t, include/smmhip.h), "
                              "not an arbitrary host function")


def _chol_opt(L, N, np_):
    """opts["chol_L"]: None (the reference's isotropic kernel), a factor [np][np] or [N][np][np], or "identity": one identity factor per
    chain — the isotropic kernel bit for bit, and a context whose factors adapt_proposal can reshape"""
    if isinstance(L, str):
        if L != "identity":
            raise ValueError('opts["chol_L"]: a factor, None or "identity"')
        return np.ascontiguousarray(np.broadcast_to(np.eye(np_), (N, np_, np_)))
    return L


class MAlgoBGP:
    def __init__(self, m, opts=None, tables=None):
        opts = dict(_DEFAULT_OPTS) if opts is None else opts
        self.m, self.opts, self.i = m, opts, 0
        N = int(opts["N"])
        if N > 1:
            temps = np.linspace(1.0, float(opts["maxtemp"]), N)  # range(1.0, stop=maxtemp, length=N), :508
        else:
            temps = np.ones(1)
        sigma = opts.get("sigma", 0.05) * temps                                   # :518
        self._min_improve = np.asarray(opts.get("min_improve", [0.5] * N), float)[:N]   # :522
        self._acc_tuner = np.asarray(opts.get("acc_tuners", [2.0] * N), float)[:N]      # :523
        if len(self._min_improve) < N or len(self._acc_tuner) < N:
            raise IndexError("min_improve / acc_tuners need one entry per chain (AlgoBGP.jl:522-523)")
        self._dist_fun = _dist_fun_id(opts.get("dist_fun", None))                 # :537
        prob = _flat_problem(m)
        self._flat = dict(sigma_update_steps=int(opts.get("sigma_update_steps", 10)),
                          sigma_adjust_by=float(opts.get("sigma_adjust_by", 0.01)),
                          smpl_iters=int(opts.get("smpl_iters", 1000)))
        bo = BGPOpts(N=N, maxiter=int(opts["maxiter"]), sigma=sigma, acc_tuner=self._acc_tuner,
                     min_improve=self._min_improve, batch_size=opts.get("batch_size", None),
                     seed=int(opts.get("seed", 12)), device=int(opts.get("device", 0)),
                     dist_fun=self._dist_fun,
                     chol_L=_chol_opt(opts.get("chol_L", None), N, len(prob.init)),   # general Gaussian proposals (include/smmhip.h)
                     **self._flat)
        self._prob, self._bopts, self._tables = prob, bo, tables
        self._ctx = hip_context(prob, bo, tables)
        self._invalidate()
        self.chains = [BGPChain(self, j) for j in range(N)]
        self.dist_fun = lambda a, b: a - b

    def __getitem__(self, key):  # algo["N"], AlgoAbstract.jl:13-19
        return self.opts[key]

    def _invalidate(self):
        self._hist = None
        self._st = None
        self._stats = {}
        self._last = None
        self._cov = None
        self._diag = {}
        self._pooled = {}

    def _chain_stats(self, accepted_only, probs):
        key = (self.i, accepted_only, probs)
        if key not in self._stats:
            self._stats[key] = self._ctx.chain_stats(0, self.i, accepted_only, probs)
        return self._stats[key]

    def _last_row(self):
        if self._last is None or self._last[0] != self.i:
            self._last = (self.i, self._ctx.history(self.i - 1, self.i))
        return self._last[1]

    def _history(self):
        if self._hist is None:
            self._hist = self._ctx.history(0, self.i)
        return self._hist

    def _state(self):
        if self._st is None:
            self._st = self._ctx.state()
        return self._st


def computeNextIteration(algo):
    """computeNextIteration!(algo::MAlgoBGP), AlgoBGP.jl:589-640: one iteration of all chains + exchangeMoves!.
    The reference's run! sets algo.i = i before the call (AlgoAbstract.jl:38-45); here algo.i is set to the iteration the
    device has completed, so both `algo.i = i; computeNextIteration(algo)` and a bare call keep chains/history in step."""
    algo._ctx.step(1)
    algo._invalidate()
    algo.i = algo._ctx.state().iter


def run(algo):
    """run!(algo), AlgoAbstract.jl:27-76.  Without per-iteration hooks all remaining iterations are
    enqueued in one call; with opts["save_frequency"] the loop is cut at the save points."""
    t0 = _time.time()
    maxiter = int(algo["maxiter"])
    sf, fn = algo.opts.get("save_frequency"), algo.opts.get("filename")
    while algo.i < maxiter:
        n = maxiter - algo.i
        if sf and fn:
            n = min(n, sf - (algo.i % sf))
        algo._ctx.step(n)
        algo.i += n
        algo._invalidate()
        if sf and fn and algo.i % sf == 0:
            save(algo, fn)
    algo.opts["time"] = round((_time.time() - t0) / 60.0, 1)
    if fn:
        save(algo, fn)
    return algo


def _install_start(algo, r):
    algo._invalidate()
    algo.i = algo._ctx.state().iter
    return r


def set_start(algo, starts):
    """every chain from its own point instead of MProb.initial_value: starts [np][N] (or a list of N parameter dicts), installed on the
    device as every chain's completed iteration 1 (smm_set_population).  Only on a fresh MAlgoBGP (algo.i == 0); afterwards algo.i == 1
    and run / computeNextIteration / history / summary / save / readMalgo / restart behave as after one iteration.  Returns a dict:
    start [np][N], value [N], pick [N], evaluated"""
    if len(starts) and isinstance(starts[0], dict):
        names = ps2s_names(algo.m)
        starts = np.array([[float(d[k]) for d in starts] for k in names])
    return _install_start(algo, algo._ctx.set_population(starts))


def scatter_start(algo, M=64, spread=1.0, keep_init=True):
    """scatter search for every chain's start, on the device (smm_scatter_population; the role of the reference's sobolsearch.jl): M
    candidates per chain in the box of width `spread` (in [0, 1]-space) around MProb.initial_value, the best valid one installed as the
    chain's completed iteration 1; keep_init: initial_value competes and wins ties.  Only on a fresh MAlgoBGP (algo.i == 0); afterwards
    algo.i == 1.  Returns a dict: start [np][N], value [N], pick [N] (-1 = initial_value), evaluated"""
    return _install_start(algo, algo._ctx.scatter_population(M, spread, keep_init))


def polish(algo, npoints, per="chain", tol=1e-5, update=None, maxiter=1000, groups=None, method="slices", **simplex):
    """the estimate: a coordinate search on grids of npoints values (optSlices, slices.jl:114-242) from every chain's best point
    (per="chain") or from the best point of every group of chains (per="group": a group id per chain in `groups`, -1 = none; by default
    those of rhat), all searches at once on the device (smm_opt_slices).  The best points are those chain_stats reports (best_value,
    best_iter over the accepted draws); the chains are not touched.  Returns the searches' results sorted by value, each the reference's
    {"best": {"p", "value"}, "iterations", "converged"} and "start": {"chain" or "group", "p", "value"}.
    method="simplex": Nelder–Mead searches inside the box instead (smm_opt_simplex), for valleys that do not run along the axes; npoints,
    tol, update and maxiter are ignored and the search's options go through keywords (step, adaptive, xatol, fatol, max_iter); the records
    carry "status", "n_eval" and "moves" too.
    method="lm": Levenberg–Marquardt searches on the moments' residuals (smm_opt_lm), in the same way: the keywords are fd_step, lambda0,
    lambda_up, lambda_down, xtol, ftol, gtol, max_iter and max_tries, and the records carry "status", "n_eval", "tries", "ssr" and "lambda"."""
    from .callers import lm_results, opt_results, simplex_results
    if method not in ("slices", "simplex", "lm"):
        raise ValueError('polish: method must be "slices", "simplex" or "lm"')
    if simplex and method == "slices":
        raise TypeError("polish: %s belong to method=\"simplex\" or \"lm\"" % sorted(simplex))
    if per not in ("chain", "group"):
        raise ValueError('polish: per must be "chain" or "group"')
    if algo.i == 0:
        raise ValueError("polish: no completed iteration to start from")
    st = algo._chain_stats(True, ())
    bv, bi = np.asarray(st["best_value"], float), np.asarray(st["best_iter"])
    if per == "chain":
        who = [(j, j) for j in range(len(bv))]
    else:
        g = np.asarray(_default_groups(algo) if groups is None else groups, int)
        who = []
        for gid in sorted(set(int(x) for x in g if x >= 0)):
            members = np.flatnonzero(g == gid)
            ok = members[~np.isnan(bv[members])]
            members = ok if len(ok) else members
            who.append((gid, int(members[np.argmin(bv[members])])))   # (argmin: the lowest chain among equals)
    P = algo._history().params   # [t][np][N]
    starts = np.array([[P[int(bi[j]) - 1, k, j] for _, j in who] for k in range(P.shape[1])], float).reshape(P.shape[1], len(who))
    if method == "simplex":
        res = simplex_results(algo.m, algo._ctx.opt_simplex(starts, **simplex))
    elif method == "lm":
        res = lm_results(algo.m, algo._ctx.opt_lm(starts, **simplex))
    else:
        res = opt_results(algo.m, algo._ctx.opt_slices(starts, npoints, tol, update, maxiter))
    names = ps2s_names(algo.m)
    for s, (r, (label, j)) in enumerate(zip(res, who)):
        r["start"] = {per: label, "p": OrderedDict((k, float(starts[i, s])) for i, k in enumerate(names)), "value": float(bv[j])}
    return sorted(res, key=lambda r: r["best"]["value"])   # (stable: equal values keep the order of their starts)


class ABCPMCResult:
    """what abc_pmc returns: the final weighted particles of smm_abc_pmc under the MProb's parameter names.  raw: the call's arrays"""

    def __init__(self, names, raw):
        self.names, self.raw = list(names), raw
        self.n_kept, self.generations, self.status, self.ess, self.evaluated = (raw[f] for f in ("n_kept", "generations", "status", "ess", "evaluated"))
        self.eps = raw["eps"][:self.generations + 1]
        self.p_acc = raw["p_acc"][:self.generations + 1]

    def mean(self):
        return OrderedDict((k, float(v)) for k, v in zip(self.names, self.raw["mean"]))

    def cov(self):
        return np.array(self.raw["cov"])

    def quantile(self):
        """{name: [the quantile at each of the call's probs]}"""
        return OrderedDict((k, [float(v) for v in self.raw["quantile"][:, i]]) for i, k in enumerate(self.names))

    def draws(self):
        """(theta [np][n_kept], weight [n_kept]): the kept particles and their normalised weights"""
        n = self.n_kept
        return np.array(self.raw["theta"][:, :n]), np.array(self.raw["weight"][:n])


def abc_pmc(algo, n_particles, keep=0.5, max_gen=20, p_acc_min=0.05, scale=2.0, ridge=0.0, probs=(0.025, 0.5, 0.975)):
    """sample without chains: the adaptive population Monte Carlo ABC sampler on the device (smm_abc_pmc; Lenormand, Jabot & Deffuant 2013)
    over the MProb's box with its objective value as the distance; keep is the kept fraction of the particles (or, >= 2, their number).  The
    chains of algo are not touched.  Returns an ABCPMCResult: mean(), cov(), quantile(), draws(), eps, p_acc, status, ess, evaluated"""
    A = int(keep) if keep >= 2 else int(np.floor(keep * n_particles))
    return ABCPMCResult(ps2s_names(algo.m), algo._ctx.abc_pmc(n_particles, A, max_gen, p_acc_min, scale, ridge, probs))


class SobolResult:
    """what global_sensitivity returns: the Sobol' indices of smm_sens_sobol as tables, output name ("value", then the moment names) ->
    parameter name -> index.  raw: the call's arrays"""

    def __init__(self, params, moments, raw):
        self.params, self.outputs, self.raw = list(params), ["value"] + list(moments), raw
        self.n_complete, self.n_invalid, self.evaluated = (raw[f] for f in ("n_complete", "n_invalid", "evaluated"))

    def _table(self, a):
        return OrderedDict((o, OrderedDict((k, float(a[f, i])) for i, k in enumerate(self.params))) for f, o in enumerate(self.outputs))

    def first(self):
        return self._table(self.raw["first"])

    def total(self):
        return self._table(self.raw["total"])

    def interaction(self):
        """total - first: what a parameter moves only together with others"""
        return self._table(self.raw["total"] - self.raw["first"])

    def se(self):
        """{"first": table, "total": table}: the standard errors of the two indices"""
        return {"first": self._table(self.raw["se_first"]), "total": self._table(self.raw["se_total"])}

    def ranking(self, output="value"):
        """the parameters sorted by their total index on `output`, the largest first (a NaN last; equal ones in the MProb's order)"""
        t = self.raw["total"][self.outputs.index(output)]
        return [self.params[i] for i in sorted(range(len(self.params)), key=lambda i: (np.isnan(t[i]), -t[i] if not np.isnan(t[i]) else 0.0))]

    def unidentified(self, tol=1e-3):
        """the parameters whose total index on every moment is at most tol (no moment moves with them anywhere in the box: the global
        form of smm_opt_lm's status 4); a NaN index — a constant moment — counts as not moving"""
        t = self.raw["total"][1:]
        return [k for i, k in enumerate(self.params) if all(not (v > tol) for v in t[:, i])]


def global_sensitivity(algo, n_base=4096, box=None):
    """identify: variance-based global sensitivity on the device (smm_sens_sobol): the Sobol' first-order and total-order indices of the
    objective value and of every simulated moment with respect to every sampled parameter, from n_base (np + 2) evaluations over the
    MProb's box, or over a sub-box around an estimate: box = {name: (lo, hi)}, the parameters it does not name keep their bounds.  The
    chains of algo are not touched.  Returns a SobolResult: first(), total(), interaction(), se(), ranking(output), unidentified(tol)"""
    return _sobol_result(algo.m, algo._ctx, n_base, box)


def _sobol_result(m, ctx, n_base, box):
    names = ps2s_names(m)
    lo = hi = None
    if box is not None:
        unknown = [k for k in box if k not in names]
        if unknown:
            raise KeyError("global_sensitivity: %s are no sampled parameters" % unknown)
        bounds = [box.get(k, (m.params_to_sample[k]["lb"], m.params_to_sample[k]["ub"])) for k in names]
        lo, hi = [float(b[0]) for b in bounds], [float(b[1]) for b in bounds]
    return SobolResult(names, ms_names(m), ctx.sens_sobol(n_base, lo, hi))


def plan_beside(algo):
    """(the run plans each next exchange window beside its persistent kernel, windows planned that way so far, windows planned on the
    main stream): smm_get_plan_beside"""
    return algo._ctx.plan_beside_info()


def set_proposal(algo, L):
    """install proposal factor(s) between iterations (smm_set_proposal): [np][np] on a shared-factor run, [N][np][np] per chain"""
    algo._ctx.set_proposal(L)


def adapt_proposal(algo, window=None, accepted_only=True, min_draws=None, normalize=True, ridge=1e-8):
    """each chain's proposal factor from the covariance of its own draws (adaptive Metropolis, smm_adapt_proposal): window = (t0, t1)
    0-based iterations, default all completed ones.  Needs per-chain factors (opts["chol_L"] = "identity" or [N][np][np]).
    Returns the per-chain status (0 installed; 1 too few draws; 2 non-finite covariance; 3 not positive definite)"""
    t0, t1 = (0, algo.i) if window is None else window
    st = algo._ctx.adapt_proposal(t0, t1, accepted_only, min_draws, normalize, ridge)
    algo._invalidate()
    return st


def save(algo, filename):
    """save(algo, filename), AlgoAbstract.jl:83-88 (JLD2 there; a self-describing .npz here); the installed proposal factor too"""
    h, s = algo._ctx.history(0, algo.i), algo._ctx.state()
    d = {"i": algo.i}
    if algo._ctx.proposal_layout is not None:
        d["chol_L"] = algo._ctx.proposal()
    d.update({"h_" + f: getattr(h, f) for f in A.HistoryBuffers.FIELDS})
    d.update({"s_" + f: getattr(s, f) for f in A.StateBuffers.FIELDS})
    np.savez(filename if filename.endswith(".npz") else filename + ".npz", **d)


def readMalgo(algo, filename):
    """readMalgo, AlgoAbstract.jl:95-102: restore a saved run into an MAlgoBGP built from the same MProb/opts"""
    z = np.load(filename if filename.endswith(".npz") else filename + ".npz")
    i = int(z["i"])
    hb = A.HistoryBuffers(i, algo._ctx.N, algo._ctx.np, algo._ctx.nm)
    sb = A.StateBuffers(algo._ctx.N, algo._ctx.np, algo._ctx.nm)
    for f in A.HistoryBuffers.FIELDS:
        getattr(hb, f)[...] = z["h_" + f]
    for f in A.StateBuffers.FIELDS:
        getattr(sb, f)[...] = z["s_" + f]
    sb.iter = i
    algo._ctx.set_state(sb, hb)
    if "chol_L" in z.files:
        algo._ctx.set_proposal(z["chol_L"])
    algo.i = i
    algo._invalidate()
    return algo


def restart(algo, extra_iter):
    """restart!(algo, extraIter), AlgoBGP.jl:804-884, with clean resume semantics (continue at i+1): the
    history capacity is extended by building a new device context and uploading the saved state."""
    new_maxiter = int(algo.opts["maxiter"]) + int(extra_iter)
    tb = algo._tables
    if tb is not None and tb.covers_iterations() is not None and tb.covers_iterations() < new_maxiter:
        # injected per-iteration randomness (parity runs) was made for the old maxiter: the extended run would read past it
        raise ValueError("restart: the injected randomness tables cover %d iterations, the extended run needs %d — "
                         "build the MAlgoBGP with tables for the whole run, or without tables" % (tb.covers_iterations(), new_maxiter))
    h, s = algo._ctx.history(0, algo.i), algo._ctx.state()
    algo.opts["maxiter"] = new_maxiter
    bo = algo._bopts
    bo.maxiter = new_maxiter
    if algo._ctx.proposal_layout is not None:   # the factor installed now (adapted or set since creation), not the creation-time one
        bo.chol_L = algo._ctx.proposal()
    algo._ctx.close()
    algo._ctx = hip_context(algo._prob, bo, tb)
    s.iter = algo.i
    algo._ctx.set_state(s, h)
    algo._invalidate()
    return run(algo)


# ------------------------------------------------------------------------------------------
# Example drivers: Examples.jl:118-153 (serialNormal), :373-446 (snorm_impl)
# ------------------------------------------------------------------------------------------
def snorm_impl(opts, niter=200, npar=2):
    """snorm_impl(opts, niter; npar), Examples.jl:373-416.  For npar > 2 the reference draws the extra parameters' bounds,
    start values and target moments from Julia's global generator after Random.seed!(12) (:390-405); that stream cannot be
    reproduced here, so the same construction draws from numpy's default_rng(12) (same ranges, different numbers)."""
    pb = OrderedDict()
    pb["p1"] = [0.2, -3, 3]
    pb["p2"] = [-0.2, -20, 20]
    moms = {"name": ["mu1", "mu2"], "value": [-1.0, 10.0], "weight": [1.0, 1.0]}
    if npar > 2:
        rng = np.random.default_rng(12)

        def map_range(a1, a2, b1, b2, x):
            return b1 + (x - a1) * (b2 - b1) / (a2 - a1)
        spaces = np.concatenate([rng.random(2), [4.0 ** -4], (np.linspace(0.25, 0.45, npar - 1) ** -4.0)[::-1]])   # :391
        for j in range(3, npar + 1):
            sp = float(spaces[j - 1])
            pb["p%d" % j] = [map_range(0, 1, -sp, sp, rng.random()), -sp, sp]
            y = map_range(0, 1, -sp, sp, rng.random())
            moms["name"].append("mu%d" % j); moms["value"].append(y); moms["weight"].append(y)
    mprob = MProb()
    addSampledParam(mprob, pb)
    addMoment(mprob, moms)
    addEvalFunc(mprob, objfunc_norm)
    MA = MAlgoBGP(mprob, opts)
    run(MA)
    return MA


def serialNormal(npars=2, niter=200):
    """SMM.serialNormal(npars, niter), Examples.jl:118-153"""
    nchains = 3
    opts = {"N": nchains, "maxiter": niter, "maxtemp": 5, "coverage": 0.02, "smpl_iters": 1000, "parallel": False,
            "min_improve": [0.0] * nchains, "acc_tuners": [20.0, 2.0, 1.0], "animate": False}
    return snorm_impl(opts, niter, npar=npars)
