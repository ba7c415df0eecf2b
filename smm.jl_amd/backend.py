"""Thin object wrapper over the C ABI of include/smmhip.h (libsmmhip.so).
There is deliberately no CPU code path in here."""
import builtins as _builtins
import ctypes as C

import numpy as np

from . import _abi as A


class Problem:
    """Flattened MProb (mprob.jl:29-53): what smm_problem_t carries."""

    def __init__(self, init, lb, ub, mom, w=None, ns=10000, objective_id=A.SMM_OBJ_NORM, obj_params=None):
        self.init = A.f64(init); self.lb = A.f64(lb); self.ub = A.f64(ub)
        self.mom = A.f64(mom)
        self.w = A.f64(np.full(len(self.mom), np.nan) if w is None else w)
        self.np = len(self.init); self.nm = len(self.mom); self.ns = int(ns)
        self.objective_id = int(objective_id)
        self.obj_params = None if obj_params is None else A.f64(obj_params)
        assert len(self.lb) == self.np and len(self.ub) == self.np and len(self.w) == self.nm

    def struct(self):
        p = A.smm_problem_t()
        p.np, p.nm, p.ns, p.objective_id = self.np, self.nm, self.ns, self.objective_id
        p.init, p.lb, p.ub, p.mom, p.w = map(A.dptr, (self.init, self.lb, self.ub, self.mom, self.w))
        p.obj_params = A.dptr(self.obj_params)
        p.n_obj_params = 0 if self.obj_params is None else len(self.obj_params)
        return p


class BGPOpts:
    """Flattened opts Dict of MAlgoBGP (AlgoBGP.jl:505-537). Per-chain vectors are GLOBAL
    (length N_global); the context owns chains [chain_offset, chain_offset+N)."""

    def __init__(self, N, maxiter, sigma, acc_tuner, min_improve, sigma_update_steps=10, sigma_adjust_by=0.01,
                 smpl_iters=1000, batch_size=None, exchange_from_iter=2, seed=12, chain_offset=0, N_global=None,
                 device=0, chol_L=None, dist_fun=0):
        self.N = int(N); self.maxiter = int(maxiter)
        self.N_global = int(N if N_global is None else N_global)
        self.sigma = A.f64(sigma, (self.N_global,)); self.acc_tuner = A.f64(acc_tuner, (self.N_global,))
        self.min_improve = A.f64(min_improve, (self.N_global,))
        self.sigma_update_steps = int(sigma_update_steps); self.sigma_adjust_by = float(sigma_adjust_by)
        self.smpl_iters = int(smpl_iters); self.batch_size = batch_size
        self.exchange_from_iter = int(exchange_from_iter); self.seed = int(seed)
        self.chain_offset = int(chain_offset); self.device = int(device)
        # general Gaussian proposals: a lower-triangular factor [np][np] (shared) or [N_global][np][np] (per chain), see smmhip.h
        self.chol_L = None if chol_L is None else A.f64(chol_L)
        self.dist_fun = int(dist_fun)   # smm_dist_fun_t: 0 `-` (AlgoBGP.jl:537), 1 |a - b|, 2 (a - b) / |a|

    def struct(self, np_):
        o = A.smm_bgp_opts_t()
        o.N, o.maxiter = self.N, self.maxiter
        o.sigma, o.acc_tuner, o.min_improve = map(A.dptr, (self.sigma, self.acc_tuner, self.min_improve))
        o.sigma_update_steps, o.smpl_iters = self.sigma_update_steps, self.smpl_iters
        o.sigma_adjust_by = self.sigma_adjust_by
        o.batch_size = np_ if self.batch_size is None else int(self.batch_size)
        o.exchange_from_iter = self.exchange_from_iter
        o.seed = self.seed
        o.chain_offset, o.N_global, o.device = self.chain_offset, self.N_global, self.device
        o.chol_L = A.dptr(self.chol_L)
        o.dist_fun = self.dist_fun
        o.chol_per_chain = 0 if self.chol_L is None or self.chol_L.ndim == 2 else 1
        if self.chol_L is not None:
            want = (np_, np_) if self.chol_L.ndim == 2 else (self.N_global, np_, np_)
            if self.chol_L.shape != want:
                raise ValueError("chol_L must be [np][np] or [N_global][np][np]")
        return o


class Tables:
    """Injected randomness (smm_tables_t). All optional."""

    def __init__(self, probs_acc=None, prop_normals=None, pairs=None, Z=None):
        self.probs_acc = None if probs_acc is None else A.f64(probs_acc)          # [T][N]
        self.prop_normals = None if prop_normals is None else A.f64(prop_normals)  # [T][K][np][N]
        self.pairs = None if pairs is None else np.ascontiguousarray(pairs, dtype=np.int32)  # [T][K][2]
        self.Z = None if Z is None else A.f64(Z)                                   # [nm][ns]

    def check(self, problem, opts):
        """the C ABI reads T x ... entries out of these host arrays (include/smmhip.h, smm_tables_t): shapes that do not cover
        opts.maxiter iterations of this shard would be a host over-read, so they are refused here"""
        T, N, npar = opts.maxiter, opts.N, problem.np
        if self.probs_acc is not None and self.probs_acc.shape != (T, N):
            raise ValueError("Tables.probs_acc must be [maxiter][N] = %s, got %s" % ((T, N), self.probs_acc.shape))
        if self.prop_normals is not None and (self.prop_normals.ndim != 4 or self.prop_normals.shape[0] != T or
                                              self.prop_normals.shape[1] < 1 or self.prop_normals.shape[2:] != (npar, N)):
            raise ValueError("Tables.prop_normals must be [maxiter][tries][np][N] = (%d, K, %d, %d), got %s"
                             % (T, npar, N, self.prop_normals.shape))
        if self.pairs is not None and (self.pairs.ndim != 3 or self.pairs.shape[0] != T or self.pairs.shape[2] != 2):
            raise ValueError("Tables.pairs must be [maxiter][n_pairs][2] with maxiter = %d, got %s" % (T, self.pairs.shape))
        if self.Z is not None and self.Z.shape != (problem.nm, problem.ns):
            raise ValueError("Tables.Z must be [nm][ns] = %s, got %s" % ((problem.nm, problem.ns), self.Z.shape))

    def covers_iterations(self):
        """iterations the per-iteration tables were made for (None: nothing injected per iteration)"""
        ts = [a.shape[0] for a in (self.probs_acc, self.prop_normals, self.pairs) if a is not None]
        return min(ts) if ts else None

    def struct(self):
        t = A.smm_tables_t()
        t.probs_acc = A.dptr(self.probs_acc)
        t.prop_normals = A.dptr(self.prop_normals)
        t.prop_tries = 0 if self.prop_normals is None else self.prop_normals.shape[1]
        t.pairs = None if self.pairs is None else self.pairs.ctypes.data_as(A.c_int32_p)
        t.n_pairs = 0 if self.pairs is None else self.pairs.shape[1]
        t.Z = A.dptr(self.Z)
        return t


class BGPContext:
    """One device context of libsmmhip.so = the chains of one MAlgoBGP shard."""

    _p = "smm_"   # symbol prefix of the C ABI

    def __init__(self, problem, opts, tables=None):
        self._lib = A.load()
        self._create(problem, opts, tables)

    def _create(self, problem, opts, tables):
        self.problem, self.opts = problem, opts
        self.tables = tables
        self._ctx = C.c_void_p()
        ps, os_ = problem.struct(), opts.struct(problem.np)
        if tables is not None:
            tables.check(problem, opts)
        ts = tables.struct() if tables is not None else None
        rc = self._fn("ctx_create")(C.byref(ps), C.byref(os_), C.byref(ts) if ts is not None else None,
                                    C.byref(self._ctx))
        if rc != 0:
            msg = self._fn("last_error")(None)
            raise A.SMMHipError(rc, msg.decode() if msg else "ctx_create failed")
        self.N, self.np, self.nm = opts.N, problem.np, problem.nm
        # the proposal factor's layout, fixed at creation like the sizes above (the caller may reuse opts for other contexts):
        # None (isotropic), "shared" [np][np] or "per_chain" [N][np][np] (the local chains)
        self.proposal_layout = None if opts.chol_L is None else ("shared" if opts.chol_L.ndim == 2 else "per_chain")

    def _fn(self, name):
        return getattr(self._lib, self._p + name)

    def _check(self, rc):
        if rc != 0:
            msg = self._fn("last_error")(self._ctx)
            raise A.SMMHipError(rc, msg.decode() if msg else "")

    def close(self):
        if self._ctx:
            self._fn("ctx_destroy")(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- the path ---------------------------------------------------------------------
    def step(self, n_iters=1):
        self._check(self._fn("bgp_step")(self._ctx, int(n_iters)))

    def step_async(self, n_iters=1):
        self._check(self._fn("bgp_step_async")(self._ctx, int(n_iters)))

    def sync(self):
        self._check(self._fn("sync")(self._ctx))

    def local_step(self):
        self._check(self._fn("bgp_local_step")(self._ctx))

    def record_doubles(self):
        return self._fn("bgp_record_doubles")(self._ctx)

    def export_records_dev(self, ptr):
        self._check(self._fn("bgp_export_records_dev")(self._ctx, C.c_void_p(ptr)))

    def exchange_dev(self, ptr):
        self._check(self._fn("bgp_exchange_dev")(self._ctx, C.c_void_p(ptr)))

    # the values form of the exchange phase (include/smmhip.h): device pointers
    def a2a_capacity(self):
        return self._fn("bgp_a2a_capacity")(self._ctx)

    def export_values_dev(self, ptr):
        self._check(self._fn("bgp_export_values_dev")(self._ctx, C.c_void_p(ptr)))

    def a2a_pack_dev(self, vals_all_ptr, send_ptr):
        self._check(self._fn("bgp_a2a_pack_dev")(self._ctx, C.c_void_p(vals_all_ptr), C.c_void_p(send_ptr)))

    def a2a_apply_dev(self, recv_ptr):
        self._check(self._fn("bgp_a2a_apply_dev")(self._ctx, C.c_void_p(recv_ptr)))

    def sharded_step(self, prev_ptr, next_ptr):
        """fused sharded iteration (include/smmhip.h): prev/next are device pointers of [N_global][RW] buffers"""
        self._check(self._fn("bgp_sharded_step")(self._ctx, C.c_void_p(prev_ptr or 0), C.c_void_p(next_ptr)))

    def sharded_finish(self, ptr):
        self._check(self._fn("bgp_sharded_finish")(self._ctx, C.c_void_p(ptr or 0)))

    # the p2p form of the sharded iteration (include/smmhip.h): windows mapped by every rank, no collective
    def p2p_init(self):
        """allocate this rank's window; returns (ipc handle bytes, device pointer)"""
        h = C.create_string_buffer(A.SMM_P2P_HANDLE_BYTES)
        w = C.c_void_p()
        self._check(self._fn("bgp_p2p_init")(self._ctx, h, C.byref(w)))
        return bytes(h.raw), int(w.value)

    def p2p_attach(self, rank, handle=None, window=None):
        """rank's window: by IPC handle (another process) or device pointer (a context of this process)"""
        hb = C.create_string_buffer(handle, A.SMM_P2P_HANDLE_BYTES) if handle is not None else None
        self._check(self._fn("bgp_p2p_attach")(self._ctx, int(rank), hb, C.c_void_p(window) if window is not None else None))

    def p2p_step(self, n_iters=1):
        self._check(self._fn("bgp_p2p_step")(self._ctx, int(n_iters)))

    def p2p_finish(self):
        self._check(self._fn("bgp_p2p_finish")(self._ctx))

    def stream(self):
        return self._fn("stream")(self._ctx)

    def eval_batch(self, params):
        params = A.f64(params)
        assert params.shape[0] == self.np
        M = params.shape[1]
        value = np.empty(M); simM = np.empty((self.nm, M)); status = np.empty(M, np.int8)
        self._check(self._fn("eval_batch")(self._ctx, A.dptr(params), M, A.dptr(value), A.dptr(simM),
                                           status.ctypes.data_as(A.c_int8_p)))
        return value, simM, status

    def eval_batch_noseed(self, params, base_seed):
        """objfunc_norm with noseed=true (ObjExamples.jl:71-75): evaluation i draws its own shocks (base_seed + i); likewise a user
        objective registered with rng=True (its stream keyed by base_seed + i)"""
        params = A.f64(params)
        assert params.shape[0] == self.np
        M = params.shape[1]
        value = np.empty(M); simM = np.empty((self.nm, M)); status = np.empty(M, np.int8)
        self._check(self._fn("eval_batch_noseed")(self._ctx, A.dptr(params), M, C.c_uint64(int(base_seed)), A.dptr(value),
                                                  A.dptr(simM), status.ctypes.data_as(A.c_int8_p)))
        return value, simM, status

    # --- read back --------------------------------------------------------------------
    def _t1(self, t1):
        """a window's end: by default the iterations completed so far"""
        return self.state().iter if t1 is None else t1

    def _groups(self, who, groups, n_groups=None, default=1):
        """who's groups argument as the ABI takes it: (the int32 vector the pointer points into, or None; the pointer, or None; the number
        of groups: n_groups, else groups.max() + 1, else `default` without a vector)"""
        g = None if groups is None else np.ascontiguousarray(groups, np.int32)
        if g is not None and g.shape != (self.N,):
            raise ValueError("%s: groups needs one entry per chain, got shape %s" % (who, g.shape))
        ng = (default if g is None else (int(g.max()) + 1 if len(g) else 0)) if n_groups is None else int(n_groups)
        return g, (g.ctypes.data_as(A.c_int32_p) if g is not None else None), ng

    _SELECT = {"all": 0, "accepted": 1, "state": 2}

    def _select(self, select):
        return self._SELECT[select] if isinstance(select, str) else int(select)

    @staticmethod
    def _out(struct_t, arrays, skip=()):
        """a call's out-struct pointing at the arrays of its fields' names, but for the fields to skip (left NULL: not asked for)"""
        s = struct_t()
        for f, t in struct_t._fields_:
            if f in arrays and f not in skip:
                setattr(s, f, arrays[f].ctypes.data_as(t))
        return s

    def history(self, t0=0, t1=None):
        t1 = self._t1(t1)
        hb = A.HistoryBuffers(t1 - t0, self.N, self.np, self.nm)
        hs = hb.struct()
        self._check(self._fn("get_history")(self._ctx, t0, t1, C.byref(hs)))
        return hb

    def chain_stats(self, t0=0, t1=None, accepted_only=True, probs=()):
        """summaries of every local chain over iterations [t0, t1), reduced on the device (smm_get_chain_stats, include/smmhip.h):
        a dict of numpy arrays count [N], mean / median [np][N], quantile [len(probs)][np][N], best_value, best_iter, n_exchanged,
        most_exchanged_with [N].  accepted_only: the accepted draws only, as params(c)"""
        t1 = self._t1(t1)
        p = A.f64(probs).reshape(-1)
        N, np_ = self.N, self.np
        r = dict(count=np.empty(N, np.int32), mean=np.empty((np_, N)), median=np.empty((np_, N)), quantile=np.empty((len(p), np_, N)),
                 best_value=np.empty(N), best_iter=np.empty(N, np.int32), n_exchanged=np.empty(N, np.int32),
                 most_exchanged_with=np.empty(N, np.int32))
        s = self._out(A.smm_chain_stats_t, r, () if len(p) else ("quantile",))
        self._check(self._fn("get_chain_stats")(self._ctx, int(t0), int(t1), int(bool(accepted_only)), A.dptr(p) if len(p) else None,
                                                len(p), C.byref(s)))
        return r

    def chain_cov(self, t0=0, t1=None, accepted_only=True, unit_space=False):
        """covariance of every local chain's selected draws over iterations [t0, t1), on the device (smm_get_chain_cov,
        include/smmhip.h): (count [N], mean [np][N], cov [np][np][N]); unit_space: the draws mapped to [0, 1] first"""
        t1 = self._t1(t1)
        N, np_ = self.N, self.np
        count, mean, cov = np.empty(N, np.int32), np.empty((np_, N)), np.empty((np_, np_, N))
        self._check(self._fn("get_chain_cov")(self._ctx, int(t0), int(t1), int(bool(accepted_only)), int(bool(unit_space)),
                                              count.ctypes.data_as(A.c_int32_p), A.dptr(mean), A.dptr(cov)))
        return count, mean, cov

    def chain_diag(self, t0=0, t1=None, max_lag=None, n_acf=0, groups=None):
        """convergence diagnostics of every local chain over iterations [t0, t1), on the device (smm_get_chain_diag,
        include/smmhip.h): a dict of numpy arrays accept_rate [N], ess / status [S][N] (S = np + 1: the parameters, then the objective
        value), acf [n_acf][S][N] and, with groups (an int per chain, -1 = none), rhat [n_groups][S], n_groups = groups.max() + 1.
        max_lag defaults to t1 - t0 - 1: the whole of Geyer's sequence, the device stopping where it is truncated"""
        t1 = self._t1(t1)
        max_lag = t1 - t0 - 1 if max_lag is None else max_lag
        N, S = self.N, self.np + 1
        g, gp, ng = self._groups("chain_diag", groups, default=0)
        r = dict(accept_rate=np.empty(N), ess=np.empty((S, N)), status=np.empty((S, N), np.int32), acf=np.empty((max(int(n_acf), 0), S, N)),
                 rhat=np.empty((max(ng, 0), S)))
        s = self._out(A.smm_chain_diag_t, r, (() if n_acf > 0 else ("acf",)) + (() if ng > 0 else ("rhat",)))
        self._check(self._fn("get_chain_diag")(self._ctx, int(t0), int(t1), int(max_lag), int(n_acf), gp, ng, C.byref(s)))
        return r

    def rank_diag(self, t0=0, t1=None, max_lag=None, n_bins=20, groups=None, n_groups=None):
        """rank-normalised diagnostics of groups of local chains over iterations [t0, t1), on the device (smm_get_rank_diag,
        include/smmhip.h): a dict of numpy arrays rhat_rank / rhat_bulk / rhat_folded / ess_bulk / ess_tail / ess_mean [n_groups][S]
        (S = np + 1: the parameters, then the objective value), status [4][n_groups][S] (bulk, folded, tail, mean) and rank_hist
        [n_bins][S][N], each chain's pooled ranks binned (the rank plot; n_bins = 0: none).  groups: an int per chain (-1 = none),
        n_groups by default groups.max() + 1, None: every local chain in one group.  max_lag defaults to (t1 - t0) // 2 - 1: the whole of
        Geyer's sequence, the device stopping where it is truncated"""
        t1 = self._t1(t1)
        t0, t1, n_bins = int(t0), int(t1), int(n_bins)
        if t1 - t0 < 8:
            raise ValueError("rank_diag: the window must hold at least 8 iterations, got [%d, %d)" % (t0, t1))
        h = (t1 - t0) // 2
        max_lag = h - 1 if max_lag is None else int(max_lag)
        if not 1 <= max_lag <= h - 1:
            raise ValueError("rank_diag: max_lag must lie in [1, %d], got %d" % (h - 1, max_lag))
        if n_bins < 0:
            raise ValueError("rank_diag: n_bins must be >= 0, got %d" % n_bins)
        g, gp, ng = self._groups("rank_diag", groups, n_groups)
        if ng < 1:
            raise ValueError("rank_diag: n_groups must be at least 1, got %d" % ng)
        N, S = self.N, self.np + 1
        r = {f: np.empty((ng, S)) for f in ("rhat_rank", "rhat_bulk", "rhat_folded", "ess_bulk", "ess_tail", "ess_mean")}
        r.update(status=np.empty((4, ng, S), np.int32), rank_hist=np.empty((n_bins, S, N), np.int64))
        s = self._out(A.smm_rank_diag_t, r, () if n_bins > 0 else ("rank_hist",))
        self._check(self._fn("get_rank_diag")(self._ctx, t0, t1, max_lag, n_bins, gp, ng, C.byref(s)))
        return r

    def group_stats(self, t0=0, t1=None, accepted_only=True, groups=None, probs=(), n_groups=None):
        """the pooled draws of groups of local chains over iterations [t0, t1), summarised on the device (smm_get_group_stats,
        include/smmhip.h): a dict of numpy arrays count / n_chains [n_groups], mean / median [n_groups][np], quantile
        [len(probs)][n_groups][np], cov [n_groups][np][np].  groups: an int per chain (-1 = none), n_groups by default groups.max() + 1;
        None: every local chain in one group"""
        t1 = self._t1(t1)
        p = A.f64(probs).reshape(-1)
        np_ = self.np
        g, gp, ng = self._groups("group_stats", groups, n_groups)
        r = dict(count=np.empty(ng, np.int64), n_chains=np.empty(ng, np.int32), mean=np.empty((ng, np_)), median=np.empty((ng, np_)),
                 quantile=np.empty((len(p), ng, np_)), cov=np.empty((ng, np_, np_)))
        s = self._out(A.smm_group_stats_t, r, () if len(p) else ("quantile",))
        self._check(self._fn("get_group_stats")(self._ctx, int(t0), int(t1), int(bool(accepted_only)), gp, ng,
                                                A.dptr(p) if len(p) else None, len(p), C.byref(s)))
        return r

    def histogram(self, t0=0, t1=None, select="accepted", groups=None, bins=10, range=None, pairs=(), bins2=None, n_groups=None):
        """histograms of the draws of groups of local chains over iterations [t0, t1), counted on the device (smm_get_histogram,
        include/smmhip.h): a dict of numpy arrays count [n_groups], status / lo / hi [n_groups][np], edges [n_groups][np][bins + 1],
        hist [n_groups][np][bins] and, with pairs, edges2 [n_groups][np][bins2 + 1], hist2 [n_groups][len(pairs)][bins2][bins2].
        select: "all", "accepted" (params(c, accepted_only)) or "state" (the chain's state series); groups: an int per chain (-1 = none),
        n_groups by default groups.max() + 1, None: every local chain in one group; range: [np][2] or a dict parameter index -> (lo, hi)
        naming every parameter, None: each group's own min and max; pairs: (j, k) parameter indexes; bins2 defaults to bins"""
        t1 = self._t1(t1)
        np_ = self.np
        sel = self._select(select)
        g, gp, ng = self._groups("histogram", groups, n_groups)
        if isinstance(range, dict):
            if sorted(range) != list(_builtins.range(np_)):
                raise ValueError("histogram: a range dict names every parameter index 0 .. np-1")
            range = [range[k] for k in _builtins.range(np_)]
        rg = None if range is None else np.ascontiguousarray(range, np.float64).reshape(np_, 2)
        pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        b, b2 = int(bins), int(bins if bins2 is None else bins2)
        npr = len(pr)
        r = dict(count=np.empty(ng, np.int64), status=np.empty((ng, np_), np.int32), lo=np.empty((ng, np_)), hi=np.empty((ng, np_)),
                 edges=np.empty((ng, np_, max(b, 0) + 1)), hist=np.empty((ng, np_, max(b, 0)), np.int64))
        if npr:
            r.update(edges2=np.empty((ng, np_, max(b2, 0) + 1)), hist2=np.empty((ng, npr, max(b2, 0), max(b2, 0)), np.int64))
        s = self._out(A.smm_histogram_t, r)
        self._check(self._fn("get_histogram")(self._ctx, int(t0), int(t1), sel, gp, ng, b, A.dptr(rg) if rg is not None else None,
                                              pr.ctypes.data_as(A.c_int32_p) if npr else None, npr, b2, C.byref(s)))
        return r

    def density(self, t0=0, t1=None, select="accepted", groups=None, mass=(0.94,), n_grid=128, range=None, bw=None, n_groups=None):
        """highest-density intervals, half-sample modes and Gaussian kernel densities of the draws of groups of local chains over
        iterations [t0, t1), on the device (smm_get_density, include/smmhip.h): a dict of numpy arrays count [n_groups], status / mode
        [n_groups][np], hdi_lo / hdi_hi [len(mass)][n_groups][np] and, with n_grid > 0, bw / kde_status / kde_mode [n_groups][np], grid /
        density [n_groups][np][n_grid].  select, groups, n_groups and range as in histogram(); mass: the intervals' masses in (0, 1];
        bw: a bandwidth per parameter, None: R's bw.nrd0 of each column; range None: three bandwidths past each column's extremes"""
        t1 = self._t1(t1)
        np_ = self.np
        sel = self._select(select)
        g, gp, ng = self._groups("density", groups, n_groups)
        if isinstance(range, dict):
            if sorted(range) != list(_builtins.range(np_)):
                raise ValueError("density: a range dict names every parameter index 0 .. np-1")
            range = [range[k] for k in _builtins.range(np_)]
        rg = None if range is None else np.ascontiguousarray(range, np.float64).reshape(np_, 2)
        bwv = None if bw is None else np.ascontiguousarray(np.broadcast_to(np.asarray(bw, np.float64), (np_,)))
        m = A.f64(mass).reshape(-1)
        ngr = int(n_grid)
        r = dict(count=np.empty(ng, np.int64), status=np.empty((ng, np_), np.int32), mode=np.empty((ng, np_)), bw=np.empty((ng, np_)),
                 kde_status=np.empty((ng, np_), np.int32))
        if len(m):
            r.update(hdi_lo=np.empty((len(m), ng, np_)), hdi_hi=np.empty((len(m), ng, np_)))
        if ngr != 0:
            r.update(kde_mode=np.empty((ng, np_)), grid=np.empty((ng, np_, max(ngr, 0))), density=np.empty((ng, np_, max(ngr, 0))))
        s = self._out(A.smm_density_t, r)
        self._check(self._fn("get_density")(self._ctx, int(t0), int(t1), sel, gp, ng, A.dptr(m) if len(m) else None, len(m), ngr,
                                            A.dptr(rg) if rg is not None else None, A.dptr(bwv) if bwv is not None else None, C.byref(s)))
        return r

    def derived(self, transform, t0=0, t1=None, select="accepted", groups=None, probs=(), tdata=(), n_groups=None):
        """the posterior of a user function of each draw, over the pooled rows of groups of local chains over iterations [t0, t1), on
        the device (smm_get_derived, include/smmhip.h): a dict of numpy arrays count / n_chains [n_groups], n_nonfinite / mean / median
        [n_groups][Q], quantile [len(probs)][n_groups][Q], cov [n_groups][Q][Q], Q = the transform's n_out.  transform: what
        user_transform() returned; select, groups and n_groups as in histogram(); tdata: the call's vector for the function"""
        t1 = self._t1(t1)
        sel = self._select(select)
        g, gp, ng = self._groups("derived", groups, n_groups)
        p, td = A.f64(probs).reshape(-1), A.f64(tdata).reshape(-1)
        Q = transform.n_out
        r = dict(count=np.empty(ng, np.int64), n_chains=np.empty(ng, np.int32), n_nonfinite=np.empty((ng, Q), np.int64),
                 mean=np.empty((ng, Q)), median=np.empty((ng, Q)), quantile=np.empty((len(p), ng, Q)), cov=np.empty((ng, Q, Q)))
        s = self._out(A.smm_derived_t, r, () if len(p) else ("quantile",))
        self._check(self._fn("get_derived")(self._ctx, transform.handle(self._lib), int(t0), int(t1), sel, gp, ng,
                                            A.dptr(td) if len(td) else None, len(td), A.dptr(p) if len(p) else None, len(p), C.byref(s)))
        return r

    def trace(self, t0=0, t1=None, stride=1, select="state", moments=False, groups=None, probs=(), n_groups=None):
        """the population per iteration over the kept iterations t0, t0 + stride, .. < t1, reduced across the chains of each group on the
        device (smm_get_trace, include/smmhip.h): a dict of numpy arrays iter [nt], n_chains [n_groups], count / n_accepted / n_exchanged /
        n_failed / best_value / best_chain [nt][n_groups], mean / var / median [nt][n_groups][S], quantile [len(probs)][nt][n_groups][S];
        the S series are the parameters, the objective value and, with moments, the simulated moments.  select: "all", "accepted" or
        "state" (the chain's state series); groups: an int per chain (-1 = none), n_groups by default groups.max() + 1, None: every
        local chain in one group"""
        t1 = self._t1(t1)
        p = A.f64(probs).reshape(-1)
        sel = self._select(select)
        g, gp, ng = self._groups("trace", groups, n_groups)
        st = int(stride)
        nt = max(0, -(-(int(t1) - int(t0)) // st)) if st >= 1 else 0
        G, S = max(ng, 0), self.np + 1 + (self.nm if moments else 0)
        r = dict(iter=np.empty(nt, np.int32), n_chains=np.empty(G, np.int32), count=np.empty((nt, G), np.int32),
                 n_accepted=np.empty((nt, G), np.int32), n_exchanged=np.empty((nt, G), np.int32), n_failed=np.empty((nt, G), np.int32),
                 mean=np.empty((nt, G, S)), var=np.empty((nt, G, S)), median=np.empty((nt, G, S)), quantile=np.empty((len(p), nt, G, S)),
                 best_value=np.empty((nt, G)), best_chain=np.empty((nt, G), np.int32))
        s = self._out(A.smm_trace_t, r, () if len(p) else ("quantile",))
        self._check(self._fn("get_trace")(self._ctx, int(t0), int(t1), st, sel, int(bool(moments)), gp, ng,
                                          A.dptr(p) if len(p) else None, len(p), C.byref(s)))
        return r

    def draws(self, t0=0, t1=None, select=1, groups=None, thin=1, max_rows=10000, moments=True, n_groups=None):
        """the posterior sample itself: thinned draws of groups of local chains over iterations [t0, t1), gathered on the device
        (smm_get_draws, include/smmhip.h): a dict of numpy arrays count / n_chains [n_groups], row0 [n_groups + 1] (group g's rows are
        row0[g] .. row0[g + 1]), params [R][np], value [R], sim_moments [R][nm] (moments=False: [0][nm], not read), chain / iter /
        src_iter [R] (1-based; chain is the global id).  select: 0 / "all", 1 / "accepted" or 2 / "state"; every thin-th selected row of
        a chain is kept, and a group with more than max_rows kept rows is thinned systematically to max_rows.  groups: an int per chain
        (-1 = none), n_groups by default groups.max() + 1, None: every local chain in one group.  A sizing call, then the row call"""
        t0, t1 = int(t0), int(self._t1(t1))
        sel, thin, max_rows = self._select(select), int(thin), int(max_rows)
        g, gp, ng = self._groups("draws", groups, n_groups)
        G = max(ng, 0)
        r = dict(count=np.zeros(G, np.int64), n_chains=np.zeros(G, np.int32), row0=np.zeros(G + 1, np.int64))
        fn = self._fn("get_draws")
        self._check(fn(self._ctx, t0, t1, sel, gp, ng, thin, max_rows, 0, C.byref(self._out(A.smm_draws_t, r))))
        R = int(r["row0"][G])
        r.update(params=np.empty((R, self.np)), value=np.empty(R), sim_moments=np.empty((R if moments else 0, self.nm)),
                 chain=np.empty(R, np.int32), iter=np.empty(R, np.int32), src_iter=np.empty(R, np.int32))
        s = self._out(A.smm_draws_t, r, () if moments else ("sim_moments",))
        self._check(fn(self._ctx, t0, t1, sel, gp, ng, thin, max_rows, R, C.byref(s)))
        return r

    def moment_stats(self, t0=0, t1=None, select="state", groups=None, probs=(), ridge=0.0, n_groups=None):
        """the simulated moments of groups of local chains over iterations [t0, t1), on the device (smm_get_moment_stats,
        include/smmhip.h): a dict of numpy arrays count / n_chains / status [n_groups], p_mean / se [n_groups][np], m_mean / m_median /
        fit_z [n_groups][nm], m_quantile [len(probs)][n_groups][nm], cov_pp [n_groups][np][np], cov_pm / sens [n_groups][np][nm], cov_mm
        [n_groups][nm][nm], jac [n_groups][nm][np].  select: 0 / "all", 1 / "accepted" or 2 / "state"; groups: an int per chain
        (-1 = none), n_groups by default groups.max() + 1, None: every local chain in one group; ridge: the relative ridge on the
        diagonal of the parameter covariance before it is factored"""
        t1 = self._t1(t1)
        p = A.f64(probs).reshape(-1)
        np_, nm = self.np, self.nm
        sel = self._select(select)
        g, gp, ng = self._groups("moment_stats", groups, n_groups)
        G = max(ng, 0)
        r = dict(count=np.empty(G, np.int64), n_chains=np.empty(G, np.int32), status=np.empty(G, np.int32), p_mean=np.empty((G, np_)),
                 m_mean=np.empty((G, nm)), m_median=np.empty((G, nm)), m_quantile=np.empty((len(p), G, nm)), cov_pp=np.empty((G, np_, np_)),
                 cov_pm=np.empty((G, np_, nm)), cov_mm=np.empty((G, nm, nm)), fit_z=np.empty((G, nm)), jac=np.empty((G, nm, np_)),
                 sens=np.empty((G, np_, nm)), se=np.empty((G, np_)))
        s = self._out(A.smm_moment_stats_t, r, () if len(p) else ("m_quantile",))
        self._check(self._fn("get_moment_stats")(self._ctx, int(t0), int(t1), sel, gp, ng, A.dptr(p) if len(p) else None, len(p),
                                                 float(ridge), C.byref(s)))
        return r

    ADJUST_KERNELS = {"uniform": 0, "epanechnikov": 1}

    def adjustment(self, t0=0, t1=None, select="state", groups=None, tol=0.2, kernel="epanechnikov", scale=None, ridge=0.0, probs=(),
                   n_groups=None):
        """the regression-adjusted posterior of groups of local chains over iterations [t0, t1), on the device (smm_get_adjustment,
        include/smmhip.h: Beaumont, Zhang & Balding's local-linear adjustment): a dict of numpy arrays count / n_chains / status /
        n_kept / bandwidth / sum_w / ess [n_groups], x_mean [n_groups][nm], raw_mean / adj_mean / adj_sd / n_outside [n_groups][np],
        beta [n_groups][nm][np], adj_quantile [len(probs)][n_groups][np].  select and groups as in moment_stats; tol: the fraction of a
        group's rows kept; kernel: 0 / "uniform" or 1 / "epanechnikov"; scale: None (the moments' weights) or nm positive values;
        ridge: the relative ridge on the diagonal of the discrepancies' weighted pair sums before they are factored"""
        t1 = self._t1(t1)
        p = A.f64(probs).reshape(-1)
        np_, nm = self.np, self.nm
        sel = self._select(select)
        kern = self.ADJUST_KERNELS[kernel] if isinstance(kernel, str) else int(kernel)
        sc = None if scale is None else A.f64(scale).reshape(-1)
        if sc is not None and len(sc) != nm:
            raise ValueError("adjustment: scale needs one value per moment")
        g, gp, ng = self._groups("adjustment", groups, n_groups)
        G = max(ng, 0)
        r = dict(count=np.empty(G, np.int64), n_chains=np.empty(G, np.int32), status=np.empty(G, np.int32), n_kept=np.empty(G, np.int64),
                 bandwidth=np.empty(G), sum_w=np.empty(G), ess=np.empty(G), x_mean=np.empty((G, nm)), raw_mean=np.empty((G, np_)),
                 beta=np.empty((G, nm, np_)), adj_mean=np.empty((G, np_)), adj_sd=np.empty((G, np_)),
                 adj_quantile=np.empty((len(p), G, np_)), n_outside=np.empty((G, np_), np.int64))
        s = self._out(A.smm_adjustment_t, r, () if len(p) else ("adj_quantile",))
        self._check(self._fn("get_adjustment")(self._ctx, int(t0), int(t1), sel, gp, ng, float(tol), kern,
                                               A.dptr(sc) if sc is not None else None, float(ridge), A.dptr(p) if len(p) else None, len(p),
                                               C.byref(s)))
        return r

    def reweighted(self, t0=0, t1=None, select="state", groups=None, targets=(1.0,), probs=(), n_groups=None):
        """the target posterior from every temperature: the scored rows of groups of local chains over iterations [t0, t1)
        importance-reweighted from each chain's own acc_tuner to every target, on the device (smm_get_reweighted, include/smmhip.h): a
        dict of numpy arrays count / n_scored / n_chains [n_groups], chain_n [N], chain_ess / chain_logz [R][N], status / n_kept /
        sum_u / ess / value_mean [R][n_groups], mean [R][n_groups][np], cov [R][n_groups][np][np], m_mean [R][n_groups][nm], quantile
        [len(probs)][R][n_groups][np], R = len(targets).  select and groups as in moment_stats ("state" is the selection the theory is
        about); targets: 1 to 64 finite values >= 0 on acc_tuner's scale"""
        t1 = self._t1(t1)
        p, tg = A.f64(probs).reshape(-1), A.f64(targets).reshape(-1)
        np_, nm, N = self.np, self.nm, self.N
        sel = self._select(select)
        g, gp, ng = self._groups("reweighted", groups, n_groups)
        G, R = max(ng, 0), len(tg)
        r = dict(count=np.empty(G, np.int64), n_scored=np.empty(G, np.int64), n_chains=np.empty(G, np.int32),
                 status=np.empty((R, G), np.int32), chain_n=np.empty(N, np.int32), chain_ess=np.empty((R, N)), chain_logz=np.empty((R, N)),
                 n_kept=np.empty((R, G), np.int64), sum_u=np.empty((R, G)), ess=np.empty((R, G)), mean=np.empty((R, G, np_)),
                 cov=np.empty((R, G, np_, np_)), value_mean=np.empty((R, G)), m_mean=np.empty((R, G, nm)),
                 quantile=np.empty((len(p), R, G, np_)))
        s = self._out(A.smm_reweighted_t, r, () if len(p) else ("quantile",))
        self._check(self._fn("get_reweighted")(self._ctx, int(t0), int(t1), sel, gp, ng, A.dptr(tg) if R else None, R,
                                               A.dptr(p) if len(p) else None, len(p), C.byref(s)))
        return r

    def profile(self, t0=0, t1=None, select="accepted", groups=None, bins=20, range=None, pairs=(), bins2=None, n_groups=None,
                moments=True):
        """the objective and the simulated moments binned along parameters over iterations [t0, t1), on the device (smm_get_profile,
        include/smmhip.h): a dict of numpy arrays count [n_groups], status [n_groups][np], edges [n_groups][np][bins + 1], n / n_scored /
        v_min / min_chain / min_iter / v_mean [n_groups][np][bins], theta_at_min [n_groups][np][bins][np], with moments m_mean
        [n_groups][np][bins][nm] and, with pairs, edges2 [n_groups][np][bins2 + 1] and n2 / n_scored2 / v_min2 / min_chain2 / min_iter2 /
        v_mean2 [n_groups][len(pairs)][bins2][bins2].  select, groups, range, pairs and bins2 as in histogram"""
        t1 = self._t1(t1)
        np_, nm = self.np, self.nm
        sel = self._select(select)
        g, gp, ng = self._groups("profile", groups, n_groups)
        if isinstance(range, dict):
            if sorted(range) != list(_builtins.range(np_)):
                raise ValueError("profile: a range dict names every parameter index 0 .. np-1")
            range = [range[k] for k in _builtins.range(np_)]
        rg = None if range is None else np.ascontiguousarray(range, np.float64).reshape(np_, 2)
        pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        b, b2 = int(bins), int(bins if bins2 is None else bins2)
        npr, G, bb, bb2 = len(pr), max(ng, 0), max(b, 0), max(b2, 0)
        r = dict(count=np.empty(G, np.int64), status=np.empty((G, np_), np.int32), edges=np.empty((G, np_, bb + 1)),
                 n=np.empty((G, np_, bb), np.int64), n_scored=np.empty((G, np_, bb), np.int64), v_min=np.empty((G, np_, bb)),
                 min_chain=np.empty((G, np_, bb), np.int32), min_iter=np.empty((G, np_, bb), np.int32),
                 theta_at_min=np.empty((G, np_, bb, np_)), v_mean=np.empty((G, np_, bb)))
        if moments:
            r.update(m_mean=np.empty((G, np_, bb, nm)))
        if npr:
            r.update(edges2=np.empty((G, np_, bb2 + 1)), n2=np.empty((G, npr, bb2, bb2), np.int64),
                     n_scored2=np.empty((G, npr, bb2, bb2), np.int64), v_min2=np.empty((G, npr, bb2, bb2)),
                     min_chain2=np.empty((G, npr, bb2, bb2), np.int32), min_iter2=np.empty((G, npr, bb2, bb2), np.int32),
                     v_mean2=np.empty((G, npr, bb2, bb2)))
        s = self._out(A.smm_profile_t, r)
        self._check(self._fn("get_profile")(self._ctx, int(t0), int(t1), sel, gp, ng, b, A.dptr(rg) if rg is not None else None,
                                            pr.ctypes.data_as(A.c_int32_p) if npr else None, npr, b2, C.byref(s)))
        return r

    def _proposal_shape(self):
        if self.proposal_layout is None:
            return None
        return (self.np, self.np) if self.proposal_layout == "shared" else (self.N, self.np, self.np)

    def proposal(self):
        """the installed proposal factor(s): [np][np] (shared) or [N][np][np] (the local chains), zeros above the diagonal"""
        shape = self._proposal_shape()
        L = np.empty(shape if shape is not None else (self.np, self.np))
        self._check(self._fn("get_proposal")(self._ctx, A.dptr(L)))
        return L

    def set_proposal(self, L):
        """install proposal factor(s) of proposal()'s shape between steps (smm_set_proposal); above the diagonal is ignored"""
        shape = self._proposal_shape()
        L = A.f64(L)
        if shape is not None and L.shape != shape:
            raise ValueError("set_proposal: the factor must be %s, got %s" % (shape, L.shape))
        self._check(self._fn("set_proposal")(self._ctx, A.dptr(L)))

    def adapt_proposal(self, t0, t1, accepted_only=True, min_draws=None, normalize=True, ridge=1e-8):
        """each local chain's factor from the covariance of its own draws of [t0, t1) in [0, 1]-space (smm_adapt_proposal): returns
        status [N] — 0 installed, 1 fewer than min_draws (default np + 1) draws, 2 non-finite covariance, 3 not positive definite"""
        status = np.empty(self.N, np.int32)
        md = self.np + 1 if min_draws is None else int(min_draws)
        self._check(self._fn("adapt_proposal")(self._ctx, int(t0), int(t1), int(bool(accepted_only)), md, int(bool(normalize)),
                                               float(ridge), status.ctypes.data_as(A.c_int32_p)))
        return status

    def state(self):
        sb = A.StateBuffers(self.N, self.np, self.nm)
        ss = sb.struct()
        self._check(self._fn("get_state")(self._ctx, C.byref(ss)))
        sb.iter = ss.iter
        return sb

    def set_state(self, sb, hb):
        ss, hs = sb.struct(), hb.struct()
        self._check(self._fn("set_state")(self._ctx, C.byref(ss), C.byref(hs)))

    # --- the starting population (include/smmhip.h: smm_set_population, smm_scatter_population) --------------------------------
    def _population(self, call):
        r = dict(start=np.empty((self.np, self.N)), value=np.empty(self.N), pick=np.empty(self.N, np.int32))
        s = self._out(A.smm_population_t, r)
        self._check(call(C.byref(s)))
        r["evaluated"] = int(s.evaluated)
        return r

    def set_population(self, starts):
        """every local chain from its own point, starts [np][N], installed on the device as the chain's completed iteration 1
        (smm_set_population; only before the first step).  Returns a dict: start [np][N], value [N], pick [N] (0), evaluated"""
        st = A.f64(starts)
        if st.shape != (self.np, self.N):
            raise ValueError("set_population: starts must be [np][N] = %s, got %s" % ((self.np, self.N), st.shape))
        return self._population(lambda out: self._fn("set_population")(self._ctx, A.dptr(st), out))

    def scatter_population(self, M, spread=1.0, keep_init=True):
        """scatter search on the device (smm_scatter_population; only before the first step): M candidates per chain in the box of width
        `spread` (in [0, 1]-space) around initial_value, evaluated, the best valid one installed as the chain's completed iteration 1;
        keep_init: initial_value competes (and wins ties).  Returns a dict: start [np][N], value [N], pick [N] (the chosen candidate,
        -1 = initial_value), evaluated"""
        return self._population(lambda out: self._fn("scatter_population")(self._ctx, int(M), float(spread), int(bool(keep_init)), out))

    # --- the estimate (include/smmhip.h: smm_opt_slices, smm_opt_simplex, smm_opt_lm) ------------------------------------------------------------------------
    def _opt_starts(self, name, starts):
        """an optimiser's starts as the library reads them, [np][K] of float64, and K"""
        st = A.f64(starts)
        if st.ndim != 2 or st.shape[0] != self.np:
            raise ValueError("%s: starts must be [np][K] with np = %d, got %s" % (name, self.np, st.shape))
        return st, st.shape[1]

    def opt_slices(self, starts, npoints, tol=1e-5, update=None, max_cycles=1000):
        """K cyclic coordinate searches on grids of npoints values, starts [np][K], advancing together on the device (smm_opt_slices:
        optSlices of slices.jl from many starts; the context's chains are not touched).  update=None: the ranges never shrink.
        Returns a dict: best [np][K], value [K], sim_moments [nm][K], lo / hi [np][K], delta [K], cycle_value [max_cycles][K],
        cycles [K], converged [K], evaluated"""
        st, K = self._opt_starts("opt_slices", starts)
        mc = max(int(max_cycles), 0)
        r = dict(best=np.empty((self.np, K)), value=np.empty(K), sim_moments=np.empty((self.nm, K)), lo=np.empty((self.np, K)),
                 hi=np.empty((self.np, K)), delta=np.empty(K), cycle_value=np.empty((mc, K)), cycles=np.empty(K, np.int32),
                 converged=np.empty(K, np.int32))
        s = self._out(A.smm_opt_slices_t, r)
        self._check(self._fn("opt_slices")(self._ctx, A.dptr(st), K, int(npoints), float(tol), float("nan") if update is None else float(update),
                                           int(max_cycles), C.byref(s)))
        r["evaluated"] = int(s.evaluated)
        return r

    def opt_simplex(self, starts, step=0.05, adaptive=False, xatol=1e-4, fatol=1e-4, max_iter=None):
        """K Nelder–Mead searches inside the box, starts [np][K], advancing together on the device (smm_opt_simplex: scipy's bounded
        Nelder–Mead made exact, the initial simplex `step` of each range wide; the context's chains are not touched).  max_iter=None:
        200 * np.  Returns a dict: best [np][K], value [K], sim_moments [nm][K], simplex [np+1][np][K], simplex_value [np+1][K], size_x /
        size_f [K], iterations [K], status [K] (1 converged, 0 max_iter, 2 no finite value), moves [5][K], n_eval [K], evaluated"""
        st, K = self._opt_starts("opt_simplex", starts)
        V = self.np + 1
        r = dict(best=np.empty((self.np, K)), value=np.empty(K), sim_moments=np.empty((self.nm, K)), simplex=np.empty((V, self.np, K)),
                 simplex_value=np.empty((V, K)), size_x=np.empty(K), size_f=np.empty(K), iterations=np.empty(K, np.int32),
                 status=np.empty(K, np.int32), moves=np.empty((5, K), np.int32), n_eval=np.empty(K, np.int32))
        s = self._out(A.smm_opt_simplex_t, r)
        self._check(self._fn("opt_simplex")(self._ctx, A.dptr(st), K, float(step), int(bool(adaptive)), float(xatol), float(fatol),
                                            200 * self.np if max_iter is None else int(max_iter), C.byref(s)))
        r["evaluated"] = int(s.evaluated)
        return r

    def opt_lm(self, starts, fd_step=1e-4, lambda0=1e-3, lambda_up=10, lambda_down=10, xtol=1e-8, ftol=1e-12, gtol=0.0, max_iter=100,
               max_tries=12):
        """K Levenberg–Marquardt searches inside the box, starts [np][K], advancing together on the device (smm_opt_lm: least squares on the
        moments' residuals (sim - mom) / s with forward-difference Jacobians, fd_step of each range wide; the context's chains are not
        touched).  Returns a dict: best [np][K], value [K], sim_moments [nm][K], ssr [K], grad [np][K], jac [nm][np][K], lambda / step / dF
        [K], active [np][K], iterations / tries / n_eval [K], status [K] (1 converged, 0 max_iter, 2 not finite, 3 no descent found, 4 a
        parameter moves no moment), evaluated"""
        st, K = self._opt_starts("opt_lm", starts)
        i32 = lambda *shape: np.empty(shape, np.int32)      # noqa: E731
        r = dict(best=np.empty((self.np, K)), value=np.empty(K), sim_moments=np.empty((self.nm, K)), ssr=np.empty(K), grad=np.empty((self.np, K)),
                 jac=np.empty((self.nm, self.np, K)), step=np.empty(K), dF=np.empty(K), active=i32(self.np, K), iterations=i32(K), tries=i32(K),
                 n_eval=i32(K), status=i32(K))
        r["lambda"] = np.empty(K)
        s = self._out(A.smm_opt_lm_t, r)
        self._check(self._fn("opt_lm")(self._ctx, A.dptr(st), K, float(fd_step), float(lambda0), float(lambda_up), float(lambda_down), float(xtol),
                                       float(ftol), float(gtol), int(max_iter), int(max_tries), C.byref(s)))
        r["evaluated"] = int(s.evaluated)
        return r

    # --- sampling without chains (include/smmhip.h: smm_abc_pmc) ----------------------------------------------------------------------------------
    def abc_pmc(self, n_particles, n_keep, max_gen=20, p_acc_min=0.05, scale=2.0, ridge=0.0, probs=()):
        """the adaptive population Monte Carlo ABC sampler on the device (smm_abc_pmc: Lenormand, Jabot & Deffuant 2013; uniform prior on the
        box, the objective value as the distance; the context's chains are not touched).  Returns a dict: theta [np][A], value [A],
        sim_moments [nm][A], weight / logw [A], born [A], the per-generation eps, p_acc, gen_ess, n_outside, n_invalid, n_underflow,
        n_new_kept [max_gen + 1], mean [np], cov [np][np], quantile [len(probs)][np], and the scalars ess, n_kept, generations, status
        (0 max_gen, 1 p_acc <= p_acc_min, 2 fewer than 2 finite particles, 3 kernel covariance not positive definite), evaluated"""
        Ap, G1 = max(int(n_keep), 0), max(int(max_gen), 0) + 1
        pr = A.f64(list(probs))
        r = dict(theta=np.empty((self.np, Ap)), value=np.empty(Ap), sim_moments=np.empty((self.nm, Ap)), weight=np.empty(Ap), logw=np.empty(Ap),
                 born=np.empty(Ap, np.int32), eps=np.empty(G1), p_acc=np.empty(G1), gen_ess=np.empty(G1), n_outside=np.empty(G1, np.int32),
                 n_invalid=np.empty(G1, np.int32), n_underflow=np.empty(G1, np.int32), n_new_kept=np.empty(G1, np.int32),
                 mean=np.empty(self.np), cov=np.empty((self.np, self.np)), quantile=np.empty((len(pr), self.np)))
        s = self._out(A.smm_abc_pmc_t, r)
        self._check(self._fn("abc_pmc")(self._ctx, int(n_particles), int(n_keep), int(max_gen), float(p_acc_min), float(scale), float(ridge),
                                        A.dptr(pr) if len(pr) else None, len(pr), C.byref(s)))
        for f in ("ess", "n_kept", "generations", "status", "evaluated"):
            r[f] = getattr(s, f)
        return r

    # --- global sensitivity (include/smmhip.h: smm_sens_sobol) -------------------------------------------------------------------------------------
    def sens_sobol(self, n_base, lo=None, hi=None):
        """variance-based global sensitivity on the device (smm_sens_sobol: Sobol' first-order and total-order indices of the objective value
        and of every simulated moment over the box [lo, hi], None = [lb, ub]; n_base (np + 2) evaluations; the context's chains are not
        touched).  Returns a dict: mean / var / centre [F], first / total / v_first / v_total / se_first / se_total [F][np] (F = nm + 1:
        output 0 is the value, 1 + f moment f), and the scalars n_complete, n_invalid, evaluated"""
        F = self.nm + 1
        box = [None if b is None else A.f64(list(np.asarray(b, float).reshape(-1))) for b in (lo, hi)]
        for b in box:
            if b is not None and len(b) != self.np:
                raise ValueError("sens_sobol: lo and hi take one entry per parameter")
        r = dict(mean=np.empty(F), var=np.empty(F), centre=np.empty(F))
        for f in ("first", "total", "v_first", "v_total", "se_first", "se_total"):
            r[f] = np.empty((F, self.np))
        s = self._out(A.smm_sens_sobol_t, r)
        self._check(self._fn("sens_sobol")(self._ctx, int(n_base), *[None if b is None else A.dptr(b) for b in box], C.byref(s)))
        for f in ("n_complete", "n_invalid", "evaluated"):
            r[f] = int(getattr(s, f))
        return r

    def timing(self):
        t = A.smm_timing_t()
        self._check(self._fn("get_timing")(self._ctx, C.byref(t)))
        return t

    def set_profiling(self, on=True):
        """0/False off; 1/True event brackets; 2 per-kernel begin/end timestamps (see include/smmhip.h)"""
        self._check(self._fn("set_profiling")(self._ctx, int(on)))

    def set_persistent(self, on=True):
        """the persistent form of step() (one launch per look-ahead window; include/smmhip.h): on by default where a context qualifies"""
        self._check(self._fn("set_persistent")(self._ctx, int(bool(on))))

    def describe(self):
        """the forms this context was given at creation, as a dict (smm_describe: chain / walk / exchange / persistent / plan / window)"""
        buf = C.create_string_buffer(256)
        self._check(self._fn("describe")(self._ctx, buf, 256))
        return dict(kv.split("=", 1) for kv in buf.value.decode().split())

    def persistent_info(self):
        """(would the next step take the persistent form, launches of it so far, repairs so far)"""
        a, l, r = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self._check(self._fn("get_persistent")(self._ctx, C.byref(a), C.byref(l), C.byref(r)))
        return bool(a.value), int(l.value), int(r.value)

    def plan_beside_info(self):
        """(does the context plan its next exchange window beside the persistent kernel, windows planned beside so far, windows planned on the main stream)"""
        b, wb, wi = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self._check(self._fn("get_plan_beside")(self._ctx, C.byref(b), C.byref(wb), C.byref(wi)))
        return bool(b.value), int(wb.value), int(wi.value)

    def Z(self):
        z = np.empty((self.nm, self.problem.ns))
        self._check(self._fn("get_Z")(self._ctx, A.dptr(z)))
        return z


def register_user_objective(source, n_sums=None, lanes=256, rng=False):
    """Compile a user objective for the device and return its objective_id handle (include/smmhip.h).
    n_sums=None: `source` defines SMM_USER_OBJECTIVE(...), evaluated by one thread per chain.
    n_sums=k:    map-reduce form — `source` defines SMM_USER_PARTIAL(...) and SMM_USER_FINISH(...); `lanes` threads
                 evaluate one chain and their k partial sums are reduced in a fixed order.
    rng=True:    the same forms with the library's random stream as an argument — SMM_USER_OBJECTIVE_RNG(...) or
                 SMM_USER_PARTIAL_RNG(...) + SMM_USER_FINISH(...), drawing with smm_normal / smm_normal2 / smm_uniform;
                 such objectives also have noseed evaluations (eval_batch_noseed, getSigma).
    Raises with the compiler log if the source does not compile."""
    lib = A.load()
    oid = C.c_int32(0)
    if rng:
        rc = lib.smm_register_user_objective_rng(source.encode(), 0 if n_sums is None else int(n_sums), int(lanes), C.byref(oid))
    elif n_sums is None:
        rc = lib.smm_register_user_objective(source.encode(), C.byref(oid))
    else:
        rc = lib.smm_register_user_objective_lanes(source.encode(), int(n_sums), int(lanes), C.byref(oid))
    if rc != 0:
        raise RuntimeError("smm_register_user_objective failed (%d): %s" % (rc, lib.smm_last_error(None).decode()))
    return int(oid.value)


class UserTransform:
    """a user function of one history row (SMM_USER_TRANSFORM, include/smmhip.h) with n_out outputs: compiled for the device when it is
    made, its handle kept per loaded library (the handles of smm_register_user_transform are the library's own)"""

    def __init__(self, source, n_out):
        self.source, self.n_out = source, int(n_out)
        self._handles = {}
        self.handle(A.load())

    def handle(self, lib):
        if id(lib) not in self._handles:
            tid = C.c_int32(-1)
            rc = lib.smm_register_user_transform(self.source.encode(), self.n_out, C.byref(tid))
            if rc != 0:
                raise A.SMMHipError(rc, "smm_register_user_transform failed: %s" % lib.smm_last_error(None).decode())
            self._handles[id(lib)] = int(tid.value)
        return self._handles[id(lib)]


def user_transform(source, n_out):
    """Compile a user transform for the device (smm_register_user_transform, include/smmhip.h): `source` defines
    SMM_USER_TRANSFORM(theta, np, sim_moments, nm, value, mom, w, udata, n_udata, tdata, n_tdata, out, n_out), a deterministic function of
    one history row writing out[0 .. n_out); it may call smm_exp and smm_log.  Returns what BGPContext.derived and host.derived take.
    Raises SMMHipError with the compiler's log if the source does not compile."""
    return UserTransform(source, n_out)


def hip_context(problem, opts, tables=None):
    """A BGPContext on libsmmhip.so. Raises if the library is missing."""
    return BGPContext(problem, opts, tables)
