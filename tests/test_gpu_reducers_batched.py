"""The history reducers (smm_get_chain_stats, smm_get_chain_cov, smm_adapt_proposal, smm_get_chain_diag; include/smmhip.h) in their
batched paths: chains reduced in batches of Nb (offset c0), stats' parameters in batches of kb (offset k0, the `first` flag), the
kb = 0 branch of a raw C caller, the partner mode's passes over the ids and their tie rule, and the scratch the three share, freed
and grown across calls.  The test build's seams SMMHIP_STATS_SCRATCH (the scratch cap) and SMMHIP_STATS_MODE_BINS (ids per pass)
reach these paths at small sizes; the C5 and C3 cases reach them in the shipped library at the sizes that take them.  Every output
is held bit for bit (NaN equal to NaN) against the restatements (chain_stats_ref, chain_cov_ref, chain_diag_ref) and against the same
call on an unbatched context holding the same history, and every case asserts the batch plan it claims (Plan: the host's formulas)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import chain_cov_ref as CR
import chain_diag_ref as DR
import chain_stats_ref as R
import common as cm

pytestmark = pytest.mark.gpu
PROBS = (0.0, 0.025, 0.5, 0.975, 1.0)
STATS_SCRATCH_CAP = 256 << 20    # smm_reducers_host.hpp: REDUCER_BATCH_CAP
STATS_MODE_BINS = 16384          # smm_stats.hpp


class Plan:
    """the host's batch plan of the reducers (smm_reducers_host.hpp: chain_stats_scratch_bytes, reducer_scratch, chain_batches,
    smm_get_chain_stats, chain_cov_device, smm_get_chain_diag), following one context's shared scratch st_scr across its calls"""

    def __init__(self, N, T, npar, cap=STATS_SCRATCH_CAP):
        self.N, self.T, self.np, self.cap = N, T, npar, cap
        self.scr = 0

    def _alloc(self):
        return min(self.N * self.T * (8 * self.np + 4), max(self.cap, 12 * self.T))

    def _one(self, one):   # cov / diag: the scratch holds at least one chain's columns of the whole capacity
        if self.scr and self.scr < one:
            self.scr = 0
        if not self.scr:
            self.scr = max(self._alloc(), one)

    def stats(self, n, cols=True):
        """(kb, Nb, [(k0, kbb)], chain batches) of a call over n iterations; None: nothing reduced"""
        if n == 0:
            return None
        if not self.scr:
            self.scr = self._alloc()
        kb = self.np if cols else 0
        per = lambda k: n * (8 * k + 4)
        while kb > 1 and per(kb) > self.scr:
            kb = (kb + 1) // 2
        Nb = min(self.N, self.scr // per(kb))
        kbs = [(k0, min(kb, self.np - k0)) for k0 in range(0, self.np, kb)] if kb else [(0, 0)]
        return SimpleNamespace(kb=kb, Nb=Nb, kbatches=kbs, cbatches=-(-self.N // Nb))

    def cov(self, n):
        if n == 0:
            return None
        self._one(self.T * (8 * self.np + 4))
        Nb = min(self.N, self.scr // (n * (8 * self.np + 4)))
        return SimpleNamespace(Nb=Nb, cbatches=-(-self.N // Nb))

    def diag(self, n):
        S = self.np + 1
        self._one(self.T * 8 * S)
        Nb = min(self.N, self.scr // (n * 8 * S))
        return SimpleNamespace(Nb=Nb, cbatches=-(-self.N // Nb), lds_n=min(8192, n))


def stats_cap(n, npar, Nb):
    """a cap under which a stats call over n iterations takes Nb chains per batch with every parameter"""
    return Nb * n * (8 * npar + 4)


def batched_context(S, monkeypatch, prob, opts, cap=None, bins=None, snap=None):
    """a context of the test build created under the seams (they are read at creation only), restored to snap if given"""
    for var, v in (("SMMHIP_STATS_SCRATCH", cap), ("SMMHIP_STATS_MODE_BINS", bins)):
        if v is not None:
            monkeypatch.setenv(var, str(v))
    h = S.hip_context(prob, opts)
    for var in ("SMMHIP_STATS_SCRATCH", "SMMHIP_STATS_MODE_BINS"):
        monkeypatch.delenv(var, raising=False)
    if snap is not None:
        h.set_state(*snap)
    return h


def base_run(S, prob, opts, T):
    """an unbatched context stepped T iterations, and its (state, history)"""
    h = S.hip_context(prob, opts)
    h.step(T)
    assert Plan(opts.N, opts.maxiter, prob.np).stats(T).cbatches == 1
    return h, (h.state(), h.history())


def assert_arrays_equal(got, want):
    for g, w in zip(got, want):
        assert g.shape == w.shape and np.array_equal(g, w, equal_nan=True)


def stats_twice(h, base, t0, t1, acc, probs, want):
    got = h.chain_stats(t0, t1, acc, probs)
    R.assert_stats_equal(got, want)
    R.assert_stats_equal(got, base.chain_stats(t0, t1, acc, probs))
    return got


def ref_cov(prob, hist, t0, t1, acc, unit):
    kw = dict(lb=prob.lb, ub=prob.ub) if unit else {}
    return CR.chain_cov(hist.params, hist.accepted, t0, t1, acc, **kw)


def ref_diag(hist, t0, t1, max_lag=None, n_acf=0, groups=None):
    with np.errstate(invalid="ignore", divide="ignore"):
        return DR.diag_from_history(hist, t0, t1, max_lag, n_acf, groups)


# --- stats under the scratch seam -------------------------------------------------------------------------------------------------------

def stats_problem(which):
    from smm_jl_amd.workloads import build_problem
    if which == "serial100":
        return cm.serial_normal(N=100, T=60, ns=200), 60
    if which == "general5":
        return cm.general_normal(5, N=32, T=50, ns=200), 50
    if which == "c5_32":
        return build_problem("c5", 32, 32, 0, 60, 0), 60
    assert which == "long"
    return cm.serial_normal(N=4, T=9000, ns=50), 9000


# for each problem: (cap, the full window's kb, Nb) — the first always kb = 1, Nb = 1 (the floor 12 x maxiter)
STATS_CASES = {
    "serial100": lambda T: [(12 * T, 1, 1), (stats_cap(T, 2, 1), 2, 1), (stats_cap(T, 2, 7), 2, 7)],
    "general5": lambda T: [(12 * T, 1, 1), (20 * T, 2, 1), (28 * T, 3, 1), (stats_cap(T, 5, 3), 5, 3)],
    "c5_32": lambda T: [(12 * T, 1, 1), (stats_cap(T, 50, 5), 50, 5), (stats_cap(T, 50, 24), 50, 24)],
    "long": lambda T: [(12 * T, 1, 1), (stats_cap(T, 2, 3), 2, 3)],
}


@pytest.mark.parametrize("which", list(STATS_CASES))
def test_stats_batches_of_chains_and_parameters(S, hooks, monkeypatch, which):
    (prob, opts), T = stats_problem(which)
    base, snap = base_run(S, prob, opts, T)
    hist = snap[1]
    N, npar = opts.N, prob.np
    windows = [(0, T), (T // 5, T - T // 7), (T // 2, T // 2), (T - 1, T)]
    want = {(w, acc): R.stats_from_history(hist, w[0], w[1], acc, PROBS) for w in windows for acc in (True, False)}
    seen_kb = set()
    for cap, kb, Nb in STATS_CASES[which](T):
        h = batched_context(S, monkeypatch, prob, opts, cap=cap, snap=snap)
        plan = Plan(N, T, npar, cap)
        p = plan.stats(T)
        assert (p.kb, p.Nb) == (kb, Nb) and p.cbatches > 1
        if Nb > 1:
            assert N % Nb != 0 or Nb % 8 == 0          # a short last batch, or batches of whole XCD groups
        seen_kb.update(k for _, k in p.kbatches)
        for w in windows:
            for acc in (True, False):
                stats_twice(h, base, w[0], w[1], acc, PROBS, want[(w, acc)])
        cm.assert_history_equal(h.history(), hist, exact_floats=True)
    if which == "general5":
        assert seen_kb == {1, 2, 3, 5}                 # kb 5 -> 3 -> 2 -> 1; the batches of 3 and 2 end short
    if which == "c5_32":
        assert [k for _, k in Plan(N, T, npar, 12 * T).stats(T).kbatches] == [1] * 50   # kb halved from 50 to 1
    if which == "long":
        assert T > 8192 and want[((0, T), False)]["count"].min() > 8192


def test_stats_kb0_branch_through_the_raw_abi(S, hooks, monkeypatch):
    A = hooks
    prob, opts = cm.serial_normal(N=100, T=60, ns=200)
    T = 60
    base, snap = base_run(S, prob, opts, T)
    cap = 7 * 4 * T
    h = batched_context(S, monkeypatch, prob, opts, cap=cap, snap=snap)
    plan = Plan(100, T, 2, cap)
    p0 = plan.stats(T, cols=False)
    assert p0.kb == 0 and p0.Nb == 7 and p0.cbatches == 15
    fn = h._fn("get_chain_stats")
    probs = np.array([0.0, 0.5, 1.0])
    for acc in (True, False):
        for t0, t1 in ((0, T), (9, 47)):
            full = h.chain_stats(t0, t1, acc, probs)
            R.assert_stats_equal(full, R.stats_from_history(snap[1], t0, t1, acc, probs))
            R.assert_stats_equal(full, base.chain_stats(t0, t1, acc, probs))
            for fields in (("count", "best_value", "best_iter", "n_exchanged", "most_exchanged_with"), ("count",)):
                r = {f: np.full(full[f].shape, -7, full[f].dtype) for f in fields}
                s = A.smm_chain_stats_t()
                for f, t in A.smm_chain_stats_t._fields_:
                    if f in r:
                        setattr(s, f, r[f].ctypes.data_as(t))
                assert not s.mean and not s.median and not s.quantile
                assert fn(h._ctx, t0, t1, int(acc), probs.ctypes.data_as(A.c_double_p), len(probs), C.byref(s)) == A.SMM_OK
                R.assert_stats_equal(r, full, fields)
    assert plan.stats(T).kb == 2 and plan.stats(T).Nb == 1    # (the full calls on the same scratch: every parameter, a chain a batch)


# --- cov and adapt --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["serial100", "c5_32"])
def test_cov_batches_of_chains(S, hooks, monkeypatch, which):
    (prob, opts), T = stats_problem(which)
    base, snap = base_run(S, prob, opts, T)
    hist = snap[1]
    N, npar = opts.N, prob.np
    one = T * (8 * npar + 4)
    for cap, Nb in ((12 * T, 1), (7 * one, 7), (5 * one, 5)):
        h = batched_context(S, monkeypatch, prob, opts, cap=cap, snap=snap)
        plan = Plan(N, T, npar, cap)
        p = plan.cov(T)
        assert p.Nb == Nb and p.cbatches > 1
        for unit in (False, True):
            for acc in (True, False):
                for t0, t1 in ((0, T), (T // 4, T - 3), (5, 6)):
                    got = h.chain_cov(t0, t1, acc, unit)
                    assert_arrays_equal(got, ref_cov(prob, hist, t0, t1, acc, unit))
                    assert_arrays_equal(got, base.chain_cov(t0, t1, acc, unit))


def test_adapt_batched_then_the_run_goes_on_as_its_unbatched_twin(S, hooks, monkeypatch):
    N, npar, T1, K = 48, 6, 80, 20
    prob, opts = cm.general_normal(npar, N=N, T=T1 + K, ns=200)
    opts.chol_L = np.ascontiguousarray(np.broadcast_to(np.eye(npar), (N, npar, npar)))
    base = S.hip_context(prob, opts)
    base.step(T1)
    snap = (base.state(), base.history())
    n = T1 - 10
    for cap, Nb in ((12 * (T1 + K), 1), (5 * n * (8 * npar + 4), 5)):
        twin = S.hip_context(prob, opts)
        twin.set_state(*snap)
        h = batched_context(S, monkeypatch, prob, opts, cap=cap, snap=snap)
        p = Plan(N, T1 + K, npar, cap).cov(n)
        assert p.Nb == Nb and p.cbatches > 1 and (N % Nb != 0 or Nb == 1)
        st = h.adapt_proposal(10, T1, ridge=1e-9)
        count, _, cov = ref_cov(prob, snap[1], 10, T1, True, True)
        L, want = CR.adapt(count, cov, npar + 1, True, 1e-9)
        assert np.array_equal(st, want) and (st == 0).sum() >= 4
        got = h.proposal()
        for c in range(N):
            assert np.array_equal(got[c], L[c] if st[c] == 0 else np.eye(npar)), c
        assert np.array_equal(twin.adapt_proposal(10, T1, ridge=1e-9), st)
        assert np.array_equal(twin.proposal(), got)
        h.step(K)
        twin.step(K)
        cm.assert_history_equal(h.history(), twin.history(), exact_floats=True)
        cm.assert_state_equal(h.state(), twin.state(), rtol=0)


# --- diag ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["serial100", "long"])
def test_diag_batches_of_chains(S, hooks, monkeypatch, which):
    (prob, opts), T = stats_problem(which)
    base, snap = base_run(S, prob, opts, T)
    hist = snap[1]
    N, npar = opts.N, prob.np
    one = T * 8 * (npar + 1)
    groups = np.arange(N) % 4 if N > 4 else np.array([0, 1, 0, 1])   # every group's members in different batches
    calls = [(0, T, None, 6), (T // 3, T - 1, 9, 10), (T - 40, T, None, 0)]
    if which == "long":
        assert T > 8192                                                # the full window: the columns centred in place in the scratch
        calls = [(0, T, 600, 3), (T - 100, T, None, 5)]
    for cap, Nb in ((12 * T, 1), (3 * one, 3)):
        h = batched_context(S, monkeypatch, prob, opts, cap=cap, snap=snap)
        plan = Plan(N, T, npar, cap)
        p = plan.diag(T)
        assert p.Nb == Nb and p.cbatches > 1 and (N % Nb != 0 or Nb == 1)
        assert (p.lds_n < T) == (which == "long")
        for g in (groups, None):
            for t0, t1, ml, na in calls:
                q = plan.diag(t1 - t0)
                assert q.cbatches > 1 or t1 - t0 < T
                got = h.chain_diag(t0, t1, ml, na, g)
                DR.assert_diag_equal(got, ref_diag(hist, t0, t1, ml, na, g))
                DR.assert_diag_equal(got, base.chain_diag(t0, t1, ml, na, g))
        assert plan.diag(40).lds_n < 8192


# --- one context, every reducer in turn, on a small scratch --------------------------------------------------------------------------------

def test_call_order_on_a_small_shared_scratch(S, hooks, monkeypatch):
    N, npar, T1, K = 40, 5, 60, 20
    prob, opts = cm.general_normal(npar, N=N, T=T1 + K, ns=200)
    T = T1 + K
    quiet = S.hip_context(prob, opts)                      # no reducer is ever called on it
    cap = 12 * T
    h = batched_context(S, monkeypatch, prob, opts, cap=cap)
    quiet.step(T1)
    h.step(T1)
    hist = h.history()
    plan = Plan(N, T, npar, cap)
    seq = []

    def stats(t0, t1, acc, probs):
        seq.append(("stats", plan.stats(t1 - t0), plan.scr))
        R.assert_stats_equal(h.chain_stats(t0, t1, acc, probs), R.stats_from_history(hist, t0, t1, acc, probs))

    def cov(t0, t1, acc, unit):
        seq.append(("cov", plan.cov(t1 - t0), plan.scr))
        assert_arrays_equal(h.chain_cov(t0, t1, acc, unit), ref_cov(prob, hist, t0, t1, acc, unit))

    def diag(t0, t1, na, g):
        seq.append(("diag", plan.diag(t1 - t0), plan.scr))
        DR.assert_diag_equal(h.chain_diag(t0, t1, None, na, g), ref_diag(hist, t0, t1, None, na, g))

    stats(0, T1, True, (0.5,))                             # allocates max(cap, 12 x maxiter): one parameter at a time
    cov(0, T1, False, True)                                # below one chain's columns: freed and allocated again
    stats(5, T1, False, (0.5,))                            # the larger scratch: more parameters per batch
    diag(3, T1, 4, np.arange(N) % 3)                       # below one chain's S columns: freed and allocated again
    stats(0, T1, True, PROBS)                              # more probs: the results buffer grows
    diag(10, 50, 0, None)                                  # a different n on the same scratch
    cov(0, T1, True, False)
    scr = [s for _, _, s in seq]
    assert scr[0] == 12 * T and scr[1] == T * (8 * npar + 4) and scr[3] == T * 8 * (npar + 1) and scr[-1] == scr[3]
    assert seq[0][1].kb == 1 and seq[2][1].kb > 1 and all(p.cbatches > 1 for _, p, _ in seq)
    h.step(K)
    quiet.step(K)
    cm.assert_history_equal(h.history(), quiet.history(), exact_floats=True)
    cm.assert_state_equal(h.state(), quiet.state(), rtol=0)


# --- the partner mode's passes --------------------------------------------------------------------------------------------------------------

def test_partner_mode_in_several_passes(S, hooks, monkeypatch):
    N, T, bins = 40, 40, 7
    prob, opts = cm.serial_normal(N=N, T=T, ns=100)
    h0 = S.hip_context(prob, opts)
    h0.step(2)
    st = h0.state()
    hb = h0.history(0, 2)
    rng = np.random.default_rng(5)
    from smm_jl_amd import _abi as A
    c = A.HistoryBuffers(T, N, prob.np, prob.nm)
    for f in A.HistoryBuffers.FIELDS:
        getattr(c, f)[...] = getattr(hb, f)[rng.integers(0, 2, T)]
    c.exchanged[...] = np.where(rng.random((T, N)) < 0.5, rng.integers(1, N + 1, (T, N)), 0)
    crafted = {   # chain: (partner ids in the window, the mode); passes of 7 ids: 1-7, 8-14, ..., 29-35, 36-40
        0: ([1, 2, 38, 38, 38, 9, 9], 38),             # found only in the last, partial pass
        1: ([10, 10, 3, 3], 3),                        # a tie across two passes, the same bin: the smaller id
        2: ([40, 40, 4, 4], 4),                        # a tie across passes, different bins
        3: ([6, 6, 2, 2], 2),                          # a tie within a pass
        4: ([40, 40, 40, 1], 40),                      # the id N_global
        5: ([], 0),                                    # no exchange
        6: ([38, 38, 31, 31, 24, 24], 24),             # a tie across three passes, the same bin
        7: ([1, 1, 1, 36, 36], 1),                     # the first pass wins over a smaller count in the last
        8: ([37] * T, 37),                             # exchanged at every iteration
    }
    for j, (ids, _) in crafted.items():
        c.exchanged[:, j] = 0
        c.exchanged[np.sort(rng.choice(T, len(ids), replace=False)), j] = ids
    assert c.exchanged.min() >= 0 and c.exchanged.max() == N
    st.iter = T
    snap = (st, c)
    base = S.hip_context(prob, opts)                      # ids per pass min(16384, max(N, 64)) = 64: one pass
    base.set_state(*snap)
    back = base.history(0, T)
    assert np.array_equal(back.exchanged, c.exchanged)
    cap = stats_cap(T, 2, 3)
    for kw in (dict(bins=bins), dict(bins=bins, cap=cap)):
        h = batched_context(S, monkeypatch, prob, opts, snap=snap, **kw)
        if "cap" in kw:
            assert Plan(N, T, 2, cap).stats(T).Nb == 3
        for acc in (True, False):
            for t0, t1 in ((0, T), (3, T - 5)):
                got = stats_twice(h, base, t0, t1, acc, (0.5,), R.stats_from_history(back, t0, t1, acc, (0.5,)))
                most = got["most_exchanged_with"]
                assert ((most >= 1) & (most <= N) | (most == 0) & (got["n_exchanged"] == 0)).all()
        got = h.chain_stats(0, T)
        for j, (ids, mode) in crafted.items():
            assert got["most_exchanged_with"][j] == mode and got["n_exchanged"][j] == len(ids), j
    assert -(-N // bins) == 6 and N % bins != 0               # (the premise: six passes, the last one short)


# --- p2p shards -------------------------------------------------------------------------------------------------------------------------------

def test_batched_shards_report_their_slice(S, hooks, monkeypatch):
    from test_gpu_p2p import p2p_contexts, p2p_run_lockstep
    G, T = 2, 30
    prob, opts = cm.serial_normal(N=128, T=T, ns=1000)
    single = S.hip_context(prob, opts)
    single.step(T)
    n = T - 2
    cap = stats_cap(n, 2, 5)
    monkeypatch.setenv("SMMHIP_STATS_SCRATCH", str(cap))
    ctxs = p2p_contexts(S, prob, opts, G)
    monkeypatch.delenv("SMMHIP_STATS_SCRATCH")
    p2p_run_lockstep(ctxs, T)
    plan = Plan(64, T, 2, cap)
    assert plan.stats(n).Nb == 5 and plan.cov(n).Nb < 64 and plan.diag(n).Nb < 64
    g = np.arange(64) % 3
    for acc in (True, False):
        whole = single.chain_stats(2, T, acc, PROBS)
        wcov = single.chain_cov(2, T, acc, True)
        wdiag = single.chain_diag(2, T, None, 4)
        for r, c in enumerate(ctxs):
            sl = slice(64 * r, 64 * (r + 1))
            part = c.chain_stats(2, T, acc, PROBS)
            R.assert_stats_equal(part, {k: v[..., sl] for k, v in whole.items()})
            if r == 1:
                assert part["most_exchanged_with"].max() > 64 and part["most_exchanged_with"].min() >= 0
            assert_arrays_equal(c.chain_cov(2, T, acc, True), [x[..., sl] for x in wcov])
            DR.assert_diag_equal(c.chain_diag(2, T, None, 4), {k: v[..., sl] for k, v in wdiag.items() if k != "rhat"})
            DR.assert_diag_equal(c.chain_diag(2, T, None, 0, g), ref_diag(c.history(0, T), 2, T, None, 0, g))


# --- the shipped library at the sizes that batch ---------------------------------------------------------------------------------------------

def download(h, T, fields):
    """the history's fields named (the others NULL: smm_get_history skips them), as a HistoryBuffers-like namespace"""
    from smm_jl_amd import _abi as A
    N, npar = h.N, h.np
    shapes = dict(value=((T, N), np.float64), params=((T, npar, N), np.float64), exchanged=((T, N), np.int32),
                  accepted=((T, N), np.uint8))
    out = SimpleNamespace(**{f: np.empty(*shapes[f]) for f in fields})
    hs = A.smm_history_t()
    for f, t in A.smm_history_t._fields_:
        if f in fields:
            setattr(hs, f, getattr(out, f).ctypes.data_as(t))
    h._check(h._fn("get_history")(h._ctx, 0, T, C.byref(hs)))
    return out


def sliced(hist, cols):
    return SimpleNamespace(**{f: np.ascontiguousarray(v[..., cols]) for f, v in vars(hist).items()})


def test_c5_past_the_cap(S):
    from smm_jl_amd.workloads import build_problem
    N, T = 4096, 200
    prob, opts = build_problem("c5", N, N, 0, T, 0)
    npar = prob.np
    opts.chol_L = np.ascontiguousarray(np.broadcast_to(np.eye(npar), (N, npar, npar)))
    h = S.hip_context(prob, opts)
    h.step(T)
    ps, pc, pd = Plan(N, T, npar).stats(T), Plan(N, T, npar).cov(T), Plan(N, T, npar).diag(T)
    assert ps.kb == npar and ps.cbatches == pc.cbatches == pd.cbatches == 2      # 4096 x 200 x 404 B = 331 MB: two batches of chains
    cols = sorted(set(range(0, N, 128)) | {b + d for b in (ps.Nb, pc.Nb, pd.Nb) for d in (-2, -1, 0, 1)})
    hist = sliced(download(h, T, ("value", "params", "exchanged", "accepted")), cols)
    for acc in (True, False):
        got = h.chain_stats(0, T, acc, PROBS)
        R.assert_stats_equal({k: v[..., cols] for k, v in got.items()}, R.stats_from_history(hist, 0, T, acc, PROBS))
        assert acc or (got["count"] == T).all()
    for acc, unit in ((True, True), (False, False)):
        got = h.chain_cov(0, T, acc, unit)
        assert_arrays_equal([x[..., cols] for x in got], ref_cov(prob, hist, 0, T, acc, unit))
    groups = np.full(N, -1)
    groups[cols] = np.arange(len(cols)) % 3                   # members on both sides of the boundary
    got = h.chain_diag(0, T, None, 3, groups)
    want = ref_diag(hist, 0, T, None, 3, groups[cols])
    DR.assert_diag_equal({k: (v if k == "rhat" else v[..., cols]) for k, v in got.items()}, want)
    st = h.adapt_proposal(0, T, accepted_only=False)
    count, _, cov = ref_cov(prob, hist, 0, T, False, True)
    L, want = CR.adapt(count, cov, npar + 1, True, 1e-8)
    assert np.array_equal(st[cols], want)
    P = h.proposal()
    for q, c in enumerate(cols):
        assert np.array_equal(P[c], L[q] if want[q] == 0 else np.eye(npar)), c


def test_c3_partner_modes_past_one_pass(S):
    from smm_jl_amd.workloads import build_problem
    N, T = 32768, 40
    prob, opts = build_problem("c3", N, N, 0, T, 0)
    h = S.hip_context(prob, opts)
    h.step(T)
    ex = download(h, T, ("exchanged",)).exchanged
    got = h.chain_stats(0, T, False)
    assert np.array_equal(got["n_exchanged"], (ex != 0).sum(axis=0))
    want = np.array([R.mode_of_partners(ex[:, j]) for j in range(N)], np.int32)
    assert np.array_equal(got["most_exchanged_with"], want)
    assert N > STATS_MODE_BINS and want.max() > STATS_MODE_BINS
    lo, hi = ((ex > 0) & (ex <= STATS_MODE_BINS)).any(axis=0), (ex > STATS_MODE_BINS).any(axis=0)
    assert (lo & hi).any()                                     # some chain's partners in both passes
