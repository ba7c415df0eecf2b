"""The proposal factor's layout (none, shared [np][np], per chain [N][np][np]) is fixed when a context is created: the host buffers of
BGPContext.proposal / set_proposal follow the context, never the caller's opts object, which may be reused for other contexts.  CPU
only: the context's library is replaced by a stand-in that records what it is handed."""
import numpy as np
import pytest

from smm_jl_amd import BGPContext, BGPOpts, Problem


class StandIn:
    """what BGPContext calls of libsmmhip.so; get/set_proposal record the length of the array they were handed"""

    def __init__(self):
        self.seen = []

    def smm_ctx_create(self, p, o, t, ctx):
        return 0

    def smm_ctx_destroy(self, ctx):
        pass

    def smm_last_error(self, ctx):
        return b"stand-in"

    def smm_get_proposal(self, ctx, ptr):
        return 0

    def smm_set_proposal(self, ctx, ptr):
        return 0


class Ctx(BGPContext):
    def __init__(self, problem, opts):
        self._lib = StandIn()
        self._create(problem, opts, None)


def make(N, npar, chol_L):
    prob = Problem(init=np.zeros(npar), lb=-np.ones(npar), ub=np.ones(npar), mom=np.zeros(npar), w=np.ones(npar), ns=10)
    opts = BGPOpts(N=N, maxiter=5, sigma=np.full(N, 0.1), acc_tuner=np.ones(N), min_improve=np.zeros(N), chol_L=chol_L)
    return prob, opts


@pytest.mark.parametrize("reuse", [None, "shared"])
def test_per_chain_layout_survives_reuse_of_opts(reuse):
    N, npar = 7, 3
    prob, opts = make(N, npar, np.broadcast_to(np.eye(npar), (N, npar, npar)))
    h = Ctx(prob, opts)
    opts.chol_L = None if reuse is None else np.eye(npar)   # the caller builds another context from the same opts
    assert h.proposal_layout == "per_chain"
    assert h.proposal().shape == (N, npar, npar)
    with pytest.raises(ValueError):
        h.set_proposal(np.eye(npar))
    h.set_proposal(np.broadcast_to(np.eye(npar), (N, npar, npar)))


def test_shared_layout_survives_reuse_of_opts():
    N, npar = 5, 4
    prob, opts = make(N, npar, np.eye(npar))
    h = Ctx(prob, opts)
    opts.chol_L = np.broadcast_to(np.eye(npar), (N, npar, npar))
    assert h.proposal_layout == "shared"
    assert h.proposal().shape == (npar, npar)
    with pytest.raises(ValueError):
        h.set_proposal(opts.chol_L)


def test_no_factor_layout():
    prob, opts = make(4, 2, None)
    h = Ctx(prob, opts)
    opts.chol_L = np.eye(2)
    assert h.proposal_layout is None and h._proposal_shape() is None
