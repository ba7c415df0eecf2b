"""smm_abc_pmc on the device at the edges its continuous test objectives never reach (tests/test_gpu_abc_pmc.py covers the shapes): every output
field bit for bit against the contract's restatement (tests/pmc_ref.py), a zero's sign included.  The crafted objectives, the committed sizes
and seeds and each case's condition are tests/pmc_craft.py's, held on the CPU in tests/test_pmc_craft.py.  Every case first runs the restatement
with an evaluator that is not new code (the context's eval_batch; the oracle for the built-in objective), asserts its condition on that, and
only then compares the device.
  A  ties at eps in every select (the staircase): the tie class over two and three iterations of k_pmc_select and over its waves, old kept
     and new candidates tied, -0.0 against +0.0 and negative distances in the key order, new particles at exactly the previous eps (p_acc's <)
  B  every distance equal (the constant): nothing new is kept, p_acc = 0 stops the run
  C  weights of 1 beside 2^20 (the bowl at ten parameters): parents from a skewed prefix; k_pmc_quantile asked at the integer CDF's own
     steps and their neighbours; and, at 64 parameters, log-weights 800 below the largest: smm_exp gives 0.0 and k_pmc_weights' floor alone
     makes q = 1
  D  1023, 1024, 1025 kept particles: k_pmc_weights' stride of 1024 with a non-uniform prefix behind it, a parent beyond index 1023
  E  k_pmc_kernel's grid with blockIdx.x > 0 and blockIdx.y > 0 together; a second pass added onto the D of a second workgroup
  F  generations without an evaluation (all outside) and without a finite distance (all invalid), kept sets below A that carry on and
     grow, A' == 1 and A' == 0 reached by parameter values
The underflow rule (D < DBL_MIN) cannot be reached through the public call (tests/pmc_craft.py): it stays with the CPU tier."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import common as cm  # noqa: E402
import pmc_craft as PC  # noqa: E402
from test_gpu_abc_pmc import compare  # noqa: E402
from test_gpu_opt_simplex import oracle_evaluator, registered  # noqa: E402

pytestmark = pytest.mark.gpu


def craft_case(S, name, udata, seed, npar=None):
    oid = registered(S, "pmc_" + name, lambda: S.register_user_objective(PC.SOURCES[name]))
    prob, opts = PC.problem(S, name, oid, udata, seed, npar)
    return prob, opts, S.hip_context(prob, opts)


def norm_case(S, O, ns, seed=12):
    prob, opts = cm.serial_normal(N=3, T=4, ns=ns, seed=seed)
    h = S.hip_context(prob, opts)
    return prob, opts, h, oracle_evaluator(S, O, prob, opts, h)


# ---- A, B -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,A,seed", list(PC.TIES_CASES))
def test_ties_at_eps_in_every_select(S, O, P, A, seed):
    prob, opts, h = craft_case(S, "staircase", PC.TIES_UDATA, seed)
    compare(O, h, h.eval_batch, prob, opts, P, A, condition=PC.ties_condition(P, A, seed), **PC.TIES)


def test_every_distance_equal(S, O):
    c = PC.CONSTANT_CASE
    prob, opts, h = craft_case(S, "constant", (), c["seed"])
    compare(O, h, h.eval_batch, prob, opts, c["P"], c["A"], c["max_gen"], c["p_acc_min"], condition=PC.constant_condition)


# ---- C --------------------------------------------------------------------------------------------------------------------------------------------
def test_skewed_weights_and_quantiles_at_the_cdf_steps(S, O):
    c = PC.SKEW
    prob, opts, h = craft_case(S, "bowl", (), c["seed"])
    kw = dict(P=c["P"], A=c["A"], max_gen=c["max_gen"], p_acc_min=c["p_acc_min"], scale=c["scale"], ridge=c["ridge"])
    _, plain = compare(O, h, h.eval_batch, prob, opts, probs=(), condition=PC.skew_condition, **kw)
    probs, steps = PC.skew_probs(plain)
    compare(O, h, h.eval_batch, prob, opts, probs=probs, condition=PC.skew_quantile_condition(steps), **kw)


def test_the_floor_of_the_sampling_weights(S, O):
    """smm_exp(lw - M) == 0.0 for the new kept particles: ceil gives 0, the floor makes q = 1"""
    c = PC.FLOOR
    prob, opts, h = craft_case(S, "bowl", (), c["seed"], c["npar"])
    compare(O, h, h.eval_batch, prob, opts, c["P"], c["A"], c["max_gen"], c["p_acc_min"], c["scale"], c["ridge"], c["probs"], condition=PC.floor_condition)


# ---- D, E -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", PC.STRIDE_A)
def test_kept_particles_around_the_weight_kernels_stride(S, O, A):
    c = PC.STRIDE
    prob, opts, h, ev = norm_case(S, O, 20, c["seed"])
    compare(O, h, ev, prob, opts, A + PC.STRIDE_NEW, A, c["max_gen"], c["p_acc_min"], c["scale"], probs=c["probs"], condition=PC.stride_condition(A))


def test_a_second_block_of_T_with_a_second_workgroup(S, O):
    c = PC.CORNER
    prob, opts, h, ev = norm_case(S, O, c["ns"])
    compare(O, h, ev, prob, opts, c["A"] + c["n_new"], c["A"], c["max_gen"], c["p_acc_min"], c["scale"], condition=PC.corner_condition)


def test_a_second_pass_with_a_second_workgroup(S, O):
    c = PC.PASS2
    prob, opts, h, ev = norm_case(S, O, c["ns"])
    compare(O, h, ev, prob, opts, c["P"], c["A"], c["max_gen"], c["p_acc_min"], c["scale"], probs=c["probs"], condition=PC.pass2_condition)


# ---- F --------------------------------------------------------------------------------------------------------------------------------------------
def test_every_new_particle_outside_the_box(S, O):
    c = PC.OUTSIDE
    for seed in c["seeds"]:
        prob, opts, h = craft_case(S, "islands", (c["hw"],), seed)
        compare(O, h, h.eval_batch, prob, opts, c["P"], c["A"], c["max_gen"], c["p_acc_min"], c["scale"], condition=PC.outside_condition)


@pytest.mark.parametrize("name", list(PC.THIN_CASES))
def test_thin_and_empty_generations(S, O, name):
    hw, P, scale, seeds = PC.THIN_CASES[name]
    for seed in seeds:
        prob, opts, h = craft_case(S, "islands", (hw,), seed)
        compare(O, h, h.eval_batch, prob, opts, P, PC.THIN_A, PC.THIN["max_gen"], PC.THIN["p_acc_min"], scale, probs=PC.THIN["probs"],
                condition=PC.thin_condition(name))
