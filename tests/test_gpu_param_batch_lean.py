"""Parameter-set batch on the lean slot kernels (option batch_lean = 1): the batch entry points share one sweep launch on the lean slot
family (2^4 / 2^5 Lindblad, fp64) and on the fp32-mixed sweeps, where the kernel's solver is a stationary iteration.  Those launches run
on k_forward_q32_sets / k_adjoint_q32_sets, which read one control table per set; qd_last_kernel names them with the five template
arguments of the kernel the single evaluation runs on.  Without the option (the default) such systems go set by set, as before.

Every system is synthetic (helpers.synthetic_spec) with at most 20 time steps and 32 initial conditions.  The control vectors of a call
come from a seeded generator with amplitudes that differ by a factor of 3 to 10 from set to set (the idea of test_gpu_param_batch.py): a
set that read another set's control table cannot pass.  The fp64 cases are held against the CPU oracle through helpers.check_parity; the
fp32-mixed cases against the single fp32-mixed evaluation on the same handle, bit for bit - its parity is what test_gpu_f32mixed.py
asserts, so no new tolerance appears here.
"""
import numpy as np
import pytest

from helpers import OBJ_KEYS, check_parity, synthetic_spec
from oracle.oracle import Oracle
from quandary_amd import capi

pytestmark = pytest.mark.gpu

LEAN = {"batch_lean": "1"}


def _alphas(sp, amps, seed, same=()):
    """One control vector per amplitude (rad/ns, uniform in +-amp); same = pairs (j, i): set j is a copy of set i."""
    rng = np.random.default_rng(seed)
    a = np.stack([amp * rng.uniform(-1.0, 1.0, sp.params0.size) for amp in amps])
    for j, i in same:
        a[j] = a[i]
    return a


def _oracle(sp, alphas):
    orc = Oracle(sp)
    out = [orc.evalGradF(a) for a in alphas]
    orc.close()
    return out


def _kernels(h):
    return h.last_kernel("forward"), h.last_kernel("adjoint")


def _sets_kernels(args):
    return f"k_forward_q32_sets<{args}>", f"k_adjoint_q32_sets<{args}>"


def _plain_kernels(args):
    return f"k_forward_q32<{args}>", f"k_adjoint_q32<{args}>"


def _same_eval(a, b):
    (va, ga), (vb, gb) = a, b
    return all(va[k] == vb[k] for k in OBJ_KEYS) and np.array_equal(ga, gb)


# ---- the 2^4 Lindblad system of tests 1, 2, 6 and 7: sixteen states, ten steps; the oracle asked once ---------------------------------
def _q4_spec(options):
    sp = synthetic_spec([2, 2, 2, 2], lindblad=True, ntime=10, init="diagonal", linsolve="neumann")
    sp.options = dict(options)
    return sp


@pytest.fixture(scope="module")
def q4():
    sp = _q4_spec(LEAN)
    alphas = _alphas(sp, (0.02, 0.1, 0.02, 0.2), seed=31415, same=((2, 0),))
    return alphas, _oracle(sp, alphas)


Q4 = "4, 0, double, false, false"


def test_batch_is_identical_to_single_evaluations(q4):
    """Three sets in one launch, set 2 a copy of set 0: values and gradients are bit for bit those of three evalGradF calls on the same
    handle, sets 0 and 2 are identical, 0 and 1 differ, every set agrees with the oracle, and evalF_batch returns the same parts."""
    alphas, ref = q4
    sp = _q4_spec(LEAN)
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    assert opt.ninit == 16
    vals, grads = opt.evalGradF_batch(alphas[:3])
    assert opt.last_batch_sets == 3
    assert _kernels(h) == _sets_kernels(Q4), _kernels(h)
    assert grads.shape == (3, h.ndesign)
    singles = [opt.evalGradF(a) for a in alphas[:3]]
    assert _kernels(h) == _plain_kernels(Q4), _kernels(h)  # (the single evaluation keeps its own kernels)
    for j in range(3):
        print(j, vals[j]["objective"], singles[j][0]["objective"], np.linalg.norm(grads[j] - singles[j][1]))
        assert _same_eval((vals[j], grads[j]), singles[j]), j
        check_parity(sp, vals[j], grads[j], *ref[j], alpha=alphas[j], msg=j)
    assert _same_eval((vals[0], grads[0]), (vals[2], grads[2]))
    assert not np.allclose(grads[0], grads[1], rtol=1e-3)
    fvals = opt.evalF_batch(alphas[:3])
    assert opt.last_batch_sets == 3 and h.last_kernel("forward") == _sets_kernels(Q4)[0]
    for j in range(3):
        for k in OBJ_KEYS:
            assert fvals[j][k] == vals[j][k], (j, k)
    opt.close(); h.close()


def test_default_stays_set_by_set(q4):
    """The same system without the option: a loop over the single evaluation on the plain kernels (passes with and without the feature)."""
    alphas, ref = q4
    sp = _q4_spec({})
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    vals, grads = opt.evalGradF_batch(alphas[:3])
    assert opt.last_batch_sets == 1
    assert _kernels(h) == _plain_kernels(Q4), _kernels(h)
    for j in range(3):
        check_parity(sp, vals[j], grads[j], *ref[j], alpha=alphas[j], msg=j)
    opt.evalF_batch(alphas[:3])
    assert opt.last_batch_sets == 1 and h.last_kernel("forward") == _plain_kernels(Q4)[0]
    opt.close(); h.close()


# ---- table stride and columns, fp64 ---------------------------------------------------------------------------------------------------
def _batch_against_oracle_and_singles(sp, alphas, ref, args):
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    assert opt.ninit <= 32
    vals, grads = opt.evalGradF_batch(alphas)
    assert opt.last_batch_sets == len(alphas)
    assert _kernels(h) == _sets_kernels(args), _kernels(h)
    for j in range(len(alphas)):
        single = opt.evalGradF(alphas[j])
        assert _kernels(h) == _plain_kernels(args), _kernels(h)
        print(j, vals[j]["objective"], ref[j][0]["objective"], np.linalg.norm(grads[j] - ref[j][1]) / np.linalg.norm(ref[j][1]))
        assert _same_eval((vals[j], grads[j]), single), j
        check_parity(sp, vals[j], grads[j], *ref[j], alpha=alphas[j], msg=j)
    assert not np.allclose(grads[0], grads[1], rtol=1e-3)
    opt.close(); h.close()


def test_pair_columns_substeps_and_penalty():
    """2^4 with dipole-dipole coupling under IMR4 with penalties: the pair columns cos / sin(eta t) widen a row, three sub-steps per step
    lengthen a table, and the weighted-J penalty makes the adjoint sweep read the stored states."""
    sp = synthetic_spec([2, 2, 2, 2], lindblad=True, ntime=10, init="diagonal", linsolve="neumann", jkl=0.02, penalties=True, stepper="IMR4")
    sp.options = dict(LEAN)
    alphas = _alphas(sp, (0.03, 0.2), seed=77)
    _batch_against_oracle_and_singles(sp, alphas, _oracle(sp, alphas), "4, 0, double, false, true")


def _q5_spec(options):
    sp = synthetic_spec([2, 2, 2, 2, 2], lindblad=True, ntime=6, init="diagonal", linsolve="neumann")
    sp.options = dict(options)
    return sp


@pytest.fixture(scope="module")
def q5():
    sp = _q5_spec(LEAN)
    alphas = _alphas(sp, (0.03, 0.2), seed=55)
    return alphas, _oracle(sp, alphas)


@pytest.mark.parametrize("sb", [1, 2])
def test_two_to_the_five_with_pinned_elements_per_thread(q5, sb):
    """2^5, 32 states: two (512 threads) and four (256 threads) elements per thread.  The automatic choice counts the states of the whole
    launch, so a batch may pick another instantiation than the single evaluation: bit-identity is asserted under the pinned value."""
    alphas, ref = q5
    sp = _q5_spec({**LEAN, "lean64_sb": str(sb)})
    _batch_against_oracle_and_singles(sp, alphas, ref, f"5, {sb}, double, false, false")


def test_two_to_the_five_coupled():
    sp = synthetic_spec([2, 2, 2, 2, 2], lindblad=True, ntime=6, init="diagonal", linsolve="neumann", jkl=0.02)
    sp.options = dict(LEAN)
    alphas = _alphas(sp, (0.03, 0.2), seed=56)
    _batch_against_oracle_and_singles(sp, alphas, _oracle(sp, alphas), "5, 1, double, false, true")


# ---- fp32-mixed -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,kw,opts,args", [
    pytest.param(3, {}, {}, "3, 0, float, false, false", id="q3"),
    pytest.param(4, dict(jkl=0.02), {}, "4, 0, float, false, true", id="q4-coupled"),
    pytest.param(5, {}, {"lean64_sb": "1"}, "5, 1, float, false, false", id="q5-sb1"),
])
def test_f32mixed_batch_is_identical_to_single_evaluations(nq, kw, opts, args):
    """Two sets in one launch of the fp32-mixed sweeps: bit for bit the single fp32-mixed evaluations on the same handle."""
    sp = synthetic_spec([2] * nq, lindblad=True, ntime=20, init="diagonal", linsolve="neumann", **kw)
    sp.precision = "f32mixed"
    sp.options = {**LEAN, **opts}
    alphas = _alphas(sp, (0.03, 0.2), seed=90 + nq)
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    assert opt.ninit == 2 ** nq
    vals, grads = opt.evalGradF_batch(alphas)
    assert opt.last_batch_sets == 2
    assert _kernels(h) == _sets_kernels(args), _kernels(h)
    for j in range(2):
        single = opt.evalGradF(alphas[j])
        assert _kernels(h) == _plain_kernels(args), _kernels(h)
        print(j, vals[j]["objective"], single[0]["objective"], np.linalg.norm(grads[j] - single[1]))
        assert _same_eval((vals[j], grads[j]), single), j
    assert vals[0]["objective"] != vals[1]["objective"] and not np.allclose(grads[0], grads[1], rtol=1e-3)
    fvals = opt.evalF_batch(alphas)
    assert opt.last_batch_sets == 2
    for j in range(2):
        for k in OBJ_KEYS:
            assert fvals[j][k] == vals[j][k], (j, k)
    opt.close(); h.close()


# ---- what stays set by set, groups, handle state ------------------------------------------------------------------------------------------
def test_krylov_plan_falls_back():
    """linearsolver_type = gmres with gmres_split = 0 keeps the Krylov kernels, which have no set axis: set by set under batch_lean too.
    The degree of their polynomial preconditioner is tuned from sweep to sweep until it freezes (qd_handle::forward_finish), so two
    evaluations of one control vector are bit-identical only at the same degree: the comparison with the single calls runs with the
    degree pinned (option gmres_poly), after the fallback itself has been checked under the tuner."""
    sp = synthetic_spec([2, 2, 2, 2], lindblad=True, ntime=10, init="diagonal", linsolve="gmres")
    sp.options = {"gmres_split": "0", **LEAN}
    alphas = _alphas(sp, (0.02, 0.1), seed=5)
    ref = _oracle(sp, alphas)
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    vals, grads = opt.evalGradF_batch(alphas)
    assert opt.last_batch_sets == 1 and h.last_solver == "krylov"
    assert _kernels(h) == _plain_kernels("4, 0, double, true, false"), _kernels(h)
    for j in range(2):
        check_parity(sp, vals[j], grads[j], *ref[j], alpha=alphas[j], msg=j)
    h.set_option("gmres_poly", 6)
    vals, grads = opt.evalGradF_batch(alphas)
    assert opt.last_batch_sets == 1 and h.last_solver == "krylov"
    for j in range(2):
        assert _same_eval((vals[j], grads[j]), opt.evalGradF(alphas[j])), j
    opt.close(); h.close()


def test_sets_that_do_not_fit_together_go_in_groups(q4):
    """Four sets under a trajectory budget that holds two sets' stored stages and not three: two launches of two sets each."""
    alphas, ref = q4
    sp = _q4_spec(LEAN)
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    per_set = sp.time.ntime * opt.ninit * 2 * h.dim * 8  # primal stages of one set in bytes (this adjoint sweep reads no states)
    h.set_option("traj_budget_mb", 2.5 * per_set / 1048576.0)
    vals, grads = opt.evalGradF_batch(alphas)
    assert opt.last_batch_sets == 2
    assert _kernels(h) == _sets_kernels(Q4), _kernels(h)
    h.set_option("traj_budget_mb", 0)
    for j in range(4):
        assert _same_eval((vals[j], grads[j]), opt.evalGradF(alphas[j])), j
        check_parity(sp, vals[j], grads[j], *ref[j], alpha=alphas[j], msg=j)
    opt.close(); h.close()


def test_handle_state_after_a_batch_call(q4):
    alphas, _ = q4
    sp = _q4_spec(LEAN)
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    before = opt.evalF(sp.params0)
    opt.evalGradF(sp.params0)
    opt.evalGradF_batch(alphas[:2])
    assert opt.last_batch_sets == 2
    with pytest.raises(capi.QuandaryAmdError, match=r"rc=-5"):  # QD_ERR_STATE: no stored trajectory after a batch call
        h.get_state(0, opt.ninit)
    assert opt.evalF(sp.params0) == before
    opt.evalF_batch(alphas[:2])
    assert opt.last_batch_sets == 2
    assert opt.evalF(sp.params0) == before
    opt.close(); h.close()
