"""Parameter-set batch: qd_optim_evalF_batch / qd_optim_evalGradF_batch evaluate several control vectors in one sweep launch.

Every system is synthetic (helpers.synthetic_spec), has at most 20 time steps and 16 initial conditions, and is held against the CPU
oracle through helpers.check_parity like the parity tests.  The control vectors of a call come from a seeded generator with amplitudes
that differ by a factor of 3 to 10 from set to set: a set that read another set's control table, or sums that mixed two sets' states,
cannot pass.  On the concurrent path the sweeps run on the SETS instantiations of the general kernels - qd_last_kernel names them with a
seventh template argument `true`.
"""
import numpy as np
import pytest

from helpers import OBJ_KEYS, check_parity, synthetic_cfg, synthetic_spec
from oracle.oracle import Oracle
from quandary_amd import capi, config

pytestmark = pytest.mark.gpu


def _alphas(sp, amps, seed, same=()):
    """One control vector per amplitude (rad/ns, uniform in +-amp); same = pairs (j, i): set j is a copy of set i."""
    rng = np.random.default_rng(seed)
    a = np.stack([amp * rng.uniform(-1.0, 1.0, sp.params0.size) for amp in amps])
    for j, i in same:
        a[j] = a[i]
    return a


def _oracle(sp, alphas, grad=True):
    orc = Oracle(sp)
    out = [orc.evalGradF(a) if grad else (orc.evalF(a)[0], None) for a in alphas]
    orc.close()
    return out


def _ran_on_set_kernels(h):
    """The general kernel family, in the instantiation that reads one control table per set."""
    f, a = h.last_kernel("forward"), h.last_kernel("adjoint")
    # (six template arguments as the single evaluation names them - the last one PLAIN - and SETS = true as the seventh)
    return all(k.startswith(b) and k.endswith(", true>") and k.count(",") == 6 for k, b in ((f, "k_forward<"), (a, "k_adjoint<")))


def _same_eval(a, b):
    (va, ga), (vb, gb) = a, b
    return all(va[k] == vb[k] for k in OBJ_KEYS) and np.array_equal(ga, gb)


# ---- the 2^4 Schroedinger system of tests 1 and 5: built once, the oracle asked once -------------------------------------------------
@pytest.fixture(scope="module")
def c3():
    sp = synthetic_spec([2, 2, 2, 2], lindblad=False, ntime=20, linsolve="neumann", stepper="IMR")
    sp.options = {"neumann_split": "0"}
    alphas = _alphas(sp, (0.02, 0.1, 0.02, 0.3), seed=20240, same=((2, 0),))
    return sp, alphas, _oracle(sp, alphas)


def test_batch_is_identical_to_single_evaluations(c3):
    """Three sets in one launch, set 2 a copy of set 0: values and gradients are bit for bit those of three evalGradF calls on the same
    handle (the same kernel instantiation sweeps every state, and every reduction runs per set in the order of the single evaluation),
    sets 0 and 2 are identical, and every set agrees with the oracle."""
    sp, alphas, ref = c3
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    assert opt.ninit <= 16
    vals, grads = opt.evalGradF_batch(alphas[:3])
    assert opt.last_batch_sets == 3
    assert _ran_on_set_kernels(h), (h.last_kernel("forward"), h.last_kernel("adjoint"))
    assert grads.shape == (3, h.ndesign)
    singles = [opt.evalGradF(a) for a in alphas[:3]]
    assert not _ran_on_set_kernels(h) and h.last_kernel("forward").count(",") == 5  # (the single evaluation keeps its own instantiation)
    for j in range(3):
        print(j, vals[j]["objective"], singles[j][0]["objective"], np.linalg.norm(grads[j] - singles[j][1]))
        assert _same_eval((vals[j], grads[j]), singles[j]), j
        check_parity(sp, vals[j], grads[j], *ref[j], alpha=alphas[j], msg=j)
    assert _same_eval((vals[0], grads[0]), (vals[2], grads[2]))
    assert not np.allclose(grads[0], grads[1], rtol=1e-3)
    opt.close(); h.close()


def test_adjoint_seeds_come_from_the_sets_own_cost():
    """Schroedinger + Jtrace seeds the adjoint sweep with the REDUCED cost (src/optimproblem.cpp:495-511): two sets whose fidelities are
    far apart, on C1's shape (2x2, CNOT, gmres) - a seed formed from the other set's cost, or from both, misses the oracle's gradient."""
    sp = synthetic_spec([2, 2], lindblad=False, ntime=20, dt=0.1, linsolve="gmres", stepper="IMR", gate="cnot", objective="Jtrace")
    alphas = _alphas(sp, (0.3, 2.0), seed=411)
    ref = _oracle(sp, alphas)
    assert abs(ref[0][0]["fidelity"] - ref[1][0]["fidelity"]) >= 0.1, (ref[0][0]["fidelity"], ref[1][0]["fidelity"])
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    vals, grads = opt.evalGradF_batch(alphas)
    assert opt.last_batch_sets == 2 and _ran_on_set_kernels(h), (h.last_kernel("forward"), h.last_kernel("adjoint"))
    for j in range(2):
        print(j, vals[j]["fidelity"], ref[j][0]["fidelity"], np.linalg.norm(grads[j] - ref[j][1]) / np.linalg.norm(ref[j][1]))
        check_parity(sp, vals[j], grads[j], *ref[j], alpha=alphas[j], msg=j)
    opt.close(); h.close()


@pytest.mark.parametrize("kw", [
    # rows of a table: 3 x ntime sub-steps; leakage, weighted-J and energy penalties on (the energy table has a set axis of its own)
    pytest.param(dict(nlevels=[3, 3], lindblad=True, nessential=[2, 2], penalties=True, stepper="IMR4"), id="3a-3x3-lindblad-guard-penalties-IMR4"),
    # columns of a row: 2 + 2Q + 2 npairs, the pair columns cos / sin(eta t) with three different rotating frames
    pytest.param(dict(nlevels=[2, 2, 2], lindblad=False, jkl=0.02, target="pure", objective="Jmeasure"), id="3b-2x2x2-coupled"),
    # explicit Euler: ntime + 1 rows, the adjoint sweep reads row s + 1
    pytest.param(dict(nlevels=[2, 2], lindblad=True, stepper="EE"), id="3c-2x2-lindblad-EE"),
    pytest.param(dict(nlevels=[2, 2], lindblad=False, stepper="EE"), id="3c-2x2-schroedinger-EE"),
])
def test_table_stride_between_sets(kw):
    """The second set's table starts (rows the table really has) x cs doubles behind the first: composite steppers, the extra row of
    explicit Euler and the pair columns of coupled systems all move it."""
    sp = synthetic_spec(**{"ntime": 12, "linsolve": "neumann", **kw})
    alphas = _alphas(sp, (0.1, 0.5), seed=77)
    ref = _oracle(sp, alphas)
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    assert opt.ninit <= 16
    vals, grads = opt.evalGradF_batch(alphas)
    assert opt.last_batch_sets == 2 and _ran_on_set_kernels(h), (h.last_kernel("forward"), h.last_kernel("adjoint"))
    for j in range(2):
        print(j, vals[j]["objective"], ref[j][0]["objective"], np.linalg.norm(grads[j] - ref[j][1]) / np.linalg.norm(ref[j][1]))
        check_parity(sp, vals[j], grads[j], *ref[j], alpha=alphas[j], msg=j)
    # forward only: the same objective parts
    fvals = opt.evalF_batch(alphas)
    assert opt.last_batch_sets == 2
    for j in range(2):
        for k in OBJ_KEYS:
            assert fvals[j][k] == vals[j][k], (j, k)
    opt.close(); h.close()


def test_fallback_serves_the_lean_kernels_set_by_set():
    """2^4 Lindblad runs on the lean slot kernels, which have no set axis: the call is a loop over the single evaluation."""
    sp = synthetic_spec([2, 2, 2, 2], lindblad=True, ntime=10, init="diagonal")
    alphas = _alphas(sp, (0.02, 0.1), seed=5)
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    assert opt.ninit == 16
    vals, grads = opt.evalGradF_batch(alphas)
    assert opt.last_batch_sets == 1
    assert h.last_kernel("forward").startswith("k_forward_q32<"), h.last_kernel("forward")
    for j in range(2):
        assert _same_eval((vals[j], grads[j]), opt.evalGradF(alphas[j])), j
    fvals = opt.evalF_batch(alphas)
    assert opt.last_batch_sets == 1 and all(fvals[j] == opt.evalF(alphas[j]) for j in range(2))
    opt.close(); h.close()


def test_sets_that_do_not_fit_together_go_in_groups(c3):
    """Four sets under a trajectory budget that holds two sets' states and stages, not three: two launches of two sets each, the same
    numbers as the single evaluations."""
    sp, alphas, ref = c3
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    per_set = (2 * sp.time.ntime + 1) * opt.ninit * 2 * h.dim * 8  # states x_0..x_n and primal stages of one set, in bytes
    h.set_option("traj_budget_mb", 2.5 * per_set / 1048576.0)
    vals, grads = opt.evalGradF_batch(alphas)
    assert opt.last_batch_sets == 2 and _ran_on_set_kernels(h)
    h.set_option("traj_budget_mb", 0)
    for j in range(4):
        assert _same_eval((vals[j], grads[j]), opt.evalGradF(alphas[j])), j
        check_parity(sp, vals[j], grads[j], *ref[j], alpha=alphas[j], msg=j)
    h.set_option("traj_budget_mb", 0.5 * per_set / 1048576.0)  # not even one set: the single evaluation's chunks, set by set
    vals1, grads1 = opt.evalGradF_batch(alphas[:2])
    assert opt.last_batch_sets == 1 and opt.last_chunks >= 2
    for j in range(2):
        check_parity(sp, vals1[j], grads1[j], *ref[j], alpha=alphas[j], msg=j)
    opt.close(); h.close()


def test_handle_state_and_errors():
    sp = synthetic_spec([2, 2], lindblad=True, ntime=10)
    alphas = _alphas(sp, (0.03, 0.2), seed=9)
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    before = opt.evalF(sp.params0)
    opt.evalGradF(sp.params0)
    opt.evalGradF_batch(alphas)
    assert opt.last_batch_sets == 2
    with pytest.raises(capi.QuandaryAmdError, match=r"rc=-5"):  # QD_ERR_STATE: no stored trajectory after a batch call
        h.get_state(0, opt.ninit)
    assert opt.evalF(sp.params0) == before
    opt.evalF_batch(alphas)
    assert opt.evalF(sp.params0) == before
    with pytest.raises(capi.QuandaryAmdError, match=r"rc=-1"):  # QD_ERR_INVALID
        opt.evalF_batch(np.zeros((0, h.ndesign)))
    with pytest.raises(capi.QuandaryAmdError, match=r"rc=-1"):
        opt.evalGradF_batch(np.zeros((0, h.ndesign)))
    shard = capi.Optim(h, sp, rank=0, nranks=2)
    with pytest.raises(capi.QuandaryAmdError, match=r"rc=-5"):  # QD_ERR_STATE: single rank only
        shard.evalF_batch(alphas)
    with pytest.raises(capi.QuandaryAmdError, match=r"rc=-5"):
        shard.evalGradF_batch(alphas)
    shard.close(); opt.close(); h.close()


def test_pipulse_system_forward_only():
    """A pi-pulse has no derivative in the reference: the forward batch works, the gradient batch is rejected like the single call."""
    text = synthetic_cfg([2, 2], lindblad=True, ntime=20) + "apply_pipulse = 0, 0.05, 0.1, 2.0\n"
    sp = config.build_spec(config.parse_config_text(text))
    alphas = _alphas(sp, (0.03, 0.2), seed=10)
    ref = _oracle(sp, alphas, grad=False)
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    vals = opt.evalF_batch(alphas)
    for j in range(2):
        check_parity(sp, vals[j], None, ref[j][0], None, alpha=alphas[j], msg=j)
        assert vals[j] == opt.evalF(alphas[j])
    with pytest.raises(capi.QuandaryAmdError, match=r"rc=-2") as single:  # QD_ERR_UNSUPPORTED
        opt.evalGradF(alphas[0])
    with pytest.raises(capi.QuandaryAmdError, match=r"rc=-2") as batch:
        opt.evalGradF_batch(alphas)
    assert "pi-pulses" in str(single.value) and "pi-pulses" in str(batch.value)
    opt.close(); h.close()
