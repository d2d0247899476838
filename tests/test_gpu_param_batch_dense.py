"""Parameter-set batch on user-supplied Hamiltonians (qd_set_hamiltonian): qd_optim_evalF_batch / qd_optim_evalGradF_batch share one
sweep launch on the dense kernels of the general family - variants 11, 12, 13 (DenseStencil), 15 and 17 (matrix cores) - where every
set reads its own table of G(t) = -i H(t) beside its own control table (SweepArgs::gtab_set, k_gmat with the sets on grid.y).

Every system has at most 12 time steps of 0.004 ns and 16 initial conditions, random Hermitian Hsys / Hc_k, and is held against the CPU
oracle through helpers.check_parity.  The control vectors of a call come from a seeded generator with amplitudes a factor 3 to 10 apart,
and before any GPU assertion the oracle's own gradients of two sets are checked to differ (rtol 1e-3): a set that read another set's
G(t) table cannot pass.  On the concurrent path qd_last_kernel names the SETS instantiation, a seventh template argument `true`.
"""
import numpy as np
import pytest

from helpers import OBJ_KEYS, check_parity, synthetic_spec
from oracle.oracle import Oracle
from quandary_amd import capi

pytestmark = pytest.mark.gpu


def _random_hamiltonians(n, nosc, seed):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    hsys = 0.3 * (a + a.conj().T)
    hc = []
    for _ in range(nosc):
        b = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
        hc.append(0.5 * (b + b.conj().T))
    return hsys, np.array(hc)


def _dense_spec(nlevels, ham_seed=11, options=None, **kw):
    sp = synthetic_spec(nlevels, **{"ntime": 12, "dt": 0.004, "linsolve": "neumann", **kw})
    assert sp.time.ntime <= 12 and sp.time.dt == 0.004
    sp.hamiltonian = _random_hamiltonians(int(np.prod(nlevels)), len(nlevels), ham_seed)
    if options:
        sp.options = dict(options)
    return sp


def _alphas(sp, amps, seed, same=()):
    """One control vector per amplitude (rad/ns, uniform in +-amp); same = pairs (j, i): set j is a copy of set i."""
    rng = np.random.default_rng(seed)
    a = np.stack([amp * rng.uniform(-1.0, 1.0, sp.params0.size) for amp in amps])
    for j, i in same:
        a[j] = a[i]
    return a


def _oracle(sp, alphas):
    """The oracle's evaluations of every set; the first two must differ, or the test could not tell the sets' tables apart."""
    orc = Oracle(sp)
    out = [orc.evalGradF(a) for a in alphas]
    orc.close()
    assert not np.allclose(out[0][1], out[1][1], rtol=1e-3), "the oracle's gradients of sets 0 and 1 do not differ"
    return out


VECTOR = (11, 12, 13)  # DenseStencil on the vector units: one, two and four elements per thread


def _variant(h):
    return int(h.last_kernel("forward").split(",")[2])


def _set_kernels(h, q, lind, var=None):
    """Both sweeps ran on the SETS instantiation k_*<Q, LIND, VAR, QUBIT, GM, PLAIN, true> of the given dense variant (None: of
    whichever vector variant the forward sweep names)."""
    if var is None:
        var = _variant(h)
        assert var in VECTOR, h.last_kernel("forward")
    head = f"<{q}, {'true' if lind else 'false'}, {var}, "
    f, a = h.last_kernel("forward"), h.last_kernel("adjoint")
    return all(k.startswith(b + head) and k.endswith(", true>") and k.count(",") == 6 for k, b in ((f, "k_forward"), (a, "k_adjoint")))


def _single_kernels(h, q, lind, var):
    head = f"<{q}, {'true' if lind else 'false'}, {var}, "
    f, a = h.last_kernel("forward"), h.last_kernel("adjoint")
    return all(k.startswith(b + head) and k.count(",") == 5 for k, b in ((f, "k_forward"), (a, "k_adjoint")))


def _same_eval(a, b):
    (va, ga), (vb, gb) = a, b
    return all(va[k] == vb[k] for k in OBJ_KEYS) and np.array_equal(ga, gb)


def _kernels(h):
    return h.last_kernel("forward"), h.last_kernel("adjoint")


# ---- the 2x2 Lindblad system of tests 1 and 5: built once, the oracle asked once ------------------------------------------------------
@pytest.fixture(scope="module")
def l22():
    sp = _dense_spec([2, 2], lindblad=True)
    alphas = _alphas(sp, (0.02, 0.1, 0.02, 0.3), seed=20240, same=((2, 0),))
    return sp, alphas, _oracle(sp, alphas)


def test_batch_is_identical_to_single_evaluations(l22):
    """1. Three sets in one launch, set 2 a copy of set 0: values and gradients are bit for bit those of three evalGradF calls on the
    same handle (k_gmat forms every element of a set's G(t) with the fma order of the single table), sets 0 and 2 are identical, and
    every set agrees with the oracle."""
    sp, alphas, ref = l22
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    assert opt.ninit == 16
    vals, grads = opt.evalGradF_batch(alphas[:3])
    assert opt.last_batch_sets == 3
    assert _set_kernels(h, 2, True, 11), _kernels(h)
    assert grads.shape == (3, h.ndesign)
    singles = [opt.evalGradF(a) for a in alphas[:3]]
    assert _single_kernels(h, 2, True, 11), _kernels(h)  # (the single evaluation keeps its own instantiation)
    for j in range(3):
        print(j, vals[j]["objective"], singles[j][0]["objective"], np.linalg.norm(grads[j] - singles[j][1]))
        assert _same_eval((vals[j], grads[j]), singles[j]), j
        check_parity(sp, vals[j], grads[j], *ref[j], alpha=alphas[j], msg=j)
    assert _same_eval((vals[0], grads[0]), (vals[2], grads[2]))
    assert not np.allclose(grads[0], grads[1], rtol=1e-3)
    opt.close(); h.close()


@pytest.mark.parametrize("kw,var,options", [
    pytest.param(dict(nlevels=[3, 4], lindblad=True, nessential=[2, 3], target="pure", objective="Jfrobenius", init="diagonal"), 12, None, id="2a-3x4-lindblad-guard-v12"),
    # 4x6 Lindblad was listed for variant 13 under the default options.  That expectation was wrong: pick_config gives every dense Lindblad
    # system with 22 <= N <= 32 rows to the matrix-core kernel on padded tiles (17); variant 13 - four elements per thread - serves the
    # same system under no_mfma = 1.  Both run: the case as listed, asserting the variant it really runs on, and its twin on 13.
    pytest.param(dict(nlevels=[4, 6], lindblad=True, target="pure", objective="Jmeasure", init="diagonal, 0"), 17, None, id="2b-4x6-lindblad-v17"),
    pytest.param(dict(nlevels=[4, 6], lindblad=True, target="pure", objective="Jmeasure", init="diagonal, 0"), 13, {"no_mfma": "1"}, id="2b-4x6-lindblad-no_mfma-v13"),
    pytest.param(dict(nlevels=[10, 12], lindblad=False, target="pure", objective="Jmeasure", init="pure, 1, 2"), None, None, id="2c-120-schroedinger-L2"),
    pytest.param(dict(nlevels=[4, 4], lindblad=True, nessential=[3, 3], target="pure", objective="Jfrobenius", init="diagonal, 0"), 15, None, id="2d-4x4-lindblad-v15"),
    pytest.param(dict(nlevels=[3, 3, 3], lindblad=True, nessential=[2, 3, 2], target="pure", objective="Jfrobenius", init="diagonal, 1"), 17, None, id="2e-3x3x3-lindblad-v17"),
    pytest.param(dict(nlevels=[4, 4], lindblad=True, nessential=[3, 3], target="pure", objective="Jfrobenius", init="diagonal, 0"), "vector", {"no_mfma": "1"}, id="2f-4x4-lindblad-no_mfma"),
])
def test_every_dense_variant(kw, var, options):
    """2. Two sets on every dense variant: G(t) of the sub-step staged in LDS (N <= 64, S.dense == 2) and read through L2 (N = 120,
    S.dense == 1), the vector kernels with one and four elements per thread, and both matrix-core kernels."""
    sp = _dense_spec(options=options, penalties=True, **kw)
    alphas = _alphas(sp, (0.1, 0.5), seed=77)
    ref = _oracle(sp, alphas)
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    assert opt.ninit <= 16
    vals, grads = opt.evalGradF_batch(alphas)
    q, lind = len(kw["nlevels"]), kw["lindblad"]
    print(_kernels(h))
    assert opt.last_batch_sets == 2, _kernels(h)
    f, ran = h.last_kernel("forward"), _variant(h)
    if var == "vector":
        assert ran in VECTOR, f
    elif var is None:
        assert ran in VECTOR and int(np.prod(kw["nlevels"])) > 64, f  # (N = 120: the table is too large for LDS)
    else:
        assert ran == var, f
    assert _set_kernels(h, q, lind, ran), _kernels(h)
    for j in range(2):
        print(j, vals[j]["objective"], ref[j][0]["objective"], np.linalg.norm(grads[j] - ref[j][1]) / np.linalg.norm(ref[j][1]))
        check_parity(sp, vals[j], grads[j], *ref[j], alpha=alphas[j], msg=j)
    single = opt.evalGradF(alphas[1])
    assert _single_kernels(h, q, lind, ran), _kernels(h)
    assert _same_eval((vals[1], grads[1]), single)
    opt.close(); h.close()


@pytest.mark.parametrize("kw", [
    pytest.param(dict(nlevels=[2, 2], lindblad=True, stepper="IMR4"), id="3a-2x2-lindblad-IMR4"),      # three rows per step
    pytest.param(dict(nlevels=[2, 2], lindblad=False, stepper="EE"), id="3b-2x2-schroedinger-EE"),    # one row more; the adjoint reads row s + 1
])
def test_table_stride_between_sets(kw):
    """3. The second set's G(t) table starts (rows the table really has) x N^2 x 2 doubles behind the first."""
    sp = _dense_spec(**kw)
    alphas = _alphas(sp, (0.1, 0.5), seed=77)
    ref = _oracle(sp, alphas)
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    assert opt.ninit <= 16
    vals, grads = opt.evalGradF_batch(alphas)
    assert opt.last_batch_sets == 2 and _set_kernels(h, 2, kw["lindblad"]), _kernels(h)
    for j in range(2):
        print(j, vals[j]["objective"], ref[j][0]["objective"], np.linalg.norm(grads[j] - ref[j][1]) / np.linalg.norm(ref[j][1]))
        check_parity(sp, vals[j], grads[j], *ref[j], alpha=alphas[j], msg=j)
    fvals = opt.evalF_batch(alphas)  # forward only: the same objective parts
    assert opt.last_batch_sets == 2
    for j in range(2):
        for k in OBJ_KEYS:
            assert fvals[j][k] == vals[j][k], (j, k)
    opt.close(); h.close()


# control amplitudes (a factor 10 apart), generator seed and Hamiltonian seed of test 4: chosen on the CPU so that the oracle's two
# fidelities lie at least 0.1 apart over 12 steps of 0.004 ns
SEEDS_AMPS, SEEDS_SEED, SEEDS_HAM = (3.0, 30.0), 411, 11


@pytest.mark.parametrize("mode", [None, "0"], ids=["default-solver", "gmres_split-0"])
def test_adjoint_seeds_come_from_the_sets_own_cost(mode):
    """4. Schroedinger + Jtrace seeds the adjoint sweep with the REDUCED cost: two sets whose fidelities are far apart, under a gmres
    request - served by the default solver path and, with gmres_split = 0, by the Krylov kernels (the GM = true SETS instantiation)."""
    sp = _dense_spec([2, 2], lindblad=False, linsolve="gmres", gate="cnot", objective="Jtrace", ham_seed=SEEDS_HAM,
                     options=None if mode is None else {"gmres_split": mode})
    alphas = _alphas(sp, SEEDS_AMPS, seed=SEEDS_SEED)
    ref = _oracle(sp, alphas)
    assert abs(ref[0][0]["fidelity"] - ref[1][0]["fidelity"]) >= 0.1, (ref[0][0]["fidelity"], ref[1][0]["fidelity"])
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    vals, grads = opt.evalGradF_batch(alphas)
    print(_kernels(h), h.last_solver)
    assert opt.last_batch_sets == 2 and _set_kernels(h, 2, False), _kernels(h)
    if mode == "0":
        assert h.last_solver == "krylov" and h.last_kernel("forward").split(", ")[4] == "true", (h.last_solver, _kernels(h))
    for j in range(2):
        print(j, vals[j]["fidelity"], ref[j][0]["fidelity"], np.linalg.norm(grads[j] - ref[j][1]) / np.linalg.norm(ref[j][1]))
        check_parity(sp, vals[j], grads[j], *ref[j], alpha=alphas[j], msg=j)
    opt.close(); h.close()


def test_sets_that_do_not_fit_together_go_in_groups(l22):
    """5. Four sets under a trajectory budget that holds two sets' states, stages and G(t) tables, not three: two launches of two sets
    each, the same numbers as the single evaluations.  A budget below one set: set by set."""
    sp, alphas, ref = l22
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    n = 4  # rows of the density matrix = rows of G
    traj = (2 * sp.time.ntime + 1) * opt.ninit * 2 * h.dim * 8  # states x_0..x_n and primal stages of one set, in bytes
    gtab = sp.time.ntime * n * n * 16                            # one row of G(t) per step of the implicit midpoint rule
    per_set = traj + gtab
    h.set_option("traj_budget_mb", 2.5 * per_set / 1048576.0)
    vals, grads = opt.evalGradF_batch(alphas)
    assert opt.last_batch_sets == 2 and _set_kernels(h, 2, True, 11), _kernels(h)
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


def test_global_memory_kernels_go_set_by_set():
    """6a. 6x6 Lindblad with guard levels (dim 1296) runs on the global-memory kernels, which have no set axis: the call is a loop
    over the single evaluation."""
    sp = _dense_spec([6, 6], lindblad=True, nessential=[3, 3], target="pure", objective="Jfrobenius", init="diagonal, 0")
    alphas = _alphas(sp, (0.1, 0.5), seed=5)
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    assert opt.ninit <= 16 and h.dim == 1296
    vals, grads = opt.evalGradF_batch(alphas)
    assert opt.last_batch_sets == 1
    assert h.last_kernel("forward").startswith("k_forward_big<"), h.last_kernel("forward")
    for j in range(2):
        assert _same_eval((vals[j], grads[j]), opt.evalGradF(alphas[j])), j
    assert not np.allclose(grads[0], grads[1], rtol=1e-3)
    opt.close(); h.close()


def test_handle_state_after_a_dense_batch():
    """6b. The batch leaves the handle's own control and G(t) tables alone: the next single evaluation returns what it returned
    before, and no trajectory is stored."""
    sp = _dense_spec([2, 2], lindblad=True)
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
    assert opt.last_batch_sets == 2
    assert opt.evalF(sp.params0) == before
    opt.close(); h.close()
