"""Risk-neutral objective: qd_optim_evalF_ensemble / qd_optim_evalGradF_ensemble evaluate ONE control vector on several system
Hamiltonians in shared sweep launches (the variants are the sets of a parameter-set batch on the dense kernels; k_gmat builds set j's
table of G(t) from the variant's own G0 = -i Hsys) and form the weighted mean of objectives and gradients (k_ensemble_mean).

Conventions of tests/test_gpu_param_batch_dense.py: at most 12 time steps of 0.004 ns and 16 initial conditions, linsolve = neumann unless
stated, every variant held against the CPU oracle on a spec whose hamiltonian is (hsys_j, hc) through helpers.check_parity.  The variants
are random Hermitian matrices from different seeds, scaled SCALE x (1, 2, 3, ...); before any GPU assertion the oracle's own gradients
of variants 0 and 1 are checked to differ (rtol 1e-3): a variant that read its neighbour's G0 cannot pass.
"""
from fractions import Fraction

import numpy as np
import pytest

from helpers import GMRES_MODES, OBJ_KEYS, check_parity, synthetic_spec, with_gmres_mode
from oracle.oracle import Oracle
from quandary_amd import capi
from quandary_amd.models import standard_hamiltonians

pytestmark = pytest.mark.gpu

# Hsys of variant j = SCALE x (j + 1) x 0.3 (A + A^H), A complex standard normal: chosen on the CPU so that the oracle's gradients of
# variants 0 and 1 differ at rtol 1e-3 over 12 steps of 0.004 ns on every system below
SCALE = 1.0
EPS = np.finfo(float).eps


def _hermitian(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    return 0.3 * (a + a.conj().T)


def _variants(n, nvar, seed=500, same=()):
    """nvar system Hamiltonians, variant j from seed + j and SCALE x (j + 1) strong; same = pairs (j, i): variant j is a copy of i."""
    hs = [SCALE * (j + 1) * _hermitian(n, seed + j) for j in range(nvar)]
    for j, i in same:
        hs[j] = hs[i].copy()
    return hs


def _dense_spec(nlevels, options=None, **kw):
    """The handle's own system: Hsys and Hc_k from seed 11 (no variant is built from it)."""
    sp = synthetic_spec(nlevels, **{"ntime": 12, "dt": 0.004, "linsolve": "neumann", **kw})
    assert sp.time.ntime <= 12 and sp.time.dt == 0.004
    n = int(np.prod(nlevels))
    sp.hamiltonian = (_hermitian(n, 11), np.array([0.5 / 0.3 * _hermitian(n, 12 + k) for k in range(len(nlevels))]))
    if options:
        sp.options = dict(options)
    return sp


def _alpha(sp, amp=0.3, seed=31):
    return amp * np.random.default_rng(seed).uniform(-1.0, 1.0, sp.params0.size)


def _with_hsys(sp, hsys):
    """sp as it describes variant hsys (the spec is shared: use the result before the next call)."""
    sp.hamiltonian = (hsys, sp.hamiltonian[1])
    return sp


def _oracle(sp, alpha, variants):
    """The oracle's evaluation of every variant; the first two must differ, or the test could not tell the variants' tables apart."""
    own = sp.hamiltonian
    out = []
    for hs in variants:
        orc = Oracle(_with_hsys(sp, hs))
        out.append(orc.evalGradF(alpha))
        orc.close()
    sp.hamiltonian = own
    assert not np.allclose(out[0][1], out[1][1], rtol=1e-3), "the oracle's gradients of variants 0 and 1 do not differ"
    return out


def _parity(sp, alpha, variants, vals, grads, ref, **kw):
    own = sp.hamiltonian
    for j, hs in enumerate(variants):
        print(j, vals[j]["objective"], ref[j][0]["objective"], np.linalg.norm(grads[j] - ref[j][1]) / np.linalg.norm(ref[j][1]))
        check_parity(_with_hsys(sp, hs), vals[j], grads[j], *ref[j], alpha=alpha, msg=j, **kw)
    sp.hamiltonian = own


def _variant(h):
    return int(h.last_kernel("forward").split(",")[2])


def _kernels(h):
    return h.last_kernel("forward"), h.last_kernel("adjoint")


def _set_kernels(h, q, lind, var):
    """Both sweeps ran on the SETS instantiation k_*<Q, LIND, VAR, QUBIT, GM, PLAIN, true>."""
    head = f"<{q}, {'true' if lind else 'false'}, {var}, "
    f, a = _kernels(h)
    return all(k.startswith(b + head) and k.endswith(", true>") and k.count(",") == 6 for k, b in ((f, "k_forward"), (a, "k_adjoint")))


def _same_eval(a, b):
    (va, ga), (vb, gb) = a, b
    return all(va[k] == vb[k] for k in OBJ_KEYS) and np.array_equal(ga, gb)


def _fma_chain(w, g):
    """sum_j w[j] g[j] as k_ensemble_mean forms it: one correctly rounded fma per variant, in variant order (exact rational arithmetic,
    rounded once per step)."""
    acc = np.zeros(g.shape[1])
    for wj, gj in zip(w, g):
        acc = np.array([float(Fraction(float(wj)) * Fraction(float(x)) + Fraction(float(a))) for x, a in zip(gj, acc)])
    return acc


def _check_mean(w, vals, grads, mean, grad_mean):
    """Every field of the mean and every component of grad_mean against numpy's weighted sum, within the rounding of len(w) fmas."""
    w = np.asarray(w, dtype=float)
    for k in OBJ_KEYS:
        v = np.array([val[k] for val in vals])
        assert abs(mean[k] - np.dot(w, v)) <= 4 * EPS * np.sum(np.abs(w * v)), k
    if grad_mean is not None:
        bound = 4 * EPS * np.sum(np.abs(w[:, None] * grads), axis=0)
        assert np.all(np.abs(grad_mean - w @ grads) <= bound)


# ---- the 2x2 Lindblad system of tests 1, 3, 4 and 5: built once, the oracle asked once ------------------------------------------------
@pytest.fixture(scope="module")
def l22():
    sp = _dense_spec([2, 2], lindblad=True)
    alpha = _alpha(sp)
    variants = _variants(4, 5, same=((2, 0),))
    return sp, alpha, variants, _oracle(sp, alpha, variants)


def test_ensemble_is_identical_to_single_evaluations_on_fresh_handles(l22):
    """1. Three variants in one launch, variant 2 a copy of variant 0: values and gradients are bit for bit those of evalGradF on three
    fresh handles whose set_hamiltonian received hsys[j]; every variant agrees with the oracle; the handle's own evaluation after the
    call is the one before it."""
    sp, alpha, variants, ref = l22
    variants, ref = variants[:3], ref[:3]
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    assert opt.ninit == 16
    before = opt.evalGradF(alpha)
    mean, grad_mean, vals, grads = opt.evalGradF_ensemble(alpha, variants)
    assert opt.last_batch_sets == 3
    assert _set_kernels(h, 2, True, 11), _kernels(h)
    assert grads.shape == (3, h.ndesign) and grad_mean.shape == (h.ndesign,)
    after = opt.evalGradF(alpha)
    assert _same_eval(before, after)
    own = sp.hamiltonian
    for j, hs in enumerate(variants):
        hj = capi.Handle(_with_hsys(sp, hs))
        oj = capi.Optim(hj, sp)
        single = oj.evalGradF(alpha)
        print(j, vals[j]["objective"], single[0]["objective"], np.linalg.norm(grads[j] - single[1]))
        assert _same_eval((vals[j], grads[j]), single), j
        oj.close(); hj.close()
    sp.hamiltonian = own
    assert _same_eval((vals[0], grads[0]), (vals[2], grads[2]))
    assert not np.allclose(grads[0], grads[1], rtol=1e-3)
    assert not np.allclose(grads[0], before[1], rtol=1e-3)  # (and no variant is the handle's own system)
    _parity(sp, alpha, variants, vals, grads, ref)
    _check_mean(np.full(3, 1.0 / 3.0), vals, grads, mean, grad_mean)
    opt.close(); h.close()


@pytest.mark.parametrize("kw,var,options", [
    pytest.param(dict(nlevels=[3, 4], lindblad=True, nessential=[2, 3], target="pure", objective="Jfrobenius", init="diagonal"), 12, None, id="2a-3x4-lindblad-guard-v12"),
    pytest.param(dict(nlevels=[4, 6], lindblad=True, target="pure", objective="Jmeasure", init="diagonal, 0"), 17, None, id="2b-4x6-lindblad-v17"),
    pytest.param(dict(nlevels=[4, 6], lindblad=True, target="pure", objective="Jmeasure", init="diagonal, 0"), 13, {"no_mfma": "1"}, id="2b-4x6-lindblad-no_mfma-v13"),
    pytest.param(dict(nlevels=[10, 12], lindblad=False, target="pure", objective="Jmeasure", init="pure, 1, 2"), None, None, id="2c-120-schroedinger-L2"),
    pytest.param(dict(nlevels=[4, 4], lindblad=True, nessential=[3, 3], target="pure", objective="Jfrobenius", init="diagonal, 0"), 15, None, id="2d-4x4-lindblad-v15"),
    pytest.param(dict(nlevels=[3, 3, 3], lindblad=True, nessential=[2, 3, 2], target="pure", objective="Jfrobenius", init="diagonal, 1"), 17, None, id="2e-3x3x3-lindblad-v17"),
])
def test_every_dense_variant(kw, var, options):
    """2. Two variants on every dense kernel variant the batch test covers, penalties on: G(t) staged in LDS (N <= 64) and read through
    L2 (N = 120), the vector kernels and both matrix-core kernels."""
    sp = _dense_spec(options=options, penalties=True, **kw)
    alpha = _alpha(sp)
    n = int(np.prod(kw["nlevels"]))
    variants = _variants(n, 2)
    ref = _oracle(sp, alpha, variants)
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    assert opt.ninit <= 16
    mean, grad_mean, vals, grads = opt.evalGradF_ensemble(alpha, variants)
    print(_kernels(h))
    assert opt.last_batch_sets == 2, _kernels(h)
    ran = _variant(h)
    if var is None:
        assert ran in (11, 12, 13) and n > 64 and not kw["lindblad"], _kernels(h)  # (N = 120: the table is too large for LDS)
    else:
        assert ran == var, _kernels(h)
    assert _set_kernels(h, len(kw["nlevels"]), kw["lindblad"], ran), _kernels(h)
    _parity(sp, alpha, variants, vals, grads, ref)
    _check_mean((0.5, 0.5), vals, grads, mean, grad_mean)
    opt.close(); h.close()


def test_mean_and_weights(l22):
    """3. Four variants, weights (0.1, 0.2, 0.3, 0.4) used as given; weights = None is 1 / nvar each; without per-variant output the
    mean and grad_mean are the same bits."""
    sp, alpha, variants, ref = l22
    variants = variants[:4]
    w = np.array([0.1, 0.2, 0.3, 0.4])
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    mean, grad_mean, vals, grads = opt.evalGradF_ensemble(alpha, variants, weights=w)
    assert opt.last_batch_sets == 4
    _check_mean(w, vals, grads, mean, grad_mean)
    print(np.abs(grad_mean - _fma_chain(w, grads)).max())
    assert np.array_equal(grad_mean, _fma_chain(w, grads))  # (the regularisation terms went into every variant before the weighting)
    mean2, grad_mean2, vals2, grads2 = opt.evalGradF_ensemble(alpha, variants, weights=2.0 * w)  # (not normalised)
    _check_mean(2.0 * w, vals2, grads2, mean2, grad_mean2)
    assert mean2["objective"] == pytest.approx(2.0 * mean["objective"], rel=1e-14)
    mean_n, grad_mean_n, vals_n, grads_n = opt.evalGradF_ensemble(alpha, variants)
    mean_q, grad_mean_q, _, _ = opt.evalGradF_ensemble(alpha, variants, weights=np.full(4, 0.25))
    assert mean_n == mean_q and np.array_equal(grad_mean_n, grad_mean_q)
    _check_mean(np.full(4, 0.25), vals_n, grads_n, mean_n, grad_mean_n)
    mean_o, grad_mean_o, vals_o, none = opt.evalGradF_ensemble(alpha, variants, weights=w, per_variant=False)
    assert none is None and vals_o == vals
    assert mean_o == mean and np.array_equal(grad_mean_o, grad_mean)
    opt.close(); h.close()


def test_forward_only_call(l22):
    """4. evalF_ensemble: the values of the gradient call, bit for bit."""
    sp, alpha, variants, ref = l22
    variants = variants[:3]
    w = np.array([0.5, 0.25, 0.25])
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    mean, _, vals, _ = opt.evalGradF_ensemble(alpha, variants, weights=w)
    fmean, fvals = opt.evalF_ensemble(alpha, variants, weights=w)
    assert opt.last_batch_sets == 3
    assert fvals == vals and fmean == mean
    for j in range(3):
        check_parity(sp, fvals[j], None, ref[j][0], None, alpha=alpha, msg=j)
    opt.close(); h.close()


def test_variants_that_do_not_fit_together_go_in_groups(l22):
    """5. Five variants under a trajectory budget that holds three variants' states, stages and G(t) tables, not four: launches of three
    and two variants, the numbers of the ungrouped call - grad_mean accumulated across the groups included."""
    sp, alpha, variants, ref = l22
    w = np.array([0.3, 0.1, 0.2, 0.15, 0.25])
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    mean, grad_mean, vals, grads = opt.evalGradF_ensemble(alpha, variants, weights=w)
    assert opt.last_batch_sets == 5
    n = 4  # rows of the density matrix = rows of G
    traj = (2 * sp.time.ntime + 1) * opt.ninit * 2 * h.dim * 8  # states x_0..x_n and primal stages of one variant, in bytes
    gtab = sp.time.ntime * n * n * 16                            # one row of G(t) per step of the implicit midpoint rule
    h.set_option("traj_budget_mb", 3.5 * (traj + gtab) / 1048576.0)
    mean_g, grad_mean_g, vals_g, grads_g = opt.evalGradF_ensemble(alpha, variants, weights=w)
    assert opt.last_batch_sets == 3 and _set_kernels(h, 2, True, 11), _kernels(h)
    assert vals_g == vals and np.array_equal(grads_g, grads)
    assert mean_g == mean and np.array_equal(grad_mean_g, grad_mean)
    mean_o, grad_mean_o, _, _ = opt.evalGradF_ensemble(alpha, variants, weights=w, per_variant=False)
    assert opt.last_batch_sets == 3
    assert mean_o == mean and np.array_equal(grad_mean_o, grad_mean)
    assert np.array_equal(grad_mean, _fma_chain(w, grads))
    _parity(sp, alpha, variants, vals_g, grads_g, ref)
    opt.close(); h.close()


@pytest.mark.parametrize("mode", GMRES_MODES)
def test_gmres_request(mode):
    """6. The 2x2 Lindblad system under a gmres request, in both modes of helpers.with_gmres_mode (the shipped default and the Krylov
    kernels): two variants in one launch."""
    sp = with_gmres_mode(_dense_spec([2, 2], lindblad=True, linsolve="gmres"), mode)
    alpha = _alpha(sp)
    variants = _variants(4, 2)
    ref = _oracle(sp, alpha, variants)
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    mean, grad_mean, vals, grads = opt.evalGradF_ensemble(alpha, variants)
    print(_kernels(h), h.last_solver)
    assert opt.last_batch_sets == 2 and _set_kernels(h, 2, True, 11), _kernels(h)
    if mode == "0":
        assert h.last_solver == "krylov", h.last_solver
    _parity(sp, alpha, variants, vals, grads, ref, any_solver=True)
    _check_mean((0.5, 0.5), vals, grads, mean, grad_mean)
    opt.close(); h.close()


def test_global_memory_kernels_go_variant_by_variant(monkeypatch):
    """7. The 2x2 Lindblad system forced onto the global-memory kernels, which have no set axis: the call is a loop over the single
    evaluation with the handle pointed at one variant after the other."""
    monkeypatch.setenv("QD_VAR", "16")
    sp = _dense_spec([2, 2], lindblad=True, penalties=True)
    alpha = _alpha(sp)
    variants = _variants(4, 3)
    ref = _oracle(sp, alpha, variants)
    w = np.array([0.2, 0.5, 0.3])
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    before = opt.evalGradF(alpha)
    mean, grad_mean, vals, grads = opt.evalGradF_ensemble(alpha, variants, weights=w)
    assert opt.last_batch_sets == 1
    assert h.last_kernel("forward").startswith("k_forward_big<"), h.last_kernel("forward")
    _parity(sp, alpha, variants, vals, grads, ref)
    _check_mean(w, vals, grads, mean, grad_mean)
    assert np.array_equal(grad_mean, _fma_chain(w, grads))
    mean_o, grad_mean_o, vals_o, none = opt.evalGradF_ensemble(alpha, variants, weights=w, per_variant=False)
    assert none is None and vals_o == vals and mean_o == mean and np.array_equal(grad_mean_o, grad_mean)
    fmean, fvals = opt.evalF_ensemble(alpha, variants, weights=w)
    assert opt.last_batch_sets == 1 and fvals == vals and fmean == mean
    assert _same_eval(before, opt.evalGradF(alpha))
    opt.close(); h.close()


# transition frequencies of oscillator 0 in test 8, GHz: samples 4 MHz apart around the nominal 4.1
TRANSFREQ0 = (4.096, 4.100, 4.104)


def test_standard_model_through_the_helper():
    """8. Robust control end to end: a 3x3 Lindblad standard-model spec, three samples of the first transition frequency a few MHz
    apart, each written as a dense Hsys by models.standard_hamiltonians.  Variant j agrees with the stencil oracle of the spec with
    that transfreq."""
    kw = dict(nlevels=[3, 3], lindblad=True, nessential=[2, 2], detuned=True, ntime=12, dt=0.004, linsolve="neumann", target="gate",
              objective="Jtrace", init="basis", penalties=True)
    sp = synthetic_spec(**kw)
    alpha = _alpha(sp)
    hsys0, hc = standard_hamiltonians(sp)
    variants, ref = [], []
    for f in TRANSFREQ0:
        spj = synthetic_spec(**kw)
        spj.system.transfreq[0] = f
        variants.append(standard_hamiltonians(spj)[0])
        orc = Oracle(spj)  # (the standard model itself: the stencil)
        ref.append((spj, orc.evalGradF(alpha)))
        orc.close()
    # (a gate on basis states sees the phases: 4 MHz over 0.048 ns move single gradient components by more than 1e-3 of their size and
    #  the whole gradient by 3e-4 of its norm, against 1e-8 in check_parity; populations alone - a pure target from diagonal states - do not)
    assert not np.allclose(ref[0][1][1], ref[1][1][1], rtol=1e-3), "the oracle's gradients of variants 0 and 1 do not differ"
    sp.hamiltonian = (hsys0, hc)
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    assert opt.ninit == 16
    mean, grad_mean, vals, grads = opt.evalGradF_ensemble(alpha, variants)
    assert opt.last_batch_sets == 3, _kernels(h)
    assert not np.allclose(grads[0], grads[1], rtol=1e-3)
    for j, (spj, (oval, ograd)) in enumerate(ref):
        print(j, vals[j]["objective"], oval["objective"], np.linalg.norm(grads[j] - ograd) / np.linalg.norm(ograd))
        check_parity(spj, vals[j], grads[j], oval, ograd, alpha=alpha, msg=j)
    _check_mean(np.full(3, 1.0 / 3.0), vals, grads, mean, grad_mean)
    opt.close(); h.close()


def test_errors_leave_the_handle_usable():
    """9. A handle without set_hamiltonian: QD_ERR_STATE; nvar = 0 and a negative weight: QD_ERR_INVALID; the handle evaluates
    normally after each."""
    sp = synthetic_spec([2, 2], lindblad=True, ntime=12, dt=0.004, linsolve="neumann")
    alpha = _alpha(sp)
    variants = _variants(4, 2)
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    before = opt.evalGradF(alpha)
    with pytest.raises(capi.QuandaryAmdError, match=r"rc=-5"):  # QD_ERR_STATE: the standard model has no Hc_k to keep
        opt.evalGradF_ensemble(alpha, variants)
    with pytest.raises(capi.QuandaryAmdError, match=r"rc=-5"):
        opt.evalF_ensemble(alpha, variants)
    assert _same_eval(before, opt.evalGradF(alpha))
    opt.close(); h.close()
    sp = _dense_spec([2, 2], lindblad=True)
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    before = opt.evalGradF(alpha)
    with pytest.raises(capi.QuandaryAmdError, match=r"rc=-1"):  # QD_ERR_INVALID
        opt.evalGradF_ensemble(alpha, [])
    assert _same_eval(before, opt.evalGradF(alpha))
    for bad in ([0.5, -0.5], [0.5, np.nan], [np.inf, 0.5]):
        with pytest.raises(capi.QuandaryAmdError, match=r"rc=-1"):
            opt.evalGradF_ensemble(alpha, variants, weights=bad)
        with pytest.raises(capi.QuandaryAmdError, match=r"rc=-1"):
            opt.evalF_ensemble(alpha, variants, weights=bad)
        assert _same_eval(before, opt.evalGradF(alpha))
    opt.close(); h.close()
