"""Ket classes of the lean column forward pass (qd_col.h, ColLean::apply<false, true, KC> / ColTeam::passes): where every column of a
wave shares the level i'_0 of oscillator 0 (USLOT) the diagonal-split forward kernel runs one form of its pass per wave - bottom level
(no ket-down neighbour of oscillator 0), interior, top level (no ket-up neighbour, no T1 term) - with the waves permuted so that
neighbouring waves differ in class.  Shapes: n_0 = 3 (one wave set of each class, the headline's shape), n_0 = 2 (bottom and top only),
n_0 = 4 with N = 60 (two interior levels), N = 45 (nine waves), and 4 x 12 with guard levels, whose stride of oscillator 0 is no multiple
of the five columns of a wave: no USLOT, the class forms must not be selected."""
import numpy as np
import pytest

from helpers import REF_RTOL, col_kernels, synthetic_spec
from oracle.oracle import Oracle
from quandary_amd import capi

OBJ_KEYS = ["objective", "fidelity", "cost", "regul", "penalty", "penalty_dpdm", "penalty_energy", "penalty_variation"]

KET_SHAPES = [
    pytest.param(dict(nlevels=[3, 20], lindblad=True, target="pure", objective="Jmeasure", init="diagonal, 0"), True, id="3x20"),
    pytest.param(dict(nlevels=[2, 20], lindblad=True, nessential=[2, 18], target="pure", objective="Jtrace", init="diagonal, 1"), True, id="2x20"),
    pytest.param(dict(nlevels=[4, 15], lindblad=True, nessential=[3, 14], target="pure", objective="Jfrobenius", init="diagonal, 0"), True, id="4x15"),
    pytest.param(dict(nlevels=[3, 15], lindblad=True, detuned=True, target="pure", objective="Jmeasure", init="diagonal, 1"), True, id="3x15"),
    pytest.param(dict(nlevels=[4, 12], lindblad=True, nessential=[3, 10], target="pure", objective="Jfrobenius", init="diagonal, 1"), False, id="4x12-guard"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("linsolve", ["neumann", "gmres"])
@pytest.mark.parametrize("stepper", ["IMR", "IMR4"])
@pytest.mark.parametrize("kw,uslot", KET_SHAPES)
def test_forward_sweep_with_ket_class_passes(kw, uslot, stepper, linsolve):
    """Operator and transpose at 1e-13; objective parts (1e-7, the suite's 1e-12 floor for parts that vanish) and gradient (1e-8 of its
    norm) against the oracle with every Lindblad penalty, under a neumann request and a gmres request served by the diagonal-split
    iteration (one more tested pass), IMR and IMR4 (the step size changes inside a step); the kernel names are those of
    helpers.col_kernels; a batch cut into time slices gives bit-identical final states to the unsliced one; never more applications per
    step than the oracle's solver (+ 0.25, the rule of test_lean_column_kernels for the diagonal-split iteration).
    The gmres cases ask for the column variant (option var = 9): below N = 44 a gmres request is otherwise planned on the
    eight-elements-per-thread variant (pick_config), where no diagonal-split stand-in exists and 2 x 20 under IMR4 runs GMRES on the
    general kernel.  The stand-in's own gate (gmres_split = auto) is left to decide, and must accept."""
    sp = synthetic_spec(**{**kw, "ntime": 12, "penalties": True, "stepper": stepper, "dt": 0.001, "linsolve": linsolve})
    sp.options = {"gmres_split": "auto", "var": "9"} if linsolve == "gmres" else {"neumann_split": "auto"}
    h, orc = capi.Handle(sp), Oracle(sp)
    rng = np.random.default_rng(29)
    h.set_params(sp.params0)
    orc.set_params(sp.params0)
    x = rng.standard_normal((3, 2 * h.dim))
    t = 0.37 * sp.time.ntime * sp.time.dt
    kernels = col_kernels(kw["nlevels"], "auto", stepper)
    fields = kernels["forward"][len("k_forward_col<"):-1].split(", ")
    assert (fields[2], fields[3], fields[5]) == ("true", "true" if uslot else "false", "false")  # (SPLIT, USLOT, KRY)
    for tr in (False, True):
        yo = orc.apply_rhs(t, x, transpose=tr)
        np.testing.assert_allclose(h.apply_rhs(t, x, transpose=tr), yo, rtol=1e-13, atol=1e-13 * np.abs(yo).max())
        assert h.last_kernel("apply") == kernels["apply"]
    opt = capi.Optim(h, sp)
    val, g = opt.evalGradF(sp.params0)
    assert (h.last_kernel("forward"), h.last_kernel("adjoint")) == (kernels["forward"], kernels["adjoint"])
    assert h.last_solver == ("gmres_as_split" if linsolve == "gmres" else "neumann")
    oval, og = orc.evalGradF(sp.params0)
    for k in OBJ_KEYS:
        print(k, val[k], oval[k])
        assert val[k] == pytest.approx(oval[k], rel=REF_RTOL, abs=1e-12), k
    gerr = np.linalg.norm(g - og) / np.linalg.norm(og)
    print("gradient", gerr)
    assert gerr < 1e-8
    orc.reset_stats()
    orc.evalF(sp.params0)
    opt.evalF(sp.params0)
    print("applications per step", h.mean_applies, orc.mean_applies)
    assert h.mean_applies < orc.mean_applies + 0.25
    # time-sliced batch against the unsliced one
    x0 = rng.standard_normal((5, 2 * h.dim))
    h.set_option("col_slices", 1)
    ref = h.forward(x0)
    assert h.last_kernel("forward") == kernels["forward"]
    h.set_option("col_slices", 3)
    res = h.forward(x0)
    assert h.last_kernel("forward") == kernels["forward"]
    np.testing.assert_array_equal(res["final_states"], ref["final_states"])
    opt.close(); h.close(); orc.close()
