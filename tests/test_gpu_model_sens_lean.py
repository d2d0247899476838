"""Model-constant sensitivities on the lean column kernels (qd_optim_evalGradF_model under option sens_lean = 1): the adjoint sweep on
k_adjoint_col_sens / k_adjoint_colj_sens, the forward sweep on the plain k_forward_col / k_forward_colj.

Reference and tolerance are those of tests/test_gpu_model_sens.py: a Richardson-extrapolated central difference of the oracle's
objective with its own error estimate e_ref (tests/test_model_sens_cpu.py, tests/test_model_sens_lean_cpu.py: capped at 1e-6 of the norm
of the case's sensitivity vector); every entry must lie within max(1e-8 ||ref||, 4 e_ref) of it - 1e-8 is the gradient tolerance of
helpers.check_parity, the factor 4 covers that e_ref estimates the reference's error and does not bound it.  The lean form and the
general one (sens_lean = 0, k_adjoint_sens) each sit within that of the reference, hence within twice that of each other.

The cases are the smallest shapes that reach every instantiation <Q, EPT> of both units, both USLOT forms and both SKIP forms; every
system has constants of its own per oscillator and pair, penalties are on throughout."""
import re

import numpy as np
import pytest

from helpers import OBJ_KEYS, unequal_constants
from quandary_amd import capi
from test_ensemble_model_cpu import model_spec
from test_model_sens_cpu import ARRAYS, is_exact_zero, ref_norm, reference, sens_spec
from test_model_sens_lean_cpu import lean_reference, lean_spec

pytestmark = pytest.mark.gpu

LEAN = {"sens_lean": "1"}
# id -> (case of test_model_sens_cpu (False) or test_model_sens_lean_cpu (True), its name, options beside sens_lean, kernel unit, "Q, EPT")
CASES = {
    "3x20-lindblad": (False, "3x20-lindblad", {}, "col", "2, 5"),
    "8x8-guard": (True, "8x8-guard", {}, "col", "2, 8"),
    "3x3x5-lindblad": (False, "3x3x5-lindblad", {}, "col", "3, 5"),
    "4x4x4": (True, "4x4x4", {}, "col", "3, 8"),
    "3x20-coupled": (True, "3x20-coupled", {}, "colj", "2, 5"),
    "4x4x4-coupled": (True, "4x4x4-coupled", {}, "colj", "3, 8"),
    "3x20-imr4": (True, "3x20-imr4", {}, "col", "2, 5"),
    "3x20-col_skip-0": (False, "3x20-lindblad", {"col_skip": "0"}, "col", "2, 5"),
    "3x20-gmres": (True, "3x20-gmres", {}, "col", "2, 5"),
    "3x20-13steps-sliced": (True, "3x20-13steps", {"col_slices": "3"}, "col", "2, 5"),
    "3x20-13steps-unsliced": (True, "3x20-13steps", {"col_slices": "1"}, "col", "2, 5"),
}
# plans the units cannot serve: the general family, as without the option
FALLBACKS = {
    "3x20-gmres_split-0": (True, "3x20-gmres", {"gmres_split": "0"}),
    "3x20-neumann_split-0": (False, "3x20-lindblad", {"neumann_split": "0"}),
    "2x2x2x2-lindblad": (False, "2x2x2x2-lindblad", {}),
}


def _spec(lean, name, options):
    return lean_spec(name, options=options) if lean else sens_spec(name, options=options)


def _ref(lean, name):
    """{array: (R, e_ref)}"""
    ref = lean_reference(name) if lean else reference(name)
    return {a: (ref[a][0], ref[a][1]) for a in ARRAYS}


def _same_eval(a, b):
    (va, ga), (vb, gb) = a, b
    return all(va[k] == vb[k] for k in OBJ_KEYS) and np.array_equal(ga, gb)


def _kernels(h):
    return h.last_kernel("forward"), h.last_kernel("adjoint")


def _run(lean, name, options):
    """On one handle: evalGradF, evalGradF_model, evalGradF, evalGradF_model - results and the kernels of each."""
    sp = _spec(lean, name, options)
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    out = {"sp": sp}
    out["first"] = opt.evalGradF(sp.params0)
    out["k_first"] = _kernels(h)
    out["model"] = opt.evalGradF_model(sp.params0)
    out["k_model"] = _kernels(h)
    out["third"] = opt.evalGradF(sp.params0)
    out["k_third"] = _kernels(h)
    out["model2"] = opt.evalGradF_model(sp.params0)
    out["none"] = opt.evalGradF_model(sp.params0, want=())
    out["only"] = opt.evalGradF_model(sp.params0, want=("crosskerr",))
    out["last"] = opt.evalGradF(sp.params0)
    opt.close(); h.close()
    return out


@pytest.fixture(scope="module")
def runs():
    """Every case with sens_lean = 1 and with sens_lean = 0, every fallback with sens_lean = 1: once."""
    out = {}
    for cid, (lean, name, options, _, _) in CASES.items():
        out[cid, 1] = _run(lean, name, {**LEAN, **options})
        out[cid, 0] = _run(lean, name, {"sens_lean": "0", **options})
    for cid, (lean, name, options) in FALLBACKS.items():
        out[cid, 1] = _run(lean, name, {**LEAN, **options})
    return out


def _check_against_reference(label, sp, sens, ref):
    norm = ref_norm(ref)
    worst = 0.0
    for array in ARRAYS:
        R, E = ref[array]
        assert sens[array].shape == R.shape, array
        for i in range(len(R)):
            tol = max(1e-8 * norm, 4.0 * E[i])
            err = abs(sens[array][i] - R[i])
            worst = max(worst, err / tol)
            print(f"{label} {array}[{i}]: {sens[array][i]:+.9e} vs {R[i]:+.9e}, |diff| / norm = {err / norm:.1e}, tolerance / norm = {tol / norm:.1e}")
    print(f"{label}: worst |diff| / tolerance = {worst:.2e}")
    for array in ARRAYS:
        R, E = ref[array]
        for i in range(len(R)):
            assert abs(sens[array][i] - R[i]) <= max(1e-8 * norm, 4.0 * E[i]), (label, array, i)
            if is_exact_zero(sp, array, i):
                assert sens[array][i] == 0.0, (label, array, i)


@pytest.mark.parametrize("cid", list(CASES))
def test_sensitivities_match_the_reference_on_the_lean_kernels(runs, cid):
    """Tolerance and kernels: k_adjoint_col_sens / k_adjoint_colj_sens behind the plain forward kernel of the same unit."""
    lean, name, _, unit, qept = CASES[cid]
    r = runs[cid, 1]
    kf, ka = r["k_model"]
    print(f"{cid}: {kf} / {ka}")
    assert ka.startswith(f"k_adjoint_{unit}_sens<{qept}, true, ") and ka.endswith(", false>"), ka
    assert kf.startswith(f"k_forward_{unit}<{qept}, true, "), kf
    _check_against_reference(cid, r["sp"], r["model"][2], _ref(lean, name))


@pytest.mark.parametrize("cid", list(CASES))
def test_value_gradient_and_instantiation_are_those_of_the_plain_call(runs, cid):
    """val and grad are bit for bit those of evalGradF on the same handle; the template arguments of the sensitivity kernel are those of
    that call's k_adjoint_col / k_adjoint_colj, the forward kernel is the same one."""
    unit = CASES[cid][3]
    r = runs[cid, 1]
    assert _same_eval(r["model"][:2], r["first"])
    assert r["k_first"][1].startswith(f"k_adjoint_{unit}<"), r["k_first"]
    assert r["k_model"][0] == r["k_first"][0]
    assert r["k_model"][1] == r["k_first"][1].replace(f"k_adjoint_{unit}<", f"k_adjoint_{unit}_sens<"), (r["k_model"], r["k_first"])


def test_both_uslot_and_both_skip_forms_ran(runs):
    seen = set()
    for cid in CASES:
        ka = runs[cid, 1]["k_model"][1]
        args = [s.strip() for s in re.match(r"k_adjoint_colj?_sens<([^>]*)>", ka).group(1).split(",")]
        seen.add((args[3], args[4]))
        print(f"{cid}: USLOT = {args[3]}, SKIP = {args[4]}")
    print("instantiations (USLOT, SKIP):", sorted(seen))
    assert {u for u, _ in seen} == {"true", "false"}
    assert {s for _, s in seen} == {"true", "false"}


@pytest.mark.parametrize("cid", list(CASES))
def test_the_general_form_agrees(runs, cid):
    """sens_lean = 0 runs the same case on k_adjoint_sens; the two results differ by at most twice the tolerance."""
    lean, name, _, _, _ = CASES[cid]
    g, l = runs[cid, 0], runs[cid, 1]
    assert g["k_model"][0].startswith("k_forward<") and g["k_model"][1].startswith("k_adjoint_sens<"), g["k_model"]
    ref = _ref(lean, name)
    norm = ref_norm(ref)
    _check_against_reference(cid + " general", g["sp"], g["model"][2], ref)
    worst = 0.0
    for array in ARRAYS:
        E = ref[array][1]
        for i in range(len(E)):
            d = abs(g["model"][2][array][i] - l["model"][2][array][i])
            worst = max(worst, d / norm)
            print(f"{cid} {array}[{i}]: |lean - general| / norm = {d / norm:.1e}")
            assert d <= 2.0 * max(1e-8 * norm, 4.0 * E[i]), (array, i)
    print(f"{cid}: worst |lean - general| / norm = {worst:.1e}")


def test_sliced_and_unsliced_sweeps_agree_with_the_reference(runs):
    """Three time slices over 13 steps (5 + 4 + 4: the scheduler, the carry of the adjoint state, one row of sums per task) and the
    unsliced sweep: both within the tolerance (asserted per case above); the observed difference of the two."""
    s, u = runs["3x20-13steps-sliced", 1], runs["3x20-13steps-unsliced", 1]
    ref = _ref(True, "3x20-13steps")
    norm = ref_norm(ref)
    for r, label in ((s, "sliced"), (u, "unsliced")):
        _check_against_reference(label, r["sp"], r["model"][2], ref)
    for array in ARRAYS:
        for i in range(len(ref[array][0])):
            print(f"{array}[{i}]: |sliced - unsliced| / norm = {abs(s['model'][2][array][i] - u['model'][2][array][i]) / norm:.1e}")


@pytest.mark.parametrize("cid", list(CASES))
def test_the_handle_is_put_back(runs, cid):
    """evalGradF, evalGradF_model, evalGradF on one handle: the third equals the first bit for bit on the same kernels; a second
    evalGradF_model returns the bits of the first (no atomics anywhere in the sums); NULL output arrays are accepted."""
    r = runs[cid, 1]
    assert _same_eval(r["first"], r["third"]) and r["k_first"] == r["k_third"]
    assert _same_eval(r["first"], r["last"])
    val, grad, sens = r["model"]
    val2, grad2, sens2 = r["model2"]
    assert _same_eval((val, grad), (val2, grad2))
    assert all(np.array_equal(sens[a], sens2[a]) for a in ARRAYS)
    val3, grad3, none = r["none"]
    assert _same_eval((val, grad), (val3, grad3)) and all(none[a] is None for a in ARRAYS)
    only = r["only"][2]
    assert only["transfreq"] is None and only["selfkerr"] is None and np.array_equal(only["crosskerr"], sens["crosskerr"])


@pytest.mark.parametrize("cid", list(FALLBACKS))
def test_plans_without_a_lean_form_take_the_general_family(runs, cid):
    """The lean column Krylov kernels (gmres_split = 0), the plain Neumann form (neumann_split = 0) and a lean slot system under
    sens_lean = 1: k_adjoint_sens, the same tolerance, and the handle is put back."""
    lean, name, _ = FALLBACKS[cid]
    r = runs[cid, 1]
    assert r["k_model"][0].startswith("k_forward<") and r["k_model"][1].startswith("k_adjoint_sens<"), r["k_model"]
    assert not r["k_first"][1].startswith("k_adjoint<"), r["k_first"]  # (a lean family: the call left it and came back)
    assert r["k_first"] == r["k_third"]
    if r["k_first"][1].endswith(", true>"):
        # (the Krylov kernels: the degree tuner of their polynomial preconditioner moves between the first evaluations of a handle, with
        #  or without a sensitivity call in between - the same equations to the solver tolerance, not the same bits)
        for k in OBJ_KEYS:
            assert r["third"][0][k] == pytest.approx(r["first"][0][k], rel=1e-9, abs=1e-12), k
        assert np.linalg.norm(r["third"][1] - r["first"][1]) <= 1e-8 * np.linalg.norm(r["first"][1])
    else:
        assert _same_eval(r["first"], r["third"])
    _check_against_reference(cid, r["sp"], r["model"][2], _ref(lean, name))


def _refused(opt, h, sp, rc):
    with pytest.raises(capi.QuandaryAmdError, match=rf"rc={rc}"):
        opt.evalGradF_model(sp.params0)
    assert h.last_kernel("forward") == "" and h.last_kernel("adjoint") == ""  # no sweep was launched


def test_refusals_stay():
    """Two ranks: QD_ERR_STATE; explicit Euler and fp32-mixed precision: QD_ERR_UNSUPPORTED - under sens_lean = 1 as without it, and no
    sweep is launched for any of them."""
    sp = sens_spec("2x2-schroedinger", options=LEAN)  # (four initial conditions: two ranks divide them)
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp, rank=0, nranks=2)
    _refused(opt, h, sp, -5)
    opt.close(); h.close()
    ee = model_spec([3, 20], stepper="EE", options=LEAN, **unequal_constants(2, coupled=False))
    h = capi.Handle(ee)
    opt = capi.Optim(h, ee)
    _refused(opt, h, ee, -2)
    opt.close(); h.close()
    sp = sens_spec("2x2x2x2-lindblad", options=LEAN)  # (all qubits, every level essential: what fp32-mixed takes)
    h = capi.Handle(sp)
    h.set_precision("f32mixed")
    opt = capi.Optim(h, sp)
    _refused(opt, h, sp, -2)
    opt.close(); h.close()
