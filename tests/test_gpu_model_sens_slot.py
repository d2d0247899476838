"""Model-constant sensitivities on the lean slot kernels (qd_optim_evalGradF_model under option sens_slot = 1): the adjoint sweep on
k_adjoint_q32_sens, the forward sweep on the plain k_forward_q32 of the same instantiation <Q, SB, double, false, HJ>.

Reference and tolerance are those of tests/test_gpu_model_sens.py: a Richardson-extrapolated central difference of the oracle's
objective with its own error estimate e_ref (tests/test_model_sens_cpu.py, tests/test_model_sens_slot_cpu.py: capped at 1e-6 of the norm
of the case's sensitivity vector); every entry must lie within max(1e-8 ||ref||, 4 e_ref) of it - 1e-8 is the gradient tolerance of
helpers.check_parity, the factor 4 covers that e_ref estimates the reference's error and does not bound it.  The lean form and the
general one (sens_slot = 0, k_adjoint_sens) each sit within that of the reference, hence within twice that of each other.

The cases are 2^4 and 2^5 Lindblad systems (dim 256 and 1024), three states, 20 steps, and reach the five instantiations the launcher
can pick: <4, 0>, <5, 1> and <5, 2> (the uncoupled 2^5 case once under lean64_sb = 1 and once under 2), <4, 0, ..., HJ> and
<5, 1, ..., HJ>.  Index order: every system has constants of its own per oscillator and pair (helpers.unequal_constants, asserted on the
CPU), so the entries of the reference all differ and a kernel that decoded the level bits in another oscillator order, or numbered the
pairs differently from qd_sens.h, would return a permutation of them and fail the parity test - no separate test is needed for it.
Penalties are on throughout."""
import re

import numpy as np
import pytest

from helpers import OBJ_KEYS, unequal_constants
from quandary_amd import capi
from test_ensemble_model_cpu import model_spec
from test_model_sens_cpu import ARRAYS, is_exact_zero, ref_norm, reference, sens_spec
from test_model_sens_slot_cpu import slot_reference, slot_spec

pytestmark = pytest.mark.gpu

SLOT = {"sens_slot": "1"}
# id -> (case of test_model_sens_cpu (False) or test_model_sens_slot_cpu (True), its name, options beside sens_slot, "Q, SB", HJ)
CASES = {
    "2x2x2x2-lindblad": (False, "2x2x2x2-lindblad", {}, "4, 0", "false"),
    "2x2x2x2x2-sb1": (True, "2x2x2x2x2", {"lean64_sb": "1"}, "5, 1", "false"),
    "2x2x2x2x2-sb2": (True, "2x2x2x2x2", {"lean64_sb": "2"}, "5, 2", "false"),
    "2x2x2x2-coupled": (True, "2x2x2x2-coupled", {}, "4, 0", "true"),
    "2x2x2x2x2-coupled": (True, "2x2x2x2x2-coupled", {}, "5, 1", "true"),
    "2x2x2x2-gmres": (True, "2x2x2x2-gmres", {}, "4, 0", "false"),
    "2x2x2x2-imr4": (True, "2x2x2x2-imr4", {}, "4, 0", "false"),
}
# under sens_slot = 1, plans the form cannot serve: the general family, as without the option
FALLBACKS = {
    "2x2x2x2-gmres_split-0": (True, "2x2x2x2-gmres", {"gmres_split": "0"}),
    "3x20-lindblad": (False, "3x20-lindblad", {}),
}


def _spec(slot, name, options):
    return slot_spec(name, options=options) if slot else sens_spec(name, options=options)


def _ref(slot, name):
    """{array: (R, e_ref)}"""
    ref = slot_reference(name) if slot else reference(name)
    return {a: (ref[a][0], ref[a][1]) for a in ARRAYS}


def _same_eval(a, b):
    (va, ga), (vb, gb) = a, b
    return all(va[k] == vb[k] for k in OBJ_KEYS) and np.array_equal(ga, gb)


def _kernels(h):
    return h.last_kernel("forward"), h.last_kernel("adjoint")


def _run(sp):
    """On one handle: evalGradF, evalGradF_model, evalGradF, evalGradF_model - results and the kernels of each."""
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
    """Every case with sens_slot = 1 and with sens_slot = 0, every fallback with sens_slot = 1, and the two families side by side under
    both options: once, in this process."""
    out = {}
    for cid, (slot, name, options, _, _) in CASES.items():
        out[cid, 1] = _run(_spec(slot, name, {**SLOT, **options}))
        out[cid, 0] = _run(_spec(slot, name, {"sens_slot": "0", **options}))
    for cid, (slot, name, options) in FALLBACKS.items():
        out[cid, 1] = _run(_spec(slot, name, {**SLOT, **options}))
    both = {**SLOT, "sens_lean": "1"}
    out["both", "col"] = _run(sens_spec("3x20-lindblad", options=both))
    out["both", "slot"] = _run(sens_spec("2x2x2x2-lindblad", options=both))
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
def test_sensitivities_match_the_reference_on_the_lean_slot_kernels(runs, cid):
    """Tolerance and kernels: k_adjoint_q32_sens behind the plain k_forward_q32 of the same instantiation; every selfkerr entry == 0.0."""
    slot, name, _, qsb, hj = CASES[cid]
    r = runs[cid, 1]
    kf, ka = r["k_model"]
    print(f"{cid}: {kf} / {ka}")
    assert ka == f"k_adjoint_q32_sens<{qsb}, double, false, {hj}>", ka
    assert kf == f"k_forward_q32<{qsb}, double, false, {hj}>", kf
    sens = r["model"][2]
    assert len(sens["selfkerr"]) == r["sp"].system.nosc and all(v == 0.0 for v in sens["selfkerr"])
    _check_against_reference(cid, r["sp"], sens, _ref(slot, name))


@pytest.mark.parametrize("cid", list(CASES))
def test_value_gradient_and_instantiation_are_those_of_the_plain_call(runs, cid):
    """val and grad are bit for bit those of evalGradF on the same handle; the template arguments of the sensitivity kernel are those of
    that call's k_adjoint_q32, the forward kernel is the same one."""
    r = runs[cid, 1]
    assert _same_eval(r["model"][:2], r["first"])
    assert r["k_first"][1].startswith("k_adjoint_q32<"), r["k_first"]
    assert r["k_model"][0] == r["k_first"][0]
    assert r["k_model"][1] == r["k_first"][1].replace("k_adjoint_q32<", "k_adjoint_q32_sens<"), (r["k_model"], r["k_first"])


def test_all_five_instantiations_ran(runs):
    seen = {re.match(r"k_adjoint_q32_sens<([^>]*)>", runs[cid, 1]["k_model"][1]).group(1) for cid in CASES}
    print("instantiations:", sorted(seen))
    assert seen == {"4, 0, double, false, false", "5, 1, double, false, false", "5, 2, double, false, false", "4, 0, double, false, true",
                    "5, 1, double, false, true"}


@pytest.mark.parametrize("cid", list(CASES))
def test_the_general_form_agrees(runs, cid):
    """sens_slot = 0 runs the same case on k_adjoint_sens; the two results differ by at most twice the tolerance."""
    slot, name, _, _, _ = CASES[cid]
    g, l = runs[cid, 0], runs[cid, 1]
    assert g["k_model"][0].startswith("k_forward<") and g["k_model"][1].startswith("k_adjoint_sens<"), g["k_model"]
    ref = _ref(slot, name)
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


def _check_put_back(r):
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


@pytest.mark.parametrize("cid", list(CASES))
def test_the_handle_is_put_back(runs, cid):
    """evalGradF, evalGradF_model, evalGradF on one handle: the third equals the first bit for bit on the same kernels; a second
    evalGradF_model returns the bits of the first (no atomics anywhere in the sums); NULL output arrays are accepted."""
    _check_put_back(runs[cid, 1])


@pytest.mark.parametrize("cid", list(FALLBACKS))
def test_plans_without_a_slot_form_take_the_general_family(runs, cid):
    """The Krylov kernels of the lean slot family (gmres_split = 0) and a 3x20 system without sens_lean, under sens_slot = 1:
    k_adjoint_sens, the same tolerance, and the handle is put back."""
    slot, name, _ = FALLBACKS[cid]
    r = runs[cid, 1]
    assert r["k_model"][0].startswith("k_forward<") and r["k_model"][1].startswith("k_adjoint_sens<"), r["k_model"]
    assert not r["k_first"][1].startswith("k_adjoint<"), r["k_first"]  # (a lean family: the call left it and came back)
    assert r["k_first"] == r["k_third"]
    if r["k_first"][1].startswith("k_adjoint_q32<"):
        assert re.match(r"k_adjoint_q32<\d, \d, double, true, ", r["k_first"][1]), r["k_first"]  # (the Krylov kernel: why the form is not built)
        # (the degree tuner of its polynomial preconditioner moves between the first evaluations of a handle, with or without a
        #  sensitivity call in between - the same equations to the solver tolerance, not the same bits)
        for k in OBJ_KEYS:
            assert r["third"][0][k] == pytest.approx(r["first"][0][k], rel=1e-9, abs=1e-12), k
        assert np.linalg.norm(r["third"][1] - r["first"][1]) <= 1e-8 * np.linalg.norm(r["first"][1])
    else:
        assert _same_eval(r["first"], r["third"])
    _check_against_reference(cid, r["sp"], r["model"][2], _ref(slot, name))


def test_both_options_serve_both_families_in_one_process(runs):
    """sens_slot = 1 together with sens_lean = 1: the 3x20 system on k_adjoint_col_sens, the 2^4 system on k_adjoint_q32_sens."""
    c, s = runs["both", "col"], runs["both", "slot"]
    assert c["k_model"][0].startswith("k_forward_col<") and c["k_model"][1].startswith("k_adjoint_col_sens<"), c["k_model"]
    assert s["k_model"] == ("k_forward_q32<4, 0, double, false, false>", "k_adjoint_q32_sens<4, 0, double, false, false>"), s["k_model"]
    for r, name in ((c, "3x20-lindblad"), (s, "2x2x2x2-lindblad")):
        assert _same_eval(r["model"][:2], r["first"])
        _check_put_back(r)
        _check_against_reference("both " + name, r["sp"], r["model"][2], _ref(False, name))


def _refused(opt, h, sp, rc):
    with pytest.raises(capi.QuandaryAmdError, match=rf"rc={rc}"):
        opt.evalGradF_model(sp.params0)
    assert h.last_kernel("forward") == "" and h.last_kernel("adjoint") == ""  # no sweep was launched


def test_refusals_stay():
    """Two ranks: QD_ERR_STATE; explicit Euler and fp32-mixed precision: QD_ERR_UNSUPPORTED - under sens_slot = 1 as without it, and no
    sweep is launched for any of them."""
    sp = sens_spec("2x2-schroedinger", options=SLOT)  # (four initial conditions: two ranks divide them)
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp, rank=0, nranks=2)
    _refused(opt, h, sp, -5)
    opt.close(); h.close()
    ee = model_spec([2, 2, 2, 2], stepper="EE", options=SLOT, nessential=[2, 2, 2, 2], **unequal_constants(4, coupled=False))
    h = capi.Handle(ee)
    opt = capi.Optim(h, ee)
    _refused(opt, h, ee, -2)
    opt.close(); h.close()
    sp = sens_spec("2x2x2x2-lindblad", options=SLOT)  # (all qubits, every level essential: what fp32-mixed takes)
    h = capi.Handle(sp)
    h.set_precision("f32mixed")
    opt = capi.Optim(h, sp)
    _refused(opt, h, sp, -2)
    opt.close(); h.close()
