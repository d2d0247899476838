"""Model-constant sensitivities on the GPU (qd_optim_evalGradF_model): d objective / d (transfreq, selfkerr, crosskerr) from the
sensitivity form of the general adjoint sweep, k_adjoint_sens.

Reference and tolerance: tests/test_model_sens_cpu.py - a Richardson-extrapolated central difference of the oracle's objective with its
own error estimate e_ref, capped there at 1e-6 of the norm of the case's sensitivity vector.  Every entry must lie within
max(1e-8 ||ref||, 4 e_ref) of it: 1e-8 is the gradient tolerance of helpers.check_parity, the factor 4 covers that e_ref estimates the
reference's error and does not bound it.  Every system has constants of its own per oscillator and pair; penalties are on throughout."""
import numpy as np
import pytest

from helpers import OBJ_KEYS, unequal_constants, with_gmres_mode
from quandary_amd import capi
from test_ensemble_model_cpu import model_spec
from test_model_sens_cpu import ARRAYS, CASES, H, H_DEFAULT, is_exact_zero, n_of, ref_norm, reference, sens_spec

pytestmark = pytest.mark.gpu

GENERAL = {"no_collean": "1", "no_lean64": "1"}
# (case, gmres_split): one per stencil and axis that can go wrong, the steppers and the solvers of the 3 x 3 Lindblad system
PARITY = [(name, None) for name in CASES if name != "3x3-lindblad-gmres"] + [("3x3-lindblad-gmres", "auto"), ("3x3-lindblad-gmres", "0")]
# the kernel family a plain evalGradF of the case runs on where it is not the general one
LEAN = {"2x2x2x2-lindblad": "k_adjoint_q32<", "3x20-lindblad": "k_adjoint_col<"}


def _same_eval(a, b):
    (va, ga), (vb, gb) = a, b
    return all(va[k] == vb[k] for k in OBJ_KEYS) and np.array_equal(ga, gb)


def _open(name, mode=None, options=None):
    sp = with_gmres_mode(sens_spec(name, options=options), mode)
    h = capi.Handle(sp)
    return sp, h, capi.Optim(h, sp)


@pytest.fixture(scope="module")
def calls():
    """evalGradF_model of every parity case on a fresh handle, once: (val, grad, sens, forward kernel, adjoint kernel)."""
    out = {}
    for name, mode in PARITY:
        sp, h, opt = _open(name, mode)
        val, grad, sens = opt.evalGradF_model(sp.params0)
        out[name, mode] = (val, grad, sens, h.last_kernel("forward"), h.last_kernel("adjoint"))
        opt.close(); h.close()
    return out


@pytest.mark.parametrize("name,mode", PARITY)
def test_sensitivities_match_the_extrapolated_difference_of_the_oracle(calls, name, mode):
    sens = calls[name, mode][2]
    ref = reference(name)
    norm = ref_norm(ref)
    sp = sens_spec(name)
    worst = 0.0
    for array in ARRAYS:
        R, E, _ = ref[array]
        assert sens[array].shape == R.shape, array
        for i in range(len(R)):
            tol = max(1e-8 * norm, 4.0 * E[i])
            err = abs(sens[array][i] - R[i])
            worst = max(worst, err / tol)
            print(f"{name} {mode} {array}[{i}]: {sens[array][i]:+.9e} vs {R[i]:+.9e}, |diff| / norm = {err / norm:.1e}, tolerance / norm = {tol / norm:.1e}")
            if is_exact_zero(sp, array, i):
                assert sens[array][i] == 0.0, (array, i)
    print(f"{name} {mode}: worst |diff| / tolerance = {worst:.2e}")
    for array in ARRAYS:
        R, E, _ = ref[array]
        for i in range(len(R)):
            assert abs(sens[array][i] - R[i]) <= max(1e-8 * norm, 4.0 * E[i]), (array, i)


@pytest.mark.parametrize("name,mode", PARITY)
def test_value_gradient_and_kernels_are_those_of_the_general_family(calls, name, mode):
    """val and grad are bit for bit those of evalGradF on a second handle with no_collean = 1, no_lean64 = 1; the adjoint sweep ran on
    k_adjoint_sens with the template arguments of that handle's k_adjoint, the forward sweep on the same k_forward."""
    val, grad, _, kf, ka = calls[name, mode]
    sp, h, opt = _open(name, mode, options=GENERAL)
    plain = opt.evalGradF(sp.params0)
    gf, ga = h.last_kernel("forward"), h.last_kernel("adjoint")
    opt.close(); h.close()
    assert _same_eval((val, grad), plain)
    assert gf.startswith("k_forward<") and ga.startswith("k_adjoint<"), (gf, ga)
    assert kf == gf
    assert ka.startswith("k_adjoint_sens<") and ka == ga.replace("k_adjoint<", "k_adjoint_sens<"), (ka, ga)


@pytest.mark.parametrize("name", ["3x3-lindblad", "2x2x2x2-lindblad", "3x20-lindblad", "3x3-schroedinger"])
def test_the_handle_is_put_back(calls, name):
    """evalGradF, evalGradF_model, evalGradF on one handle: the third equals the first bit for bit, on the kernels of the first (the lean
    ones where the system has them); a second evalGradF_model returns the bits of the first; NULL output arrays are accepted."""
    sp, h, opt = _open(name)
    first = opt.evalGradF(sp.params0)
    k0 = (h.last_kernel("forward"), h.last_kernel("adjoint"))
    assert k0[1].startswith(LEAN.get(name, "k_adjoint<")), k0
    val, grad, sens = opt.evalGradF_model(sp.params0)
    assert h.last_kernel("adjoint").startswith("k_adjoint_sens<")
    third = opt.evalGradF(sp.params0)
    assert (h.last_kernel("forward"), h.last_kernel("adjoint")) == k0
    assert _same_eval(first, third)
    val2, grad2, sens2 = opt.evalGradF_model(sp.params0)
    assert _same_eval((val, grad), (val2, grad2))
    assert all(np.array_equal(sens[a], sens2[a]) for a in ARRAYS)
    assert _same_eval((val, grad), calls[name, None][:2]) and all(np.array_equal(sens[a], calls[name, None][2][a]) for a in ARRAYS)
    val3, grad3, none = opt.evalGradF_model(sp.params0, want=())
    assert _same_eval((val, grad), (val3, grad3)) and all(none[a] is None for a in ARRAYS)
    _, _, only = opt.evalGradF_model(sp.params0, want=("crosskerr",))
    assert only["transfreq"] is None and only["selfkerr"] is None and np.array_equal(only["crosskerr"], sens["crosskerr"])
    assert _same_eval(first, opt.evalGradF(sp.params0))
    opt.close(); h.close()


def _refused(opt, h, sp, rc):
    with pytest.raises(capi.QuandaryAmdError, match=rf"rc={rc}"):
        opt.evalGradF_model(sp.params0)
    assert h.last_kernel("forward") == "" and h.last_kernel("adjoint") == ""  # no sweep was launched


def test_errors():
    """A user-Hamiltonian handle and nranks = 2: QD_ERR_STATE; explicit Euler, fp32-mixed precision and a state beyond one CU's LDS:
    QD_ERR_UNSUPPORTED.  No sweep is launched for any of them."""
    from test_gpu_ensemble import _dense_spec
    sp = _dense_spec([2, 2], lindblad=True)
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    _refused(opt, h, sp, -5)
    opt.close(); h.close()
    sp = sens_spec("2x2-schroedinger")  # (four initial conditions: two ranks divide them)
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp, rank=0, nranks=2)
    _refused(opt, h, sp, -5)
    opt.close(); h.close()
    ee = model_spec([3, 3], stepper="EE", **unequal_constants(2, coupled=False))
    h = capi.Handle(ee)
    opt = capi.Optim(h, ee)
    _refused(opt, h, ee, -2)
    opt.close(); h.close()
    sp = sens_spec("2x2x2x2-lindblad")  # (all qubits, every level essential: what fp32-mixed takes)
    h = capi.Handle(sp)
    h.set_precision("f32mixed")
    opt = capi.Optim(h, sp)
    _refused(opt, h, sp, -2)
    opt.close(); h.close()
    big = model_spec([9, 9], ntime=2, **unequal_constants(2, coupled=False))  # dim 6561 > 4096: the global-memory kernels
    h = capi.Handle(big)
    opt = capi.Optim(h, big)
    _refused(opt, h, big, -2)
    opt.close(); h.close()


def test_the_ensemble_call_samples_the_function_the_sensitivities_differentiate(calls):
    """evalF_ensemble_model at theta +- h e_i against 2 h d_i, for every constant of the 3 x 3 Lindblad system.  The difference of the two
    objectives is 2 h D(h) with D the central difference, d_i sits within max(1e-8 ||ref||, 4 e_ref) of the reference R (the parity test
    above) and D(h) - R = O(h^2) is what the oracle's own central difference at the same step is away from R (reference(): D(h));
    each of the two objectives carries round-off of 1e-12 (helpers.check_parity's absolute objective tolerance)."""
    name = "3x3-lindblad"
    sens = calls[name, None][2]
    ref = reference(name)
    norm = ref_norm(ref)
    sp, h, opt = _open(name)
    for array in ARRAYS:
        R, E, D0 = ref[array]
        step = H.get((name, array), H_DEFAULT)
        for i in range(n_of(sp, array)):
            plus, minus = sens_spec(name).system, sens_spec(name).system
            getattr(plus, array)[i] += step
            getattr(minus, array)[i] -= step
            _, vals = opt.evalF_ensemble_model(sp.params0, [plus, minus])
            diff = vals[0]["objective"] - vals[1]["objective"]
            bound = 2.0 * step * (max(1e-8 * norm, 4.0 * E[i]) + abs(D0[i] - R[i])) + 2e-12
            print(f"{array}[{i}]: J+ - J- = {diff:+.9e}, 2 h d = {2.0 * step * sens[array][i]:+.9e}, bound {bound:.1e}")
            assert abs(diff - 2.0 * step * sens[array][i]) <= bound, (array, i)
    opt.close(); h.close()
