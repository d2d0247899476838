"""Model-parameter ensemble on the general kernel family (option ensemble_general) on the CPU: the shape table of
tests/test_gpu_ensemble_general.py and what makes its fixtures worth running.

The fixtures are those of tests/test_ensemble_model_cpu.py (model_spec / variant_specs / BLOCKS: 12 steps, the `3states` set for
Lindblad and the `basis` set for Schroedinger systems, at most 8 initial conditions, four blocks of constants with block 2 a copy of
block 0 and the last block with every coupling zero on coupled systems) on the small systems that reach each stencil and variant of the
general family.  The witness is the one stated there for 3 x 20: changing ONLY one of the four arrays between blocks 0 and 1 moves the
oracle's gradient by at least ten times the tolerance helpers.check_parity compares gradients at (1e-8 of the norm + 1e-13).  One array
is exempt where the model has no such term: selfkerr on an all-qubit system (the self-Kerr term a (a - 1) vanishes on two levels).

The step stays 0.002 ns.  The oracle's own Neumann iteration (linearsolver_maxiter = 20) converges there on every fixture: its gradient
is compared with the exact discrete solution (helpers.tight_oracle) below and must sit within a tenth of the parity tolerance of it.
Distances measured (relative to the gradient norm): 2 x 2 Schroedinger 3e-15 (without penalties 2e-12, explicit Euler 0: no linear
solve), 3 x 3 Schroedinger 2e-13, 3 x 3 Lindblad 2e-14 (coupled, IMR4: 2e-13), 2^3 coupled 3e-14, 3 x 3 x 3 3e-14, 2^4 3e-16, 2^5 7e-16,
3 x 20 5e-11 (the largest: 5e-3 of the parity tolerance), 6 x 6 x 6 x 6 Schroedinger 1e-13."""
import numpy as np
import pytest

from helpers import tight_oracle
from test_ensemble_model_cpu import ARRAYS, BLOCKS, model_spec, oracle_grads, variant_specs

SCHR = dict(lindblad=False, init="basis")

# id, nlevels, model_spec keywords, coupled, handle options, "<Q, LIND, VAR, QUBIT" of the kernels the system runs on (the GM and PLAIN
# arguments follow from the solver and the penalties).  Each the smallest system that reaches its stencil and variant:
#   QubitStencil: 2 x 2 (one wave, variant 0), 2^3 Lindblad coupled (dim 64, variant 0), 2^4 Lindblad (dim 256, four waves, variant 1; the
#                 lean slot kernels switched off)
#   QubitSlotStencil: 2^5 Lindblad (dim 1024, four elements per thread, variant 2; the lean slot kernels switched off)
#   GenStencil: 3 x 3 Schroedinger (variant 0) and Lindblad (dim 81, variant 1) with guard levels and every penalty; 6^4 Schroedinger
#               (dim 1296 > 1024: eight elements per thread, variant 4)
#   ColStencil: 3 x 3 x 3 Lindblad (N = 27: packed columns, four elements per thread, variant 14); 3 x 20 with the lean column kernels
#               switched off (N = 60: variant 9)
SHAPES = [
    ("2x2-schroedinger", [2, 2], dict(SCHR, nessential=[2, 2]), False, {}, "2, false, 0, true"),
    ("2x2-schroedinger-plain", [2, 2], dict(SCHR, nessential=[2, 2], penalties=False), False, {}, "2, false, 0, true"),
    ("2x2-schroedinger-coupled-EE", [2, 2], dict(SCHR, nessential=[2, 2], jkl=0.004, detuned=True, stepper="EE"), True, {}, "2, false, 0, true"),
    ("3x3-schroedinger", [3, 3], dict(SCHR), False, {}, "2, false, 0, false"),
    ("3x3-lindblad", [3, 3], {}, False, {}, "2, true, 1, false"),
    ("3x3-lindblad-coupled-IMR4", [3, 3], dict(jkl=0.004, detuned=True, stepper="IMR4"), True, {}, "2, true, 1, false"),
    ("2x2x2-lindblad-coupled", [2, 2, 2], dict(nessential=[2, 2, 2], jkl=0.004, detuned=True), True, {}, "3, true, 0, true"),
    ("3x3x3-lindblad", [3, 3, 3], {}, False, {}, "3, true, 14, false"),
    ("2^4-lindblad-no_lean64", [2, 2, 2, 2], dict(nessential=[2, 2, 2, 2]), False, {"no_lean64": "1"}, "4, true, 1, true"),
    ("2^5-lindblad-no_lean64", [2, 2, 2, 2, 2], dict(nessential=[2, 2, 2, 2, 2], jkl=0.004), True, {"no_lean64": "1"}, "5, true, 2, true"),
    ("3x20-no_collean", [3, 20], {}, False, {"no_collean": "1"}, "2, true, 9, false"),
    ("6x6x6x6-schroedinger", [6, 6, 6, 6], dict(SCHR), False, {}, "4, false, 4, false"),
]
SHAPE_PARAMS = [pytest.param(*s[1:], id=s[0]) for s in SHAPES]


def shape(name):
    """(nlevels, kw, coupled, options, args) of the named row."""
    return next(s[1:] for s in SHAPES if s[0] == name)


def applies(name, nlevels, coupled):
    if name == "Jkl":
        return coupled
    if name == "selfkerr":
        return any(n > 2 for n in nlevels)
    return name != "crosskerr" or len(nlevels) > 1


@pytest.mark.parametrize("nlevels,kw,coupled,options,args", SHAPE_PARAMS)
def test_each_array_alone_moves_the_oracle_gradient(nlevels, kw, coupled, options, args):
    def make():
        return model_spec(nlevels, **kw)
    base = make()
    assert base.time.ntime == 12 and base.time.dt == 0.002
    (_, g0), = oracle_grads([base], base.params0)
    tol = 1e-8 * np.linalg.norm(g0) + 1e-13  # helpers.check_parity's gradient tolerance
    tight = tight_oracle(base)
    _, gt = tight.evalGradF(base.params0)
    tight.close()
    dist = np.linalg.norm(g0 - gt)
    print(f"oracle against the exact discrete solution: {dist / np.linalg.norm(g0):.1e} of the gradient norm ({dist / tol:.1e} x the parity tolerance)")
    assert dist <= 0.1 * tol  # the oracle's own Neumann iteration has converged at this step
    for name in ARRAYS:
        if not applies(name, nlevels, coupled):
            continue
        one = variant_specs(make, coupled, only=name, blocks=BLOCKS[:2])[1]
        for other in ARRAYS:  # only that array differs
            same = list(getattr(one.system, other)) == list(getattr(base.system, other))
            assert same == (other != name), (name, other)
        (_, g1), = oracle_grads([one], base.params0)
        moved = np.linalg.norm(g1 - g0)
        print(f"{name}: moves the gradient by {moved / np.linalg.norm(g0):.2e} of its norm ({moved / tol:.1e} x the parity tolerance)")
        assert moved >= 10.0 * tol, name


def test_the_table_covers_what_the_gpu_tests_promise():
    args = [s[5] for s in SHAPES]
    assert {a.split(", ")[2] for a in args} == {"0", "1", "2", "4", "9", "14"}  # every LDS variant of the standard model
    assert {(a.split(", ")[1], a.split(", ")[3]) for a in args} == {("false", "true"), ("false", "false"), ("true", "true"), ("true", "false")}
    steppers = {s[2].get("stepper", "IMR") for s in SHAPES}
    assert steppers == {"IMR", "IMR4", "EE"}
    for _, nlevels, kw, coupled, _, _ in SHAPES:
        sp = model_spec(nlevels, **kw)
        assert coupled == any(j != 0.0 for j in sp.system.Jkl)
    three = variant_specs(lambda: model_spec([2, 2, 2], **shape("2x2x2-lindblad-coupled")[1]), True)
    assert all(len(set(sp.system.Jkl[:3])) == 3 for sp in three[:3])  # pair-wise different couplings
    assert all(j == 0.0 for j in three[3].system.Jkl)                 # ... and one block without any
