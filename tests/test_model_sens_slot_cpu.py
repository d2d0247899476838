"""Model-constant sensitivities on the lean slot kernels (option sens_slot), the CPU side: the references
tests/test_gpu_model_sens_slot.py needs beyond the 2x2x2x2-lindblad case of tests/test_model_sens_cpu.py, and what they are worth.

Built the same way: a Richardson-extrapolated central difference of the ORACLE's objective, R(h) = (4 D(h/2) - D(h)) / 3 at (h, h/2) and
(h/2, h/4); the finer one is the value, the absolute difference of the two its error estimate e_ref.  Every case is an all-qubit
Lindblad system with every level essential - what the lean slot kernels take -, constants of its own per oscillator and pair
(helpers.unequal_constants), every penalty on, the three `3states` initial conditions, and is driven like the 2x2x2x2-lindblad case
of the other file (ctrl_init "random, 0.5", 20 steps of 0.002 ns) for the reason its docstring gives: without guard levels the
sensitivity vector is 2e-7 of the objective under the weaker controls, and the round-off of a difference quotient would be its e_ref.
The two assertions are those of the other file: e_ref <= 1e-6 of the 2-norm of the case's sensitivity vector, and every entry that is
not an exact zero - the self-Kerr derivative of a two-level oscillator, all of them here - at least 1e-3 of that norm.  No entry is
exempt: there is no NOT_A_WITNESS table.

Steps (H, GHz): the default 2e-2 of the other file throughout - the largest phase over the sweep, 2 pi h T with T = 0.04 ns, is 0.005
(two levels: i_k i_l <= 1).  The gmres request is held against helpers.tight_oracle like the ones of the other files."""
import functools

import numpy as np
import pytest

from helpers import tight_oracle, unequal_constants
from oracle.oracle import Oracle
from test_ensemble_model_cpu import model_spec
from test_model_sens_cpu import ARRAYS, CAP, H_DEFAULT, WITNESS, is_exact_zero, n_of, ref_norm


def _case(Q, tight=False, coupled=False, **kw):
    nlevels = [2] * Q
    return dict(nlevels=nlevels, tight=tight, coupled=coupled, kw={**dict(nessential=list(nlevels), ctrl_init="random, 0.5", ntime=20), **kw})


# the instantiations <Q, SB, double, false, HJ> of k_adjoint_q32_sens the 2x2x2x2-lindblad case of the other file (<4, 0>) does not reach,
# and the two requests that differ in the solver and the stepper
CASES = {
    # <5, 1> and <5, 2> (option lean64_sb)
    "2x2x2x2x2": _case(5),
    # <4, 0, ..., HJ> / <5, 1, ..., HJ>: every pair coupled, the rotating frames differ (the coupling rotates)
    "2x2x2x2-coupled": _case(4, coupled=True, detuned=True),
    "2x2x2x2x2-coupled": _case(5, coupled=True, detuned=True),
    # a gmres request (served by the stand-in iteration of the lean slot kernels; with gmres_split = 0 by the general family)
    "2x2x2x2-gmres": _case(4, tight=True, linsolve="gmres"),
    # composite steps
    "2x2x2x2-imr4": _case(4, stepper="IMR4"),
}
H = {}  # (case, array) -> step, everything else H_DEFAULT


def slot_spec(name, options=None):
    """A fresh spec of the case (the GPU tests create their handles from it)."""
    c = CASES[name]
    return model_spec(c["nlevels"], options=options, **{**unequal_constants(len(c["nlevels"]), coupled=c["coupled"]), **c["kw"]})


def _objective(name, array, i, delta):
    sp = slot_spec(name)
    getattr(sp.system, array)[i] += delta
    orc = tight_oracle(sp) if CASES[name]["tight"] else Oracle(sp)
    try:
        return orc.evalF(sp.params0)[0]["objective"]
    finally:
        orc.close()


@functools.lru_cache(maxsize=None)
def slot_reference(name):
    """{array: (R [n], e_ref [n])} of the case, computed once per process and read-only."""
    sp = slot_spec(name)
    out = {}
    for array in ARRAYS:
        n = n_of(sp, array)
        R, E = np.zeros(n), np.zeros(n)
        h = H.get((name, array), H_DEFAULT)
        for i in range(n):
            if is_exact_zero(sp, array, i):
                # (the objective does not see the self-Kerr coefficient of a two-level oscillator: checked below on one entry per case)
                continue
            D = [(_objective(name, array, i, s) - _objective(name, array, i, -s)) / (2.0 * s) for s in (h, h / 2.0, h / 4.0)]
            r1, r2 = (4.0 * D[1] - D[0]) / 3.0, (4.0 * D[2] - D[1]) / 3.0
            R[i], E[i] = r2, abs(r2 - r1)
        for a in (R, E):
            a.setflags(write=False)
        out[array] = (R, E)
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_reference_error_is_capped_and_every_entry_is_a_witness(name):
    ref = slot_reference(name)
    sp = slot_spec(name)
    norm = ref_norm(ref)
    assert norm > 0.0
    for array in ARRAYS:
        R, E = ref[array]
        for i in range(len(R)):
            print(f"{name} {array}[{i}]: R = {R[i]:+.6e}, e_ref / norm = {E[i] / norm:.1e}, |R| / norm = {abs(R[i]) / norm:.1e}")
    for array in ARRAYS:
        R, E = ref[array]
        for i in range(len(R)):
            assert E[i] <= CAP * norm, (array, i)
            if is_exact_zero(sp, array, i):
                assert R[i] == 0.0 and E[i] == 0.0, (array, i)
            else:
                assert abs(R[i]) >= WITNESS * norm, (array, i)
    # the exact zeros are zeros of the oracle too: the objective is the same number with the last oscillator's self-Kerr moved
    last = sp.system.nosc - 1
    assert _objective(name, "selfkerr", last, H_DEFAULT) == _objective(name, "selfkerr", last, -H_DEFAULT)


def test_systems_are_what_the_lean_slot_kernels_take_with_constants_of_their_own():
    for name in CASES:
        sp = slot_spec(name)
        s = sp.system
        Q = s.nosc
        assert Q in (4, 5) and list(s.nlevels)[:Q] == [2] * Q and list(s.nessential)[:Q] == [2] * Q and sp.ninit == 3
        for array in ARRAYS:
            v = list(getattr(s, array))[:n_of(sp, array)]
            assert len(set(v)) == len(v), (name, array)  # a swapped oscillator or pair index shows
        npairs = Q * (Q - 1) // 2
        if CASES[name]["coupled"]:
            assert all(s.Jkl[p] != 0.0 for p in range(npairs)) and list(s.rotfreq)[:Q] != list(s.transfreq)[:Q]
        else:
            assert all(s.Jkl[p] == 0.0 for p in range(npairs))
