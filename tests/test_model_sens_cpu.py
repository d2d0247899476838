"""Model-constant sensitivities on the CPU: the reference tests/test_gpu_model_sens.py holds qd_optim_evalGradF_model against, and
what that reference is worth.

The reference for d objective / d constant is a Richardson-extrapolated central difference of the ORACLE's objective: with D(h) the
central difference over specs whose one constant is moved by +-h (GHz, everything else - rotation frequencies included - as it was),
R(h) = (4 D(h/2) - D(h)) / 3.  reference() takes R at (h, h/2) and at (h/2, h/4); the finer one is the value, the absolute difference
of the two its own error estimate e_ref.  The tests here assert, for every case and constant the GPU tests use,
  * e_ref <= 1e-6 of the 2-norm of the case's whole sensitivity vector (a cap on the reference's error, not a measurement), and
  * every entry is at least 1e-3 of that norm, so that a kernel that returned zero for it could not pass - except the self-Kerr
    derivative of a two-level oscillator, which is exactly 0.0 (i (i - 1) = 0 for i = 0, 1) and is asserted as such on the GPU.

Steps: H below, per case and array.  2e-2 GHz wherever the table does not say otherwise.  On 3 x 20 the self-Kerr phase of the 20-level
oscillator, pi n (n - 1) h T with n (n - 1) = 380 and T = 0.024 ns, is 0.57 at 2e-2 - not small, the extrapolation no longer converges
(2e-4 of the norm) - so that system takes 5e-4 for selfkerr (phase 0.014) and the same for crosskerr (i_k i_l up to 38).
The Frobenius distance to a pure target hardly moves with the constants over so short a time: with the controls of the other cases
(amplitude 0.005, 12 steps) the whole sensitivity vector is 3e-7 of the objective, and the round-off of a difference quotient, about
1e-16 |J| / h = 3e-15, is 2e-8 of that vector at h = 2e-2 - above the 1e-8 the GPU result is held at, so its e_ref would be rounding
noise.  That case therefore drives harder and longer (amplitude 0.5, 20 steps: the vector is 2e-5 of the objective) and takes h = 5e-2
(largest phase 2 pi 2 h T = 0.025), which puts the round-off of the quotient at 1e-10 of the vector.
A case marked tight takes helpers.tight_oracle - every linear system solved to round-off - where the plain oracle's solver noise
(abstol 1e-10 per solve, divided by the step) is what would limit the difference quotient: the gmres requests."""
import functools

import numpy as np
import pytest

from helpers import tight_oracle, unequal_constants
from oracle.oracle import Oracle
from test_ensemble_model_cpu import model_spec

ARRAYS = ("transfreq", "selfkerr", "crosskerr")
H_DEFAULT = 2e-2


def _case(nlevels, tight=False, coupled=False, **kw):
    return dict(nlevels=nlevels, tight=tight, coupled=coupled, kw=kw)


# every system with constants of its own per oscillator and pair (helpers.unequal_constants); penalties on throughout (model_spec)
CASES = {
    "2x2-schroedinger": _case([2, 2], lindblad=False, init="basis"),
    "3x3-schroedinger": _case([3, 3], lindblad=False, init="basis"),
    "3x3-lindblad": _case([3, 3]),
    "2x2x2-lindblad": _case([2, 2, 2]),
    # (every level essential: what the lean slot kernels take; driven like the Frobenius case below, for the same reason - without
    # guard levels the vector is 2e-7 of the objective under the controls of the other cases)
    "2x2x2x2-lindblad": _case([2, 2, 2, 2], nessential=[2, 2, 2, 2], ctrl_init="random, 0.5", ntime=20),
    "3x20-lindblad": _case([3, 20]),
    "3x3x5-lindblad": _case([3, 3, 5]),
    "3x3-lindblad-coupled": _case([3, 3], coupled=True, detuned=True),
    "3x3-lindblad-frobenius-pure": _case([3, 3], objective="Jfrobenius", target="pure", ctrl_init="random, 0.5", ntime=20),
    "3x3-lindblad-imr4": _case([3, 3], stepper="IMR4"),
    "3x3-lindblad-imr8": _case([3, 3], stepper="IMR8"),
    "3x3-lindblad-gmres": _case([3, 3], tight=True, linsolve="gmres"),
}
# GHz; (case, array) -> step, everything else H_DEFAULT
H = {
    ("3x20-lindblad", "selfkerr"): 5e-4,
    ("3x20-lindblad", "crosskerr"): 5e-4,
    ("3x3-lindblad-frobenius-pure", "transfreq"): 5e-2,
    ("3x3-lindblad-frobenius-pure", "selfkerr"): 5e-2,
    ("3x3-lindblad-frobenius-pure", "crosskerr"): 5e-2,
}
CAP = 1e-6      # e_ref <= CAP x ||R||_2
WITNESS = 1e-3  # |entry| >= WITNESS x ||R||_2
# Entries that are NOT counted as witnesses (their parity is still checked on the GPU, at the same tolerance): on 3 x 20 the norm is the
# self-Kerr derivative of the 20-level oscillator (0.2), and the one of the 3-level oscillator is 9.6e-4 of it - just under the line.
# Oscillator 0 of that system is witnessed by its transfreq entry (1.7e-3) and by the cross-Kerr entry.
NOT_A_WITNESS = {("3x20-lindblad", "selfkerr", 0)}


def sens_spec(name, options=None):
    """A fresh spec of the case (the GPU tests create their handles from it)."""
    c = CASES[name]
    return model_spec(c["nlevels"], options=options, **{**unequal_constants(len(c["nlevels"]), coupled=c["coupled"]), **c["kw"]})


def n_of(sp, array):
    Q = sp.system.nosc
    return Q if array in ("transfreq", "selfkerr") else Q * (Q - 1) // 2


def is_exact_zero(sp, array, i):
    return array == "selfkerr" and sp.system.nlevels[i] == 2


def _objective(name, array, i, delta):
    sp = sens_spec(name)
    getattr(sp.system, array)[i] += delta
    orc = tight_oracle(sp) if CASES[name]["tight"] else Oracle(sp)
    try:
        return orc.evalF(sp.params0)[0]["objective"]
    finally:
        orc.close()


@functools.lru_cache(maxsize=None)
def reference(name):
    """{array: (R [n], e_ref [n], D(h) [n])} of the case, computed once per process; D(h) is the plain central difference at the
    table's step (what the cross-check against the ensemble call measures its O(h^2) term with)."""
    sp = sens_spec(name)
    out = {}
    for array in ARRAYS:
        n = n_of(sp, array)
        R, E, D0 = np.zeros(n), np.zeros(n), np.zeros(n)
        h = H.get((name, array), H_DEFAULT)
        for i in range(n):
            D = [(_objective(name, array, i, s) - _objective(name, array, i, -s)) / (2.0 * s) for s in (h, h / 2.0, h / 4.0)]
            r1, r2 = (4.0 * D[1] - D[0]) / 3.0, (4.0 * D[2] - D[1]) / 3.0
            R[i], E[i], D0[i] = r2, abs(r2 - r1), D[0]
        for a in (R, E, D0):
            a.setflags(write=False)
        out[array] = (R, E, D0)
    return out


def ref_norm(ref):
    return float(np.linalg.norm(np.concatenate([ref[a][0] for a in ARRAYS])))


@pytest.mark.parametrize("name", list(CASES))
def test_reference_error_is_capped_and_every_entry_is_a_witness(name):
    ref = reference(name)
    sp = sens_spec(name)
    norm = ref_norm(ref)
    assert norm > 0.0
    for array in ARRAYS:
        R, E, _ = ref[array]
        for i in range(len(R)):
            print(f"{name} {array}[{i}]: R = {R[i]:+.6e}, e_ref / norm = {E[i] / norm:.1e}, |R| / norm = {abs(R[i]) / norm:.1e}")
            assert E[i] <= CAP * norm, (array, i)
            if is_exact_zero(sp, array, i):
                assert R[i] == 0.0 and E[i] == 0.0, (array, i)
            elif (name, array, i) in NOT_A_WITNESS:
                assert 0.0 < abs(R[i]) < WITNESS * norm, (array, i)  # (or it does not belong in that table)
            else:
                assert abs(R[i]) >= WITNESS * norm, (array, i)


def test_systems_have_constants_of_their_own():
    for name in CASES:
        s = sens_spec(name).system
        Q = s.nosc
        for array in ARRAYS:
            v = list(getattr(s, array))[:n_of(sens_spec(name), array)]
            assert len(set(v)) == len(v), (name, array)  # a swapped oscillator or pair index shows
        assert list(s.rotfreq)[:Q] == list(sens_spec(name).system.rotfreq)[:Q]
    s = sens_spec("3x3-lindblad-coupled").system
    assert s.Jkl[0] != 0.0 and list(s.rotfreq)[:2] != list(s.transfreq)[:2]  # coupled AND detuned: the coupling rotates
