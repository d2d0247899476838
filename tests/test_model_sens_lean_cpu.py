"""Model-constant sensitivities on the lean column kernels (option sens_lean), the CPU side: the references
tests/test_gpu_model_sens_lean.py needs beyond those of tests/test_model_sens_cpu.py, and what they are worth.

Built the same way: a Richardson-extrapolated central difference of the ORACLE's objective, R(h) = (4 D(h/2) - D(h)) / 3 at (h, h/2) and
(h/2, h/4); the finer one is the value, the absolute difference of the two its error estimate e_ref.  Every case has constants of its
own per oscillator and pair (helpers.unequal_constants), every penalty on, 12 steps of 0.002 ns (one case 13: the step count three
time slices do not divide).  The two assertions are those of the other file: e_ref <= 1e-6 of the 2-norm of the case's sensitivity
vector, and every entry at least 1e-3 of that norm unless NOT_A_WITNESS names it, in which case it is asserted to lie below the line.

Steps (H, GHz): chosen per case so that the largest Kerr phase pi n (n - 1) h T over the sweep, T = 0.024 ns, stays around 1e-2 - the
3 x 20 systems take the 5e-4 of the other file (n (n - 1) = 380: 0.014), 8 x 8 takes 2e-3 (n (n - 1) = 56: 0.008; cross-Kerr i_k i_l up
to 49), 4 x 4 x 4 takes 1e-2 (n (n - 1) = 12: 0.009).  transfreq keeps the default 2e-2 (phase 2 pi i h T <= 0.06 at i = 19).
The gmres request is held against helpers.tight_oracle like the one of the other file."""
import functools

import numpy as np
import pytest

from helpers import tight_oracle, unequal_constants
from oracle.oracle import Oracle
from test_ensemble_model_cpu import model_spec
from test_model_sens_cpu import ARRAYS, CAP, H_DEFAULT, WITNESS, is_exact_zero, n_of, ref_norm


def _case(nlevels, tight=False, coupled=False, **kw):
    return dict(nlevels=nlevels, tight=tight, coupled=coupled, kw=kw)


# the smallest shapes that reach the instantiations <Q, EPT> of k_adjoint_col_sens / k_adjoint_colj_sens the other file has no case for
CASES = {
    # <2, 8>: N = 64, guard levels (the adjoint sweep reads stored states for the leakage penalty)
    "8x8-guard": _case([8, 8], nessential=[7, 8]),
    # <3, 8>: N = 64, three oscillators
    "4x4x4": _case([4, 4, 4]),
    # colj <2, 5> / colj <3, 8>: every pair coupled, the rotating frames differ (the coupling rotates)
    "3x20-coupled": _case([3, 20], coupled=True, detuned=True),
    "4x4x4-coupled": _case([4, 4, 4], coupled=True, detuned=True),
    # composite steps: the kernels that test every pass.  linearsolver_maxiter 60 instead of the 20 of the other cases: the sub-steps of
    # IMR4 are up to 1.7 x the step, alpha |diag M| of the 20-level oscillator reaches 0.43 and the reference's plain Neumann iteration
    # - the oracle's and the general kernels' - needs 28 iterations for abstol 1e-10; cut off at 20 (5e-8) it would solve, and
    # differentiate, other equations than the diagonal-split iteration of the lean kernels, which converges in a few
    "3x20-imr4": _case([3, 20], stepper="IMR4", maxiter=60),
    # a gmres request (served by the diagonal-split iteration; with gmres_split = 0 by the Krylov kernels of the general family)
    "3x20-gmres": _case([3, 20], tight=True, linsolve="gmres"),
    # 13 steps: three time slices do not divide them
    "3x20-13steps": _case([3, 20], ntime=13),
}
KERR = ("selfkerr", "crosskerr")
H = {**{(name, a): 5e-4 for name in CASES if name.startswith("3x20") for a in KERR},
     **{("8x8-guard", a): 2e-3 for a in KERR},
     **{(name, a): 1e-2 for name in ("4x4x4", "4x4x4-coupled") for a in KERR}}
# Entries below the witness line, asserted to be there (their parity is still checked on the GPU at the same tolerance).  On 3 x 20 the
# norm is the self-Kerr derivative of the 20-level oscillator and the one of the 3-level oscillator sits just under 1e-3 of it in these
# two cases (8.5e-4, 9.6e-4), as in tests/test_model_sens_cpu.py; oscillator 0 is witnessed by its transfreq entry and by the cross-Kerr
# entry.  Under IMR4 and on 13 steps the same entry is above the line (1.3e-3, 3.5e-3).
NOT_A_WITNESS = {("3x20-coupled", "selfkerr", 0), ("3x20-gmres", "selfkerr", 0)}


def lean_spec(name, options=None):
    """A fresh spec of the case (the GPU tests create their handles from it)."""
    c = CASES[name]
    return model_spec(c["nlevels"], options=options, **{**unequal_constants(len(c["nlevels"]), coupled=c["coupled"]), **c["kw"]})


def _objective(name, array, i, delta):
    sp = lean_spec(name)
    getattr(sp.system, array)[i] += delta
    orc = tight_oracle(sp) if CASES[name]["tight"] else Oracle(sp)
    try:
        return orc.evalF(sp.params0)[0]["objective"]
    finally:
        orc.close()


@functools.lru_cache(maxsize=None)
def lean_reference(name):
    """{array: (R [n], e_ref [n])} of the case, computed once per process and read-only."""
    sp = lean_spec(name)
    out = {}
    for array in ARRAYS:
        n = n_of(sp, array)
        R, E = np.zeros(n), np.zeros(n)
        h = H.get((name, array), H_DEFAULT)
        for i in range(n):
            D = [(_objective(name, array, i, s) - _objective(name, array, i, -s)) / (2.0 * s) for s in (h, h / 2.0, h / 4.0)]
            r1, r2 = (4.0 * D[1] - D[0]) / 3.0, (4.0 * D[2] - D[1]) / 3.0
            R[i], E[i] = r2, abs(r2 - r1)
        for a in (R, E):
            a.setflags(write=False)
        out[array] = (R, E)
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_reference_error_is_capped_and_every_entry_is_a_witness(name):
    ref = lean_reference(name)
    sp = lean_spec(name)
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
            assert not is_exact_zero(sp, array, i)  # (no two-level oscillator among these systems)
            if (name, array, i) in NOT_A_WITNESS:
                assert 0.0 < abs(R[i]) < WITNESS * norm, (array, i)  # (or it does not belong in that table)
            else:
                assert abs(R[i]) >= WITNESS * norm, (array, i)


def test_systems_have_constants_of_their_own():
    for name in CASES:
        s = lean_spec(name).system
        for array in ARRAYS:
            v = list(getattr(s, array))[:n_of(lean_spec(name), array)]
            assert len(set(v)) == len(v), (name, array)  # a swapped oscillator or pair index shows
    for name in ("3x20-coupled", "4x4x4-coupled"):
        s = lean_spec(name).system
        Q = s.nosc
        assert all(s.Jkl[p] != 0.0 for p in range(Q * (Q - 1) // 2)) and list(s.rotfreq)[:Q] != list(s.transfreq)[:Q]
