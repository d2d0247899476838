"""Model-parameter ensemble on the CPU: the fixtures of tests/test_gpu_ensemble_model.py and what makes them worth running.

A variant of the ensemble replaces transfreq, selfkerr, crosskerr and Jkl of a system.  variant_specs() builds the specs the oracle is
asked with: block 0 is the system itself, block 1 moves every array, block 2 is a copy of block 0, block 3 moves them the other way
(coupled systems: with every coupling zero).  The objective is the gate trace on the three initial states of the `3states` set, which
carry coherences: it sees the phases a detuning or a Kerr shift winds up, where the populations of twelve short steps alone would not.
The tests here state the witness: changing ONLY one of the four arrays between blocks 0 and 1 moves the oracle's gradient by at least ten
times the tolerance helpers.check_parity compares gradients at (1e-8 of the norm + 1e-13) - so a kernel that read a constant of the wrong
variant, or left one array at the handle's own value, could not pass the GPU tests.

The step is 0.002 ns: at 0.004 ns the reference's own Neumann iteration (linearsolver_maxiter = 20) no longer converges on the 20-level
oscillator of 3 x 20 - the oracle's gradient then sits 1.2e-8 of its norm from the exact discrete solution (helpers.tight_oracle), above
the 1e-8 it is compared at; at 0.002 ns that distance is 4e-11, at 0.001 ns 1e-12."""
import numpy as np
import pytest

from helpers import synthetic_spec
from oracle.oracle import Oracle

ARRAYS = ("transfreq", "selfkerr", "crosskerr", "Jkl")
# GHz per unit of a block's multiplier, entry i of an array scaled by (1 + 0.3 i): pair-wise different cross-Kerr and coupling values
STEP = {"transfreq": 0.3, "selfkerr": 0.1, "crosskerr": 0.05, "Jkl": 0.01}
BLOCKS = (0.0, 1.0, 0.0, -0.7)  # multiplier of the four distinct blocks; block 2 is a copy of block 0


def model_spec(nlevels, options=None, ntime=12, **kw):
    """12 steps of 0.002 ns, every Lindblad penalty, gate trace on the three `3states` initial conditions (essential levels 2 x 2 (x 1 ...): a CNOT target)."""
    kw = {**dict(lindblad=True, target="gate", objective="Jtrace", init="3states", ntime=ntime, dt=0.002, penalties=True,
                 nessential=([2, 2] + [1] * len(nlevels))[:len(nlevels)]), **kw}
    sp = synthetic_spec(nlevels, **kw)
    for i in range(len(sp.system.Jkl)):  # (coupled systems: pairs that differ, so that a mixed-up pair column shows)
        sp.system.Jkl[i] *= 1.0 + 0.37 * i
    sp.options = dict(options or {})
    return sp


def n_of(sp, name):
    Q = sp.system.nosc
    return Q if name in ("transfreq", "selfkerr") else Q * (Q - 1) // 2


def variant_specs(make, coupled, only=None, blocks=BLOCKS):
    """One spec per block, from make() (a fresh spec of the system): every array that applies moved by the block's multiplier - Jkl on
    coupled systems only, where the last block has every coupling zero instead.  only: move that one array and leave the others."""
    out = []
    for b, mult in enumerate(blocks):
        sp = make()
        for name in ARRAYS:
            if (only is not None and name != only) or (name == "Jkl" and not coupled):
                continue
            arr = getattr(sp.system, name)
            for i in range(n_of(sp, name)):
                arr[i] = 0.0 if (name == "Jkl" and b == 3 and only is None) else arr[i] + mult * STEP[name] * (1.0 + 0.3 * i)
        out.append(sp)
    return out


def oracle_grads(specs, alpha):
    out = []
    for sp in specs:
        orc = Oracle(sp)
        out.append(orc.evalGradF(alpha))
        orc.close()
    return out


CASES = [pytest.param([3, 20], {}, False, id="3x20"), pytest.param([3, 20], dict(jkl=0.004, detuned=True), True, id="3x20-coupled"),
         pytest.param([3, 3, 5], {}, False, id="3x3x5")]


@pytest.mark.parametrize("nlevels,kw,coupled", CASES)
def test_each_array_alone_moves_the_oracle_gradient(nlevels, kw, coupled):
    def make():
        return model_spec(nlevels, **kw)
    base = make()
    (_, g0), = oracle_grads([base], base.params0)
    tol = 1e-8 * np.linalg.norm(g0) + 1e-13  # helpers.check_parity's gradient tolerance
    for name in ARRAYS:
        if name == "Jkl" and not coupled:
            continue
        one = variant_specs(make, coupled, only=name, blocks=BLOCKS[:2])[1]
        for other in ARRAYS:  # only that array differs
            same = list(getattr(one.system, other)) == list(getattr(base.system, other))
            assert same == (other != name), (name, other)
        (_, g1), = oracle_grads([one], base.params0)
        moved = np.linalg.norm(g1 - g0)
        print(f"{name}: moves the gradient by {moved / np.linalg.norm(g0):.2e} of its norm ({moved / tol:.1e} x the parity tolerance)")
        assert moved >= 10.0 * tol, name


def test_blocks_are_what_the_gpu_tests_assume():
    specs = variant_specs(lambda: model_spec([3, 20], jkl=0.004, detuned=True), True)
    s = [sp.system for sp in specs]
    for name in ARRAYS:
        assert list(getattr(s[0], name)) == list(getattr(s[2], name)), name  # block 2 is a copy of block 0
        assert list(getattr(s[0], name)) != list(getattr(s[1], name)) != list(getattr(s[3], name)), name
    assert s[3].Jkl[0] == 0.0 and s[0].Jkl[0] != 0.0  # one block with every coupling zero
    three = variant_specs(lambda: model_spec([3, 3, 5]), False)
    ck = [tuple(sp.system.crosskerr[:3]) for sp in three]
    assert all(len(set(c)) == 3 for c in (ck[1], ck[3]))  # pair-wise different cross-Kerr where a block moves it
    assert all(list(sp.system.rotfreq) == list(three[0].system.rotfreq) for sp in three)  # the frame stays
    assert all(np.array_equal(sp.params0, three[0].params0) for sp in three)  # ... and so does the control vector
