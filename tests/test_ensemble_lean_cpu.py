"""Model-parameter ensemble on the lean slot and fp32-mixed kernels (option ensemble_lean) on the CPU: the shape table of
tests/test_gpu_ensemble_lean.py and what makes its fixtures worth running.

The fixtures are those of tests/test_ensemble_model_cpu.py (model_spec / variant_specs / BLOCKS: 12 steps of 0.002 ns, every penalty, the
gate trace on the three `3states` initial conditions, four blocks of constants with block 2 a copy of block 0 and, on coupled systems,
the last block with every coupling zero) on the all-qubit Lindblad systems the two families serve: 2 x 2 x 2 (fp32-mixed only), 2^4 and
2^5, uncoupled and coupled.  The witness is the one stated there: changing ONLY transfreq, only crosskerr or - coupled systems - only
Jkl between blocks 0 and 1 moves the oracle's gradient by at least ten times the tolerance helpers.check_parity compares gradients at
(1e-8 of the norm + 1e-13), so a kernel that read a constant of the wrong variant, or left one array at the handle's own value, could not
pass the GPU tests.  selfkerr is exempt: the self-Kerr term a (a - 1) vanishes on two levels, and Q32::init has no such term."""
import numpy as np
import pytest

from test_ensemble_model_cpu import ARRAYS, BLOCKS, model_spec, oracle_grads, variant_specs

COUPLED = dict(jkl=0.004, detuned=True)

# id, number of qubits, coupled
SYSTEMS = [("2x2x2", 3, False), ("2^4", 4, False), ("2^4-coupled", 4, True), ("2^5", 5, False), ("2^5-coupled", 5, True)]


def qubit_spec(Q, coupled, options=None, **kw):
    """model_spec of Q qubits, all levels essential."""
    return model_spec([2] * Q, options=options, nessential=[2] * Q, **{**(COUPLED if coupled else {}), **kw})


@pytest.mark.parametrize("Q,coupled", [pytest.param(q, c, id=i) for i, q, c in SYSTEMS])
def test_each_array_alone_moves_the_oracle_gradient(Q, coupled):
    def make():
        return qubit_spec(Q, coupled)
    base = make()
    assert base.time.ntime == 12 and base.time.dt == 0.002 and base.ninit == 3
    (_, g0), = oracle_grads([base], base.params0)
    tol = 1e-8 * np.linalg.norm(g0) + 1e-13  # helpers.check_parity's gradient tolerance
    for name in ARRAYS:
        if name == "selfkerr" or (name == "Jkl" and not coupled):
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
    for _, Q, coupled in SYSTEMS:
        specs = variant_specs(lambda: qubit_spec(Q, coupled), coupled)
        s = [sp.system for sp in specs]
        npairs = Q * (Q - 1) // 2
        for name in ("transfreq", "crosskerr") + (("Jkl",) if coupled else ()):
            assert list(getattr(s[0], name)) == list(getattr(s[2], name)), name  # block 2 is a copy of block 0
            assert list(getattr(s[0], name)) != list(getattr(s[1], name)) != list(getattr(s[3], name)), name
        assert len(set(s[1].crosskerr[:npairs])) == npairs  # pair-wise different cross-Kerr where a block moves it
        assert coupled == any(j != 0.0 for j in s[0].Jkl[:npairs])
        if coupled:
            assert len(set(s[0].Jkl[:npairs])) == npairs and all(j == 0.0 for j in s[3].Jkl[:npairs])  # one block with every coupling zero
        assert all(np.array_equal(sp.params0, specs[0].params0) for sp in specs)  # the control vector stays
