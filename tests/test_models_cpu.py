"""quandary_amd.models.standard_hamiltonians: the dense matrices it builds describe the system the spec describes.  The oracle applies
its right-hand side once with the standard model of the spec (matrix-free stencil) and once with the matrices as a user-supplied
Hamiltonian (dense operator); both must agree, plain and transposed."""
import numpy as np
import pytest

from helpers import synthetic_spec
from oracle.oracle import Oracle
from quandary_amd.models import standard_hamiltonians

CASES = {
    "2x2-schroedinger": dict(nlevels=[2, 2], lindblad=False, detuned=True),
    "3x4-lindblad-guard": dict(nlevels=[3, 4], lindblad=True, nessential=[2, 3], detuned=True),  # T1 / T2 decay, one guard level each
    "2x2x2-lindblad-jkl": dict(nlevels=[2, 2, 2], lindblad=True, detuned=True, jkl=0.02),        # coupled, one rotation frequency
}


@pytest.mark.parametrize("case", list(CASES))
def test_matrices_reproduce_the_standard_model(case):
    kw = {"ntime": 10, "dt": 0.01, **CASES[case]}
    sp, spd = synthetic_spec(**kw), synthetic_spec(**kw)
    if kw.get("jkl"):
        assert len(set(sp.system.rotfreq[k] for k in range(sp.system.nosc))) == 1 and sp.system.Jkl[0] != 0.0
    hsys, hc = standard_hamiltonians(sp)
    n = int(np.prod(kw["nlevels"]))
    assert hsys.shape == (n, n) and hc.shape == (len(kw["nlevels"]), n, n)
    assert np.array_equal(hsys, hsys.conj().T) and np.abs(hsys).max() > 0.0
    spd.hamiltonian = (hsys, hc)
    stencil, dense = Oracle(sp), Oracle(spd)
    alpha = 40.0 * sp.params0  # (amplitudes of 2 pi x 0.2 rad/ns: of the size of the Kerr terms)
    stencil.set_params(alpha)
    dense.set_params(alpha)
    x = np.random.default_rng(2024).standard_normal(2 * stencil.dim)
    for t in (0.013, 0.071):
        assert np.abs(stencil.eval_controls(np.array([t]))).min() > 0.0  # every p_k, q_k is non-zero at both times
        for transpose in (False, True):
            y = stencil.apply_rhs(t, x, transpose=transpose)[0]
            yd = dense.apply_rhs(t, x, transpose=transpose)[0]
            scale = np.abs(y).max()
            print(case, t, transpose, np.abs(y - yd).max() / scale)
            # both sides are the oracle and differ by summation order only: fewer than 200 terms per row at 1.1e-16 each
            assert scale > 0.0 and np.abs(y - yd).max() <= 1e-12 * scale
    stencil.close()
    dense.close()


def test_time_dependent_coupling_is_rejected():
    """Coupled oscillators that rotate at different frequencies: eta_kl != 0, the coupling oscillates, no constant Hsys."""
    sp = synthetic_spec([2, 2, 2], lindblad=True, detuned=False, jkl=0.02, ntime=10)
    assert sp.system.rotfreq[0] != sp.system.rotfreq[1]
    with pytest.raises(ValueError):
        standard_hamiltonians(sp)
    sp = synthetic_spec([2, 2, 2], lindblad=True, detuned=False, jkl=0.0, ntime=10)  # uncoupled: every frame is fine
    assert standard_hamiltonians(sp)[0].shape == (8, 8)
