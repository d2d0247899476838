"""The premise of the paired forward sweep (option pair_hermitian), on the CPU oracle alone: the Lindblad step is complex-linear on
vec(rho) and maps Hermitian to Hermitian, so one propagation of X = A + i B carries two Hermitian states, A(t) = (X + X^dagger) / 2
and B(t) = (X - X^dagger) / 2i."""
import numpy as np
import pytest

from helpers import synthetic_spec
from oracle.oracle import Oracle

NSTEPS = 6


def _basis_state(N, k, j):
    """The reference's basis initial condition B_kj as (u, v) of vec(rho), column-major: element (r, c) at r + c N."""
    rho = np.zeros((N, N), dtype=complex)
    if k == j:
        rho[k, k] = 1.0
    elif k < j:
        rho[k, k] = rho[j, j] = 0.5
        rho[k, j] = rho[j, k] = 0.5
    else:
        rho[k, k] = rho[j, j] = 0.5
        rho[k, j] = -0.5j
        rho[j, k] = 0.5j
    return rho


def _vec(rho):
    f = rho.flatten(order="F")
    return np.concatenate([f.real, f.imag])


def _mat(x, N):
    return (x[: N * N] + 1j * x[N * N:]).reshape(N, N, order="F")


@pytest.mark.parametrize("kw,pairs", [
    (dict(nlevels=[3, 20]), [((0, 1), (1, 0)), ((2, 2), (21, 40))]),
    (dict(nlevels=[4, 12], nessential=[3, 11]), [((13, 0), (0, 25)), ((1, 1), (12, 1))]),
], ids=["3x20", "4x12-guard"])
def test_two_hermitian_states_travel_as_one_complex_state(kw, pairs):
    sp = synthetic_spec(**kw, lindblad=True, target="pure", objective="Jmeasure", init="basis, 0", ntime=NSTEPS, dt=0.001, penalties=True)
    N = int(np.prod(kw["nlevels"]))
    orc = Oracle(sp)
    orc.set_params(sp.params0)
    assert np.abs(orc.eval_controls((np.arange(NSTEPS) + 0.5) * sp.time.dt)).max() > 0  # controls on
    for (ka, ja), (kb, jb) in pairs:
        A, B = _basis_state(N, ka, ja), _basis_state(N, kb, jb)
        xa, xb, xx = _vec(A), _vec(B), _vec(A + 1j * B)
        for n in range(NSTEPS):
            t0, t1 = n * sp.time.dt, (n + 1) * sp.time.dt
            xa, xb, xx = orc.step_fwd(t0, t1, xa), orc.step_fwd(t0, t1, xb), orc.step_fwd(t0, t1, xx)
        X = _mat(xx, N)
        Ah, Bh = 0.5 * (X + X.conj().T), (X - X.conj().T) / 2j
        # (the oracle's own stopping error, about abstol per step, sets the bound: 1e-9 of the state norm)
        ea, eb = np.linalg.norm(Ah - _mat(xa, N)), np.linalg.norm(Bh - _mat(xb, N))
        print((ka, ja), (kb, jb), ea / np.linalg.norm(xa), eb / np.linalg.norm(xb))
        assert ea < 1e-9 * np.linalg.norm(xa) and eb < 1e-9 * np.linalg.norm(xb)
        # ... and the diagonals the in-loop penalties read are the real and imaginary parts of X's
        assert np.abs(np.diag(X).real - np.diag(_mat(xa, N)).real).max() < 1e-9 * np.linalg.norm(xa)
        assert np.abs(np.diag(X).imag - np.diag(_mat(xb, N)).real).max() < 1e-9 * np.linalg.norm(xb)
    orc.close()
