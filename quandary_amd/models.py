"""Dense matrices of the standard Hamiltonian model, for the entry points that take user-supplied Hamiltonians.

standard_hamiltonians(spec) writes the rotating-frame model of a spec's qd_system block - detuning, self-Kerr, cross-Kerr and
dipole-dipole terms, ladder-operator controls - as the matrices Handle.set_hamiltonian and
Optim.evalGradF_ensemble take.  A spec with sp.hamiltonian = standard_hamiltonians(sp) describes the same system as the spec itself; what
it buys is the ensemble: sample transfreq, crosskerr or Jkl, build one Hsys per sample, and evaluate one control vector on all of them
in shared sweep launches (risk-neutral control).
"""
import numpy as np


def _lift(op, k, nlevels):
    """op on oscillator k, identity elsewhere; oscillator 0 is the slowest index of a Hilbert-space index."""
    out = np.eye(1)
    for j, n in enumerate(nlevels):
        out = np.kron(out, op if j == k else np.eye(n))
    return out


def standard_hamiltonians(spec):
    """(hsys complex [N, N], hc complex [nosc, N, N]) in rad/ns, in the convention of qd_set_hamiltonian:

        H(t) = Hsys + sum_k p_k(t) Re(Hc_k) + i q_k(t) Im(Hc_k),

        Hsys = sum_k delta_k n_k - xi_k / 2 n_k (n_k - 1) - sum_{k<l} xi_kl n_k n_l + sum_{k<l} J_kl (a_k^+ a_l + a_k a_l^+),
        Hc_k = (a_k + a_k^+) + i (a_k - a_k^+),

    with delta_k = 2 pi (transfreq_k - rotfreq_k), xi_k = 2 pi selfkerr_k, xi_kl = 2 pi crosskerr_kl, J_kl = 2 pi Jkl_kl and the pairs in
    the order 01, 02, ..., 0(Q-1), 12, ...  A pair with J_kl != 0 whose rotation frequencies differ has the time-dependent coupling
    J_kl (cos(eta t) (a_k^+ a_l + a_k a_l^+) + i sin(eta t) (a_k^+ a_l - a_k a_l^+)), eta = 2 pi (rotfreq_k - rotfreq_l): no constant
    Hsys describes it, and the spec is rejected with ValueError.
    """
    s = spec.system
    Q = int(s.nosc)
    nlevels = [int(s.nlevels[k]) for k in range(Q)]
    N = int(np.prod(nlevels))
    two_pi = 2.0 * np.pi
    lower = [_lift(np.diag(np.sqrt(np.arange(1.0, n)), 1), k, nlevels) for k, n in enumerate(nlevels)]  # a_k
    number = [_lift(np.diag(np.arange(float(n))), k, nlevels) for k, n in enumerate(nlevels)]           # n_k = a_k^+ a_k
    eye = np.eye(N)
    hsys = np.zeros((N, N), dtype=complex)
    for k in range(Q):
        hsys += two_pi * (s.transfreq[k] - s.rotfreq[k]) * number[k]
        hsys -= two_pi * s.selfkerr[k] / 2.0 * (number[k] @ (number[k] - eye))
    pair = 0
    for k in range(Q):
        for l in range(k + 1, Q):
            hsys -= two_pi * s.crosskerr[pair] * (number[k] @ number[l])
            J = two_pi * s.Jkl[pair]
            if abs(J) > 1e-10:  # (the threshold below which the model drops the coupling)
                if s.rotfreq[k] != s.rotfreq[l]:
                    raise ValueError(f"standard_hamiltonians: oscillators {k} and {l} are coupled (Jkl = {s.Jkl[pair]}) and rotate at different "
                                     f"frequencies ({s.rotfreq[k]}, {s.rotfreq[l]}): the coupling is time-dependent, no constant Hsys exists")
                hsys += J * (lower[k].T @ lower[l] + lower[k] @ lower[l].T)
            pair += 1
    hc = np.array([(a + a.T) + 1j * (a - a.T) for a in lower], dtype=complex).reshape(Q, N, N)
    return hsys, hc
