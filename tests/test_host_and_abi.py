"""CPU-only checks: the C-ABI library loads and exports every declared symbol, host logic of the
config front end, and properties of the oracle that do not need golden files."""
import os
import re

import numpy as np
import pytest

from helpers import ROOT, master_equation_rhs, synthetic_cfg, synthetic_spec
from oracle.oracle import Oracle
from quandary_amd import capi, config


def test_library_exports_every_declared_symbol():
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = capi.load_library()
    header = open(os.path.join(ROOT, "include", "quandary_amd.h")).read()
    declared = set(re.findall(r"\b(qd_[a-z_A-Z0-9]+)\s*\(", header))
    assert declared == set(capi.EXPORTS)
    for s in capi.EXPORTS:
        assert hasattr(lib, s), s
    assert b"gfx950" in lib.qd_version()


def test_no_gpu_means_loud_failure():
    """The product has no CPU fallback: without a device qd_create must fail with QD_ERR_DEVICE."""
    lib = capi.load_library()
    if lib.qd_device_count() > 0:
        pytest.skip("a GPU is visible")
    sp = synthetic_spec([2, 2], lindblad=False, ntime=5)
    with pytest.raises(capi.QuandaryAmdError):
        capi.Handle(sp)


def test_config_parser_semantics():
    cfg = config.parse_config_text("# c\n// c\n a = 1 , 2\t,3 \n\nb=x\nb = y\n")
    assert cfg == {"a": "1,2,3", "b": "y"}


def test_random_initialisation_matches_std_mt19937():
    # first outputs of std::mt19937 seeded with 1234 (known answers of the MT19937 reference generator)
    rng = config.MT19937(1234)
    assert [rng.next_u32() for _ in range(3)] == [822569775, 2137449171, 2671936806]
    sp = synthetic_spec([2, 2], lindblad=False, ntime=5)
    a = 2 * np.pi * 0.005
    assert sp.params0.size == 2 * 2 * 2 * 10 and np.all(np.abs(sp.params0) <= a)
    # the engine is copied per oscillator: both oscillators draw the same stream
    np.testing.assert_array_equal(sp.params0[:40], sp.params0[40:])


@pytest.mark.parametrize("lindblad", [False, True])
def test_oracle_transpose_is_adjoint(lindblad):
    sp = synthetic_spec([3, 2, 2], lindblad=lindblad, jkl=0.02, detuned=True, ntime=5)
    orc = Oracle(sp)
    orc.set_params(sp.params0)
    rng = np.random.default_rng(7)
    x, y = rng.standard_normal((2, 2 * orc.dim))
    lhs = np.dot(orc.apply_rhs(0.02, x)[0], y)
    rhs = np.dot(x, orc.apply_rhs(0.02, y, transpose=True)[0])
    assert lhs == pytest.approx(rhs, rel=1e-13)
    orc.close()


@pytest.mark.parametrize("lindblad,linsolve,stepper", [(True, "neumann", "IMR"), (False, "gmres", "IMR"), (True, "gmres", "IMR4"),
                                                       (False, "gmres", "IMR8")])
def test_oracle_gradient_matches_finite_differences(lindblad, linsolve, stepper):
    # (ExplEuler is excluded: the reference's EE adjoint evaluates M and the control derivative at
    #  t_stop while the forward step uses t_start, src/timestepper.cpp:493-520, so it is not the exact
    #  discrete gradient; the oracle restates it as it is.)
    sp = synthetic_spec([2, 3], lindblad=lindblad, jkl=0.01, detuned=True, ntime=10, nspline=6, linsolve=linsolve, stepper=stepper,
                        penalties=True, maxiter=30)
    orc = Oracle(sp)
    _, g = orc.evalGradF(sp.params0)
    rng = np.random.default_rng(3)
    for i in rng.choice(sp.params0.size, 4, replace=False):
        e = np.zeros_like(sp.params0)
        e[i] = 1e-6
        fp = orc.evalF(sp.params0 + e)[0]["objective"]
        fm = orc.evalF(sp.params0 - e)[0]["objective"]
        assert (fp - fm) / 2e-6 == pytest.approx(g[i], rel=2e-5, abs=1e-9)
    orc.close()


@pytest.mark.parametrize("lindblad", [False, True])
def test_oracle_operator_is_the_master_equation(lindblad):
    """Independent of every golden file: the oracle's matrix-free operator equals the rotating-frame master equation
    built from Kronecker products of ladder operators (helpers.master_equation_rhs states the model)."""
    nl = [3, 2, 2]
    sp = synthetic_spec(nl, lindblad=lindblad, jkl=0.02, detuned=True, ntime=5)
    orc = Oracle(sp)
    orc.set_params(sp.params0)
    t = 0.02
    pq = orc.eval_controls(np.array([t]))[0]
    x = np.random.default_rng(1).standard_normal(2 * orc.dim)
    mx, dim = orc.apply_rhs(t, x)[0], orc.dim
    want = master_equation_rhs(sp, pq, t, x)
    np.testing.assert_allclose(mx[:dim] + 1j * mx[dim:], want, rtol=0, atol=1e-13 * np.abs(want).max())
    orc.close()


def _hermitian(n, nosc, seed):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    hc = []
    for _ in range(nosc):
        b = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
        hc.append(0.5 * (b + b.conj().T))
    return 0.3 * (a + a.conj().T), np.array(hc)


@pytest.mark.parametrize("lindblad", [False, True])
def test_oracle_user_hamiltonian_model(lindblad):
    """The oracle's dense user-Hamiltonian mode beyond the two golden cases: the operator equals the explicit
    Hilbert-space formula y = -i(H rho - rho H) (+ nothing else without dissipation), its transpose is the adjoint,
    and its gradient matches central differences."""
    sp = synthetic_spec([2, 3], lindblad=lindblad, ntime=10, nspline=5, penalties=True, target="pure", objective="Jfrobenius", dt=0.01)
    hsys, hc = _hermitian(6, 2, 3)
    sp.hamiltonian = (hsys, hc)
    orc = Oracle(sp)
    orc.set_params(sp.params0)
    rng = np.random.default_rng(1)
    x, y = rng.standard_normal((2, 2 * orc.dim))
    t = 0.03
    mx = orc.apply_rhs(t, x)[0]
    assert np.dot(mx, y) == pytest.approx(np.dot(x, orc.apply_rhs(t, y, transpose=True)[0]), rel=1e-12)
    pq = orc.eval_controls(np.array([t]))[0]  # [nosc][2]
    H = hsys + sum(pq[k, 0] * hc[k].real + 1j * pq[k, 1] * hc[k].imag for k in range(2))
    dim = orc.dim
    if lindblad:
        # no decay/dephasing contribution can be separated here, so compare the commutator part through a
        # system without dissipation: collapse_type stays "both", hence test the difference of two Hamiltonians
        sp2 = synthetic_spec([2, 3], lindblad=True, ntime=10, nspline=5, penalties=True, target="pure", objective="Jfrobenius", dt=0.01)
        sp2.hamiltonian = (np.zeros_like(hsys), None)
        orc2 = Oracle(sp2)
        orc2.set_params(sp2.params0)
        diss = orc2.apply_rhs(t, x)[0]
        orc2.close()
        rho = (x[:dim] + 1j * x[dim:]).reshape(6, 6).T  # column-major vec
        want = (-1j * (H @ rho - rho @ H)).T.reshape(-1)
        got = (mx - diss)[:dim] + 1j * (mx - diss)[dim:]
    else:
        psi = x[:dim] + 1j * x[dim:]
        want = -1j * (H @ psi)
        got = mx[:dim] + 1j * mx[dim:]
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-13)
    _, g = orc.evalGradF(sp.params0)
    for i in rng.choice(sp.params0.size, 4, replace=False):
        e = np.zeros_like(sp.params0)
        e[i] = 1e-6
        fd = (orc.evalF(sp.params0 + e)[0]["objective"] - orc.evalF(sp.params0 - e)[0]["objective"]) / 2e-6
        assert fd == pytest.approx(g[i], rel=2e-5, abs=1e-9)
    orc.close()


def test_hamiltonian_files_are_parsed_like_the_reference_reader():
    from helpers import load_case

    sp = load_case("hamiltonian-reader-lindblad")
    hsys, hc = sp.hamiltonian
    assert hsys.shape == (4, 4) and hc.shape == (2, 4, 4)
    np.testing.assert_allclose(hsys, hsys.conj().T, atol=1e-14)  # the golden system Hamiltonian is Hermitian
    assert np.abs(hc).max() > 0


def test_oracle_solvers_agree():
    vals = []
    for ls in ("gmres", "neumann"):
        sp = synthetic_spec([2, 2, 2], lindblad=True, ntime=20, linsolve=ls)
        orc = Oracle(sp)
        vals.append(orc.evalGradF(sp.params0))
        orc.close()
    assert vals[0][0]["objective"] == pytest.approx(vals[1][0]["objective"], rel=1e-9)
    np.testing.assert_allclose(vals[0][1], vals[1][1], rtol=1e-6, atol=1e-10)
