"""Which kernel instantiation every test runs on, stated rather than inferred.

The lean column kernels (qd_col.hip: k_{forward,adjoint}_col<Q, EPT, SPLIT, USLOT, SKIP, KRY>, k_apply_col<Q, EPT, SPLIT>) and the slot
kernels (qd_q32.hip: k_{forward,adjoint}_q32<Q, SB, R, GM, HJ>, k_apply_q32<Q, SB, R, HJ>, k_apply_mfma32) are picked at run time by host
code from the shape, the layout, the stepper, the solver, the batch and the precision.  The manifest below names, for every instantiation
the library contains, a case that launches it: either a CASE run here - a small synthetic system against the oracle, with the kernel it
ran checked through qd_last_kernel - or an existing test that asserts the same names (PINNED).  An instantiation no selectable input
reaches belongs in UNREACHABLE with the reason.  The completeness test reads the names out of libquandary_amd.so on the CPU: a kernel
added without a case, or a case that no longer holds a kernel of its own, fails there without a GPU."""
import os
import re
import shutil
import subprocess
from dataclasses import dataclass, field

import numpy as np
import pytest

from helpers import OBJ_KEYS, REF_RTOL, check_parity, col_kernels, synthetic_spec
from quandary_amd import capi

# the fp32-mixed budgets of tests/test_gpu_f32mixed.py (measured at ntime 1000)
from test_gpu_f32mixed import APPLY_TOL, FID_ATOL, GRAD_TOL, OBJ_RTOL

ROLES = ("forward", "adjoint", "apply")


@dataclass
class Case:
    id: str
    kw: dict            # helpers.synthetic_spec arguments
    options: dict       # qd_set_option
    kernels: dict       # role -> instantiation this case must launch
    precision: str = "f64"


def _col(id, nlevels, stepper="IMR", split="0", krylov=False, **extra):
    """A lean column case: a Lindblad system of 33..64 rows, controls of 0.02 on every oscillator, a short fine time grid."""
    kw = {**dict(nlevels=nlevels, lindblad=True, target="pure", objective="Jfrobenius", init="diagonal, 0", ntime=16, dt=0.001,
                 stepper=stepper, linsolve="gmres" if krylov else "neumann", ctrl_init="random, 0.02", penalties=True), **extra}
    opts = {"gmres_split": "0"} if krylov else {"neumann_split": split}
    k = col_kernels(nlevels, split, stepper, krylov)
    if krylov:  # (the operator application does not depend on the solver: the stationary cases hold it)
        del k["apply"]
    return Case(id, kw, opts, k)


def _slot(id, q, jkl=0.0, krylov=False, sb=None, precision="f64", fwd=None, app=None, **extra):
    kw = {**dict(nlevels=[2] * q, lindblad=True, init="diagonal, 0, 1", ntime=12, dt=0.01, jkl=jkl, linsolve="gmres" if krylov else "neumann",
                 ctrl_init="random, 0.02", penalties=True), **extra}
    opts = {"gmres_split": "0"} if krylov else {}
    if sb is not None:
        opts["lean64_sb"] = sb
    k = {"forward": "k_forward_q32<" + fwd + ">", "adjoint": "k_adjoint_q32<" + fwd + ">"}
    if app:
        k["apply"] = "k_apply_q32<" + app + ">"
    return Case(id, kw, opts, k, precision)


CASES = [
    # three oscillators, 61..64 rows: eight columns per wave.  2x4x8: strides 32 and 8 - the columns of a wave share the level indices
    # of the first two oscillators (USLOT); 4x4x4 (stride 4) and 3x3x7 (N = 63) do not.
    _col("2x4x8-IMR-split0", [2, 4, 8], "IMR", "0"),
    _col("2x4x8-IMR-split1", [2, 4, 8], "IMR", "1"),
    _col("2x4x8-IMR4-split0", [2, 4, 8], "IMR4", "0"),
    _col("2x4x8-IMR4-split1", [2, 4, 8], "IMR4", "1"),
    _col("2x4x8-krylov", [2, 4, 8], krylov=True),
    _col("4x4x4-IMR-split0", [4, 4, 4], "IMR", "0"),
    _col("4x4x4-IMR4-split1", [4, 4, 4], "IMR4", "1"),
    _col("3x3x7-IMR-split1", [3, 3, 7], "IMR", "1"),
    _col("3x3x7-IMR4-split0", [3, 3, 7], "IMR4", "0"),
    # the Krylov kernels of the layouts without USLOT (the USLOT ones and 4x4x4: test_lean_column_krylov_solver and its restarts)
    _col("4x12-krylov", [4, 12], krylov=True),
    _col("7x9-krylov", [7, 9], krylov=True),
    _col("2x4x7-krylov", [2, 4, 7], krylov=True),
    # fp64 slot kernels (2^4: one element per thread; 2^5: two (SB = 1, batches of at most one state per CU, the coupled stencil) or
    # four (SB = 2) elements; GM = the Krylov solver; HJ = dipole-dipole coupling)
    _slot("q4", 4, fwd="4, 0, double, false, false", app="4, 0, double, false"),
    _slot("q4-krylov", 4, krylov=True, fwd="4, 0, double, true, false"),
    _slot("q4-J", 4, jkl=0.004, fwd="4, 0, double, false, true", app="4, 0, double, true"),
    _slot("q4-J-krylov", 4, jkl=0.004, krylov=True, fwd="4, 0, double, true, true"),
    _slot("q5-sb1", 5, sb=1, fwd="5, 1, double, false, false"),
    _slot("q5-sb2", 5, sb=2, fwd="5, 2, double, false, false", app="5, 2, double, false"),
    _slot("q5-krylov", 5, krylov=True, fwd="5, 2, double, true, false"),
    _slot("q5-J", 5, jkl=0.004, fwd="5, 1, double, false, true", app="5, 1, double, true"),
    _slot("q5-J-krylov", 5, jkl=0.004, krylov=True, fwd="5, 1, double, true, true"),
    # BASELINE config 5 (2^5 fp32-mixed, more than 256 initial conditions per handle: four elements per thread), with lean64_sb = 2
    # standing in for the batch; the budgets of test_gpu_f32mixed.py hold at the ntime they were measured for
    _slot("q5-f32-sb2", 5, sb=2, precision="f32mixed", fwd="5, 2, float, false, false", app="5, 2, float, false", ntime=1000, nspline=30, init="diagonal, 0",
          ctrl_init="random, 0.005", penalties=False),
]


@dataclass
class Pinned:
    test: str           # the test that launches these and asserts them through Handle.last_kernel
    kernels: set = field(default_factory=set)


def _col_all(nlevels):
    """Every stationary kernel of a column layout - test_lean_column_kernels runs it under neumann_split 0 and 1, IMR and IMR4."""
    return {k for s in ("0", "1") for st in ("IMR", "IMR4") for k in col_kernels(nlevels, s, st).values()}


def _q32(role, args):
    return f"k_{role}_q32<{args}>"


PINNED = [
    Pinned("test_gpu_parity.py::test_lean_column_kernels[*-3x20]", _col_all([3, 20])),
    Pinned("test_gpu_parity.py::test_lean_column_kernels[*-4x12-guard]", _col_all([4, 12])),
    Pinned("test_gpu_parity.py::test_lean_column_kernels[*-8x8-N64]", _col_all([8, 8])),
    Pinned("test_gpu_parity.py::test_lean_column_kernels[*-7x9-N63]", _col_all([7, 9])),
    Pinned("test_gpu_parity.py::test_lean_column_kernels[*-3x3x5-N45]", _col_all([3, 3, 5])),
    Pinned("test_gpu_parity.py::test_lean_column_kernels[*-2x4x7-N56]", _col_all([2, 4, 7])),
    Pinned("test_gpu_parity.py::test_lean_column_krylov_solver[3x20-*]", {col_kernels([3, 20], krylov=True)[r] for r in ROLES[:2]}),
    Pinned("test_gpu_parity.py::test_lean_column_krylov_solver[3x3x5-N45-*]", {col_kernels([3, 3, 5], krylov=True)[r] for r in ROLES[:2]}),
    Pinned("test_gpu_parity.py::test_lean_column_krylov_solver[4x4x4-guard-eight-columns-*]", {col_kernels([4, 4, 4], krylov=True)[r] for r in ROLES[:2]}),
    Pinned("test_gpu_parity.py::test_lean_column_krylov_solver_restarts[8x8-N64-*]", {col_kernels([8, 8], krylov=True)[r] for r in ROLES[:2]}),
    Pinned("test_gpu_f32mixed.py::test_f32_operator_application", {_q32("apply", f"{q}, 0, float, false") for q in (3, 4)} | {_q32("apply", "5, 2, float, false")}),
    Pinned("test_gpu_f32mixed.py::test_f32_objective_and_gradient_budget_ntime1000",
           {_q32(r, a) for r in ROLES[:2] for a in ("3, 0, float, false, false", "4, 0, float, false, false", "5, 1, float, false, false")}),
    Pinned("test_gpu_f32mixed.py::test_f32_gmres_objective_and_gradient_budget_ntime1000[*-gmres-krylov]",
           {_q32(r, a) for r in ROLES[:2] for a in ("3, 0, float, true, false", "4, 0, float, true, false", "5, 2, float, true, false")}),
    Pinned("test_gpu_f32mixed.py::test_f32_coupled_operator_application", {_q32("apply", "4, 0, float, true"), _q32("apply", "5, 1, float, true")}),
    Pinned("test_gpu_f32mixed.py::test_f32_coupled_objective_and_gradient_budget_ntime1000",
           {_q32(r, a) for r in ROLES[:2] for a in ("4, 0, float, false, true", "5, 1, float, false, true")}),
    Pinned("test_gpu_f32mixed.py::test_mfma_f32_dense_product_vs_stencil", {"k_apply_mfma32"}),
]

# instantiation -> why no selectable input launches it (removing it from the build is a change of its own)
UNREACHABLE = {}

KERNEL_RE = re.compile(r"k_(?:forward|adjoint|apply)_(?:col|q32)<[^>]*>|k_apply_mfma32")


def _entries():
    return [(c.id, set(c.kernels.values())) for c in CASES] + [(p.test, set(p.kernels)) for p in PINNED]


def library_kernels():
    """The lean column and slot kernel instantiations libquandary_amd.so contains (nm -C; built first if missing)."""
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-C", capi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    return set(KERNEL_RE.findall(out))


def test_every_instantiation_has_a_case():
    built = library_kernels()
    assert len(built) == 134, len(built)  # 88 column, 45 slot, 1 MFMA
    assert sum("_col<" in n for n in built) == 88 and sum("_q32<" in n for n in built) == 45
    declared = set().union(*(k for _, k in _entries())) | set(UNREACHABLE)
    assert not declared - built, ("declared but not in the library", sorted(declared - built))
    assert not built - declared, ("in the library without a case", sorted(built - declared))
    assert not set(UNREACHABLE) & set().union(*(k for _, k in _entries())), "an UNREACHABLE kernel is launched by a case"


def test_every_case_holds_a_kernel_of_its_own():
    """No case is redundant: deleting any one of them leaves a kernel without a case (and fails the test above)."""
    entries = _entries()
    assert len({n for n, _ in entries}) == len(entries)
    for i, (name, ks) in enumerate(entries):
        others = set().union(*(k for j, (_, k) in enumerate(entries) if j != i))
        assert ks - others, name


def test_column_cases_follow_the_dispatch_rule():
    """The column names of the manifest, spelled out for the 61..64-row layouts the suite did not reach before."""
    by_id = {c.id: c.kernels for c in CASES}
    assert by_id["2x4x8-IMR-split0"]["forward"] == "k_forward_col<3, 8, false, true, true, false>"
    assert by_id["2x4x8-krylov"]["adjoint"] == "k_adjoint_col<3, 8, true, true, false, true>"
    assert by_id["4x4x4-IMR4-split1"]["forward"] == "k_forward_col<3, 8, true, false, false, false>"
    assert by_id["3x3x7-IMR-split1"]["apply"] == "k_apply_col<3, 8, true>"
    assert by_id["4x12-krylov"]["forward"] == "k_forward_col<2, 5, true, false, false, true>"


def _check_apply(h, orc, case):
    rng = np.random.default_rng(17)
    x = rng.standard_normal((2, 2 * h.dim))
    t = 0.41 * case.kw["ntime"] * case.kw["dt"]
    for tr in (False, True):
        y, yo = h.apply_rhs(t, x, transpose=tr), orc.apply_rhs(t, x, transpose=tr)
        assert h.last_kernel("apply") == case.kernels["apply"]
        if case.precision == "f64":
            np.testing.assert_allclose(y, yo, rtol=1e-13, atol=1e-13 * np.abs(yo).max())
        else:
            assert np.abs(y - yo).max() <= APPLY_TOL * np.abs(yo).max(), tr
    # <M x, z> = <x, M^T z> on the device alone
    z = rng.standard_normal((2, 2 * h.dim))
    mx, mtz = h.apply_rhs(t, x), h.apply_rhs(t, z, transpose=True)
    lhs, rhs = np.sum(mx * z), np.sum(x * mtz)
    tol = 1e-13 if case.precision == "f64" else APPLY_TOL
    assert abs(lhs - rhs) <= tol * np.linalg.norm(mx) * np.linalg.norm(z), (lhs, rhs)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_case_launches_its_kernels_and_matches_the_oracle(case):
    from oracle.oracle import Oracle
    sp = synthetic_spec(**case.kw)
    sp.options = dict(case.options)
    orc = Oracle(sp)
    if case.precision != "f64":
        sp.precision = case.precision
    h = capi.Handle(sp)
    assert [h.last_kernel(r) for r in ROLES] == ["", "", ""]
    h.set_params(sp.params0)
    orc.set_params(sp.params0)
    if "apply" in case.kernels:
        _check_apply(h, orc, case)
    opt = capi.Optim(h, sp)
    val, g = opt.evalGradF(sp.params0)
    for r in ("forward", "adjoint"):
        assert h.last_kernel(r) == case.kernels[r], r
    if "krylov" in case.id:
        assert h.last_solver == "krylov"
    oval, og = orc.evalGradF(sp.params0)
    if case.precision == "f64":
        if sp.solver.linsolve == capi.LINSOLVE["gmres"]:
            check_parity(sp, val, g, oval, og, msg=case.id)
        else:
            for k in OBJ_KEYS:
                assert val[k] == pytest.approx(oval[k], rel=REF_RTOL, abs=1e-12), k
            assert np.linalg.norm(g - og) <= 1e-8 * np.linalg.norm(og)
    else:
        assert abs(val["objective"] - oval["objective"]) <= OBJ_RTOL * abs(oval["objective"])
        assert abs(val["fidelity"] - oval["fidelity"]) <= FID_ATOL
        assert np.linalg.norm(g - og) <= GRAD_TOL * np.linalg.norm(og)
    opt.close(); h.close(); orc.close()
