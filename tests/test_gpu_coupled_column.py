"""The lean column kernels for systems with dipole-dipole coupling (qd_colj.hip: k_{forward,adjoint}_colj<Q, EPT, SPLIT, USLOT, SKIP, KRY>,
k_apply_colj<Q, EPT, SPLIT>).

What is built: Q in {2, 3}, five (N <= 60) or eight columns per wave, both USLOT forms, SPLIT = true only, SKIP = false only, the stationary
iteration and the Krylov solver, one operator application per (Q, EPT): 36 kernels.  The selection rule (qd_handle::col_sweep,
collean_available): a coupled Lindblad system of 44..64 rows with two or three oscillators runs on them; a coupled sweep that asks for the
plain Neumann iteration (neumann_split = 0), coupled systems below 44 rows, Schroedinger systems and the option no_collean stay on the
kernels they ran on before.

The manifest names, for every instantiation the library contains, the shape that launches it; the CPU test compares it with `nm -C` in
both directions.  The GPU tests run every shape against the oracle with a different J on every pair, with rotating frames that differ
(eta != 0: sine and cosine terms, time dependent) and that coincide (eta = 0: the cosine term only)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from helpers import OBJ_KEYS, REF_RTOL, check_parity, synthetic_spec
from quandary_amd import capi

ROLES = ("forward", "adjoint", "apply")
COLJ_RE = re.compile(r"k_(?:forward|adjoint|apply)_colj<[^>]*>")

# shape -> (columns per wave, USLOT); all have N >= 44
SHAPES = {
    "3x20": ([3, 20], 5, True),
    "4x12": ([4, 12], 5, False),
    "8x8": ([8, 8], 8, True),
    "7x9": ([7, 9], 8, False),      # N = 63: an idle lane and an idle column
    "3x3x5": ([3, 3, 5], 5, True),  # three pairs
    "2x4x7": ([2, 4, 7], 5, False),
    "2x4x8": ([2, 4, 8], 8, True),
    "3x3x7": ([3, 3, 7], 8, False),  # N = 63, three pairs
}


def _b(v):
    return "true" if v else "false"


def colj_kernels(shape, krylov=False):
    """The instantiations a coupled system of this shape runs on, per role, as qd_last_kernel spells them."""
    nl, ept, uslot = SHAPES[shape]
    args = f"{len(nl)}, {ept}, true, {_b(uslot)}, false, {_b(krylov)}"
    return {"forward": f"k_forward_colj<{args}>", "adjoint": f"k_adjoint_colj<{args}>", "apply": f"k_apply_colj<{len(nl)}, {ept}, true>"}


def _manifest():
    m = {}
    for shape in SHAPES:
        for kry in (False, True):
            for role, name in colj_kernels(shape, kry).items():
                m.setdefault(name, []).append(f"{shape}-{'krylov' if kry else 'stationary'}-{role}")
    return m


def test_manifest_follows_the_dispatch_rule():
    """The names of the manifest re-derived from the shapes: five columns per wave up to N = 60, eight above; USLOT where N and the strides
    of all oscillators but the last are multiples of the column count."""
    for shape, (nl, ept, uslot) in SHAPES.items():
        N = int(np.prod(nl))
        assert N >= 44 and ept == (5 if N <= 60 else 8), shape
        post = [int(np.prod(nl[k + 1:])) for k in range(len(nl))]
        assert uslot == (N % ept == 0 and all(p % ept == 0 for p in post[:-1])), shape
    assert colj_kernels("3x20")["forward"] == "k_forward_colj<2, 5, true, true, false, false>"
    assert colj_kernels("3x3x7", krylov=True)["adjoint"] == "k_adjoint_colj<3, 8, true, false, false, true>"


def test_library_contains_the_coupled_column_kernels():
    """Every coupled column kernel in libquandary_amd.so is launched by a shape below, and every kernel the shapes name is built."""
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-C", capi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    built, declared = set(COLJ_RE.findall(out)), set(_manifest())
    assert not declared - built, ("declared but not in the library", sorted(declared - built))
    assert not built - declared, ("in the library without a case", sorted(built - declared))
    assert len(built) == 36 and len(built) <= 40


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------------
def _spec(shape, detuned, stepper="IMR", linsolve="neumann", zero_pair=None, jkl=0.004, nlevels=None, **extra):
    """A coupled Lindblad system in the manner of the _col cases of test_gpu_kernel_coverage.py: controls of 0.02, a short fine time grid,
    every penalty on; J_kl = 0.004 (1 + 0.37 pair), so that a mixed-up pair index shows."""
    nl = nlevels if nlevels is not None else SHAPES[shape][0]
    kw = {**dict(nlevels=nl, lindblad=True, target="pure", objective="Jfrobenius", init="diagonal, 0", ntime=12, dt=0.001, stepper=stepper,
                 linsolve=linsolve, ctrl_init="random, 0.02", penalties=True, jkl=jkl, detuned=detuned), **extra}
    sp = synthetic_spec(**kw)
    for i in range(len(nl) * (len(nl) - 1) // 2):
        sp.system.Jkl[i] *= 1.0 + 0.37 * i
    if zero_pair is not None:
        sp.system.Jkl[zero_pair] = 0.0
    return sp


def _check_apply(h, orc, sp, kernel):
    """As _check_apply of test_gpu_kernel_coverage.py: operator and transpose at 1e-13 against the oracle, <M x, z> = <x, M^T z> on the device."""
    rng = np.random.default_rng(17)
    x = rng.standard_normal((2, 2 * h.dim))
    t = 0.41 * sp.time.ntime * sp.time.dt
    for tr in (False, True):
        y, yo = h.apply_rhs(t, x, transpose=tr), orc.apply_rhs(t, x, transpose=tr)
        assert h.last_kernel("apply") == kernel
        err = np.abs(y - yo).max() / np.abs(yo).max()
        print(f"apply transpose={tr}: max |y - oracle| / max |oracle| = {err:.3e}")
        np.testing.assert_allclose(y, yo, rtol=1e-13, atol=1e-13 * np.abs(yo).max())
    z = rng.standard_normal((2, 2 * h.dim))
    mx, mtz = h.apply_rhs(t, x), h.apply_rhs(t, z, transpose=True)
    lhs, rhs = np.sum(mx * z), np.sum(x * mtz)
    assert abs(lhs - rhs) <= 1e-13 * np.linalg.norm(mx) * np.linalg.norm(z), (lhs, rhs)


def _check_eval(sp, val, g, oval, og, msg):
    """Neumann request: objective parts at REF_RTOL, gradient at 1e-8 of its norm.  gmres request: check_parity."""
    rel = np.linalg.norm(g - og) / np.linalg.norm(og)
    print(f"{msg}: objective {val['objective']:.12e} (oracle {oval['objective']:.12e}), |g - oracle| / |oracle| = {rel:.3e}")
    if sp.solver.linsolve == capi.LINSOLVE["gmres"]:
        return check_parity(sp, val, g, oval, og, msg=msg)
    for k in OBJ_KEYS:
        assert val[k] == pytest.approx(oval[k], rel=REF_RTOL, abs=1e-12), (k, msg)
    assert np.linalg.norm(g - og) <= 1e-8 * np.linalg.norm(og), msg
    return "plain"


def _is_general(name):
    return re.match(r"k_(forward|adjoint|apply)<", name) is not None


@pytest.mark.gpu
@pytest.mark.parametrize("detuned", [True, False], ids=["eta0", "eta"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_coupled_operator_application(shape, detuned):
    from oracle.oracle import Oracle
    sp = _spec(shape, detuned)
    h, orc = capi.Handle(sp), Oracle(sp)
    h.set_params(sp.params0)
    orc.set_params(sp.params0)
    _check_apply(h, orc, sp, colj_kernels(shape)["apply"])
    h.close(); orc.close()


# (linearsolver_type, gmres_split, the solver the handle reports, Krylov kernels)
SOLVER_FORMS = [pytest.param(("neumann", None, "neumann", False), id="neumann"),
                pytest.param(("gmres", "auto", None, False), id="gmres"),
                pytest.param(("gmres", "0", "krylov", True), id="gmres-krylov")]


@pytest.mark.gpu
@pytest.mark.parametrize("form", SOLVER_FORMS)
@pytest.mark.parametrize("stepper", ["IMR", "IMR4"])
@pytest.mark.parametrize("detuned", [True, False], ids=["eta0", "eta"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_coupled_sweeps_against_the_oracle_and_the_general_kernel(shape, detuned, stepper, form):
    """evalGradF with every penalty on the coupled kernels: against the oracle, and against the same evaluation under no_collean = 1 (the
    general column kernel: the path these systems ran on before), which is held to the same tolerances and names a general kernel."""
    from oracle.oracle import Oracle
    linsolve, mode, solver, krylov = form
    sp = _spec(shape, detuned, stepper, linsolve)
    sp.options = {} if mode is None else {"gmres_split": mode}
    orc = Oracle(sp)
    oval, og = orc.evalGradF(sp.params0)
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    val, g = opt.evalGradF(sp.params0)
    if mode == "auto":  # (served by the diagonal-split iteration where its gate holds, else by the Krylov kernels: both are coupled kernels)
        krylov = h.last_solver == "krylov"
    k = colj_kernels(shape, krylov)
    assert (h.last_kernel("forward"), h.last_kernel("adjoint")) == (k["forward"], k["adjoint"]), h.last_solver
    if solver is not None:
        assert h.last_solver == solver
    _check_eval(sp, val, g, oval, og, (shape, detuned, stepper, form))
    opt.close(); h.close()
    # A/B: the general column kernel on the same request
    sp.options = {**sp.options, "no_collean": "1"}
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    val0, g0 = opt.evalGradF(sp.params0)
    assert _is_general(h.last_kernel("forward")) and _is_general(h.last_kernel("adjoint")), (h.last_kernel("forward"), h.last_kernel("adjoint"))
    _check_eval(sp, val0, g0, oval, og, (shape, detuned, stepper, form, "no_collean"))
    for k in OBJ_KEYS:  # ... and the two paths against each other
        assert val[k] == pytest.approx(val0[k], rel=REF_RTOL, abs=1e-12), k
    assert np.linalg.norm(g - g0) <= 1e-8 * np.linalg.norm(g0)
    opt.close(); h.close(); orc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("zero_pair", [0, 1, 2])
@pytest.mark.parametrize("shape", ["3x3x5", "2x4x7"])
def test_one_uncoupled_pair_among_coupled_ones(shape, zero_pair):
    """Three oscillators with J = 0 on one pair: its weights vanish, the other two pairs keep their own J."""
    from oracle.oracle import Oracle
    sp = _spec(shape, False, zero_pair=zero_pair)
    h, orc = capi.Handle(sp), Oracle(sp)
    h.set_params(sp.params0)
    orc.set_params(sp.params0)
    _check_apply(h, orc, sp, colj_kernels(shape)["apply"])
    opt = capi.Optim(h, sp)
    val, g = opt.evalGradF(sp.params0)
    assert h.last_kernel("forward") == colj_kernels(shape)["forward"]
    oval, og = orc.evalGradF(sp.params0)
    _check_eval(sp, val, g, oval, og, (shape, zero_pair))
    opt.close(); h.close(); orc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("linsolve,mode", [("neumann", None), ("gmres", "0")], ids=["neumann", "gmres-krylov"])
@pytest.mark.parametrize("slices", [1, 3])
def test_coupled_sweeps_time_sliced(slices, linsolve, mode):
    """The sliced scheduler (col_slices) with the coupled kernels."""
    from oracle.oracle import Oracle
    sp = _spec("3x20", False, linsolve=linsolve, ntime=16)
    sp.options = {"col_slices": slices, **({} if mode is None else {"gmres_split": mode})}
    h, orc = capi.Handle(sp), Oracle(sp)
    opt = capi.Optim(h, sp)
    val, g = opt.evalGradF(sp.params0)
    k = colj_kernels("3x20", krylov=mode == "0")
    assert (h.last_kernel("forward"), h.last_kernel("adjoint")) == (k["forward"], k["adjoint"])
    oval, og = orc.evalGradF(sp.params0)
    _check_eval(sp, val, g, oval, og, ("3x20", slices, linsolve))
    opt.close(); h.close(); orc.close()


@pytest.mark.gpu
def test_requests_the_coupled_kernels_do_not_serve():
    """The boundaries of the selection: what the built set does not cover, and what it must not touch."""
    def kernels(sp, apply=True):
        h = capi.Handle(sp)
        opt = capi.Optim(h, sp)
        opt.evalGradF(sp.params0)
        out = [h.last_kernel("forward"), h.last_kernel("adjoint")]
        if apply:
            h.apply_rhs(0.004, np.ones((1, 2 * h.dim)))
            out.append(h.last_kernel("apply"))
        opt.close(); h.close()
        return out

    # neumann_split = 0 on a coupled system: SPLIT = false is not built - the general column kernel, as before
    sp = _spec("3x20", False)
    sp.options = {"neumann_split": "0"}
    fwd, adj = kernels(sp, apply=False)
    assert _is_general(fwd) and _is_general(adj), (fwd, adj)
    # ... while the Krylov kernels (always the split form) serve the same option
    sp = _spec("3x20", False, linsolve="gmres")
    sp.options = {"neumann_split": "0", "gmres_split": "0"}
    assert kernels(sp, apply=False) == [colj_kernels("3x20", True)[r] for r in ROLES[:2]]
    # a coupled system of 40 rows: below 44 rows nothing moves
    for name in kernels(_spec(None, False, nlevels=[5, 2, 4])):
        assert _is_general(name), name
    # a coupled Schroedinger system
    for name in kernels(_spec(None, False, nlevels=[3, 20], lindblad=False)):
        assert "col" not in name, name
    # the uncoupled 3 x 20 keeps its kernels
    fwd, adj, app = kernels(_spec("3x20", False, jkl=0.0))
    assert fwd.startswith("k_forward_col<2, 5, ") and adj.startswith("k_adjoint_col<2, 5, ") and app.startswith("k_apply_col<2, 5, "), (fwd, adj, app)
    # explicit Euler never runs on the lean kernels; one operator application does
    sp = _spec("3x20", False, stepper="EE")
    fwd, adj, app = kernels(sp)
    assert _is_general(fwd) and _is_general(adj) and app == colj_kernels("3x20")["apply"], (fwd, adj, app)
