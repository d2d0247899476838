"""Every kernel family on systems whose oscillators and pairs all differ, under collapse_type decay, dephase and both.

helpers.synthetic_cfg gives every oscillator one self-Kerr, T1 and T2 and every pair one cross-Kerr (and, but for the coupled-column tests,
one J), and only ever asks for both dissipators or none: a kernel - or the host code that fills its tables, the row sums behind the
split iterations and the degree gate - that read xi_kl, gamma_1, gamma_2 or xi_k with the wrong pair or oscillator index, or that mixed
up the two dissipators, passes everything else in this suite.  Here every case takes its constants from helpers.unequal_constants (all
distinct; oscillator 1 of three or more does not decay at all); tests/test_unequal_constants_cpu.py shows that an exchanged pair of
them moves the operator by 1e-2 of its maximum, and that the oracle is right on such systems.  The sweeps are short, so their
fixtures are held to a condition of their own on the CPU (test_sweep_fixtures_see_exchanged_constants): the oracle's objective or
gradient moves by ten times the tolerance or more when two constants change places.

One table of cases.  A case names the family, the shape, the options or QD_VAR that force the family, and the kernel names
qd_last_kernel must report (or begin with): a case cannot quietly run on another family.  Per case:
  - the operator and its transpose against the oracle at 1e-13, and <M x, z> = <x, M^T z> on the device, under all three collapse types
    (cases that differ from another one only in the stepper or the solver share that one's operator check: operator=False);
  - evalGradF against the oracle - objective parts at REF_RTOL with the 1e-12 floor, gradient at 1e-8 of its norm; gmres requests through
    helpers.check_parity - under both, and under decay and dephase for one shape per family (partial=True).
12 steps of 0.001 ns (column shapes) or 0.01 ns, at most 8 initial conditions, every penalty on.  No tolerance is new: they are those of
tests/test_gpu_kernel_coverage.py, test_user_hamiltonian_operator_vs_oracle (dense) and test_gpu_f32mixed.py (APPLY_TOL)."""
from dataclasses import dataclass, field

import numpy as np
import pytest

from helpers import OBJ_KEYS, REF_RTOL, check_parity, col_kernels, synthetic_cfg, synthetic_spec, unequal_constants
from oracle.oracle import Oracle
from quandary_amd import capi, config, models
from test_gpu_coupled_column import colj_kernels
from test_gpu_f32mixed import APPLY_TOL

ROLES = ("forward", "adjoint", "apply")
COLLAPSES = ("decay", "dephase", "both")
STAND_INS = ("gmres_as_split", "gmres_as_neumann")
BASE = dict(lindblad=True, ntime=12, dt=0.01, penalties=True, ctrl_init="random, 0.02", target="pure", objective="Jfrobenius")


@dataclass
class Case:
    id: str
    family: str
    kw: dict                 # helpers.synthetic_spec arguments on top of BASE
    kernels: dict            # role -> what qd_last_kernel must begin with (a whole name where the instantiation is known)
    options: dict = field(default_factory=dict)   # qd_set_option
    env: dict = field(default_factory=dict)       # QD_VAR
    coupled: bool = True     # J on every pair (all distinct)
    zero_pair: int = None    # ... but this one
    precision: str = "f64"
    dense: bool = False      # the handle gets models.standard_hamiltonians of the spec, the oracle keeps its stencil
    operator: bool = True    # run the operator check
    sweep: bool = True       # run evalGradF
    partial: bool = False    # ... under decay and dephase as well
    solvers: tuple = None    # what qd_last_solver may report
    team: int = None         # workgroups per initial condition (global-memory kernels)

    @property
    def lindblad(self):
        return self.kw.get("lindblad", True)


def _var(q, lind, var, qubit):
    a = f"{q}, {'true' if lind else 'false'}, {var}, {'true' if qubit else 'false'}"
    return {"forward": f"k_forward<{a}, ", "adjoint": f"k_adjoint<{a}, ", "apply": f"k_apply<{a}>"}


def _big(q, lind, dense=False):
    a = f"{q}, {'true' if lind else 'false'}, {'true' if dense else 'false'}"
    return {"forward": f"k_forward_big<{a}, ", "adjoint": f"k_adjoint_big<{a}, ", "apply": f"k_apply_big<{a}>"}


def _q32(fwd, app):
    return {"forward": f"k_forward_q32<{fwd}>", "adjoint": f"k_adjoint_q32<{fwd}>", "apply": f"k_apply_q32<{app}>"}


SCHROEDINGER = dict(lindblad=False, objective="Jmeasure")


def _col_init(nlevels):
    """The diagonal states of the last oscillator where that is at most 8 initial conditions, else of the first."""
    return f"diagonal, {len(nlevels) - 1}" if nlevels[-1] <= 8 else "diagonal, 0"


COLUMN = dict(dt=0.001, target="gate", objective="Jtrace")

CASES = [
    # ---- general stencil, state in LDS, the kernel the library picks: one thread per element up to dim 64 (variant 0); several columns
    # of rho per wave for Lindblad systems of up to 32 rows with a level beyond the second (variant 14)
    Case("general-2x3x2-schroedinger-eta", "general", dict(nlevels=[2, 3, 2], init="diagonal, 0, 1", **SCHROEDINGER), _var(3, False, 0, False)),
    Case("general-3x3x2-lindblad-eta", "general", dict(nlevels=[3, 3, 2], init="diagonal, 0"), _var(3, True, 14, False), partial=True),
    Case("general-2x3x2x2-lindblad", "general", dict(nlevels=[2, 3, 2, 2], init="diagonal, 1", detuned=True), _var(4, True, 14, False)),
    Case("general-2x2x3x2x2-schroedinger", "general", dict(nlevels=[2, 2, 3, 2, 2], init="diagonal, 2", detuned=True, **SCHROEDINGER), _var(5, False, 0, False)),
    # ... and the layout with one workgroup thread per few elements that Lindblad systems of this size ran on before variant 14
    Case("general-3x3x2-lindblad-var2", "general", dict(nlevels=[3, 3, 2], init="diagonal, 0", detuned=True), _var(3, True, 2, False), env={"QD_VAR": "2"}),
    # ---- all-qubit stencil
    Case("qubit-2x2x2-lindblad-eta", "qubit", dict(nlevels=[2, 2, 2], init="diagonal, 0, 1, 2"), _var(3, True, 0, True), partial=True),
    Case("qubit-2^4-schroedinger", "qubit", dict(nlevels=[2] * 4, init="diagonal, 0, 1, 2", detuned=True, **SCHROEDINGER), _var(4, False, 0, True)),
    Case("qubit-2^6-schroedinger-15-pairs", "qubit", dict(nlevels=[2] * 6, init="diagonal, 0, 1, 2", detuned=True, **SCHROEDINGER), _var(6, False, 0, True)),
    # ---- lean slot kernels, fp64 (k_*_q32<Q, SB, R, GM, HJ>; the names: tests/test_gpu_kernel_coverage.py)
    Case("slot-2^4", "slot", dict(nlevels=[2] * 4, init="diagonal, 0, 1"), _q32("4, 0, double, false, false", "4, 0, double, false"), coupled=False, partial=True),
    Case("slot-2^4-krylov", "slot", dict(nlevels=[2] * 4, init="diagonal, 0, 1", linsolve="gmres"), _q32("4, 0, double, true, false", "4, 0, double, false"),
         options={"gmres_split": "0"}, coupled=False, operator=False, solvers=("krylov",)),
    Case("slot-2^4-J", "slot", dict(nlevels=[2] * 4, init="diagonal, 0, 1", detuned=True), _q32("4, 0, double, false, true", "4, 0, double, true")),
    Case("slot-2^4-J-krylov", "slot", dict(nlevels=[2] * 4, init="diagonal, 0, 1", detuned=True, linsolve="gmres"), _q32("4, 0, double, true, true", "4, 0, double, true"),
         options={"gmres_split": "0"}, operator=False, solvers=("krylov",)),
    Case("slot-2^5", "slot", dict(nlevels=[2] * 5, init="diagonal, 0, 1"), _q32("5, 2, double, false, false", "5, 2, double, false"), options={"lean64_sb": "2"},
         coupled=False),
    Case("slot-2^5-krylov", "slot", dict(nlevels=[2] * 5, init="diagonal, 0, 1", linsolve="gmres"), _q32("5, 2, double, true, false", "5, 2, double, false"),
         options={"gmres_split": "0", "lean64_sb": "2"}, coupled=False, operator=False, solvers=("krylov",)),
    Case("slot-2^5-J-eta", "slot", dict(nlevels=[2] * 5, init="diagonal, 0, 1"), _q32("5, 1, double, false, true", "5, 1, double, true"), partial=True),
    Case("slot-2^5-J-eta-krylov", "slot", dict(nlevels=[2] * 5, init="diagonal, 0, 1", linsolve="gmres"), _q32("5, 1, double, true, true", "5, 1, double, true"),
         options={"gmres_split": "0"}, operator=False, solvers=("krylov",)),
    # ... in fp32-mixed the operator application only (the sweep budgets of test_gpu_f32mixed.py were measured at ntime 1000)
    Case("slot-2^4-f32", "slot", dict(nlevels=[2] * 4, init="diagonal, 0, 1"), {"apply": "k_apply_q32<4, 0, float, false>"}, coupled=False, precision="f32mixed", sweep=False),
    Case("slot-2^4-J-f32", "slot", dict(nlevels=[2] * 4, init="diagonal, 0, 1"), {"apply": "k_apply_q32<4, 0, float, true>"}, precision="f32mixed", sweep=False),
    Case("slot-2^5-f32", "slot", dict(nlevels=[2] * 5, init="diagonal, 0, 1"), {"apply": "k_apply_q32<5, 2, float, false>"}, options={"lean64_sb": "2"}, coupled=False,
         precision="f32mixed", sweep=False),
    Case("slot-2^5-J-f32", "slot", dict(nlevels=[2] * 5, init="diagonal, 0, 1"), {"apply": "k_apply_q32<5, 1, float, true>"}, precision="f32mixed", sweep=False),
    # ---- column layouts of the general kernel: 3x3x3 with guard levels (COL_SHAPES[3] of test_gpu_parity.py)
    Case("column-layout-var9-3x3x3", "column-layout", dict(nlevels=[3, 3, 3], nessential=[2, 3, 2], init="diagonal, 1", detuned=True, target="gate", objective="Jtrace"),
         _var(3, True, 9, False), env={"QD_VAR": "9"}, partial=True),
    Case("column-layout-var14-3x3x3", "column-layout", dict(nlevels=[3, 3, 3], nessential=[2, 3, 2], init="diagonal, 1", detuned=True, target="gate", objective="Jtrace"),
         _var(3, True, 14, False), env={"QD_VAR": "14"}),
]

# ---- lean column kernels (k_*_col<Q, EPT, SPLIT, USLOT, SKIP, KRY>): five and eight columns per wave, both USLOT forms, two and three
# oscillators, under neumann_split 0 and 1, IMR and IMR4.  The real-drive frame and the phasor table of the forward sweep never touch
# these constants; the diagonal of the split iteration (SPLIT) is made of them.
for _nl in ([3, 20], [3, 3, 5], [2, 4, 8], [3, 3, 7]):
    for _stepper in ("IMR", "IMR4"):
        for _split in ("0", "1"):
            CASES.append(Case(f"col-{'x'.join(map(str, _nl))}-{_stepper}-split{_split}", "col", dict(nlevels=_nl, stepper=_stepper, init=_col_init(_nl), **COLUMN),
                              col_kernels(_nl, _split, _stepper), options={"neumann_split": _split}, coupled=False, operator=_stepper == "IMR",
                              partial=(_nl, _stepper, _split) == ([3, 3, 5], "IMR", "1")))
CASES += [
    Case("col-3x3x5-krylov", "col", dict(nlevels=[3, 3, 5], linsolve="gmres", init=_col_init([3, 3, 5]), **COLUMN), {r: col_kernels([3, 3, 5], krylov=True)[r] for r in ROLES[:2]},
         options={"gmres_split": "0"}, coupled=False, operator=False, solvers=("krylov",)),
    # the shipped default on a gmres request: a stand-in where its gate (row sums of these constants) holds, else the Krylov solver
    Case("col-3x20-gmres-auto", "col", dict(nlevels=[3, 20], linsolve="gmres", init=_col_init([3, 20]), **COLUMN), {"forward": "k_forward_col<2, 5, ", "adjoint": "k_adjoint_col<2, 5, "},
         options={"gmres_split": "auto"}, coupled=False, operator=False, solvers=STAND_INS + ("krylov",)),
]
# ---- coupled lean column kernels (k_*_colj): J on two pairs of three, none on pair (0, 2); frames that coincide and that differ
for _shape in ("3x3x5", "2x4x8"):
    for _detuned in (True, False):
        _nl = [int(n) for n in _shape.split("x")]
        CASES.append(Case(f"colj-{_shape}-{'eta0' if _detuned else 'eta'}", "colj", dict(nlevels=_nl, detuned=_detuned, init=_col_init(_nl), **COLUMN), colj_kernels(_shape), zero_pair=1,
                          partial=(_shape, _detuned) == ("3x3x5", False)))
CASES += [
    # ---- global-memory kernels: forced onto small systems (QD_VAR = 16), in a team of eight workgroups, and where they are the only choice
    Case("global-3x3x2-lindblad", "global", dict(nlevels=[3, 3, 2], init="diagonal, 0"), _big(3, True), env={"QD_VAR": "16"}, partial=True, team=1),
    Case("global-2x3x2-schroedinger", "global", dict(nlevels=[2, 3, 2], init="diagonal, 0, 1", **SCHROEDINGER), _big(3, False), env={"QD_VAR": "16"}, team=1),
    Case("global-3x3x2-lindblad-team8", "global", dict(nlevels=[3, 3, 2], init="diagonal, 0"), _big(3, True), env={"QD_VAR": "16"}, options={"big_team": "8"},
         operator=False, team=8),
    Case("global-3^4-lindblad-dim6561", "global", dict(nlevels=[3] * 4, nessential=[2] * 4, init="pure, 1, 0, 1, 0", detuned=True, target="gate", objective="Jtrace",
                                                        ntime=4, nspline=5), {"apply": _big(4, True)["apply"]}, sweep=False),
    # ---- dense user Hamiltonians: the standard model of the same constants as matrices (models.standard_hamiltonians) on the dense
    # kernels, against the stencil oracle; the dissipators stay the handle's, so T1 and T2 are read on this path too
    Case("dense-3x3x3-lindblad-N27", "dense", dict(nlevels=[3, 3, 3], init="diagonal, 2", detuned=True, dt=0.004, target="gate", objective="Jtrace"), _var(3, True, 17, False), dense=True, partial=True),
    Case("dense-2x3x2-schroedinger", "dense", dict(nlevels=[2, 3, 2], init="diagonal, 0, 1", detuned=True, dt=0.004, **SCHROEDINGER), _var(3, False, 11, False), dense=True),
]
BY_ID = {c.id: c for c in CASES}


def test_case_table_is_complete():
    """Every family is there, every one has a shape of three or more oscillators whose sweep also runs under decay and dephase, and
    every case states the kernels of the roles it runs."""
    assert len(BY_ID) == len(CASES)
    for family in ("general", "qubit", "slot", "column-layout", "col", "colj", "global", "dense"):
        mine = [c for c in CASES if c.family == family]
        assert any(c.partial and c.sweep and c.lindblad and len(c.kw["nlevels"]) >= 3 for c in mine), family
    for c in CASES:
        want = (set(ROLES[:2]) if c.sweep else set()) | ({"apply"} if c.operator else set())
        assert want <= set(c.kernels) and want, c.id


def _kwargs(case, collapse):
    kw = {**BASE, **case.kw, **unequal_constants(len(case.kw["nlevels"]), coupled=case.coupled, zero_pair=case.zero_pair)}
    if case.lindblad:
        kw["collapse"] = collapse
    return kw


def _open(case, collapse, monkeypatch):
    """(spec, handle, oracle) of a case; the oracle first, so that it keeps the stencil where the handle gets matrices."""
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    sp = synthetic_spec(**_kwargs(case, collapse))
    sp.options = dict(case.options)
    orc = Oracle(sp)
    if case.dense:
        sp.hamiltonian = models.standard_hamiltonians(sp)
    if case.precision != "f64":
        sp.precision = case.precision
    return sp, capi.Handle(sp), orc


_references = {}


def _reference(case, collapse):
    """The oracle's evalGradF at params0, computed once per system (the config text names it: options, QD_VAR and the dense form of the
    Hamiltonian do not reach the oracle) and shared by the cases that run it on different kernels."""
    text = synthetic_cfg(**_kwargs(case, collapse))
    if text not in _references:
        sp = config.build_spec(config.parse_config_text(text))
        orc = Oracle(sp)
        _references[text] = orc.evalGradF(sp.params0)
        orc.close()
    return _references[text]


def _exchanges(case):
    """(keyword, i, j): the pairs of constants whose exchange a sweep of this system must see."""
    nl = case.kw["nlevels"]
    Q, npairs = len(nl), len(nl) * (len(nl) - 1) // 2
    out = [("crosskerr", 0, npairs - 1)]
    if case.lindblad:
        out += [("dephase_time", 0, Q - 1), ("decay_time", 0, Q - 1)]
    deep = [k for k in range(Q) if nl[k] >= 3]
    if len(deep) >= 2:
        out.append(("selfkerr", deep[0], deep[-1]))
    return out


def _sweep_systems():
    """One case per system of three or more oscillators that a sweep runs on: the first of those that differ only in stepper or solver."""
    seen = {}
    for c in CASES:
        if c.sweep and len(c.kw["nlevels"]) >= 3:
            seen.setdefault(synthetic_cfg(**{**_kwargs(c, "both"), "stepper": "IMR", "linsolve": "neumann"}), c)
    return list(seen.values())


@pytest.mark.parametrize("case", _sweep_systems(), ids=lambda c: c.id)
def test_sweep_fixtures_see_exchanged_constants(case):
    """A condition on the inputs, checked with the oracle on the CPU: a system on which two pairs exchanged their cross-Kerr constants, or
    two oscillators their T1, T2 or self-Kerr constants, has an objective or a gradient at least ten times the tolerance of
    test_sweeps_with_unequal_constants away - on twelve short steps that takes initial states and an objective chosen for it (the
    lean column cases: diagonal states of the last oscillator, a gate target and Jtrace)."""
    kw = _kwargs(case, "both")
    oval, og = _reference(case, "both")
    for key, i, j in _exchanges(case):
        values = list(kw[key])
        values[i], values[j] = values[j], values[i]
        sp = synthetic_spec(**{**kw, key: values})
        orc = Oracle(sp)
        val, g = orc.evalGradF(sp.params0)
        orc.close()
        dg = np.linalg.norm(g - og) / np.linalg.norm(og)
        dj = max(abs(val[k] - oval[k]) / max(abs(oval[k]), 1e-12 / REF_RTOL) for k in OBJ_KEYS)
        print(f"{case.id}: {key} of {i} and {j} exchanged moves the gradient by {dg:.1e} of its norm, an objective part by {dj:.1e}")
        assert dg >= 10 * 1e-8 or dj >= 10 * REF_RTOL, key


def _runs(flag):
    """(case, collapse) for the cases with case.<flag>: all three collapse types for the operator, `both` and - for partial cases -
    decay and dephase for the sweep; a Schroedinger system has no collapse type and runs once."""
    out = []
    for c in CASES:
        if not getattr(c, flag):
            continue
        for collapse in COLLAPSES if c.lindblad and (flag == "operator" or c.partial) else ("both",):
            out.append(pytest.param(c, collapse, id=f"{c.id}-{collapse if c.lindblad else 'none'}"))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case,collapse", _runs("operator"))
def test_operator_with_unequal_constants(case, collapse, monkeypatch):
    sp, h, orc = _open(case, collapse, monkeypatch)
    h.set_params(sp.params0)
    orc.set_params(sp.params0)
    rng = np.random.default_rng(17)
    x, z = rng.standard_normal((2, 2, 2 * h.dim))
    t = 0.41 * sp.time.ntime * sp.time.dt
    for tr in (False, True):
        y, yo = h.apply_rhs(t, x, transpose=tr), orc.apply_rhs(t, x, transpose=tr)
        name = h.last_kernel("apply")
        err = np.abs(y - yo).max() / np.abs(yo).max()
        print(f"{case.id} {collapse} transpose={tr}: {name}, max |y - oracle| / max |oracle| = {err:.3e}")
        assert name.startswith(case.kernels["apply"]), (name, case.kernels["apply"])
        if case.precision != "f64":
            assert np.abs(y - yo).max() <= APPLY_TOL * np.abs(yo).max(), tr
        elif case.dense:
            np.testing.assert_allclose(y, yo, rtol=1e-12, atol=1e-12 * np.abs(yo).max())
        else:
            np.testing.assert_allclose(y, yo, rtol=1e-13, atol=1e-13 * np.abs(yo).max())
    # <M x, z> = <x, M^T z> on the device alone
    mx, mtz = h.apply_rhs(t, x), h.apply_rhs(t, z, transpose=True)
    lhs, rhs = np.sum(mx * z), np.sum(x * mtz)
    print(f"<Mx, z> - <x, M^T z> = {lhs - rhs:.3e} of {np.linalg.norm(mx) * np.linalg.norm(z):.3e}")
    if case.dense:
        assert lhs == pytest.approx(rhs, rel=1e-11)
    else:
        assert abs(lhs - rhs) <= (1e-13 if case.precision == "f64" else APPLY_TOL) * np.linalg.norm(mx) * np.linalg.norm(z), (lhs, rhs)
    h.close(); orc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case,collapse", _runs("sweep"))
def test_sweeps_with_unequal_constants(case, collapse, monkeypatch):
    sp, h, orc = _open(case, collapse, monkeypatch)
    orc.close()
    opt = capi.Optim(h, sp)
    assert opt.ninit <= 8
    if case.team is not None and opt.ninit * case.team > 256:  # (members dealt over all XCDs: one slot per initial condition)
        opt.close(); h.close()
        pytest.skip("these teams would not be resident together")
    val, g = opt.evalGradF(sp.params0)
    names = h.last_kernel("forward"), h.last_kernel("adjoint")
    oval, og = _reference(case, collapse)
    rel = np.linalg.norm(g - og) / np.linalg.norm(og)
    print(f"{case.id} {collapse}: {names[0]} / {names[1]} ({h.last_solver}), objective {val['objective']:.12e} (oracle {oval['objective']:.12e}), "
          f"|g - oracle| / |oracle| = {rel:.3e}")
    assert names[0].startswith(case.kernels["forward"]) and names[1].startswith(case.kernels["adjoint"]), (names, case.kernels)
    if case.solvers is not None:
        assert h.last_solver in case.solvers, h.last_solver
    if case.team is not None:
        assert h.last_team == case.team
    if sp.solver.linsolve == capi.LINSOLVE["gmres"]:
        check_parity(sp, val, g, oval, og, msg=case.id)
    else:
        for k in OBJ_KEYS:
            assert val[k] == pytest.approx(oval[k], rel=REF_RTOL, abs=1e-12), k
        assert np.linalg.norm(g - og) <= 1e-8 * np.linalg.norm(og)
    opt.close(); h.close()


# ---- the SETS twins (qd_optim_evalGradF_batch): two control vectors in one launch ----------------------------------------------------------
SETS = [
    pytest.param(dict(nlevels=[2, 3, 2], init="diagonal, 0, 1"), {}, ("k_forward<3, true, ", "k_adjoint<3, true, "), ", true>", id="general-2x3x2-lindblad"),
    pytest.param(dict(nlevels=[2] * 4, init="diagonal, 0, 1", detuned=True), {"batch_lean": "1"}, ("k_forward_q32_sets<4, ", "k_adjoint_q32_sets<4, "), ", true>", id="slot-2^4-J"),
    pytest.param(dict(nlevels=[3, 3, 5], init="diagonal, 2", **COLUMN), {"batch_lean": "1", "col_slices": "1"}, ("k_forward_col_sets<3, 5, ", "k_adjoint_col_sets<3, 5, "), ">", id="col-3x3x5"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("kw,options,prefixes,suffix", SETS)
def test_parameter_set_batch_with_unequal_constants(kw, options, prefixes, suffix):
    """Each set of a two-set launch is bit for bit its single evaluation, and agrees with the oracle."""
    sp = synthetic_spec(**{**BASE, **kw, **unequal_constants(len(kw["nlevels"]), coupled="_col_" not in prefixes[0])})
    sp.options = dict(options)
    rng = np.random.default_rng(2718)
    alphas = np.stack([amp * rng.uniform(-1.0, 1.0, sp.params0.size) for amp in (0.02, 0.1)])
    orc = Oracle(sp)
    ref = [orc.evalGradF(a) for a in alphas]
    orc.close()
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    assert opt.ninit <= 8
    vals, grads = opt.evalGradF_batch(alphas)
    names = h.last_kernel("forward"), h.last_kernel("adjoint")
    print(names)
    assert opt.last_batch_sets == 2
    for name, prefix in zip(names, prefixes):
        assert name.startswith(prefix) and name.endswith(suffix), name
        assert "_sets<" in name or name.count(",") == 6, name  # (the general kernels: SETS = true is the seventh template argument)
    for j in range(2):
        v1, g1 = opt.evalGradF(alphas[j])
        assert "_sets<" not in h.last_kernel("forward") and h.last_kernel("forward").count(",") < 6
        print(j, vals[j]["objective"], ref[j][0]["objective"], np.linalg.norm(grads[j] - g1), np.linalg.norm(grads[j] - ref[j][1]) / np.linalg.norm(ref[j][1]))
        assert all(vals[j][k] == v1[k] for k in OBJ_KEYS) and np.array_equal(grads[j], g1), j
        check_parity(sp, vals[j], grads[j], *ref[j], alpha=alphas[j], msg=j)
    assert not np.allclose(grads[0], grads[1], rtol=1e-3)
    opt.close(); h.close()
