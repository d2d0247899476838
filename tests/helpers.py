"""Shared helpers for the parity tests (golden-file readers, synthetic systems)."""
import json
import os

import numpy as np
import pytest

from quandary_amd import config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
# tolerance of the reference's own regression harness (tests/regression/regression_test.py:14-15)
REF_RTOL, REF_ATOL = 1e-7, 1e-15

# gmres_split settings every gmres parity test runs under: "auto" = the shipped default (requests served by a stationary iteration where
# it provably contracts fast), "0" = the Krylov kernels (the oracle's own iteration path)
GMRES_MODES = ["auto", "0"]
# (linearsolver_type, gmres_split) pairs for tests parametrised over the solver
SOLVERS = [pytest.param(("neumann", None), id="neumann"), pytest.param(("gmres", "auto"), id="gmres"),
           pytest.param(("gmres", "0"), id="gmres-krylov")]


def with_gmres_mode(sp, mode):
    """Set the gmres_split option on a spec (applied by capi.Handle through qd_set_option); None leaves the default."""
    if mode is not None:
        sp.options = {**(getattr(sp, "options", None) or {}), "gmres_split": mode}
    return sp


HIST_COLS = ["iter", "objective", "gnorm", "ls_step", "fidelity", "cost", "regul", "penalty", "penalty_dpdm",
             "penalty_energy", "penalty_variation"]


def load_case(case):
    return config.load(os.path.join(GOLDEN, case, case + ".cfg"))


def golden_history(case, row=0):
    rows = [l.split() for l in open(os.path.join(GOLDEN, case, "base", "optim_history.dat")) if not l.startswith("#")]
    return dict(zip(HIST_COLS, [float(v) for v in rows[row]]))


def golden_grad(case):
    return np.loadtxt(os.path.join(GOLDEN, case, "base", "grad.dat"))


_manifest = None


def golden_rows(case, fname):
    """(row indices into the full output file, data without the time column)."""
    global _manifest
    if _manifest is None:
        _manifest = json.load(open(os.path.join(GOLDEN, "manifest.json")))
    m = _manifest[f"{case}/base/{fname}"]
    d = np.loadtxt(os.path.join(GOLDEN, case, "base", fname), ndmin=2)
    rows = list(range(0, m["nrows_full"], m["row_stride"]))
    if m["last_row_appended"]:
        rows.append(m["nrows_full"] - 1)
    return rows, d[:, 0], d[:, 1:]


def synthetic_cfg(nlevels, lindblad=True, ntime=20, dt=0.01, nspline=10, jkl=0.0, linsolve="neumann", stepper="IMR",
                  init="basis", target="gate", objective="Jtrace", nessential=None, maxiter=20, penalties=False,
                  detuned=False, gate=None, segments=None, carrier="0.0, -0.2", ctrl_init="random, 0.005", enforce_bc=False,
                  selfkerr=None, crosskerr=None, decay_time=None, dephase_time=None, jkl_pairs=None, collapse="both"):
    """Synthetic systems in the style of SURVEY 8(d) / tests/performance/configs of the reference.

    selfkerr, decay_time, dephase_time (one entry per oscillator), crosskerr, jkl_pairs (one entry per pair, in the order (0,1), (0,2), ...,
    (1,2), ...; jkl_pairs replaces jkl) and collapse ("both" | "decay" | "dephase", Lindblad systems only) override the constants every
    oscillator and pair shares by default (unequal_constants); without them the text is what it always was."""
    Q = len(nlevels)
    assert collapse in ("both", "decay", "dephase"), collapse

    def csv(values, default):
        return default if values is None else ",".join(repr(float(v)) for v in values)
    lines = [
        "nlevels = " + ",".join(str(n) for n in nlevels),
        f"ntime = {ntime}", f"dt = {dt}",
        "transfreq = " + ",".join(f"{4.1 + 0.1 * k:.4f}" for k in range(Q)),
        "rotfreq = " + (",".join(["4.1"] * Q) if detuned else ",".join(f"{4.1 + 0.1 * k:.4f}" for k in range(Q))),
        "selfkerr = " + csv(selfkerr, ",".join(["0.2"] * Q)),
        "crosskerr = " + csv(crosskerr, "0.001"), "Jkl = " + csv(jkl_pairs, f"{jkl}"),
        "collapse_type = " + (collapse if lindblad else "none"),
        "decay_time = " + csv(decay_time, ",".join(["80.0"] * Q)), "dephase_time = " + csv(dephase_time, ",".join(["26.0"] * Q)),
        f"initialcondition = {init}",
        "control_enforceBC = " + ("true" if enforce_bc else "false"),
        f"optim_objective = {objective}", "optim_regul = 1e-4",
        f"linearsolver_type = {linsolve}", f"linearsolver_maxiter = {maxiter}", f"timestepper = {stepper}",
        "rand_seed = 1234", "usematfree = true", "runtype = gradient",
    ]
    if nessential:
        lines.append("nessential = " + ",".join(str(n) for n in nessential))
    for k in range(Q):
        seg = f"spline, {nspline}" if segments is None else segments if isinstance(segments, str) else segments[k]
        ini = ctrl_init if isinstance(ctrl_init, str) else ctrl_init[k]
        lines += [f"control_segments{k} = {seg}", f"control_initialization{k} = {ini}", f"carrier_frequency{k} = {carrier}"]
    if target == "gate":
        dim_ess = int(np.prod(nessential if nessential else nlevels))
        lines.append("optim_target = gate, " + (gate if gate else "cnot" if dim_ess == 4 else ("xgate" if dim_ess == 2 else "qft")))
    else:
        lines.append("optim_target = pure, " + ",".join(["0"] * Q))
    if penalties:
        lines += ["optim_penalty = 0.3", "optim_penalty_param = 0.5", "optim_penalty_energy = 0.1"]
        if not lindblad:
            lines.append("optim_penalty_dpdm = 0.01")
    else:
        lines += ["optim_penalty = 0.0", "optim_penalty_energy = 0.0", "optim_penalty_dpdm = 0.0"]
    lines.append("optim_penalty_variation = 0.0")
    return "\n".join(lines) + "\n"


def synthetic_spec(*args, **kw):
    return config.build_spec(config.parse_config_text(synthetic_cfg(*args, **kw)))


def unequal_constants(Q, coupled=True, zero_pair=None):
    """synthetic_cfg keywords that give every oscillator and every pair constants of its own, so that a kernel (or the host code that
    fills its tables) reading them with the wrong oscillator or pair index computes something else: self-Kerr 0.2 + 0.07 k, T1 =
    80 / (1 + 0.6 k), T2 = 26 / (1 + 0.45 k), cross-Kerr 0.05 (1 + 0.41 i), J = 0.02 (1 + 0.37 i) for oscillator k and pair i.  From
    three oscillators on, oscillator 1 does not decay (decay_time = 0: no L1 term for it in a system that decays elsewhere).
    coupled=False leaves J to the caller's jkl; zero_pair names one pair with J = 0 among the coupled ones."""
    npairs = Q * (Q - 1) // 2
    kw = dict(selfkerr=[0.2 + 0.07 * k for k in range(Q)],
              decay_time=[0.0 if (k == 1 and Q >= 3) else 80.0 / (1.0 + 0.6 * k) for k in range(Q)],
              dephase_time=[26.0 / (1.0 + 0.45 * k) for k in range(Q)],
              crosskerr=[0.05 * (1.0 + 0.41 * i) for i in range(npairs)])
    if coupled:
        kw["jkl_pairs"] = [0.0 if i == zero_pair else 0.02 * (1.0 + 0.37 * i) for i in range(npairs)]
    return kw


def master_equation_rhs(sp, pq, t, x, transpose=False):
    """The right-hand side of the rotating-frame master equation of spec `sp` at time t, applied to x = [Re; Im] (Lindblad: the
    column-major vec of rho, src/util.cpp:150), from Kronecker products of ladder operators and nothing else (docs/mkdocs/user_guide.md,
    model section):
      H_d = sum_k (w_k - w_k^rot) n_k - xi_k/2 a^+a^+aa - sum_kl xi_kl n_k n_l
            + sum_kl J_kl [cos(eta t)(a_k^+ a_l + a_k a_l^+) + i sin(eta t)(a_k^+ a_l - a_k a_l^+)],  eta = w_k^rot - w_l^rot
      H_c = sum_k p_k (a_k + a_k^+) + i q_k (a_k - a_k^+),   L_1k = a_k / sqrt(T1_k),  L_2k = n_k / sqrt(T2_k)
    with pq[k] = (p_k, q_k).  L_1k enters under collapse_type decay / both and L_2k under dephase / both, each only where its time is
    above 1e-14 (src/mastereq.cpp:14-60).  transpose: the dense real matrix M of the operator, column by column from unit vectors, and
    M^T x - for systems of a few hundred elements."""
    from quandary_amd import capi
    nl, sy = list(sp.nlevels), sp.system
    Q, N, tw = len(nl), int(np.prod(nl)), 2 * np.pi
    lindblad = sy.lindblad_type != capi.LINDBLAD["none"]
    dim = N * N if lindblad else N
    a = []
    for k in range(Q):
        op = np.array([[1.0 + 0j]])
        for m in range(Q):
            op = np.kron(op, np.diag(np.sqrt(np.arange(1, nl[m])), 1) if m == k else np.eye(nl[m]))
        a.append(op)
    dag = lambda m: m.conj().T
    H = np.zeros((N, N), complex)
    pair = 0
    for k in range(Q):
        nk = dag(a[k]) @ a[k]
        H += tw * (sy.transfreq[k] - sy.rotfreq[k]) * nk - tw * sy.selfkerr[k] / 2 * (nk @ nk - nk)
        for l in range(k + 1, Q):
            eta, J = tw * (sy.rotfreq[k] - sy.rotfreq[l]), tw * sy.Jkl[pair]
            H -= tw * sy.crosskerr[pair] * nk @ (dag(a[l]) @ a[l])
            H += J * (np.cos(eta * t) * (dag(a[k]) @ a[l] + a[k] @ dag(a[l])) + 1j * np.sin(eta * t) * (dag(a[k]) @ a[l] - a[k] @ dag(a[l])))
            pair += 1
        H += pq[k][0] * (a[k] + dag(a[k])) + 1j * pq[k][1] * (a[k] - dag(a[k]))
    collapse = []
    if lindblad:
        for k in range(Q):
            if sy.lindblad_type in (capi.LINDBLAD["decay"], capi.LINDBLAD["both"]) and sy.decay_time[k] > 1e-14:
                collapse.append(a[k] / np.sqrt(sy.decay_time[k]))
            if sy.lindblad_type in (capi.LINDBLAD["dephase"], capi.LINDBLAD["both"]) and sy.dephase_time[k] > 1e-14:
                collapse.append(dag(a[k]) @ a[k] / np.sqrt(sy.dephase_time[k]))
    LdL = [dag(L) @ L for L in collapse]

    def apply(v):
        if not lindblad:
            return -1j * (H @ (v[:dim] + 1j * v[dim:]))
        rho = (v[:dim] + 1j * v[dim:]).reshape(N, N).T
        y = -1j * (H @ rho - rho @ H)
        for L, ll in zip(collapse, LdL):
            y += L @ rho @ dag(L) - 0.5 * (ll @ rho + rho @ ll)
        return y.T.reshape(-1)

    x = np.asarray(x, dtype=float)
    if not transpose:
        return apply(x)
    M = np.empty((2 * dim, 2 * dim))
    e = np.zeros(2 * dim)
    for j in range(2 * dim):
        e[j] = 1.0
        col = apply(e)
        M[:dim, j], M[dim:, j] = col.real, col.imag
        e[j] = 0.0
    y = M.T @ x
    return y[:dim] + 1j * y[dim:]


# ---- parity of whole evaluations against the oracle -------------------------------------------------------------------------------------
OBJ_KEYS = ["objective", "fidelity", "cost", "regul", "penalty", "penalty_dpdm", "penalty_energy", "penalty_variation"]


def tight_oracle(sp):
    """The oracle on the same problem with every linear system solved to round-off (GMRES, abstol 1e-14, no iteration cap that matters):
    the exact solution of the discrete equations, up to fp64."""
    from oracle.oracle import Oracle
    from quandary_amd import capi
    keep = (sp.solver.abstol, sp.solver.maxiter, sp.solver.linsolve)
    sp.solver.abstol, sp.solver.maxiter, sp.solver.linsolve = 1e-14, 200, capi.LINSOLVE["gmres"]
    try:
        return Oracle(sp)  # (qo_create copies the solver block)
    finally:
        sp.solver.abstol, sp.solver.maxiter, sp.solver.linsolve = keep


def check_parity(sp, val, g, oval, og, alpha=None, obj_abs=1e-12, grad_abs=1e-13, msg=None, any_solver=False):
    """Objective parts at the reference harness tolerance (rtol 1e-7), gradient at 1e-8 of its norm against the oracle.

    A gmres request may miss that by the ORACLE's own stopping error: both sides stop at residual <= abstol = 1e-10 per linear system
    (src/timestepper.cpp:535-550), which over a long time grid or on a tiny gradient norm exceeds 1e-8 relative.  Such an evaluation is then
    held against the exact discrete solution (tight_oracle) instead and must be no farther from it than the reference-tolerance oracle is -
    factor 1.25 (classical against modified Gram-Schmidt stop at slightly different points of the same method) plus 1 % of abstol - and
    its deviation from the oracle must itself be of the order of abstol.  Returns "plain" or "stopping-error" (which of the two applied).
    any_solver (the wide sweeps of profiles/seed_sweep_all.py): the same criterion for a Neumann request - the reference's Neumann iteration
    stops on an update norm <= abstol as well (src/timestepper.cpp:713-720), and on gradient norms of 1e-5 its own distance from the exact
    discrete solution (1e-12 ... 1e-11) exceeds 1e-8 relative (profiles/r4_neumann_marginal_probe.txt)."""
    plain = all(val[k] == pytest.approx(oval[k], rel=REF_RTOL, abs=obj_abs) for k in OBJ_KEYS)
    if g is not None:
        plain = plain and np.linalg.norm(g - og) <= 1e-8 * np.linalg.norm(og) + grad_abs
    if plain:
        return "plain"
    from quandary_amd import capi
    assert any_solver or sp.solver.linsolve == capi.LINSOLVE["gmres"], ("beyond the tolerance without a gmres request", msg)
    tight = tight_oracle(sp)
    a = sp.params0 if alpha is None else alpha
    if g is not None:
        tval, tg = tight.evalGradF(a)
    else:
        tval, tg = tight.evalF(a)[0], None
    tight.close()
    for k in OBJ_KEYS:
        assert abs(val[k] - tval[k]) <= 1.25 * abs(oval[k] - tval[k]) + 1e-12 * max(1.0, abs(tval[k])), (k, msg)
        assert val[k] == pytest.approx(oval[k], rel=10 * REF_RTOL, abs=1e-9), (k, msg)
    if g is not None:
        assert np.linalg.norm(g - tg) <= 1.25 * np.linalg.norm(og - tg) + 1e-12, msg
        assert np.linalg.norm(g - og) <= 1e-8 * np.linalg.norm(og) + 5e-10, msg
    return "stopping-error"


# ---- which kernel instantiation a sweep runs on (qd_last_kernel) -------------------------------------------------------------------------
def _b(v):
    return "true" if v else "false"


def col_kernels(nlevels, split="0", stepper="IMR", krylov=False):
    """The lean column kernels (qd_col.hip) a Lindblad system of 33 <= N <= 64 rows runs on, as qd_last_kernel names them, per role.
    The dispatch rule of QD_COL_DISPATCH / col_uslot / col_sweep / col_apply (qd_col.h): five columns per wave up to N = 60, eight above; USLOT where N and the
    strides of all oscillators but the last are multiples of it; SPLIT from the option neumann_split ("auto" is on for these ladders; the
    operator application takes SPLIT only from neumann_split = 1); SKIP on the one-stage implicit midpoint rule with reltol = 0 (the
    synthetic systems: 1e-20); the Krylov kernels (gmres_split = 0) are always SPLIT and never SKIP."""
    N, Q = int(np.prod(nlevels)), len(nlevels)
    ept = 5 if N <= 60 else 8
    post = [int(np.prod(nlevels[k + 1:])) for k in range(Q)]
    uslot = N % ept == 0 and all(p % ept == 0 for p in post[:-1])
    sw_split, skip = (True, False) if krylov else (split != "0", stepper == "IMR")
    args = f"{Q}, {ept}, {_b(sw_split)}, {_b(uslot)}, {_b(skip)}, {_b(krylov)}"
    return {"forward": f"k_forward_col<{args}>", "adjoint": f"k_adjoint_col<{args}>", "apply": f"k_apply_col<{Q}, {ept}, {_b(split == '1')}>"}
