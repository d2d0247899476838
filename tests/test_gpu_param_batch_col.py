"""Parameter-set batch on the lean column kernels (option batch_lean = 1): the batch entry points share one sweep launch on the lean
column family (Lindblad, two or three oscillators, 33..64 rows: qd_col.h) where the kernel's solver is a stationary iteration - a neumann
request, or a gmres request served by the stand-in.  Those launches run on k_*_col_sets / k_*_colj_sets, which read one control table per
set; qd_last_kernel names them with the six template arguments of the kernel the single evaluation runs on.  A Krylov plan, and every
plan without the option, goes set by set as before.

Every system is synthetic (helpers.synthetic_spec: 12 steps of 0.001 ns, every Lindblad penalty) with at most 8 initial conditions per
set.  The four control vectors of a case come from a seeded generator with amplitudes 3 to 10 times apart, set 2 a copy of set 0: a set
that read another set's control table cannot pass, and with four sets over three initial conditions neither can a kernel that divides
the state number by the wrong count.  Each set is held bit for bit against the single evaluation on the same handle and against the CPU
oracle through helpers.check_parity: no new tolerance appears here.
"""
import numpy as np
import pytest

from helpers import OBJ_KEYS, check_parity, synthetic_spec
from oracle.oracle import Oracle
from quandary_amd import capi

pytestmark = pytest.mark.gpu

LEAN = {"batch_lean": "1", "col_slices": "1"}
AMPS = (0.01, 0.05, 0.01, 0.1)  # rad/ns


def _spec(nlevels, options=LEAN, ntime=12, **kw):
    kw = {**dict(lindblad=True, target="pure", objective="Jmeasure", init="diagonal, 0", ntime=ntime, dt=0.001, penalties=True), **kw}
    sp = synthetic_spec(nlevels, **kw)
    for i in range(len(sp.system.Jkl)):  # (coupled systems: pairs that differ, so that a mixed-up pair column shows)
        sp.system.Jkl[i] *= 1.0 + 0.37 * i
    sp.options = dict(options)
    return sp


def _alphas(sp, seed):
    """One control vector per amplitude (uniform in +-amp); set 2 is a copy of set 0."""
    rng = np.random.default_rng(seed)
    a = np.stack([amp * rng.uniform(-1.0, 1.0, sp.params0.size) for amp in AMPS])
    a[2] = a[0]
    return a


def _oracle(sp, alphas):
    orc = Oracle(sp)
    out = [orc.evalGradF(a) for a in alphas]
    orc.close()
    return out


def _kernels(h):
    return h.last_kernel("forward"), h.last_kernel("adjoint")


def _sets_names(plain):
    """The SETS twins of the plain kernels a single evaluation reported: the same template arguments under the _sets name."""
    for n in plain:
        assert "_sets<" not in n and ("_col<" in n or "_colj<" in n), n
    return tuple(n.replace("_col<", "_col_sets<").replace("_colj<", "_colj_sets<") for n in plain)


def _same_eval(a, b):
    (va, ga), (vb, gb) = a, b
    return all(va[k] == vb[k] for k in OBJ_KEYS) and np.array_equal(ga, gb)


def _batch_against_singles_and_oracle(sp, alphas, ref, family="_col", solver=None, expect_args=None):
    """Everything the cases share.  Returns the template arguments of the kernels the sweeps ran on."""
    nset = len(alphas)
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    assert opt.ninit <= 8
    vals, grads = opt.evalGradF_batch(alphas)
    assert opt.last_batch_sets == nset
    batch_kernels = _kernels(h)
    if solver is not None:
        assert h.last_solver == solver, h.last_solver
    assert grads.shape == (nset, h.ndesign)
    for j in range(nset):
        single = opt.evalGradF(alphas[j])
        plain = _kernels(h)
        assert plain[0].startswith(f"k_forward{family}<") and plain[1].startswith(f"k_adjoint{family}<"), plain
        assert batch_kernels == _sets_names(plain), (batch_kernels, plain)
        print(j, plain[0], vals[j]["objective"], ref[j][0]["objective"], np.linalg.norm(grads[j] - single[1]),
              np.linalg.norm(grads[j] - ref[j][1]) / np.linalg.norm(ref[j][1]))
        assert _same_eval((vals[j], grads[j]), single), j
        check_parity(sp, vals[j], grads[j], *ref[j], alpha=alphas[j], msg=j)
    assert _same_eval((vals[0], grads[0]), (vals[2], grads[2]))
    assert not np.allclose(grads[0], grads[1], rtol=1e-3)
    fvals = opt.evalF_batch(alphas)
    assert opt.last_batch_sets == nset and h.last_kernel("forward") == batch_kernels[0]
    for j in range(nset):
        for k in OBJ_KEYS:
            assert fvals[j][k] == vals[j][k], (j, k)
    opt.close(); h.close()
    args = batch_kernels[0][batch_kernels[0].index("<") + 1:-1]
    if expect_args is not None:
        assert args == expect_args, args
    return args


# ---- the 3 x 20 system most cases share: three initial conditions, twelve steps; the oracle asked once ------------------------------------
@pytest.fixture(scope="module")
def c320():
    sp = _spec([3, 20])
    alphas = _alphas(sp, seed=27182)
    return alphas, _oracle(sp, alphas)


# <Q, EPT, SPLIT, USLOT, SKIP, KRY>: what col_sweep / col_uslot / QD_COL_DISPATCH of qd_col.h pick for the shape (helpers.col_kernels)
SHAPES = [
    pytest.param([3, 20], {}, "_col", "2, 5, true, true, true, false", id="3x20"),  # EPT 5, USLOT, ket-class forward form, SKIP
    pytest.param([5, 7], dict(objective="Jfrobenius"), "_col", "2, 5, true, false, true, false", id="5x7-N35"),  # no USLOT, idle lanes
    pytest.param([8, 8], dict(nessential=[7, 8], objective="Jtrace"), "_col", "2, 8, true, true, true, false", id="8x8-N64"),
    pytest.param([7, 9], dict(detuned=True), "_col", "2, 8, true, false, true, false", id="7x9-N63"),
    pytest.param([3, 3, 5], dict(nessential=[2, 3, 4]), "_col", "3, 5, true, true, true, false", id="3x3x5-N45"),
    pytest.param([3, 20], dict(jkl=0.004, detuned=True, objective="Jfrobenius"), "_colj", "2, 5, true, true, false, false", id="3x20-coupled"),
    pytest.param([4, 4, 4], dict(jkl=0.004, objective="Jfrobenius"), "_colj", "3, 8, true, false, false, false", id="4x4x4-coupled"),
]


@pytest.mark.parametrize("nlevels,kw,family,args", SHAPES)
def test_batch_is_identical_to_single_evaluations(nlevels, kw, family, args, c320):
    """Four sets in one launch per sweep.  The pair columns of the coupled shapes widen the table row: the set stride is not that of the
    uncoupled ones."""
    sp = _spec(nlevels, **kw)
    if kw:
        alphas = _alphas(sp, seed=1000 + int(np.prod(nlevels)) + len(kw))
        ref = _oracle(sp, alphas)
    else:
        alphas, ref = c320
    _batch_against_singles_and_oracle(sp, alphas, ref, family, "neumann", args)


def test_plain_neumann_iteration(c320):
    """neumann_split = 0: the reference's own iteration (SPLIT = false)."""
    alphas, ref = c320
    sp = _spec([3, 20], {**LEAN, "neumann_split": "0"})
    _batch_against_singles_and_oracle(sp, alphas, ref, "_col", "neumann", "2, 5, false, true, true, false")


def test_three_table_rows_per_step():
    """IMR4: three sub-steps per step lengthen every set's table; the stopping test runs in every pass (no SKIP)."""
    sp = _spec([3, 20], stepper="IMR4")
    alphas = _alphas(sp, seed=4)
    _batch_against_singles_and_oracle(sp, alphas, _oracle(sp, alphas), "_col", "neumann", "2, 5, true, true, false, false")


def test_gmres_request_served_by_the_stand_in():
    """linearsolver_type = gmres under the default gmres_split: the diagonal-split iteration under GMRES's stopping rule."""
    sp = _spec([3, 20], linsolve="gmres")
    alphas = _alphas(sp, seed=5)
    args = _batch_against_singles_and_oracle(sp, alphas, _oracle(sp, alphas), "_col", "gmres_as_split")
    assert args.startswith("2, 5, true, true, ") and args.endswith(", false"), args


def test_time_slices():
    """col_slices = 3 on the handle for the batch and the singles: twelve tasks in the batch launch, three in a single one; the
    scheduler words and the carry buffers are those of the batch's states."""
    sp = _spec([3, 20], {**LEAN, "col_slices": "3"}, ntime=20)
    alphas = _alphas(sp, seed=6)
    _batch_against_singles_and_oracle(sp, alphas, _oracle(sp, alphas), "_col", "neumann", "2, 5, true, true, true, false")


# ---- what stays set by set, groups ----------------------------------------------------------------------------------------------------------
def test_krylov_plan_stays_set_by_set():
    """gmres with gmres_split = 0 keeps the Krylov kernels, which have no set axis: set by set under batch_lean too."""
    sp = _spec([3, 20], {**LEAN, "gmres_split": "0"}, linsolve="gmres")
    alphas = _alphas(sp, seed=7)
    ref = _oracle(sp, alphas)
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    vals, grads = opt.evalGradF_batch(alphas)
    assert opt.last_batch_sets == 1 and h.last_solver == "krylov"
    assert _kernels(h) == ("k_forward_col<2, 5, true, true, false, true>", "k_adjoint_col<2, 5, true, true, false, true>"), _kernels(h)
    for j in range(4):
        check_parity(sp, vals[j], grads[j], *ref[j], alpha=alphas[j], msg=j)
    opt.close(); h.close()


def test_default_stays_set_by_set(c320):
    """The same 3 x 20 system without the option: a loop over the single evaluation on the plain kernels (passes with and without the
    feature)."""
    alphas, ref = c320
    sp = _spec([3, 20], {"col_slices": "1"})
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    vals, grads = opt.evalGradF_batch(alphas)
    assert opt.last_batch_sets == 1
    assert _kernels(h) == ("k_forward_col<2, 5, true, true, true, false>", "k_adjoint_col<2, 5, true, true, true, false>"), _kernels(h)
    for j in range(4):
        check_parity(sp, vals[j], grads[j], *ref[j], alpha=alphas[j], msg=j)
    opt.evalF_batch(alphas)
    assert opt.last_batch_sets == 1 and h.last_kernel("forward") == "k_forward_col<2, 5, true, true, true, false>"
    opt.close(); h.close()


def test_sets_that_do_not_fit_together_go_in_groups(c320):
    """Four sets under a trajectory budget that holds two sets' stored trajectories and not three: two launches of two sets each."""
    alphas, ref = c320
    sp = _spec([3, 20])
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    # what one set stores, in bytes: the primal stages of every step and - the weighted-J penalty of this Jmeasure objective is a constant
    # per row, the system has no guard levels - no states (qd_handle::adjoint_reads_states)
    per_set = sp.time.ntime * opt.ninit * 2 * h.dim * 8
    h.set_option("traj_budget_mb", 2.5 * per_set / 1048576.0)
    vals, grads = opt.evalGradF_batch(alphas)
    assert opt.last_batch_sets == 2
    assert _kernels(h) == ("k_forward_col_sets<2, 5, true, true, true, false>", "k_adjoint_col_sets<2, 5, true, true, true, false>"), _kernels(h)
    h.set_option("traj_budget_mb", 0)
    for j in range(4):
        assert _same_eval((vals[j], grads[j]), opt.evalGradF(alphas[j])), j
        check_parity(sp, vals[j], grads[j], *ref[j], alpha=alphas[j], msg=j)
    opt.close(); h.close()
