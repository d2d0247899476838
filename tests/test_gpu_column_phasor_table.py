"""Phasor table of the real-drive frame (qd_gauge.h, k_gauge; read by ColTeam::stage of qd_col.h): the lean column forward kernels of
the diagonal-split solver without coupling read r_k and the row phasors of a sub-step from a table built with the control table.  What is
new, and what these cases aim at: WHICH table row a step reads (composite steppers, time slices that start at rows other than 0), WHICH
set's table (parameter-set batch), and WHEN the table is rebuilt (a parameter update, an option that changes the kernel after qd_create).
The arithmetic of the phasors themselves is that of tests/test_gpu_column_real_drive.py, which runs on the same code path.

Every system is synthetic: 12 or 13 steps of 0.001 ns, neumann_split = 1, at most 8 initial conditions."""
import numpy as np
import pytest

from helpers import OBJ_KEYS, REF_RTOL, col_kernels, synthetic_spec
from oracle.oracle import Oracle
from quandary_amd import capi

pytestmark = pytest.mark.gpu

SPLIT = {"neumann_split": "1"}


def _spec(nlevels, options=SPLIT, **kw):
    kw = {**dict(lindblad=True, target="pure", objective="Jmeasure", init="diagonal, 0", ntime=12, dt=0.001, penalties=True), **kw}
    sp = synthetic_spec(nlevels, **kw)
    sp.options = dict(options)
    return sp


def _sweep_vector(sp):
    """The "sweep" vector of test_gpu_column_real_drive.py: 40 x the amplitude of params0, the coefficient phase turning by 0.3 of a circle
    from spline to spline - the phases visit all four quadrants within the sweep (checked on the oracle's controls)."""
    n, q = sp.params0.size, sp.system.nosc
    assert n % q == 0
    a = np.zeros_like(sp.params0)
    amp = 40.0 * np.abs(sp.params0).max()
    for k in range(q):
        b = slice(k * n // q, (k + 1) * n // q)
        half = (b.stop - b.start) // 4  # two carriers x (first part, second part)
        ph = 2.0 * np.pi * (0.3 * np.arange(half) + 0.17 * k)
        a[b] = amp * np.concatenate([np.cos(ph), np.sin(ph), np.cos(ph + 1.0), np.sin(ph + 1.0)])
    orc = Oracle(sp)
    orc.set_params(a)
    pq = orc.eval_controls((np.arange(sp.time.ntime) + 0.5) * sp.time.dt)
    orc.close()
    quadrants = {(bool(p > 0), bool(q > 0)) for p, q in pq.reshape(-1, 2)}
    assert len(quadrants) == 4, quadrants
    return a


def _same_eval(a, b):
    (va, ga), (vb, gb) = a, b
    return all(va[k] == vb[k] for k in OBJ_KEYS) and np.array_equal(ga, gb)


def _gradient_against_oracle(sp, alpha, kernels, nstages=1):
    """The rule of test_gpu_column_real_drive.py, restated: objective parts (1e-7, the suite's 1e-12 floor) and gradient (1e-8 of its norm)
    of one evaluation against the oracle, on the kernels named, all finite.  The input must be one the reference itself solves: the
    oracle's Neumann iteration stays below the iteration cap per solve."""
    h, orc = capi.Handle(sp), Oracle(sp)
    opt = capi.Optim(h, sp)
    val, g = opt.evalGradF(alpha)
    assert (h.last_kernel("forward"), h.last_kernel("adjoint")) == (kernels["forward"], kernels["adjoint"])
    orc.reset_stats()
    orc.evalF(alpha)
    print("oracle applications per solve, forward sweep", orc.mean_applies / nstages, "cap", sp.solver.maxiter)
    assert orc.mean_applies / nstages < sp.solver.maxiter - 1
    oval, og = orc.evalGradF(alpha)
    for k in OBJ_KEYS:
        print(k, val[k], oval[k])
        assert np.isfinite(val[k]), k
        assert val[k] == pytest.approx(oval[k], rel=REF_RTOL, abs=1e-12), k
    assert np.isfinite(g).all()
    print("gradient", np.linalg.norm(g - og), np.linalg.norm(og))
    assert np.linalg.norm(og) > 0
    assert np.linalg.norm(g - og) < 1e-8 * np.linalg.norm(og)
    opt.close(); h.close(); orc.close()


@pytest.mark.parametrize("nlevels", [[3, 20], [3, 3, 5]], ids=["3x20", "3x3x5"])
def test_table_rows_under_a_composite_stepper_and_time_slices(nlevels):
    """IMR4 (three table rows per step, negative middle sub-step) on 13 steps: 3 and 5 slices do not divide 13, so slices start at table
    rows 12, 24 / 6, 15, 21, 30.  Random non-Hermitian states, penalties on.  One slice against the oracle's stepper (1e-9 of the state
    norm); 3 and 5 slices against one, bit for bit."""
    sp = _spec(nlevels, ntime=13, stepper="IMR4")
    h, orc = capi.Handle(sp), Oracle(sp)
    h.set_params(sp.params0)
    orc.set_params(sp.params0)
    x0 = np.random.default_rng(17).standard_normal((3, 2 * h.dim))
    # (the in-loop penalties of the spec - weighted Jmeasure at the end of every full step - at the stepper level)
    h.set_target(capi.TARGET["pure"], capi.OBJECTIVE["Jmeasure"], purestate_id=0, nb=x0.shape[0])
    h.set_penalty(gamma_penalty=0.3, penalty_param=0.5)
    h.set_option("col_slices", 1)
    ref = h.forward(x0)
    assert h.last_kernel("forward") == col_kernels(nlevels, "1", "IMR4")["forward"]
    assert np.isfinite(ref["final_states"]).all() and np.isfinite(ref["penalty_integral"]).all()
    for i in range(x0.shape[0]):
        x = x0[i]
        for n in range(sp.time.ntime):
            x = orc.step_fwd(n * sp.time.dt, (n + 1) * sp.time.dt, x)
        print(i, np.linalg.norm(ref["final_states"][i] - x) / np.linalg.norm(x))
        assert np.linalg.norm(ref["final_states"][i] - x) < 1e-9 * np.linalg.norm(x)
    for k in (3, 5):
        h.set_option("col_slices", k)
        res = h.forward(x0)
        assert h.last_kernel("forward") == col_kernels(nlevels, "1", "IMR4")["forward"]
        np.testing.assert_array_equal(res["final_states"], ref["final_states"])
    h.close(); orc.close()


def test_table_follows_every_parameter_update():
    """A, B, A on one handle: both A results bit-identical, B bit-identical to a fresh handle's - through qd_forward and through
    Optim.evalGradF.  B is the "sweep" vector: no phasor of A's table fits it."""
    sp = _spec([3, 20])
    a, b = sp.params0, _sweep_vector(sp)
    want = col_kernels([3, 20], "1", "IMR")["forward"]
    x0 = np.random.default_rng(5).standard_normal((3, 2 * 60 * 60))

    def forward(h, alpha):
        h.set_params(alpha)
        res = h.forward(x0)
        assert h.last_kernel("forward") == want
        return res["final_states"]

    h, fresh = capi.Handle(sp), capi.Handle(sp)
    a1, b1, a2 = forward(h, a), forward(h, b), forward(h, a)
    np.testing.assert_array_equal(a1, a2)
    np.testing.assert_array_equal(b1, forward(fresh, b))
    assert not np.array_equal(a1, b1)
    h.close(); fresh.close()

    h, fresh = capi.Handle(sp), capi.Handle(sp)
    opt, ofresh = capi.Optim(h, sp), capi.Optim(fresh, sp)
    ea1, eb1, ea2 = opt.evalGradF(a), opt.evalGradF(b), opt.evalGradF(a)
    assert h.last_kernel("forward") == want
    assert _same_eval(ea1, ea2)
    assert _same_eval(eb1, ofresh.evalGradF(b))
    assert not np.array_equal(ea1[1], eb1[1])
    opt.close(); ofresh.close(); h.close(); fresh.close()


def test_one_table_per_set_of_a_parameter_set_batch():
    """batch_lean = 1, three sets - params0, no drive at all, the "sweep" vector - on 3 x 20 with four diagonal initial conditions: every
    set bit-identical to its single evaluation on the same handle (the rule of tests/test_gpu_param_batch_col.py), and the sets permuted
    give the permuted results."""
    sp = _spec([3, 20], {**SPLIT, "batch_lean": "1", "col_slices": "1"}, nessential=[3, 4], init="diagonal, 1")
    alphas = np.stack([sp.params0, np.zeros_like(sp.params0), _sweep_vector(sp)])
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    assert opt.ninit == 4
    plain = col_kernels([3, 20], "1", "IMR")
    sets = tuple(plain[k].replace("_col<", "_col_sets<") for k in ("forward", "adjoint"))
    vals, grads = opt.evalGradF_batch(alphas)
    assert opt.last_batch_sets == 3
    assert (h.last_kernel("forward"), h.last_kernel("adjoint")) == sets
    for j in range(3):
        single = opt.evalGradF(alphas[j])
        assert (h.last_kernel("forward"), h.last_kernel("adjoint")) == (plain["forward"], plain["adjoint"])
        assert np.isfinite(grads[j]).all() and all(np.isfinite(vals[j][k]) for k in OBJ_KEYS)
        assert _same_eval((vals[j], grads[j]), single), j
    assert not np.array_equal(grads[0], grads[2])
    perm = [2, 0, 1]
    pvals, pgrads = opt.evalGradF_batch(alphas[perm])
    assert opt.last_batch_sets == 3 and h.last_kernel("forward") == sets[0]
    for j, src in enumerate(perm):
        assert _same_eval((pvals[j], pgrads[j]), (vals[src], grads[src])), (j, src)
    fvals = opt.evalF_batch(alphas[perm])
    assert opt.last_batch_sets == 3 and h.last_kernel("forward") == sets[0]
    for j, src in enumerate(perm):
        for k in OBJ_KEYS:
            assert fvals[j][k] == vals[src][k], (j, k)
    opt.close(); h.close()


def test_option_that_selects_the_kernel_changes_after_create():
    """neumann_split = 0 at qd_create and for a first evaluation (the plain Neumann kernel reads no table), then 1: the result of a handle
    created with 1."""
    sp0, sp1 = _spec([3, 20], {"neumann_split": "0"}), _spec([3, 20])
    h = capi.Handle(sp0)
    opt = capi.Optim(h, sp0)
    opt.evalGradF(sp0.params0)
    assert h.last_kernel("forward") == col_kernels([3, 20], "0", "IMR")["forward"]
    h.set_option("neumann_split", 1)
    got = opt.evalGradF(sp0.params0)
    assert h.last_kernel("forward") == col_kernels([3, 20], "1", "IMR")["forward"]
    h1 = capi.Handle(sp1)
    opt1 = capi.Optim(h1, sp1)
    assert _same_eval(got, opt1.evalGradF(sp1.params0))
    opt.close(); h.close(); opt1.close(); h1.close()


@pytest.mark.parametrize("kw", [
    pytest.param(dict(nlevels=[8, 8], objective="Jtrace"), id="8x8-N64"),  # every lane a row: no padding entry in a table row
    pytest.param(dict(nlevels=[4, 12], nessential=[3, 11], objective="Jfrobenius"), id="4x12-N48-guard"),  # 16 padding rows, guard levels
])
def test_full_and_padded_lane_rows(kw):
    sp = _spec(**kw)
    _gradient_against_oracle(sp, sp.params0, col_kernels(kw["nlevels"], "1", "IMR"))


def test_chunked_gradient():
    """3 x 20 with eight initial conditions under a trajectory budget that forces at least two chunks: every chunk's sweeps read the one
    table.  The rule of test_chunked_gradient_when_the_trajectory_does_not_fit (tests/test_gpu_parity.py): objective parts to 1e-13,
    gradient to 1e-11 (1e-12 of its norm absolute)."""
    sp = _spec([3, 20], nessential=[3, 8], init="diagonal, 1")
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    assert opt.ninit == 8
    val, g = opt.evalGradF(sp.params0)
    assert opt.last_chunks == 1
    assert h.last_kernel("forward") == col_kernels([3, 20], "1", "IMR")["forward"]
    per_ic = (13 + 12) * 2 * h.dim * 8  # states + primal stages of one initial condition
    h.set_option("traj_budget_mb", per_ic * 5 / 1048576.0)
    val2, g2 = opt.evalGradF(sp.params0)
    print("chunks", opt.last_chunks)
    assert opt.last_chunks >= 2
    assert h.last_kernel("forward") == col_kernels([3, 20], "1", "IMR")["forward"]
    for k in OBJ_KEYS:
        assert val2[k] == pytest.approx(val[k], rel=1e-13, abs=1e-15), k
    np.testing.assert_allclose(g2, g, rtol=1e-11, atol=1e-15 + 1e-12 * np.linalg.norm(g))
    opt.close(); h.close()
