"""Forward sweeps on Hermitian pairs (option pair_hermitian; qd_handle::pair_gate, the penalty block of k_forward in qd_col.h, k_pair /
k_unpair in qd_kernels.hip): a sweep that stores nothing propagates the exactly Hermitian initial conditions of a Lindblad shard two
at a time, X = rho_a + i rho_b.  Every case runs with pair_hermitian = 1 against pair_hermitian = 0 on the same handle and against the
oracle, per initial condition (Optim.last_local_results): with equal weights only per-state values can see an a / b mix-up."""
import uuid

import numpy as np
import pytest

from helpers import REF_RTOL, ROOT, col_kernels, synthetic_cfg, synthetic_spec
from oracle.oracle import Oracle
from quandary_amd import capi, config

pytestmark = pytest.mark.gpu

# partial sums (include/quandary_amd.h)
SUM_PENALTY, SUM_COST_RE, SUM_COST_IM, SUM_FID_RE, SUM_FID_IM = 0, 3, 4, 5, 6

BASE = dict(lindblad=True, target="pure", init="basis, 0", ntime=12, dt=0.001)
SHAPES = {
    "3x20": dict(nlevels=[3, 20]),                        # 9 states: odd count, imaginary off-diagonals, EPT 5, ket classes, real-drive frame
    "4x12-guard": dict(nlevels=[4, 12], nessential=[3, 11]),  # leakage sum; N = 48
    "8x8": dict(nlevels=[8, 8]),                          # EPT 8, no idle lanes
    "3x3x5": dict(nlevels=[3, 3, 5]),                     # three oscillators
}


def _spec(shape, objective="Jmeasure", penalties=True, **kw):
    sp = synthetic_spec(**{**BASE, **SHAPES[shape], "objective": objective, "penalties": penalties, **kw})
    sp.options = {"neumann_split": "1", "col_slices": "1"}
    return sp


def _scaled(sp, ninit, pen, out4):
    """Per-state results as the oracle's one-state shards report them: [w gamma pen, w J_re, w J_im, fid_re / ninit, fid_im / ninit]."""
    w, gamma = 1.0 / ninit, sp.objective.penalty.gamma_penalty
    return np.column_stack([w * gamma * pen, w * out4[:, 0], w * out4[:, 1], out4[:, 2] / ninit, out4[:, 3] / ninit])


def _run(opt, h, alpha, mode):
    h.set_option("pair_hermitian", mode)
    sums = opt.forward_local(alpha)
    pen, out4 = opt.last_local_results()
    return sums, pen, out4, opt.last_paired, h.mean_applies, h.last_kernel("forward"), h.last_solver


def _against_oracle_and_unpaired(shape, objective, penalties):
    sp = _spec(shape, objective, penalties)
    alpha = sp.params0
    h, orc = capi.Handle(sp), Oracle(sp)
    opt = capi.Optim(h, sp)
    ninit = opt.ninit
    want = col_kernels(SHAPES[shape]["nlevels"], "1", "IMR")["forward"]
    want_pair = want.replace("k_forward_col<", "k_forward_col_pair<")  # the same instantiation of the lean column kernel, in its pair form
    s0, pen0, o0, paired0, app0, k0, _ = _run(opt, h, alpha, 0)
    s1, pen1, o1, paired1, app1, k1, solver1 = _run(opt, h, alpha, 1)
    print(shape, objective, "states", ninit, "passes per step: paired", app1, "unpaired", app0, "cap", sp.solver.maxiter)
    assert paired0 == 0 and paired1 == 1
    assert k0 == want and k1 == want_pair and solver1 == "neumann", (k0, k1, solver1)
    assert app1 <= sp.solver.maxiter
    # against the unpaired run, per initial condition
    for name, a, b in (("penalty", pen1, pen0), ("out4", o1, o0)):
        err = np.abs(a - b) / np.maximum(1.0, np.abs(b))
        print(" paired vs unpaired", name, err.max())
        assert (err <= 1e-9).all(), (name, err.max())
    # against the oracle's one-state shards
    got = _scaled(sp, ninit, pen1, o1)
    ref = np.zeros((ninit, 5))
    osum = np.zeros(capi.NSUMS)
    for i in range(ninit):
        p = orc.forward_local(alpha, i, ninit)
        ref[i] = [p[SUM_PENALTY], p[SUM_COST_RE], p[SUM_COST_IM], p[SUM_FID_RE], p[SUM_FID_IM]]
        osum += p
    print(" paired vs oracle, worst per-state", np.abs(got - ref).max(), "of", np.abs(ref).max())
    np.testing.assert_allclose(got, ref, rtol=1e-7, atol=1e-12)
    np.testing.assert_allclose(s1, osum, rtol=REF_RTOL, atol=1e-12)
    if penalties and shape == "4x12-guard":
        assert (pen1 > 0).all()
    # three time slices: the carry is the pair as computed, so every number the final states give keeps its bits; the penalty sums are
    # added slice by slice, as the single sum of an unpaired sliced sweep is (another order of the same additions)
    h.set_option("col_slices", 3)
    s3, pen3, o3, paired3, _, k3, _ = _run(opt, h, alpha, 1)
    assert paired3 == 1 and k3 == want_pair
    np.testing.assert_array_equal(o3, o1)
    np.testing.assert_allclose(pen3, pen1, rtol=1e-13, atol=1e-16)
    opt.close(); h.close(); orc.close()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_paired_sweep_per_initial_condition(shape):
    """Penalties on, Jmeasure, neumann: penalty and the four objective numbers of every initial condition, the seven sums, the kernel,
    the pass counts, three time slices."""
    _against_oracle_and_unpaired(shape, "Jmeasure", True)


@pytest.mark.parametrize("objective", ["Jfrobenius", "Jtrace"])
@pytest.mark.parametrize("shape", ["3x20", "4x12-guard"])
def test_any_final_objective_with_the_penalty_off(shape, objective):
    """k_objective runs behind the un-pairing: any objective type."""
    _against_oracle_and_unpaired(shape, objective, False)


def test_the_gate():
    """auto on a small shard, a weighted penalty that reads off-diagonal elements, a gmres request, a stored trajectory; and a gradient
    evaluation, which stays unpaired and keeps its bits whatever evalF did in between."""
    sp = _spec("3x20")
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    h.set_option("pair_hermitian", "auto")
    opt.evalF(sp.params0)
    assert opt.last_paired == 0  # (9 states: fewer than the device has compute units)
    h.set_option("pair_hermitian", 1)
    val_a, g_a = opt.evalGradF(sp.params0)
    assert opt.last_paired == 0
    opt.evalF(sp.params0)
    assert opt.last_paired == 1
    val_b, g_b = opt.evalGradF(sp.params0)
    assert opt.last_paired == 0
    assert val_a == val_b and np.array_equal(g_a, g_b)
    opt.forward_local(sp.params0, store_trajectory=True)
    assert opt.last_paired == 0
    opt.forward_local(sp.params0)
    assert opt.last_paired == 1
    opt.close(); h.close()
    # weighted penalty + Jtrace: off-diagonal elements every step
    sp = _spec("3x20", "Jtrace", True)
    sp.options["pair_hermitian"] = "1"
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    opt.evalF(sp.params0)
    assert opt.last_paired == 0
    opt.close(); h.close()
    # ... the same objective without the penalty pairs
    sp = _spec("3x20", "Jtrace", False)
    sp.options["pair_hermitian"] = "1"
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    opt.evalF(sp.params0)
    assert opt.last_paired == 1
    opt.close(); h.close()
    # a gmres request: its threshold uses ||b|| of the state
    for split in ("auto", "0"):
        sp = _spec("3x20", linsolve="gmres")
        sp.options = {"gmres_split": split, "pair_hermitian": "1"}
        h = capi.Handle(sp)
        opt = capi.Optim(h, sp)
        opt.evalF(sp.params0)
        assert h.last_solver != "neumann" and opt.last_paired == 0, (split, h.last_solver)
        opt.close(); h.close()


def _rank_worker(rank, world, name, cfg_text, options, q):
    import ctypes as C
    import sys
    sys.path.insert(0, ROOT)
    from quandary_amd import capi, config
    try:
        lib = capi.load_library()
        sp = config.build_spec(config.parse_config_text(cfg_text))
        sp.options = dict(options)
        h = capi.Handle(sp)
        opt = capi.Optim(h, sp, rank=rank, nranks=world)
        comm = C.c_void_p()
        capi.check(lib.qd_comm_create_host(name.encode(), rank, world, 0, 120.0, C.byref(comm)), "qd_comm_create_host")
        val, _ = opt.evalF_dist(comm, sp.params0)
        q.put((rank, "ok", dict(val=val, paired=opt.last_paired, nlocal=opt.ninit_local)))
        capi.check(lib.qd_comm_barrier(comm), "barrier")
        lib.qd_comm_destroy(comm)
        opt.close(); h.close()
    except Exception as e:  # noqa: BLE001
        q.put((rank, "error", f"{type(e).__name__}: {e}"))


def test_two_ranks_sharing_the_gpu():
    """evalF_dist on two ranks (host backend), 8 states each of the 4 x 12 system's 16, against the single-rank paired result."""
    import multiprocessing as mp

    kw = {**BASE, "nlevels": [4, 12], "nessential": [4, 11], "objective": "Jmeasure", "penalties": True}
    options = {"neumann_split": "1", "pair_hermitian": "1"}
    cfg_text = synthetic_cfg(**kw)
    sp = config.build_spec(config.parse_config_text(cfg_text))
    sp.options = dict(options)
    h = capi.Handle(sp)
    one = capi.Optim(h, sp)
    ref = one.evalF(sp.params0)
    assert one.last_paired == 1 and one.ninit == 16
    one.close(); h.close()
    name = "p" + uuid.uuid4().hex[:16]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, name, cfg_text, options, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    for _ in procs:
        rank, status, out = q.get(timeout=300)
        assert status == "ok", (rank, out)
        res[rank] = out
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for rank in range(2):
        assert res[rank]["paired"] == 1 and res[rank]["nlocal"] == 8
        for k in ref:
            assert res[rank]["val"][k] == pytest.approx(ref[k], rel=1e-12, abs=1e-15), (rank, k)
