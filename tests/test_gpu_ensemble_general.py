"""Model-parameter ensemble on the general kernel family (option ensemble_general = 1): the variants of one call share launches on
k_forward_vars / k_adjoint_vars, which read one block of model constants per variant (qd_gen_vars.h); qd_last_kernel names them with the
six template arguments of the kernel the single evaluation on the same handle runs on.  Without the option, and on every family without
such a form, the call goes variant by variant as before.

Fixtures, shape table and their witness: tests/test_ensemble_general_cpu.py.  Each variant is held against the oracle of a spec with that
variant's constants through helpers.check_parity: no new tolerance appears here."""
import numpy as np
import pytest

from helpers import GMRES_MODES, OBJ_KEYS, with_gmres_mode
from quandary_amd import capi
from test_ensemble_general_cpu import SHAPE_PARAMS, shape
from test_ensemble_model_cpu import BLOCKS, model_spec, oracle_grads, variant_specs
from test_gpu_ensemble import _dense_spec, _fma_chain
from test_gpu_ensemble_model import _alpha, _kernels, _parity, _same_eval, _systems

pytestmark = pytest.mark.gpu

ON = {"ensemble_general": "1"}


def _fixture(nlevels, kw, coupled, options, nblocks=4):
    """(make, alpha, variant specs, the oracle's evaluation of every variant); make() gives the spec with ensemble_general = 1."""
    def make():
        return model_spec(nlevels, options={**options, **ON}, **kw)
    specs = variant_specs(make, coupled, blocks=BLOCKS[:nblocks])
    alpha = _alpha(specs[0])
    ref = oracle_grads(specs, alpha)
    assert not np.allclose(ref[0][1], ref[1][1], rtol=1e-3), "the oracle's gradients of variants 0 and 1 do not differ"
    return make, alpha, specs, ref


def _twins(plain):
    """The variant twins of the plain general kernels a single evaluation reported."""
    for n in plain:
        assert n.startswith(("k_forward<", "k_adjoint<")), n
    return tuple(n.replace("k_forward<", "k_forward_vars<").replace("k_adjoint<", "k_adjoint_vars<") for n in plain)


@pytest.mark.parametrize("nlevels,kw,coupled,options,args", SHAPE_PARAMS)
def test_every_shape(monkeypatch, nlevels, kw, coupled, options, args):
    """1. Four variants in one launch on the twins of the kernels the single evaluation runs on; every variant against the oracle of its
    own spec; variant 2 (a copy of block 0) bit for bit variant 0; the handle's own evaluation before and after identical and variant 0."""
    make, alpha, specs, ref = _fixture(nlevels, kw, coupled, options)
    h = capi.Handle(make())
    opt = capi.Optim(h, h.spec)
    assert opt.ninit <= 8
    before = opt.evalGradF(alpha)
    plain = _kernels(h)
    assert all(n.startswith((f"k_forward<{args}, ", f"k_adjoint<{args}, ")) for n in plain), plain
    mean, grad_mean, vals, grads = opt.evalGradF_ensemble_model(alpha, _systems(specs))
    assert opt.last_batch_sets == 4
    assert _kernels(h) == _twins(plain), (_kernels(h), plain)
    _parity(specs, alpha, vals, grads, ref)
    assert _same_eval((vals[0], grads[0]), (vals[2], grads[2]))
    after = opt.evalGradF(alpha)
    assert _kernels(h) == plain
    assert _same_eval(before, after) and _same_eval(before, (vals[0], grads[0]))
    opt.close(); h.close()


@pytest.mark.parametrize("name", ["2x2-schroedinger", "3x3-lindblad"])
def test_neumann_request_is_fresh_handles_the_loop_and_the_default(name):
    """2. A Neumann request: the shared call is bit for bit evalGradF on fresh handles created from each variant's spec, the same call
    under ensemble_loop = 1 and the same call under ensemble_general = 0."""
    nlevels, kw, coupled, options, args = shape(name)
    make, alpha, specs, ref = _fixture(nlevels, kw, coupled, options)
    h = capi.Handle(make())
    opt = capi.Optim(h, h.spec)
    mean, grad_mean, vals, grads = opt.evalGradF_ensemble_model(alpha, _systems(specs))
    assert opt.last_batch_sets == 4
    shared = _kernels(h)
    assert shared[0].startswith(f"k_forward_vars<{args}, "), shared
    for key in ("ensemble_loop", "ensemble_general"):
        h.set_option(key, "1" if key == "ensemble_loop" else "0")
        mean_l, grad_mean_l, vals_l, grads_l = opt.evalGradF_ensemble_model(alpha, _systems(specs))
        assert opt.last_batch_sets == 1 and _twins(_kernels(h)) == shared, (key, _kernels(h))
        assert vals_l == vals and np.array_equal(grads_l, grads) and mean_l == mean and np.array_equal(grad_mean_l, grad_mean), key
        h.set_option(key, "0" if key == "ensemble_loop" else "1")
    opt.close(); h.close()
    for j, sp in enumerate(specs):
        hj = capi.Handle(sp)
        oj = capi.Optim(hj, sp)
        fresh = oj.evalGradF(alpha)
        print(j, vals[j]["objective"], fresh[0]["objective"], np.linalg.norm(grads[j] - fresh[1]))
        assert _twins(_kernels(hj)) == shared
        assert _same_eval((vals[j], grads[j]), fresh), j
        oj.close(); hj.close()


@pytest.mark.parametrize("name", ["2x2-schroedinger", "3x3-lindblad", "3x3x3-lindblad"])
@pytest.mark.parametrize("mode", GMRES_MODES)
def test_gmres_request(name, mode):
    """2 (continued). linearsolver_type = gmres.  gmres_split = 0: the Krylov kernels share the launch (3 x 3 x 3: the basis in global
    memory, sized for all states of the launch) and the result is the loop's bit for bit.  auto: the stand-in shares the launch and is
    held to the oracle with any_solver.

    The shared plan comes from the row bounds maximised over the variants, a variant's own plan in the loop from its own bounds.  The
    fields of the plan that reach a general kernel are the solver (use_gmres), the polynomial degree of the Krylov kernels and, for the
    stand-in, standin_tau2 and the iteration cap; the loop is compared bit for bit where last_solver and the kernel names of both calls
    agree (asserted for gmres_split = 0: both are the Krylov kernels, degree 1 on the general family), and every call to the oracle."""
    nlevels, kw, coupled, options, args = shape(name)
    make, alpha, specs, ref = _fixture(nlevels, dict(kw, linsolve="gmres"), coupled, options, nblocks=3)
    sp = with_gmres_mode(make(), mode)
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    mean, grad_mean, vals, grads = opt.evalGradF_ensemble_model(alpha, _systems(specs))
    shared, solver = _kernels(h), h.last_solver
    print(mode, shared, solver, opt.last_batch_sets)
    assert opt.last_batch_sets == 3
    assert shared[0].startswith(f"k_forward_vars<{args}, ") and shared[1].startswith(f"k_adjoint_vars<{args}, "), shared
    _parity(specs, alpha, vals, grads, ref, any_solver=True)
    assert _same_eval((vals[0], grads[0]), (vals[2], grads[2]))
    h.set_option("ensemble_loop", "1")
    mean_l, grad_mean_l, vals_l, grads_l = opt.evalGradF_ensemble_model(alpha, _systems(specs))
    assert opt.last_batch_sets == 1
    if mode == "0":
        assert solver == "krylov" and h.last_solver == "krylov" and _twins(_kernels(h)) == shared, (solver, h.last_solver, _kernels(h))
        assert f"k_forward_vars<{args}, true, " in shared[0], shared
        assert vals_l == vals and np.array_equal(grads_l, grads) and mean_l == mean and np.array_equal(grad_mean_l, grad_mean)
    else:
        _parity(specs, alpha, vals_l, grads_l, ref, any_solver=True)
        if h.last_solver == solver and _twins(_kernels(h)) == shared:
            assert vals_l == vals and np.array_equal(grads_l, grads)
    opt.close(); h.close()


def test_weights_mean_forward_only_and_groups():
    """3. Five variants over three states, weighted: the fma chain of k_ensemble_mean; per_variant = False gives the same mean bits; the
    forward-only call gives the same values; under a trajectory budget that holds three variants the groups are three and two and the
    results those of the ungrouped call."""
    nlevels, kw, coupled, options, args = shape("3x3-lindblad")
    make, alpha, specs, ref = _fixture(nlevels, kw, coupled, options)
    systems = _systems(specs)
    five = systems + [systems[1]]
    w5 = np.array([0.3, 0.1, 0.2, 0.15, 0.25])
    h = capi.Handle(make())
    opt = capi.Optim(h, h.spec)
    assert opt.ninit == 3
    mean5, grad_mean5, vals5, grads5 = opt.evalGradF_ensemble_model(alpha, five, weights=w5)
    assert opt.last_batch_sets == 5 and _kernels(h)[0].startswith("k_forward_vars<"), _kernels(h)
    _parity(specs, alpha, vals5[:4], grads5[:4], ref)
    assert _same_eval((vals5[1], grads5[1]), (vals5[4], grads5[4]))
    assert np.array_equal(grad_mean5, _fma_chain(w5, grads5))
    chain = _fma_chain(w5, np.array([[v[k] for k in OBJ_KEYS] for v in vals5]))
    assert [mean5[k] for k in OBJ_KEYS] == list(chain)
    mean_o, grad_mean_o, vals_o, none = opt.evalGradF_ensemble_model(alpha, five, weights=w5, per_variant=False)
    assert none is None and vals_o == vals5 and mean_o == mean5 and np.array_equal(grad_mean_o, grad_mean5)
    fmean, fvals = opt.evalF_ensemble_model(alpha, five, weights=w5)
    assert opt.last_batch_sets == 5 and fvals == vals5 and fmean == mean5
    nt = h.spec.time.ntime
    traj = (2 * nt + 1) * opt.ninit * 2 * h.dim * 8  # states and primal stages of one variant, bytes
    h.set_option("traj_budget_mb", 3.5 * traj / 1048576.0)
    mean_g, grad_mean_g, vals_g, grads_g = opt.evalGradF_ensemble_model(alpha, five, weights=w5)
    assert opt.last_batch_sets == 3, opt.last_batch_sets
    assert vals_g == vals5 and np.array_equal(grads_g, grads5) and mean_g == mean5 and np.array_equal(grad_mean_g, grad_mean5)
    opt.close(); h.close()


def test_without_the_option_nothing_changes():
    """4. The default: variant by variant on the plain kernels."""
    nlevels, kw, coupled, options, args = shape("3x3-lindblad")
    make, alpha, specs, ref = _fixture(nlevels, kw, coupled, options, nblocks=2)
    sp = make()
    del sp.options["ensemble_general"]
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    mean, grad_mean, vals, grads = opt.evalGradF_ensemble_model(alpha, _systems(specs))
    assert opt.last_batch_sets == 1
    assert _kernels(h)[0].startswith(f"k_forward<{args}, ") and _kernels(h)[1].startswith(f"k_adjoint<{args}, "), _kernels(h)
    _parity(specs, alpha, vals, grads, ref)
    opt.close(); h.close()


FALLBACK = [
    pytest.param([2, 2, 2, 2], dict(nessential=[2, 2, 2, 2]), None, "k_forward_q32<", id="2^4-lindblad-slot"),
    pytest.param([2, 2], {}, "16", "k_forward_big<", id="2x2-lindblad-global"),
]


@pytest.mark.parametrize("nlevels,kw,var,kernel", FALLBACK)
def test_other_families_still_go_variant_by_variant(monkeypatch, nlevels, kw, var, kernel):
    """4 (continued). With the option set, a lean slot plan and a global-memory plan behave as without it."""
    if var is not None:
        monkeypatch.setenv("QD_VAR", var)
    make, alpha, specs, ref = _fixture(nlevels, kw, False, {}, nblocks=2)
    h = capi.Handle(make())
    opt = capi.Optim(h, h.spec)
    before = opt.evalGradF(alpha)
    w = np.array([0.3, 0.7])
    mean, grad_mean, vals, grads = opt.evalGradF_ensemble_model(alpha, _systems(specs), weights=w)
    assert opt.last_batch_sets == 1
    assert h.last_kernel("forward").startswith(kernel), h.last_kernel("forward")
    _parity(specs, alpha, vals, grads, ref)
    assert np.array_equal(grad_mean, _fma_chain(w, grads))
    assert _same_eval(before, (vals[0], grads[0])) and _same_eval(before, opt.evalGradF(alpha))
    opt.close(); h.close()


def test_a_dense_handle_is_refused_as_before():
    sp = _dense_spec([2, 2], lindblad=True)
    sp.options = {**(getattr(sp, "options", None) or {}), **ON}
    a = _alpha(sp, amp=0.3)
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    before = opt.evalGradF(a)
    with pytest.raises(capi.QuandaryAmdError, match=r"rc=-5"):  # QD_ERR_STATE
        opt.evalGradF_ensemble_model(a, [sp.system, sp.system])
    assert _same_eval(before, opt.evalGradF(a))
    opt.close(); h.close()


def test_errors_leave_the_handle_usable():
    """5. nvar = 0, a NaN constant, a negative weight: QD_ERR_INVALID; a coupling on an uncoupled handle: QD_ERR_UNSUPPORTED.  The handle
    evaluates bit-identically after each."""
    nlevels, kw, coupled, options, args = shape("3x3-lindblad")

    def make():
        return model_spec(nlevels, options={**options, **ON}, **kw)
    specs = variant_specs(make, False, blocks=BLOCKS[:2])
    systems = _systems(specs)
    alpha = _alpha(specs[0])
    h = capi.Handle(make())
    opt = capi.Optim(h, h.spec)
    before = opt.evalGradF(alpha)
    with pytest.raises(capi.QuandaryAmdError, match=r"rc=-1"):  # QD_ERR_INVALID
        opt.evalGradF_ensemble_model(alpha, [])
    assert _same_eval(before, opt.evalGradF(alpha))
    bad = make().system
    bad.transfreq[1] = np.nan
    with pytest.raises(capi.QuandaryAmdError, match=r"rc=-1"):
        opt.evalGradF_ensemble_model(alpha, [systems[0], bad])
    assert _same_eval(before, opt.evalGradF(alpha))
    with pytest.raises(capi.QuandaryAmdError, match=r"rc=-1"):
        opt.evalF_ensemble_model(alpha, systems, weights=[0.5, -0.5])
    assert _same_eval(before, opt.evalGradF(alpha))
    coupled_sys = make().system
    coupled_sys.Jkl[0] = 0.004
    with pytest.raises(capi.QuandaryAmdError, match=r"rc=-2"):  # QD_ERR_UNSUPPORTED
        opt.evalGradF_ensemble_model(alpha, [systems[0], coupled_sys])
    assert _same_eval(before, opt.evalGradF(alpha))
    mean, grad_mean, vals, grads = opt.evalGradF_ensemble_model(alpha, systems)  # ... and still shares launches
    assert opt.last_batch_sets == 2 and _same_eval(before, (vals[0], grads[0]))
    opt.close(); h.close()
