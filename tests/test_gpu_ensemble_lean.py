"""Model-parameter ensemble on the lean slot and fp32-mixed kernels (option ensemble_lean = 1): the variants of one call share launches
on k_forward_q32_vars / k_adjoint_q32_vars, which read one block of model constants per variant (qd_q32.hip with -DQD_VARS=1, the table
of qd_col_vars.h); qd_last_kernel names them with the five template arguments of the kernel the single evaluation on the same handle
runs on.  Without the option (the default), and on a Krylov plan, the call goes variant by variant as before.

Fixtures and their witness: tests/test_ensemble_lean_cpu.py (12 steps, three initial conditions, four blocks of constants).  The fp64
cases hold each variant against the oracle of a spec with that variant's constants through helpers.check_parity; the fp32-mixed cases
are compared bit for bit with the variant-by-variant call (ensemble_loop = 1: the handle pointed at one variant after the other, the plain
kernels) and with fresh fp32-mixed handles - their parity is what test_gpu_f32mixed.py asserts.  No new tolerance appears here."""
import numpy as np
import pytest

from helpers import GMRES_MODES, OBJ_KEYS, with_gmres_mode
from quandary_amd import capi
from test_ensemble_lean_cpu import qubit_spec
from test_ensemble_model_cpu import BLOCKS, oracle_grads, variant_specs
from test_gpu_ensemble import _fma_chain
from test_gpu_ensemble_model import _alpha, _kernels, _parity, _same_eval, _systems

pytestmark = pytest.mark.gpu

ON = {"ensemble_lean": "1"}


def _make(Q, coupled, options, precision=None, **kw):
    def make():
        sp = qubit_spec(Q, coupled, options=options, **kw)
        if precision:
            sp.precision = precision
        return sp
    return make


def _fixture(Q, coupled, options, nblocks=4, **kw):
    """(make, alpha, variant specs, the oracle's evaluation of every variant); make() gives the spec with the options."""
    make = _make(Q, coupled, options, **kw)
    specs = variant_specs(make, coupled, blocks=BLOCKS[:nblocks])
    alpha = _alpha(specs[0])
    ref = oracle_grads(specs, alpha)
    assert not np.allclose(ref[0][1], ref[1][1], rtol=1e-3), "the oracle's gradients of variants 0 and 1 do not differ"
    return make, alpha, specs, ref


def _names(prefix, args):
    return f"k_forward_{prefix}<{args}>", f"k_adjoint_{prefix}<{args}>"


def _twins(plain):
    """The variant twins of the plain lean slot kernels a single evaluation reported."""
    for n in plain:
        assert n.startswith(("k_forward_q32<", "k_adjoint_q32<")), n
    return tuple(n.replace("_q32<", "_q32_vars<") for n in plain)


def _same_call(a, b):
    (mean_a, gm_a, vals_a, grads_a), (mean_b, gm_b, vals_b, grads_b) = a, b
    return vals_a == vals_b and np.array_equal(grads_a, grads_b) and mean_a == mean_b and np.array_equal(gm_a, gm_b)


def _pattern_is_the_handles(sp, coupled):
    """A fresh handle of this variant picks the kernels of the ensemble's handle: coupled like it."""
    return coupled == any(j != 0.0 for j in sp.system.Jkl)


# qubits, coupled, extra options, "<Q, SB, R, GM, HJ>" of the kernels
SHAPES64 = [
    pytest.param(4, False, {}, "4, 0, double, false, false", id="2^4"),
    pytest.param(4, True, {}, "4, 0, double, false, true", id="2^4-coupled"),
    pytest.param(5, False, {}, "5, 1, double, false, false", id="2^5"),  # twelve states of the launch: two elements per thread
    pytest.param(5, False, {"lean64_sb": "2"}, "5, 2, double, false, false", id="2^5-sb2"),
    pytest.param(5, True, {}, "5, 1, double, false, true", id="2^5-coupled"),
]


@pytest.mark.parametrize("Q,coupled,options,args", SHAPES64)
def test_every_instantiation_fp64(Q, coupled, options, args):
    """1. Four variants in one launch on the twins of the kernels the single evaluation runs on; every variant against the oracle of its
    own spec; variant 2 (a copy of block 0) bit for bit variant 0; the handle's own evaluation before and after identical and variant 0."""
    make, alpha, specs, ref = _fixture(Q, coupled, {**options, **ON})
    h = capi.Handle(make())
    opt = capi.Optim(h, h.spec)
    assert opt.ninit == 3
    before = opt.evalGradF(alpha)
    plain = _kernels(h)
    assert plain == _names("q32", args), plain
    mean, grad_mean, vals, grads = opt.evalGradF_ensemble_model(alpha, _systems(specs))
    assert opt.last_batch_sets == 4
    assert _kernels(h) == _twins(plain) == _names("q32_vars", args), _kernels(h)
    _parity(specs, alpha, vals, grads, ref)
    assert _same_eval((vals[0], grads[0]), (vals[2], grads[2]))
    after = opt.evalGradF(alpha)
    assert _kernels(h) == plain
    assert _same_eval(before, after) and _same_eval(before, (vals[0], grads[0]))
    opt.close(); h.close()


@pytest.mark.parametrize("coupled", [pytest.param(False, id="2^4"), pytest.param(True, id="2^4-coupled")])
def test_neumann_request_is_fresh_handles_the_loop_and_the_default(coupled):
    """2. A neumann request: the shared call is bit for bit the same call under ensemble_loop = 1, the same call under ensemble_lean = 0 and
    evalGradF on fresh handles created from each variant's spec (the block with every coupling zero: a fresh handle would pick the
    uncoupled kernel - that block is compared with the loop only)."""
    make, alpha, specs, ref = _fixture(4, coupled, ON, linsolve="neumann")
    h = capi.Handle(make())
    opt = capi.Optim(h, h.spec)
    shared_call = opt.evalGradF_ensemble_model(alpha, _systems(specs))
    assert opt.last_batch_sets == 4
    shared = _kernels(h)
    assert shared == _names("q32_vars", f"4, 0, double, false, {'true' if coupled else 'false'}"), shared
    for key in ("ensemble_loop", "ensemble_lean"):
        h.set_option(key, "1" if key == "ensemble_loop" else "0")
        other = opt.evalGradF_ensemble_model(alpha, _systems(specs))
        assert opt.last_batch_sets == 1 and _twins(_kernels(h)) == shared, (key, _kernels(h))
        assert _same_call(other, shared_call), key
        h.set_option(key, "0" if key == "ensemble_loop" else "1")
    opt.close(); h.close()
    mean, grad_mean, vals, grads = shared_call
    compared = 0
    for j, sp in enumerate(specs):
        if not _pattern_is_the_handles(sp, coupled):
            continue
        hj = capi.Handle(sp)
        oj = capi.Optim(hj, sp)
        fresh = oj.evalGradF(alpha)
        print(j, vals[j]["objective"], fresh[0]["objective"], np.linalg.norm(grads[j] - fresh[1]))
        assert _twins(_kernels(hj)) == shared
        assert _same_eval((vals[j], grads[j]), fresh), j
        oj.close(); hj.close()
        compared += 1
    assert compared == (3 if coupled else 4)


SHAPES32 = [
    pytest.param(3, False, {}, "3, 0, float, false, false", id="2x2x2"),
    pytest.param(4, False, {}, "4, 0, float, false, false", id="2^4"),
    pytest.param(5, False, {}, "5, 1, float, false, false", id="2^5"),
    pytest.param(5, False, {"lean64_sb": "2"}, "5, 2, float, false, false", id="2^5-sb2"),
    pytest.param(4, True, {}, "4, 0, float, false, true", id="2^4-coupled"),
    pytest.param(5, True, {}, "5, 1, float, false, true", id="2^5-coupled"),
]


def _f32_specs(Q, coupled, options):
    make = _make(Q, coupled, options, precision="f32mixed")
    specs = variant_specs(make, coupled)
    return make, _alpha(specs[0]), specs


def _f32_against_fresh_handles(specs, coupled, alpha, vals, grads, kernels):
    for j, sp in enumerate(specs):
        if not _pattern_is_the_handles(sp, coupled):
            continue
        hj = capi.Handle(sp)
        oj = capi.Optim(hj, sp)
        fresh = oj.evalGradF(alpha)
        print(j, vals[j]["objective"], fresh[0]["objective"], np.linalg.norm(grads[j] - fresh[1]))
        assert _kernels(hj) == kernels, _kernels(hj)
        assert _same_eval((vals[j], grads[j]), fresh), j
        oj.close(); hj.close()


@pytest.mark.parametrize("Q,coupled,options,args", SHAPES32)
def test_every_instantiation_f32mixed(Q, coupled, options, args):
    """3. fp32-mixed: the shared call on the float twins is bit for bit the ensemble_loop = 1 call on the same handle - which reaches the
    constants through the plain kernels, so a kernel that read another variant's block cannot pass - and, for blocks whose coupling
    pattern is the handle's, fresh fp32-mixed handles.  Variants 0 and 1 differ, variant 2 equals variant 0."""
    make, alpha, specs = _f32_specs(Q, coupled, {**options, **ON})
    h = capi.Handle(make())
    opt = capi.Optim(h, h.spec)
    assert opt.ninit == 3
    before = opt.evalGradF(alpha)
    plain = _kernels(h)
    assert plain == _names("q32", args), plain
    shared_call = opt.evalGradF_ensemble_model(alpha, _systems(specs))
    assert opt.last_batch_sets == 4
    assert _kernels(h) == _names("q32_vars", args), _kernels(h)
    mean, grad_mean, vals, grads = shared_call
    assert not np.allclose(grads[0], grads[1], rtol=1e-3)
    assert _same_eval((vals[0], grads[0]), (vals[2], grads[2]))
    assert _same_eval(before, (vals[0], grads[0])) and _same_eval(before, opt.evalGradF(alpha))
    h.set_option("ensemble_loop", "1")
    loop_call = opt.evalGradF_ensemble_model(alpha, _systems(specs))
    assert opt.last_batch_sets == 1 and _kernels(h) == plain, _kernels(h)
    assert _same_call(loop_call, shared_call)
    opt.close(); h.close()
    _f32_against_fresh_handles(specs, coupled, alpha, vals, grads, plain)


@pytest.mark.parametrize("Q,coupled,args", [pytest.param(3, False, "3, 0, float, false, false", id="2x2x2"),
                                            pytest.param(4, True, "4, 0, float, false, true", id="2^4-coupled")])
def test_f32mixed_without_the_option_goes_variant_by_variant(Q, coupled, args):
    """3 (continued). The default: the same fp32-mixed call variant by variant on the plain kernels, bit for bit fresh handles (passes with
    and without the feature)."""
    make, alpha, specs = _f32_specs(Q, coupled, {})
    h = capi.Handle(make())
    opt = capi.Optim(h, h.spec)
    mean, grad_mean, vals, grads = opt.evalGradF_ensemble_model(alpha, _systems(specs))
    assert opt.last_batch_sets == 1
    assert _kernels(h) == _names("q32", args), _kernels(h)
    assert not np.allclose(grads[0], grads[1], rtol=1e-3)
    assert _same_eval((vals[0], grads[0]), (vals[2], grads[2]))
    opt.close(); h.close()
    _f32_against_fresh_handles(specs, coupled, alpha, vals, grads, _names("q32", args))


@pytest.mark.parametrize("mode", GMRES_MODES)
def test_gmres_request(mode):
    """4. linearsolver_type = gmres on 2^4.  auto: the Neumann stand-in shares the launch and is held to the oracle with any_solver; it is
    bit for bit the loop where last_solver and the kernel names of both calls agree (the shared plan comes from the row bounds maximised
    over the variants, a variant's own plan in the loop from its own).  gmres_split = 0: a Krylov plan has no variants form - variant by
    variant on the plain Krylov kernels, the results of the same call on a handle without the option bit for bit."""
    make, alpha, specs, ref = _fixture(4, False, ON, nblocks=3, linsolve="gmres")
    sp = with_gmres_mode(make(), mode)
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    call = opt.evalGradF_ensemble_model(alpha, _systems(specs))
    mean, grad_mean, vals, grads = call
    kernels, solver, nsets = _kernels(h), h.last_solver, opt.last_batch_sets
    print(mode, kernels, solver, nsets)
    _parity(specs, alpha, vals, grads, ref, any_solver=True)
    assert _same_eval((vals[0], grads[0]), (vals[2], grads[2]))
    if mode == "0":
        assert nsets == 1 and solver == "krylov"
        assert kernels == _names("q32", "4, 0, double, true, false"), kernels
        # (the degree tuner of the Krylov kernels moves over a handle's first sweeps: the comparator is the first call of a handle too)
        sp_off = with_gmres_mode(_make(4, False, {}, linsolve="gmres")(), mode)
        h_off = capi.Handle(sp_off)
        opt_off = capi.Optim(h_off, sp_off)
        off = opt_off.evalGradF_ensemble_model(alpha, _systems(specs))
        assert opt_off.last_batch_sets == 1 and _kernels(h_off) == kernels
        assert _same_call(off, call)
        opt_off.close(); h_off.close()
    else:
        assert nsets == 3
        assert kernels == _names("q32_vars", "4, 0, double, false, false"), kernels
        h.set_option("ensemble_loop", "1")
        loop = opt.evalGradF_ensemble_model(alpha, _systems(specs))
        assert opt.last_batch_sets == 1
        _parity(specs, alpha, loop[2], loop[3], ref, any_solver=True)
        if h.last_solver == solver and _twins(_kernels(h)) == kernels:
            assert loop[2] == vals and np.array_equal(loop[3], grads)
    opt.close(); h.close()


def test_weights_mean_forward_only_and_groups():
    """5. Five weighted variants on 2^4: the fma chain of k_ensemble_mean; per_variant = False gives the same mean bits; the forward-only
    call gives the same values; under a trajectory budget that holds three variants the groups are three and two and the results those
    of the ungrouped call."""
    make, alpha, specs, ref = _fixture(4, False, ON)
    systems = _systems(specs)
    five = systems + [systems[1]]
    w5 = np.array([0.3, 0.1, 0.2, 0.15, 0.25])
    h = capi.Handle(make())
    opt = capi.Optim(h, h.spec)
    assert opt.ninit == 3
    mean5, grad_mean5, vals5, grads5 = opt.evalGradF_ensemble_model(alpha, five, weights=w5)
    assert opt.last_batch_sets == 5 and _kernels(h) == _names("q32_vars", "4, 0, double, false, false"), _kernels(h)
    _parity(specs, alpha, vals5[:4], grads5[:4], ref)
    assert _same_eval((vals5[1], grads5[1]), (vals5[4], grads5[4]))
    assert np.array_equal(grad_mean5, _fma_chain(w5, grads5))
    chain = _fma_chain(w5, np.array([[v[k] for k in OBJ_KEYS] for v in vals5]))
    assert [mean5[k] for k in OBJ_KEYS] == list(chain)
    mean_o, grad_mean_o, vals_o, none = opt.evalGradF_ensemble_model(alpha, five, weights=w5, per_variant=False)
    assert none is None and vals_o == vals5 and mean_o == mean5 and np.array_equal(grad_mean_o, grad_mean5)
    fmean, fvals = opt.evalF_ensemble_model(alpha, five, weights=w5)
    assert opt.last_batch_sets == 5 and h.last_kernel("forward") == "k_forward_q32_vars<4, 0, double, false, false>"
    assert fvals == vals5 and fmean == mean5
    nt = h.spec.time.ntime
    traj = (2 * nt + 1) * opt.ninit * 2 * h.dim * 8  # states and primal stages of one variant, bytes
    h.set_option("traj_budget_mb", 3.5 * traj / 1048576.0)
    mean_g, grad_mean_g, vals_g, grads_g = opt.evalGradF_ensemble_model(alpha, five, weights=w5)
    assert opt.last_batch_sets == 3, opt.last_batch_sets
    assert vals_g == vals5 and np.array_equal(grads_g, grads5) and mean_g == mean5 and np.array_equal(grad_mean_g, grad_mean5)
    opt.close(); h.close()


def test_errors_leave_the_handle_usable():
    """6. A coupling on an uncoupled 2^4 handle: QD_ERR_UNSUPPORTED; a NaN constant: QD_ERR_INVALID.  The handle evaluates bit-identically
    after each, and still shares launches."""
    make = _make(4, False, ON)
    specs = variant_specs(make, False, blocks=BLOCKS[:2])
    systems = _systems(specs)
    alpha = _alpha(specs[0])
    h = capi.Handle(make())
    opt = capi.Optim(h, h.spec)
    before = opt.evalGradF(alpha)
    coupled_sys = make().system
    coupled_sys.Jkl[0] = 0.004
    with pytest.raises(capi.QuandaryAmdError, match=r"rc=-2"):  # QD_ERR_UNSUPPORTED
        opt.evalGradF_ensemble_model(alpha, [systems[0], coupled_sys])
    assert _same_eval(before, opt.evalGradF(alpha))
    bad = make().system
    bad.transfreq[1] = np.nan
    with pytest.raises(capi.QuandaryAmdError, match=r"rc=-1"):  # QD_ERR_INVALID
        opt.evalGradF_ensemble_model(alpha, [systems[0], bad])
    assert _same_eval(before, opt.evalGradF(alpha))
    mean, grad_mean, vals, grads = opt.evalGradF_ensemble_model(alpha, systems)
    assert opt.last_batch_sets == 2 and _kernels(h) == _names("q32_vars", "4, 0, double, false, false")
    assert _same_eval(before, (vals[0], grads[0]))
    opt.close(); h.close()
