"""Model-parameter ensemble (qd_optim_evalF_ensemble_model / qd_optim_evalGradF_ensemble_model): one control vector on variants of the
standard model's transition frequencies, Kerr coefficients and couplings.  Where the plan's sweep is a diagonal-split stationary
iteration of the lean column family the variants share launches on k_*_col_vars / k_*_colj_vars, which read one block of model constants
per variant; qd_last_kernel names them with the six template arguments of the kernel the single evaluation runs on.  Everything else goes
variant by variant.

Fixtures and their witness: tests/test_ensemble_model_cpu.py (12 steps of 0.002 ns, every penalty, the gate trace on the three `3states`
initial conditions; four blocks of constants, block 2 a copy of block 0, so four variants over three states do not divide evenly either
way).  Before any GPU assertion the oracle's gradients of variants 0 and 1 are asserted to differ; each variant is held against the
oracle of a spec with that variant's constants through helpers.check_parity: no new tolerance appears here."""
import numpy as np
import pytest

from helpers import GMRES_MODES, OBJ_KEYS, check_parity, with_gmres_mode
from quandary_amd import capi
from test_ensemble_model_cpu import BLOCKS, model_spec, oracle_grads, variant_specs
from test_gpu_ensemble import _dense_spec, _fma_chain

pytestmark = pytest.mark.gpu

SPLIT = {"neumann_split": "1", "col_slices": "1"}


def _alpha(sp, amp=0.05, seed=31):
    return amp * np.random.default_rng(seed).uniform(-1.0, 1.0, sp.params0.size)


def _fixture(nlevels, coupled, options=SPLIT, nblocks=4, **kw):
    """(make, alpha, variant specs, the oracle's evaluation of every variant)."""
    def make():
        return model_spec(nlevels, options=options, **kw)
    specs = variant_specs(make, coupled, blocks=BLOCKS[:nblocks])
    alpha = _alpha(specs[0])
    ref = oracle_grads(specs, alpha)
    assert not np.allclose(ref[0][1], ref[1][1], rtol=1e-3), "the oracle's gradients of variants 0 and 1 do not differ"
    return make, alpha, specs, ref


def _systems(specs):
    return [sp.system for sp in specs]


def _kernels(h):
    return h.last_kernel("forward"), h.last_kernel("adjoint")


def _vars_names(plain):
    """The variant twins of the plain kernels a single evaluation reported: the same template arguments under the _vars name."""
    for n in plain:
        assert "_vars<" not in n and ("_col<" in n or "_colj<" in n), n
    return tuple(n.replace("_col<", "_col_vars<").replace("_colj<", "_colj_vars<") for n in plain)


def _same_eval(a, b):
    (va, ga), (vb, gb) = a, b
    return all(va[k] == vb[k] for k in OBJ_KEYS) and np.array_equal(ga, gb)


def _parity(specs, alpha, vals, grads, ref, **kw):
    for j, sp in enumerate(specs):
        print(j, vals[j]["objective"], ref[j][0]["objective"], np.linalg.norm(grads[j] - ref[j][1]) / np.linalg.norm(ref[j][1]))
        check_parity(sp, vals[j], grads[j], *ref[j], alpha=alpha, msg=j, **kw)


def _compute_units():
    """Compute units of device 0 from the HIP runtime (hipDeviceGetAttribute; the wavefront size is asked too, as a check that the
    attribute numbers are those of the installed runtime)."""
    import ctypes as C
    import os
    hip = None
    for name in ("libamdhip64.so", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so")):
        try:
            hip = C.CDLL(name)
            break
        except OSError:
            continue
    assert hip is not None, "libamdhip64.so not found"
    MULTIPROCESSOR_COUNT, WARP_SIZE = 63, 87  # hipDeviceAttribute_t of hip_runtime_api.h
    cus, warp = C.c_int(0), C.c_int(0)
    assert hip.hipDeviceGetAttribute(C.byref(warp), WARP_SIZE, 0) == 0 and warp.value == 64, warp.value
    assert hip.hipDeviceGetAttribute(C.byref(cus), MULTIPROCESSOR_COUNT, 0) == 0 and 16 <= cus.value <= 1024, cus.value
    return cus.value


# ---- the 3 x 20 system of cases 1, 3 and 4: the oracle asked once for the four blocks ---------------------------------------------------
@pytest.fixture(scope="module")
def c320():
    return _fixture([3, 20], False)


@pytest.fixture(scope="module")
def c320_call(c320):
    """Case 1's four-variant call, kept for the cases that compare with it: (vals, grads, mean, grad_mean, kernels)."""
    make, alpha, specs, ref = c320
    h = capi.Handle(make())
    opt = capi.Optim(h, h.spec)
    mean, grad_mean, vals, grads = opt.evalGradF_ensemble_model(alpha, _systems(specs))
    out = (vals, grads, mean, grad_mean, _kernels(h), opt.last_batch_sets)
    opt.close(); h.close()
    return out


def test_headline_twin_is_identical_to_fresh_handles_and_to_the_loop(c320, c320_call):
    """1. 3 x 20, neumann request, neumann_split = 1: four variants in one launch on the twin of the headline kernel; values and gradients
    bit for bit those of evalGradF on fresh handles created from each variant's spec and those of the same call under ensemble_loop = 1;
    the handle's own evaluation before and after is identical."""
    make, alpha, specs, ref = c320
    vals, grads, mean, grad_mean, kernels, nsets = c320_call
    assert nsets == 4
    assert kernels == ("k_forward_col_vars<2, 5, true, true, true, false>", "k_adjoint_col_vars<2, 5, true, true, true, false>"), kernels
    h = capi.Handle(make())
    opt = capi.Optim(h, h.spec)
    assert opt.ninit == 3
    before = opt.evalGradF(alpha)
    assert kernels == _vars_names(_kernels(h))
    again = opt.evalGradF_ensemble_model(alpha, _systems(specs))
    assert opt.last_batch_sets == 4 and _kernels(h) == kernels
    assert again[2] == vals and np.array_equal(again[3], grads) and again[0] == mean and np.array_equal(again[1], grad_mean)
    assert _same_eval(before, opt.evalGradF(alpha))
    assert _same_eval(before, (vals[0], grads[0]))  # (block 0 is the handle's own system)
    h.set_option("ensemble_loop", "1")
    mean_l, grad_mean_l, vals_l, grads_l = opt.evalGradF_ensemble_model(alpha, _systems(specs))
    assert opt.last_batch_sets == 1 and _vars_names(_kernels(h)) == kernels
    assert vals_l == vals and np.array_equal(grads_l, grads) and mean_l == mean
    assert np.array_equal(grad_mean_l, grad_mean)
    assert _same_eval(before, opt.evalGradF(alpha))
    opt.close(); h.close()
    for j, sp in enumerate(specs):
        hj = capi.Handle(sp)
        oj = capi.Optim(hj, sp)
        fresh = oj.evalGradF(alpha)
        print(j, vals[j]["objective"], fresh[0]["objective"], np.linalg.norm(grads[j] - fresh[1]))
        assert _vars_names(_kernels(hj)) == kernels
        assert _same_eval((vals[j], grads[j]), fresh), j
        oj.close(); hj.close()
    assert _same_eval((vals[0], grads[0]), (vals[2], grads[2]))
    _parity(specs, alpha, vals, grads, ref)


# <Q, EPT, SPLIT, USLOT, SKIP, KRY> as in tests/test_gpu_param_batch_col.py::SHAPES
SHAPES = [
    pytest.param([5, 7], {}, False, "_col", "2, 5, true, false, true, false", id="5x7-N35"),
    pytest.param([8, 8], {}, False, "_col", "2, 8, true, true, true, false", id="8x8-N64"),
    pytest.param([7, 9], dict(detuned=True), False, "_col", "2, 8, true, false, true, false", id="7x9-N63"),
    pytest.param([3, 3, 5], {}, False, "_col", "3, 5, true, true, true, false", id="3x3x5-N45"),
    pytest.param([3, 20], dict(jkl=0.004, detuned=True), True, "_colj", "2, 5, true, true, false, false", id="3x20-coupled"),
    pytest.param([4, 4, 4], dict(jkl=0.004), True, "_colj", "3, 8, true, false, false, false", id="4x4x4-coupled"),
]


@pytest.mark.parametrize("nlevels,kw,coupled,family,args", SHAPES)
def test_every_shape(nlevels, kw, coupled, family, args):
    """2. Every variant differs in all arrays that apply (pair-wise different crosskerr; Jkl on the coupled systems, the last variant with
    every coupling zero)."""
    make, alpha, specs, ref = _fixture(nlevels, coupled, **kw)
    h = capi.Handle(make())
    opt = capi.Optim(h, h.spec)
    assert opt.ninit <= 8
    mean, grad_mean, vals, grads = opt.evalGradF_ensemble_model(alpha, _systems(specs))
    assert opt.last_batch_sets == 4
    assert _kernels(h) == (f"k_forward{family}_vars<{args}>", f"k_adjoint{family}_vars<{args}>"), _kernels(h)
    _parity(specs, alpha, vals, grads, ref)
    assert _same_eval((vals[0], grads[0]), (vals[2], grads[2]))
    single = opt.evalGradF(alpha)
    assert _vars_names(_kernels(h)) == (f"k_forward{family}_vars<{args}>", f"k_adjoint{family}_vars<{args}>")
    assert _same_eval(single, (vals[0], grads[0]))
    opt.close(); h.close()


def test_a_workgroup_that_changes_variant(c320, c320_call):
    """3. 64 variants cycling through the four blocks x 3 states x 3 time slices: more tasks than twice the compute units, so a resident
    workgroup draws tasks of different variants.  Variant j is bit for bit variant j % 4 of case 1's call, and the sliced call the
    unsliced one.

    (A sliced launch of these kernels carries every thread's penalty sum from slice to slice and reduces it once, so the penalty too
    has the bits of the unsliced sweep.)"""
    make, alpha, specs, ref = c320
    vals4, grads4 = c320_call[0], c320_call[1]
    systems = [_systems(specs)[j % 4] for j in range(64)]
    cus = _compute_units()
    out = {}
    for slices in ("3", "1"):
        h = capi.Handle(model_spec([3, 20], options={**SPLIT, "col_slices": slices}))
        opt = capi.Optim(h, h.spec)
        if slices == "3":
            assert 64 * opt.ninit * 3 > 2 * cus, cus
        mean, grad_mean, vals, grads = opt.evalGradF_ensemble_model(alpha, systems)
        assert opt.last_batch_sets == 64 and _kernels(h)[0] == "k_forward_col_vars<2, 5, true, true, true, false>", _kernels(h)
        out[slices] = (mean, grad_mean, vals, grads)
        opt.close(); h.close()
    mean, grad_mean, vals, grads = out["3"]
    for j in range(64):
        assert _same_eval((vals[j], grads[j]), (vals4[j % 4], grads4[j % 4])), j
    assert out["1"][2] == vals and np.array_equal(out["1"][3], grads) and out["1"][0] == mean and np.array_equal(out["1"][1], grad_mean)
    _parity(specs, alpha, vals[:4], grads[:4], ref)


def test_coupled_sliced_call_is_the_unsliced_one():
    """3 (continued). The coupled kernels, whose Jtrace penalty has a uniform part of its own that is carried between the slices too:
    four variants x 3 states x 3 time slices against the unsliced call, bit for bit."""
    make, alpha, specs, ref = _fixture([3, 20], True, jkl=0.004, detuned=True)
    out = {}
    for slices in ("3", "1"):
        h = capi.Handle(model_spec([3, 20], options={**SPLIT, "col_slices": slices}, jkl=0.004, detuned=True))
        opt = capi.Optim(h, h.spec)
        out[slices] = opt.evalGradF_ensemble_model(alpha, _systems(specs))
        assert opt.last_batch_sets == 4 and _kernels(h)[0] == "k_forward_colj_vars<2, 5, true, true, false, false>", _kernels(h)
        opt.close(); h.close()
    assert out["3"][2] == out["1"][2] and np.array_equal(out["3"][3], out["1"][3])
    assert out["3"][0] == out["1"][0] and np.array_equal(out["3"][1], out["1"][1])
    _parity(specs, alpha, out["3"][2], out["3"][3], ref)


def test_weights_mean_forward_only_and_groups(c320, c320_call):
    """4. Weights as given, None = 1 / nvar; per_variant = False gives the same mean bits; the fma chain of k_ensemble_mean; the
    forward-only call; five variants under a trajectory budget that holds three."""
    make, alpha, specs, ref = c320
    systems = _systems(specs)
    vals4, grads4, mean4, grad_mean4 = c320_call[:4]
    h = capi.Handle(make())
    opt = capi.Optim(h, h.spec)
    w = np.array([0.1, 0.2, 0.3, 0.4])
    mean, grad_mean, vals, grads = opt.evalGradF_ensemble_model(alpha, systems, weights=w)
    assert vals == vals4 and np.array_equal(grads, grads4)
    assert np.array_equal(grad_mean, _fma_chain(w, grads))
    chain = _fma_chain(w, np.array([[v[k] for k in OBJ_KEYS] for v in vals]))  # (the host forms every field of the mean the same way)
    assert [mean[k] for k in OBJ_KEYS] == list(chain)
    quarter = opt.evalGradF_ensemble_model(alpha, systems, weights=[0.25] * 4)
    assert quarter[0] == mean4 and np.array_equal(quarter[1], grad_mean4)  # None = 1 / nvar
    assert np.array_equal(grad_mean4, _fma_chain([0.25] * 4, grads4))
    mean_o, grad_mean_o, vals_o, none = opt.evalGradF_ensemble_model(alpha, systems, weights=w, per_variant=False)
    assert none is None and vals_o == vals and mean_o == mean and np.array_equal(grad_mean_o, grad_mean)
    fmean, fvals = opt.evalF_ensemble_model(alpha, systems, weights=w)
    assert opt.last_batch_sets == 4 and fvals == vals and fmean == mean
    # five variants, groups of three and two
    five = systems + [systems[1]]
    w5 = np.array([0.3, 0.1, 0.2, 0.15, 0.25])
    mean5, grad_mean5, vals5, grads5 = opt.evalGradF_ensemble_model(alpha, five, weights=w5)
    assert opt.last_batch_sets == 5
    nt = h.spec.time.ntime
    traj = (2 * nt + 1) * opt.ninit * 2 * h.dim * 8  # states and primal stages of one variant, bytes
    gauge = nt * 136 * 8                              # one row of the phasor table per step
    h.set_option("traj_budget_mb", 3.5 * (traj + gauge) / 1048576.0)
    mean_g, grad_mean_g, vals_g, grads_g = opt.evalGradF_ensemble_model(alpha, five, weights=w5)
    assert opt.last_batch_sets == 3, opt.last_batch_sets
    assert vals_g == vals5 and np.array_equal(grads_g, grads5) and mean_g == mean5 and np.array_equal(grad_mean_g, grad_mean5)
    assert np.array_equal(grad_mean5, _fma_chain(w5, grads5))
    opt.close(); h.close()


@pytest.mark.parametrize("mode", GMRES_MODES)
def test_gmres_request(mode):
    """5. A gmres request: the stand-in shares the launch, the Krylov kernels (gmres_split = 0) go variant by variant."""
    make, alpha, specs, ref = _fixture([3, 20], False, options={"col_slices": "1"}, nblocks=2, linsolve="gmres")
    sp = with_gmres_mode(make(), mode)
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    mean, grad_mean, vals, grads = opt.evalGradF_ensemble_model(alpha, _systems(specs))
    print(mode, _kernels(h), h.last_solver, opt.last_batch_sets)
    if mode == "0":
        assert opt.last_batch_sets == 1 and h.last_solver == "krylov", (opt.last_batch_sets, h.last_solver)
        assert _kernels(h)[0] == "k_forward_col<2, 5, true, true, false, true>", _kernels(h)
    else:
        assert opt.last_batch_sets == 2 and _kernels(h)[0].startswith("k_forward_col_vars<2, 5, true, true, "), _kernels(h)
    _parity(specs, alpha, vals, grads, ref, any_solver=True)
    assert np.array_equal(grad_mean, _fma_chain([0.5, 0.5], grads))
    opt.close(); h.close()


def test_plain_neumann_plan_goes_variant_by_variant():
    """5 (continued). neumann_split = 0: no variant form of the plain iteration."""
    make, alpha, specs, ref = _fixture([3, 20], False, options={"neumann_split": "0", "col_slices": "1"}, nblocks=2)
    h = capi.Handle(make())
    opt = capi.Optim(h, h.spec)
    mean, grad_mean, vals, grads = opt.evalGradF_ensemble_model(alpha, _systems(specs))
    assert opt.last_batch_sets == 1 and _kernels(h)[0] == "k_forward_col<2, 5, false, true, true, false>", _kernels(h)
    _parity(specs, alpha, vals, grads, ref)
    opt.close(); h.close()


FALLBACK = [
    pytest.param([2, 2], dict(lindblad=False, init="basis"), {}, None, "k_forward<", id="2x2-schroedinger-general"),
    pytest.param([2, 2, 2, 2], dict(nessential=[2, 2, 2, 2]), {}, None, "k_forward_q32<", id="2^4-lindblad-slot"),  # (all levels essential: the lean slot kernels)
    pytest.param([2, 2], {}, {}, "16", "k_forward_big<", id="2x2-lindblad-global"),
    pytest.param([3, 20], {}, {"no_collean": "1"}, None, "k_forward<", id="3x20-no_collean"),
]


@pytest.mark.parametrize("nlevels,kw,options,var,kernel", FALLBACK)
def test_other_families_go_variant_by_variant(monkeypatch, nlevels, kw, options, var, kernel):
    """6. Two variants on the families without a variant form: the numbers of a handle of each variant, one launch per variant, and
    the handle's own evaluation untouched (global-memory kernels: the element table is rebuilt and restored)."""
    if var is not None:
        monkeypatch.setenv("QD_VAR", var)
    make, alpha, specs, ref = _fixture(nlevels, False, options=options, nblocks=2, **kw)
    h = capi.Handle(make())
    opt = capi.Optim(h, h.spec)
    assert opt.ninit <= 8
    before = opt.evalGradF(alpha)
    w = np.array([0.3, 0.7])
    mean, grad_mean, vals, grads = opt.evalGradF_ensemble_model(alpha, _systems(specs), weights=w)
    assert opt.last_batch_sets == 1
    assert h.last_kernel("forward").startswith(kernel), h.last_kernel("forward")
    _parity(specs, alpha, vals, grads, ref)
    assert np.array_equal(grad_mean, _fma_chain(w, grads))
    assert _same_eval(before, (vals[0], grads[0]))
    assert _same_eval(before, opt.evalGradF(alpha))
    opt.close(); h.close()
    h1 = capi.Handle(specs[1])
    o1 = capi.Optim(h1, specs[1])
    assert _same_eval(o1.evalGradF(alpha), (vals[1], grads[1]))
    o1.close(); h1.close()


def test_errors_leave_the_handle_usable():
    """7. A user-Hamiltonian handle: QD_ERR_STATE; nvar = 0, a NaN constant, a negative weight: QD_ERR_INVALID; a coupling on an
    uncoupled handle: QD_ERR_UNSUPPORTED.  The handle evaluates normally after each."""
    def make():
        return model_spec([3, 20], options=SPLIT)
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
    coupled = make().system
    coupled.Jkl[0] = 0.004
    with pytest.raises(capi.QuandaryAmdError, match=r"rc=-2"):  # QD_ERR_UNSUPPORTED
        opt.evalGradF_ensemble_model(alpha, [systems[0], coupled])
    assert _same_eval(before, opt.evalGradF(alpha))
    opt.close(); h.close()
    # a user-Hamiltonian handle has no model constants
    sp = _dense_spec([2, 2], lindblad=True)
    a = _alpha(sp, amp=0.3)
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    before = opt.evalGradF(a)
    with pytest.raises(capi.QuandaryAmdError, match=r"rc=-5"):  # QD_ERR_STATE
        opt.evalGradF_ensemble_model(a, [sp.system, sp.system])
    with pytest.raises(capi.QuandaryAmdError, match=r"rc=-5"):
        opt.evalF_ensemble_model(a, [sp.system, sp.system])
    assert _same_eval(before, opt.evalGradF(a))
    opt.close(); h.close()
