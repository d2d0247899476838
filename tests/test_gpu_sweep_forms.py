"""The four forms of a sweep - plain, SETS (parameter-set batch), VARS (model-parameter ensemble), SENS (model-constant sensitivities) -
interleaved on ONE handle per kernel family.  The host names the form once per plan (SweepPlan::form, qd_handle.h) and dispatches on
(family, form); the per-form tests each open a handle for one form, so a plan that carried the form of the call before would pass them
all.  Here every call must record the kernel of its own form (qd_last_kernel), and the results must be the bits of the single evaluation.

Systems: the smallest each family's per-form tests use (test_ensemble_model_cpu.model_spec / test_ensemble_lean_cpu.qubit_spec), 8 time
steps, three initial conditions.  Every comparison is bit for bit; no tolerance appears here."""
import numpy as np
import pytest

from helpers import OBJ_KEYS
from quandary_amd import capi
from test_ensemble_lean_cpu import qubit_spec
from test_ensemble_model_cpu import BLOCKS, model_spec, variant_specs

pytestmark = pytest.mark.gpu

NTIME = 8
GENERAL33 = "2, true, 1, false"  # <Q, LIND, VAR, QUBIT of the 3 x 3 Lindblad system (tests/test_ensemble_general_cpu.py)


def _general():
    return model_spec([3, 3], ntime=NTIME, options={"ensemble_general": "1"})


def _slot():
    return qubit_spec(4, False, ntime=NTIME, options={"batch_lean": "1", "ensemble_lean": "1"})


def _f32():
    sp = _slot()
    sp.precision = "f32mixed"
    return sp


def _col():
    return model_spec([3, 20], ntime=NTIME, options={"neumann_split": "1", "col_slices": "1", "batch_lean": "1"})


def _pair(fwd, adj=None):
    return fwd, (adj if adj is not None else fwd.replace("k_forward", "k_adjoint"))


# family: spec, then the (forward, adjoint) kernel names - or their beginnings - of the plain, SETS and VARS forms; sens: evalGradF_model
# runs (on the general family: the only one with k_adjoint_sens) or is refused (fp32-mixed: QD_ERR_UNSUPPORTED)
FAMILIES = {
    "general": dict(make=_general, plain=_pair(f"k_forward<{GENERAL33}, "), sets=_pair(f"k_forward<{GENERAL33}, "),
                    vars=_pair(f"k_forward_vars<{GENERAL33}, "), sens=True),
    "lean-slot": dict(make=_slot, plain=_pair("k_forward_q32<4, 0, double, false, false>"), sets=_pair("k_forward_q32_sets<4, 0, double, false, false>"),
                      vars=_pair("k_forward_q32_vars<4, 0, double, false, false>"), sens=True),
    "fp32-mixed": dict(make=_f32, plain=_pair("k_forward_q32<4, 0, float, false, false>"), sets=_pair("k_forward_q32_sets<4, 0, float, false, false>"),
                       vars=_pair("k_forward_q32_vars<4, 0, float, false, false>"), sens=False),
    "lean-column": dict(make=_col, plain=_pair("k_forward_col<2, 5, true, true, true, false>"),
                        sets=_pair("k_forward_col_sets<2, 5, true, true, true, false>"),
                        vars=_pair("k_forward_col_vars<2, 5, true, true, true, false>"), sens=True),
}


def _kernels(h):
    return h.last_kernel("forward"), h.last_kernel("adjoint")


def _ran_on(h, names, commas=None):
    """Both sweeps recorded the expected names (a beginning, where the name ends in arguments the case does not pin); commas: the number
    of commas of the general family's names - five for k_forward<...>, six with the SETS flag."""
    got = _kernels(h)
    ok = all(g.startswith(n) if n.endswith(", ") else g == n for g, n in zip(got, names))
    return ok and (commas is None or all(g.count(",") == commas for g in got))


def _same_eval(a, b):
    (va, ga), (vb, gb) = a, b
    return all(va[k] == vb[k] for k in OBJ_KEYS) and np.array_equal(ga, gb)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_forms_interleaved_on_one_handle(family):
    f = FAMILIES[family]
    general = family == "general"
    sp = f["make"]()
    assert sp.time.ntime == NTIME
    # variant 0: the handle's own constants; variant 1: every constant moved (tests/test_ensemble_model_cpu.py)
    systems = [s.system for s in variant_specs(f["make"], False, blocks=BLOCKS[:2])]
    alpha = 0.05 * np.random.default_rng(31).uniform(-1.0, 1.0, sp.params0.size)
    other = 0.3 * np.random.default_rng(32).uniform(-1.0, 1.0, sp.params0.size)
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    # 1. a single gradient
    first = opt.evalGradF(alpha)
    assert _ran_on(h, f["plain"], 5 if general else None), _kernels(h)
    # 2. a 2-set batch: set 0 has the controls of the single evaluation
    vals, grads = opt.evalGradF_batch(np.stack([alpha, other]))
    assert opt.last_batch_sets == 2
    assert _ran_on(h, f["sets"], 6 if general else None), _kernels(h)
    assert not general or all(k.endswith(", true>") for k in _kernels(h)), _kernels(h)
    assert _same_eval(first, (vals[0], grads[0]))
    assert not np.array_equal(grads[0], grads[1])
    # 3. a 2-variant model ensemble: variant 0 has the handle's own constants
    mean, grad_mean, evals, egrads = opt.evalGradF_ensemble_model(alpha, systems)
    assert opt.last_batch_sets == 2
    assert _ran_on(h, f["vars"], 5 if general else None), _kernels(h)
    assert _same_eval(first, (evals[0], egrads[0]))
    assert not np.array_equal(egrads[0], egrads[1])
    # 4. the sensitivity form, or its refusal
    if f["sens"]:
        val, grad, sens = opt.evalGradF_model(alpha)
        kf, ka = _kernels(h)
        assert kf.startswith("k_forward<") and ka.startswith("k_adjoint_sens<") and kf.count(",") == ka.count(",") == 5, (kf, ka)
        assert all(np.all(np.isfinite(sens[a])) for a in ("transfreq", "selfkerr", "crosskerr"))
    else:
        with pytest.raises(capi.QuandaryAmdError, match=r"rc=-2"):  # QD_ERR_UNSUPPORTED
            opt.evalGradF_model(alpha)
    # 5. the single gradient again: the plain form, the bits of the first
    last = opt.evalGradF(alpha)
    assert _ran_on(h, f["plain"], 5 if general else None), _kernels(h)
    assert _same_eval(first, last)
    opt.close(); h.close()


def test_dense_batch_records_the_sets_form():
    """A 2 x 2 user Hamiltonian keeps its matrices where the VARS form keeps its constants table (DevSys::hcr): a 2-set batch must run the
    SETS form, k_forward<..., true>, never a _vars kernel - and give the bits of the single evaluations before and after."""
    from test_gpu_param_batch_dense import _alphas, _dense_spec
    sp = _dense_spec([2, 2], lindblad=True, ntime=NTIME)
    alphas = _alphas(sp, (0.02, 0.1), seed=20240)
    h = capi.Handle(sp)
    opt = capi.Optim(h, sp)
    first = opt.evalGradF(alphas[0])
    assert _ran_on(h, _pair("k_forward<2, true, "), 5), _kernels(h)
    vals, grads = opt.evalGradF_batch(alphas)
    assert opt.last_batch_sets == 2
    assert _ran_on(h, _pair("k_forward<2, true, "), 6) and all(k.endswith(", true>") for k in _kernels(h)), _kernels(h)
    assert not any("_vars" in k for k in _kernels(h))
    assert _same_eval(first, (vals[0], grads[0]))
    assert _same_eval(first, opt.evalGradF(alphas[0]))
    assert _ran_on(h, _pair("k_forward<2, true, "), 5), _kernels(h)
    opt.close(); h.close()
