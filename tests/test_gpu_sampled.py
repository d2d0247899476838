"""Sampled controls (qd_optim_evalF_sampled / qd_optim_evalGradF_sampled): the objective and d objective / d sample with p_k, q_k given
as samples - one per control-table row ('rows'), zero-order hold ('hold') or linear interpolation ('linear').

One handle per kernel family, so that the table filled from samples is read wherever a family derives something from it: general (3x3
Schroedinger), lean slot (2^4 Lindblad), lean column with its phasor table (3x20 Lindblad), dense (4x4 Lindblad user Hamiltonian, whose
G(t) table is built from the control table), and the 3x3 system under IMR4, whose table has three rows per step at non-uniform times.
gamma_tik, the variation and the energy penalty are 0; the leakage / weighted and dpdm penalties are on as helpers.synthetic_cfg(penalties
= True) sets them for the parity tests.

Tolerances: objective parts rel 1e-7, abs 1e-12 - what tests/test_gpu_parity.py holds the GPU to against the oracle; gradients 1e-8 of
the norm, the project's gradient tolerance (helpers.check_parity)."""
import numpy as np
import pytest

from helpers import OBJ_KEYS, REF_RTOL, synthetic_spec
from quandary_amd import capi
from quandary_amd.models import standard_hamiltonians

pytestmark = pytest.mark.gpu


def _plain(sp):
    """no term that is defined on alpha or on a time grid the samples do not have"""
    sp.objective.gamma_tik = 0.0
    sp.objective.gamma_penalty_variation = 0.0
    sp.objective.penalty.gamma_penalty_energy = 0.0
    return sp


def _spec(name, **over):
    if name == "general":
        kw = dict(nlevels=[3, 3], lindblad=False, ntime=20, penalties=True, nessential=[2, 2])
    elif name == "imr4":
        kw = dict(nlevels=[3, 3], lindblad=False, ntime=20, penalties=True, nessential=[2, 2], stepper="IMR4")
    elif name == "slot":
        kw = dict(nlevels=[2, 2, 2, 2], lindblad=True, ntime=10, init="3states", penalties=True)
    elif name == "column":
        kw = dict(nlevels=[3, 20], lindblad=True, ntime=12, init="diagonal, 0", target="pure", objective="Jmeasure",
                  nessential=[2, 20], penalties=True)
    elif name == "dense":
        kw = dict(nlevels=[4, 4], lindblad=True, ntime=10, init="diagonal, 0", target="pure", objective="Jmeasure", penalties=True)
    else:
        raise KeyError(name)
    kw.update(over)
    nl = kw.pop("nlevels")
    sp = _plain(synthetic_spec(nl, **kw))
    if name == "dense":
        sp.hamiltonian = standard_hamiltonians(sp)
    return sp


HANDLES = ["general", "slot", "column", "dense"]
_cache = {}


def _case(name):
    """(spec, handle, optim, t, samples of alpha = params0 at the rows, evalGradF(alpha), rows call at those samples) - made once"""
    if name not in _cache:
        sp = _spec(name)
        h = capi.Handle(sp, device=0)
        opt = capi.Optim(h, sp)
        t, _ = h.sampled_times()
        h.set_params(sp.params0)
        samples = h.eval_controls(t)
        ref = opt.evalGradF(sp.params0)
        rows = opt.evalGradF_sampled(samples, "rows")
        _cache[name] = (sp, h, opt, t, samples, ref, rows)
    return _cache[name]


def _same_values(a, b):
    for k in OBJ_KEYS:
        assert a[k] == pytest.approx(b[k], rel=REF_RTOL, abs=1e-12), k


def _close_grad(g, ref):
    err, nrm = np.linalg.norm(g - ref), np.linalg.norm(ref)
    print(f"|g - ref| = {err:.3e}, |ref| = {nrm:.3e}")
    assert err <= 1e-8 * nrm


def test_family_of_every_handle():
    """the four handles do sit on four kernel families"""
    want = {"general": "k_forward<", "slot": "k_forward_q32<", "column": "k_forward_col<", "dense": "k_forward"}
    for name in HANDLES:
        sp, h, opt, *_ = _case(name)
        assert h.last_kernel("forward").startswith(want[name]), (name, h.last_kernel("forward"))
    assert _case("dense")[0].hamiltonian is not None


@pytest.mark.parametrize("name", HANDLES + ["imr4"])
def test_same_function_two_spellings(name):
    """1. The samples of the spline controls at the table rows give the objective of the spline evaluation, field by field."""
    sp, h, opt, t, samples, (val, _), (sval, _) = _case(name)
    assert t.size == sp.time.ntime * (3 if name == "imr4" else 1)
    fval = opt.evalF_sampled(samples, "rows")
    for k in OBJ_KEYS:
        print(name, k, val[k], sval[k], fval[k])
    _same_values(fval, val)
    _same_values(sval, val)


@pytest.mark.parametrize("name", HANDLES + ["imr4"])
def test_chain_rule_against_the_spline_gradient(name):
    """2. p, q are linear in alpha for the spline bases: with A = d samples / d alpha from eval_controls on the unit vectors,
    A^T grad_samples is the gradient of the spline evaluation."""
    sp, h, opt, t, samples, (_, g), (_, gs) = _case(name)
    if name == "imr4":
        assert np.ptp(np.diff(t)) > 1e-3 * sp.time.dt  # the row times are not uniform
    nd = sp.params0.size
    A = np.empty((samples.size, nd))
    for d in range(nd):
        e = np.zeros(nd)
        e[d] = 1.0
        h.set_params(e)
        A[:, d] = h.eval_controls(t).reshape(-1)
    h.set_params(sp.params0)
    assert np.allclose(A @ sp.params0, samples.reshape(-1), rtol=0, atol=1e-14)
    _close_grad(A.T @ gs.reshape(-1), g)


def _w_hold(t, T, nsamp):
    W = np.zeros((t.size, nsamp))
    for s, ts in enumerate(t):
        W[s, min(nsamp - 1, int(np.floor(ts * nsamp / T)))] = 1.0
    return W


def _w_linear(t, T, nsamp):
    W = np.zeros((t.size, nsamp))
    for s, ts in enumerate(t):
        x = ts * (nsamp - 1) / T
        j = min(nsamp - 2, int(np.floor(x)))
        W[s, j], W[s, j + 1] = 1.0 - (x - j), x - j
    return W


# general: 20 rows; imr4: 60 rows at non-uniform times; column: 12 rows
@pytest.mark.parametrize("name,mode,nsamp", [
    ("general", "hold", 1), ("general", "hold", 7), ("general", "hold", 20), ("general", "hold", 33),
    ("general", "linear", 2), ("general", "linear", 7), ("general", "linear", 33),
    ("imr4", "hold", 7), ("imr4", "hold", 90), ("imr4", "linear", 7),
    ("column", "hold", 5), ("column", "linear", 5),
])
def test_interpolation_modes(name, mode, nsamp):
    """3. 'hold' and 'linear' are the rows call behind the interpolation matrix W the definitions give: the same value, W^T its gradient -
    exact zeros for the slots that own no row."""
    sp, h, opt, t, samples, *_ = _case(name)
    T, Q = sp.time.ntime * sp.time.dt, samples.shape[1]
    W = (_w_hold if mode == "hold" else _w_linear)(t, T, nsamp)
    assert np.allclose(W.sum(axis=1), 1.0, rtol=0, atol=1e-14) and W.min() >= 0.0
    rng = np.random.default_rng(nsamp)
    v = np.abs(samples).max() * rng.uniform(-1.0, 1.0, (nsamp, Q, 2))
    val, g = opt.evalGradF_sampled(v, mode)
    rval, rg = opt.evalGradF_sampled(np.einsum("sj,jkc->skc", W, v), "rows")
    _same_values(val, rval)
    _close_grad(g, np.einsum("sj,skc->jkc", W, rg))
    empty = W.sum(axis=0) == 0.0
    if mode == "hold" and nsamp > t.size:
        assert empty.any()
    assert np.all(g[empty] == 0.0)
    _same_values(opt.evalF_sampled(v, mode), val)


@pytest.mark.parametrize("name", HANDLES)
def test_reproducible_and_side_effect_free(name):
    """4. Two sampled calls return the same bits, and the spline evaluation around them is what it was, on the kernels it ran on."""
    sp, h, opt, t, samples, *_ = _case(name)
    before = opt.evalGradF(sp.params0)
    kernels = (h.last_kernel(0), h.last_kernel(1), h.last_solver)
    a = opt.evalGradF_sampled(3.0 * samples, "rows")
    b = opt.evalGradF_sampled(3.0 * samples, "rows")
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    c = opt.evalGradF_sampled(samples[::3], "linear")
    d = opt.evalGradF_sampled(samples[::3], "linear")
    assert c[0] == d[0] and np.array_equal(c[1], d[1])
    after = opt.evalGradF(sp.params0)
    assert after[0] == before[0] and np.array_equal(after[1], before[1])
    assert (h.last_kernel(0), h.last_kernel(1), h.last_solver) == kernels
    opt.evalGradF_sampled(samples, "rows")
    with pytest.raises(capi.QuandaryAmdError, match="no stored trajectory"):
        h.get_state(0, opt.ninit_local)


def test_fresh_handle_without_set_params():
    """a sampled call on a handle that never saw qd_set_params"""
    sp, _, _, t, samples, _, (sval, sg) = _case("general")
    h = capi.Handle(_spec("general"), device=0)
    opt = capi.Optim(h, h.spec)
    val, g = opt.evalGradF_sampled(samples, "rows")
    _same_values(val, sval)
    _close_grad(g, sg)
    opt.close()
    h.close()


def _row_bound(sp, amp):
    """dt / 2 x the Gershgorin row bound (diag + off) of an all-qubit Lindblad system whose controls are bounded by amp[k] (rad/ns):
    level energies 2 max |h(I)|, decay 1/T1 + 1/(2 T2) per qubit on the diagonal, 1/T1 and 4 amp[k] per qubit beside it."""
    sy, Q, tw = sp.system, sp.system.nosc, 2 * np.pi
    hmax = 0.0
    for I in range(2 ** Q):
        dg = [(I >> (Q - 1 - k)) & 1 for k in range(Q)]
        hd, pair = 0.0, 0
        for k in range(Q):
            hd += tw * (sy.transfreq[k] - sy.rotfreq[k]) * dg[k]
            for l in range(k + 1, Q):
                hd -= tw * sy.crosskerr[pair] * dg[k] * dg[l]
                pair += 1
        hmax = max(hmax, abs(hd))
    diag = 2.0 * hmax + sum(0.5 / sy.dephase_time[k] + 1.0 / sy.decay_time[k] for k in range(Q))
    off = sum(1.0 / sy.decay_time[k] + 4.0 * amp[k] for k in range(Q))
    return sp.time.dt / 2.0 * (diag + off)


def test_solver_gates_read_the_sample_amplitudes():
    """4. (the amplitude-bound hazard) 2^4 Lindblad, gmres on the Krylov kernels of the lean slot family, whose polynomial preconditioner is
    a Neumann series admitted where dt / 2 x (row bound) <= 0.7.  The bound from the spline coefficients of alpha passes that gate, the
    bound from the samples (4 rad/ns) does not: the sampled call must run un-preconditioned, i.e. exactly as on a handle whose option
    gmres_poly = 1 switches the polynomial off - and agree with the spline evaluation of the same pulse on that handle."""
    def make(options):
        sp = _spec("slot", linsolve="gmres", dt=0.1)
        sp.options = {"gmres_split": "0", **options}
        h = capi.Handle(sp, device=0)
        return sp, h, capi.Optim(h, sp)

    sp, h, opt = make({})
    Q = sp.system.nosc
    # spline bound per oscillator: sum over the carriers of max |alpha^1| + max |alpha^2| (one segment)
    a = sp.params0.reshape(Q, -1, 2, 10)
    spline_amp = np.abs(a).max(axis=3).sum(axis=(1, 2))
    t, _ = h.sampled_times()
    rng = np.random.default_rng(5)
    v = rng.uniform(-4.0, 4.0, (t.size, Q, 2))
    v[0] = 4.0
    sample_amp = np.abs(v).max(axis=(0, 2))
    lo, hi = _row_bound(sp, spline_amp), _row_bound(sp, sample_amp)
    print(f"gate value from alpha {lo:.4f}, from the samples {hi:.4f}")
    assert lo <= 0.7 < hi
    opt.evalGradF(sp.params0)  # (the handle has seen alpha, and its plan is the preconditioned one)
    assert h.last_solver == "krylov"
    val, g = opt.evalGradF_sampled(v, "rows")
    assert h.last_solver == "krylov"
    applies = h.mean_applies
    sp1, h1, opt1 = make({"gmres_poly": "1"})
    val1, g1 = opt1.evalGradF_sampled(v, "rows")
    print(f"applications per step {applies} / {h1.mean_applies}")
    assert applies == h1.mean_applies
    assert val == val1 and np.array_equal(g, g1)
    for o_, h_ in ((opt, h), (opt1, h1)):
        o_.close()
        h_.close()


def test_refusals():
    """5. Every refusal comes before the first launch: last_kernel is what it was."""
    sp, h, opt, t, samples, *_ = _case("general")
    kernels = (h.last_kernel(0), h.last_kernel(1))
    lib, val = h.lib, capi.qd_objective_value()
    n, g = samples.shape[0], np.zeros_like(samples)
    dp, ref = capi.dptr, capi.byref

    def rc_f(o, mode, nsamp, s, v):
        return lib.qd_optim_evalF_sampled(o, mode, nsamp, s, v)

    def rc_g(o, mode, nsamp, s, v, gp):
        return lib.qd_optim_evalGradF_sampled(o, mode, nsamp, s, v, gp)

    INVALID, UNSUPPORTED, STATE = -1, -2, -5
    assert rc_f(None, 0, n, dp(samples), ref(val)) == INVALID
    assert rc_f(opt._o, 0, n, None, ref(val)) == INVALID
    assert rc_f(opt._o, 0, n, dp(samples), None) == INVALID
    assert rc_g(opt._o, 0, n, dp(samples), ref(val), None) == INVALID
    assert rc_f(opt._o, 3, n, dp(samples), ref(val)) == INVALID and rc_f(opt._o, -1, n, dp(samples), ref(val)) == INVALID
    assert rc_f(opt._o, 0, n - 1, dp(samples), ref(val)) == INVALID  # rows: nsamp != nrows
    assert rc_f(opt._o, 1, 0, dp(samples), ref(val)) == INVALID       # hold: nsamp < 1
    assert rc_g(opt._o, 2, 1, dp(samples), ref(val), dp(g)) == INVALID  # linear: nsamp < 2
    for bad in (np.nan, np.inf):
        s = samples.copy()
        s[3, 1, 0] = bad
        assert rc_g(opt._o, 0, n, dp(s), ref(val), dp(g)) == INVALID
        assert b"non-finite" in lib.qd_last_error()
    assert lib.qd_sampled_times(h._h, None, None) == INVALID
    assert (h.last_kernel(0), h.last_kernel(1)) == kernels

    def refused(spx, code, word, nranks=1, precision=None):
        hx = capi.Handle(spx, device=0)
        if precision:
            hx.set_precision(precision)
        ox = capi.Optim(hx, spx, rank=0, nranks=nranks)
        nr = spx.time.ntime
        s = np.zeros((nr, spx.system.nosc, 2))
        gx = np.zeros_like(s)
        v = capi.qd_objective_value()
        for mode, ns in ((0, nr), (1, 3), (2, 3)):
            assert lib.qd_optim_evalF_sampled(ox._o, mode, ns, dp(s), ref(v)) == code, (word, mode)
            assert word in lib.qd_last_error().decode(), lib.qd_last_error()
            assert lib.qd_optim_evalGradF_sampled(ox._o, mode, ns, dp(s), ref(v), dp(gx)) == code, (word, mode)
        assert hx.last_kernel(0) == "" and hx.last_kernel(1) == ""
        ox.close()
        hx.close()
        return hx

    refused(_spec("general"), STATE, "single-rank", nranks=2)
    refused(_spec("general", stepper="EE"), UNSUPPORTED, "explicit Euler")
    spe = _spec("general", stepper="EE")
    he = capi.Handle(spe, device=0)
    assert lib.qd_sampled_nrows(he._h) == UNSUPPORTED
    he.close()
    spp = _spec("general")
    spp.objective.penalty.gamma_penalty_energy = 0.1
    refused(spp, UNSUPPORTED, "energy penalty")
    from quandary_amd import config
    from helpers import synthetic_cfg
    txt = synthetic_cfg([3, 3], lindblad=False, ntime=20, nessential=[2, 2]) + "apply_pipulse = 0, 0.05, 0.1, 0.5\n"
    refused(_plain(config.build_spec(config.parse_config_text(txt))), UNSUPPORTED, "pi-pulses")
    refused(_spec("slot"), UNSUPPORTED, "fp32-mixed", precision="f32mixed")


def test_torch_function():
    """6. p_k(t) = a_k sin(w t), q_k = 0 with a leaf tensor a: backward() is sum_s grad_samples[s, k, 0] sin(w t_s)."""
    import torch

    from quandary_amd.torch_controls import SampledObjective
    sp, h, opt, t, samples, *_ = _case("general")
    w = 2 * np.pi / (sp.time.ntime * sp.time.dt)
    a = torch.tensor([0.03, -0.02], dtype=torch.float64, requires_grad=True)
    s = torch.sin(w * torch.from_numpy(t))
    pq = torch.stack([a[None, :] * s[:, None], torch.zeros(t.size, 2, dtype=torch.float64)], dim=2)
    obj = SampledObjective.apply(pq, opt, "rows")
    assert obj.dim() == 0 and obj.dtype == torch.float64
    (2.0 * obj).backward()
    val, g = opt.evalGradF_sampled(pq.detach().numpy(), "rows")
    assert obj.item() == val["objective"]
    want = 2.0 * (g[:, :, 0] * np.sin(w * t)[:, None]).sum(axis=0)
    assert np.allclose(a.grad.numpy(), want, rtol=1e-12, atol=0.0)


def test_zz_close():
    for sp, h, opt, *_ in _cache.values():
        opt.close()
        h.close()
    _cache.clear()
