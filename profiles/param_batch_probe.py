"""Parameter-set batch probe (run on the GPU box): what several control vectors in one sweep launch buy on the small BASELINE
configurations, whose single sweeps leave most of the device idle (C1: 4 one-wave workgroups, C3: 16), and - with option batch_lean = 1 -
on the lean slot and fp32-mixed families (q4: 256 states, one dependent chain each; c5: 1024 chains on 256 CUs; c2f32: the fp32-mixed
2x2x2 system, 64 one-wave workgroups) and on the lean column family, one workgroup = one CU per state (c4pure / c4diag: the 3 x 20
Lindblad system with the C4 constants over 250 steps from one initial condition - the reference's AxC case, ONE workgroup - and from the
60 diagonal ones; c4jpure / c4jdiag: the same with Jkl = 1.0, the coupled kernels), and on user Hamiltonians (random Hermitian Hsys /
Hc_k, 1000 steps of 0.004 ns), which share launches by default (d22: 2x2 Schroedinger with the CNOT gate, 4 one-wave workgroups; d16:
4x4 Lindblad from the 4 diagonal states of oscillator 0, the N = 16 matrix-core kernel; d27: 3x3x3 Lindblad from 3 diagonal states,
N = 27 on zero-padded 32 x 32 tiles).  For those the comparison that counts is the batch call of this build against the batch call of
a build in which it still was the set-by-set loop, run in the same lease: both sets of lines are in profiles/param_batch_probe.txt.
For every nset: ONE evalGradF_batch / evalF_batch call against the same sets as nset consecutive evalGradF / evalF calls - alternating,
each twice, in one process on one lease; the comparator is the single-evaluation path as it was (for q4, c5, c2f32 and the c4 probes
that loop is what a batch call runs without the option).  Both times of either form are printed: the distance between the two single
times is the noise a ratio has to be read against (nset 1 against the single call above all).  Wall-clock times (the host side is part of what a caller of either form pays).  The control
vectors are the workload's own scaled by 1 ... 3.  Nothing here asserts a speed-up.
e22 / e16 / e27: the ensemble call (one control vector on nvar system Hamiltonians, evalGradF_ensemble / evalF_ensemble) on the systems of
d22 / d16 / d27 against what it replaces - a loop of single evaluations over nvar handles, each prepared with its own Hsys before the
clock starts; the variants are the workload's Hsys plus j x 0.1 % of a random Hermitian matrix of its size (64 samples span 6 %; a first run with 2 % per
variant is recorded too: a launch lasts as long as its stiffest variant).
m320pure / m320diag / m320j: the model-parameter ensemble (evalGradF_ensemble_model / evalF_ensemble_model: one control vector on nvar
variants of the standard model's constants) on the systems of c4pure / c4diag / c4jpure - the shared launches of k_*_col_vars against the
same call under ensemble_loop = 1 (variant by variant on one handle) and against a loop of single evaluations over nvar handles, each
created with its variant's constants before the clock starts.  Variant j: every transition frequency + j x 0.1 MHz, self- and cross-Kerr
coefficients (and J_kl) x (1 + j x 1e-4).  The figure to hold it against is the parameter-set batch of the same set count (c4pure /
c4diag / c4jpure): a variants launch should cost what that costs, plus the re-derivation per task.
m22 / m16 / m27: the same call with option ensemble_general = 1 on the systems of e22 / e16 / e27 as standard-model specs (2x2
Schroedinger, 4x4 and 3x3x3 Lindblad, 1000 steps of 0.004 ns; 4 / 4 / 3 one-workgroup states per variant) - the shared launches of
k_forward_vars / k_adjoint_vars against the same call under ensemble_loop = 1, which is what a build without the option runs, and against
the e22 / e16 / e27 lines.  Variant j: every constant x (1 + j x 1e-3).  single_spread_ms is the distance between the two consecutive
single calls of a line: what the nvar 1 ensemble time has to be within, against the single time.
mq4 / mc5 / mq3f32 / mq4j: the same call with option ensemble_lean = 1 on the lean slot and fp32-mixed families - 2^4 and 2^5 Lindblad in
fp64 (the q4 / c5 workloads), 2x2x2 Lindblad in fp32-mixed (c2), the coupled 2^4 system (q4j) - from the three `3states` initial
conditions over 1000 steps: three workgroups per variant on 256 CUs.  The shared launches of k_forward_q32_vars / k_adjoint_q32_vars
against the same call under ensemble_loop = 1, alternating in one process.  Variant j: every constant x (1 + j x 1e-3).  loop_spread_ms is
the distance between the two loop calls of a line: what one shared variant against a loop of one has to be read against.
usage: param_batch_probe.py [c1 c3 q4 c5 c2f32 c4pure c4diag c4jpure c4jdiag d22 d16 d27 e22 e16 e27 m320pure m320diag m320j m22 m16 m27 mq4 mc5 mq3f32 mq4j ...] > profiles/param_batch_probe.txt"""
import os
import sys
import time

import numpy as np

_r = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _r)
from quandary_amd import capi  # noqa: E402
from quandary_amd.workloads import workload_spec  # noqa: E402

# name -> (workload, precision, options, nset values, configuration overrides)
COL = (1, 2, 4, 16, 64)
DENSE = {"dt": 0.004, "synthetic_hamiltonian_seed": 1234}  # (workloads.random_hamiltonians: the generator of tests/test_gpu_parity.py)
PROBES = {
    "c1": ("c1", "f64", {}, (1, 2, 4, 16, 64, 256), {}),
    "c3": ("c3", "f64", {}, (1, 2, 4, 16, 64, 256), {}),
    "q4": ("q4", "f64", {"batch_lean": "1"}, (1, 2, 4, 8, 16), {}),
    "c5": ("c5", "f64", {"batch_lean": "1"}, (1, 2, 4, 8, 16), {}),
    "c2f32": ("c2", "f32mixed", {"batch_lean": "1"}, (1, 2, 4, 16, 64), {}),
    "c4pure": ("c4", "f64", {"batch_lean": "1"}, COL, {"ntime": 250, "initialcondition": "pure, 0, 0"}),
    "c4diag": ("c4", "f64", {"batch_lean": "1"}, COL, {"ntime": 250, "initialcondition": "diagonal"}),
    "c4jpure": ("c4", "f64", {"batch_lean": "1"}, COL, {"ntime": 250, "initialcondition": "pure, 0, 0", "Jkl": 1.0}),
    "c4jdiag": ("c4", "f64", {"batch_lean": "1"}, COL, {"ntime": 250, "initialcondition": "diagonal", "Jkl": 1.0}),
    "d22": ("c1", "f64", {}, COL, {**DENSE}),
    "d16": ("c1", "f64", {}, COL, {**DENSE, "nlevels": "4, 4", "collapse_type": "both", "initialcondition": "diagonal, 0",
                                   "optim_target": "pure, 0, 0", "optim_objective": "Jmeasure"}),
    "d27": ("c2", "f64", {}, COL, {**DENSE, "nlevels": "3, 3, 3", "initialcondition": "diagonal, 1", "optim_target": "pure, 0, 0, 0",
                                   "optim_objective": "Jmeasure"}),
}
ENSEMBLE = {"e22": "d22", "e16": "d16", "e27": "d27"}


def ensemble_probe(which):
    workload, precision, options, nvars, overrides = PROBES[ENSEMBLE[which]]
    for grad in (True, False):
        sp = workload_spec(workload, "gradient" if grad else "simulation", overrides)
        h = capi.Handle(sp)
        o = capi.Optim(h, sp)
        hsys, hc = sp.hamiltonian
        rng = np.random.default_rng(4321)
        a = rng.standard_normal(hsys.shape) + 1j * rng.standard_normal(hsys.shape)
        pert = 0.001 * np.abs(hsys).max() * (a + a.conj().T)
        own, pairs = sp.hamiltonian, []
        for j in range(max(nvars)):  # the comparator's handles: variant j uploaded once, outside the timed region
            sp.hamiltonian = (hsys + j * pert, hc)
            hj = capi.Handle(sp)
            pairs.append((hj, capi.Optim(hj, sp)))
        sp.hamiltonian = own
        alpha = sp.params0
        for nvar in nvars:
            variants = [hsys + j * pert for j in range(nvar)]
            ens = (lambda: o.evalGradF_ensemble(alpha, variants, per_variant=False)) if grad else (lambda: o.evalF_ensemble(alpha, variants))
            single = (lambda: [oj.evalGradF(alpha) for _, oj in pairs[:nvar]]) if grad else (lambda: [oj.evalF(alpha) for _, oj in pairs[:nvar]])
            ens(), single()  # (allocations, solver latch, tuner)
            t = {"ensemble": [], "single": []}
            for rep in range(2):
                for tag, fn in (("ensemble", ens), ("single", single)):
                    t0 = time.perf_counter()
                    fn()
                    t[tag].append((time.perf_counter() - t0) * 1e3)
                    if tag == "ensemble":
                        sets, kern = o.last_batch_sets, h.last_kernel("forward")
            b, s = min(t["ensemble"]), min(t["single"])
            print(which, "grad" if grad else "fwd", "ninit", sp.ninit, "ntime", sp.time.ntime, "nvar", nvar, "variants_per_launch", sets,
                  "ensemble_ms", " ".join("%.2f" % v for v in t["ensemble"]), "single_ms", " ".join("%.2f" % v for v in t["single"]),
                  "single_over_ensemble %.2f" % (s / b), "ensemble_ms_per_variant %.3f" % (b / nvar), kern, flush=True)
        for hj, oj in pairs:
            oj.close()
            hj.close()
        o.close()
        h.close()


MODEL = {"m320pure": "c4pure", "m320diag": "c4diag", "m320j": "c4jpure", "m22": "d22", "m16": "d16", "m27": "d27"}
GENERAL = ("m22", "m16", "m27")  # on the general kernel family: option ensemble_general, variants 0.1 % apart
# on the lean slot / fp32-mixed families: option ensemble_lean, variants 0.1 % apart; name -> (workload, precision, nvar values, overrides)
S3 = {"initialcondition": "3states"}
LEAN = {"mq4": ("q4", "f64", COL, S3), "mc5": ("c5", "f64", COL, S3), "mq3f32": ("c2", "f32mixed", COL, S3), "mq4j": ("q4j", "f64", COL, S3)}


def model_variant(sp, j, rel=None):
    """The system block of variant j (a copy: the spec keeps its own).  rel: every constant x (1 + j rel) instead."""
    s = type(sp.system).from_buffer_copy(sp.system)
    Q = s.nosc
    for k in range(Q):
        s.transfreq[k] = s.transfreq[k] + 1e-4 * j if rel is None else s.transfreq[k] * (1.0 + rel * j)
        s.selfkerr[k] *= 1.0 + (1e-4 if rel is None else rel) * j
    for i in range(Q * (Q - 1) // 2):
        s.crosskerr[i] *= 1.0 + (1e-4 if rel is None else rel) * j
        s.Jkl[i] *= 1.0 + (1e-4 if rel is None else rel) * j
    return s


def model_probe(which):
    lean = which in LEAN
    if lean:
        workload, precision, nvars, overrides = LEAN[which]
    else:
        workload, precision, options, nvars, overrides = PROBES[MODEL[which]]
    general = which in GENERAL
    rel = 1e-3 if general or lean else None
    if general:  # the standard model of the same system: no user Hamiltonian
        overrides = {k: v for k, v in overrides.items() if k != "synthetic_hamiltonian_seed"}
    for grad in (True, False):
        def spec():
            sp = workload_spec(workload, "gradient" if grad else "simulation", overrides)
            sp.precision = precision
            return sp
        sp = spec()
        h, hl = capi.Handle(sp), capi.Handle(sp)
        if general:
            h.set_option("ensemble_general", "1")
        if lean:
            h.set_option("ensemble_lean", "1")
        hl.set_option("ensemble_loop", "1")
        o, ol = capi.Optim(h, sp), capi.Optim(hl, sp)
        pairs = []
        for j in range(max(nvars)):  # the comparator's handles: created with variant j's constants, outside the timed region
            spj = spec()
            spj.system = model_variant(sp, j, rel)
            hj = capi.Handle(spj)
            pairs.append((hj, capi.Optim(hj, spj)))
        alpha = sp.params0
        for nvar in nvars:
            variants = [model_variant(sp, j, rel) for j in range(nvar)]
            if grad:
                forms = (("ensemble", lambda: o.evalGradF_ensemble_model(alpha, variants, per_variant=False)),
                         ("loop", lambda: ol.evalGradF_ensemble_model(alpha, variants, per_variant=False)),
                         ("single", lambda: [oj.evalGradF(alpha) for _, oj in pairs[:nvar]]))
            else:
                forms = (("ensemble", lambda: o.evalF_ensemble_model(alpha, variants)), ("loop", lambda: ol.evalF_ensemble_model(alpha, variants)),
                         ("single", lambda: [oj.evalF(alpha) for _, oj in pairs[:nvar]]))
            for _, fn in forms:
                fn()  # (allocations, solver latch)
            t = {tag: [] for tag, _ in forms}
            for rep in range(2):
                for tag, fn in forms:
                    t0 = time.perf_counter()
                    fn()
                    t[tag].append((time.perf_counter() - t0) * 1e3)
                    if tag == "ensemble":
                        sets, kern = o.last_batch_sets, h.last_kernel("forward")
            b, l, s = min(t["ensemble"]), min(t["loop"]), min(t["single"])
            print(which, "grad" if grad else "fwd", "ninit", sp.ninit, "ntime", sp.time.ntime, "nvar", nvar, "variants_per_launch", sets,
                  "ensemble_ms", " ".join("%.2f" % v for v in t["ensemble"]), "loop_ms", " ".join("%.2f" % v for v in t["loop"]),
                  "single_ms", " ".join("%.2f" % v for v in t["single"]), "loop_over_ensemble %.2f" % (l / b),
                  "single_over_ensemble %.2f" % (s / b), "ensemble_ms_per_variant %.3f" % (b / nvar),
                  "single_spread_ms %.3f" % abs(t["single"][0] - t["single"][1]), "loop_spread_ms %.3f" % abs(t["loop"][0] - t["loop"][1]),
                  kern, flush=True)
        for hj, oj in pairs:
            oj.close()
            hj.close()
        for x in (o, ol, h, hl):
            x.close()


for which in (sys.argv[1:] or ["c1", "c3"]):
    if which in ENSEMBLE:
        ensemble_probe(which)
        continue
    if which in MODEL or which in LEAN:
        model_probe(which)
        continue
    workload, precision, options, nsets, overrides = PROBES[which]
    for grad in (True, False):
        sp = workload_spec(workload, "gradient" if grad else "simulation", overrides)
        sp.precision = precision
        sp.options = {**(getattr(sp, "options", None) or {}), **options}
        h = capi.Handle(sp)
        o = capi.Optim(h, sp)
        for nset in nsets:
            alphas = np.stack([sp.params0 * (1.0 + 2.0 * j / max(nset - 1, 1)) for j in range(nset)])
            batch = (lambda: o.evalGradF_batch(alphas)) if grad else (lambda: o.evalF_batch(alphas))
            single = (lambda: [o.evalGradF(a) for a in alphas]) if grad else (lambda: [o.evalF(a) for a in alphas])
            batch(), single()  # (allocations, solver latch, tuner)
            t = {"batch": [], "single": []}
            for rep in range(2):
                for tag, fn in (("batch", batch), ("single", single)):
                    t0 = time.perf_counter()
                    fn()
                    t[tag].append((time.perf_counter() - t0) * 1e3)
                    if tag == "batch":
                        sets, kern = o.last_batch_sets, h.last_kernel("forward")
            b, s = min(t["batch"]), min(t["single"])
            print(which, "grad" if grad else "fwd", "ninit", sp.ninit, "ntime", sp.time.ntime, "nset", nset, "sets_per_launch", sets,
                  "batch_ms", " ".join("%.2f" % v for v in t["batch"]), "single_ms", " ".join("%.2f" % v for v in t["single"]),
                  "single_over_batch %.2f" % (s / b), "batch_ms_per_set %.3f" % (b / nset), kern, flush=True)
        o.close()
        h.close()
