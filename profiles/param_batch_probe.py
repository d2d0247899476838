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
usage: param_batch_probe.py [c1 c3 q4 c5 c2f32 c4pure c4diag c4jpure c4jdiag d22 d16 d27 ...] > profiles/param_batch_probe.txt"""
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
for which in (sys.argv[1:] or ["c1", "c3"]):
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
