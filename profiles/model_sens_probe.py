"""Model-constant sensitivity probe (run on the GPU box): what the sensitivity form of the general adjoint sweep (k_adjoint_sens,
qd_optim_evalGradF_model) costs over k_adjoint itself - one product and NS = 2 Q + Q (Q - 1) / 2 integer-weighted multiply-adds per
element and sub-step, one workgroup reduction per sweep.  The handle has the general family forced (no_collean = 1, no_lean64 = 1), so
evalGradF and evalGradF_model run the same forward kernel and the adjoint kernels differ in the sensitivity sums alone; the two calls
alternate in one process, three times each after a warm-up of both, and qd_last_adjoint_ms (device time of the adjoint kernel, HIP
events) is what is printed.  Systems: 3x3 Schroedinger (basis), 4x4 Lindblad, 3x3x3 Lindblad and 3x20 Lindblad (the three `3states`
initial conditions), 1000 steps of 0.002 ns, penalties on - the systems of tests/helpers.py.  Nothing here asserts anything.

c4lean / c4jlean: the sensitivity form of the lean column adjoint (option sens_lean = 1: k_adjoint_col_sens / k_adjoint_colj_sens) on the
3x20 workload with the C4 constants, without coupling and with Jkl = 1.0 - 60 diagonal initial conditions, 1000 steps, penalties on.  Two
handles in one process, one with sens_lean = 1 and one with sens_lean = 0 (the general family, k_adjoint_sens), alternating, three times
each after a warm-up.  Line "form": qd_last_adjoint_ms of evalGradF_model against plain evalGradF on the sens_lean = 1 handle - the cost
of the form over the lean adjoint kernel.  Line "call": forward + adjoint device time and wall time of the whole evalGradF_model call,
sens_lean = 1 against sens_lean = 0; spread = largest relative distance of a repetition from the best of its own three.

q4slot / c5slot / q4jslot: the same two lines for the sensitivity form of the lean slot adjoint (option sens_slot = 1: k_adjoint_q32_sens)
on the workloads q4, c5 and q4j - 2^4, 2^5 and coupled 2^4 Lindblad, their 256 / 1024 / 256 basis initial conditions, 1000 steps -
with the penalties on (optim_penalty = optim_penalty_energy = 0.1); the handles differ in sens_slot.
usage: model_sens_probe.py [s33 l44 l333 l320 c4lean c4jlean q4slot c5slot q4jslot ...] >> profiles/model_sens_probe.txt"""
import os
import sys
import time

_r = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _r)
sys.path.insert(0, os.path.join(_r, "tests"))
from helpers import synthetic_spec, unequal_constants  # noqa: E402
from quandary_amd import capi  # noqa: E402

L = dict(lindblad=True, init="3states", nessential=[2, 2, 1])
PROBES = {
    "s33": ([3, 3], dict(lindblad=False, init="basis", nessential=[2, 2])),
    "l44": ([4, 4], {**L, "nessential": [2, 2]}),
    "l333": ([3, 3, 3], L),
    "l320": ([3, 20], {**L, "nessential": [2, 2]}),
}

# name -> (option that keeps the call on the lean family, workload, overrides)
C4 = {"ntime": 1000, "initialcondition": "diagonal, 0, 1"}
PEN = {"optim_penalty": 0.1, "optim_penalty_energy": 0.1}
LEAN_PROBES = {"c4lean": ("sens_lean", "c4", C4), "c4jlean": ("sens_lean", "c4", {**C4, "Jkl": 1.0}),
               "q4slot": ("sens_slot", "q4", PEN), "c5slot": ("sens_slot", "c5", PEN), "q4jslot": ("sens_slot", "q4j", PEN)}


def lean_probe(which):
    from quandary_amd.workloads import workload_spec

    key, workload, overrides = LEAN_PROBES[which]

    def open_handle(on):
        sp = workload_spec(workload, "gradient", overrides)
        sp.options = {key: on}
        h = capi.Handle(sp)
        return sp, h, capi.Optim(h, sp)

    (sp, hl, ol), (_, hg, og) = open_handle("1"), open_handle("0")

    def timed(h, fn):
        t0 = time.perf_counter()
        fn()
        return h.adjoint_ms, h.forward_ms + h.adjoint_ms, (time.perf_counter() - t0) * 1e3

    forms = (("plain", lambda: timed(hl, lambda: ol.evalGradF(sp.params0))), ("lean", lambda: timed(hl, lambda: ol.evalGradF_model(sp.params0))),
             ("general", lambda: timed(hg, lambda: og.evalGradF_model(sp.params0))))
    for _, fn in forms:
        fn()  # (allocations, solver latch)
    t, kern = {tag: [] for tag, _ in forms}, {}
    for rep in range(3):
        for tag, fn in forms:
            t[tag].append(fn())
            kern[tag] = (hg if tag == "general" else hl).last_kernel("adjoint")
    col = lambda tag, i: [v[i] for v in t[tag]]
    spread = lambda v: max(v) / min(v) - 1.0
    fmt = lambda v: " ".join("%.3f" % x for x in v)
    print(which, "form ninit", sp.ninit, "ntime", sp.time.ntime, "adjoint_ms plain", fmt(col("plain", 0)), key + "=1", fmt(col("lean", 0)),
          "sens_over_plain %.3f" % (min(col("lean", 0)) / min(col("plain", 0))), "spread plain %.3f sens %.3f" % (spread(col("plain", 0)), spread(col("lean", 0))),
          kern["plain"], kern["lean"], flush=True)
    for i, what in ((1, "fwd+adj_ms"), (2, "wall_ms")):
        print(which, "call ninit", sp.ninit, "ntime", sp.time.ntime, what, key + "=1", fmt(col("lean", i)), key + "=0", fmt(col("general", i)),
              "general_over_lean %.3f" % (min(col("general", i)) / min(col("lean", i))), "spread lean %.3f general %.3f" % (spread(col("lean", i)), spread(col("general", i))),
              kern["lean"], kern["general"], flush=True)
    for o, h in ((ol, hl), (og, hg)):
        o.close()
        h.close()


for which in (sys.argv[1:] or list(PROBES)):
    if which in LEAN_PROBES:
        lean_probe(which)
        continue
    nlevels, kw = PROBES[which]
    sp = synthetic_spec(nlevels, ntime=1000, dt=0.002, penalties=True, **unequal_constants(len(nlevels), coupled=False), **kw)
    sp.options = {"no_collean": "1", "no_lean64": "1"}
    h = capi.Handle(sp)
    o = capi.Optim(h, sp)
    forms = (("plain", lambda: o.evalGradF(sp.params0)), ("sens", lambda: o.evalGradF_model(sp.params0)))
    for _, fn in forms:
        fn()  # (allocations, solver latch)
    t, kern = {tag: [] for tag, _ in forms}, {}
    for rep in range(3):
        for tag, fn in forms:
            fn()
            t[tag].append(h.adjoint_ms)
            kern[tag] = h.last_kernel("adjoint")
    p, s = min(t["plain"]), min(t["sens"])
    Q = len(nlevels)
    print(which, "ninit", sp.ninit, "ntime", sp.time.ntime, "NS", 2 * Q + Q * (Q - 1) // 2, "adjoint_ms plain", " ".join("%.3f" % v for v in t["plain"]),
          "sens", " ".join("%.3f" % v for v in t["sens"]), "sens_over_plain %.3f" % (s / p), kern["plain"], kern["sens"], flush=True)
    o.close()
    h.close()
