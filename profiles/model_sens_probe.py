"""Model-constant sensitivity probe (run on the GPU box): what the sensitivity form of the general adjoint sweep (k_adjoint_sens,
qd_optim_evalGradF_model) costs over k_adjoint itself - one product and NS = 2 Q + Q (Q - 1) / 2 integer-weighted multiply-adds per
element and sub-step, one workgroup reduction per sweep.  The handle has the general family forced (no_collean = 1, no_lean64 = 1), so
evalGradF and evalGradF_model run the same forward kernel and the adjoint kernels differ in the sensitivity sums alone; the two calls
alternate in one process, three times each after a warm-up of both, and qd_last_adjoint_ms (device time of the adjoint kernel, HIP
events) is what is printed.  Systems: 3x3 Schroedinger (basis), 4x4 Lindblad, 3x3x3 Lindblad and 3x20 Lindblad (the three `3states`
initial conditions), 1000 steps of 0.002 ns, penalties on - the systems of tests/helpers.py.  Nothing here asserts anything.
usage: model_sens_probe.py [s33 l44 l333 l320 ...] > profiles/model_sens_probe.txt"""
import os
import sys

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

for which in (sys.argv[1:] or list(PROBES)):
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
