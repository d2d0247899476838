"""Sampled-controls probe (run on the GPU box): what qd_optim_evalGradF_sampled costs over qd_optim_evalGradF at the same controls.  The
samples are the spline controls of alpha at the control-table rows (mode 'rows'), so both calls sweep the same kernels over the same
table values; the sampled call uploads nrows x nosc x 2 doubles and runs k_table_sampled / k_grad_sampled in place of k_controls /
k_grad.  One handle, the two calls alternating, three times each after a warm-up of both; per call the wall time and the device times
of the two sweeps (qd_last_forward_ms, qd_last_adjoint_ms).  "spread" = the largest relative distance of a repetition from the best of
its own three: what two identical calls differ by.  Workloads: c4 (3x20 Lindblad, the 60 diagonal initial conditions of
model_sens_probe.py, 250 steps) and q4 (the 4-qubit Lindblad workload); the energy penalty, which the sampled call refuses, is off for
both calls.  Nothing here asserts anything.
usage: sampled_probe.py [c4 q4] >> profiles/sampled_probe.txt"""
import os
import sys
import time

_r = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _r)
from quandary_amd import capi  # noqa: E402
from quandary_amd.workloads import workload_spec  # noqa: E402

PROBES = {"c4": ("c4", {"ntime": 250, "initialcondition": "diagonal, 0, 1"}), "q4": ("q4", {})}

for which in (sys.argv[1:] or list(PROBES)):
    workload, overrides = PROBES[which]
    sp = workload_spec(workload, "gradient", overrides)
    sp.objective.penalty.gamma_penalty_energy = 0.0
    h = capi.Handle(sp)
    o = capi.Optim(h, sp)
    t, _ = h.sampled_times()
    h.set_params(sp.params0)
    samples = h.eval_controls(t)

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3, h.forward_ms, h.adjoint_ms

    forms = (("spline", lambda: o.evalGradF(sp.params0)), ("sampled", lambda: o.evalGradF_sampled(samples, "rows")))
    for _, fn in forms:
        fn()  # (allocations, solver latch)
    res, kern = {tag: [] for tag, _ in forms}, {}
    for rep in range(3):
        for tag, fn in forms:
            res[tag].append(timed(fn))
            kern[tag] = h.last_kernel("adjoint")
    col = lambda tag, i: [v[i] for v in res[tag]]
    spread = lambda v: max(v) / min(v) - 1.0
    fmt = lambda v: " ".join("%.3f" % x for x in v)
    for i, what in ((0, "wall_ms"), (1, "forward_ms"), (2, "adjoint_ms")):
        a, b = col("spline", i), col("sampled", i)
        print(which, "ninit", sp.ninit, "nrows", t.size, what, "evalGradF", fmt(a), "evalGradF_sampled", fmt(b),
              "sampled_over_spline %.3f" % (min(b) / min(a)), "spread spline %.3f sampled %.3f" % (spread(a), spread(b)),
              kern["spline"], kern["sampled"], flush=True)
    o.close()
    h.close()
