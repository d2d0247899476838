"""Coupled column-kernel probe (run on the GPU box): systems with dipole-dipole coupling on the lean column kernels of qd_colj.hip and,
under the option no_collean = 1, on the general column kernel of qd_device.h (the path they ran on before) - alternating, same lease,
same process.  Forward sweep and gradient, linearsolver_type neumann and gmres with gmres_split = 0 (the Krylov kernels).
  c4j:  workload c4 (3 x 20, AxC constants, 3600 basis initial conditions) with Jkl = <J> (default 1.0, the order of its cross-Kerr
        1.176; the two rotating frames differ, so eta != 0); c4: the same workload uncoupled, for the ratio
  444j: 4 x 4 x 4 (N = 64, 4096 basis initial conditions), J_kl = 0.004 (1 + 0.37 pair), rotating frames 0.1 GHz apart
usage: colj_probe.py <c4j|444j> <ntime> [J] [general-only]     (QD_LIB=<other build> for an A/B of two builds)"""
import os
import sys
import time

_r = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _r)
from quandary_amd import capi, config  # noqa: E402
from quandary_amd.workloads import workload_spec  # noqa: E402

if os.environ.get("QD_LIB"):
    capi.LIB_PATH = os.environ["QD_LIB"]

which, ntime = sys.argv[1], int(sys.argv[2])
J = float(sys.argv[3]) if len(sys.argv) > 3 else 1.0
general_only = len(sys.argv) > 4 and sys.argv[4] == "general-only"


def spec(coupled, linsolve, grad):
    mode = "gradient" if grad else "simulation"
    if which == "c4j":
        over = {"ntime": ntime, "linearsolver_type": linsolve}
        if coupled:
            over["Jkl"] = J
        return workload_spec("c4", mode, over)
    lines = ["nlevels = 4, 4, 4", f"ntime = {ntime}", "dt = 0.001", "transfreq = 4.1, 4.2, 4.3", "rotfreq = 4.1, 4.2, 4.3",
             "selfkerr = 0.2, 0.2, 0.2", "crosskerr = 0.001", "Jkl = " + (", ".join("%g" % (0.004 * (1 + 0.37 * i)) for i in range(3)) if coupled else "0.0"),
             "collapse_type = both", "decay_time = 80.0, 80.0, 80.0", "dephase_time = 26.0, 26.0, 26.0", "initialcondition = basis",
             "control_enforceBC = false", "optim_objective = Jtrace", "optim_regul = 1e-4", f"linearsolver_type = {linsolve}",
             "linearsolver_maxiter = 20", "timestepper = IMR", "rand_seed = 1234", "usematfree = true", f"runtype = {mode}",
             "optim_target = pure, 0, 0, 0", "optim_penalty = 0.0", "optim_penalty_energy = 0.0", "optim_penalty_dpdm = 0.0", "optim_penalty_variation = 0.0"]
    for k in range(3):
        lines += [f"control_segments{k} = spline, 10", f"control_initialization{k} = random, 0.005", f"carrier_frequency{k} = 0.0, -0.2"]
    return config.build_spec(config.parse_config_text("\n".join(lines) + "\n"))


settings = [("coupled-lean", True, {}), ("coupled-general", True, {"no_collean": 1})]
if general_only:
    settings = settings[1:]
else:
    settings.append(("uncoupled-lean", False, {}))
for linsolve, sopts in (("neumann", {}), ("gmres", {"gmres_split": 0})):
    for grad in (False, True):
        for rep in range(2):
            for tag, coupled, opts in settings:
                sp = spec(coupled, linsolve, grad)
                sp.options = {**sopts, **opts}
                h = capi.Handle(sp)
                o = capi.Optim(h, sp)
                for i in range(2):  # (the second evaluation is the measurement: the first one allocates and tunes)
                    t0 = time.perf_counter()
                    if grad:
                        v, g = o.evalGradF(sp.params0)
                        extra = " adj_ms %.2f |g| %.12e %s" % (h.adjoint_ms, float((g ** 2).sum() ** 0.5), h.last_kernel("adjoint"))
                    else:
                        v = o.evalF(sp.params0)
                        extra = ""
                    wall = (time.perf_counter() - t0) * 1e3
                    print(which, tag, linsolve, "grad" if grad else "fwd", "rep", rep, "eval", i, "ninit", sp.ninit, "ntime", ntime, "solver", h.last_solver,
                          "applies %.3f" % h.mean_applies, "fwd_ms %.2f" % h.forward_ms, "wall_ms %.1f" % wall, "objective %.15e" % v["objective"],
                          h.last_kernel("forward") + extra, flush=True)
                o.close()
                h.close()
