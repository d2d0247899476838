"""Lean column forward sweep with the step size folded into the pass coefficients (qd_col.h, ColTeam::stage / set_alpha): the
diagonal-split pass forms x + alpha C z with alpha inside p, q and the thread's T1 factor.  Two-oscillator systems whose waves share the
level of the first oscillator (USLOT), with every kind of wave by that level - bottom (no ket-down neighbour), interior, top (no ket-up
neighbour, no T1 term): n_0 = 2 (bottom and top waves only), 3 and 4 (half interior), N = 40, 45, 60."""
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import REF_RTOL, col_kernels, synthetic_spec
from oracle.oracle import Oracle
from quandary_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ_KEYS = ["objective", "fidelity", "cost", "regul", "penalty", "penalty_dpdm", "penalty_energy", "penalty_variation"]

FOLD_SHAPES = [
    pytest.param(dict(nlevels=[3, 20], lindblad=True, target="pure", objective="Jmeasure", init="diagonal, 0"), id="3x20"),
    pytest.param(dict(nlevels=[2, 20], lindblad=True, nessential=[2, 18], target="pure", objective="Jtrace", init="diagonal, 1"), id="2x20"),
    pytest.param(dict(nlevels=[4, 15], lindblad=True, nessential=[3, 14], target="pure", objective="Jfrobenius", init="diagonal, 0"), id="4x15"),
    pytest.param(dict(nlevels=[3, 15], lindblad=True, detuned=True, target="pure", objective="Jmeasure", init="diagonal, 1"), id="3x15"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("split", ["0", "1"])
@pytest.mark.parametrize("stepper", ["IMR", "IMR4"])
@pytest.mark.parametrize("kw", FOLD_SHAPES)
def test_column_forward_sweep_with_folded_step_size(kw, stepper, split):
    """Operator and transpose at 1e-13; objective parts (1e-7, the suite's 1e-12 floor for parts that vanish) and gradient (1e-8 of its
    norm) against the oracle with every Lindblad penalty; the kernel names are those of helpers.col_kernels; a batch cut into time slices
    gives bit-identical final states to the unsliced one."""
    sp = synthetic_spec(**{**kw, "ntime": 12, "penalties": True, "stepper": stepper, "dt": 0.001})
    sp.options = {"neumann_split": split}
    h, orc = capi.Handle(sp), Oracle(sp)
    rng = np.random.default_rng(23)
    h.set_params(sp.params0)
    orc.set_params(sp.params0)
    x = rng.standard_normal((3, 2 * h.dim))
    t = 0.37 * sp.time.ntime * sp.time.dt
    kernels = col_kernels(kw["nlevels"], split, stepper)
    assert kernels["forward"][len("k_forward_col<"):-1].split(", ")[3] == "true"  # (USLOT)
    for tr in (False, True):
        yo = orc.apply_rhs(t, x, transpose=tr)
        np.testing.assert_allclose(h.apply_rhs(t, x, transpose=tr), yo, rtol=1e-13, atol=1e-13 * np.abs(yo).max())
        assert h.last_kernel("apply") == kernels["apply"]
    opt = capi.Optim(h, sp)
    val, g = opt.evalGradF(sp.params0)
    assert (h.last_kernel("forward"), h.last_kernel("adjoint")) == (kernels["forward"], kernels["adjoint"])
    oval, og = orc.evalGradF(sp.params0)
    for k in OBJ_KEYS:
        assert val[k] == pytest.approx(oval[k], rel=REF_RTOL, abs=1e-12), k
    assert np.linalg.norm(g - og) / np.linalg.norm(og) < 1e-8
    # time-sliced batch against the unsliced one
    x0 = rng.standard_normal((5, 2 * h.dim))
    h.set_option("col_slices", 1)
    ref = h.forward(x0)
    assert h.last_kernel("forward") == kernels["forward"]
    h.set_option("col_slices", 3)
    res = h.forward(x0)
    assert h.last_kernel("forward") == kernels["forward"]
    np.testing.assert_array_equal(res["final_states"], ref["final_states"])
    opt.close(); h.close(); orc.close()


def test_headline_forward_kernel_registers():
    """The headline kernel keeps three waves per SIMD (at most 168 VGPRs) and no more scratch than before the fold (156 B)."""
    obj = os.path.join(ROOT, "quandary_amd", "csrc", "build", "qd_col.o")
    if not os.path.exists(obj):
        pytest.skip("qd_col.o has not been built")
    out = subprocess.check_output(["bash", os.path.join(ROOT, "profiles", "kres.sh"), obj], text=True)
    line = next((l for l in out.splitlines() if "k_forward_col<2, 5, true, true, true, false>" in l), None)
    assert line is not None, out
    vgpr = int(re.search(r"\bvgpr (\d+)", line).group(1))
    scratch = int(re.search(r"\bscratch (\d+)", line).group(1))
    print(line)
    assert vgpr <= 168
    assert scratch <= 156
