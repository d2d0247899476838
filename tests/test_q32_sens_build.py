"""The sensitivity form of the lean slot adjoint sweep (model-constant sensitivities under option sens_slot) as the build contains it, on
the CPU: the object build/qd_q32_sens.o among the Makefile's OBJS with a rule that compiles qd_q32.hip under -DQD_SENS=1; in
libquandary_amd.so, read with nm -C, k_adjoint_q32_sens in the five fp64 stationary-iteration instantiations launch_sweep_lean64 can
pick and nothing else - no forward twin (the forward sweep of the call is k_forward_q32 itself), no Krylov (GM = true) and no float
instantiation, no operator application - and the entry point launch_sweep_lean64_sens; sens_slot among the keys of the option list.
The names lie outside every pattern the other build tests and the census of test_gpu_kernel_coverage.py count with."""
import os
import re

from quandary_amd import capi
from test_batch_lean_build import _library_symbols

Q32_SENS_RE = re.compile(r"(k_\w+_q32_sens<[^>]*>)")
# <Q, SB, R = double, GM = false, HJ>: qd_q32.hip, launch_sweep_lean64_sens
INSTANTIATIONS = ["4, 0, double, false, false", "5, 1, double, false, false", "5, 2, double, false, false", "4, 0, double, false, true",
                  "5, 1, double, false, true"]
CSRC = os.path.dirname(capi.LIB_PATH)


def test_the_object_is_in_the_makefile():
    text = open(os.path.join(CSRC, "Makefile")).read()
    objs = re.search(r"^OBJS := (.*)$", text, re.M).group(1)
    assert "$(OBJDIR)/qd_q32_sens.o" in objs.split()
    rule = re.search(r"^\$\(OBJDIR\)/qd_q32_sens\.o: qd_q32\.hip [^\n]*\n\t([^\n]*)$", text, re.M)
    assert rule, "no rule for build/qd_q32_sens.o"
    assert "-DQD_SENS=1" in rule.group(1).split() and "-fno-slp-vectorize" in rule.group(1).split()
    assert "-DQD_SETS" not in rule.group(1) and "-DQD_VARS" not in rule.group(1)  # (mutually exclusive: an #error in qd_q32.hip)


def test_library_holds_the_five_sensitivity_kernels_and_the_entry_point():
    out = _library_symbols()
    built = set(Q32_SENS_RE.findall(out))
    want = {f"k_adjoint_q32_sens<{a}>" for a in INSTANTIATIONS}
    assert len(want) == 5
    assert not want - built, ("missing from the library", sorted(want - built))
    assert not built - want, ("in the library without a launcher that picks it", sorted(built - want))
    for absent in ("k_forward_q32_sens", "k_apply_q32_sens"):
        assert absent not in out, absent
    assert re.search(r" T qd::launch_sweep_lean64_sens\(", out)
    assert "launch_sweep_f32_sens" not in out and "launch_apply_lean64_sens" not in out


def test_sens_slot_is_a_known_key():
    """The key list of qd_kernels.hip (what qd_set_option and the QD_<KEY> environment variables are matched against), the parser, and
    the string in the library."""
    text = open(os.path.join(CSRC, "qd_kernels.hip")).read()
    keys = re.search(r"kOptKeys\[\] = \{(.*?)\};", text, re.S).group(1)
    assert '"sens_slot"' in keys and '"sens_lean"' in keys
    assert re.search(r'k == "sens_slot"\) sens_slot = ', text)
    _library_symbols()  # (builds the library first if it is missing)
    assert b"sens_slot\0" in open(capi.LIB_PATH, "rb").read()


def test_the_names_lie_outside_every_other_pattern_and_the_census():
    from test_batch_col_build import SETS_RE as COL_SETS_RE
    from test_batch_lean_build import SETS_RE
    from test_col_sens_build import COL_SENS_RE
    from test_col_vars_build import VARS_RE as COL_VARS_RE
    from test_ensemble_lean_build import VARS_RE
    from test_general_vars_build import VARS_RE as GENERAL_VARS_RE
    from test_gpu_kernel_coverage import KERNEL_RE
    from test_model_sens_build import SENS_RE
    for a in INSTANTIATIONS:
        line = f"0000000000001000 T void qd::k_adjoint_q32_sens<{a}>(qd::SweepArgs)"
        assert Q32_SENS_RE.findall(line)
        for pattern in (KERNEL_RE, SETS_RE, VARS_RE, COL_SETS_RE, COL_VARS_RE, COL_SENS_RE, GENERAL_VARS_RE, SENS_RE):
            assert not pattern.findall(line), (a, pattern.pattern)
    assert len(set(KERNEL_RE.findall(_library_symbols()))) == 134
