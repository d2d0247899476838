"""The sensitivity form of the general adjoint sweep (k_adjoint_sens, qd_optim_evalGradF_model) as libquandary_amd.so contains it, read
with nm -C on the CPU: the k_adjoint_sens<...> instantiations are exactly those of k_adjoint_vars<...> - every LDS variant of the
standard model, both stencils, Schroedinger and Lindblad, Neumann and GMRES kernels, no dense and no global-memory variant - there is no
forward twin (the forward sweep of the call is k_forward itself), and the new name lies outside the census of
test_gpu_kernel_coverage.py, which stays at 134, and outside the twin test of test_general_vars_build.py."""
import re

from test_general_vars_build import NOT_STANDARD, SWEEP_RE, VARS_RE, _library_symbols

SENS_RE = re.compile(r"(k_adjoint_sens<([^<>]*)>)")


def test_the_sens_instantiations_are_those_of_the_variants_form():
    out = _library_symbols()
    sens = set()
    for _, args in SENS_RE.findall(out):
        a = [s.strip() for s in args.split(",")]
        assert len(a) == 6, args
        assert int(a[2]) not in NOT_STANDARD, args
        sens.add(", ".join(a))
    vars_adj = {", ".join(s.strip() for s in args.split(",")) for _, role, args in VARS_RE.findall(out) if role == "adjoint"}
    assert len(vars_adj) > 50, len(vars_adj)
    assert sens == vars_adj, (sorted(vars_adj - sens), sorted(sens - vars_adj))


def test_there_is_no_forward_sens_kernel():
    out = _library_symbols()
    assert "k_forward_sens" not in out
    assert "inst_forwardsens" not in out


def test_the_name_lies_outside_the_census_and_the_twin_test():
    from test_gpu_kernel_coverage import KERNEL_RE
    out = _library_symbols()
    assert len(set(KERNEL_RE.findall(out))) == 134
    for name in ("k_adjoint_sens<2, false, 0, true, false, true>", "k_adjoint_sens<3, true, 9, false, true, false>"):
        line = f"0000000000001000 T void qd::{name}(qd::SweepArgs)"
        assert not KERNEL_RE.findall(line), name
        assert not SWEEP_RE.findall(line), name
        assert not VARS_RE.findall(line), name
