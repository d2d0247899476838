"""The variants form of the lean slot sweep kernels (model-parameter ensemble under option ensemble_lean) as libquandary_amd.so contains
it, read with nm -C on the CPU: k_forward_q32_vars / k_adjoint_q32_vars in the eleven stationary-iteration instantiations the launchers
of the lean slot and fp32-mixed families can pick - those of the SETS form, tests/test_batch_lean_build.py - and no Krylov (GM = true)
instantiation.  The names lie outside the pattern the census of test_gpu_kernel_coverage.py counts, which stays at 134."""
import re

from test_batch_lean_build import INSTANTIATIONS, SETS_RE, _library_symbols
from test_gpu_kernel_coverage import KERNEL_RE

VARS_RE = re.compile(r"(k_(?:forward|adjoint)_q32_vars<[^>]*>)")


def test_library_holds_the_vars_kernels_of_the_stationary_iterations():
    symbols = _library_symbols()
    built = set(VARS_RE.findall(symbols))
    want = {f"k_{d}_q32_vars<{a}>" for d in ("forward", "adjoint") for a in INSTANTIATIONS}
    assert len(want) == 22
    assert not want - built, ("missing from the library", sorted(want - built))
    assert not built - want, ("in the library without a launcher that picks it", sorted(built - want))
    assert not any(re.search(r"<\d, \d, \w+, true,", n) for n in built)  # no variants form of the Krylov kernels
    # the twins of the SETS kernels, name for name
    assert {n.replace("_q32_vars<", "_q32_sets<") for n in built} == set(SETS_RE.findall(symbols))


def test_the_names_lie_outside_the_census():
    for d in ("forward", "adjoint"):
        for a in INSTANTIATIONS:
            line = f"0000000000000000 T void qd::k_{d}_q32_vars<{a}>(qd::SweepArgs)"
            assert VARS_RE.search(line) and not KERNEL_RE.search(line), line
