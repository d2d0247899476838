"""The SETS form of the lean slot sweep kernels (parameter-set batch under option batch_lean) as libquandary_amd.so contains it, read
with nm -C on the CPU: k_forward_q32_sets / k_adjoint_q32_sets in the eleven stationary-iteration instantiations the launchers of the
lean slot and fp32-mixed families can pick, and no Krylov (GM = true) instantiation.  The names lie outside the pattern the census of
test_gpu_kernel_coverage.py counts, which stays at 134."""
import os
import re
import shutil
import subprocess

from quandary_amd import capi

# <Q, SB, R, GM = false, HJ>: qd_q32.hip, launch_sweep_lean64_sets / launch_sweep_f32_sets
INSTANTIATIONS = [
    "4, 0, double, false, false", "4, 0, double, false, true", "5, 1, double, false, false", "5, 2, double, false, false",
    "5, 1, double, false, true",
    "3, 0, float, false, false", "4, 0, float, false, false", "5, 1, float, false, false", "5, 2, float, false, false",
    "4, 0, float, false, true", "5, 1, float, false, true",
]
SETS_RE = re.compile(r"(k_(?:forward|adjoint)_q32_sets<[^>]*>)")


def _library_symbols():
    if not os.path.exists(capi.LIB_PATH):  # (built first if missing, like the census)
        import __graft_entry__
        __graft_entry__.build()
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    return subprocess.run([nm, "-C", capi.LIB_PATH], check=True, capture_output=True, text=True).stdout


def test_library_holds_the_sets_kernels_of_the_stationary_iterations():
    built = set(SETS_RE.findall(_library_symbols()))
    want = {f"k_{d}_q32_sets<{a}>" for d in ("forward", "adjoint") for a in INSTANTIATIONS}
    assert len(want) == 22
    assert not want - built, ("missing from the library", sorted(want - built))
    assert not built - want, ("in the library without a launcher that picks it", sorted(built - want))
    assert not any(re.search(r"<\d, \d, \w+, true,", n) for n in built)  # no SETS form of the Krylov kernels
