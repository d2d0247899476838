"""The SETS form of the lean column sweep kernels (parameter-set batch under option batch_lean) as libquandary_amd.so contains it, read
with nm -C on the CPU: k_forward_col_sets / k_adjoint_col_sets and k_forward_colj_sets / k_adjoint_colj_sets in every
stationary-iteration instantiation col_sweep (qd_col.h) can pick - 80 kernels - and nothing else: no Krylov (KRY = true) instantiation
and no operator application.  The names lie outside the pattern the census of test_gpu_kernel_coverage.py counts, which stays at 134."""
import itertools
import os
import re
import shutil
import subprocess

from quandary_amd import capi

SETS_RE = re.compile(r"(k_(?:forward|adjoint|apply)_colj?_sets<[^>]*>)")


def _b(v):
    return "true" if v else "false"


def _instantiations():
    """<Q, EPT, SPLIT, USLOT, SKIP, KRY = false>: uncoupled, both forms of the iteration with and without skipped stopping tests;
    coupled, the diagonal-split form that tests every pass; each in both USLOT forms, for two and three oscillators, five and eight
    columns per wave."""
    col = [f"{q}, {ept}, {_b(split)}, {_b(uslot)}, {_b(skip)}, false"
           for q, ept, split, uslot, skip in itertools.product((2, 3), (5, 8), (False, True), (False, True), (False, True))]
    colj = [f"{q}, {ept}, true, {_b(uslot)}, false, false" for q, ept, uslot in itertools.product((2, 3), (5, 8), (False, True))]
    return col, colj


def _library_symbols():
    if not os.path.exists(capi.LIB_PATH):  # (built first if missing, like the census)
        import __graft_entry__
        __graft_entry__.build()
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    return subprocess.run([nm, "-C", capi.LIB_PATH], check=True, capture_output=True, text=True).stdout


def test_library_holds_the_sets_kernels_of_the_stationary_column_sweeps():
    built = set(SETS_RE.findall(_library_symbols()))
    col, colj = _instantiations()
    want_col = {f"k_{d}_col_sets<{a}>" for d in ("forward", "adjoint") for a in col}
    want_colj = {f"k_{d}_colj_sets<{a}>" for d in ("forward", "adjoint") for a in colj}
    assert len(want_col) == 64 and len(want_colj) == 16
    want = want_col | want_colj
    assert not want - built, ("missing from the library", sorted(want - built))
    assert not built - want, ("in the library without a launcher that picks it", sorted(built - want))
    assert not any(n.endswith(", true>") for n in built)  # no SETS form of the Krylov kernels (KRY is the last argument)
    assert not any(n.startswith("k_apply") for n in built)  # ... nor of the operator application


def test_the_names_lie_outside_the_census_of_the_kernel_coverage_test():
    from test_gpu_kernel_coverage import KERNEL_RE
    col, colj = _instantiations()
    for name in (f"k_forward_col_sets<{col[0]}>", f"k_adjoint_colj_sets<{colj[0]}>"):
        assert not KERNEL_RE.findall(f"0000000000001000 T void qd::{name}(qd::SweepArgs)"), name
