"""The third form of the lean column sweep kernels (model-parameter ensemble: one block of model constants per variant) as
libquandary_amd.so contains it, read with nm -C on the CPU: k_forward_col_vars / k_adjoint_col_vars and k_forward_colj_vars /
k_adjoint_colj_vars in every diagonal-split stationary instantiation col_sweep (qd_col.h) can pick - 48 kernels - and nothing else: no
Krylov (KRY = true) instantiation, no plain-Neumann form (SPLIT = false) and no operator application.  The names lie outside the pattern
of the SETS kernels (test_batch_col_build.py) and outside the census of test_gpu_kernel_coverage.py, which stays at 134."""
import itertools
import os
import re
import shutil
import subprocess

from quandary_amd import capi

VARS_RE = re.compile(r"(k_(?:forward|adjoint|apply)_colj?_vars<[^>]*>)")


def _b(v):
    return "true" if v else "false"


def _instantiations():
    """<Q, EPT, SPLIT = true, USLOT, SKIP, KRY = false>: uncoupled with and without skipped stopping tests; coupled, the form that tests
    every pass; each in both USLOT forms, for two and three oscillators, five and eight columns per wave."""
    col = [f"{q}, {ept}, true, {_b(uslot)}, {_b(skip)}, false" for q, ept, uslot, skip in itertools.product((2, 3), (5, 8), (False, True), (False, True))]
    colj = [f"{q}, {ept}, true, {_b(uslot)}, false, false" for q, ept, uslot in itertools.product((2, 3), (5, 8), (False, True))]
    return col, colj


def _library_symbols():
    if not os.path.exists(capi.LIB_PATH):  # (built first if missing, like the census)
        import __graft_entry__
        __graft_entry__.build()
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    return subprocess.run([nm, "-C", capi.LIB_PATH], check=True, capture_output=True, text=True).stdout


def test_library_holds_the_variant_kernels_of_the_diagonal_split_column_sweeps():
    built = set(VARS_RE.findall(_library_symbols()))
    col, colj = _instantiations()
    want_col = {f"k_{d}_col_vars<{a}>" for d in ("forward", "adjoint") for a in col}
    want_colj = {f"k_{d}_colj_vars<{a}>" for d in ("forward", "adjoint") for a in colj}
    assert len(want_col) == 32 and len(want_colj) == 16
    want = want_col | want_colj
    assert not want - built, ("missing from the library", sorted(want - built))
    assert not built - want, ("in the library without a launcher that picks it", sorted(built - want))
    assert not any(n.endswith(", true>") for n in built)  # no Krylov instantiation (KRY is the last argument)
    assert all(re.match(r"k_\w+<\d, \d, true, ", n) for n in built)  # no plain-Neumann form (SPLIT is the third)
    assert not any(n.startswith("k_apply") for n in built)  # ... and no operator application


def test_the_names_lie_outside_the_sets_pattern_and_the_census():
    from test_batch_col_build import SETS_RE
    from test_gpu_kernel_coverage import KERNEL_RE
    col, colj = _instantiations()
    for name in (f"k_forward_col_vars<{col[0]}>", f"k_adjoint_colj_vars<{colj[0]}>"):
        line = f"0000000000001000 T void qd::{name}(qd::SweepArgs)"
        assert not SETS_RE.findall(line), name
        assert not KERNEL_RE.findall(line), name
