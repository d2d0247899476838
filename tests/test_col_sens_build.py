"""The sensitivity form of the lean column adjoint sweep (model-constant sensitivities under option sens_lean) as libquandary_amd.so
contains it, read with nm -C on the CPU: k_adjoint_col_sens and k_adjoint_colj_sens in every diagonal-split stationary instantiation
col_sweep (qd_col.h) can pick - 16 + 8 kernels - and nothing else: no Krylov (KRY = true) instantiation, no plain-Neumann form
(SPLIT = false), no forward twin (the forward sweep of the call is k_forward_col / k_forward_colj itself) and no operator application.
The names lie outside every pattern the other build tests and the census of test_gpu_kernel_coverage.py count with."""
import itertools
import re

from test_col_vars_build import _b, _library_symbols

COL_SENS_RE = re.compile(r"(k_(?:forward|adjoint|apply)_colj?_sens<[^>]*>)")


def _instantiations():
    """<Q, EPT, SPLIT = true, USLOT, SKIP, KRY = false>: uncoupled with and without skipped stopping tests; coupled, the form that tests
    every pass; each in both USLOT forms, for two and three oscillators, five and eight columns per wave."""
    col = [f"{q}, {ept}, true, {_b(uslot)}, {_b(skip)}, false" for q, ept, uslot, skip in itertools.product((2, 3), (5, 8), (False, True), (False, True))]
    colj = [f"{q}, {ept}, true, {_b(uslot)}, false, false" for q, ept, uslot in itertools.product((2, 3), (5, 8), (False, True))]
    return col, colj


def test_library_holds_the_sensitivity_kernels_of_the_diagonal_split_column_adjoint():
    out = _library_symbols()
    built = set(COL_SENS_RE.findall(out))
    col, colj = _instantiations()
    want_col = {f"k_adjoint_col_sens<{a}>" for a in col}
    want_colj = {f"k_adjoint_colj_sens<{a}>" for a in colj}
    assert len(want_col) == 16 and len(want_colj) == 8
    want = want_col | want_colj
    assert not want - built, ("missing from the library", sorted(want - built))
    assert not built - want, ("in the library without a launcher that picks it", sorted(built - want))
    assert not any(n.endswith(", true>") for n in built)  # no Krylov instantiation (KRY is the last argument)
    assert all(re.match(r"k_\w+<\d, \d, true, ", n) for n in built)  # no plain-Neumann form (SPLIT is the third)
    for absent in ("k_forward_col_sens", "k_forward_colj_sens", "k_apply_col_sens", "k_apply_colj_sens"):
        assert absent not in out, absent


def test_the_names_lie_outside_every_other_pattern_and_the_census():
    from test_batch_col_build import SETS_RE
    from test_col_vars_build import VARS_RE as COL_VARS_RE
    from test_general_vars_build import VARS_RE as GENERAL_VARS_RE
    from test_gpu_coupled_column import COLJ_RE
    from test_gpu_kernel_coverage import KERNEL_RE
    from test_model_sens_build import SENS_RE
    col, colj = _instantiations()
    for name in [f"k_adjoint_col_sens<{a}>" for a in col] + [f"k_adjoint_colj_sens<{a}>" for a in colj]:
        line = f"0000000000001000 T void qd::{name}(qd::SweepArgs)"
        for pattern in (KERNEL_RE, SETS_RE, COL_VARS_RE, GENERAL_VARS_RE, SENS_RE, COLJ_RE):
            assert not pattern.findall(line), (name, pattern.pattern)
    assert len(set(KERNEL_RE.findall(_library_symbols()))) == 134
