"""CPU-only: the sampled-control entry points (qd_sampled_nrows, qd_sampled_times, qd_optim_evalF_sampled, qd_optim_evalGradF_sampled) are
exported by the library and declared in the header with the argument lists quandary_amd.capi gives them; the QD_SAMPLED_* values of the
header are those of capi.SAMPLED_MODES."""
import ctypes as C
import os
import re

import pytest

from helpers import ROOT
from quandary_amd import capi

VP, DP, VAL = C.c_void_p, capi.c_dp, C.POINTER(capi.qd_objective_value)
SYMBOLS = {
    "qd_sampled_nrows": ([VP], ["qd_handle*"]),
    "qd_sampled_times": ([VP, DP, DP], ["qd_handle*", "double*", "double*"]),
    "qd_optim_evalF_sampled": ([VP, C.c_int, C.c_int, DP, VAL], ["qd_optim*", "int", "int", "double*", "qd_objective_value*"]),
    "qd_optim_evalGradF_sampled": ([VP, C.c_int, C.c_int, DP, VAL, DP],
                                   ["qd_optim*", "int", "int", "double*", "qd_objective_value*", "double*"]),
}


def _lib():
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return capi.load_library()


def _header():
    return open(os.path.join(ROOT, "include", "quandary_amd.h")).read()


@pytest.mark.parametrize("symbol", sorted(SYMBOLS))
def test_sampled_symbol_is_exported_and_declared(symbol):
    lib = _lib()
    argtypes, ctypes_ = SYMBOLS[symbol]
    assert symbol in capi.EXPORTS and hasattr(lib, symbol)
    assert getattr(lib, symbol).argtypes == argtypes
    m = re.search(r"\bint\s+" + symbol + r"\s*\(([^)]*)\)\s*;", _header())
    assert m
    declared = [re.sub(r"\bconst\b|\s+", "", re.sub(r"\w+$", "", a.strip())) for a in m.group(1).split(",")]
    assert declared == ctypes_, declared


def test_sampled_modes_match_the_header():
    m = re.search(r"enum\s*\{\s*QD_SAMPLED_ROWS\s*=\s*(\d+)\s*,\s*QD_SAMPLED_HOLD\s*=\s*(\d+)\s*,\s*QD_SAMPLED_LINEAR\s*=\s*(\d+)\s*\}", _header())
    assert m
    assert capi.SAMPLED_MODES == {"rows": int(m.group(1)), "hold": int(m.group(2)), "linear": int(m.group(3))}


def test_sampled_calls_are_wrapped():
    assert callable(getattr(capi.Handle, "sampled_times", None))
    assert callable(getattr(capi.Optim, "evalF_sampled", None)) and callable(getattr(capi.Optim, "evalGradF_sampled", None))
