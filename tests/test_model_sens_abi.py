"""CPU-only: the model-constant sensitivity entry point (qd_optim_evalGradF_model) is exported by the library, declared in the header
with the argument list quandary_amd.capi gives it, and wrapped as capi.Optim.evalGradF_model."""
import ctypes as C
import os
import re

from helpers import ROOT
from quandary_amd import capi

SYMBOL = "qd_optim_evalGradF_model"


def _lib():
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return capi.load_library()


def test_model_sens_symbol_is_exported_and_wrapped():
    lib = _lib()
    assert SYMBOL in capi.EXPORTS and hasattr(lib, SYMBOL)
    assert callable(getattr(capi.Optim, "evalGradF_model", None))


def test_model_sens_argtypes_match_the_header():
    lib = _lib()
    vp, dp, val = C.c_void_p, capi.c_dp, C.POINTER(capi.qd_objective_value)
    # o, alpha, val, grad, d_transfreq, d_selfkerr, d_crosskerr
    assert getattr(lib, SYMBOL).argtypes == [vp, dp, val, dp, dp, dp, dp]
    header = open(os.path.join(ROOT, "include", "quandary_amd.h")).read()
    ctype = {vp: "qd_optim*", dp: "double*", val: "qd_objective_value*"}
    m = re.search(r"\bint\s+" + SYMBOL + r"\s*\(([^)]*)\)\s*;", header)
    assert m
    declared = [re.sub(r"\bconst\b|\s+", "", re.sub(r"\w+$", "", a.strip())) for a in m.group(1).split(",")]
    assert declared == [ctype[t] for t in getattr(lib, SYMBOL).argtypes], declared
