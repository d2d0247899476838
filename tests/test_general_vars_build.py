"""The third form of the general sweep kernels (model-parameter ensemble on the general family, option ensemble_general: one block of
model constants per variant) as libquandary_amd.so contains it, read with nm -C on the CPU: every k_forward<...> / k_adjoint<...>
instantiation of a standard-model variant without a set axis has a k_forward_vars / k_adjoint_vars twin with the same six template
arguments <Q, LIND, VAR, QUBIT, GM, PLAIN>, and there is no twin of a dense variant (11, 12, 13, 15, 17) or of the global-memory
kernels (16, which have names of their own).  The new names lie outside the census of test_gpu_kernel_coverage.py, which stays at 134."""
import os
import re
import shutil
import subprocess

from quandary_amd import capi

SWEEP_RE = re.compile(r"(k_(forward|adjoint)<([^<>]*)>)")
VARS_RE = re.compile(r"(k_(forward|adjoint)_vars<([^<>]*)>)")
NOT_STANDARD = {11, 12, 13, 15, 17, 16}


def _library_symbols():
    if not os.path.exists(capi.LIB_PATH):  # (built first if missing, like the census)
        import __graft_entry__
        __graft_entry__.build()
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    return subprocess.run([nm, "-C", capi.LIB_PATH], check=True, capture_output=True, text=True).stdout


def test_every_standard_model_sweep_kernel_has_a_variants_twin_and_no_other_has():
    out = _library_symbols()
    plain = set()
    for _, role, args in SWEEP_RE.findall(out):
        a = [s.strip() for s in args.split(",")]
        assert len(a) in (6, 7), args
        sets = len(a) == 7 and a[6] == "true"
        if int(a[2]) not in NOT_STANDARD and not sets:
            plain.add((role, ", ".join(a[:6])))
    twins = set()
    for _, role, args in VARS_RE.findall(out):
        a = [s.strip() for s in args.split(",")]
        assert len(a) == 6, args
        assert int(a[2]) not in NOT_STANDARD, args
        twins.add((role, ", ".join(a)))
    assert len(plain) > 100, len(plain)
    assert not plain - twins, ("without a twin", sorted(plain - twins))
    assert not twins - plain, ("a twin of no kernel", sorted(twins - plain))
    # both stencils, Schroedinger and Lindblad, Neumann and GMRES kernels, and every LDS variant of the standard model
    assert {a.split(", ")[2] for _, a in twins} == {"0", "1", "2", "4", "9", "14"}
    assert {tuple(a.split(", ")[i] for i in (1, 3, 4)) for _, a in twins} == {(l, q, g) for l in ("false", "true") for q in ("false", "true")
                                                                           for g in ("false", "true")}


def test_the_names_lie_outside_the_census():
    from test_gpu_kernel_coverage import KERNEL_RE
    out = _library_symbols()
    assert len(set(KERNEL_RE.findall(out))) == 134
    for name in ("k_forward_vars<2, false, 0, true, false, true>", "k_adjoint_vars<3, true, 9, false, true, false>"):
        line = f"0000000000001000 T void qd::{name}(qd::SweepArgs)"
        assert not KERNEL_RE.findall(line), name
        assert not SWEEP_RE.findall(line), name
