"""The SETS form of the dense sweep kernels (parameter-set batch on user-supplied Hamiltonians, qd_set_hamiltonian) as
libquandary_amd.so contains it, read with nm -C on the CPU: every k_forward / k_adjoint instantiation of the dense variants 11, 12, 13
(DenseStencil), 15 and 17 (matrix cores) has its twin with a seventh template argument `true`, and the global-memory variant 16 has
none.  The names lie outside the pattern the census of test_gpu_kernel_coverage.py counts, which stays at 134."""
import os
import re
import shutil
import subprocess

from quandary_amd import capi

DENSE_VARIANTS = ("11", "12", "13", "15", "17")
SWEEP_RE = re.compile(r"(k_(?:forward|adjoint)<([^<>]*)>)")


def _library_symbols():
    if not os.path.exists(capi.LIB_PATH):  # (built first if missing, like the census)
        import __graft_entry__
        __graft_entry__.build()
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    return subprocess.run([nm, "-C", capi.LIB_PATH], check=True, capture_output=True, text=True).stdout


def test_every_dense_sweep_kernel_has_its_sets_twin():
    """nm -C prints the defaulted arguments too: <Q, LIND, VAR, QUBIT, GM, PLAIN, SETS>.  qd_last_kernel names the SETS = false
    instantiation with six arguments and its twin with a seventh, `true`; a name of six here is read as SETS = false."""
    names = {n: [a.strip() for a in args.split(",")] for n, args in SWEEP_RE.findall(_library_symbols())}
    assert all(len(a) in (6, 7) for a in names.values())
    plain = {n: a[:6] for n, a in names.items() if (len(a) == 6 or a[6] == "false") and a[2] in DENSE_VARIANTS}
    sets = {n: a for n, a in names.items() if len(a) == 7 and a[6] == "true"}
    # both directions x both solver forms, for Schroedinger and Lindblad systems of one to eight oscillators
    assert len(plain) >= 2 * 2 * 2 * 8, sorted(plain)
    assert {a[2] for a in plain.values()} == set(DENSE_VARIANTS)
    twins = {tuple(a[:6]) for a in sets.values()}
    missing = [n for n, a in plain.items() if tuple(a) not in twins]
    assert not missing, ("dense instantiations without a SETS twin", sorted(missing))
    assert not [n for n, a in sets.items() if a[2] == "16"], "the global-memory variant has no SETS form"
    assert sum(a[2] in DENSE_VARIANTS for a in sets.values()) == len(plain)


def test_census_does_not_count_the_sets_names():
    """The census of test_gpu_kernel_coverage.py counts the lean column and slot instantiations: the new names are none of them."""
    from test_gpu_kernel_coverage import KERNEL_RE, library_kernels
    assert len(library_kernels()) == 134
    assert not any(KERNEL_RE.search(n) for n, _ in SWEEP_RE.findall(_library_symbols()))
