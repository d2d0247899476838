"""Is the gfx950 device code of two builds the same?  For a host-only change it has to be.

    python profiles/codeobj_diff.py PARENT_BUILD_DIR NEW_BUILD_DIR [PREFIX ...]

Compares every object whose file name starts with one of the prefixes (default: the sweep kernel units - qd_inst / qd_sets / qd_vars /
qd_sens from qd_inst.hip, qd_q32*, qd_col*) in the two directories.  From each object the gfx950 code object is taken the way
profiles/kmeta.py takes it (.hip_fatbin unbundled); two code objects are the same when their .text bytes and their kernel metadata
notes (registers, scratch, LDS, arguments of every kernel) are.  Prints one line per object that differs or is missing on one side,
the per-kernel metadata lines that changed, and a summary line; exit status 1 if anything differs."""
import hashlib, os, subprocess, sys, tempfile

L = "/opt/rocm/lib/llvm/bin"
PREFIXES = ("qd_inst_", "qd_sets_", "qd_vars_", "qd_sens_", "qd_q32", "qd_col")


def code_object(obj, tmp):
    """(sha256 of .text, notes text) of the gfx950 code object inside a hipcc object file"""
    fat, dev, text = (os.path.join(tmp, n) for n in ("fat.bin", "dev.co", "text.bin"))
    subprocess.check_call([f"{L}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
    for trg in ("hipv4-amdgcn-amd-amdhsa--gfx950", "hip-amdgcn-amd-amdhsa--gfx950"):
        r = subprocess.run([f"{L}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}", f"--targets={trg}", f"--output={dev}"],
                           capture_output=True)
        if r.returncode == 0 and os.path.getsize(dev) > 0:
            break
    else:
        return "no device code", ""  # (an entry-point object: host code only)
    subprocess.check_call([f"{L}/llvm-objcopy", "-O", "binary", "--only-section=.text", dev, text])
    notes = subprocess.check_output([f"{L}/llvm-readelf", "--notes", dev], text=True)
    with open(text, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest(), notes


def main():
    old, new = sys.argv[1], sys.argv[2]
    prefixes = tuple(sys.argv[3:]) or PREFIXES
    names = sorted(n for n in set(os.listdir(old)) | set(os.listdir(new)) if n.endswith(".o") and n.startswith(prefixes))
    differ = 0
    with tempfile.TemporaryDirectory() as tmp:
        for n in names:
            a, b = os.path.join(old, n), os.path.join(new, n)
            if not (os.path.exists(a) and os.path.exists(b)):
                print(f"{n}: only in {old if os.path.exists(a) else new}")
                differ += 1
                continue
            (ta, na), (tb, nb) = code_object(a, tmp), code_object(b, tmp)
            if ta == tb and na == nb:
                continue
            differ += 1
            print(f"{n}: .text {'same' if ta == tb else 'DIFFERS'}, kernel metadata {'same' if na == nb else 'DIFFERS'}")
            la, lb = na.splitlines(), nb.splitlines()
            for x, y in zip(la, lb):
                if x != y:
                    print(f"    - {x.strip()}\n    + {y.strip()}")
            if len(la) != len(lb):
                print(f"    notes: {len(la)} lines against {len(lb)}")
    print(f"{len(names)} objects compared, {differ} differ")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
