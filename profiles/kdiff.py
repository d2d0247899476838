"""Are the gfx950 kernels of two hipcc objects the same?  Per demangled kernel name: the disassembly (instruction text and encoding, without
addresses - the order of the instantiations may differ) and the kmeta.py line (VGPR, spill, scratch, SGPR).  Exit status 1 on a difference.
    python profiles/kdiff.py OLD/qd_col.o NEW/qd_col.o"""
import os, re, subprocess, sys, tempfile
L = "/opt/rocm/lib/llvm/bin"
HERE = os.path.dirname(os.path.abspath(__file__))


def kernels(obj):
    t = tempfile.mkdtemp()
    subprocess.check_call([f"{L}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, f"{t}/fat.bin"])
    for trg in ("hipv4-amdgcn-amd-amdhsa--gfx950", "hip-amdgcn-amd-amdhsa--gfx950"):  # (as kmeta.py)
        r = subprocess.run([f"{L}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={t}/fat.bin", f"--targets={trg}", f"--output={t}/dev.co"], capture_output=True)
        if r.returncode == 0 and os.path.getsize(f"{t}/dev.co") > 0:
            break
    code, cur = {}, None
    for line in subprocess.check_output([f"{L}/llvm-objdump", "-d", f"{t}/dev.co"], text=True).splitlines():
        m = re.match(r"[0-9a-f]+ <(\S+)>:$", line)
        if m:
            cur = code.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            cur.append(re.sub(r"// [0-9A-F]+:", "//", line))
    names = subprocess.check_output(["c++filt"], input="\n".join(code), text=True).splitlines()
    code = {n: "\n".join(c) for n, c in zip(names, code.values()) if "k_" in n}
    meta = {}
    for line in subprocess.check_output([sys.executable, f"{HERE}/kmeta.py", obj], text=True).splitlines():
        name, rest = line.split(" vgpr ", 1)
        meta[name.strip()] = rest
    return code, meta


(c0, m0), (c1, m1) = kernels(sys.argv[1]), kernels(sys.argv[2])
bad = sorted(set(c0) ^ set(c1))
for n in bad:
    print("only in", sys.argv[1 if n in c0 else 2], ":", n)
same = [n for n in c0 if n in c1 and c0[n] == c1[n]]
for n in sorted(set(c0) & set(c1) - set(same)):
    print("disassembly differs:", n)
msame = [n for n in m0 if m0[n] == m1.get(n)]
for n in sorted(set(m0) | set(m1)):
    if m0.get(n) != m1.get(n):
        print("metadata differs:", n, "|", m0.get(n), "|", m1.get(n))
print(f"{os.path.basename(sys.argv[2])}: {len(c0)} / {len(c1)} kernels, disassembly {len(same)} of {len(c0)} identical, metadata {len(msame)} of {len(m0)} identical")
sys.exit(0 if not bad and len(same) == len(c0) == len(c1) and len(msame) == len(m0) == len(m1) else 1)
