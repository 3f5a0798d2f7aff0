"""Per-kernel instruction-stream and resource comparison of two AMDGPU assembly files.

    hipcc <build_native.kernel_flags(src)> --cuda-device-only -S src.hip -o a.s      (once per build)
    python scripts/isa_kernel_diff.py parent.s new.s

Per kernel: labels and symbol names normalised, comments and directives dropped; `same-isa` / `diff-isa`, the
instruction count and VGPR / AGPR / SGPR / scratch / LDS / occupancy as `parent -> new`.  Forward kernels
(`fwd` in the name) that are identical with equal resources are counted but not listed.
"""
import re
import shutil
import subprocess
import sys


def parse(path):
    kern, res = {}, {}
    cur, body = None, None
    last = None
    for ln in open(path, errors="replace"):
        s = ln.rstrip("\n")
        m = re.match(r"^(_Z\w+):", s)
        if m and cur is None:
            cur, body = m.group(1), []
            continue
        if cur is not None:
            if re.match(r"^\.Lfunc_end\d+:", s):
                kern[cur] = body
                last, cur = cur, None
                continue
            t = s.split(";")[0].strip()
            if not t or (t.startswith(".") and not t.endswith(":")):
                continue
            t = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", t)
            body.append(t)
        elif last:
            m = re.match(r"^; (NumVgprs|NumAgprs|TotalNumVgprs|TotalNumSgprs|ScratchSize|Occupancy|LDSByteSize|codeLenInByte):? *=? *(\d+)", s.replace(" [waves/SIMD]", ""))
            if m:
                res.setdefault(last, {})[m.group(1)] = int(m.group(2))
    return kern, res


def demangle(names):
    out = subprocess.run([shutil.which("c++filt") or shutil.which("llvm-cxxfilt") or "c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, out))


def main():
    a, ra = parse(sys.argv[1])
    b, rb = parse(sys.argv[2])
    dm = demangle(sorted(set(a) | set(b)))
    keys = ["NumVgprs", "NumAgprs", "TotalNumSgprs", "ScratchSize", "LDSByteSize", "Occupancy"]
    fam = {}
    print("| kernel | isa | instr (parent -> new) | VGPR | AGPR | SGPR | scratch | LDS | occupancy |")
    print("|---|---|---|---|---|---|---|---|---|")
    for k in sorted(set(a) | set(b), key=lambda n: dm[n]):
        if k not in a or k not in b:
            print("| %s | ONLY-%s |" % (dm[k], "parent" if k in a else "new"))
            continue
        same = a[k] == b[k]
        name = re.sub(r"^void hfrep::", "", dm[k]).split("(")[0]
        f = name.split("<")[0]
        fam.setdefault(f, [0, 0])[0 if same else 1] += 1
        if "fwd" in f and same and ra[k] == rb[k]:
            continue
        cols = []
        for q in keys:
            x, y = ra[k].get(q), rb[k].get(q)
            cols.append(str(x) if x == y else "%s -> %s" % (x, y))
        n1 = sum(1 for t in a[k] if not t.endswith(":"))
        n2 = sum(1 for t in b[k] if not t.endswith(":"))
        print("| `%s` | %s | %s | %s |" % (name, "same-isa" if same else "diff-isa", n1 if n1 == n2 else "%d -> %d" % (n1, n2), " | ".join(cols)))
    print()
    for f, (s, d) in sorted(fam.items()):
        print("%s: %d same-isa, %d diff-isa" % (f, s, d))


if __name__ == "__main__":
    main()
