"""Compare the gfx950 code generation of the MLP kernel sources of two trees (no GPU needed).

    python profiles/mlp_plan/compare_codegen.py PARENT_TREE RESULT_TREE OUT_DIR

Compiles every ``csrc/mlp*.hip`` of both trees to assembly with the library's own kernel flags
(``build_native.kernel_flags``) plus ``-Rpass-analysis=kernel-resource-usage``, one source at a time, and writes

* ``resources_parent.tsv`` / ``resources_result.tsv``: VGPRs, AGPRs, scratch and occupancy of every kernel;
* ``codegen_diff.txt``: kernels missing from or new in the result, kernels with more scratch or lower
  occupancy, and the kernels whose instruction stream differs (compared per mangled name with comments,
  directives and the function index of local labels stripped); for these, the number of differing lines of
  the opcode sequence (operands dropped, so that a register renumbering does not count) in the LDS prologue
  (up to the first ``s_barrier``) and after it;
* ``compile_times.tsv``: wall time of each source.

``RENAMED`` maps a parent kernel to its name in the result where the signature changed on purpose.
"""
from __future__ import annotations

import difflib
import glob
import importlib.util
import os
import re
import subprocess
import sys
import time

PKG = "do-you-really-need-to-pay-2-20-hedge-fund-strategy-replication-via-machine-learning_amd"
# mlp_critic_dx_kernel<T, F, 100, 0> lost its HEAD parameter and its label argument
RENAMED = {
    f"_ZN5hfrep20mlp_critic_dx_kernelI{t}Li{f}ELi100ELi0EEEvPKT_NS_9MlpCriticEfPS1_Pflif":
    f"_ZN5hfrep20mlp_critic_dx_kernelI{t}Li{f}ELi100EEEvPKT_NS_9MlpCriticEPS1_Pflif"
    for t in ("f", "t") for f in (32, 36)
}
# retired on purpose: the staged GP critic kernel and the unreachable BCE branch of mlp_critic_dx
RETIRED = re.compile(r"mlp_wgp_critic_w_kernel|mlp_critic_dx_kernelI.Li3[26]ELi100ELi1E")


def compile_tree(tree: str, out: str):
    pkg = os.path.join(tree, PKG)
    spec = importlib.util.spec_from_file_location("bn_" + str(abs(hash(tree))), os.path.join(pkg, "build_native.py"))
    bn = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bn)
    os.makedirs(out, exist_ok=True)
    res, streams, times = {}, {}, []
    for src in sorted(glob.glob(os.path.join(pkg, "csrc", "mlp*.hip"))):
        base = os.path.basename(src)
        asm = os.path.join(out, base + ".s")
        cmd = [bn._hipcc()] + bn.kernel_flags(src) + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                                                      src, "-o", asm]
        t0 = time.time()
        p = subprocess.run(cmd, capture_output=True, text=True)
        times.append((base, time.time() - t0))
        if p.returncode:
            sys.exit(p.stderr)
        cur = None
        for line in p.stderr.splitlines():
            m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\S+)", line)
            if not m:
                continue
            if m.group(1) == "Function Name":
                cur = res.setdefault(m.group(2), {})
            elif cur is not None:
                cur[m.group(1).split()[0]] = int(m.group(2))
        name, body = None, []
        for line in open(asm):
            m = re.match(r"^(_Z\w+):", line)
            if m and m.group(1) in res:
                name, body = m.group(1), []
                continue
            if name is None:
                continue
            if line.startswith(".Lfunc_end"):
                streams[name], name = body, None
                continue
            code = line.split(";")[0].rstrip()
            if not code.strip() or code.lstrip().startswith(".") and not code.startswith(".LBB"):
                continue
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", code))
    return res, streams, times


def split_ops(body):
    """Opcodes (operands and so register numbers dropped) up to and after the first s_barrier, the end of the
    LDS prologue; a kernel without one is all 'after'."""
    ops = ["label" if c.startswith(".LBB") else c.split()[0] for c in body]
    cut = ops.index("s_barrier") + 1 if "s_barrier" in ops else 0
    return ops[:cut], ops[cut:]


def ndiff(a, b):
    return sum(1 for l in difflib.unified_diff(a, b, lineterm="", n=0) if l[:1] in "+-" and l[:3] not in ("+++", "---"))


def table(res, path):
    with open(path, "w") as fh:
        fh.write("kernel\tVGPRs\tAGPRs\tscratch_bytes_per_lane\toccupancy\n")
        for k in sorted(res):
            r = res[k]
            fh.write(f"{k}\t{r['VGPRs']}\t{r['AGPRs']}\t{r['ScratchSize']}\t{r['Occupancy']}\n")


def main():
    parent, result, out = sys.argv[1:4]
    pr, ps, pt = compile_tree(parent, os.path.join(out, "asm_parent"))
    rr, rs, rt = compile_tree(result, os.path.join(out, "asm_result"))
    table(pr, os.path.join(out, "resources_parent.tsv"))
    table(rr, os.path.join(out, "resources_result.tsv"))
    with open(os.path.join(out, "compile_times.tsv"), "w") as fh:
        for tag, tt in (("parent", pt), ("result", rt)):
            for base, sec in tt:
                fh.write(f"{tag}\t{base}\t{sec:.1f}\n")
            fh.write(f"{tag}\tsum\t{sum(s for _, s in tt):.1f}\n")
    lines, bad = [], 0
    lines.append(f"kernels: parent {len(pr)}, result {len(rr)}")
    matched = set()
    for k in sorted(pr):
        n = RENAMED.get(k, k)
        if n not in rr:
            if RETIRED.search(k):
                lines.append(f"retired\t{k}")
            else:
                bad += 1
                lines.append(f"MISSING\t{k}")
            continue
        matched.add(n)
        a, b = pr[k], rr[n]
        if b["ScratchSize"] > a["ScratchSize"] or b["Occupancy"] < a["Occupancy"]:
            bad += 1
            lines.append(f"WORSE\t{n}\tscratch {a['ScratchSize']} -> {b['ScratchSize']}, occupancy {a['Occupancy']} -> {b['Occupancy']}")
        if a != b:
            lines.append(f"resources\t{n}\t{a} -> {b}")
        if ps[k] != rs[n]:
            pa, pb, ra, rb = split_ops(ps[k]) + split_ops(rs[n])
            lines.append(f"differs\t{n}\t{len(ps[k])} -> {len(rs[n])} instructions; opcode diff lines: "
                         f"{ndiff(pa, ra)} in the prologue ({len(pa)} -> {len(ra)}), {ndiff(pb, rb)} after it")
    for n in sorted(set(rr) - matched):
        lines.append(f"new\t{n}")
    lines.append(f"violations: {bad}")
    with open(os.path.join(out, "codegen_diff.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
