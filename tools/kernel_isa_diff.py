#!/usr/bin/env python3
"""Compare the gfx950 machine code of two builds kernel by kernel:  tools/kernel_isa_diff.py OBJDIR_A OBJDIR_B
Every *.o of a directory is unbundled to its code object and disassembled.  Kernels are matched on their names without the
internal-linkage mark (a `static` may come and go; demangled for display where a c++filt exists) and compared instruction by
instruction (without the s_nop fill behind a kernel's last instruction, which follows its place in the unit), with their VGPR / SGPR / LDS / scratch numbers.  One line per kernel: copies in A, copies in B (units that hold
it), then SAME / DIFF / ONLY_A / ONLY_B.  SAME means that every copy in B equals SOME copy in A: where A's own copies differ
(units built with different flags) the line names the units of A whose copy B kept, and it is for the reader to check that
the launched one is among them.  Exit status 1 unless everything is SAME.  Needs no GPU."""
import collections
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
RES = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def external_name(sym):
    """The mangled name without the internal-linkage mark: the L before the last component of _ZL<n>name / _ZN<n>ns..L<n>nameE."""
    m = re.match(r"_ZN?", sym)
    pos = m.end() if m else 0
    while m:
        n = re.match(r"\d+", sym[pos:])
        if sym[pos:pos + 1] == "L" and sym[pos + 1:pos + 2].isdigit():
            return sym[:pos] + sym[pos + 1:]
        if not n:
            break
        pos += n.end() + int(n.group())
    return sym


def kernels(objdir):
    """{demangled kernel name: [(unit, [instruction lines], {resource: value})]}"""
    out = collections.defaultdict(list)
    with tempfile.TemporaryDirectory() as tmp:
        for obj in sorted(glob.glob(os.path.join(objdir, "*.o"))):
            fat, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "co")
            if subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj], capture_output=True).returncode:
                continue  # (a unit without device code)
            run(f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={fat}", f"--output={co}")
            res, rec = {}, {}  # metadata: one YAML record per kernel, "  - .key: v" opens it, "    .key: v" continues it
            for line in run(f"{LLVM}/llvm-readelf", "--notes", co).splitlines() + ["  - .end: 0"]:
                m = re.match(r"  (- | {2})(\.\w+):\s*(\S*)$", line)
                if m and m.group(1) == "- " and rec.get(".name"):
                    res[rec[".name"]] = {k: rec.get(k) for k in RES}
                if m:
                    rec = {} if m.group(1) == "- " else rec
                    rec[m.group(2)] = m.group(3)
            body = collections.defaultdict(list)
            cur = None
            for line in run(f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co).splitlines():
                m = re.match(r"<(.+)>:$", line.strip())
                if m:
                    cur = m.group(1)
                elif cur and line.strip() and line.strip() != "...":
                    body[cur].append(line.split("//")[0].strip())
            names = [s for s in body if s in res]  # kernels only (not device functions kept out of line)
            for s in names:
                while body[s] and body[s][-1] == "s_nop 0":  # (the fill up to the next function or behind the unit's last one: it
                    body[s].pop()                            # follows the kernel's place in its unit, not the kernel)
                out[external_name(s)].append((os.path.basename(obj), body[s], res[s]))
    filt = shutil.which("llvm-cxxfilt", path=LLVM) or shutil.which("c++filt")
    if filt and out:
        return dict(zip(run(filt, *out).splitlines(), out.values()))
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    tally = collections.Counter()
    for name in sorted(set(a) | set(b)):
        ca, cb = a.get(name, []), b.get(name, [])
        verdict, note = "SAME", ""
        if not ca or not cb:
            verdict = "ONLY_A" if ca else "ONLY_B"
        else:
            same = lambda x, y: x[1] == y[1] and x[2] == y[2]
            odd = next((y for y in cb if not any(same(x, y) for x in ca)), None)  # a copy in B that no unit of A holds
            if odd:
                ref = ca[0]
                verdict = "DIFF"
                i = next((i for i, (x, y) in enumerate(zip(odd[1], ref[1])) if x != y), min(len(odd[1]), len(ref[1])))
                note = f"\n    A {ref[0]} {ref[2]}\n    B {odd[0]} {odd[2]}\n    first difference at instruction {i}:\n      A: {ref[1][i:i + 3]}\n      B: {odd[1][i:i + 3]}"
            elif not all(same(ca[0], x) for x in ca):  # A's own copies differ (per-unit flags): say which ones B kept
                note = "  (A's copies differ; B has that of " + ", ".join(x[0] for x in ca if any(same(x, y) for y in cb)) + ")"
        tally[verdict] += 1
        print(f"{len(ca):2d} {len(cb):2d} {verdict:6s} {name}  [{ca[0][2]['.vgpr_count'] if ca else cb[0][2]['.vgpr_count']} vgpr]{note}")
    copies = lambda k: sum(len(v) for v in k.values())
    print(f"# A: {len(a)} kernels in {copies(a)} copies; B: {len(b)} kernels in {copies(b)} copies; " + ", ".join(f"{k} {v}" for k, v in sorted(tally.items())))
    return 0 if set(tally) <= {"SAME"} else 1


if __name__ == "__main__":
    sys.exit(main())
