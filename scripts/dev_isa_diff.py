#!/usr/bin/env python3
"""Per-function diff of the gfx950 assembly text two revisions compile to (CPU only, no GPU needed).

    scripts/dev_isa_diff.py <rev-a> <rev-b> [--rename OLD=NEW ...] [--jobs N]

For nusi_kernels.hip, nusi_cascade.hip and nusi_detector.hip: both revisions are exported with `git archive` (a <rev>
that names a directory is taken as a source tree as it stands, e.g. `.` for uncommitted work), the device side is compiled
with the Makefile's own command for that file plus `--cuda-device-only -S`, the text is split per symbol, and
three lists are printed: symbols only in A, only in B, and symbols whose text differs (with a unified diff).
Normalised before comparing: local label numbers (.LBB<n>_, .Ltmp<n>, .Lfunc_end<n>), comments, and the
--rename mapping (re.sub on A's text; mangled names hold no regex metacharacter but '.' and '$').  Assembly
text, not the linked code object: there the pc-relative literals to out-of-line callees shift whenever any
function moves.  After the lists, every kernel's instruction lines, SGPRs, VGPRs, scratch and LDS bytes in A and B
(the compiler's "Kernel info" comments).  Exit status 1 if anything differs.
"""
import argparse
import concurrent.futures
import difflib
import os
import re
import shlex
import subprocess
import sys
import tarfile
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ("nusi_kernels.hip", "nusi_cascade.hip", "nusi_detector.hip")
TYPE = re.compile(r"^\s*\.type\s+([^\s,]+),@(function|object)")
LABEL = re.compile(r"\.(LBB|Ltmp|Lfunc_end|Lfunc_begin)\d+")
# directives that open the *next* symbol and so trail the previous symbol's chunk
INFO = re.compile(r"^; (TotalNumSgprs|NumVgprs|ScratchSize|LDSByteSize): (\d+)")
PREAMBLE = re.compile(r"^\s*\.(text|section|protected|globl|weak|hidden|p2align)\b")


def export(rev, dst):
    if os.path.isdir(rev):
        return os.path.abspath(rev)
    tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "include", "nusiprop_amd/csrc"], check=True,
                         stdout=subprocess.PIPE).stdout
    with tempfile.TemporaryFile() as f:
        f.write(tar)
        f.seek(0)
        tarfile.open(fileobj=f).extractall(dst)
    return dst


def assemble(tree, name, out):
    """The Makefile's compile command for `name`, its `-c -o <obj>` replaced by device-only assembly output."""
    csrc = os.path.join(tree, "nusiprop_amd", "csrc")
    obj = "_build/" + name.replace(".hip", ".o")
    lines = subprocess.run(["make", "-n", "-B", obj], cwd=csrc, check=True, stdout=subprocess.PIPE,
                           text=True).stdout.splitlines()
    cmd = shlex.split(next(l for l in lines if name in l and " -c " in l))
    i = cmd.index("-c")
    assert cmd[i + 1] == "-o"
    cmd[i:i + 3] = ["--cuda-device-only", "-S", "-o", out]
    subprocess.run(cmd, cwd=csrc, check=True, stderr=subprocess.DEVNULL)
    return out


def split(path, rename):
    syms, name, cur = {}, None, []
    for line in open(path):
        line = line.split(";", 1)[0].rstrip()
        if not line:
            continue
        for old, new in rename:
            line = old.sub(new, line)
        line = LABEL.sub(lambda m: "." + m.group(1) + "N", line)
        m = TYPE.match(line)
        if m or line.strip() == ".amdgpu_metadata":
            if name:
                while cur and PREAMBLE.match(cur[-1]):
                    cur.pop()
                syms[name] = cur
            name, cur = (m.group(1) if m else None), []
        if name:
            cur.append(line)
    return syms


def kernel_info(path):
    """{kernel: {figure: value}} from the "Kernel info" comment block that follows each kernel's text."""
    info, name = {}, None
    for line in open(path):
        m = TYPE.match(line)
        if m:
            name = m.group(1)
        m = INFO.match(line)
        if m and name:
            info.setdefault(name, {})[m.group(1)] = int(m.group(2))
    return info


def ninstr(lines):
    """The instruction lines of a symbol's chunk: neither directives nor labels."""
    return sum(1 for l in lines if not l.lstrip().startswith(".") and not l.endswith(":"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("rev_a")
    ap.add_argument("rev_b")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW",
                    help="symbol of A renamed in B (re.sub pattern and replacement)")
    ap.add_argument("--jobs", type=int, default=2)
    a = ap.parse_args()
    rename = [(re.compile(o), n) for o, n in (r.split("=", 1) for r in a.rename)]
    differs = False
    with tempfile.TemporaryDirectory() as tmp:
        trees = [export(r, os.path.join(tmp, s)) for r, s in ((a.rev_a, "a"), (a.rev_b, "b"))]
        with concurrent.futures.ThreadPoolExecutor(a.jobs) as ex:
            asm = {(t, f): ex.submit(assemble, trees[t], f, os.path.join(tmp, "%d_%s.s" % (t, f)))
                   for f in FILES for t in (0, 1)}
        for f in FILES:
            A = split(asm[0, f].result(), rename)
            B = split(asm[1, f].result(), [])
            diff = [s for s in A if s in B and A[s] != B[s]]
            print("== %s: %d symbols in A, %d in B" % (f, len(A), len(B)))
            for title, names in (("only in A", [s for s in A if s not in B]), ("only in B", [s for s in B if s not in A]),
                                 ("differ", diff)):
                print("-- %s (%d)" % (title, len(names)))
                for s in names:
                    print("   " + s)
            for s in diff:
                sys.stdout.writelines(l + "\n" for l in difflib.unified_diff(A[s], B[s], "a/" + s, "b/" + s, lineterm="", n=1))
            KA, KB = kernel_info(asm[0, f].result()), kernel_info(asm[1, f].result())
            print("-- kernels: instruction lines, SGPRs, VGPRs, scratch, LDS bytes (A -> B)")
            for s in KA:
                if s in KB and s in A and s in B and "LDSByteSize" in KA[s]:   # (out-of-line functions have none)
                    print("   %s  %d -> %d" % (s, ninstr(A[s]), ninstr(B[s])) + "".join(
                        ", %d -> %d" % (KA[s][k], KB[s][k]) for k in ("TotalNumSgprs", "NumVgprs", "ScratchSize", "LDSByteSize")))
            differs = differs or len(A) != len(B) or bool(diff) or set(A) != set(B)
    return 1 if differs else 0


if __name__ == "__main__":
    sys.exit(main())
