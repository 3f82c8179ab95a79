#!/usr/bin/env python3
"""Is the gfx950 code of two build trees the same?  The acceptance check of a refactor of the device sources.

    python scripts/isa_equal.py TREE_A TREE_B [--jobs N] [--keep DIR]

CPU only: needs hipcc, no GPU.  For every device translation unit of each tree (the hipcc compile lines `make -n -B`
prints for the library, flags exactly as the Makefile gives them, with `--cuda-device-only -S` in place of `-c`) it takes
the assembly and compares, whichever file or unit a function lives in:

  * per function symbol (kernels and out-of-line helpers): the instruction text, after dropping comments, blank lines
    and source-position directives and renumbering local labels in order of first appearance;
  * per kernel: its .amdhsa_* descriptor lines (registers, scratch, LDS, occupancy hints);
  * the set of kernel symbols of the whole library;
  * the compiler's kernel-resource-usage remarks, sorted (what `make resource-usage` prints).

It compares text; it does not look for particular instructions.  Exit status 0: equal, 1: not, 2: could not build.
Not a test: neither pytest nor bench.py runs it.
"""
import argparse
import collections
import concurrent.futures
import difflib
import os
import re
import shlex
import subprocess
import sys
import tempfile
import time

LIB = "chess2rt_amd/libc2rt.so"
LABEL = re.compile(r"\.L[A-Za-z_]*\d[\w$]*")
DROPPED = re.compile(r"\s*\.(file|loc|ident|cfi_\w+|addrsig\w*)\b")
REMARK = re.compile(r".*remark: [^ ]* *(.*?)(?: \[-Rpass-analysis=kernel-resource-usage\])?$")


def compile_lines(tree):
    """(object name, argv) of every hipcc device compile behind the library, as the tree's Makefile spells it"""
    out = subprocess.run(["make", "-n", "-B", LIB], cwd=tree, check=True, capture_output=True, text=True).stdout
    units = []
    for line in out.splitlines():
        argv = shlex.split(line)
        if "-c" not in argv or "-o" not in argv or not any(a.endswith(".hip") for a in argv):
            continue
        obj = os.path.basename(argv[argv.index("-o") + 1])
        units.append((obj, argv))
    if not units:
        sys.exit(f"{tree}: `make -n -B {LIB}` shows no hipcc compile of a .hip file")
    return units


def assemble(tree, obj, argv, outdir):
    asm = os.path.join(outdir, os.path.splitext(obj)[0] + ".s")
    argv = list(argv)
    argv[argv.index("-c")] = "-S"
    argv[argv.index("-o") + 1] = asm
    argv[1:1] = ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"]
    t0 = time.time()
    r = subprocess.run(argv, cwd=tree, capture_output=True, text=True)
    if r.returncode:
        sys.stderr.write(r.stderr)
        sys.exit(2)
    remarks = [m.group(1) for m in map(REMARK.match, r.stderr.splitlines()) if m]
    return obj, asm, remarks, time.time() - t0


def parse(asm):
    """{symbol: normalised function text}, {kernel symbol: descriptor lines}"""
    funcs, kernels = {}, {}
    types = set()
    name, body, desc = None, None, None
    for raw in open(asm):
        line = raw.split(";", 1)[0].rstrip()
        if not line.strip() or DROPPED.match(line):
            continue
        s = line.strip()
        if desc is not None:  # (a kernel's descriptor sits between its last instruction and its .size)
            if s == ".end_amdhsa_kernel":
                kernels[desc[0]] = "\n".join(desc[1])
                desc = None
            else:
                desc[1].append(" ".join(s.split()))
        elif s.startswith(".amdhsa_kernel"):
            desc = (s.split()[1], [])
        elif s.startswith(".type") and s.endswith(",@function"):
            types.add(s.split()[1].split(",")[0])
        elif name is None and s.endswith(":") and s[:-1] in types:
            name, body = s[:-1], []
        elif name is not None:
            if s.startswith(".size") and s.split()[1].rstrip(",") == name:
                labels = {}
                text = "\n".join(body)
                text = LABEL.sub(lambda m: labels.setdefault(m.group(0), f".L{len(labels)}"), text)
                funcs[name] = text
                name = None
            else:
                body.append(" ".join(s.split()))
    return funcs, kernels


def survey(tree, outdir, jobs):
    os.makedirs(outdir, exist_ok=True)
    funcs, kernels, remarks = collections.defaultdict(list), collections.defaultdict(list), []
    with concurrent.futures.ThreadPoolExecutor(jobs) as pool:
        for obj, asm, rem, secs in pool.map(lambda u: assemble(tree, u[0], u[1], outdir), compile_lines(tree)):
            print(f"  {tree}: {obj} {secs:.0f} s", flush=True)
            f, k = parse(asm)
            for sym, text in f.items():
                funcs[sym].append((text, obj))
            for sym, text in k.items():
                kernels[sym].append((text, obj))
            remarks += rem
    return funcs, kernels, sorted(remarks)


def compare(what, a, b):
    """a, b: {symbol: [(text, object), ...]} — equal as multisets of texts per symbol"""
    bad = 0
    for sym in sorted(set(a) | set(b)):
        ta, tb = sorted(t for t, _ in a.get(sym, [])), sorted(t for t, _ in b.get(sym, []))
        if ta == tb:
            continue
        bad += 1
        where = lambda side: ", ".join(o for _, o in side.get(sym, [])) or "absent"
        print(f"DIFFERENT {what}: {sym}\n  A: {where(a)}\n  B: {where(b)}")
        for x, y in zip(ta, tb):
            if x != y:
                diff = list(difflib.unified_diff(x.splitlines(), y.splitlines(), "A", "B", lineterm="", n=2))
                print("\n".join("    " + d for d in diff[:40]))
                break
    return bad


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--keep", help="keep the assembly files under this directory")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.abspath(args.keep or tmp)
        fa, ka, ra = survey(args.tree_a, os.path.join(root, "a"), args.jobs)
        fb, kb, rb = survey(args.tree_b, os.path.join(root, "b"), args.jobs)
    bad = compare("function text", fa, fb) + compare("kernel descriptor", ka, kb)
    if set(ka) != set(kb):
        bad += 1
        print("DIFFERENT kernel symbols:", *sorted(set(ka) ^ set(kb)), sep="\n  ")
    if ra != rb:
        bad += 1
        print("DIFFERENT resource-usage remarks:")
        print("\n".join("    " + d for d in difflib.unified_diff(ra, rb, "A", "B", lineterm="", n=0)))
    n_inst = sum(len(v) for v in fa.values())
    print(f"{len(fa)} function symbols ({n_inst} instances), {len(ka)} kernels, {len(ra)} resource remarks: "
          + ("EQUAL" if not bad else f"{bad} DIFFERENCES"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
