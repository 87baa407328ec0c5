#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds, kernel by kernel.  No GPU needed, nothing is started on one.

  tools/codeobj_diff.py OLD NEW [-v] [--rename FROM=TO ...]

OLD / NEW: a source tree (its sparsebench_amd/csrc/sbhip.hip is compiled device-only with the Makefile's flags) or a device
object made that way (hipcc ... --cuda-device-only -c).  Each is unbundled, disassembled and its metadata notes are read;
then every symbol is classed as
  identical     same instructions in the same order (branch-target comments stripped) and the same notes
                (registers, LDS, scratch, kernarg layout)
  vector-equal  same notes and the same multiset of non-scalar mnemonics (everything that does not start with s_);
                order, operand order and scalar instructions may differ
  different     anything else
Exit status 1 if a symbol is missing on either side or different.  -v prints a unified diff of each symbol that is
not identical.  DESIGN.md 4.6 says which symbols may be vector-equal.

--rename FROM=TO (repeatable): a type was renamed between OLD and NEW, and kernel symbols carry their parameter types.  FROM is
replaced by TO in OLD's mangled symbol names and in its notes before the two sides are matched, so a renamed kernel is compared
with its parent instead of being reported missing twice.  Give the mangled component with its length, e.g. 7SgsHalf=8SellRows
(the substitution indices S_, S0_, ... behind it do not move: the number of components does not change).
"""
import collections
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
LLVM = os.path.join(ROCM, "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "--cuda-device-only", "-c"]


def run(*cmd):
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True).stdout


def device_elf(path, tmp, tag):
    obj = path
    if os.path.isdir(path):
        obj = os.path.join(tmp, tag + ".o")
        run(os.path.join(ROCM, "bin", "hipcc"), *FLAGS, os.path.join(path, "sparsebench_amd/csrc/sbhip.hip"), "-o", obj)
    with open(obj, "rb") as f:
        if f.read(4) == b"\x7fELF":
            return obj
    elf = os.path.join(tmp, tag + ".elf")
    run(os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + obj,
        "--output=" + elf)
    return elf


def functions(elf):
    """symbol -> list of instructions, comments (address, encoding, branch target) stripped"""
    out, cur = {}, None
    for line in run(os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", elf).splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.startswith("\t"):
            if line.strip() == "...":  # llvm-objdump's mark for a run of zero bytes: alignment padding behind the last instruction
                continue
            cur.append(" ".join(line.split("//")[0].split()))
    return out


def notes(elf):
    """kernel name -> its amdhsa.kernels entry, as text"""
    out, cur, inside = {}, None, False
    for line in run(os.path.join(LLVM, "llvm-readelf"), "--notes", elf).splitlines():
        if line.startswith("amdhsa.kernels:"):
            inside = True
        elif inside and line.startswith("  - "):
            cur = [line]
        elif inside and line.startswith("    "):
            cur.append(line)
            m = re.match(r"^    \.name:\s+(\S+)", line)
            if m:
                out[m.group(1)] = cur
        elif inside:
            inside = False
    return {k: "\n".join(v) for k, v in out.items()}


def vector_mnemonics(insns):
    return collections.Counter(i.split()[0] for i in insns if not i.startswith("s_"))


def demangle(names):
    for filt in (os.path.join(LLVM, "llvm-cxxfilt"), "c++filt"):
        try:
            return dict(zip(names, run(filt, *names).splitlines()))
        except (OSError, subprocess.CalledProcessError):
            pass
    return {n: n for n in names}


def renamed(table, renames):
    """the keys and, where they are text, the values of OLD's table with every FROM replaced by TO"""
    def sub(t):
        for old, new in renames:
            t = t.replace(old, new)
        return t
    return {sub(k): sub(v) if isinstance(v, str) else v for k, v in table.items()}


def main():
    args, renames, verbose = [], [], False
    argv = sys.argv[1:]
    while argv:
        a = argv.pop(0)
        if a == "-v":
            verbose = True
        elif a == "--rename" or a.startswith("--rename="):
            pair = a[len("--rename="):] if "=" in a else (argv.pop(0) if argv else "")
            if pair.count("=") != 1 or not all(pair.split("=")):
                sys.exit("--rename takes FROM=TO, got %r" % pair)
            renames.append(tuple(pair.split("=")))
        else:
            args.append(a)
    if len(args) != 2:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        elfs = [device_elf(p, tmp, t) for p, t in zip(args, ("old", "new"))]
        (fa, fb), (na, nb) = [functions(e) for e in elfs], [notes(e) for e in elfs]
    fa, na = renamed(fa, renames), renamed(na, renames)
    pretty = demangle(sorted(set(fa) | set(fb)))
    count = collections.Counter()
    for s in sorted(set(fa) | set(fb), key=lambda s: pretty[s]):
        if s not in fa or s not in fb:
            cls = "missing in " + ("OLD" if s not in fa else "NEW")
        elif na.get(s) != nb.get(s):
            cls = "different (notes)"
        elif fa[s] == fb[s]:
            cls = "identical"
        elif vector_mnemonics(fa[s]) == vector_mnemonics(fb[s]):
            cls = "vector-equal (%d -> %d instructions)" % (len(fa[s]), len(fb[s]))
        else:
            cls = "different (%d -> %d instructions)" % (len(fa[s]), len(fb[s]))
        count[cls.split()[0]] += 1
        if cls != "identical":
            print("%-40s %s" % (cls, pretty[s]))
        if verbose and cls != "identical" and s in fa and s in fb:
            print("\n".join(difflib.unified_diff(fa[s], fb[s], "OLD", "NEW", n=1, lineterm="")))
            if na.get(s) != nb.get(s):
                print("\n".join(difflib.unified_diff(na.get(s, "").splitlines(), nb.get(s, "").splitlines(), "OLD notes", "NEW notes", n=1, lineterm="")))
    print("symbols: %d old, %d new; identical %d, vector-equal %d, different %d, missing %d"
          % (len(fa), len(fb), count["identical"], count["vector-equal"], count["different"], count["missing"]))
    return 1 if count["different"] or count["missing"] else 0


if __name__ == "__main__":
    sys.exit(main())
