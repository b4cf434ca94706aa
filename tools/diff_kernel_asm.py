#!/usr/bin/env python3
"""Compare the gfx950 code of kernels in two builds of the shared library, function by function.

  python tools/diff_kernel_asm.py OLD.so NEW.so [name-regex] [--rename OLD_SUFFIX=NEW_SUFFIX ...]

Extracts the gfx950 code objects of each library (llvm-objdump --offloading), disassembles them, and cuts the listing
into functions: a function starts at a `<symbol>:` line and ends at the next line that is not an instruction (the next
symbol, or the `file format` / `Disassembly of section` header of the next code object).  Branch targets and the
`// address: encoding` comments are normalised away, since code placed before a kernel moves its addresses.  A kernel
whose mangled name changed (a new template parameter) is paired through --rename, e.g. `EEEvPKh=ELb0EEEvPKh`.
Prints, per kernel, the instruction counts and every differing line.
"""
import difflib
import os
import re
import subprocess
import sys
import tempfile

OBJDUMP = "/opt/rocm/llvm/bin/llvm-objdump"


def functions(lib):
    with tempfile.TemporaryDirectory() as tmp:
        dst = os.path.join(tmp, "lib.so")
        with open(lib, "rb") as f, open(dst, "wb") as g:
            g.write(f.read())
        subprocess.run([OBJDUMP, "--offloading", dst], cwd=tmp, capture_output=True, check=True)
        text = ""
        for name in sorted(os.listdir(tmp)):
            if name.endswith("gfx950"):
                text += subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", "--no-leading-addr",
                                        os.path.join(tmp, name)], capture_output=True, text=True, check=True).stdout
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^<(\S+)>:$", line)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if not line.startswith(("\t", " ")):        # blank line, code-object header, section header: not code
            if line.strip():
                cur = None
            continue
        if cur is None:
            continue
        x = re.sub(r"//.*", "", line).strip()
        if not x or x == "...":
            continue
        x = re.sub(r"(s_cbranch_\w+|s_branch)\s+\S+", r"\1 <target>", x)
        x = re.sub(r"<[^>]*>", "<target>", x)
        out[cur].append(x)
    return out


def main():
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("old_lib")
    ap.add_argument("new_lib")
    ap.add_argument("pattern", nargs="?", default=".")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW",
                    help="substring of an old mangled name and what it became in the new library")
    a = ap.parse_args()
    renames = [r.split("=", 1) for r in a.rename]
    pat = re.compile(a.pattern)
    old, new = functions(a.old_lib), functions(a.new_lib)
    rc = 0
    for name in sorted(n for n in old if pat.search(n)):
        target = name
        for x, y in renames:
            target = target.replace(x, y)
        cands = [n for n in new if n == target or (target != name and n.startswith(target))]
        if len(cands) != 1:
            print("%s: no unique counterpart in the new library (%s)" % (name, cands[:3]))
            rc = 1
            continue
        d = [x for x in difflib.unified_diff(old[name], new[cands[0]], lineterm="", n=0)
             if x[:1] in "+-" and not x.startswith(("+++", "---"))]
        print("%s -> %s: %d instructions before, %d after, %d differing lines" % (name, cands[0], len(old[name]),
                                                                                 len(new[cands[0]]), len(d)))
        for x in d:
            print("    " + x)
    return rc


if __name__ == "__main__":
    sys.exit(main())
