#!/usr/bin/env python3
"""Build-time audit of the fast compressor's hand-issued ring loads (zig-lz4_amd/csrc/zlz4_compress_fast.hip).

k_compress_fast keeps the window path's input in three VGPRs (r0, r1, r2; see the kernel's ring comment).  Their loads are
issued from one asm statement per call site; r0 and r1 are waited for inside it, but the youngest, r2, stays in flight
across windows until the statement's next run.  The compiler does not know that register is pending, so a copy, spill or
reuse of it before its load has completed would read stale data silently (cdna_hip_programming.md section 5.7 item 1).
A load has completed at an `s_waitcnt vmcnt(N)` -- the compiler's or an asm one -- when at least N vector-memory
operations were issued after it: vmcnt counts in issue order.  This script compiles the file to assembly and checks, for
every global_load inside an asm statement of every k_compress_fast instantiation, that no instruction names its
destination register on any control-flow path from the load to a wait that covers it, counting the vector-memory
operations along each path, and that no path reaches s_endpgm first.  Local asm labels (`1:`, `1f`, `1b`) are followed
as well as the compiler's `.LBB` ones, and a path that leaves the statement on one side of its own
`s_cmpk_lt_u32 sN, IMM` branch does not take the other side of the same compare repeated by the compiler behind it.
Run by `make check-asm` and tests/test_compress_ring_asm.py; re-run it -- and the fast-compress parity tests on the
GPU -- after any toolchain or flag change.
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "zig-lz4_amd", "csrc", "zlz4_compress_fast.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# scalar instructions that leave scc alone (every other s_ instruction is assumed to write it)
NO_SCC_WRITE = ("s_mov_", "s_movk_", "s_cselect_", "s_waitcnt", "s_nop", "s_branch", "s_cbranch", "s_setprio",
                "s_memtime", "s_load_", "s_sleep")


def regs_in(text):
    out = set()
    for m in re.finditer(r"\bv(\d+)\b", text):
        out.add(int(m.group(1)))
    for m in re.finditer(r"\bv\[(\d+):(\d+)\]", text):
        out.update(range(int(m.group(1)), int(m.group(2)) + 1))
    return out


def audit(asm_text):
    lines = asm_text.splitlines()
    kernels, start = [], None
    for i, ln in enumerate(lines):
        if re.match(r"^_ZN4zlz415k_compress_fast\w*:", ln):
            start = i
        elif start is not None and re.match(r"^\s*s_endpgm", ln):
            kernels.append((lines[start].split(":")[0], start, i))
            start = None
    problems, checked = [], 0
    load_re = re.compile(r"^global_load_\w+\s+(v\d+|v\[\d+:\d+\])")
    vmem_re = re.compile(r"^(global|buffer|flat|scratch)_(load|store|atomic)")
    for name, k0, k1 in kernels:
        label_at = {}
        local_labels = []                                   # (line, number) of `N:` labels inside asm statements
        asm_region = [False] * (k1 + 2)
        inside = False
        for i in range(k0, k1 + 1):
            s = lines[i].strip()
            if ";;#ASMSTART" in s:
                inside = True
            asm_region[i] = inside
            if ";;#ASMEND" in s:
                inside = False
            m = re.match(r"^(\.LBB\d+_\d+):", s)
            if m:
                label_at[m.group(1)] = i
            m = re.match(r"^(\d+):$", s)
            if m and inside:
                local_labels.append((i, m.group(1)))

        def target(j, lab):
            m = re.match(r"^(\d+)([fb])$", lab)
            if m:
                n, d = m.groups()
                if d == "f":
                    c = [ln for ln, x in local_labels if x == n and ln > j]
                    return min(c) if c else None
                c = [ln for ln, x in local_labels if x == n and ln < j]
                return max(c) if c else None
            return label_at.get(lab)

        for i in range(k0, k1 + 1):
            t = lines[i].strip()
            m0 = load_re.match(t) if asm_region[i] else None
            if not m0:
                continue
            dest = regs_in(m0.group(1))
            checked += 1
            # a load on the fall-through side of the asm statement's own `s_cmpk_lt_u32 sN, IMM; s_cbranch_scc1` was
            # issued with that compare false; the compiler re-tests the same condition after the statement, and a path
            # that takes the other side there does not exist.  known = (sN, IMM, outcome) while sN is not written
            known = None
            for b in range(i - 1, k0, -1):
                tb = lines[b].strip()
                if re.match(r"^\d+:$", tb) or not asm_region[b]:
                    break
                if tb.startswith("s_cbranch_scc1"):
                    mc = re.match(r"^s_cmpk_lt_u32\s+(s\d+),\s*(\S+)", lines[b - 1].strip())
                    if mc:
                        known = (mc.group(1), mc.group(2), False)
                    break
            # state: (line, vector-memory operations issued since the load (capped), known compare, scc if known)
            seen, stack, covered = set(), [(i + 1, 0, known, None)], 0
            while stack:
                j, younger, known, scc = stack.pop()
                while j <= k1:
                    if (j, younger, known, scc) in seen:
                        break
                    seen.add((j, younger, known, scc))
                    t = lines[j].strip()
                    t = "" if t.startswith(";") else t.split(";")[0].strip()
                    if not t or t.startswith((".", "//")) or t.endswith(":"):
                        j += 1
                        continue
                    mc = re.match(r"^s_cmpk_lt_u32\s+(s\d+),\s*(\S+)$", t)
                    if known and mc and (mc.group(1), mc.group(2)) == known[:2]:
                        scc = known[2]
                    elif t.startswith("s_") and not t.startswith(NO_SCC_WRITE):
                        scc = None                          # (may write scc)
                    if known:
                        first = re.match(r"^\w+\s+(s\d+|s\[(\d+):(\d+)\])", t)
                        if first and not t.startswith(("s_cmp", "s_cbranch", "s_waitcnt")):
                            n = int(known[0][1:])
                            hit = first.group(1) == known[0] if first.group(2) is None else \
                                int(first.group(2)) <= n <= int(first.group(3))
                            if hit:
                                known = None                # sN written (scc keeps what it holds)
                    mw = re.match(r"^s_waitcnt\b.*\bvmcnt\((\d+)\)", t)
                    if mw and younger >= int(mw.group(1)):
                        covered += 1
                        break                                   # the load has completed on this path
                    if t.startswith("s_endpgm"):
                        problems.append("%s: the load at line %d reaches s_endpgm while in flight" % (name, i + 1))
                        break
                    if dest & regs_in(t):
                        problems.append("%s: v%s (in flight since line %d) is named at line %d: %s" %
                                        (name, sorted(dest), i + 1, j + 1, t))
                    if vmem_re.match(t):
                        younger = min(younger + 1, 64)
                    m = re.match(r"^(s_branch|s_cbranch_\w+)\s+(\S+)", t)
                    if m:
                        op = m.group(1)
                        taken = fall = True
                        if scc is not None and op in ("s_cbranch_scc0", "s_cbranch_scc1"):
                            taken = (op == "s_cbranch_scc1") == scc
                            fall = not taken
                        tgt = target(j, m.group(2))
                        if tgt is None:
                            problems.append("%s: branch target %s at line %d not found" % (name, m.group(2), j + 1))
                        elif taken:
                            stack.append((tgt, younger, known, scc))
                        if op == "s_branch" or not fall:
                            break
                    if t.startswith(("s_setpc", "s_swappc")):
                        problems.append("%s: indirect branch at line %d" % (name, j + 1))
                        break
                    j += 1
            if covered == 0:
                problems.append("%s: no covering wait reachable from the load at line %d" % (name, i + 1))
    return len(kernels), checked, problems


def main():
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "f.s")
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-S",
                               "--cuda-device-only", SRC, "-o", out], stderr=subprocess.DEVNULL)
        nk, checked, problems = audit(open(out).read())
    print("compress ring asm audit: %d kernels, %d hand-issued loads checked, %d problems" % (nk, checked, len(problems)))
    for p in problems:
        print("  " + p)
    return 1 if problems or checked == 0 else 0


if __name__ == "__main__":
    sys.exit(main())
