"""Test-side model of whole .lz4 files (tests/test_lz4file_cpu.py, tests/test_gpu_lz4file.py; include/zlz4_amd.h, DESIGN.md
section 4.4j): a buffer of modern frames, skippable frames and -- with `legacy` -- legacy frames in any order.  It composes
the two models that exist: multiframegen (`_member`, `_decode_frame`) for frames and skippable frames, legacygen (`walk`,
`read`) for legacy members.

* `split(buf, legacy)`: -> [Member]; a legacy member has kind 4, nb = the blocks of its walk, and is the last one only
  where the walk meets a defect (it then reaches to the end).  `split(buf, False)` is multiframegen.split(buf).
* `expected(buf, flags, legacy)`: -> (result, bytes or None, [item result]); the first member that is not OK decides.
* `totals(buffers, legacy)`: what the split reports: members, frame chain blocks, legacy members, legacy blocks.
"""
import legacygen as lg
import multiframegen as mg

FRAME, SKIPPABLE, SKIPPABLE_TRUNCATED, LEGACY = 1, 2, 3, 4
SPLIT_LEGACY = 1
Member = mg.Member


def _member(buf, pos, legacy):
    rest = len(buf) - pos
    if legacy and rest >= 4 and mg.u32(buf, pos) == lg.MAGIC:
        w = lg.walk(buf[pos:])
        return Member(pos, w.consumed, LEGACY, 0, len(w.blocks), w.verdict < 0)
    return mg._member(buf, pos)


def split(buf, legacy=True):
    buf = bytes(buf)
    out, pos = [], 0
    while pos < len(buf):
        m = _member(buf, pos, legacy)
        out.append(m)
        if m.last:
            break
        pos += m.len
    return out


def table(buf, legacy=True):
    """what lz4f.multiframeMembers(.., legacy=legacy) reports for `buf`"""
    return [(m.pos, m.len, m.kind, m.nibble) for m in split(buf, legacy)]


def totals(buffers, legacy=True):
    t = [0, 0, 0, 0]
    for b in buffers:
        for m in split(b, legacy):
            t[0] += 1
            if m.kind == LEGACY:
                t[2] += 1
                t[3] += m.nb
            else:
                t[1] += m.nb
    return t


def expected(buf, flags=0, legacy=True):
    """an item result is the member's decoded size, its code, or None for a skippable member"""
    buf = bytes(buf)
    items, parts, code = [], [], None
    for m in split(buf, legacy):
        body = buf[m.pos:m.pos + m.len]
        if m.kind in (FRAME, LEGACY):
            if m.kind == FRAME:
                r = mg._decode_frame(body, flags)
            else:
                rd = lg.read(body)
                r = rd.content if rd.result >= 0 else rd.result
            if isinstance(r, int):
                items.append(r)
                code = r if code is None else code
            else:
                items.append(len(r))
                parts.append(r if code is None else b"")
        else:
            items.append(None)
            if m.kind == SKIPPABLE_TRUNCATED and code is None:
                code = mg.HEADER_INCOMPLETE if m.len < 8 else mg.SIZE_WRONG
    if code is not None:
        return code, None, items
    out = b"".join(parts)
    return len(out), out, items
