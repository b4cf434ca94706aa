"""Test-side helpers for multiframe buffers (tests/test_multiframe_cpu.py, tests/test_gpu_multiframe.py; include/zlz4_amd.h,
DESIGN.md section 4.4h): a buffer of zero or more lz4 frames and skippable frames back to back, its members.

* `corpus()`: frames of 0, 1, 65 535, 65 536, 65 537 and 200 000 input bytes at 64 KiB blocks from oracle.compress_frame,
  with and without block checksum, content checksum and content size, one of stored blocks, the empty frame.
* `skippable(nibble, payload)`: a hand-made skippable frame.
* `split(buf)`: a model of the split written from the frame format: magic, FLG / BD, the header checksum, the chain of
  block header words up to the end mark, the content checksum word.  Whatever cannot be delimited is the last member.
* `expected(buf, flags)`: the model's members fed one by one to oracle.decompress_frame and concatenated; a linked member
  decodes (with DECODE_LINKED) to the input its fixture records (tests/golden/linked_frames.json).
* `defects()`: buffers with one defective member, last, in the middle and alone.
"""
import collections
import functools
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools", "pyref"))
import datagen as dg  # noqa: E402
import linkedgen  # noqa: E402
from oracle import binding as oracle  # noqa: E402
from zig_lz4_sizes import xxh32  # noqa: E402

MAGIC, SKIP_MAGIC, LEGACY_MAGIC = 0x184D2204, 0x184D2A50, 0x184C2102
FRAME, SKIPPABLE, SKIPPABLE_TRUNCATED = 1, 2, 3
DECODE_LINKED = 1
INVALID_STATE, BLOCK_CHECKSUM, DST_TOO_SMALL, HEADER_INCOMPLETE, TYPE_UNKNOWN = -5, -107, -111, -112, -113
SIZE_WRONG, FAILED, CONTENT_CHECKSUM, PARAMETER_INVALID = -114, -116, -118, -104

Member = collections.namedtuple("Member", "pos len kind nibble nb last")


def u32(b, pos):
    return int.from_bytes(b[pos:pos + 4], "little")


# ----------------------------------------------------------------------------- the model of the split
def _header_size(b):
    """the size of the frame header at b[0], or None where there is no valid one (the frame call names the error)"""
    if len(b) < 7 or u32(b, 0) != MAGIC:
        return None
    flg, bd = b[4], b[5]
    if (flg >> 6) != 1 or flg & 0x02 or bd & 0x8F or ((bd >> 4) & 7) in (1, 2, 3):    # (id 0 reads as the default, 64 KiB)
        return None
    size = 7 + (8 if flg & 0x08 else 0) + (4 if flg & 0x01 else 0)
    if len(b) < size or b[size - 1] != (xxh32(bytes(b[4:size - 1])) >> 8) & 0xFF:
        return None
    return size


def _member(buf, pos):
    n = len(buf)
    rest = n - pos
    if rest >= 4 and (u32(buf, pos) & 0xFFFFFFF0) == SKIP_MAGIC:
        nib = u32(buf, pos) & 15
        if rest < 8 or 8 + u32(buf, pos + 4) > rest:
            return Member(pos, rest, SKIPPABLE_TRUNCATED, nib, 0, True)
        return Member(pos, 8 + u32(buf, pos + 4), SKIPPABLE, nib, 0, False)
    open_end = Member(pos, rest, FRAME, 0, 0, True)
    hs = _header_size(buf[pos:pos + 19])
    if hs is None:
        return open_end
    flg = buf[pos + 4]
    p, nb = pos + hs, 0
    while True:
        if p + 4 > n:                                 # no end mark, or a torn header word
            return open_end._replace(nb=nb)
        w = u32(buf, p)
        p += 4
        if w == 0:
            break
        if p + (w & 0x7FFFFFFF) > n:                  # the block runs off the buffer
            return open_end._replace(nb=nb)
        p += w & 0x7FFFFFFF
        nb += 1
        if flg & 0x10:
            if p + 4 > n:
                return open_end._replace(nb=nb)
            p += 4
    if flg & 0x04:
        if p + 4 > n:
            return open_end._replace(nb=nb)
        p += 4
    return Member(pos, p - pos, FRAME, 0, nb, False)


def split(buf):
    """-> [Member]: the members of `buf` in order (nb = the blocks of a frame member's chain)"""
    buf = bytes(buf)
    out, pos = [], 0
    while pos < len(buf):
        m = _member(buf, pos)
        out.append(m)
        if m.last:
            break
        pos += m.len
    return out


def table(buf):
    """what lz4f.multiframeMembers reports for `buf`"""
    return [(m.pos, m.len, m.kind, m.nibble) for m in split(buf)]


# ----------------------------------------------------------------------------- frames
def skippable(nibble=0, payload=b""):
    return (SKIP_MAGIC | nibble).to_bytes(4, "little") + len(payload).to_bytes(4, "little") + bytes(payload)


def _prefs(bc, cc, cs):
    p = oracle.Prefs()
    p.block_size_id, p.block_mode, p.block_checksum, p.content_checksum, p.content_size = 4, 1, bc, cc, cs
    return p


SIZES = (0, 1, 65535, 65536, 65537, 200000)
Frame = collections.namedtuple("Frame", "name frame content bc cc")


@functools.lru_cache(maxsize=None)
def corpus():
    """-> [Frame]; chains of 0 to 4 blocks"""
    out = []
    text = bytes(dg.text_bytes(SIZES[-1], 41))
    for n in SIZES:
        for bc in (0, 1):
            for cc in (0, 1):
                for cs in (0, 1):
                    data = text[:n]
                    f = oracle.compress_frame(data, _prefs(bc, cc, n if cs else 0))
                    out.append(Frame("text%d_bc%d_cc%d_cs%d" % (n, bc, cc, cs), f, data, bc, cc))
    rnd = bytes(dg.random_bytes(70000, 7))
    for bc, cc in ((0, 0), (1, 1)):
        out.append(Frame("stored_bc%d_cc%d" % (bc, cc), oracle.compress_frame(rnd, _prefs(bc, cc, 0)), rnd, bc, cc))
    assert u32(out[-1].frame, 7) & 0x80000000, "random bytes make a stored block"
    assert out[0].content == b"" and len(out[0].frame) == 11, "the empty frame"
    return out


def pick(*names):
    by = {c.name: c for c in corpus()}
    return [by[n] for n in names]


def few():
    """a handful of corpus frames that covers every block count and every checksum"""
    return pick("text0_bc0_cc0_cs0", "text1_bc1_cc1_cs1", "text65535_bc0_cc1_cs0", "text65536_bc1_cc0_cs1",
                "text65537_bc1_cc1_cs0", "text200000_bc0_cc0_cs1", "text200000_bc1_cc1_cs1", "stored_bc1_cc1")


@functools.lru_cache(maxsize=None)
def linked():
    """-> [(frame, input)] of the committed linked-block fixtures with 64 KiB blocks"""
    return [(f["frame"], f["input"]) for f in linkedgen.fixtures() if f["recipe"]["block_size_id"] == 4]


# ----------------------------------------------------------------------------- the expected decode
@functools.lru_cache(maxsize=None)
def _decode_frame(member, flags):
    if flags & DECODE_LINKED:
        for frame, data in linked():
            if member == frame:
                return data
    return oracle.decompress_frame(member, 255 * len(member) + 64)


def expected(buf, flags=0):
    """-> (result, bytes or None, [item result]): the first member that is not OK decides; an item result is the member's
    decoded size, its code, or None for a skippable member (the frame calls answer FrameHeaderIncomplete for its item)"""
    buf = bytes(buf)
    items, parts, code = [], [], None
    for m in split(buf):
        if m.kind == FRAME:
            r = _decode_frame(buf[m.pos:m.pos + m.len], flags)
            if isinstance(r, int):
                items.append(r)
                code = r if code is None else code
            else:
                items.append(len(r))
                parts.append(r if code is None else b"")
        else:
            items.append(None)
            if m.kind == SKIPPABLE_TRUNCATED and code is None:
                code = HEADER_INCOMPLETE if m.len < 8 else SIZE_WRONG
    if code is not None:
        return code, None, items
    out = b"".join(parts)
    return len(out), out, items


# ----------------------------------------------------------------------------- defects
def flip(b, pos):
    b = bytearray(b)
    b[pos] ^= 0x40
    return bytes(b)


def defects():
    """-> [(name, buffer, code, members in front of the defect)]: the defective member last, in the middle (where bytes
    may follow it) and alone; the code is stated here so that the tests also pin the model"""
    a, b = pick("text65537_bc1_cc1_cs0", "text1_bc0_cc0_cs1")
    plain = pick("text65536_bc0_cc0_cs0")[0]
    out = []

    def add(name, member, code, middle=True):
        out.append((name + "_last", a.frame + b.frame + member, code, 2))
        out.append((name + "_only", member, code, 0))
        if middle:
            out.append((name + "_middle", a.frame + member + b.frame, code, 1))

    for k in range(1, 8):                             # stray bytes: no header (< 7), or an unknown magic (7)
        add("stray%d" % k, b"\x01" * k, HEADER_INCOMPLETE if k < 7 else TYPE_UNKNOWN, middle=False)
    for k in range(4, 8):
        add("skip_header_%d_bytes" % k, skippable(3, b"")[:k], HEADER_INCOMPLETE, middle=False)
    add("skip_size_one_past", skippable(5, b"x" * 9)[:-1], SIZE_WRONG, middle=False)
    add("skip_size_past_what_follows", (SKIP_MAGIC | 5).to_bytes(4, "little") + (1 << 20).to_bytes(4, "little") + b"y" * 40,
        SIZE_WRONG)
    add("unknown_magic", b"\x05\x22\x4d\x18" + a.frame[4:], TYPE_UNKNOWN)
    add("legacy_magic", LEGACY_MAGIC.to_bytes(4, "little") + (5).to_bytes(4, "little") + b"\x50abcd", TYPE_UNKNOWN)
    add("block_checksum_flipped", flip(a.frame, len(a.frame) - 9), BLOCK_CHECKSUM)       # end mark 4 + content word 4 + 1
    add("content_checksum_flipped", flip(a.frame, len(a.frame) - 1), CONTENT_CHECKSUM)
    # a frame without its end mark swallows what follows: the next magic is read as a block header word
    out.append(("no_end_mark_then_frame", plain.frame[:-4] + b.frame, SIZE_WRONG, 0))
    out.append(("no_end_mark_then_frame_middle", a.frame + plain.frame[:-4] + b.frame, SIZE_WRONG, 1))
    return out
