"""Corpus and model of the lz4f block chain walk (tests/test_frame_chain_cpu.py, tests/test_gpu_frame_chain.py; DESIGN.md
section 4.4; src/lz4f.zig:563-600).  Test infrastructure: the walk below is written out from the frame format and shares
no code with the product.

* `frames()`: tiny frames of three independent blocks -- 64 bytes of sequences, a stored block of 20 bytes, 44 bytes of
  sequences -- with block checksum off / on x content checksum off / on, each also with a zero-size stored block in front
  of the first block, with the first block word replaced by 0x7FFFFFFF, and with 8 bytes (the frame magic first) behind it.
* `cases()`: every prefix frame[:cut], cut in 0 .. len(frame), of every frame.  Nothing is left out.
* `walk(case)`: (header size or error, blocks, cursor after the walk, how the walk ended).
"""
import functools
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools", "pyref"))
import dictgen  # noqa: E402
import linkedgen  # noqa: E402
from zig_lz4_sizes import xxh32  # noqa: E402

seq, pat = dictgen.seq, dictgen.pattern
MAGIC = 0x184D2204
HEADER = 7                                            # magic, FLG, BD, header checksum
TAIL = pat(9, 33)
VARIANTS = ((0, 0), (0, 1), (1, 0), (1, 1))           # (block checksum, content checksum)
# how a walk ends: the input ends at a block boundary (:563), inside a block word (:565), at the end mark (:573), inside
# a block's data (:582), inside a block's checksum word (:591: that block still counts)
BOUNDARY, WORD_CUT, END_MARK, DATA_CUT, CKS_CUT, NO_HEADER = "boundary", "word_cut", "end_mark", "data_cut", "cks_cut", "no_header"


def _blocks():
    b0 = seq(pat(46, 80), 20, 9) + seq(TAIL)          # 46 + 9 + 9 = 64
    b1 = pat(20, 81)                                  # stored
    b2 = seq(pat(12, 82), 5, 23) + seq(TAIL)          # 12 + 23 + 9 = 44
    return [(b0, False), (b1, True), (b2, False)]


def _content():
    a, c = pat(46, 80), pat(12, 82)
    d0 = bytearray(a)
    for _ in range(9):
        d0.append(d0[-20])
    d2 = bytearray(c)
    for _ in range(23):
        d2.append(d2[-5])
    return bytes(d0) + TAIL + pat(20, 81) + bytes(d2) + TAIL


CONTENT_SIZE = 128


@functools.lru_cache(maxsize=None)
def frames():
    """-> [(name, block checksum, content checksum, frame)]"""
    content = _content()
    assert len(content) == CONTENT_SIZE
    out = []
    for bc, cc in VARIANTS:
        base = linkedgen.build_frame(_blocks(), bool(bc), content if cc else None, block_mode=1)
        tag = "bc%d_cc%d" % (bc, cc)
        zero = (0x80000000).to_bytes(4, "little") + (xxh32(b"").to_bytes(4, "little") if bc else b"")
        out.append((tag, bc, cc, base))
        out.append((tag + "_zero_stored", bc, cc, base[:HEADER] + zero + base[HEADER:]))
        out.append((tag + "_huge_word", bc, cc, base[:HEADER] + (0x7FFFFFFF).to_bytes(4, "little") + base[HEADER + 4:]))
        out.append((tag + "_trailing", bc, cc, base + MAGIC.to_bytes(4, "little") + b"\x60\x40\x82\x00"))
    assert all(len(f) <= 190 for _, _, _, f in out)
    return out


@functools.lru_cache(maxsize=None)
def cases(bc=None, cc=None, only=None):
    """-> [(name, bytes)]: every prefix of every frame; bc / cc select a variant, `only` the frames whose name ends so"""
    out = []
    for name, fbc, fcc, f in frames():
        if (bc is not None and fbc != bc) or (cc is not None and fcc != cc):
            continue
        if only is not None and not any(name.endswith(s) for s in only):
            continue
        out += [("%s[:%d]" % (name, cut), f[:cut]) for cut in range(len(f) + 1)]
    return out


def _header(b):
    """header size or the error code (every corpus header is the 7-byte one, cut or whole)"""
    if len(b) < HEADER:
        return -112                                   # FrameHeaderIncomplete
    assert int.from_bytes(b[:4], "little") == MAGIC and b[4] & 0xC9 == 0x40 and b[5] == 0x40
    assert b[6] == (xxh32(b[4:6]) >> 8) & 0xFF
    return HEADER


@functools.lru_cache(maxsize=None)
def walk(b):
    """-> (header size or error, blocks, cursor after the walk, ending).  The cursor stands behind the last whole thing the
    walk took: a block with its checksum word, the end mark, and -- where a block's data is cut -- that block's word."""
    hs = _header(b)
    if hs < 0:
        return hs, 0, 0, NO_HEADER
    bc = bool(b[4] & 0x10)
    n, pos, nb = len(b), hs, 0
    while True:
        if pos >= n:
            return hs, nb, pos, BOUNDARY
        if pos + 4 > n:
            return hs, nb, pos, WORD_CUT
        w = int.from_bytes(b[pos:pos + 4], "little")
        if w == 0:
            return hs, nb, pos + 4, END_MARK
        size = w & 0x7FFFFFFF
        if pos + 4 + size > n:
            return hs, nb, pos + 4, DATA_CUT
        pos += 4 + size
        nb += 1
        if bc:
            if pos + 4 > n:
                return hs, nb, pos, CKS_CUT
            pos += 4
