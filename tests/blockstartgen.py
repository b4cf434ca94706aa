"""Blocks for the start of a block in the fast compressor: the smallest shapes at which the rule "the window path only
runs behind a match; the block's first search takes the generic path" can go wrong.

The first search of a block is the only one without a pending put of its anchor: position 0 is neither probed nor put,
the first probe is position 1.  Every shape below is cut to every size of SIZES (205 is the first size at which the
window path's bound anchor + 192 < L = size - 12 can hold at all, 204 the last at which it cannot); a shape whose
feature lies past the cut is still a valid block.  The heads are uniform random bytes, in which no 4-byte sequence
occurs twice (checked), so the only matches up to the end of the head are the planted ones; behind the head comes
D-text, so that the window path takes over after the first match and runs to the end of the block.

corpus() -> [(name, bytes)], the same list on every call."""
import numpy as np

import datagen as dg

SIZES = (13, 204, 205, 206, 260, 300, 4096, 65536)


def _rand(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _no_repeat(b):
    seen = set()
    for i in range(len(b) - 3):
        g = b[i:i + 4]
        if g in seen:
            return False
        seen.add(g)
    return True


def _head(n, seed):
    """n random bytes without a repeated 4-byte sequence"""
    while True:
        h = _rand(n, seed)
        if _no_repeat(h):
            return bytearray(h)
        seed += 1000


def _plant(h, src, dst, n):
    h[dst:dst + n] = h[src:src + n]


def shapes():
    """-> [(name, head bytes)]: the crafted start of a block; D-text follows it"""
    out = []
    # a one-byte run from position 0 (the probe at 1 finds an empty slot: position 0 was never put; the first match is
    # at 2 against 1) and from position 1 behind one other byte
    out.append(("run@0", b"\x41" * 90 + bytes(_head(30, 1))))
    out.append(("run@1", b"\x42" + b"\x41" * 90 + bytes(_head(30, 2))))
    # first match at lanes 2 (see run@1: it needs the candidate at 1), 62, 63 and 64 of what used to be the first
    # window, 9 bytes long, against position 10
    for p in (62, 63, 64):
        h = _head(160, 10 + p)
        _plant(h, 10, p, 9)
        out.append(("first@%d" % p, bytes(h)))
    # no match in the first 64, 128, 300 positions, then repeats of the head: the first search leaves its first generic
    # batch, and (300) its step schedule passes stride 1
    for n in (64, 128, 300):
        h = _head(n, 20 + n)
        out.append(("nomatch%d" % n, bytes(h) + bytes(h[7:40]) + bytes(_head(11, 21 + n)) + bytes(h[3:30])))
    # Q1: the four bytes at position 0 occur again at r and nothing else matches before.  Position 0 is never a
    # candidate, so the occurrence at r is NOT a match; `first`: a third occurrence at r + 20 is the block's first match
    # (against r); `after`: an unrelated 8-byte match (positions 12 -> 24) comes first, so the occurrence at r is
    # probed from a window (r = 5 cannot lie behind an earlier match unless the bytes are one run: there the block
    # starts with 12 equal bytes, the match at 2 covers position 5)
    for r in (5, 40, 70):
        h = _head(140, 30 + r)
        _plant(h, 0, r, 4)
        _plant(h, 0, r + 20, 6)
        out.append(("q1first@%d" % r, bytes(h)))
        if r == 5:
            h = bytearray(b"\x43" * 12) + _head(128, 35)
        else:
            h = _head(140, 40 + r)
            _plant(h, 12, 24, 8)
            _plant(h, 0, r, 4)
        out.append(("q1after@%d" % r, bytes(h)))
    # a first match of 44 bytes or more (the exact step's extension) and of 270 or more (immediate emission), right
    # behind the generic start, and the same as the SECOND match (the first one a window resolves).  (past 66 probes a
    # search steps by 2 and more, so a planted repeat may be found a few bytes in: 280 and 320 leave 270 or more)
    for ml in (44, 50, 280, 320):
        h = _head(40 + ml + 8, 50 + ml)
        out.append(("long%d" % ml, bytes(h) + bytes(h[16:16 + ml])))
        h2 = _head(60 + ml + 8, 60 + ml)
        _plant(h2, 6, 20, 5)
        out.append(("long%d_second" % ml, bytes(h2) + bytes(h2[30:30 + ml])))
    return out


_CACHE = []


def corpus():
    if not _CACHE:
        text = bytes(dg.text_bytes(65536, 2700))
        for name, head in shapes():
            full = head + text[:65536 - len(head)]
            for n in SIZES:
                _CACHE.append(("%s/%d" % (name, n), full[:n]))
        for dist in ("text", "reptext"):
            for i, b in enumerate(dg.make_blocks(dist, 16, 65536, seed=27)):
                _CACHE.append(("D-%s/%d" % (dist, i), bytes(b)))
    return list(_CACHE)


def first_match(stream):
    """(position, length, offset) of the first match of an LZ4 block, None if it has none"""
    t = stream[0]
    p, lit = 1, t >> 4
    if lit == 15:
        while True:
            x = stream[p]; p += 1; lit += x
            if x != 255:
                break
    p += lit
    if p >= len(stream):
        return None
    off = stream[p] | (stream[p + 1] << 8)
    p += 2
    ml = t & 15
    if ml == 15:
        while True:
            x = stream[p]; p += 1; ml += x
            if x != 255:
                break
    return lit, ml + 4, off
