"""Blocks built on the decision edges of the plain compressors (tests/test_edge_corpus_cpu.py,
tests/test_gpu_edge_corpus.py): zlz4_batch_compress_fast and zlz4_batch_compress_hc at levels 2-12.

A pure generator: no GPU, no oracle.  `cases()` gives [(family, name, bytes, meta)]; every case puts ONE comparison of
the reference on its edge, and comes with a twin on the other side of it:

* far          the reach of a plain candidate: a 48-byte copy exactly d = 65534 .. 65537 bytes behind its source
               (accepted while d <= 65535: src/lz4.zig MAX_DISTANCE, src/lz4hc.zig:573 / :579)
* pattern_far  a run of a 1-, 2- or 4-byte pattern whose earlier occurrence ends 65520 .. 65535 bytes back: the pattern
               step of levels >= 9 relocates the candidate, clamps it to the lowest reachable index and accepts it only
               at distance <= 65535 (src/lz4hc.zig:626-669)
* early_exit   the chain walk ends at the first candidate LONGER than the level's attempt count, although an older one
               is longer still (src/lz4hc.zig:613): candidates of nb - 1 .. nb + 2 bytes, behind 0 .. 9 short decoys
* budget       K occurrences of a 4-byte prefix, the oldest the only long one: the attempts run out exactly there
               (src/lz4hc.zig:571)
* pos0         position 0 is never a match source (src/lz4hc.zig:571, `mi > 0`; src/lz4.zig: the empty table entry)

Level 2 (lz4mid) runs through these blocks too, but its own decisions live in tests/midgen.py.

`meta` names what the case is about: "probe" (lo, hi) is the region of the block where the decision shows, "twin" the
name of the case on the other side of the edge, "accept" which side this one is on by construction (the CPU test
witnesses it on the oracle, setting by setting), and the family's own parameters.  `rnd()` has no zero byte, so a zero
filler or a prefix with a zero in it never matches it.  `walk()` is the token walk that reads a parse off a stream.
"""
import numpy as np

MAX_DIST = 65535
U16_BLOCK_MAX = 65536 + 11                           # the largest block of the fast compressor's 16-bit table
ATTEMPTS = {3: 4, 4: 8, 5: 16, 8: 128, 9: 256, 10: 96, 11: 512, 12: 16384}   # level -> nbSearches
HC_LEVELS = (2, 3, 4, 5, 8, 9, 10, 11, 12)
ACCELS = (1, 4, 65537)

FAR_D = (65534, 65535, 65536, 65537)
FAR_K = (0, 1, 31, 62, 63, 64, 65, 130)
# seeds of the literal run R_k and of the random filler: fixed, because the flip needs a copy without a second source
# (and, with the random filler, fewer filler positions on the chain of the copy's start than level 3 has attempts);
# tests/test_edge_corpus_cpu.py witnesses for every k that the oracle's parse flips between d = 65535 and 65536
FAR_R_SEED = {0: 100, 1: 101, 31: 131, 62: 162, 63: 163, 64: 164, 65: 165, 130: 230}
FAR_FILL_SEED = 300
# Bytes behind the copy / behind pos0's second G.  k_compress_fast resolves a 64-position window from registers only
# while anchor + 192 lies inside the block; with the 40 (30) bytes the parse itself needs, the copy would always be
# searched by the kernel's generic path and the window's own reach and position-0 tests never run on the edge.
FAR_TAIL = 256
POS0_TAIL = 230

PATTERNS = (b"a", b"ab", b"abcd")
PATTERN_GAPS = tuple(range(65520, 65536))
PATTERN_DEEP_REACH = (257, 258, 259, 300, 499, 500, 501, 600)

MAX_DECOYS = 9

# budget: per level (K, K + 1): with K occurrences of the prefix the walk still reaches the oldest (44 bytes), with one
# more it does not (40 bytes).  Chain members that only share the hash would use attempts too; with these seeds there
# are none, and K is the level's attempt count itself.  tests/test_edge_corpus_cpu.py witnesses each pair on the oracle.
BUDGET_K = {3: 4, 4: 8, 5: 16, 6: 32, 7: 64, 8: 128, 9: 256}
BUDGET_PREFIX = b"\x00\xfe\x00\xfd"


def rnd(n, seed):
    return np.random.default_rng(seed).integers(1, 256, n, dtype=np.uint8).tobytes()


def walk(stream):
    """Token walk of an LZ4 block -> [(position of the match in the decoded block, offset, match length)]"""
    s = memoryview(stream)
    n, i, out, seqs = len(s), 0, 0, []
    while True:
        tok = s[i]; i += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                x = s[i]; i += 1
                lit += x
                if x != 255:
                    break
        i += lit
        out += lit
        if i >= n:
            assert i == n, "the last literal run passes the end of the stream"
            return seqs
        off = s[i] | (s[i + 1] << 8); i += 2
        assert 0 < off <= out
        ml = tok & 15
        if ml == 15:
            while True:
                x = s[i]; i += 1
                ml += x
                if x != 255:
                    break
        seqs.append((out, off, ml + 4))
        out += ml + 4


def in_probe(seqs, probe):
    """the sequences that START inside the probe region"""
    return [q for q in seqs if probe[0] <= q[0] < probe[1]]


def far_block(d, k, filler):
    """X + filler(z) + R_k + X[8:56] + rnd(40) + rnd(216): the copy starts d bytes behind X[8], after a literal run of
    k bytes"""
    x = rnd(64, 1)
    z = d - 56 - k
    fill = bytes(z) if filler == "zero" else rnd(z, FAR_FILL_SEED)
    b = x + fill + rnd(k, FAR_R_SEED[k]) + x[8:56] + rnd(40, 2) + rnd(FAR_TAIL - 40, 3)
    p = 64 + z + k
    assert p - 8 == d and len(b) == d + 56 + FAR_TAIL
    return b, (p, p + 48)


def _far():
    out = []
    for filler in ("zero", "rnd"):
        for k in FAR_K:
            for d in FAR_D:
                b, probe = far_block(d, k, filler)
                twin = d + 2 if d <= MAX_DIST else d - 2
                out.append(("far", "far/%s/k%d/d%d" % (filler, k, d), b,
                            dict(probe=probe, accept=d <= MAX_DIST, twin="far/%s/k%d/d%d" % (filler, k, twin), d=d, k=k,
                                 filler=filler, fast=filler == "zero")))
    return out


def pattern_block(pat, first, gap, second):
    head = rnd(16, 11) + (pat * 700)[:first]
    b = head + rnd(gap, 12) + (pat * 700)[:second] + rnd(20, 13)
    p = len(head) + gap
    return b, (p, p + second)


def _pattern_far():
    out = []
    for pat in PATTERNS:
        for first, second in ((300, 100), (100, 300)):
            for gap in PATTERN_GAPS:
                b, probe = pattern_block(pat, first, gap, second)
                out.append(("pattern_far", "pattern_far/%s/%d_%d/gap%d" % (pat.decode(), first, second, gap), b,
                            dict(probe=probe, pat=pat, gap=gap, first=first, second=second, fast=True)))
    # In the blocks above the walk itself reaches the lowest index (at most 12 candidates are in reach), and the pattern
    # step that follows it is refused there.  Here `reach` bytes of a 700-byte run are in reach: the walk of a level
    # with nb < reach - 1 attempts leaves early at nb + 1 bytes, and only the pattern step finds the rest of the run.
    for reach in PATTERN_DEEP_REACH:
        b, probe = pattern_block(b"a", 700, MAX_DIST - reach, 500)
        out.append(("pattern_far", "pattern_far/a/deep/reach%d" % reach, b,
                    dict(probe=probe, pat=b"a", gap=MAX_DIST - reach, first=700, second=500, reach=reach, fast=True)))
    return out


def early_exit_block(e, decoys):
    """rnd(8) 01 S rnd(20) 02 S[:e] (S[e] ^ 0x55) rnd(30) [decoys] rnd(20) 03 S rnd(20), S = rnd(e + 100, 7).
    -> (block, probe, position of the old copy, position of the new copy)"""
    s = rnd(e + 100, 7)
    b = rnd(8, 21) + b"\x01"
    old = len(b)
    b += s + rnd(20, 22) + b"\x02"
    new = len(b)
    b += s[:e] + bytes([s[e] ^ 0x55]) + rnd(30, 23)
    for j in range(decoys):                           # S[:4], a fifth byte that differs, other bytes
        b += bytes([0x80 + j]) + s[:4] + bytes([s[4] ^ (j + 1)]) + rnd(7, 40 + j)
    b += rnd(20, 24) + b"\x03"
    p = len(b)
    b += s + rnd(20, 25)
    return b, (p, p + len(s)), old, new


def _early_exit():
    out = []
    for level, nb in ATTEMPTS.items():
        for j in range(min(MAX_DECOYS, nb - 2) + 1):
            for e in (nb - 1, nb, nb + 1, nb + 2):
                b, probe, old, new = early_exit_block(e, j)
                twin = e + 2 if e <= nb else e - 2
                out.append(("early_exit", "early_exit/l%d/e%d/j%d" % (level, e, j), b,
                            dict(probe=probe, accept=e <= nb, twin="early_exit/l%d/e%d/j%d" % (level, twin, j),
                                 level=level, nb=nb, e=e, decoys=j, old=old, new=new, fast=True)))
    return out


def budget_block(k):
    """k occurrences of the prefix before the probe: the oldest is followed by the 40 bytes the probe repeats, the
    others by something else.  -> (block, probe, position of the oldest occurrence)"""
    t = rnd(40, 31)
    b = rnd(8, 32) + b"\x01"
    old = len(b)
    b += BUDGET_PREFIX + t + rnd(12, 33)
    for i in range(k - 1):
        b += BUDGET_PREFIX + bytes([t[0] ^ (1 + i % 255)]) + rnd(6, 1000 + i)
    b += rnd(10, 34) + b"\x02"
    p = len(b)
    b += BUDGET_PREFIX + t + rnd(20, 35)
    return b, (p, p + 44), old


def _budget():
    out = []
    for level, k0 in BUDGET_K.items():
        for k in (k0, k0 + 1):
            b, probe, old = budget_block(k)
            out.append(("budget", "budget/l%d/k%d" % (level, k), b,
                        dict(probe=probe, accept=k == k0, twin="budget/l%d/k%d" % (level, 2 * k0 + 1 - k), level=level,
                             k=k, old=old, fast=True)))
    return out


def _pos0():
    g = rnd(16, 5)
    b = g + rnd(100, 6) + g + rnd(30, 8) + rnd(POS0_TAIL - 30, 9)
    # near: the second G lies in the first 64 positions, the ones k_compress_fast resolves as its first window
    c = g + rnd(30, 6) + g + rnd(30, 8) + rnd(POS0_TAIL - 30, 9)
    return [("pos0", "pos0/pos0", b, dict(probe=(116, 132), accept=False, twin="pos0/pos1", fast=True)),
            ("pos0", "pos0/pos1", b"\x09" + b, dict(probe=(117, 133), accept=True, twin="pos0/pos0", fast=True)),
            ("pos0", "pos0/near0", c, dict(probe=(46, 62), accept=False, twin="pos0/near1", fast=True)),
            ("pos0", "pos0/near1", b"\x09" + c, dict(probe=(47, 63), accept=True, twin="pos0/near0", fast=True))]


_cases = None


def cases():
    """-> [(family, name, bytes, meta)]; built once"""
    global _cases
    if _cases is None:
        _cases = _far() + _pattern_far() + _early_exit() + _budget() + _pos0()
        assert len({n for _, n, _, _ in _cases}) == len(_cases)
    return _cases


def small(cs=None):
    """the cases of at most 65 536 bytes (every family but far and pattern_far)"""
    return [c for c in (cases() if cs is None else cs) if len(c[2]) <= 65536]


def large(cs=None):
    return [c for c in (cases() if cs is None else cs) if len(c[2]) > 65536]
