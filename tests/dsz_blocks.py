"""Crafted inputs for the compressDestSize tests: blocks whose first sequence has a chosen literal-run length.

The step after the attempt that found a match depends on how far into the search the match lies (the skip schedule of
src/lz4.zig:327-333).  Runs of 32 q (q + 1) + 2 bytes (66, 194, 386, 642, 962, 1346, ...) are the first position
reached with step q + 1; random data rarely produces them, so these blocks place them on purpose."""
import datagen as dg

# 32 q (q + 1) + 2 for q = 1..6, and the visited positions just before and after the first two (the search skips
# 67, 193 and 195: no match can start there)
EDGE_RUNS = (65, 66, 68, 192, 194, 197, 386, 642, 962, 1346)


def first_literal_run(stream):
    """literal-run length of the first sequence of an LZ4 block stream"""
    tok = stream[0]
    lit, q = tok >> 4, 1
    if lit == 15:
        while True:
            b = stream[q]
            q += 1
            lit += b
            if b != 255:
                break
    return lit


def block_with_first_run(compress_default, lit, tail=300):
    """random bytes of lit + tail bytes whose compressDefault stream starts with a `lit`-byte literal run followed by a
    match (bytes [lit, lit + 8) repeat bytes [10, 18)); seeds are tried in order until the stream shows it (a hash
    collision can evict position 10 before the search reaches `lit`)"""
    n = lit + tail
    for seed in range(1, 200):
        b = bytearray(dg.random_bytes(n, 7000 + 131 * lit + seed).tobytes())
        b[lit:lit + 8] = b[10:18]
        b = bytes(b)
        if first_literal_run(compress_default(b)) == lit:        # (< n: a match follows)
            return b
    raise AssertionError("no block found for a %d-byte first literal run" % lit)
