"""The serial walk of k_sd_finish (zig-lz4_amd/csrc/zlz4_stream_decode.hip): calls that only the walk can decode, one by
one through decode_block_wave (zlz4_device.hpp), against tools/pyref/zig_lz4_stream_decode.py on the same device
addresses (tests/stream_decode_harness.py: every result, every successful slot's bytes, every final state).

How a call reaches the walk.  k_sd_plan looks back kLookback = 64 calls for the last success; a run that opens with 70
corrupt calls leaves every later call unresolved, so k_sd_finish walks the run with its true entry state and re-decodes
each call whose true key differs from the key it was guessed with (the guess: the call before it succeeded with r > 0,
so its key is the bound max(0, dst[j - 1] - dst[j])).  Hence, below:
  * with a dictionary pending, every call up to and including the first success has the dictionary key, which no guess
    is: the walk decodes them with decode_block_wave<true, true>;
  * without one, a call whose predecessor failed and lies elsewhere than the last success has a true bound other than
    the guessed one: the walk decodes it with decode_block_wave<true, false, true>.  A call directly behind a success is
    guessed right and never walked, so every call under test stands behind a corrupt one.
The expected results in the tables are worked out from the streams by hand; the model decides, and both must agree.

A match offset has 16 bits, so with a dictionary of 70 000 bytes no match can reach past (or onto) the first of its last
65 536 bytes: the farthest reachable byte is tend - 65535, from op = 0.  The accepted / refused pair at the dictionary's
first byte is therefore run on a dictionary of 300 bytes, next to the 70 000-byte one."""
import pytest

import datagen as dg
import dictgen
from dictgen import pattern, seq
from stream_decode_harness import batch as _batch

pytestmark = pytest.mark.gpu

BAD = b"\xF0"                    # a literal run of 15 whose extension byte is missing: CorruptedData under every key
NBAD = 70                        # > kLookback
W = bytes(range(0xA0, 0xA8))
TAIL = b"ENDOFBLOCKLITS"
OTS, CORRUPT = -1, -3

L526 = W + W + pattern(526 - 16, seed=1)          # 15 + 255 + 255 + 1: the length-extension chain 255, 255, 1
SHAPES_LEN = 526 + 2000 + 600 + 2000 + 5 + 2000 + 5 + 2000 + len(TAIL)


def _copy_shapes(head=b""):
    """`head` (whole sequences), the 526-byte literal run, then overlapping matches of 2 000 bytes at offsets 1, 3 and
    1023 (the doubling copy) and 1024 (the plain copy at distance >= 1024)"""
    return (head + seq(L526, 1, 2000) + seq(pattern(600, seed=2), 3, 2000) + seq(b"x1023", 1023, 2000)
            + seq(b"y1024", 1024, 2000) + seq(TAIL))


def _failing(match_off):
    """(name, stream, capacity, expected) of the calls that fail whatever lies in front of the block; match_off: an
    offset that is valid for a match behind 20 literals"""
    return [("literal run, capacity one short", seq(L526), 525, OTS),
            ("match, capacity one short", seq(b"0123456789" * 2, match_off, 30), 49, OTS),
            ("literal length chain cut", b"\xF0\xFF\xFF", 64, CORRUPT),
            ("match length chain cut", seq(b"abcd", 2, 4 + 15 + 255)[:-1], 400, CORRUPT),
            ("offset missing", b"\x40abcd\x01", 64, CORRUPT)]


def _check(got, first, table):
    for k, (name, _, _, exp) in enumerate(table):
        assert got[first + k] == exp, "%s: %d, worked out %d" % (name, got[first + k], exp)


def test_pending_dictionary(zl, gpu, tmp_path):
    """Three runs, each behind 70 corrupt calls with its dictionary still pending.
    Run 0, 70 000-byte dictionary: the failing shapes (the state stays), then one block with a match from the farthest
    reachable dictionary byte, one wholly inside the dictionary, one that starts 3 bytes in front of its end and runs on
    into the output, then the copy shapes.
    Run 1, 300-byte dictionary: offset = op + 301 (CorruptedData), then a block that opens with 2 dictionary bytes
    repeated with period 2 across the dictionary's end (the doubling copy behind the dictionary part) and reaches the
    dictionary's first byte with offset = op + 300.
    Run 2: a block of dictgen.encoder (dictionary matches as a compressor places them)."""
    big, small = pattern(70000, seed=70), pattern(300, seed=71)
    text = bytes(dg.make_blocks("text", 1, 70000, seed=40)[0])
    raw = text[5000:5700] + text[60000:60500]
    enc = dictgen.encoder(tmp_path)(text, raw)[0]
    head = seq(b"", 65535, 20) + seq(b"0123456789", 30 + 5000, 300) + seq(b"abcde", 335 + 3, 200)
    tables = [_failing(20 + 30) + [("dictionary matches and copy shapes", _copy_shapes(head), 535 + SHAPES_LEN + 7,
                                   535 + SHAPES_LEN)],
              [("one byte in front of the dictionary", seq(b"0123456789", 10 + 301, 4) + seq(TAIL), 64, CORRUPT),
               ("across the end, and the first byte", seq(b"", 2, 50) + seq(b"0123456789", 60 + 300, 4) + seq(TAIL), 128,
                50 + 10 + 4 + len(TAIL))],
              [("encoder block", enc, len(raw), len(raw))]]
    region = 16384
    runs = []
    for s, table in enumerate(tables):
        calls, pos = [(BAD, s * region + i, 1) for i in range(NBAD)], s * region + 128
        for _, src, cap, _ in table:
            calls.append((src, pos, cap))
            pos += cap
        assert pos <= (s + 1) * region
        runs.append(calls)
    got, _ = _batch(zl, gpu, runs, region * len(tables), dicts=[big, small, text], fill=0x5A)
    first = 0
    for s, table in enumerate(tables):
        assert got[first:first + NBAD] == [CORRUPT] * NBAD
        _check(got, first + NBAD, table)
        first += len(runs[s])


def test_bound_entry(zl, gpu):
    """One run without a dictionary.  The 70 corrupt calls lie at the top of the buffer and the slots go downwards, so
    every guess is a bound > 0.  First the true bound is 0 (nothing has succeeded): the failing shapes, a match in front
    of the output, then the copy shapes, which succeed at address P.  From there on the previous output lies above the
    new destination: each call under test has dst = P - 100, hence lo = 100, and stands behind a corrupt call at the top
    (guessed bound: thousands).  Its literals restate the bytes that lie there and the first 8 bytes at P, its match
    copies 8 bytes to out[108 .. 116): op - offset = 99 and offset > op are CorruptedData, op - offset = 100 is accepted
    and reads P's first bytes.  The slot overlaps the output at P, which a StreamDecode caller may do; whatever is
    written there equals what P holds (its output opens with W + W), so the order of the writes does not matter."""
    top, lo = 30000, 100
    below = pattern(200, seed=5)                       # what lies in the `lo` bytes in front of P
    calls = [(BAD, top + i, 1) for i in range(NBAD)]
    phase1 = _failing(4) + [("match in front of the output, lo = 0", seq(b"abcd", 5, 4) + seq(TAIL), 64, CORRUPT),
                            ("copy shapes, lo = 0", _copy_shapes(), SHAPES_LEN, SHAPES_LEN)]
    pos = 29000
    for _, src, cap, _ in phase1:
        pos -= cap
        calls.append((src, pos, cap))
    p = pos
    lits = below[200 - lo:] + W                        # op = lo + 8 at the match
    phase2 = [("op - offset = lo - 1", seq(lits, 9, 8), lo + 16, CORRUPT),
              ("offset > op", seq(lits, lo + 9, 8), lo + 16, CORRUPT),
              ("op - offset = lo", seq(lits, 8, 8), lo + 16, lo + 16)]
    for k, (_, src, cap, _) in enumerate(phase2):
        calls.append((BAD, top + NBAD + k, 1))
        calls.append((src, p - lo, cap))
    assert p - 200 >= 0
    got, fin = _batch(zl, gpu, [calls], 32768)
    _check(got, NBAD, phase1)
    assert got[NBAD + len(phase1)::2] == [CORRUPT] * len(phase2)
    _check(got[NBAD + len(phase1) + 1::2], 0, phase2)
