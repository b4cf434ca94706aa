"""Blocks on both sides of 2^24 bytes (tests/test_big_block_inputs_cpu.py, tests/test_gpu_blocks_16mib.py).

At max_in_len > 2^24 the fast compressor's 32-bit table carries no tag (a position no longer fits beside it) and the
level 3-9 search keeps no counted runs (their packed entry has 24-bit fields).  `blocks()` gives text that ends on, just
past and well past that size, and two blocks whose last 20 000 bytes have a period of 256, so that the run every start
point meets ends at n - 5 = 0xFFFFFB (the top of the 24-bit field) or 12 bytes past it.  `planted_blocks()` gives the
two seeded blocks for the streaming compressor: one whose seed lies at or above 2^24, one whose seed is the highest the
tagged table can hold.  `walk()` counts what a compressed stream proves about positions at or above 2^24.
"""
import numpy as np

import datagen as dg
import streamgen as sg

T = 1 << 24
TAIL = 20000                                     # bytes of period 256 at the end of tailT / tailT+12 (not to be enlarged:
#                                                  above 2^24 the search counts that run once per start point)
AT_T = ("T", "tailT")                            # run with max_in_len == T; the others with their own maximum


def text():
    return bytes(dg.text_bytes(T + 70001, 5))


def blocks(tx=None):
    """-> {name: bytes}, in the order T, T+1, T+70001, tailT, tailT+12"""
    tx = text() if tx is None else tx
    assert len(tx) == T + 70001
    pat = bytes(dg.random_bytes(256, 2024))
    tail = (pat * (TAIL // 256 + 1))[:TAIL]
    return {"T": tx[:T], "T+1": tx[:T + 1], "T+70001": tx, "tailT": tx[:T - TAIL] + tail,
            "tailT+12": tx[:T - TAIL + 12] + tail}


def planted_blocks():
    """-> {name: (block, table)}: streamgen.planted blocks with the table that holds their seed.
    "above": the seed v = run_end - 2 = 2^24 + 98 does not fit a 24-bit position; "top": v = 2^24 - 52 is just under
    L = n - 12, the highest a tagged entry of a 2^24-byte block can hold."""
    out = {}
    for name, n, seed, run_end in (("above", T + 5000, 11, T + 100), ("top", T, 12, T - 50)):
        b, v, G = sg.planted(n, seed, run_end=run_end, r_off=20)
        assert v == run_end - 2 and len(b) == n
        t = np.zeros(sg.ENTRIES, np.uint32)
        t[sg.hash4(G)] = v
        out[name] = (b, t)
    return out


def walk(stream, at=T):
    """Token walk of an LZ4 block -> (decoded size, matches whose source starts at or above `at`, matches whose target
    starts at or above `at` and whose source starts below it).  No byte is copied."""
    s = memoryview(stream)
    n, i, out, src_high, crossing = len(s), 0, 0, 0, 0
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
            return out, src_high, crossing
        off = s[i] | (s[i + 1] << 8); i += 2
        assert 0 < off <= out
        ml = tok & 15
        if ml == 15:
            while True:
                x = s[i]; i += 1
                ml += x
                if x != 255:
                    break
        if out >= at:
            if out - off >= at:
                src_high += 1
            else:
                crossing += 1
        out += ml + 4
