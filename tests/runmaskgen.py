"""Blocks for the run masks of the fast compressor's window: the end-lane mask E_run beside mm_run, the covered lanes by
subtraction, the literal starts from the end lanes, the fast-run trip with one exit test and the exact step that reads
its lane from masks.  320 to 4096 bytes each (a window needs anchor + 192 < L = size - 12).

A crafted block is a head of uniform random bytes in which no 4-byte sequence occurs twice, a first copy out of the head
(the block's first match, found on the generic path; the window path takes over behind it), then `gap` fresh random
bytes, a copy of `mlen` bytes out of the head -- the match lane `gap` of that window, its end lane gap + mlen -- and one
of the tails below, then fresh random bytes to the end.  gap and mlen sweep the end lane over 62, 63, 64 and beyond, the
literal run over 0, 14, 15 and 16, and the match over the lengths at which the window takes another path (4 + 44 bytes
compared in registers: 47 is the last fast one, 48 the first exact one).  Blocks below 970 bytes leave less than 512
bytes of room from the first window on (`tight`); slices of D-text have the duplicate-hash lanes of real data.

corpus() -> [(name, bytes)], the same list on every call.  events() -> the names of emulate_window.EVENTS that the
windows of the corpus went through in the emulator; corpus() asserts that every one of them occurs."""
import os
import sys

import numpy as np

import datagen as dg

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import emulate_window as ew  # noqa: E402

GAPS = (0, 1, 3, 8, 13, 14, 15, 16, 30, 44, 48, 50, 51, 52, 53, 55, 58, 60, 63, 64, 70)
MLENS = (8, 12, 47, 48, 50)
TAILS = ("next", "long", "imm", "dup", "dupcov")
HEAD = 460


def _rand(n, rng):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _head(n, seed):
    """n random bytes without a repeated 4-byte sequence"""
    while True:
        h = _rand(n, np.random.default_rng(seed))
        if len({h[i:i + 4] for i in range(n - 3)}) == n - 3:
            return h
        seed += 1000


def _block(gap, mlen, tail, seed, size):
    rng = np.random.default_rng(seed)
    h = _head(HEAD, seed)
    b = bytearray(h)
    b += h[10:26]                                   # the first match
    b += _rand(gap, rng)
    b += h[40:40 + mlen]                            # the window's match at lane `gap`
    if tail == "next":                              # a second match at the first lane that can have one: the search behind a
        b += h[120:132]                             # match starts one lane past its end (Q6), so one literal, never none
    elif tail == "long":                            # a match of 44 or more behind a pending run
        b += _rand(4, rng) + h[140:200]
    elif tail == "imm":                             # immediate emission (270 or more) behind a pending run
        b += _rand(4, rng) + h[140:440]
    elif tail == "dup":                             # a second lane of one hash, the first one a literal lane
        g = _rand(4, rng)
        b += g + _rand(6, rng) + g
    elif tail == "dupcov":                          # ... the first one strictly inside the pending match
        b += _rand(3, rng) + h[42:46]
    b += _rand(max(size - len(b), 260), rng)      # (260: the windows behind the tail still have anchor + 192 < L)
    return bytes(b)


_CACHE = []
_EVENTS = set()


def corpus():
    if not _CACHE:
        k = 0
        for gi, gap in enumerate(GAPS):
            for mi, mlen in enumerate(MLENS):
                for t in (TAILS[(gi + mi) % 5], TAILS[(gi + 2 * mi + 2) % 5]):
                    k += 1
                    _CACHE.append(("g%d/m%d/%s" % (gap, mlen, t), _block(gap, mlen, t, 9000 + k, 1400 + 37 * (k % 11))))
        # less than 512 bytes of room from the first window on: the head alone takes 480 of the n + n / 255 + 16
        for i, n in enumerate((0, 800, 850, 900, 940, 960, 975)):
            _CACHE.append(("tight/%d" % n, _block(GAPS[3 * i], 12, TAILS[i % 5], 9500 + i, n)))
        text = bytes(dg.text_bytes(65536, 2800))
        for i in range(12):
            n = (4096, 2048, 1111, 320)[i % 4]
            _CACHE.append(("D-text/%d/%d" % (i, n), text[5000 * i:5000 * i + n]))
        for i, b in enumerate(dg.make_blocks("reptext", 4, 4096, seed=28)):
            _CACHE.append(("D-reptext/%d" % i, bytes(b)))
        for name, b in _CACHE:
            assert 320 <= len(b) <= 4096, (name, len(b))
            assert ew.compress_run_masks(b, events=_EVENTS, check=False) is not None, name
        missing = [e for e in ew.EVENTS if e not in _EVENTS]
        assert not missing, "no block of the corpus shows: %s" % ", ".join(missing)
    return list(_CACHE)


def events():
    corpus()
    return set(_EVENTS)
