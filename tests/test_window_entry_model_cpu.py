"""tools/emulate_window.py, the lane-level model of k_compress_fast, with the kernel's entry rule -- the window path only
runs behind a match, with the anchor's put pending as its lane 0; the block's first search takes the generic path --
against the oracle, byte for byte, on the block-start corpus (tests/blockstartgen.py)."""
import os
import sys

import pytest

import blockstartgen as bg

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import emulate_window as ew   # noqa: E402


@pytest.fixture(scope="module")
def want(oracle):
    return [oracle.compress_default(b) for _, b in bg.corpus()]


def test_the_corpus_holds_what_it_is_for(want):
    """the oracle's parse shows the planted first matches (position, length, offset), and the Q1 blocks never match
    against position 0"""
    fm = {name: bg.first_match(w) for (name, _), w in zip(bg.corpus(), want)}
    assert fm["run@0/4096"][::2] == (2, 1) and fm["run@1/4096"][::2] == (2, 1)
    for p in (62, 63, 64):
        assert fm["first@%d/4096" % p] == (p, 9, p - 10)
    assert fm["nomatch64/4096"][0] == 64 and fm["nomatch128/4096"][0] == 128 and fm["nomatch300/4096"][0] >= 300
    for r in (5, 40, 70):
        assert fm["q1first@%d/4096" % r] == (r + 20, 4, 20)           # against r, never against 0
    assert fm["q1after@5/4096"][::2] == (2, 1)
    for r in (40, 70):
        assert fm["q1after@%d/4096" % r] == (24, 8, 12)
    for (name, b), w in zip(bg.corpus(), want):
        if name.startswith("q1") and len(b) >= 204:
            f = bg.first_match(w)
            assert f is not None and f[2] != f[0]                     # offset == position would point at position 0
    assert fm["long44/4096"][1] >= 44 and fm["long50/4096"][1] >= 44
    assert fm["long280/4096"][1] >= 270 and fm["long320/4096"][1] >= 270
    for ml in (44, 50, 280, 320):
        assert fm["long%d_second/4096" % ml] == (20, 5, 14)
    assert fm["first@62/13"] is None and fm["first@62/204"] is not None


def test_model_matches_the_oracle(want):
    bad = []
    for (name, b), w in zip(bg.corpus(), want):
        g = ew.compress(b)
        if g != w:
            bad.append("%s: %d bytes, oracle %d" % (name, len(g), len(w)))
    assert not bad, "%d mismatches: %s" % (len(bad), "; ".join(bad[:8]))


def test_a_block_without_a_match_is_literals():
    """300 bytes without a repeated 4-byte sequence: the first search runs to the end of the block on the generic path
    (has_ins stays false, so no window starts) and the block is one literal run"""
    b = bytes(bg._head(300, 99))
    assert ew.compress(b) == bytes([0xF0, 255, 300 - 15 - 255]) + b
