"""Real blocks on both sides of 2^24 bytes (tests/bigblocks.py), byte for byte against the oracle.

Above 2^24 bytes of max_in_len k_compress_fast runs with a plain 32-bit table (no tag beside the position) and
k_hc_seg_search drops its counted runs (24-bit fields); at exactly 2^24 both still run the packed forms, with positions
and run ends at the top of the field.  Every compress call is therefore made twice: the blocks of 2^24 bytes with
max_in_len = 2^24, the longer ones with their own maximum.  Levels 10-12 are not run at this size (their wide parse is
one lane per block).  Run on the GPU box: pytest -m gpu."""
import numpy as np
import pytest

import bigblocks as bb
import gpu_harness as gh
import streamgen as sg
from test_gpu_parity import _cmp

pytestmark = pytest.mark.gpu

CODECS = {"fast1": lambda o, b: o.compress_fast(b, 1), "fast7": lambda o, b: o.compress_fast(b, 7),
          "hc4": lambda o, b: o.compress_hc(b, 4), "hc9": lambda o, b: o.compress_hc(b, 9)}


class Big:
    """the five blocks and, computed once on demand, the oracle's streams of them"""

    def __init__(self, oracle):
        self.oracle, self.blocks, self._streams = oracle, bb.blocks(), {}

    def stream(self, name, codec):
        if (name, codec) not in self._streams:
            self._streams[(name, codec)] = CODECS[codec](self.oracle, self.blocks[name])
        return self._streams[(name, codec)]

    def calls(self):
        """-> [(names, max_in_len)]: each side of 2^24 meets its own build"""
        wide = [n for n in self.blocks if n not in bb.AT_T]
        return [(list(bb.AT_T), bb.T), (wide, max(len(self.blocks[n]) for n in wide))]


@pytest.fixture(scope="module")
def big(oracle):
    return Big(oracle)


@pytest.mark.parametrize("accel", [1, 7])
def test_compress_fast(zl, gpu, big, accel):
    for names, max_in in big.calls():
        assert max(len(big.blocks[n]) for n in names) == max_in
        got = gh.compress_fast(zl, [big.blocks[n] for n in names], gpu, accel=accel, max_in=max_in)
        _cmp(names, got, [big.stream(n, "fast%d" % accel) for n in names])


@pytest.mark.parametrize("level", [4, 9])
def test_compress_hc(zl, gpu, big, level):
    for names, max_in in big.calls():
        got = gh.compress_hc(zl, [big.blocks[n] for n in names], gpu, level, max_in=max_in)
        _cmp(names, got, [big.stream(n, "hc%d" % level) for n in names])
    import torch
    torch.cuda.empty_cache()


def test_decompress_and_size_query(zl, oracle, gpu, big):
    names, comp, sizes = [], [], []
    for codec in ("fast1", "hc9"):
        for n, b in big.blocks.items():
            names.append("%s/%s" % (n, codec)); comp.append(big.stream(n, codec)); sizes.append(len(b))
    got = gh.decompress(zl, comp, sizes, gpu)
    _cmp(names, got, list(big.blocks.values()) * 2)
    short = gh.decompress(zl, comp, [n - 1 for n in sizes], gpu)
    want = [oracle.decompress_safe(c, n - 1) for c, n in zip(comp, sizes)]
    assert all(isinstance(w, int) for w in want)
    _cmp(names, short, want)
    for codec in ("fast1", "hc9"):
        assert zl.decompressedSize(big.stream("T+70001", codec)) == bb.T + 70001


def test_seeded_blocks(zl, gpu, tmp_path):
    """a seed at or above 2^24 (the plain 32-bit table must hold it) and one at the top of the tagged range: result,
    bytes and output table equal the restatement's"""
    cref = sg.ref(tmp_path)
    for name, (b, table) in bb.planted_blocks().items():
        caps = [len(b) + len(b) // 255 + 16]
        wr, wo, wt = cref.batch(table[None, :], None, [b], caps, 1)
        gr, go, gt = sg.run_continue(zl, [b], caps, table[None, :], None, gpu, accel=1, max_in=len(b))
        assert gr[0] == wr[0] and go[0] == wo[0], "%s: GPU %d vs %d" % (name, gr[0], wr[0])
        assert np.array_equal(gt[0], wt[0]), "%s: the output table differs" % name


def test_host_calls(zl, gpu, big):
    text = big.blocks["T+70001"]
    assert zl.compressDefault(text) == big.stream("T+70001", "fast1")
    assert zl.compressHC(text, 4) == big.stream("T+70001", "hc4")
    assert zl.decompressSafe(big.stream("T+70001", "hc4"), len(text)) == text
