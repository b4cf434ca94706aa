"""The inputs of tests/test_gpu_blocks_16mib.py and tests/test_gpu_hc_rounds.py do what those tests need them to do:
checked here on the oracle's streams and the library's workspace arithmetic, without a GPU.

  * The oracle's streams of the T+70001 block hold matches whose source lies at or above 2^24 (a table entry or link
    that does not fit 24 bits) and matches that reach from above 2^24 to below it; those of T and T+1 hold none.
  * The seeds of the two planted blocks change the streaming compressor's output.
  * The two HC batches hold more than two chunks of blocks, i.e. at least five rounds.
"""
import ctypes as C

import numpy as np
import pytest

import bigblocks as bb
import hcrounds
import streamgen as sg

CODECS = {"fast": lambda o, b: o.compress_default(b), "hc4": lambda o, b: o.compress_hc(b, 4),
          "hc9": lambda o, b: o.compress_hc(b, 9)}


@pytest.fixture(scope="module")
def blocks():
    return bb.blocks()


@pytest.fixture(scope="module")
def streams(blocks, oracle):
    return {(name, codec): f(oracle, blocks[name]) for name in ("T", "T+1", "T+70001") for codec, f in CODECS.items()}


def test_block_sizes_and_tails(blocks):
    assert [len(b) for b in blocks.values()] == [bb.T, bb.T + 1, bb.T + 70001, bb.T, bb.T + 12]
    for name in ("tailT", "tailT+12"):
        b = blocks[name]
        tail = b[-bb.TAIL:]
        assert tail[256:] == tail[:-256] and len(set(tail[:256])) > 100          # period 256, to the last byte
        assert b[-bb.TAIL - 256:-bb.TAIL] != tail[:256]                            # and it starts where the text ends
    assert len(blocks["tailT"]) - 5 == 0xFFFFFB


@pytest.mark.parametrize("codec", list(CODECS))
def test_long_block_has_matches_at_and_across_2_pow_24(streams, codec):
    size, src_high, crossing = bb.walk(streams[("T+70001", codec)])
    print("%s: %d matches with a source >= 2^24, %d from above to below" % (codec, src_high, crossing))
    assert size == bb.T + 70001
    assert src_high >= 1000
    assert crossing >= 100


@pytest.mark.parametrize("codec", list(CODECS))
@pytest.mark.parametrize("name", ["T", "T+1"])
def test_blocks_at_2_pow_24_have_none(streams, blocks, name, codec):
    size, src_high, crossing = bb.walk(streams[(name, codec)])
    assert size == len(blocks[name])
    assert (src_high, crossing) == (0, 0)


def test_streams_decode_back(streams, blocks, oracle):
    for (name, codec), s in streams.items():
        assert oracle.decompress_safe(s, len(blocks[name])) == blocks[name], (name, codec)


def test_planted_seeds_matter(tmp_path):
    cref = sg.ref(tmp_path)
    for name, (b, table) in bb.planted_blocks().items():
        v = int(table.max())
        assert (v >= bb.T) == (name == "above") and v < len(b) - 12
        cap = len(b) + len(b) // 255 + 16
        with_seed = cref.cont(table, b, 1, cap)
        without = cref.cont(np.zeros_like(table), b, 1, cap)
        assert with_seed[0] > 0 and without[0] > 0
        assert with_seed[1] != without[1], "the seed of %r did not change the output" % name


def test_hc_round_conditions(zl):
    """more than two chunks of blocks = at least five rounds of half a chunk; pure arithmetic in the library"""
    small = hcrounds.chunk_of(zl, hcrounds.SMALL_N, hcrounds.SMALL_BIG)
    assert hcrounds.SMALL_N > 2 * small
    assert -(-hcrounds.SMALL_N // (small // 2)) >= 5
    # level 2 fits workspace / (its two tables) blocks into a trip: the batch needs a second one
    mid = zl.lib().zlz4_hc_mid_workspace_bytes
    mid.restype, mid.argtypes = C.c_size_t, [C.c_uint32]
    assert mid(1) == hcrounds.MID_TABLES
    assert zl.batch_compress_hc_workspace(hcrounds.SMALL_N, hcrounds.SMALL_BIG) // hcrounds.MID_TABLES < hcrounds.SMALL_N
    for max_in in (hcrounds.HBM_MAX_IN, 32 << 20):
        chunk = hcrounds.chunk_of(zl, 1000, max_in)
        assert 2 <= chunk <= 32
        n = 2 * chunk + 7
        assert hcrounds.chunk_of(zl, n, max_in) == chunk and n > 2 * chunk
        assert zl.batch_compress_hc_workspace(n, max_in) <= 6 << 30
