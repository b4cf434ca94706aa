"""batch_compress_hc through every round of launch_hc_chunked: more than two chunks of blocks, so that both halves of
the result area (levels 10-12: of the link area too) are reused after the event wait and, on the greedy path, the
memset; with the links in LDS (small blocks, 8192 per chunk) and in HBM (a large declared max_in_len, ~31 per chunk).
Bytes and statuses against the oracle.  The batches are described in tests/hcrounds.py.  Run on the GPU box: pytest -m gpu."""
import pytest
import torch

import gpu_harness as gh
import hcrounds
from test_gpu_packed_layout import _plain_blocks
from test_gpu_parity import _cmp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def small():
    return hcrounds.small_blocks()


@pytest.mark.parametrize("level", [2, 4, 9, 11])
def test_small_blocks_five_rounds(zl, oracle, gpu, small, level):
    """16 900 blocks, links in LDS: rounds of 4096, the fifth reuses the first half a second time; level 2 needs a
    second trip of zlz4_launch_hc_mid over its re-zeroed tables"""
    n, max_in = len(small), max(len(b) for b in small)
    assert (n, max_in) == (hcrounds.SMALL_N, hcrounds.SMALL_BIG)
    chunk = hcrounds.chunk_of(zl, n, max_in)
    assert n > 2 * chunk
    assert zl.batch_compress_hc_workspace(n, max_in) // hcrounds.MID_TABLES < n
    got = gh.compress_hc(zl, small, gpu, level)
    want = [oracle.compress_hc(b, level) for b in small]
    _cmp(["blk%d/round%d/n%d" % (i, i // (chunk // 2), len(b)) for i, b in enumerate(small)], got, want)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("level", [4, 9, 12])
def test_hbm_links_alternating_halves(zl, oracle, gpu, level):
    """small blocks under a 16 MiB + 1 bound: k_hc_build_links<u32>, k_hc_seg_search<.., false> (levels 4, 9),
    k_hc_search<u32, u64> and the wide parse (level 12) over alternating halves of the 6 GiB workspace"""
    max_in = hcrounds.HBM_MAX_IN
    chunk = hcrounds.chunk_of(zl, 1000, max_in)
    assert 2 <= chunk <= 32
    n = 2 * chunk + 7
    items = _plain_blocks(n, 60 + level, 70002) + [b for b in hcrounds.periodic_items(level) if len(b) <= 65536]
    assert len(items) > n > 2 * chunk and hcrounds.chunk_of(zl, len(items), max_in) == chunk
    assert max(len(b) for b in items) > 65536
    got = gh.compress_hc(zl, items, gpu, level, max_in=max_in)
    want = [oracle.compress_hc(b, level) for b in items]
    _cmp(["blk%d/round%d/n%d" % (i, i // (chunk // 2), len(b)) for i, b in enumerate(items)], got, want)
    del got
    torch.cuda.empty_cache()
