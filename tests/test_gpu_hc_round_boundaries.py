"""The round boundaries of the three HC pipelines at the smallest shapes that have them.  With at most 8192 small blocks
a chunk is the whole call and a round half of it, so a handful of blocks reaches every ordering rule of HcRounds
(zlz4_compress_hc.hip):

  1 block        one round, no side stream
  2 blocks       two rounds of one block: both halves, the fork and the join
  3 blocks       three rounds: half 0 is reused after the event wait and the memset
  5 and 7        an uneven last round

through the plain call (levels 4, 9: K1 / K2s / K3; level 11: K1 ahead of the parse, link halves) against the oracle, the
dictionary call against tests/hc_dict_ref.c, and linked frames against the model of tests/test_gpu_linked_frame_hc.py;
and with the links in HBM under hcrounds.HBM_MAX_IN, where a chunk holds about 31 blocks, around one and two rounds.
hcrounds.boundary_blocks fills the blocks so that a stale half shows.  Statuses and bytes equal the reference's."""
import pytest
import torch

import datagen as dg
import gpu_harness as gh
import hcdictcgen as hg
import hcrounds
import test_gpu_linked_frame_hc as tlf
from test_gpu_parity import _cmp

pytestmark = pytest.mark.gpu

COUNTS = (1, 2, 3, 5, 7)


@pytest.fixture(scope="module")
def cref(tmp_path_factory):
    return hg.ref(tmp_path_factory.mktemp("hc_dict_ref"))


def _names(items, sub):
    return ["blk%d/round%d/n%d" % (i, i // sub, len(b)) for i, b in enumerate(items)]


@pytest.mark.parametrize("level", [4, 9, 11])
@pytest.mark.parametrize("n", COUNTS)
def test_plain_call(zl, oracle, gpu, n, level):
    items = hcrounds.boundary_blocks(n, max(n // 2, 1), 4100 + n)
    max_in = max(len(b) for b in items)
    assert hcrounds.chunk_of(zl, n, max_in) == n
    got = gh.compress_hc(zl, items, gpu, level)
    _cmp(_names(items, max(n // 2, 1)), got, [oracle.compress_hc(b, level) for b in items])


@pytest.mark.parametrize("level", [4, 9])
@pytest.mark.parametrize("n", COUNTS)
def test_dictionary_call(zl, cref, gpu, n, level):
    """every record with a dictionary of its own that ends in the record's first half: matches into the dictionary in the
    text rounds and in the random ones"""
    recs = hcrounds.boundary_blocks(n, max(n // 2, 1), 4200 + n)
    dicts = [bytes(dg.reptext_bytes(300, 4300 + i)) + r[:len(r) // 2] + b"xyz" for i, r in enumerate(recs)]
    w = zl.batch_compress_hc_using_dict_workspace
    max_in, max_dict = max(len(r) for r in recs), max(len(d) for d in dicts)
    assert max_in + max_dict <= 65536                 # LDS links, and the chunk is the call:
    assert w(n, max_in, max_dict) - (20 * n + 15) // 16 * 16 == n * (w(1, max_in, max_dict) - 32)
    got, want = hg.run_batch(zl, cref, recs, [hg.bound(len(r)) for r in recs], dicts, list(range(n)), gpu, level)
    hg.check(got, want, "n=%d level=%d" % (n, level))


@pytest.mark.parametrize("level", [4, 9])
@pytest.mark.parametrize("n", COUNTS)
def test_linked_frames(zl, cref, gpu, n, level):
    """n table entries (max_blocks = n): one-block frames, an empty frame (no entry), and from three entries on a
    two-block frame in the last two: its second block, in the round that reuses half 0, repeats the 64 KiB before it"""
    items = hcrounds.boundary_blocks(n, max(n // 2, 1), 4400 + n, empty=False)
    if n >= 3:
        text = bytes(dg.text_bytes(65536, 4500 + n))
        items[n - 2:] = [text + text[1000:1000 + len(items[n - 1])]]
    items.insert(1, b"")
    p = tlf._prefs(zl.Prefs, compression_level=level)
    rc, res, frames, _ = tlf._compress_ex(zl, gpu, items, p, zl.lz4f.BATCH_LINK_BLOCKS, max_blocks=n)
    assert rc == 0
    want = [tlf.lh.compress_frame_linked_hc(b, level, None, lambda blk, d, lv: cref.compress(blk, d, lv)[1]) for b in items]
    assert sum(len(tlf.lh.blocks_of(f)) for f in want) == n
    bad = [(k, len(b), res[k], len(w)) for k, (b, w) in enumerate(zip(items, want)) if res[k] != len(w) or frames[k] != w]
    assert not bad, bad


@pytest.mark.parametrize("level", [4, 12])
@pytest.mark.parametrize("which", ["half", "half+1", "two halves+1"])
def test_plain_call_hbm_links(zl, oracle, gpu, which, level):
    """small blocks under the 16 MiB + 1 bound: k_hc_build_links<u32> and k_hc_seg_search<.., false> (level 4) or
    k_hc_search<u32, u64> and the wide parse (level 12), around one and two rounds of the ~31-block chunk"""
    max_in = hcrounds.HBM_MAX_IN
    cap = hcrounds.chunk_of(zl, 1000, max_in)
    assert 2 <= cap <= 32
    n = {"half": cap // 2, "half+1": cap // 2 + 1, "two halves+1": 2 * (cap // 2) + 1}[which]
    sub = hcrounds.round_blocks(n, hcrounds.chunk_of(zl, n, max_in))
    items = hcrounds.boundary_blocks(n, sub, 4600 + n)
    got = gh.compress_hc(zl, items, gpu, level, max_in=max_in)
    _cmp(_names(items, sub), got, [oracle.compress_hc(b, level) for b in items])
    del got
    torch.cuda.empty_cache()
