"""The level-2 corpus (tests/midgen.py) through k_hc_mid_serial on the HIP path, status for status and byte for byte
against the oracle.  tests/test_mid_corpus_cpu.py shows on the oracle that each case's parse turns on one comparison of
the kernel's loop -- the patched prefetch, the clamp at mflimit, `ml2 > match_len`, the index a moved match enters, the
entries a match leaves, 65535 / 65536, the step from the anchor -- and, with a model of that loop, that a kernel with
one of these operators changed gives other bytes on a case here.

Twins are neighbours in every batch: the two blocks of one wavefront take different branches.  Every output slot
stands between guard bands (gpu_harness).  Run on the GPU box: pytest -m gpu.
"""
import pytest
import torch

import gpu_harness as gh
import hcrounds
import midgen as mg
import test_gpu_frame_batch as tfb
from test_gpu_parity import _cmp

pytestmark = pytest.mark.gpu

_want = {}


def _oracle(oracle, sel):
    """the oracle's level-2 stream of every selected case, computed once"""
    for _, name, b, _ in sel:
        if name not in _want:
            _want[name] = oracle.compress_hc(b, 2)
    return [_want[c[1]] for c in sel]


def _pairs():
    """one accept / refuse pair per family (the reach pair is the 8-byte-hash copy at 65535 / 65536)"""
    by = {c[1]: c for c in mg.cases()}
    out = []
    for fam in mg.FAMILIES:
        c = by["reach/h8/d65535"] if fam == "reach" else \
            next(c for c in mg.cases() if c[0] == fam and c[3]["accept"] and not by[c[3]["twin"]][3]["accept"])
        out += [c, by[c[3]["twin"]]]
    return out


@pytest.mark.parametrize("layout", [None, gh.Packed(seed=29, fill="cont")], ids=["aligned", "packed"])
@pytest.mark.parametrize("max_in", [None, 65537, 1 << 24], ids=["natural", "65537", "16mib"])
def test_layouts_and_bounds(zl, oracle, gpu, max_in, layout):
    """the whole corpus under its natural bound and under 2^24, what fits under 65537; aligned, and packed back to back
    with gaps that continue the block before them"""
    sel = [c for c in mg.cases() if max_in is None or len(c[2]) <= max_in]
    assert {c[0] for c in sel} == set(mg.FAMILIES) and (max_in == 65537 or len(sel) == len(mg.cases()))
    assert max_in != 65537 or sel == mg.small()
    got = gh.compress_hc(zl, [c[2] for c in sel], gpu, 2, layout=layout, max_in=max_in)
    _cmp([c[1] for c in sel], got, _oracle(oracle, sel))
    del got
    torch.cuda.empty_cache()


def test_second_trip_over_rezeroed_tables(zl, oracle, gpu):
    """batch_compress_hc takes no workspace smaller than it reports, so: the smallest batch that zlz4_launch_hc_mid needs
    two trips for.  The second trip's blocks are the first trip's in reverse order -- block i of trip two gets the tables
    block i of trip one used, and a table entry left from trip one would meet the input that finds it"""
    small = mg.small()
    max_in = max(len(c[2]) for c in small)
    per_trip = zl.batch_compress_hc_workspace(1 << 15, max_in) // hcrounds.MID_TABLES
    n = 2 * per_trip
    assert zl.batch_compress_hc_workspace(n, max_in) // hcrounds.MID_TABLES == per_trip and len(small) < per_trip <= 16384
    first = (small * (per_trip // len(small) + 1))[:per_trip]
    sel = first + first[::-1]
    got = gh.compress_hc(zl, [c[2] for c in sel], gpu, 2, max_in=max_in)
    _cmp(["%s/blk%d" % (c[1], i) for i, c in enumerate(sel)], got, _oracle(oracle, sel))
    del got
    torch.cuda.empty_cache()


def test_capacities(zl, oracle, gpu):
    """the small cases at capacity = the oracle's size and one byte less: the same OutputTooSmall decisions, nothing
    written behind the capacity"""
    sel, caps = [], []
    for c in mg.small():
        full = len(_oracle(oracle, [c])[0])
        for cap in (full, full - 1):
            sel.append(c)
            caps.append(cap)
    want = [oracle.compress_hc_expected(c[2], 2, cap) for c, cap in zip(sel, caps)]
    assert sum(isinstance(w, int) for w in want) >= len(sel) // 2 and sum(not isinstance(w, int) for w in want) >= len(sel) // 2
    got = gh.compress_hc(zl, [c[2] for c in sel], gpu, 2, caps=caps)
    _cmp(["%s/cap%d" % (c[1], cap) for c, cap in zip(sel, caps)], got, want)


def test_single_block_calls(zl, oracle):
    """compressHC(b, 2) on one pair per family; compressHC(b, 1) as well (a level below 2 is the default level 9 in this
    API as in the reference, so that call checks the level table, not lz4mid)"""
    for fam, name, b, m in _pairs():
        assert zl.compressHC(b, 2) == _oracle(oracle, [(fam, name, b, m)])[0], name
        assert zl.compressHC(b, 1) == oracle.compress_hc(b, 1), name


def test_frames_at_level_2(zl, oracle, gpu):
    """the batch frame compressor with compression_level = 2, every small case as a one-block frame"""
    small = mg.small()
    items = [c[2] for c in small]
    prefs, oprefs = tfb._prefs(zl.Prefs, compression_level=2), tfb._prefs(oracle.Prefs, compression_level=2)
    res, frames = tfb._compress(zl, gpu, items, prefs)
    bad = []
    for c, r, f in zip(small, res, frames):
        want = oracle.compress_frame(c[2], oprefs)
        if isinstance(want, int) or r != len(want) or f != want:
            bad.append((c[1], r, want if isinstance(want, int) else len(want)))
    assert not bad, (len(bad), bad[:6])
    stream = _oracle(oracle, small)
    inside = sum(s in f for s, f in zip(stream, frames))     # the block payload is the level-2 stream, unless stored
    assert inside >= len(small) * 3 // 4
