"""zlz4_batch_compress_hc_using_dict / zlz4_compress_hc_using_dict on the GPU.  Every comparison
is with tests/hc_dict_ref.c (the C restatement), never with the code under test; every slot has guard bands, the input
and dictionary arenas must be unchanged, a failed slot is unspecified except that InvalidState writes nothing
(tests/hcdictcgen.py: run_batch).  Run on the GPU box: pytest -m gpu."""
import numpy as np
import pytest
import torch

import datagen as dg
import gpu_harness as gh
import hcdictcgen as hg

pytestmark = pytest.mark.gpu

BASE = 200000                                         # a pair (D, n) is stream[BASE - D: BASE], stream[BASE: BASE + n]
DICT_LENS = (0, 1, 3, 4, 5, 100, 4096, 65535, 65536, 65537, 200000)
REC_LENS = (0, 1, 12, 13, 14, 37, 4096, 61440, 65536, 70001)


@pytest.fixture(scope="module")
def cref(tmp_path_factory):
    return hg.ref(tmp_path_factory.mktemp("hcdictcref"))


@pytest.fixture(scope="module")
def streams():
    """one stream per generator: the record continues the dictionary's text, so it has matches there"""
    return [bytes(g(BASE + 70001, 300 + k)) for k, g in enumerate((dg.text_bytes, dg.mixed_bytes))]


def _pair(streams, k, D, n):
    s = streams[k % len(streams)]
    return s[BASE - D:BASE], s[BASE:BASE + n]


def _tail(D):
    return min(D, 65536)


def _run(zl, cref, gpu, pairs, level, caps=None, tag="", **kw):
    """pairs: [(dictionary, record)], every pair with its own dictionary"""
    recs = [r for _, r in pairs]
    caps = [hg.bound(len(r)) for r in recs] if caps is None else caps
    got, want = hg.run_batch(zl, cref, recs, caps, [d for d, _ in pairs], list(range(len(pairs))), gpu, level, **kw)
    hg.check(got, want, tag)
    return got


def _launches(pairs):
    """cut a list of (D, n) into launches with exact bounds: first-fit into launches whose D_max + n_max stays within
    65536 (LDS links), everything that cannot be in one into a last launch (HBM links)"""
    lds, hbm = [], []
    for D, n in pairs:
        if _tail(D) + n > 65536:
            hbm.append((D, n))
            continue
        for L in lds:
            if max(_tail(D), max(_tail(d) for d, _ in L)) + max(n, max(m for _, m in L)) <= 65536:
                L.append((D, n))
                break
        else:
            lds.append([(D, n)])
    return lds, hbm


@pytest.mark.parametrize("level", [3, 6, 8, 9])
def test_length_grid_both_link_widths(zl, cref, gpu, streams, level):
    lds, hbm = _launches([(D, n) for D in DICT_LENS for n in REC_LENS])
    assert len(lds) >= 2 and len(hbm) >= 20
    assert sum(len(L) for L in lds) + len(hbm) == len(DICT_LENS) * len(REC_LENS)
    for k, L in enumerate(lds + [hbm]):
        width = max(_tail(D) for D, _ in L) + max(n for _, n in L)
        assert (width <= 65536) == (k < len(lds)), (k, width)
        _run(zl, cref, gpu, [_pair(streams, i + level, D, n) for i, (D, n) in enumerate(L)], level,
             tag="launch %d %s" % (k, L))


@pytest.mark.parametrize("D,n,lds", [(61440, 4096, True), (61441, 4096, False), (65536, 1, False), (65535, 1, True)])
def test_the_width_boundary(zl, cref, gpu, streams, D, n, lds):
    assert (D + n <= 65536) == lds
    for level in (3, 9):
        pairs = [_pair(streams, k, D, n) for k in range(3)]
        got = _run(zl, cref, gpu, pairs, level, max_in=n, max_dict=D)
        assert all(r > 0 for r, _ in got)


CAP_PAIRS = ((65536, 4096), (70000, 1000), (300, 13), (4096, 65536), (0, 4096), (100, 37), (61440, 4096), (5, 14))


@pytest.mark.parametrize("level", [3, 9])
def test_capacities(zl, cref, gpu, streams, level):
    pairs, caps = [], []
    for k, (D, n) in enumerate(CAP_PAIRS):
        d, r = _pair(streams, k, D, n)
        s = cref.compress(r, d, level)[0]
        assert 0 < s <= hg.bound(n)
        for cap in (s, s - 1, 0, hg.bound(n), s + 1, s // 2):
            pairs.append((d, r))
            caps.append(cap)
    got = _run(zl, cref, gpu, pairs, level, caps=caps)
    res = [r for r, _ in got]
    for k in range(len(CAP_PAIRS)):
        s, below, zero, bnd, above, half = res[6 * k:6 * k + 6]
        assert s > 0 and bnd == s and above == s and below == zero == half == hg.OUTPUT_TOO_SMALL, CAP_PAIRS[k]


@pytest.mark.parametrize("level", [3, 4, 8, 9])
def test_crafted_records(zl, cref, gpu, level):
    cases = hg.crafted()
    got = _run(zl, cref, gpu, [(d, r) for _, d, r in cases], level)
    by = {name: hg.sequences(out) for (name, _, _), (_, out) in zip(cases, got)}
    assert by["equals_tail_4k"] == [(0, 0, 4091, 4096)]
    assert by["period_7_from_dict"][0] == (0, 0, 3000, 7)
    assert by["period_1_from_dict_64k"][0] == (0, 0, 5000, 1) and by["period_1_from_dict_9"][0] == (0, 0, 300, 1)
    assert by["offset_65535_only"] == [(19, 19, 60, 65535)] and by["offset_65536_none"] == []
    assert by["only_at_v_pos_0"] == [] and by["at_v_pos_1"] == [(30, 30, 4, 130)]
    assert by["match_ends_at_dict_end"][0] == (0, 0, 40, 40) and by["match_spans_dict_end"][0] == (0, 0, 80, 40)
    assert by["thirteen_bytes"] == [(0, 0, 8, 250)]
    # four attempts are used up by record candidates before the long dictionary candidate (hcdictcgen.traced)
    assert {op: ml for op, _, ml, _ in by["attempt_budget"]}[28] == (4 if level == 3 else 23)
    # the pattern step's reverse count crosses into the tail and places the match there
    assert by["pattern_into_tail"][:2] == [(0, 0, 300, 1), (301, 1, 350, 351) if level == 9 else
                                           (301, 1, (1 << (level - 1)) + 1, (1 << (level - 1)) + 2)]


def test_shared_dictionary_both_widths(zl, cref, gpu):
    s = bytes(dg.text_bytes(65536 + 48 * 4096, 21))
    recs = [s[65536 + i * 4096:65536 + (i + 1) * 4096] for i in range(48)]
    caps = [hg.bound(4096)] * 48
    plain = sum(r for r, _ in gh.compress_hc(zl, recs, gpu, 9))
    for dl in (65536, 61440):
        d = s[65536 - dl:65536]
        assert zl.batch_compress_hc_using_dict_workspace(48, 4096, dl) > 0 and (dl + 4096 <= 65536) == (dl == 61440)
        got, want = hg.run_batch(zl, cref, recs, caps, [d], [0] * 48, gpu, 9)
        hg.check(got, want, "shared %d" % dl)
        assert sum(r for r, _ in got) < plain


@pytest.mark.parametrize("fill", ["zero", "cont"])
def test_per_block_dictionaries_packed(zl, cref, gpu, streams, fill):
    rng = np.random.default_rng(12)
    dls = [int(x) for x in rng.choice([0, 1, 4, 7, 100, 999, 4096, 20000], 40)]
    ns = [int(x) for x in rng.choice([0, 5, 12, 13, 100, 1001, 4096, 9000], 40)]
    pairs = [_pair(streams, k, D, n) for k, (D, n) in enumerate(zip(dls, ns))]
    _run(zl, cref, gpu, pairs, 6, layout=gh.Packed(seed=3, fill=fill))


@pytest.mark.parametrize("size", [1000, 4096, 40000])
def test_previous_record_as_dictionary(zl, cref, gpu, size):
    s = bytes(dg.text_bytes(size * 12, 50 + size))
    recs = [s[i * size:(i + 1) * size] for i in range(12)]
    _, offs, _ = gh._pack(recs)
    in_input = [(0, 0)] + [(int(offs[k - 1]), size) for k in range(1, 12)]
    got, want = hg.run_batch(zl, cref, recs, [hg.bound(size)] * 12, None, None, gpu, 9, in_input=in_input)
    hg.check(got, want)
    alone = gh.compress_hc(zl, recs, gpu, 9)
    assert sum(r for r, _ in got[1:]) < sum(r for r, _ in alone[1:])


def test_loose_and_violated_bounds(zl, cref, gpu, streams):
    shapes = [(100, 1000), (4096, 4096), (0, 13), (20000, 300), (4096, 5000), (30000, 100), (100, 4000), (7, 4096)]
    pairs = [_pair(streams, k, D, n) for k, (D, n) in enumerate(shapes)]
    exact = _run(zl, cref, gpu, pairs, 9)
    for max_in, max_dict in ((6000, 40000), (70000, 30000), (5000, 65536), (5000, 1 << 31)):
        assert _run(zl, cref, gpu, pairs, 9, max_in=max_in, max_dict=max_dict) == exact
    got = _run(zl, cref, gpu, pairs, 9, max_in=4096, max_dict=20000)
    res = [r for r, _ in got]
    assert res[4] == res[5] == hg.INVALID_STATE
    assert [g for k, g in enumerate(got) if k not in (4, 5)] == [g for k, g in enumerate(exact) if k not in (4, 5)]


def _chunk_of(zl, n, max_in, max_dict):
    """blocks per chunk: the workspace is 20 bytes of descriptors per block (to 16) and a whole number of per-block shares"""
    w = zl.batch_compress_hc_using_dict_workspace
    return (w(n, max_in, max_dict) - (20 * n + 15) // 16 * 16) // (w(1, max_in, max_dict) - 32)


@pytest.mark.parametrize("level", [4, 9])
def test_rounds_lds_links(zl, cref, gpu, level):
    n = 2 * 8192 + 5
    rng = np.random.default_rng(77)
    lens = rng.integers(64, 201, n)
    s = bytes(dg.text_bytes(1 << 20, 78))
    starts = rng.integers(100, (1 << 20) - 300, n)
    pairs = [(s[int(a) - 100:int(a)], s[int(a):int(a) + int(k)]) for a, k in zip(starts, lens)]
    assert _chunk_of(zl, n, 200, 100) == 8192 and n > 2 * 8192
    _run(zl, cref, gpu, pairs, level)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("level", [4, 9])
def test_rounds_hbm_links(zl, cref, gpu, streams, level):
    max_in = (1 << 24) + 1                            # declared, not reached: the 6 GiB cap leaves ~29 blocks per chunk
    chunk = _chunk_of(zl, 1000, max_in, 65536)
    assert 2 <= chunk <= 32
    n = 2 * chunk + 7
    rng = np.random.default_rng(5)
    shapes = [(int(rng.choice([0, 100, 4096, 65536])), int(rng.choice([13, 300, 4096, 70001]))) for _ in range(n)]
    assert _chunk_of(zl, n, max_in, 65536) == chunk
    _run(zl, cref, gpu, [_pair(streams, k, D, m) for k, (D, m) in enumerate(shapes)], level, max_in=max_in, max_dict=65536)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("level", [3, 4, 5, 6, 7, 8, 9])
def test_empty_dictionary_equals_compress_hc(zl, cref, oracle, gpu, streams, level):
    recs = [_pair(streams, k, 0, n)[1] for k, n in enumerate((13, 100, 4096, 20000, 65536, 70001))]
    got = _run(zl, cref, gpu, [(b"", r) for r in recs], level)
    assert got == gh.compress_hc(zl, recs, gpu, level)
    for (r, out), rec in zip(got, recs):
        assert out == oracle.compress_hc(rec, level)


def test_round_trip_on_the_device(zl, cref, gpu, streams):
    shapes = [(65536, 4096), (200000, 70001), (100, 13), (4096, 65536), (5, 1000), (0, 4096), (61440, 4096), (1, 12)]
    pairs = [_pair(streams, k, D, n) for k, (D, n) in enumerate(shapes)]
    got = _run(zl, cref, gpu, pairs, 9)
    back = zl.decompressBlocks([out for _, out in got], [d for d, _ in pairs])
    assert [bytes(b) for b in back] == [r for _, r in pairs]


def test_single_call(zl, cref, gpu, streams):
    for k, (D, n) in enumerate(((65536, 4096), (300, 13), (0, 1000), (100, 12), (70000, 70001))):
        d, r = _pair(streams, k, D, n)
        for level in (3, 9, 1, 0):
            want = cref.compress(r, d, level)
            assert zl.compressHCUsingDict(r, d, level) == want[1]
            with pytest.raises(zl.Lz4Error) as e:
                zl.compressHCUsingDict(r, d, level, dst_cap=want[0] - 1)
            assert e.value.name == "OutputTooSmall"
    L = zl.lib()
    # the order of the entry checks: null dictionary, level, InputTooLarge, empty record, empty destination
    for args in ((None, 5, None, 0, None, 3, 2), (None, 0x7E000001, None, 0, None, 0, 2), (None, 0, None, 0, None, 0, 11),
                 (None, 0x7E000001, None, 0, None, 0, 9), (None, 0, None, 0, None, 0, 9)):
        assert L.zlz4_compress_hc_using_dict(*args) == cref.L.hd_compress(*args), args
    buf = np.zeros(16, dtype=np.uint8)
    assert L.zlz4_compress_hc_using_dict(buf.ctypes.data, 5, buf.ctypes.data, 0, None, 0, 9) == hg.OUTPUT_TOO_SMALL


def test_graph_capture(zl, cref, gpu):
    """captured once (staging, K1, K2s, K3 with the fork to the side stream and the join), replayed on new input"""
    nblocks, block, dl = 64, 4096, 61440
    slot = (zl.compressBound(block) + 15) // 16 * 16
    ar = torch.arange(nblocks, dtype=torch.int64, device=gpu)
    in_off, slot_off = ar * block, ar * slot
    in_len = torch.full((nblocks,), block, dtype=torch.int32, device=gpu)
    cap = torch.full((nblocks,), slot, dtype=torch.int32, device=gpu)
    d_off = torch.zeros(nblocks, dtype=torch.int64, device=gpu)
    d_len = torch.full((nblocks,), dl, dtype=torch.int32, device=gpu)
    inp = torch.zeros(nblocks * block, dtype=torch.uint8, device=gpu)
    dct = torch.zeros(dl, dtype=torch.uint8, device=gpu)
    comp = torch.zeros(nblocks * slot, dtype=torch.uint8, device=gpu)
    res = torch.zeros(nblocks, dtype=torch.int64, device=gpu)
    ws = torch.empty(zl.batch_compress_hc_using_dict_workspace(nblocks, block, dl), dtype=torch.uint8, device=gpu)

    def work():
        zl.batch_compress_hc_using_dict(inp, in_off, in_len, comp, slot_off, cap, dct, d_off, d_len, res, block, dl, 9, ws)

    def load(seed):
        s = bytes(dg.text_bytes(dl + nblocks * block, seed))
        dct.copy_(torch.frombuffer(bytearray(s[:dl]), dtype=torch.uint8))
        inp.copy_(torch.frombuffer(bytearray(s[dl:]), dtype=torch.uint8))
        return s

    load(61)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        work()                                        # warm-up outside the capture (lazy module load, side stream creation)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        work()
    text = load(62)
    comp.zero_()
    res.zero_()
    g.replay()
    torch.cuda.synchronize()
    r, c = res.cpu().numpy(), comp.cpu().numpy()
    for i in range(nblocks):
        want = cref.compress(text[dl + i * block:dl + (i + 1) * block], text[:dl], 9)
        assert (int(r[i]), bytes(c[i * slot:i * slot + int(r[i])])) == want, i
