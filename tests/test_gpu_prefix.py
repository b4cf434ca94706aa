"""Prefix decoding on the GPU (zlz4_batch_decompress_safe_prefix(_using_dict), the two host calls,
decompressBlockPrefixes): results and bytes [0, result) against the model
tools/pyref/zig_lz4_prefix.py over the corpus of tests/prefixgen.py -- every copy path of the decoder's single-sequence
half cut at every byte -- in both decoder builds (from 6144 blocks per call the lane-copy build, below it the
sequence-lane build).  Every slot is exactly `cap` bytes between guard bands (gpu_harness)."""
import ctypes as C

import numpy as np
import pytest

import datagen as dg
import gpu_harness as gh
import prefixgen as pg

pytestmark = pytest.mark.gpu
CORRUPTED, INVALID_STATE = -3, -5


def _both_builds(zl, items, gpu):
    assert len(items) > 6144                          # kLaneCopyMinBlocks: the lane-copy build
    pg.compare(items, pg.run_batch(zl, items, gpu))
    pg.compare(items[:512], pg.run_batch(zl, items[:512], gpu))      # the sequence-lane build


def test_exhaustive_cuts(zl, gpu):
    items = pg.plain_items()
    _both_builds(zl, items, gpu)
    pg.compare(items[-512:], pg.run_batch(zl, items[-512:], gpu))    # (the long stream in the sequence-lane build)


def test_exhaustive_cuts_through_the_dictionary_call(zl, gpu):
    """the same items through the _using_dict build with dictionaries of length 0"""
    items = pg.plain_items()
    pg.compare(items, pg.run_batch(zl, items, gpu, use_dict=True))
    pg.compare(items[-512:], pg.run_batch(zl, items[-512:], gpu, use_dict=True))


def test_dictionary_cuts(zl, gpu):
    items = pg.dict_items()
    # what the corpus is there for: every dictionary variant gives a cut, a full decode and (too short) CorruptedData
    kinds = {(d is not None and len(d), pg.expected(s, c, d)[0] == CORRUPTED) for _, s, c, d in items}
    assert {(200, False), (0, True), (0, False), (20, True), (20, False), (70000, False)} <= kinds
    _both_builds(zl, items, gpu)
    # a dictionary of more than 64 KiB counts by its tail only
    tail = {(s, c): pg.expected(s, c, d) for _, s, c, d in items if d is not None and len(d) == 200}
    assert all(pg.expected(s, c, d) == tail[(s, c)] for _, s, c, d in items if d is not None and len(d) == 70000 and (s, c) in tail)


@pytest.mark.parametrize("with_dict", [False, True])
def test_malformed_streams(zl, gpu, with_dict):
    items = list(pg.malformed_items(with_dict))
    where = {s: p for _, s, p in pg.malformed_streams()}
    # both sides of every defect, by the specification's order: cut at or before the defect's position gives cap
    for name, s, cap, d in items:
        assert pg.expected(s, cap, d)[0] == (cap if cap <= where[s] else CORRUPTED), name
    # literals that end exactly at cap in front of an offset of 0: the result is cap
    exact = [it for it in items if it[0].startswith("offset0@") and it[2] == where[it[1]]]
    assert len(exact) == 1 and pg.expected(*exact[0][1:])[0] == exact[0][2]
    pg.compare(items, pg.run_batch(zl, items, gpu, use_dict=with_dict))
    many = (items * (6200 // len(items) + 1))[:6200]                 # the lane-copy build
    pg.compare(many, pg.run_batch(zl, many, gpu, use_dict=with_dict))


@pytest.fixture(scope="module")
def real(oracle):
    blocks = [bytes(b) for b in dg.make_blocks("text", 8, 65536, seed=24)]
    return blocks, [oracle.compress_default(b) for b in blocks], [oracle.compress_hc(b, 9) for b in blocks]


@pytest.mark.parametrize("layout", [None, "packed"])
def test_real_streams(zl, gpu, real, layout):
    blocks, fast, hc = real
    items, want = [], []
    for comp in (fast, hc):
        for b, c in zip(blocks, comp):
            size = len(b)
            for cap in (1, 13, 64, 4096, 4097, size - 33, size - 32, size - 1, size, size + 1):
                items.append(("real@%d" % cap, c, cap, None))
                want.append(b[:cap])
    got = pg.run_batch(zl, items, gpu, layout=gh.Packed(seed=5, fill="cont") if layout else None)
    for (name, _, cap, _), (n, data), w in zip(items, got, want):
        assert n == len(w) and data == w, name
    if layout is None:                                # ... and through the dictionary build with a dictionary nobody reaches
        got = pg.run_batch(zl, [(n, s, c, pg.DICT) for n, s, c, _ in items], gpu)
        for (name, _, cap, _), (n, data), w in zip(items, got, want):
            assert n == len(w) and data == w, name


def _sample(items, count, seed):
    rng = np.random.default_rng(seed)
    return [items[i] for i in sorted(rng.choice(len(items), size=count, replace=False))]


@pytest.mark.parametrize("with_dict", [False, True])
def test_invariants_size_query_and_full_decode(zl, gpu, with_dict):
    import torch
    items = _sample(pg.dict_items() if with_dict else pg.plain_items(), 900, 1) + \
        _sample(pg.malformed_items(with_dict), 300, 2)
    # every stream of the sample that decodes, at its size, one byte more and with room to spare
    seen = {}
    for _, s, _, d in items:
        if (s, d) not in seen:
            seen[(s, d)] = pg.full_size(s, d)
    items += [("whole+%d" % k, s, size + k, d) for (s, d), size in seen.items() if size > 0 for k in (0, 1, 77)]
    got = pg.run_batch(zl, items, gpu, use_dict=with_dict)
    pg.compare(items, got)
    # result == min(zlz4_batch_decompressed_size, cap) wherever the size is >= 0
    streams = [it[1] for it in items]
    buf, offs, lens = gh._pack(streams)
    u32 = lambda a: torch.from_numpy(np.asarray(a).astype(np.uint32).view(np.int32)).to(gpu)
    size = torch.full((len(items),), -999, dtype=torch.int64, device=gpu)
    dl = u32([len(it[3] or b"") for it in items]) if with_dict else None
    zl.batch_decompressed_size(torch.from_numpy(buf).to(gpu), torch.from_numpy(offs).to(gpu), u32(lens), size, dl)
    sizes = size.cpu().tolist()
    assert sum(1 for s in sizes if s >= 0) > 600 and sum(1 for s in sizes if s < 0) > 100
    for it, (n, _), s in zip(items, got, sizes):
        if s >= 0:
            assert n == min(s, it[2]), it[0]
    # cap >= S: the full decoder's result and bytes
    whole = [(it, g) for it, g, s in zip(items, got, sizes) if 0 <= s <= it[2]]
    assert len(whole) >= 30
    full = pg.run_batch(zl, [it for it, _ in whole], gpu, use_dict=with_dict,
                        call=zl.batch_decompress_safe_using_dict if with_dict else zl.batch_decompress_safe)
    assert full == [g for _, g in whole]


def test_invariants_empty_and_refused(zl, gpu):
    import torch
    s = pg.exhaustive_streams()[0][1]
    items = [("cap0", s, 0, None), ("len0", b"", 9, None), ("both", b"", 0, None), ("ok", s, 9, None)]
    for use_dict in (False, True):
        got = pg.run_batch(zl, items, gpu, use_dict=use_dict)
        assert [n for n, _ in got] == [0, 0, 0, 9] and got[3][1] == pg.expected(s, 9, None)[1]
    # a null or misaligned array: InvalidState, and nothing ran (the fenced results and the output keep their fill)
    n = 4
    raw = torch.zeros(64 * 8 + 8, dtype=torch.uint8, device=gpu)
    d_in = torch.from_numpy(np.frombuffer(s, dtype=np.uint8).copy()).to(gpu)
    d_out = torch.full((n * 64,), 0xA5, dtype=torch.uint8, device=gpu)
    off64 = torch.zeros(n, dtype=torch.int64, device=gpu)
    out_off = torch.arange(n, dtype=torch.int64, device=gpu) * 64
    len32 = torch.full((n,), len(s), dtype=torch.int32, device=gpu)
    cap32 = torch.full((n,), 64, dtype=torch.int32, device=gpu)
    res = torch.full((n,), -999, dtype=torch.int64, device=gpu)
    L, p = zl.lib(), lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = [p(d_in), p(off64), p(len32), p(d_out), p(out_off), p(cap32), p(res)]
    zero32 = torch.zeros(n, dtype=torch.int32, device=gpu)
    good_d = good[:6] + [p(d_in), p(off64), p(zero32), p(res)]
    odd = lambda k: C.c_void_p(raw.data_ptr() + k)    # (raw is 256-byte aligned: + 4 breaks 8, + 2 breaks 4)
    for fn, args, wide, narrow in ((L.zlz4_batch_decompress_safe_prefix, good, (1, 4, 6), (2, 5)),
                                   (L.zlz4_batch_decompress_safe_prefix_using_dict, good_d, (1, 4, 7, 9), (2, 5, 8))):
        for k in range(len(args)):
            if fn is L.zlz4_batch_decompress_safe_prefix_using_dict and k == 6:
                continue                              # (d_dict may be null: dictionaries of length 0)
            a = list(args); a[k] = None
            assert fn(st, *a, n) == INVALID_STATE, (fn.__name__, k)
        for k in wide:
            a = list(args); a[k] = odd(4)
            assert fn(st, *a, n) == INVALID_STATE, (fn.__name__, k)
        for k in narrow:
            a = list(args); a[k] = odd(2)
            assert fn(st, *a, n) == INVALID_STATE, (fn.__name__, k)
        assert fn(st, *args, 0) == 0                  # no blocks: nothing to do
    torch.cuda.synchronize()
    assert (res.cpu() == -999).all() and (d_out.cpu() == 0xA5).all()
    assert L.zlz4_batch_decompress_safe_prefix(st, *good, n) == 0
    torch.cuda.synchronize()
    assert res.cpu().tolist() == [64] * n


def test_host_calls_and_block_prefixes(zl, gpu):
    ex = {n: s for n, s, _ in pg.exhaustive_streams()}
    dct = {n: s for n, s, _ in pg.dict_streams()}
    trio = [(ex["rle"], None), (ex["litruns"], None), (dct["span_self"], pg.DICT)]
    bad = pg.malformed_streams()[0]
    for s, d in trio:
        size = pg.full_size(s, d)
        for cap in (0, 1, 13, 100, size - 1, size, size + 1, size + 100):
            wn, wd = pg.expected(s, cap, d)
            if d is None:
                assert zl.decompressSafePrefix(s, cap) == wd
            assert zl.decompressSafePrefixUsingDict(s, cap, d) == wd
            assert len(wd) == min(size, cap)
    # a defect before the cut raises, behind it does not
    assert zl.decompressSafePrefix(bad[1], bad[2]) == pg.expected(bad[1], bad[2], None)[1]
    with pytest.raises(zl.Lz4Error) as e:
        zl.decompressSafePrefix(bad[1], bad[2] + 1)
    assert e.value.code == CORRUPTED
    # only the last 64 KiB of a dictionary is staged
    big = pg.dict_variants()[3][1]
    assert zl.decompressSafePrefixUsingDict(dct["span"], 40, big) == pg.expected(dct["span"], 40, pg.DICT)[1]
    # dict == NULL with dict_len > 0
    buf = (C.c_uint8 * 16)()
    assert zl.lib().zlz4_decompress_safe_prefix_using_dict(trio[0][0], len(trio[0][0]), C.addressof(buf), 16, None, 5) == INVALID_STATE
    # decompressBlockPrefixes: one n for all, one per block, with and without dictionaries
    blocks = [s for s, _ in trio] + [bad[1]]
    got = zl.decompressBlockPrefixes(blocks[:2], 50)
    assert got == [pg.expected(s, 50, None)[1] for s in blocks[:2]]
    ns = [7, 2000, 33, bad[2] + 5]
    dicts = [None, None, pg.DICT, None]
    got = zl.decompressBlockPrefixes(blocks, ns, dicts=dicts)
    want = [pg.expected(s, n, d) for s, n, d in zip(blocks, ns, dicts)]
    assert got == [w[1] if w[0] >= 0 else w[0] for w in want] and got[3] == CORRUPTED
    assert zl.decompressBlockPrefixes([], 5) == []
