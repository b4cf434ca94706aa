"""Legacy lz4 frames on the GPU (zlz4f_batch_compress_legacy_frame, zlz4f_batch_legacy_frame_count,
zlz4f_batch_legacy_frame_decompressed_size, zlz4f_batch_decompress_legacy_frame, the host calls and the Python one-liners;
include/zlz4_amd.h) against the model of tests/legacygen.py: results, `consumed` and bytes.  Every
run writes into slots packed back to back between guard bands filled with a pattern: nothing outside the slots may change,
a frame that succeeds changes only the bytes it returns, and a frame refused for its capacity or for the block table
changes nothing."""
import ctypes as C
import random

import numpy as np
import pytest

import legacygen as g

pytestmark = pytest.mark.gpu
FILL, BAND = 0xA5, 512
MIB8 = 8 << 20


class Run:
    pass


def _arena(torch, dev, caps):
    offs = np.cumsum([0] + list(caps)).astype(np.int64)
    whole = torch.full((int(offs[-1]) + 2 * BAND,), FILL, dtype=torch.uint8, device=dev)
    return whole, whole[BAND:], offs[:-1].tolist()


def _slots(whole, offs, caps, results, keep=()):
    """the bytes every frame returned; asserts what must not have changed.  keep: codes after which a slot is untouched"""
    host = whole.cpu().numpy()
    may = np.zeros(host.shape, dtype=bool)
    data = []
    for o, c, r in zip(offs, caps, results):
        lo = BAND + o
        if r >= 0:
            assert r <= c, "a result above the slot's capacity"
            may[lo:lo + r] = True
            data.append(host[lo:lo + r].tobytes())
        else:
            if r not in keep:
                may[lo:lo + c] = True                 # (unspecified by the contract)
            data.append(None)
    assert (host[~may] == FILL).all(), "bytes outside the returned ranges changed"
    return data


def _fits(nbs, max_blocks):
    """per frame: its blocks all number below max_blocks"""
    out, base = [], 0
    for nb in nbs:
        out.append(nb == 0 or base + nb <= max_blocks)
        base += nb
    return out


# ----------------------------------------------------------------------------- decode side
def run_decode(zl, dev, frames, caps=None, max_blocks=None):
    """count, size query and decode through the raw tensor wrappers, each checked against the model -> Run"""
    import torch
    lz4f = zl.lz4f
    n = len(frames)
    r = Run()
    d_src, src_off, src_len = zl._stage(frames, dev)

    def i64(k, fill=-999):
        return torch.full((max(1, k),), fill, dtype=torch.int64, device=dev)[:k]

    model = [g.read(f) for f in frames]
    nblocks, c0, totals = i64(n), i64(n), i64(1)
    lz4f.legacyFrameCountBatch(d_src, src_off, src_len, nblocks, c0, totals)
    r.nblocks, r.total = nblocks.cpu().tolist(), int(totals.item())
    assert r.nblocks == [m.nb for m in model] and r.total == sum(r.nblocks)
    assert c0.cpu().tolist() == [m.consumed for m in model]
    mb = r.total if max_blocks is None else max_blocks
    fits = _fits(r.nblocks, mb)

    size, c1 = i64(n), i64(n)
    lz4f.legacyFrameDecompressedSizeBatch(d_src, src_off, src_len, size, c1, mb)
    r.size = size.cpu().tolist()
    assert r.size == [m.result if ok else g.INVALID_STATE for m, ok in zip(model, fits)]
    assert c1.cpu().tolist() == [m.consumed for m in model]

    r.caps = [max(s, 0) for s in r.size] if caps is None else list(caps)
    whole, d_dst, r.offs = _arena(torch, dev, r.caps)
    result, c2 = i64(n), i64(n)
    lz4f.decompressLegacyFrameBatch(d_src, src_off, src_len, d_dst, torch.tensor(r.offs, dtype=torch.int64, device=dev),
                                    torch.tensor(r.caps, dtype=torch.int64, device=dev), result, c2, mb)
    torch.cuda.synchronize()
    r.result = result.cpu().tolist()
    assert c2.cpu().tolist() == [m.consumed for m in model]
    r.data = _slots(whole, r.offs, r.caps, r.result, keep=(g.DST_TOO_SMALL, g.INVALID_STATE))
    for f, (m, ok) in enumerate(zip(model, fits)):
        want = m if m.result < 0 or m.result <= r.caps[f] else m._replace(result=g.DST_TOO_SMALL, content=None)
        if not ok:
            want = m._replace(result=g.INVALID_STATE, content=None)
        assert r.result[f] == want.result, (f, r.result[f], want.result)
        assert r.data[f] == want.content, f
    return r


def test_chains_of_1_to_1025_blocks(zl, gpu):
    """1, 2, 65, 257 and 1 025 blocks of 1..300 bytes: every wave and workgroup boundary of the per-frame scans"""
    frames, contents = [], []
    for k, count in enumerate((1, 2, 65, 257, 1025, 64, 128, 63)):
        blocks, content = g.small_blocks(count, 20 + k)
        frames.append(g.build(blocks))
        contents.append(content)
    r = run_decode(zl, gpu, frames)
    assert r.data == contents and r.nblocks == [1, 2, 65, 257, 1025, 64, 128, 63]
    assert zl.lz4f.decompressLegacyFrames(frames) == [(c, len(f)) for c, f in zip(contents, frames)]


def test_the_crafted_table(zl, gpu):
    """every ending of the walk, every defect, the token-0x00 block, blocks of 8 MiB and of 8 MiB + 1"""
    cases = g.table()
    r = run_decode(zl, gpu, [c.buf for c in cases])
    for c, res, d in zip(cases, r.result, r.data):
        assert res == c.result, c.name
        if c.result >= 0:
            assert len(d) == c.result, c.name
    by = {c.name: k for k, c in enumerate(cases)}
    assert r.data[by["block_of_8mib"]] == bytes(MIB8) and r.result[by["block_of_8mib_plus_1"]] == g.FAILED
    assert r.result[by["corrupt_block_then_torn_tail"]] == g.FAILED and r.result[by["torn_tail_alone"]] == g.SIZE_WRONG
    assert r.result[by["word_bound_too_few_bytes"]] == g.SIZE_WRONG and r.result[by["word_bound_plus_1"]] >= 0
    got = zl.lz4f.decompressLegacyFrames([c.buf for c in cases])
    assert got == [(d if d is not None else res, c.consumed) for c, res, d in zip(cases, r.result, r.data)]


def test_consumed_chains_the_members_of_a_file(zl, gpu):
    blocks, content = g.small_blocks(5, 31)
    a, b = g.build(blocks[:2]), g.build(blocks[2:])
    buf = a + g.skippable() + b
    (d0, used0), = zl.lz4f.decompressLegacyFrames([buf])
    assert used0 == len(a)
    rest = buf[used0 + len(g.skippable()):]
    (d1, used1), = zl.lz4f.decompressLegacyFrames([rest])
    assert d0 + d1 == content and used1 == len(b)
    # the plain multiframe split still treats the legacy magic as a member it cannot delimit
    assert zl.lz4f.decompressMultiframes([buf]) == [g.TYPE_UNKNOWN]


def test_decode_slot_capacities(zl, gpu):
    blocks, content = g.small_blocks(70, 33)
    f, small = g.build(blocks), g.build(blocks[:1])
    one = len(g.read(small).content)
    frames = [f, f, small, small, g.build([g.EMPTY]), f]
    caps = [len(content), len(content) - 1, one, one - 1, 0, len(content) + 7]
    r = run_decode(zl, gpu, frames, caps=caps)
    assert r.result == [len(content), g.DST_TOO_SMALL, one, g.DST_TOO_SMALL, 0, len(content)]


def _mixed(count, seed):
    rnd = random.Random(seed)
    blocks, _ = g.small_blocks(40, 35)
    bad = [g.CORRUPT, b"", g.zeros_block(MIB8 + 1)]
    tails = [b"", b"", b"", b"\x01", b"\x01\x02\x03", g.le32(g.MODERN_MAGIC) + b"zz", g.le32(g.BLOCK_BOUND) + b"q"]
    out = []
    for _ in range(count):
        bl = [rnd.choice(blocks) for _ in range(rnd.randrange(1, 4))]
        if rnd.random() < 0.25:
            bl[rnd.randrange(len(bl))] = rnd.choice(bad)
        out.append(rnd.choice([g.build(bl) + rnd.choice(tails), g.build(bl), g.build(bl)[:rnd.randrange(0, 9)]]))
    return out


def test_batch_of_1000_mixed_frames(zl, gpu):
    frames = _mixed(1000, 13)
    r = run_decode(zl, gpu, frames)
    codes = {c for c in r.result if c < 0}
    assert codes == {g.HEADER_INCOMPLETE, g.SIZE_WRONG, g.FAILED} and sum(c >= 0 for c in r.result) > 300
    assert {1, 2, 3} <= set(r.nblocks)


def test_decode_max_blocks_one_short(zl, gpu):
    blocks, _ = g.small_blocks(9, 37)
    frames = [g.build(blocks[:3]), g.le32(g.MAGIC), g.build(blocks[3:7]), g.build([]), g.build(blocks[7:]), b"\x02\x21"]
    full = run_decode(zl, gpu, frames)
    r = run_decode(zl, gpu, frames, max_blocks=full.total - 1)
    assert r.result == full.result[:4] + [g.INVALID_STATE, g.HEADER_INCOMPLETE] and r.data[:4] == full.data[:4]
    r = run_decode(zl, gpu, frames, max_blocks=0)
    assert r.result == [g.INVALID_STATE, 0, g.INVALID_STATE, 0, g.INVALID_STATE, g.HEADER_INCOMPLETE]


# ----------------------------------------------------------------------------- compress side
def run_compress(zl, dev, items, prefs, caps=None, max_blocks=None):
    """the batch compress call into slots packed back to back, checked against the model's frames -> Run"""
    import torch
    lz4f = zl.lz4f
    bs = prefs.block_size if prefs is not None and prefs.block_size else MIB8
    level = prefs.compression_level if prefs is not None else 0
    r = Run()
    bounds = [g.bound(len(b), bs) for b in items]
    assert bounds == [lz4f.legacyCompressFrameBound(len(b), prefs) for b in items]
    r.caps = bounds if caps is None else list(caps)
    nbs = [(len(b) + bs - 1) // bs for b in items]
    mb = sum(nbs) if max_blocks is None else max_blocks
    d_src, src_off, src_len = zl._stage(items, dev)
    whole, d_dst, r.offs = _arena(torch, dev, r.caps)
    result = torch.full((len(items),), -999, dtype=torch.int64, device=dev)
    lz4f.compressLegacyFrameBatch(d_src, src_off, src_len, d_dst, torch.tensor(r.offs, dtype=torch.int64, device=dev),
                                  torch.tensor(r.caps, dtype=torch.int64, device=dev), result, prefs, max_blocks=mb)
    torch.cuda.synchronize()
    r.result = result.cpu().tolist()
    r.data = _slots(whole, r.offs, r.caps, r.result, keep=(g.DST_TOO_SMALL, g.INVALID_STATE))
    for f, (b, ok) in enumerate(zip(items, _fits(nbs, mb))):
        if r.caps[f] < bounds[f]:
            assert r.result[f] == g.DST_TOO_SMALL, f
        elif not ok:
            assert r.result[f] == g.INVALID_STATE, f
        else:
            want = g.write(b, bs, level)
            assert r.result[f] == len(want) and r.data[f] == want, (f, len(b), r.result[f], len(want))
    return r


def _items(bs, seed=3):
    """D-text of every length at which the chunking takes another path, and frames with a random, growing block"""
    t = g.text(3 * bs + 5)
    rnd = bytes(g.dg.random_bytes(bs, seed))
    items = [t[:n] for n in (0, 1, 12, 13, bs - 1, bs, bs + 1, 3 * bs + 5)] + [rnd, t[:bs] + rnd + t[:5]]
    assert len(g.write(rnd, bs)) > 4 + 4 + bs, "random bytes grow"
    return items


@pytest.mark.parametrize("bs", [4096, 70000])
def test_compress_fast_level(zl, gpu, bs):
    """bs 4096: the 16-bit table of k_compress_fast; bs 70 000: the 32-bit one"""
    r = run_compress(zl, gpu, _items(bs), zl.LegacyPrefs(bs, 0))
    assert r.result[0] == 4 and r.data[0] == g.le32(g.MAGIC)
    assert all(x >= 0 for x in r.result)


@pytest.mark.parametrize("level", [3, 9])
def test_compress_hc_levels(zl, gpu, level):
    r = run_compress(zl, gpu, _items(4096), zl.LegacyPrefs(4096, level))
    assert all(x >= 0 for x in r.result)
    assert r.data[7] != g.write(_items(4096)[7], 4096, 0), "the level reaches the compressor"


@pytest.mark.parametrize("level", [2, 12])
def test_compress_levels_2_and_12(zl, gpu, level):
    run_compress(zl, gpu, [g.text(3 * 4096 + 5)], zl.LegacyPrefs(4096, level))


def test_compress_the_real_block_size(zl, gpu):
    """8 MiB chunks and a last block of one byte, with the default preferences; the frames decode back"""
    t = g.text(MIB8 + 1)
    items = [t[:MIB8], t]
    r = run_compress(zl, gpu, items, None)
    assert [g.read(f).nb for f in r.data] == [1, 2] and g.walk(r.data[1]).blocks[1][1] == 2
    back = run_decode(zl, gpu, r.data)
    assert back.data == items
    assert run_compress(zl, gpu, items, zl.LegacyPrefs(MIB8, 0)).data == r.data


def test_compress_slot_capacities_and_max_blocks(zl, gpu):
    p = zl.LegacyPrefs(4096, 0)
    items = _items(4096)
    bounds = [g.bound(len(b), 4096) for b in items]
    caps = [b - (1 if k % 2 else 0) for k, b in enumerate(bounds)]
    r = run_compress(zl, gpu, items, p, caps=caps)
    assert [x == g.DST_TOO_SMALL for x in r.result] == [k % 2 == 1 for k in range(len(items))]
    full = run_compress(zl, gpu, items, p)
    nbs = [(len(b) + 4095) // 4096 for b in items]
    r = run_compress(zl, gpu, items, p, max_blocks=sum(nbs) - 1)
    assert r.result[:-1] == full.result[:-1] and r.data[:-1] == full.data[:-1] and r.result[-1] == g.INVALID_STATE


def test_round_trip_and_liblz4_reads_every_block(zl, gpu):
    lib = C.CDLL("liblz4.so.1")
    lib.LZ4_decompress_safe.restype = C.c_int
    lib.LZ4_decompress_safe.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_int]
    t = g.text(300000)
    items = [t[:n] for n in (0, 1, 100, 65536, 65537, 300000)] + [bytes(g.dg.random_bytes(70001, 5)), bytes(200000)]
    for prefs in (zl.LegacyPrefs(65536, 0), zl.LegacyPrefs(100000, 4)):
        frames = zl.lz4f.compressLegacyFrames(items, prefs)
        assert all(isinstance(f, bytes) for f in frames)
        assert zl.lz4f.decompressLegacyFrames(frames) == [(b, len(f)) for b, f in zip(items, frames)]
        for b, f in zip(items, frames):
            w = g.walk(f)
            assert w.verdict == 0 and len(w.blocks) == (len(b) + prefs.block_size - 1) // prefs.block_size
            dst = C.create_string_buffer(MIB8)
            out = b""
            for off, size in w.blocks:
                k = lib.LZ4_decompress_safe(f[off:off + size], dst, size, MIB8)
                assert k >= 0
                out += dst.raw[:k]
            assert out == b
    assert zl.lz4f.compressLegacyFrames([]) == [] and zl.lz4f.decompressLegacyFrames([]) == []


def test_host_calls_answer_the_batch_of_one(zl, gpu):
    lz4f = zl.lz4f
    t = g.text(3 * 4096 + 5)
    for prefs in (zl.LegacyPrefs(4096, 0), zl.LegacyPrefs(4096, 9), None):
        for b in (b"", t[:1], t):
            f = lz4f.compressLegacyFrame(b, prefs)
            assert [f] == lz4f.compressLegacyFrames([b], prefs)
            assert lz4f.decompressLegacyFrame(f) == (b, len(f)) and lz4f.legacyFrameDecompressedSize(f) == (len(b), len(f))
    f = lz4f.compressLegacyFrame(t, zl.LegacyPrefs(4096, 0))
    assert lz4f.decompressLegacyFrame(f, dst_cap=len(t) + 100) == (t, len(f))
    with pytest.raises(zl.Lz4Error) as e:
        lz4f.decompressLegacyFrame(f, dst_cap=len(t) - 1)
    assert e.value.code == g.DST_TOO_SMALL
    with pytest.raises(zl.Lz4Error) as e:
        lz4f.compressLegacyFrame(t, zl.LegacyPrefs(4096, 0), dst_cap=g.bound(len(t), 4096) - 1)
    assert e.value.code == g.DST_TOO_SMALL
    for c in g.table():
        want = lz4f.decompressLegacyFrames([c.buf])[0]
        for call in (lz4f.decompressLegacyFrame, lz4f.legacyFrameDecompressedSize):
            if c.result < 0:
                with pytest.raises(zl.Lz4Error) as e:
                    call(c.buf)
                assert e.value.code == c.result == want[0], c.name
            else:
                got = call(c.buf)
                assert got == (want if call is lz4f.decompressLegacyFrame else (len(want[0]), want[1])), c.name
                assert got[1] == c.consumed, c.name


def test_refusals_of_the_raw_c_calls(zl, gpu):
    """null and misaligned arrays, workspaces that are too small, null or misaligned, an invalid block size, nframes == 0:
    each answers its code and launches nothing"""
    import torch
    L = zl.lib()
    blocks, content = g.small_blocks(3, 39)
    frames = [g.build(blocks), g.build(blocks[:1])]
    d_src, src_off, src_len = zl._stage(frames, gpu)
    st = zl._stream()
    p = lambda t: C.c_void_p(t.data_ptr())           # noqa: E731
    i64 = lambda n, v=7: torch.full((n,), v, dtype=torch.int64, device=gpu)   # noqa: E731
    nblocks, consumed, totals, size, result = i64(2), i64(2), i64(2), i64(2), i64(2)
    dst_off, dst_cap = i64(2, 0), i64(2, len(content))
    dst_off[1] = len(content)
    d_dst = torch.full((2 * len(content),), FILL, dtype=torch.uint8, device=gpu)
    ws = torch.empty(max(L.zlz4f_batch_decompress_legacy_frame_workspace(2, 4),
                         L.zlz4f_batch_compress_legacy_frame_workspace(2, 4, None)) + 16, dtype=torch.uint8, device=gpu)
    count = (st, p(d_src), p(src_off), p(src_len), 2, p(nblocks), p(consumed), p(totals))
    query = (st, p(d_src), p(src_off), p(src_len), p(size), p(consumed), 2, 4, p(ws), ws.numel())
    dec = (st, p(d_src), p(src_off), p(src_len), p(d_dst), p(dst_off), p(dst_cap), p(result), p(consumed), 2, 4, p(ws),
           ws.numel())
    prefs = zl.LegacyPrefs(4096, 0)
    comp = (st, p(d_src), p(src_off), p(src_len), p(d_dst), p(dst_off), p(dst_cap), p(result), 2, 4, C.byref(prefs), p(ws),
            ws.numel())
    before = [t.clone() for t in (nblocks, consumed, totals, size, result, d_dst)]

    def refused(fn, args, arrays, unaligned_only=(), ws_at=None, need=0):
        for k in arrays:
            bad = list(args)
            if k not in unaligned_only:
                bad[k] = None
                assert fn(*bad) == g.INVALID_STATE, (fn.__name__, k, "null")
            bad[k] = C.c_void_p(args[k].value + 4)
            assert fn(*bad) == g.INVALID_STATE, (fn.__name__, k, "misaligned")
        if ws_at is not None:
            bad = list(args)
            bad[ws_at + 1] = need - 1
            assert need > 0 and fn(*bad) == g.INVALID_STATE, (fn.__name__, "workspace one byte short")
            bad = list(args)
            bad[ws_at] = None
            assert fn(*bad) == g.INVALID_STATE, (fn.__name__, "workspace null")
            bad[ws_at] = C.c_void_p(args[ws_at].value + 8)
            assert fn(*bad) == g.INVALID_STATE, (fn.__name__, "workspace misaligned")

    refused(L.zlz4f_batch_legacy_frame_count, count, (2, 3, 5, 6, 7), unaligned_only=(6,))
    assert L.zlz4f_batch_legacy_frame_count(*(count[:1] + (None,) + count[2:])) == g.INVALID_STATE
    refused(L.zlz4f_batch_legacy_frame_decompressed_size, query, (2, 3, 4, 5), unaligned_only=(5,), ws_at=8,
            need=L.zlz4f_batch_legacy_frame_decompressed_size_workspace(2, 4))
    assert L.zlz4f_batch_legacy_frame_decompressed_size(*(query[:1] + (None,) + query[2:])) == g.INVALID_STATE
    refused(L.zlz4f_batch_decompress_legacy_frame, dec, (2, 3, 5, 6, 7, 8), unaligned_only=(8,), ws_at=11,
            need=L.zlz4f_batch_decompress_legacy_frame_workspace(2, 4))
    for k in (1, 4):                                  # d_src, d_dst
        assert L.zlz4f_batch_decompress_legacy_frame(*(dec[:k] + (None,) + dec[k + 1:])) == g.INVALID_STATE
    refused(L.zlz4f_batch_compress_legacy_frame, comp, (2, 3, 5, 6, 7), ws_at=11,
            need=L.zlz4f_batch_compress_legacy_frame_workspace(2, 4, C.byref(prefs)))
    for k in (1, 4):
        assert L.zlz4f_batch_compress_legacy_frame(*(comp[:k] + (None,) + comp[k + 1:])) == g.INVALID_STATE
    big = zl.LegacyPrefs(MIB8 + 1, 0)
    assert L.zlz4f_batch_compress_legacy_frame(*(comp[:10] + (C.byref(big),) + comp[11:])) == g.MAX_BLOCK_SIZE_INVALID
    with pytest.raises(zl.Lz4Error) as e:
        zl.lz4f.compressLegacyFrames([b"abc"], big)
    assert e.value.code == g.MAX_BLOCK_SIZE_INVALID
    torch.cuda.synchronize()
    after = (nblocks, consumed, totals, size, result, d_dst)
    assert all(torch.equal(x, y) for x, y in zip(before, after)), "a refused call wrote"
    # nframes == 0: 0, and the count stores a total of 0
    assert L.zlz4f_batch_legacy_frame_count(st, None, None, None, 0, None, None, p(totals)) == 0
    assert L.zlz4f_batch_legacy_frame_decompressed_size(st, None, None, None, None, None, 0, 0, None, 0) == 0
    assert L.zlz4f_batch_decompress_legacy_frame(st, None, None, None, None, None, None, None, None, 0, 0, None, 0) == 0
    assert L.zlz4f_batch_compress_legacy_frame(st, None, None, None, None, None, None, None, 0, 0, None, None, 0) == 0
    assert totals.tolist() == [0, 7]
    # the calls as they stand, with and without d_consumed
    assert L.zlz4f_batch_legacy_frame_count(*count) == 0 and L.zlz4f_batch_legacy_frame_decompressed_size(*query) == 0
    assert nblocks.tolist() == [3, 1] and totals.tolist() == [4, 7] and consumed.tolist() == [len(f) for f in frames]
    assert size.tolist() == [len(content), len(g.read(frames[1]).content)]
    consumed.fill_(7)
    assert L.zlz4f_batch_decompress_legacy_frame(*(dec[:8] + (None,) + dec[9:])) == 0
    assert result.tolist() == size.tolist() and consumed.tolist() == [7, 7]
    host = d_dst.cpu().numpy().tobytes()
    assert host[:len(content)] == content and host[len(content):len(content) + result.tolist()[1]] == g.read(frames[1]).content
