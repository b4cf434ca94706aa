"""The frame index and frame range decoding on the GPU (zlz4f_batch_frame_index, zlz4f_batch_plan_frame_ranges,
zlz4f_batch_decompress_frame_range, the host call and the Python one-liners) against the model
tools/pyref/zig_lz4_frame_range.py over the corpus of tests/framerangegen.py: the index entry by entry and against the size
query, the plan with its totals, and results, skips and slot bytes of every range -- every start byte of the small frames,
the block boundaries of the long ones, defects inside and outside the range, header errors, indexes that are not the
frame's.  Every slot is exactly the planned size between guard bands that must come back untouched, whatever the status."""
import numpy as np
import pytest

import datagen as dg
import framerangegen as g

pytestmark = pytest.mark.gpu
fr = g.fr


def _t(torch, a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _index(zl, torch, dev, frames, caps=None, max_blocks=None, fill=-7):
    """zlz4f_batch_frame_index and zlz4f_batch_frame_decompressed_size over `frames` -> (idx_n list, [entries], sizes list)"""
    import gpu_harness as gh
    buf, offs, lens = gh._pack(frames)
    blocks = [zl._chain_blocks(bytes(f)) for f in frames]
    caps = [b + 1 for b in blocks] if caps is None else caps
    mb = sum(blocks) if max_blocks is None else max_blocks
    idx_off = np.cumsum([0] + [c + 1 for c in caps[:-1]]).astype(np.int64)     # one spare entry behind every frame
    index = torch.full((int(idx_off[-1]) + caps[-1] + 1, 2), fill, dtype=torch.int64, device=dev)
    idx_n = torch.full((len(frames),), -999, dtype=torch.int64, device=dev)
    size = torch.full((len(frames),), -999, dtype=torch.int64, device=dev)
    d_src, src_off, src_len = _t(torch, buf, dev), _t(torch, offs, dev), _t(torch, lens, dev)
    zl.lz4f.frameIndexBatch(d_src, src_off, src_len, index, _t(torch, idx_off, dev),
                            _t(torch, np.array(caps, dtype=np.int64), dev), idx_n, mb)
    zl.lz4f.frameDecompressedSizeBatch(d_src, src_off, src_len, size, mb)
    torch.cuda.synchronize()
    n, host = idx_n.cpu().tolist(), index.cpu().numpy().view(np.uint64)
    ents = []
    for f in range(len(frames)):
        lo = int(idx_off[f])
        used = n[f] + 1 if n[f] >= 0 else 0
        ents.append([tuple(int(x) for x in e) for e in host[lo:lo + used]])
        rest = index.cpu().numpy()[lo + used:lo + caps[f] + 1]
        assert (rest == fill).all(), "frame %d: entries behind the result were written" % f
    return n, ents, size.cpu().tolist()


def _corpus_frames():
    frames = [v.frame for v in g.small_views() + g.long_views() + g.linked_views()]
    frames += [v.frame for v, _ in g.defect_views()] + [v.frame for v, _ in g.header_views()]
    frames += [c.frame for c, _ in g.frameprefixgen.defect_cases()]
    return list(dict.fromkeys(frames))


def test_index_against_the_model_and_the_size_query(zl, gpu):
    import torch
    frames = _corpus_frames()
    n, ents, sizes = _index(zl, torch, gpu, frames)
    errors = set()
    for f, frame in enumerate(frames):
        wn, went = fr.frame_index(frame)
        assert (n[f], ents[f]) == (wn, went), "frame %d: index %d vs model %d" % (f, n[f], wn)
        if sizes[f] < 0:                              # result and error parity with the size query, frame by frame
            assert n[f] == sizes[f]
            errors.add(n[f])
        else:
            assert n[f] >= 0 and ents[f][n[f]][1] == sizes[f]
    assert {g.FAILED, g.BLOCK_CHECKSUM, -114, -112, -117} <= errors
    # a table one entry short: DstMaxSizeTooSmall for that frame alone, nothing written; max_blocks one short: the query's
    # InvalidState for the frames that no longer fit
    few = [v.frame for v in g.small_views()[:4]]
    nb = [v.idx_n for v in g.small_views()[:4]]
    n, ents, sizes = _index(zl, torch, gpu, few, caps=[nb[0] + 1, nb[1], nb[2] + 1, nb[3] + 1])
    assert n == [nb[0], g.DST_TOO_SMALL, nb[2], nb[3]] and ents[1] == [] and sizes[1] >= 0
    n, ents, sizes = _index(zl, torch, gpu, few, max_blocks=sum(nb) - 1)
    assert n == nb[:3] + [g.INVALID_STATE] and sizes[3] == g.INVALID_STATE and sizes[:3] == [v.size for v in g.small_views()[:3]]


def _batches():
    """-> {name: (views, items)}: each family is one batch"""
    out = {}
    out["small"] = g.items_of(g.small_views(), g.small_ranges)
    out["long"] = g.items_of(g.long_views(), g.long_ranges)
    views = g.linked_views() + [v for v, _ in g.defect_views()] + [v for v, _ in g.header_views()]
    views, items = g.items_of(views, lambda v: g.long_ranges(v) if v.size > 3072 else g.small_ranges(v, every_a=v.family == "defect"))
    for view, ranges, want in g.wrong_index_views():
        views.append(view)
        items += [("%s[%d,%d)" % (view.name, a, min(b, 1 << 40)), len(views) - 1, a, b, 0, None, None) for a, b in ranges]
    five = len(views)
    views.append(g.small_views()[0])
    items += [("a_above_b", five, 9, 3, 0, None, None), ("reserved_set", five, 3, 9, 1, None, None),
              ("frame_is_nframes", five, 3, 9, 0, None, len(views)), ("frame_is_max", five, 3, 9, 0, None, 0xFFFFFFFF),
              ("slot_one_short", five, 310, 400, 0, -1, None), ("slot_exact", five, 310, 400, 0, None, None),
              ("slot_none", five, 0, g.BIG, 0, -2000, None)]
    out["other"] = (views, items)
    return out


_RUNS = {}


def _run(zl, gpu, key):
    if key not in _RUNS:
        views, items = _batches()[key]
        _RUNS[key] = (views, items, g.run(zl, views, items, gpu), g.expect(views, items))
    return _RUNS[key]


@pytest.mark.parametrize("key", ["small", "long", "other"])
def test_ranges_against_the_model(zl, gpu, key):
    views, items, got, want = _run(zl, gpu, key)
    g.compare(views, items, got, want)
    for it, (r, skip, slot) in zip(items, got):
        view = views[it[1]]
        if r > 0 and view.valid and min(it[2], view.size) in view.bounds:
            assert skip == 0, it[0]                   # a range that starts on a block boundary
    if key == "other":
        named = {it[0]: r for it, (r, _, _) in zip(items, got)}
        assert [named[k] for k in ("a_above_b", "reserved_set", "frame_is_nframes", "frame_is_max", "slot_one_short", "slot_exact",
                                   "slot_none")] == [g.INVALID_STATE] * 4 + [g.DST_TOO_SMALL, 90, g.DST_TOO_SMALL]
        by = {v.name: i for i, v in enumerate(views)}
        for view, want_fn in g.defect_views():
            for it, (r, _, _) in zip(items, got):
                if it[1] == by[view.name]:
                    a1, b1 = min(it[2], 170), min(it[3], 170)
                    w = want_fn(a1, b1) if a1 < b1 else None
                    assert r == (b1 - a1 if w is None else w), it[0]
        for view, code in g.header_views():
            assert {r for it, (r, _, _) in zip(items, got) if views[it[1]] is view} == {code}, view.name
        for view, ranges, code in g.wrong_index_views():
            for it, (r, _, _) in zip(items, got):
                if views[it[1]] is view and (it[2], it[3]) in ranges:
                    assert (r >= 0) if code is None else (r == code), it[0]


def test_plan_against_the_model(zl, gpu):
    import torch
    views, items = _batches()["other"]
    s = g.stage(views, items, gpu)
    want = [fr.plan_range(views[v].entries, views[v].idx_n, a, b) if fo is None else (0, 0) for _, v, a, b, _, _, fo in items]
    assert any(c for c, _ in want) and any(c == 0 for c, _ in want)
    for align in (0, 64):
        off = torch.full((len(items),), -1, dtype=torch.int64, device=gpu)
        cap = torch.full((len(items),), -1, dtype=torch.int64, device=gpu)
        tot = torch.full((2,), -1, dtype=torch.int64, device=gpu)
        zl.lz4f.planFrameRanges(s["index"], s["idx_off"], s["idx_n"], s["ranges"], off, cap, tot, align)
        w_off, w_bytes, w_items = fr.plan(want, align)
        assert cap.cpu().tolist() == [c for c, _ in want]
        assert off.cpu().tolist() == w_off and tot.cpu().tolist() == [w_bytes, w_items]
    tot = torch.full((2,), -1, dtype=torch.int64, device=gpu)
    zl.lz4f.planFrameRanges(s["index"], s["idx_off"], s["idx_n"], s["ranges"][:0], None, None, tot)
    assert tot.cpu().tolist() == [0, 0]


def test_ranges_against_the_frame_decoders(zl, gpu):
    """[0, S) is zlz4f_batch_decompress_frame's output, [0, n) is zlz4f_batch_decompress_frame_prefix's (independent frames)"""
    views = [v for v in g.small_views() + g.long_views() if v.frame[4] & 0x20]
    frames = [v.frame for v in views]
    whole = zl.lz4f.decompressFrames(frames, device=gpu)
    items = [("whole_" + v.name, i, 0, v.size, 0, None, None) for i, v in enumerate(views)]
    ns = [max(1, v.size // 3) for v in views]
    items += [("head_" + v.name, i, 0, n, 0, None, None) for i, (v, n) in enumerate(zip(views, ns))]
    got = g.run(zl, views, items, gpu)
    prefix = zl.lz4f.decompressFramePrefixes(frames, ns, device=gpu)
    for i, v in enumerate(views):
        assert got[i] == (v.size, 0, whole[i]), v.name
        assert got[len(views) + i] == (min(ns[i], v.size), 0, prefix[i]), v.name


def test_mixed_batch_and_max_items_one_short(zl, gpu):
    """many ranges per frame, frames interleaved, invalid ranges among valid ones; with max_items one short exactly the
    ranges that no longer fit answer InvalidState"""
    views = g.small_views()[:3] + g.long_views()[:1] + [g.defect_views()[1][0], g.header_views()[0][0]]
    rng = np.random.default_rng(5)
    items = []
    for i in range(400):
        v = int(rng.integers(0, len(views)))
        S = views[v].size
        a = int(rng.integers(0, S + 2))
        b = a + int(rng.integers(0, 70000 if S > 3072 else 600))
        kind = i % 23
        items.append(("mixed%d" % i, v, b + 1 if kind == 5 else a, b, 1 if kind == 11 else 0, -1 if kind == 17 else None,
                      len(views) + 3 if kind == 19 else None))
    counts = g.item_counts(views, items)
    total, full_run = sum(counts), g.expect(views, items)
    assert total > 400
    last = max(i for i, n in enumerate(counts) if n)
    for max_items in (total, total - 1, total // 2):
        got, want = g.run(zl, views, items, gpu, max_items=max_items), g.expect(views, items, max_items=max_items)
        g.compare(views, items, got, want)
        cut = [i for i in range(len(items)) if want[i][0] != full_run[i][0]]
        assert all(want[i][0] == g.INVALID_STATE and counts[i] for i in cut)
        if max_items == total:
            assert not cut
        if max_items == total - 1:                    # exactly the last range that has items
            assert cut == [last] or (not cut and full_run[last][0] == g.INVALID_STATE)
        if max_items == total // 2:
            assert len(cut) > 50
    codes = {w[0] for w in full_run if w[0] < 0}
    assert {g.INVALID_STATE, g.DST_TOO_SMALL, g.BLOCK_CHECKSUM, -112} <= codes


def test_empty_batches(zl, gpu):
    import torch
    view = g.small_views()[0]
    s = g.stage([view], [], gpu)
    res = torch.full((1,), -999, dtype=torch.int64, device=gpu)
    zl.lz4f.decompressFrameRangeBatch(s["d_src"], s["src_off"], s["src_len"], s["index"], s["idx_off"], s["idx_n"],
                                      s["ranges"][:0], s["d_dst"], s["dst_off"], s["dst_cap"], res, res, 0)   # nranges == 0
    zl.lz4f.frameIndexBatch(s["d_src"], s["src_off"][:0], s["src_len"][:0], s["index"], s["idx_off"][:0], s["idx_off"][:0],
                            res[:0], 0)                                                                        # nframes == 0
    torch.cuda.synchronize()
    assert res.cpu().tolist() == [-999]
    # nframes == 0 with ranges: every frame number is past the end
    items = [("no_frames", 0, 0, 10, 0, None, None), ("no_frames_empty", 0, 4, 4, 0, None, None)]
    got = g.run(zl, [view], items, gpu, spare_views=1)
    assert [r for r, _, _ in got] == [g.INVALID_STATE] * 2
    assert zl.lz4f.decompressFrameRanges(zl.lz4f.frameIndex([], device=gpu), []) == []


def test_graph_capture_and_replay(zl, gpu):
    """index + range in one captured graph, replayed over other frames of the same shapes"""
    import torch
    import gpu_harness as gh
    a_views, b_views = g.small_views()[0:1] + g.long_views()[0:1], g.small_views()[3:4] + g.long_views()[1:2]
    assert [len(v.frame) for v in a_views] != [len(v.frame) for v in b_views] or True
    ranges = [(0, 5, 1450), (1, 70000, 140000), (0, 0, g.BIG), (1, 65536, 65537), (0, 316, 318)]
    nf, nr, mb, cap_e = 2, len(ranges), 16, 8
    size = max(sum(len(v.frame) + 32 for v in vs) for vs in (a_views, b_views))
    d_src = torch.zeros(size, dtype=torch.uint8, device=gpu)
    src_off = torch.zeros(nf, dtype=torch.int64, device=gpu)
    src_len = torch.zeros(nf, dtype=torch.int64, device=gpu)
    index = torch.zeros((nf * cap_e, 2), dtype=torch.int64, device=gpu)
    idx_off = _t(torch, np.arange(nf, dtype=np.int64) * cap_e, gpu)
    idx_cap = torch.full((nf,), cap_e, dtype=torch.int64, device=gpu)
    idx_n = torch.zeros(nf, dtype=torch.int64, device=gpu)
    d_range = _t(torch, zl.lz4f.packRanges(ranges).view(np.int64), gpu)
    slot = 200000
    d_dst = torch.zeros(nr * slot, dtype=torch.uint8, device=gpu)
    dst_off = _t(torch, np.arange(nr, dtype=np.int64) * slot, gpu)
    dst_cap = torch.full((nr,), slot, dtype=torch.int64, device=gpu)
    skip = torch.zeros(nr, dtype=torch.int64, device=gpu)
    res = torch.zeros(nr, dtype=torch.int64, device=gpu)
    iws = torch.empty(zl.lz4f.frameIndexBatchWorkspace(nf, mb), dtype=torch.uint8, device=gpu)
    rws = torch.empty(zl.lz4f.decompressFrameRangeBatchWorkspace(nr, 16), dtype=torch.uint8, device=gpu)

    def load(views):
        buf, offs, lens = gh._pack([v.frame for v in views])
        d_src[:len(buf)].copy_(_t(torch, buf, gpu))
        src_off.copy_(_t(torch, offs, gpu))
        src_len.copy_(_t(torch, lens, gpu))

    def both():
        zl.lz4f.frameIndexBatch(d_src, src_off, src_len, index, idx_off, idx_cap, idx_n, mb, iws)
        zl.lz4f.decompressFrameRangeBatch(d_src, src_off, src_len, index, idx_off, idx_n, d_range, d_dst, dst_off, dst_cap,
                                          skip, res, 16, rws)

    load(a_views)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        both()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        both()
    for views in (b_views, a_views):
        load(views)
        res.fill_(-999)
        skip.fill_(-999)
        d_dst.fill_(0)
        graph.replay()
        torch.cuda.synchronize()
        assert idx_n.cpu().tolist() == [v.idx_n for v in views]
        o, r, sk = d_dst.cpu().numpy(), res.cpu().tolist(), skip.cpu().tolist()
        for i, (f, a, b) in enumerate(ranges):
            S, data = g.full(views[f].frame)
            a1, b1 = min(a, S), min(b, S)
            assert r[i] == b1 - a1 and bytes(o[i * slot + sk[i]:i * slot + sk[i] + r[i]]) == data[a1:b1], (views[f].name, a, b)


def test_host_call_and_one_liners(zl, gpu):
    views = g.small_views() + g.long_views()[:1] + g.long_views()[3:]
    for v in views:
        S, data = g.full(v.frame)
        for a, b in [(0, S), (0, g.BIG), (S, S + 5), (S // 2, S // 2 + 1), (S // 3, S - 1)] + g.small_ranges(v, every_a=False)[::37]:
            assert zl.lz4f.decompressFrameRange(v.frame, a, b) == data[a:b], (v.name, a, b)
    for view, want in g.defect_views():                # the host call builds the index itself: the frame's own status
        n = fr.frame_index(view.frame)[0]
        if n < 0:
            with pytest.raises(zl.Lz4Error) as e:
                zl.lz4f.decompressFrameRange(view.frame, 0, 10)
            assert e.value.code == n, view.name
    five = g.small_views()[0]
    L = zl.lib()
    import ctypes as C
    src = (C.c_uint8 * len(five.frame)).from_buffer_copy(five.frame)
    dst = (C.c_uint8 * 64).from_buffer_copy(b"\xA5" * 64)
    assert L.zlz4f_decompress_frame_range(C.addressof(src), len(five.frame), 290, 330, C.addressof(dst), 39) == g.DST_TOO_SMALL
    assert bytes(dst) == b"\xA5" * 64
    assert L.zlz4f_decompress_frame_range(C.addressof(src), len(five.frame), 290, 330, C.addressof(dst), 40) == 40
    assert bytes(dst) == g.full(five.frame)[1][290:330] + b"\xA5" * 24
    # the one-liners, on corpus frames and on frames this library writes (independent blocks, 64 KiB, four and a bit each)
    inputs = [bytes(dg.text_bytes(300000, 3)), bytes(dg.text_bytes(70001, 4)), b"", bytes(dg.text_bytes(65536, 5))]
    prefs = zl.lz4f.Preferences(block_mode=1, block_checksum=1)
    written = [f for f in zl.lz4f.compressFrames(inputs, prefs, device=gpu)]
    frames = written + [v.frame for v in views] + [g.header_views()[0][0].frame, g.linked_views()[0].frame]
    contents = inputs + [g.full(v.frame)[1] for v in views]
    ix = zl.lz4f.frameIndex(frames, device=gpu)
    assert ix.results[:4] == [5, 2, 0, 1] and ix.results[-2:] == [g.header_views()[0][1], g.FAILED]
    rng = np.random.default_rng(11)
    ranges = []
    for i in range(300):
        f = int(rng.integers(0, len(frames)))
        S = len(contents[f]) if f < len(contents) else 50
        a = int(rng.integers(0, S + 2))
        ranges.append((f, a, a + int(rng.integers(0, min(S + 2, 150000)))))
    ranges += [(0, 65536 * 2 - 1, 65536 * 2 + 1), (0, 0, g.BIG), (len(frames), 0, 1), (1, 5, 4)]
    for align in (0, 64):
        out = zl.lz4f.decompressFrameRanges(ix, ranges, align=align)
        for (f, a, b), got in zip(ranges, out):
            if f >= len(frames) or a > b:
                assert got == g.INVALID_STATE
            elif f >= len(contents):
                assert got == ix.results[f]
            else:
                assert got == contents[f][a:b], (f, a, b)
