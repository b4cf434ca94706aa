"""The file index and file range decoding on the GPU (zlz4f_batch_file_index, zlz4f_batch_decompress_file_range, the host
call and the Python one-liners) against the model tools/pyref/zig_lz4_file_range.py and against the
whole-file decode sliced [a:b].  Corpus and runner: tests/filerangegen.py.  Every range decodes into a slot between guard
bands filled with a pattern: nothing outside the planned slots may change, whatever a range's status."""
import ctypes as C

import numpy as np
import pytest

import filerangegen as g
import legacygen as lg
import multiframegen as mg
import test_gpu_lz4file as t4

pytestmark = pytest.mark.gpu
ff, frg = g.ff, g.frg


def _t(torch, a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _check_index(bufs, got, legacy=True):
    bad = []
    for s, (buf, (n, e)) in enumerate(zip(bufs, got)):
        wn, we = ff.file_index(buf, legacy)
        if n != wn or (wn >= 0 and e != we):
            bad.append("file %d: GPU %r vs model %r" % (s, (n, e[:3]), (wn, we[:3])))
    assert not bad, "%d of %d indexes differ:\n%s" % (len(bad), len(bufs), "\n".join(bad[:10]))


# ----------------------------------------------------------------------------- the index
def test_index_of_every_ordering_against_the_model(zl, gpu):
    bufs = g.orderings()
    ix, got = g.gpu_index(zl, bufs, gpu)
    _check_index(bufs, got)
    assert ix.idx_off.cpu().tolist() == [14 * s for s in range(len(bufs) + 1)]      # the room: 13 blocks plus one
    # the members alone, pairs of them and files without a block
    m = g.members()
    few = list(m.values()) + [a + b for a in m.values() for b in m.values()] + [b"", m["SK"] + m["SK"], g.MAGIC + g.MAGIC]
    _check_index(few, g.gpu_index(zl, few, gpu)[1])
    _check_index(few, g.gpu_index(zl, few, gpu, legacy=False)[1], legacy=False)      # a legacy magic stays FrameTypeUnknown
    assert g.gpu_index(zl, [m["L3"]], gpu, legacy=False)[1] == [(lg.TYPE_UNKNOWN, [])]


def test_index_of_a_one_frame_file_is_the_frame_index(zl, gpu):
    frames = [g.members()[k] for k in ("F", "FC", "FS", "FE")] + [v.frame for v in frg.small_views() + frg.long_views()[:2]]
    frames += [v.frame for v, _ in frg.header_views() if len(v.frame)] + [v.frame for v in frg.linked_views()[:3]]
    frames += [v.frame for v, _ in frg.defect_views()]
    fx = zl.lz4f.frameIndex(frames, device=gpu)
    ix, got = g.gpu_index(zl, frames, gpu)
    assert ix.results == fx.results
    rows, off = fx.index.cpu().tolist(), fx.idx_off.cpu().tolist()
    for s, (n, e) in enumerate(got):
        if n >= 0:
            assert e == [tuple(x) for x in rows[off[s]:off[s] + n + 1]], s
    assert frg.FAILED in ix.results and any(r < 0 and r != frg.FAILED for r in ix.results)


# ----------------------------------------------------------------------------- ranges
def test_ranges_against_the_model(zl, gpu):
    views, items = g.items_of(g.range_views(), lambda v: frg.small_ranges(v, every_a=False))
    assert len(items) > 1500
    g.compare(views, items, g.run(zl, views, items, gpu), g.expect(views, items))
    # the index the GPU builds is the model's, and [0, S) is the whole-file decode
    ix, got = g.gpu_index(zl, [v.buf for v in views], gpu)
    assert got == [(v.idx_n, v.entries) for v in views]
    whole = zl.lz4f.decompressFileRanges(ix, [(s, 0, v.size) for s, v in enumerate(views)])
    assert whole == zl.lz4f.decompressFiles([v.buf for v in views], device=gpu) == [g.content(v.buf) for v in views]


def test_every_range_of_a_tiny_file(zl, gpu):
    views = [v for v in g.tiny_views() if v.name != "tiny_not_legacy"]
    views, items = g.items_of(views, g.all_ranges)
    g.compare(views, items, g.run(zl, views, items, gpu), g.expect(views, items))


def test_the_bound_is_the_members(zl, gpu):
    """70 000 zeros in one legacy block beside a frame of 64 KiB blocks: a range over both has steps of 70 000 and of 64"""
    views, items = g.items_of(g.bound_views(), g.bound_ranges)
    got, want = g.run(zl, views, items, gpu), g.expect(views, items)
    g.compare(views, items, got, want)
    assert all(r >= 0 for r, _, _ in got)
    _check_index([v.buf for v in views], g.gpu_index(zl, [v.buf for v in views], gpu)[1])
    # the same step inside the frame member is above ITS bound
    v = views[0]
    wrong = g.View("step_in_frame", v.buf, (v.idx_n, frg._mod(v.entries, 2, ddec=70000)), False)
    it = [("x", 0, 70000 + 64, 70000 + 64 + 70001, 0, None, None)]
    assert g.run(zl, [wrong], it, gpu)[0][0] == g.expect([wrong], it)[0][0] == g.INVALID_STATE


def test_one_call_of_many_buffers_and_ranges(zl, gpu):
    """72 buffers, more than 200 ranges: a member of 130 blocks (legacy and frame) with a range over all of them, a file of
    70 members -- the fold and the range kernels loop past 64 lanes"""
    edge = g.lane_edge_views()
    more = [g.View("ordering_%d" % k, buf) for k, buf in enumerate(g.orderings()[::600][:69])]
    views = edge + more
    assert len(views) >= 70 and [len(v.members) for v in edge][2] == 70 and edge[0].idx_n == 133 == edge[1].idx_n
    items = []
    for v, view in enumerate(views):
        S, B = view.size, view.bounds
        rs = [(0, S), (B[len(B) // 2], B[len(B) // 2] + 1), (max(0, S - 50), g.BIG)] if v >= 3 else \
            [(0, S), (0, g.BIG), (1, S - 1)] + [(B[k] - 1, B[min(k + 66, len(B) - 1)] + 1) for k in (1, 3, 30)] + frg.small_ranges(view, False)[::97]
        items += [("%s[%d,%d)" % (view.name, a, min(b, 1 << 40)), v, a, b, 0, None, None) for a, b in rs]
    assert len(items) >= 200
    g.compare(views, items, g.run(zl, views, items, gpu), g.expect(views, items))
    ix, got = g.gpu_index(zl, [v.buf for v in views], gpu)
    assert got == [(v.idx_n, v.entries) for v in views]
    n = max(g.item_counts(views, items))
    assert n == 133


# ----------------------------------------------------------------------------- defects
def test_defective_files(zl, gpu):
    """every defect of the whole-file tests: the model's code from the index, the same code from every range on the file,
    the neighbours in the batch unaffected; a linked member with history is DecompressionFailed"""
    good = g.range_views()[0]
    cases = [(name, buf) for name, buf, _ in t4.defect_cases()]
    cases.append(("linked_member_with_history", g.members()["F"] + frg.linked_views()[0].frame + g.members()["L3"]))
    bufs = []
    for _, buf in cases:
        bufs += [good.buf, buf]
    bufs.append(good.buf)
    ix, got = g.gpu_index(zl, bufs, gpu)
    _check_index(bufs, got)
    assert got[2 * len(cases) - 1][0] == g.FAILED
    codes = {n for n, _ in got[1::2]}
    assert {lg.SIZE_WRONG, lg.FAILED, mg.TYPE_UNKNOWN, mg.HEADER_INCOMPLETE} <= codes
    ranges, want = [], []
    for s, (n, e) in enumerate(got):
        S = e[n][1] if n >= 0 else 0
        data = g.content(bufs[s]) if n >= 0 and s % 2 == 0 else None
        for a, b in ((0, 10), (5, g.BIG), (S // 2, S // 2 + 70), (S, S)):
            ranges.append((s, a, b))
            if n < 0:
                want.append(n)
            elif data is not None:
                want.append(data[a:b])
            else:                                      # (a content checksum is set aside: the model's bytes)
                want.append(ff.file_range(bufs[s], a, b)[1])
    assert zl.lz4f.decompressFileRanges(ix, ranges) == want


# ----------------------------------------------------------------------------- wrong indexes
def test_wrong_indexes(zl, gpu):
    views, items, base = [], [], g.wrong_index_views()
    for v, (view, ranges) in enumerate(base):
        views.append(view)
        items += [("%s[%d,%d)" % (view.name, a, min(b, 1 << 40)), v, a, b, 0, None, None) for a, b in ranges]
    views.append(g.View("good_neighbour", base[0][0].buf))
    items.append(("good_neighbour", len(views) - 1, 0, g.BIG, 0, None, None))
    got, want = g.run(zl, views, items, gpu), g.expect(views, items)
    g.compare(views, items, got, want)
    assert all(r in (g.INVALID_STATE, g.FAILED) for r, _, _ in got[:-1]) and got[-1][0] == views[-1].size
    assert {r for r, _, _ in got[:-1]} == {g.INVALID_STATE, g.FAILED}
    # ranges of the same views that do not touch what is wrong still decode
    ok = [("ok", v, 0, 10, 0, None, None) for v, (view, _) in enumerate(base) if "all_pos" not in view.name
          and "pos1" not in view.name and "dec_one_too_large_in_frame" not in view.name]
    got, want = g.run(zl, views, ok, gpu), g.expect(views, ok)
    g.compare(views, ok, got, want)
    assert all(r == 10 for r, _, _ in got)


# ----------------------------------------------------------------------------- capacities and refusals
def test_capacities(zl, gpu):
    import torch
    views = g.range_views()
    v0 = views[0]
    S = v0.size
    items = [("a", 0, 0, S, 0, None, None), ("b", 1, 3, 200, 0, None, None), ("c", 0, 70, 300, 0, None, None)]
    counts = g.item_counts(views, items)
    total = sum(counts)
    # max_items one short: the last range does not fit, the others are unaffected
    got = g.run(zl, views, items, gpu, max_items=total - 1)
    want = g.expect(views, items, max_items=total - 1)
    g.compare(views, items, got, want)
    assert [r >= 0 for r, _, _ in got] == [True, True, False] and got[2][0] == g.INVALID_STATE
    # a slot one byte short; reserved set; a buffer that is none; a > b
    odd = [("short", 0, 5, 100, 0, -1, None), ("fits", 0, 5, 100, 0, 0, None), ("reserved", 0, 5, 100, 1, None, None),
           ("nobuf", 0, 5, 100, 0, None, len(views)), ("a>b", 0, 9, 8, 0, None, None), ("empty", 0, 7, 7, 0, None, None),
           ("behind", 1, views[1].size, g.BIG, 0, None, None), ("b>S", 1, 10, views[1].size + 9, 0, None, None)]
    got = g.run(zl, views, odd, gpu)
    g.compare(views, odd, got, g.expect(views, odd))
    assert [r for r, _, _ in got] == [g.DST_TOO_SMALL, 95, g.INVALID_STATE, g.INVALID_STATE, g.INVALID_STATE, 0, 0,
                                      views[1].size - 10]
    # index capacity one entry short: the last buffer answers DstMaxSizeTooSmall, the others keep their entries
    bufs = [v.buf for v in views]
    sp = zl.lz4f.splitMultiframes(bufs, gpu, legacy=True)
    cap = sp.max_blocks + sp.legacy_blocks + len(bufs)
    assert cap == sum(v.idx_n + 1 for v in views)
    for short in (0, 1):
        index = torch.full((cap + 2, 2), -7, dtype=torch.int64, device=gpu)
        idx_off = torch.full((len(bufs) + 1,), -7, dtype=torch.int64, device=gpu)
        res = torch.full((len(bufs),), -999, dtype=torch.int64, device=gpu)
        zl.lz4f.fileIndexBatch(sp.d_src, sp.src_off, sp.src_len, sp.member, sp.mem_off, sp.result, sp.item_first, sp.item_off,
                               sp.item_len, sp.leg_len, (sp.nitems, sp.max_blocks, sp.nlegacy, sp.legacy_blocks), index,
                               idx_off, res, cap - short)
        want = [v.idx_n for v in views]
        if short:
            want[-1] = g.DST_TOO_SMALL
        assert res.cpu().tolist() == want
        assert idx_off.cpu().tolist() == np.cumsum([0] + [v.idx_n + 1 for v in views]).tolist()      # a failing buffer keeps its room
        rows = index.cpu().tolist()
        used = cap - (views[-1].idx_n + 1 if short else 0)
        assert [tuple(r) for r in rows[:used]] == [e for v in views[:len(views) - short] for e in v.entries]
        assert all(r == [-7, -7] for r in rows[used:]), "entries behind the capacity were written"


@pytest.mark.parametrize("align", [0, 1, 64, 4096])
def test_align(zl, gpu, align):
    views = g.range_views()
    ix, _ = g.gpu_index(zl, [v.buf for v in views], gpu)
    ranges = [(s, a, b) for s, v in enumerate(views) for a, b in ((0, 7), (3, v.size), (v.size // 2, v.size // 2 + 99))]
    want = [g.content(views[s].buf)[a:b] for s, a, b in ranges]
    assert zl.lz4f.decompressFileRanges(ix, ranges, align=align) == want


def test_empty_batches_and_refusals(zl, gpu):
    import torch
    lz4f = zl.lz4f
    assert lz4f.decompressFileRanges(lz4f.fileIndex([], device=gpu), []) == []
    assert lz4f.decompressFilePrefixes([], 5) == []
    ix, got = g.gpu_index(zl, [b"", g.members()["SK"], b""], gpu)         # buffers without a block, two without a member
    assert got == [(0, [(0, 0)])] * 3 and lz4f.decompressFileRanges(ix, [(2, 0, 9), (1, 0, 0)]) == [b"", b""]
    views = g.range_views()[:2]
    sp = lz4f.splitMultiframes([v.buf for v in views], gpu, legacy=True)
    totals = (sp.nitems, sp.max_blocks, sp.nlegacy, sp.legacy_blocks)
    cap = sp.max_blocks + sp.legacy_blocks + 2
    index = torch.zeros((cap, 2), dtype=torch.int64, device=gpu)
    idx_off, res = torch.zeros(3, dtype=torch.int64, device=gpu), torch.zeros(2, dtype=torch.int64, device=gpu)
    ws = torch.empty(lz4f.fileIndexBatchWorkspace(2, totals) + 16, dtype=torch.uint8, device=gpu)
    args = dict(d_src=sp.d_src, src_off=sp.src_off, src_len=sp.src_len, member=sp.member, mem_off=sp.mem_off,
                split_result=sp.result, item_first=sp.item_first, item_off=sp.item_off, item_len=sp.item_len,
                leg_len=sp.leg_len, totals=totals, index=index, idx_off=idx_off, result=res, idx_cap=cap, workspace=ws)
    lz4f.fileIndexBatch(**args)
    assert res.cpu().tolist() == [v.idx_n for v in views]
    odd = torch.zeros(130, dtype=torch.int32, device=gpu)[1:]           # 4 bytes off an 8-byte boundary
    assert odd.data_ptr() % 8 == 4
    for key in ("src_off", "member", "mem_off", "split_result", "item_first", "item_off", "leg_len", "index", "idx_off", "result"):
        for bad in (None, odd):
            with pytest.raises(zl.Lz4Error) as e:
                lz4f.fileIndexBatch(**dict(args, **{key: bad}))
            assert e.value.code == g.INVALID_STATE, key
    for bad_ws in (ws[:lz4f.fileIndexBatchWorkspace(2, totals) - 1], ws[8:]):
        with pytest.raises(zl.Lz4Error) as e:
            lz4f.fileIndexBatch(**dict(args, workspace=bad_ws))
        assert e.value.code == g.INVALID_STATE
    # the range call
    d_range = _t(torch, lz4f.packRanges([(0, 0, 50), (1, 10, 90)]).view(np.int64), gpu)
    dst_off, dst_cap, skip, rres, tot = (torch.zeros(2, dtype=torch.int64, device=gpu) for _ in range(5))
    lz4f.planFrameRanges(index, idx_off, res, d_range, dst_off, dst_cap, tot)
    arena, items = tot.cpu().tolist()
    d_dst = torch.zeros(arena, dtype=torch.uint8, device=gpu)
    rws = torch.empty(lz4f.decompressFileRangeBatchWorkspace(2, items) + 16, dtype=torch.uint8, device=gpu)
    rargs = dict(d_src=sp.d_src, src_off=sp.src_off, src_len=sp.src_len, index=index, idx_off=idx_off, idx_n=res,
                 member=sp.member, mem_off=sp.mem_off, split_result=sp.result, ranges=d_range, d_dst=d_dst, dst_off=dst_off,
                 dst_cap=dst_cap, skip=skip, result=rres, max_items=items, workspace=rws)
    lz4f.decompressFileRangeBatch(**rargs)
    assert rres.cpu().tolist() == [50, 80]
    for key in ("src_len", "index", "idx_off", "member", "mem_off", "split_result", "dst_off", "dst_cap", "skip", "result"):
        for bad in (None, odd):
            with pytest.raises(zl.Lz4Error) as e:
                lz4f.decompressFileRangeBatch(**dict(rargs, **{key: bad}))
            assert e.value.code == g.INVALID_STATE, key
    with pytest.raises(zl.Lz4Error) as e:
        lz4f.decompressFileRangeBatch(**dict(rargs, workspace=rws[8:]))
    assert e.value.code == g.INVALID_STATE
    assert rres.cpu().tolist() == [50, 80]              # a refused call launches nothing


def test_host_call_and_one_liners(zl, gpu):
    lz4f, L = zl.lz4f, zl.lib()
    for v in g.range_views() + g.tiny_views()[:4] + g.lane_edge_views()[2:]:
        data, S = g.content(v.buf), v.size
        for a, b in [(0, S), (0, g.BIG), (S, S + 5), (S // 2, S // 2 + 1), (S // 3, S - 1)] + frg.small_ranges(v, False)[::211]:
            assert lz4f.decompressFileRange(v.buf, a, b) == data[a:b], (v.name, a, b)
    assert lz4f.decompressFileRange(b"", 0, 10) == b""
    one = g.range_views()[0]
    with pytest.raises(zl.Lz4Error) as e:              # without the flag a legacy member is FrameTypeUnknown
        lz4f.decompressFileRange(one.buf, 0, 10, legacy=False)
    assert e.value.code == lg.TYPE_UNKNOWN
    assert lz4f.decompressFileRange(g.members()["F"] + g.members()["FC"], 100, 300, legacy=False) == \
        g.content(g.members()["F"] + g.members()["FC"])[100:300]
    for name, buf, _ in t4.defect_cases()[::3]:
        n = ff.file_index(buf)[0]
        if n < 0:
            with pytest.raises(zl.Lz4Error) as e:
                lz4f.decompressFileRange(buf, 0, 10)
            assert e.value.code == n, name
    src = (C.c_uint8 * len(one.buf)).from_buffer_copy(one.buf)
    dst = (C.c_uint8 * 64).from_buffer_copy(b"\xA5" * 64)
    assert L.zlz4f_decompress_file_range(C.addressof(src), len(one.buf), 160, 200, C.addressof(dst), 39, 1) == g.DST_TOO_SMALL
    assert bytes(dst) == b"\xA5" * 64
    assert L.zlz4f_decompress_file_range(C.addressof(src), len(one.buf), 160, 200, C.addressof(dst), 40, 1) == 40
    assert bytes(dst) == g.content(one.buf)[160:200] + b"\xA5" * 24
    # the one-liners: prefixes are the ranges [0, n); files of this library's frames and of the whole-file corpus
    p = t4.parts()
    files = [p.l64 + p.a.frame, p.a.frame + p.l70 + p.l3, p.l4 + p.b.frame + g.MAGIC, b"", p.sk + p.l3 + b"\x07"]
    whole = lz4f.decompressFiles(files, device=gpu)
    assert whole[4] == lg.SIZE_WRONG
    for n in (0, 1, 4096, 70000, 1 << 40):
        assert lz4f.decompressFilePrefixes(files, n, device=gpu) == [w if isinstance(w, int) else w[:n] for w in whole]
    assert lz4f.decompressFilePrefixes(files[:2], [5, 150001], device=gpu) == [whole[0][:5], whole[1][:150001]]
    ix = lz4f.fileIndex(files, device=gpu)
    tail = [(s, max(0, len(w) - 4096), len(w)) for s, w in enumerate(whole[:4])]
    assert lz4f.decompressFileRanges(ix, tail) == [w[-4096:] if len(w) else b"" for w in whole[:4]]
    assert lz4f.decompressFileRanges(ix, [(0, 149990, 150010)]) == [whole[0][149990:150010]]           # legacy -> frame


def test_graph_capture_and_replay(zl, gpu):
    """index + plan + range in one captured graph on a single stream, replayed over other files of the same split totals"""
    import torch
    lz4f = zl.lz4f
    a_files = [g.join("F", "SK", "L3", "FC"), g.join("LZ", "FS", "LM", "FE")]
    b_files = [g.join("L3", "FC", "SK", "F"), g.join("FE", "LM", "FS", "LZ")]
    ranges = [(0, 5, 400), (1, 30, 250), (0, 0, g.BIG), (1, 100, 101), (0, 160, 180)]
    nr = len(ranges)
    sp = lz4f.splitMultiframes(a_files, gpu, legacy=True)
    spb = lz4f.splitMultiframes(b_files, gpu, legacy=True)
    totals = (sp.nitems, sp.max_blocks, sp.nlegacy, sp.legacy_blocks)
    assert totals == (spb.nitems, spb.max_blocks, spb.nlegacy, spb.legacy_blocks) and sp.d_src.numel() == spb.d_src.numel()
    cap = sp.max_blocks + sp.legacy_blocks + 2
    index = torch.zeros((cap, 2), dtype=torch.int64, device=gpu)
    idx_off, idx_n = torch.zeros(3, dtype=torch.int64, device=gpu), torch.zeros(2, dtype=torch.int64, device=gpu)
    d_range = _t(torch, lz4f.packRanges(ranges).view(np.int64), gpu)
    slot, max_items = 1024, 64
    d_dst = torch.zeros(nr * slot, dtype=torch.uint8, device=gpu)
    dst_off = _t(torch, np.arange(nr, dtype=np.int64) * slot, gpu)
    dst_cap = torch.full((nr,), slot, dtype=torch.int64, device=gpu)
    plan_off, plan_cap, plan_tot = (torch.zeros(n, dtype=torch.int64, device=gpu) for n in (nr, nr, 2))
    skip, res = torch.zeros(nr, dtype=torch.int64, device=gpu), torch.zeros(nr, dtype=torch.int64, device=gpu)
    iws = torch.empty(lz4f.fileIndexBatchWorkspace(2, totals), dtype=torch.uint8, device=gpu)
    rws = torch.empty(lz4f.decompressFileRangeBatchWorkspace(nr, max_items), dtype=torch.uint8, device=gpu)
    fields = ("d_src", "src_off", "src_len", "member", "item_first", "item_off", "item_len", "leg_len", "result")

    def load(other):
        for f in fields:
            getattr(sp, f).copy_(getattr(other, f))

    keep = lz4f.splitMultiframes(a_files, gpu, legacy=True)

    def all_three():
        lz4f.fileIndexBatch(sp.d_src, sp.src_off, sp.src_len, sp.member, sp.mem_off, sp.result, sp.item_first, sp.item_off,
                            sp.item_len, sp.leg_len, totals, index, idx_off, idx_n, cap, iws)
        lz4f.planFrameRanges(index, idx_off, idx_n, d_range, plan_off, plan_cap, plan_tot)
        lz4f.decompressFileRangeBatch(sp.d_src, sp.src_off, sp.src_len, index, idx_off, idx_n, sp.member, sp.mem_off, sp.result,
                                      d_range, d_dst, dst_off, dst_cap, skip, res, max_items, rws)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        all_three()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        all_three()
    for other, files in ((spb, b_files), (keep, a_files)):
        load(other)
        res.fill_(-999)
        skip.fill_(-999)
        d_dst.fill_(0)
        graph.replay()
        torch.cuda.synchronize()
        assert idx_n.cpu().tolist() == [ff.file_index(f)[0] for f in files]
        o, r, sk = d_dst.cpu().numpy(), res.cpu().tolist(), skip.cpu().tolist()
        assert plan_tot.cpu().tolist()[1] == sum(ff.plan_range(*ff.file_index(files[f])[::-1], a, b)[1] for f, a, b in ranges)
        for i, (f, a, b) in enumerate(ranges):
            data = g.content(files[f])
            assert r[i] == len(data[a:b]) and bytes(o[i * slot + sk[i]:i * slot + sk[i] + r[i]]) == data[a:b], (f, a, b)
