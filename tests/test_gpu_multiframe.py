"""Multiframe buffers on the GPU (zlz4f_batch_multiframe_split / _plan / _finish around the unchanged frame size query and
frame decode, the host calls and the Python one-liners) against the model of
tests/multiframegen.py: member tables, per-item and per-buffer results, bytes.  Every run decodes into an arena between
guard bands filled with a pattern: nothing outside the planned slots may change, whatever a buffer's result."""
import ctypes as C
import random

import numpy as np
import pytest

import multiframegen as g

pytestmark = pytest.mark.gpu
FILL, BAND = 0xA5, 512


class Run:
    pass


def run(zl, dev, buffers, flags=0, align=0, mem_cap=None, decode_max_blocks=None):
    """split (count, record), size query, plan, decode, finish through the raw tensor wrappers -> Run with everything on
    the host; checks the count against the record, the plan's layout and the guard bands"""
    import torch
    lz4f = zl.lz4f
    nbuf = len(buffers)
    r = Run()
    d_src, src_off, src_len = zl._stage(buffers, dev)

    def i64(n, fill=-999):
        return torch.full((max(1, n),), fill, dtype=torch.int64, device=dev)[:n]

    count, totals = i64(nbuf), i64(2)
    lz4f.multiframeSplitBatch(d_src, src_off, src_len, count, totals)
    r.count, (r.nitems, r.max_blocks) = count.cpu().tolist(), totals.cpu().tolist()
    assert r.nitems == sum(r.count)
    caps = list(r.count) if mem_cap is None else list(mem_cap)
    mem_off = np.cumsum([0] + [c + 1 for c in caps]).astype(np.int64)            # one spare entry behind every buffer
    member = torch.full((int(mem_off[-1]) + 1, 3), -7, dtype=torch.int64, device=dev)
    count2, totals2, item_first, split_result = i64(nbuf), i64(2), i64(nbuf + 1), i64(nbuf)
    item_off, item_len = i64(r.nitems), i64(r.nitems)
    t_mem_off = torch.from_numpy(mem_off[:nbuf].copy()).to(dev)
    lz4f.multiframeSplitBatch(d_src, src_off, src_len, count2, totals2, member, t_mem_off,
                              torch.tensor(caps, dtype=torch.int64, device=dev), item_first, item_off, item_len, split_result)
    assert count2.cpu().tolist() == r.count and totals2.cpu().tolist() == [r.nitems, r.max_blocks], "count mode vs record mode"
    r.item_first = item_first.cpu().tolist()
    assert r.item_first == np.cumsum([0] + r.count).tolist()
    r.split_result = split_result.cpu().tolist()
    rows = member.cpu().numpy()
    r.members = []
    for s in range(nbuf):
        lo, used = int(mem_off[s]), max(r.split_result[s], 0)
        r.members.append([(int(p), int(n), int(k) & 0xFF, (int(k) >> 8) & 15) for p, n, k in rows[lo:lo + used]])
        assert all((int(k) >> 32) == s for _, _, k in rows[lo:lo + used]), "buf"
        assert (rows[lo + used:int(mem_off[s + 1])] == -7).all(), "buffer %d: entries behind the result were written" % s
    r.item_off, r.item_len = item_off.cpu().tolist(), item_len.cpu().tolist()

    size, dst_off, dst_cap, item_result = i64(r.nitems), i64(r.nitems), i64(r.nitems), i64(r.nitems)
    out_off, out_size, result, ptotals = i64(nbuf), i64(nbuf), i64(nbuf), i64(2)
    if r.nitems:
        lz4f.frameDecompressedSizeBatch(d_src, item_off, item_len, size, max_blocks=r.max_blocks, flags=flags)
    lz4f.multiframePlanBatch(size, item_first, dst_off, dst_cap, out_off, out_size, ptotals, align)
    r.size, r.dst_off, r.dst_cap = size.cpu().tolist(), dst_off.cpu().tolist(), dst_cap.cpu().tolist()
    r.out_off, r.out_size, (r.arena, r.decoded) = out_off.cpu().tolist(), out_size.cpu().tolist(), ptotals.cpu().tolist()
    a, pos = max(align, 1), 0
    for s in range(nbuf):                             # the plan: buffers aligned, a buffer's items one run of bytes
        assert r.out_off[s] == pos and pos % a == 0
        run_ = pos
        for i in range(r.item_first[s], r.item_first[s + 1]):
            assert (r.dst_off[i], r.dst_cap[i]) == (run_, max(r.size[i], 0))
            run_ += r.dst_cap[i]
        assert r.out_size[s] == run_ - pos
        pos += (r.out_size[s] + a - 1) // a * a
    assert (r.arena, r.decoded) == (pos, sum(r.out_size))
    whole = torch.full((r.arena + 2 * BAND,), FILL, dtype=torch.uint8, device=dev)
    d_dst = whole[BAND:]
    if r.nitems:
        mb = r.max_blocks if decode_max_blocks is None else decode_max_blocks
        lz4f.decompressFrameBatch(d_src, item_off, item_len, d_dst, dst_off, dst_cap, item_result, max_blocks=mb, flags=flags)
    if nbuf:
        lz4f.multiframeFinishBatch(member, t_mem_off, split_result, item_first, size, item_result, result)
    torch.cuda.synchronize()
    r.item_result, r.result = item_result.cpu().tolist(), result.cpu().tolist()
    host = whole.cpu().numpy()
    untouched = np.ones(host.shape, dtype=bool)
    r.data = []
    for s in range(nbuf):
        lo = BAND + r.out_off[s]
        untouched[lo:lo + r.out_size[s]] = False
        r.data.append(host[lo:lo + r.result[s]].tobytes() if r.result[s] >= 0 else None)
    assert (host[untouched] == FILL).all(), "bytes outside the planned slots changed"
    return r


def check(r, buffers, flags=0):
    """every buffer of a run against the model: table, item results, result, bytes"""
    for s, buf in enumerate(buffers):
        want_result, want_data, want_items = g.expected(buf, flags)
        assert r.split_result[s] == r.count[s] == len(want_items), s
        assert r.members[s] == g.table(buf), s
        lo = r.item_first[s]
        for k, (m, w) in enumerate(zip(g.split(buf), want_items)):
            assert r.item_off[lo + k] == sum(len(b) for b in buffers[:s]) + m.pos
            if w is None:
                assert (r.item_len[lo + k], r.item_result[lo + k], r.dst_cap[lo + k]) == (0, g.HEADER_INCOMPLETE, 0), (s, k)
            else:
                got = r.size[lo + k] if r.size[lo + k] < 0 else r.item_result[lo + k]
                assert (r.item_len[lo + k], got) == (m.len, w), (s, k)
        assert r.result[s] == want_result, (s, r.result[s], want_result)
        if want_data is not None:
            assert r.data[s] == want_data and r.out_size[s] == want_result, s


def _torn(c):
    """the frame without its end mark / without its content checksum word"""
    out = [c.frame[:-4]]
    if c.cc:
        out.append(c.frame[:-8])
    return out


@pytest.mark.parametrize("flags", [0, g.DECODE_LINKED])
def test_one_frame_alone_answers_what_the_frame_call_answers(zl, gpu, flags):
    frames = [c.frame for c in g.corpus()] + [t for c in g.corpus() for t in _torn(c)]
    want = zl.lz4f.decompressFrames(frames, flags=flags)
    got = zl.lz4f.decompressMultiframes(frames, flags=flags)
    assert got == want
    assert g.SIZE_WRONG in want and sum(isinstance(w, bytes) for w in want) >= len(g.corpus())
    r = run(zl, gpu, frames, flags)
    assert [d if d is not None else c for d, c in zip(r.data, r.result)] == want
    assert r.members == [[(0, len(f), g.FRAME, 0)] for f in frames]
    check(r, frames, flags)


def test_concatenations(zl, gpu):
    c = g.corpus()
    rnd = random.Random(5)
    buffers = [b"".join(x.frame for x in rnd.sample(c, k)) for k in (2, 3, 5) for _ in range(4)]
    buffers.append(b"".join(x.frame for x in g.few()))
    singles = {x.frame: x.content for x in c}
    r = run(zl, gpu, buffers)
    check(r, buffers)
    for s, buf in enumerate(buffers):
        parts = [singles[buf[p:p + n]] for p, n, _, _ in r.members[s]]
        assert r.data[s] == b"".join(parts) and r.result[s] == sum(map(len, parts))
    assert zl.lz4f.multiframeMembers(buffers) == [g.table(b) for b in buffers]
    assert zl.lz4f.decompressMultiframes(buffers) == r.data


def test_skippable_frames(zl, gpu):
    a, b = g.pick("text65537_bc1_cc1_cs0", "text1_bc0_cc0_cs1")
    pay = {n: bytes(g.dg.random_bytes(n, n + 1)) for n in (0, 1, 65536, 70000)}
    buffers = [g.skippable(k, pay[1]) + a.frame for k in range(16)]
    for n, p in pay.items():
        sk = g.skippable(n & 15, p)
        buffers += [sk + a.frame, a.frame + sk + b.frame, a.frame + sk, a.frame + sk + g.skippable(3, pay[1]) + b.frame, sk,
                    sk + sk]
    buffers.append(b"")
    r = run(zl, gpu, buffers)
    check(r, buffers)
    assert [m[0][3] for m in r.members[:16]] == list(range(16))
    for s, buf in enumerate(buffers):
        frames = [buf[p:p + n] for p, n, k, _ in r.members[s] if k == g.FRAME]
        assert r.data[s] == b"".join({a.frame: a.content, b.frame: b.content}[f] for f in frames), s
    assert r.result[-1] == 0 and r.count[-1] == 0 and r.result[-2] == 0


def test_defects(zl, gpu):
    cases = g.defects()
    buffers = [buf for _, buf, _, _ in cases]
    r = run(zl, gpu, buffers)
    check(r, buffers)
    for s, (name, buf, code, front) in enumerate(cases):
        assert r.result[s] == code, name
        lo = r.item_first[s]
        for k in range(front):                        # the members in front of the defect can be salvaged
            assert r.item_result[lo + k] >= 0 or r.members[s][k][2] == g.SKIPPABLE, name
        assert r.count[s] > front
    got = zl.lz4f.decompressMultiframes(buffers)
    assert got == [code for _, _, code, _ in cases]


def test_linked_members_need_the_flag(zl, gpu):
    a, b = g.pick("text65537_bc1_cc1_cs0", "text1_bc0_cc0_cs1")
    (l0, d0), (l1, d1) = g.linked()[:2]
    buffers = [l0, a.frame + l0 + b.frame, l1 + g.skippable(1, b"meta") + l0, b.frame + a.frame]
    r = run(zl, gpu, buffers, g.DECODE_LINKED)
    check(r, buffers, g.DECODE_LINKED)
    assert r.data == [d0, a.content + d0 + b.content, d1 + d0, b.content + a.content]
    r = run(zl, gpu, buffers, 0)
    check(r, buffers, 0)
    assert r.result == [g.FAILED, g.FAILED, g.FAILED, len(b.content + a.content)]


def _mixed(nbuf, seed):
    rnd = random.Random(seed)
    small = g.pick("text0_bc0_cc0_cs0", "text1_bc1_cc1_cs1", "text1_bc0_cc0_cs0", "text0_bc1_cc1_cs1", "text65537_bc1_cc0_cs0")
    parts = [x.frame for x in small] + [g.skippable(9, b""), g.skippable(0, b"0123456789")]
    tails = [b"\x01\x02", g.skippable(4)[:6], g.skippable(4, b"abc")[:-1], b"\x03" * 9, small[1].frame[:-2]]
    out = []
    for _ in range(nbuf):
        buf = b"".join(rnd.choice(parts) for _ in range(rnd.randrange(0, 7)))
        if rnd.random() < 0.2 and len(g.split(buf)) < 6:
            buf += rnd.choice(tails)
        out.append(buf)
    return out


@pytest.mark.parametrize("align", [0, 1, 64, 4096])
def test_batch_of_300_mixed_buffers(zl, gpu, align):
    buffers = _mixed(300, 11)
    counts = {len(g.split(b)) for b in buffers}
    assert counts == set(range(7))
    r = run(zl, gpu, buffers, align=align)
    check(r, buffers)
    assert {c for c in r.result if c < 0} >= {g.HEADER_INCOMPLETE, g.SIZE_WRONG, g.TYPE_UNKNOWN}
    if align == 64:
        assert zl.lz4f.decompressMultiframes(buffers, align=64) == [d if d is not None else c for d, c in zip(r.data, r.result)]


def test_items_and_buffers_beyond_one_scan_block(zl, gpu):
    tiny, empty = g.pick("text1_bc1_cc1_cs1", "text0_bc0_cc0_cs0")
    buffers = [tiny.frame] * 1100
    r = run(zl, gpu, buffers, align=64)
    assert r.result == [1] * 1100 and r.data == [tiny.content] * 1100 and r.out_off == [64 * s for s in range(1100)]
    assert r.members == [[(0, len(tiny.frame), g.FRAME, 0)]] * 1100 and r.max_blocks == 1100
    buffers = [tiny.frame, empty.frame * 1100, tiny.frame * 3, b""]
    r = run(zl, gpu, buffers, align=64)
    assert r.count == [1, 1100, 3, 0] and r.result == [1, 0, 3, 0] and r.data[2] == tiny.content * 3
    assert r.members[1] == [(11 * k, 11, g.FRAME, 0) for k in range(1100)] and r.item_result[1:1101] == [0] * 1100
    assert r.item_first == [0, 1, 1101, 1104, 1104] and r.max_blocks == 4


def test_tables_too_small(zl, gpu):
    f = g.few()
    buffers = [f[1].frame + f[4].frame, f[0].frame + g.skippable(2, b"xy") + f[5].frame, f[6].frame]
    full = run(zl, gpu, buffers)
    check(full, buffers)
    # the member table of buffer 1 one entry short: DstMaxSizeTooSmall for that buffer alone, nothing written, its items
    # keep their room with length 0
    r = run(zl, gpu, buffers, mem_cap=[2, 2, 1])
    assert r.split_result == [2, g.DST_TOO_SMALL, 1] and r.members[1] == [] and r.count == [2, 3, 1]
    assert r.item_len[2:5] == [0, 0, 0] and r.item_first == full.item_first
    assert r.result == [full.result[0], g.DST_TOO_SMALL, full.result[2]]
    assert (r.data[0], r.data[2]) == (full.data[0], full.data[2]) and r.out_size[1] == 0
    # max_blocks one too small in the decode: the frame that no longer fits answers InvalidState and decides its buffer
    assert full.max_blocks == 1 + 2 + 0 + 4 + 4
    r = run(zl, gpu, buffers, decode_max_blocks=full.max_blocks - 1)
    assert r.result == [full.result[0], full.result[1], g.INVALID_STATE] and r.item_result[-1] == g.INVALID_STATE
    assert r.data[:2] == full.data[:2]


def test_refusals_and_the_raw_c_calls(zl, gpu):
    """the five C calls on raw device pointers, then null and misaligned arrays, nbuf == 0, unknown flag bits"""
    import torch
    L = zl.lib()
    f = g.few()
    buffers = [f[1].frame + g.skippable(6, b"abc") + f[4].frame, f[3].frame]
    want = [g.expected(b) for b in buffers]
    d_src, src_off, src_len = zl._stage(buffers, gpu)
    st = zl._stream()
    p = lambda t: C.c_void_p(t.data_ptr())           # noqa: E731
    i64 = lambda n: torch.zeros(n, dtype=torch.int64, device=gpu)   # noqa: E731
    count, totals = i64(2), i64(2)
    assert L.zlz4f_batch_multiframe_split(st, p(d_src), p(src_off), p(src_len), 2, p(count), p(totals), None, None, None, None,
                                          None, None, None) == 0
    assert count.tolist() == [3, 1] and totals.tolist() == [4, 4]
    member, mem_off, mem_cap = torch.zeros((4, 3), dtype=torch.int64, device=gpu), i64(2), i64(2)
    mem_off[1], mem_cap[0], mem_cap[1] = 3, 3, 1
    item_first, item_off, item_len, sres = i64(3), i64(4), i64(4), i64(2)
    rec = (st, p(d_src), p(src_off), p(src_len), 2, p(count), p(totals), p(member), p(mem_off), p(mem_cap), p(item_first),
           p(item_off), p(item_len), p(sres))
    assert L.zlz4f_batch_multiframe_split(*rec) == 0
    assert sres.tolist() == [3, 1] and item_first.tolist() == [0, 3, 4]
    ws = torch.empty(max(16, L.zlz4f_batch_decompress_frame_workspace_ex(4, 4, 0),
                         L.zlz4f_batch_frame_decompressed_size_workspace_ex(4, 4, 0)), dtype=torch.uint8, device=gpu)
    size, dst_off, dst_cap, ires, out_off, out_size, res, pt = i64(4), i64(4), i64(4), i64(4), i64(2), i64(2), i64(2), i64(2)
    assert L.zlz4f_batch_frame_decompressed_size_ex(st, p(d_src), p(item_off), p(item_len), p(size), 4, 4, 0, p(ws), ws.numel()) == 0
    plan = (st, p(size), p(item_first), 2, 0, p(dst_off), p(dst_cap), p(out_off), p(out_size), p(pt))
    assert L.zlz4f_batch_multiframe_plan(*plan) == 0
    assert pt.tolist() == [want[0][0] + want[1][0]] * 2
    d_dst = torch.zeros(pt.tolist()[0], dtype=torch.uint8, device=gpu)
    assert L.zlz4f_batch_decompress_frame_ex(st, p(d_src), p(item_off), p(item_len), p(d_dst), p(dst_off), p(dst_cap), p(ires),
                                             4, 4, 0, p(ws), ws.numel()) == 0
    fin = (st, p(member), p(mem_off), p(sres), p(item_first), p(size), p(ires), 2, p(res))
    assert L.zlz4f_batch_multiframe_finish(*fin) == 0
    assert res.tolist() == [w[0] for w in want] and d_dst.cpu().numpy().tobytes() == want[0][1] + want[1][1]
    # the size query alone folds to the same results
    assert L.zlz4f_batch_multiframe_finish(st, p(member), p(mem_off), p(sres), p(item_first), p(size), p(size), 2, p(res)) == 0
    assert res.tolist() == [w[0] for w in want]

    def refused(fn, args, which, keep=()):
        for k in which:
            if k in keep:
                continue
            bad = list(args)
            bad[k] = None
            assert fn(*bad) == g.INVALID_STATE, (fn.__name__, k, "null")
            bad[k] = C.c_void_p(args[k].value + 4)
            assert fn(*bad) == g.INVALID_STATE, (fn.__name__, k, "misaligned")

    before = [t.clone() for t in (count, totals, member, item_first, item_off, item_len, sres, dst_off, dst_cap, out_off, res)]
    refused(L.zlz4f_batch_multiframe_split, rec, (2, 3, 5, 6, 8, 9, 10, 11, 12, 13))
    assert L.zlz4f_batch_multiframe_split(*(rec[:1] + (None,) + rec[2:])) == g.INVALID_STATE           # d_src
    bad = list(rec)
    bad[7] = C.c_void_p(rec[7].value + 4)
    assert L.zlz4f_batch_multiframe_split(*bad) == g.INVALID_STATE                                     # d_member misaligned
    refused(L.zlz4f_batch_multiframe_plan, plan, (1, 2, 5, 6, 7, 8, 9))
    for align in (3, 8192, 48):
        assert L.zlz4f_batch_multiframe_plan(*(plan[:4] + (align,) + plan[5:])) == g.INVALID_STATE
    refused(L.zlz4f_batch_multiframe_finish, fin, (1, 2, 3, 4, 5, 6, 8))
    torch.cuda.synchronize()
    after = (count, totals, member, item_first, item_off, item_len, sres, dst_off, dst_cap, out_off, res)
    assert all(torch.equal(x, y) for x, y in zip(before, after)), "a refused call wrote"
    # nbuf == 0: 0, two zeros
    totals.fill_(7)
    pt.fill_(7)
    assert L.zlz4f_batch_multiframe_split(st, None, None, None, 0, None, p(totals), None, None, None, None, None, None, None) == 0
    assert L.zlz4f_batch_multiframe_plan(st, None, None, 0, 0, None, None, None, None, p(pt)) == 0
    assert L.zlz4f_batch_multiframe_finish(st, None, None, None, None, None, None, 0, None) == 0
    assert totals.tolist() == [0, 0] and pt.tolist() == [0, 0]
    assert zl.lz4f.decompressMultiframes([]) == [] and zl.lz4f.multiframeMembers([]) == []
    # unknown flag bits
    with pytest.raises(zl.Lz4Error) as e:
        zl.lz4f.decompressMultiframes(buffers, flags=2)
    assert e.value.code == g.PARAMETER_INVALID


def test_host_single_calls(zl, gpu):
    a, b = g.pick("text65537_bc1_cc1_cs0", "text200000_bc0_cc0_cs1")
    (l0, d0) = g.linked()[0]
    three = a.frame + g.skippable(11, b"seek table") + b.frame + g.few()[0].frame
    assert zl.lz4f.multiframeDecompressedSize(three) == len(a.content + b.content)
    assert zl.lz4f.decompressMultiframe(three) == a.content + b.content
    assert zl.lz4f.decompressMultiframe(b"") == b"" and zl.lz4f.multiframeDecompressedSize(g.skippable(1, b"x")) == 0
    assert zl.lz4f.decompressMultiframe(a.frame + l0, flags=g.DECODE_LINKED) == a.content + d0
    for buf, code in ((a.frame + l0, g.FAILED), (a.frame + g.flip(a.frame, len(a.frame) - 9) + b.frame, g.BLOCK_CHECKSUM),
                      (a.frame + b"\x01\x02\x03", g.HEADER_INCOMPLETE), (g.skippable(1, b"abc")[:-1], g.SIZE_WRONG)):
        for call in (zl.lz4f.multiframeDecompressedSize, zl.lz4f.decompressMultiframe):
            with pytest.raises(zl.Lz4Error) as e:
                call(buf)
            assert e.value.code == code
    # a flipped content checksum: the size query sets it aside, the decode reports it
    bad = a.frame + g.flip(a.frame, len(a.frame) - 1)
    assert zl.lz4f.multiframeDecompressedSize(bad) == 2 * len(a.content)
    with pytest.raises(zl.Lz4Error) as e:
        zl.lz4f.decompressMultiframe(bad)
    assert e.value.code == g.CONTENT_CHECKSUM
    with pytest.raises(zl.Lz4Error) as e:
        zl.lz4f.decompressMultiframe(three, dst_cap=len(a.content + b.content) - 1)
    assert e.value.code == g.DST_TOO_SMALL
