"""Whole .lz4 files on the GPU: legacy members in multiframe buffers (zlz4f_batch_multiframe_split_ex and
zlz4f_batch_multiframe_select around the unchanged frame and legacy frame calls, the _ex host calls and the Python
one-liners) against the model of tests/lz4filegen.py: member tables, totals, per-item and
per-buffer results, bytes.  Every run decodes into an arena between guard bands filled with a pattern: nothing outside the
planned slots may change, whatever a buffer's result."""
import ctypes as C
import functools
import itertools
import random

import numpy as np
import pytest

import legacygen as lg
import lz4filegen as g
import multiframegen as mg

pytestmark = pytest.mark.gpu
FILL, BAND = 0xA5, 512
MAGIC = lg.le32(lg.MAGIC)


class Run:
    pass


def run(zl, dev, buffers, flags=0, align=0, mem_cap=None, split_flags=g.SPLIT_LEGACY, legacy_decode_blocks=None):
    """the sequence of include/zlz4_amd.h through the raw tensor wrappers -> Run with everything on the host; checks the
    count against the record, the two length arrays against each other, the plan's layout and the guard bands"""
    import torch
    lz4f = zl.lz4f
    nbuf = len(buffers)
    r = Run()
    d_src, src_off, src_len = zl._stage(buffers, dev)

    def i64(n, fill=-999):
        return torch.full((max(1, n),), fill, dtype=torch.int64, device=dev)[:n]

    count, totals = i64(nbuf), i64(4)
    lz4f.multiframeSplitBatchEx(d_src, src_off, src_len, count, totals, split_flags=split_flags)
    r.count, r.totals = count.cpu().tolist(), totals.cpu().tolist()
    r.nitems, r.max_blocks, r.nlegacy, r.legacy_blocks = r.totals
    assert r.nitems == sum(r.count)
    caps = list(r.count) if mem_cap is None else list(mem_cap)
    mem_off = np.cumsum([0] + [c + 1 for c in caps]).astype(np.int64)            # one spare entry behind every buffer
    member = torch.full((int(mem_off[-1]) + 1, 3), -7, dtype=torch.int64, device=dev)
    count2, totals2, item_first, split_result = i64(nbuf), i64(4), i64(nbuf + 1), i64(nbuf)
    item_off, item_len, leg_len = i64(r.nitems), i64(r.nitems), i64(r.nitems)
    t_mem_off = torch.from_numpy(mem_off[:nbuf].copy()).to(dev)
    t_mem_cap = torch.tensor(caps, dtype=torch.int64, device=dev)
    lz4f.multiframeSplitBatchEx(d_src, src_off, src_len, count2, totals2, member, t_mem_off, t_mem_cap, item_first, item_off,
                                item_len, split_result, split_flags, leg_len)
    assert count2.cpu().tolist() == r.count and totals2.cpu().tolist() == r.totals, "count mode vs record mode"
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
    r.item_off, r.item_len, r.leg_len = item_off.cpu().tolist(), item_len.cpu().tolist(), leg_len.cpu().tolist()
    assert all(a == 0 or b == 0 for a, b in zip(r.item_len, r.leg_len)), "an item belongs to one family"
    r.raw = dict(count=count2, totals=totals2, member=member, item_first=item_first, item_off=item_off, item_len=item_len,
                 result=split_result, leg_len=leg_len, src=(d_src, src_off, src_len), mem=(t_mem_off, t_mem_cap))

    size, dst_off, dst_cap, item_result = i64(r.nitems), i64(r.nitems), i64(r.nitems), i64(r.nitems)
    from_legacy, consumed = i64(r.nitems), i64(r.nitems)
    out_off, out_size, result, ptotals = i64(nbuf), i64(nbuf), i64(nbuf), i64(2)
    if r.nitems:
        lz4f.frameDecompressedSizeBatch(d_src, item_off, item_len, size, max_blocks=r.max_blocks, flags=flags)
    if r.nlegacy:
        lz4f.legacyFrameDecompressedSizeBatch(d_src, item_off, leg_len, from_legacy, None, r.legacy_blocks)
        merged = i64(r.nitems)                        # (the sizes into an array of their own, the results in place)
        lz4f.multiframeSelectBatch(member, t_mem_off, split_result, item_first, size, from_legacy, merged)
        size = merged
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
        lz4f.decompressFrameBatch(d_src, item_off, item_len, d_dst, dst_off, dst_cap, item_result, max_blocks=r.max_blocks,
                                  flags=flags)
    if r.nlegacy:
        mb = r.legacy_blocks if legacy_decode_blocks is None else legacy_decode_blocks
        lz4f.decompressLegacyFrameBatch(d_src, item_off, leg_len, d_dst, dst_off, dst_cap, from_legacy, consumed, mb)
        lz4f.multiframeSelectBatch(member, t_mem_off, split_result, item_first, item_result, from_legacy, item_result)
    if nbuf:
        lz4f.multiframeFinishBatch(member, t_mem_off, split_result, item_first, size, item_result, result)
    torch.cuda.synchronize()
    r.item_result, r.result, r.consumed = item_result.cpu().tolist(), result.cpu().tolist(), consumed.cpu().tolist()
    if r.nlegacy:                                     # for every legacy item consumed == len; the others are empty items
        assert r.consumed == r.leg_len
    r.host = whole.cpu().numpy()
    untouched = np.ones(r.host.shape, dtype=bool)
    r.data = []
    for s in range(nbuf):
        lo = BAND + r.out_off[s]
        untouched[lo:lo + r.out_size[s]] = False
        r.data.append(r.host[lo:lo + r.result[s]].tobytes() if r.result[s] >= 0 else None)
    assert (r.host[untouched] == FILL).all(), "bytes outside the planned slots changed"
    return r


def check(r, buffers, flags=0, legacy=True):
    """every buffer of a run against the model: totals, table, the two length arrays, item results, result, bytes"""
    assert r.totals == g.totals(buffers, legacy)
    for s, buf in enumerate(buffers):
        want_result, want_data, want_items = g.expected(buf, flags, legacy)
        assert r.split_result[s] == r.count[s] == len(want_items), s
        assert r.members[s] == g.table(buf, legacy), s
        lo = r.item_first[s]
        for k, (m, w) in enumerate(zip(g.split(buf, legacy), want_items)):
            i = lo + k
            assert r.item_off[i] == sum(len(b) for b in buffers[:s]) + m.pos
            if w is None:
                assert (r.item_len[i], r.leg_len[i], r.item_result[i], r.dst_cap[i]) == (0, 0, mg.HEADER_INCOMPLETE, 0), (s, k)
            else:
                got = r.size[i] if r.size[i] < 0 else r.item_result[i]
                lens = (0, m.len) if m.kind == g.LEGACY else (m.len, 0)
                assert ((r.item_len[i], r.leg_len[i]), got) == (lens, w), (s, k)
        assert r.result[s] == want_result, (s, r.result[s], want_result)
        if want_data is not None:
            assert r.data[s] == want_data and r.out_size[s] == want_result, s


def answers(r):
    return [d if d is not None else c for d, c in zip(r.data, r.result)]


# ----------------------------------------------------------------------------- the parts
@functools.lru_cache(maxsize=None)
def parts():
    """legacy frames of 4 KiB blocks (5 of them) and 64 KiB blocks (3), of 3 and of 70 small blocks, frames, a skippable"""
    p = Run()
    p.text4, p.text64 = lg.text(20000, 3), lg.text(150000, 4)
    p.l4, p.l64 = lg.write(p.text4, 4096), lg.write(p.text64, 65536)
    b3, p.c3 = lg.small_blocks(3, 5)
    b70, p.c70 = lg.small_blocks(70, 9)
    p.blocks = b3
    p.l3, p.l70 = lg.build(b3), lg.build(b70)
    p.a, p.b = mg.pick("text65537_bc1_cc1_cs0", "text1_bc0_cc0_cs1")
    p.sk = mg.skippable(5, b"seek table")
    return p


def orderings():
    p = parts()
    kinds = {"L": p.l64, "F": p.a.frame, "S": p.sk}
    out = []
    for k in (2, 3):
        for perm in itertools.permutations("LFS", k):
            out.append(b"".join(kinds[c] for c in perm))
    out += [p.l4 + p.l64, MAGIC + p.a.frame + p.l4, p.b.frame + MAGIC + p.sk + p.l3, p.l4 + p.b.frame + MAGIC, MAGIC,
            MAGIC + MAGIC, p.l70, p.a.frame + p.l70 + p.l3, b"", p.sk + mg.skippable(0), p.l3]
    return out


def defect_cases():
    """-> [(name, buffer, code)]; the codes are stated here so that the test also pins the model"""
    p = parts()
    a, b, good = p.a.frame, p.b.frame, p.l3
    blk = p.blocks
    out = []

    def add(name, bad, code, middle_code=None):
        out.append((name + "_only", bad, code))
        out.append((name + "_last", a + p.l4 + bad, code))
        # bytes follow the defective member: what cannot be delimited swallows them
        out.append((name + "_middle", a + bad + b, code if middle_code is None else middle_code))

    # (a torn size word exists only at the end of a buffer: with b behind it the word is foreign and starts junk)
    add("torn_size_word", good + b"\x07\x00", lg.SIZE_WRONG, mg.TYPE_UNKNOWN)
    add("zero_size_word", good + lg.le32(0), lg.FAILED)
    add("block_runs_off", lg.build(blk[:2]) + lg.le32(len(blk[2]) + len(b) + 1) + blk[2], lg.SIZE_WRONG)
    add("corrupt_block", lg.build([blk[0], lg.CORRUPT, blk[1]]), lg.FAILED)
    add("foreign_word", good + lg.le32(lg.BLOCK_BOUND + 1) + b"xyz", mg.TYPE_UNKNOWN)
    add("foreign_word_short", good + lg.le32(0x7FFFFFFF), mg.HEADER_INCOMPLETE, mg.TYPE_UNKNOWN)
    cc = mg.flip(a, len(a) - 1)
    out.append(("content_checksum_then_legacy", cc + good, mg.CONTENT_CHECKSUM))
    out.append(("content_checksum_between_legacy", p.l4 + cc + good, mg.CONTENT_CHECKSUM))
    out.append(("skippable_cut_after_legacy", good + p.sk[:-1], mg.SIZE_WRONG))
    out.append(("skippable_header_cut_after_legacy", b + good + p.sk[:6], mg.HEADER_INCOMPLETE))
    return out


def mixed(nbuf, seed):
    p = parts()
    rnd = random.Random(seed)
    small = [x.frame for x in mg.pick("text0_bc0_cc0_cs0", "text1_bc1_cc1_cs1", "text65537_bc1_cc0_cs0")]
    pool = small + [p.l3, p.l3, p.l4, MAGIC, p.sk, mg.skippable(9), p.l70]
    tails = [b"\x01\x02", p.sk[:6], p.l3 + b"\x07", p.l3 + lg.le32(0), lg.build([lg.CORRUPT]), small[1][:-2],
             lg.le32(lg.BLOCK_BOUND + 7) + b"junkjunk"]
    out = []
    for k in range(nbuf):
        buf = b"".join(rnd.choice(pool) for _ in range(rnd.randrange(0, 6)))
        if k % 20 == 7:
            buf += p.l64
        if rnd.random() < 0.25:
            buf += rnd.choice(tails)
        out.append(buf)
    return out


# ----------------------------------------------------------------------------- tests
def test_every_ordering_against_the_model(zl, gpu):
    p = parts()
    buffers = orderings()
    r = run(zl, gpu, buffers)
    check(r, buffers)
    # content of a buffer that the calls without the flag answer with FrameTypeUnknown
    first = buffers[0]
    assert first == p.l64 + p.a.frame and r.data[0] == p.text64 + p.a.content
    assert zl.lz4f.decompressMultiframes([first]) == [mg.TYPE_UNKNOWN]
    assert zl.lz4f.decompressMultiframes([first], legacy=True) == [p.text64 + p.a.content]
    assert r.members[0] == [(0, len(p.l64), g.LEGACY, 0), (len(p.l64), len(p.a.frame), g.FRAME, 0)]
    k70 = buffers.index(p.l70)
    assert r.data[k70] == p.c70 and r.members[k70] == [(0, len(p.l70), g.LEGACY, 0)]
    assert [r.result[buffers.index(x)] for x in (MAGIC, MAGIC + MAGIC, b"", p.sk + mg.skippable(0))] == [0, 0, 0, 0]
    assert [r.count[buffers.index(x)] for x in (MAGIC, MAGIC + MAGIC, b"")] == [1, 2, 0]
    assert zl.lz4f.multiframeMembers(buffers, legacy=True) == [g.table(b) for b in buffers]
    assert zl.lz4f.multiframeMembers(buffers) == [mg.table(b) for b in buffers]
    assert zl.lz4f.decompressFiles(buffers) == answers(r)


def test_one_call_of_140_mixed_buffers(zl, gpu):
    buffers = mixed(140, 23)
    assert len(buffers) > 2 * 64 and {len(g.split(b)) for b in buffers} >= set(range(6))
    r = run(zl, gpu, buffers, align=64)
    check(r, buffers)
    assert {c for c in r.result if c < 0} >= {mg.HEADER_INCOMPLETE, mg.SIZE_WRONG, mg.TYPE_UNKNOWN, lg.FAILED}
    # the same members one by one through the frame calls and the legacy calls
    frames, legacies = [], []
    for s, buf in enumerate(buffers):
        for k, (pos, n, kind, _) in enumerate(r.members[s]):
            (legacies if kind == g.LEGACY else frames if kind == g.FRAME else []).append((r.item_first[s] + k, buf[pos:pos + n]))
    assert len(frames) > 64 and len(legacies) > 64
    singles = list(zip(frames, zl.lz4f.decompressFrames([m for _, m in frames])))
    singles += [(x, out) for x, (out, consumed) in zip(legacies, zl.lz4f.decompressLegacyFrames([m for _, m in legacies]))]
    for (i, _), want in singles:
        if isinstance(want, int):
            assert (r.size[i] if r.size[i] < 0 else r.item_result[i]) == want, i
        else:
            lo = BAND + r.dst_off[i]
            assert r.item_result[i] == len(want) and r.host[lo:lo + len(want)].tobytes() == want, i
    assert zl.lz4f.decompressFiles(buffers, align=64) == answers(r)


def test_defects(zl, gpu):
    p = parts()
    cases = defect_cases()
    buffers = [buf for _, buf, _ in cases]
    r = run(zl, gpu, buffers)
    check(r, buffers)
    for s, (name, buf, code) in enumerate(cases):
        assert r.result[s] == code, (name, r.result[s])
    by = {name: s for s, (name, _, _) in enumerate(cases)}
    # a corrupt block followed by a good frame: the block's code decides, the later frame's item still holds its size
    s = by["corrupt_block_middle"]
    assert r.count[s] == 3 and r.item_result[r.item_first[s]:r.item_first[s + 1]] == [len(p.a.content), lg.FAILED, 1]
    # a bad content checksum in front of a good legacy member: the member behind it is decoded and can be salvaged
    s = by["content_checksum_then_legacy"]
    assert r.item_result[r.item_first[s]:r.item_first[s + 1]] == [mg.CONTENT_CHECKSUM, len(p.c3)]
    lo = BAND + r.dst_off[r.item_first[s] + 1]
    assert r.host[lo:lo + len(p.c3)].tobytes() == p.c3
    assert zl.lz4f.decompressFiles(buffers) == [code for _, _, code in cases]


def test_split_flags_0_is_the_split_without_ex(zl, gpu):
    import torch
    buffers = orderings() + [buf for _, buf, _ in defect_cases()] + mixed(70, 5) + [c[1] for c in mg.defects()]
    r = run(zl, gpu, buffers, split_flags=0)
    check(r, buffers, legacy=False)
    assert r.totals[2:] == [0, 0] and not any(r.leg_len)
    d_src, src_off, src_len = r.raw["src"]
    t_mem_off, t_mem_cap = r.raw["mem"]
    nbuf = len(buffers)

    def like(t, n=None):
        return torch.full_like(t if n is None else t[:n], -999)

    count, totals = like(r.raw["count"]), like(r.raw["totals"], 2)
    zl.lz4f.multiframeSplitBatch(d_src, src_off, src_len, count, totals)
    assert totals.tolist() == r.totals[:2] and count.tolist() == r.count
    old = {k: like(r.raw[k]) for k in ("count", "member", "item_first", "item_off", "item_len", "result")}
    old["member"].fill_(-7)
    zl.lz4f.multiframeSplitBatch(d_src, src_off, src_len, old["count"], totals, old["member"], t_mem_off, t_mem_cap,
                                 old["item_first"], old["item_off"], old["item_len"], old["result"])
    assert totals.tolist() == r.totals[:2]
    for k, t in old.items():
        assert torch.equal(t, r.raw[k]), k
    # the legacy magic is an unknown frame type to this split (fewer than 7 bytes: no header at all)
    legacy_first = [s for s, b in enumerate(buffers) if b[:4] == MAGIC and len(b) >= 7]
    assert len(legacy_first) > 10 and all(r.result[s] == mg.TYPE_UNKNOWN for s in legacy_first)
    assert r.result[buffers.index(MAGIC)] == mg.HEADER_INCOMPLETE
    assert nbuf > 128


def test_linked_frames_and_legacy_members_together(zl, gpu):
    p = parts()
    (l0, d0), (l1, d1) = mg.linked()[:2]
    buffers = [l0 + p.l4 + p.a.frame, p.l3 + l1 + MAGIC + l0, p.l4 + p.b.frame]
    r = run(zl, gpu, buffers, mg.DECODE_LINKED)
    check(r, buffers, mg.DECODE_LINKED)
    assert r.data == [d0 + p.text4 + p.a.content, p.c3 + d1 + d0, p.text4 + p.b.content]
    assert zl.lz4f.decompressFiles(buffers) == r.data
    r = run(zl, gpu, buffers, 0)
    check(r, buffers, 0)
    assert r.result == [mg.FAILED, mg.FAILED, len(p.text4) + 1]
    assert zl.lz4f.decompressMultiframes(buffers, legacy=True) == [mg.FAILED, mg.FAILED, p.text4 + p.b.content]


@pytest.mark.parametrize("align", [0, 1, 64, 4096])
def test_alignment_and_slots(zl, gpu, align):
    buffers = orderings() + [buf for _, buf, _ in defect_cases()]
    r = run(zl, gpu, buffers, align=align)
    check(r, buffers)
    assert zl.lz4f.decompressMultiframes(buffers, align=align, legacy=True) == answers(r)


def test_tables_and_block_counts_too_small(zl, gpu):
    p = parts()
    buffers = [p.a.frame + p.l4, p.l3 + p.sk + p.l4, p.l64 + p.b.frame]
    full = run(zl, gpu, buffers)
    check(full, buffers)
    assert full.totals == [7, 3, 4, 5 + 3 + 5 + 3]
    # the member table of buffer 1 one entry short: DstMaxSizeTooSmall for that buffer alone, nothing written, its items
    # keep their room with both lengths 0
    r = run(zl, gpu, buffers, mem_cap=[2, 2, 2])
    assert r.split_result == [2, mg.DST_TOO_SMALL, 2] and r.members[1] == [] and r.count == [2, 3, 2]
    assert r.item_len[2:5] == [0, 0, 0] and r.leg_len[2:5] == [0, 0, 0] and r.item_first == full.item_first
    assert r.result == [full.result[0], mg.DST_TOO_SMALL, full.result[2]] and r.out_size[1] == 0
    assert (r.data[0], r.data[2]) == (full.data[0], full.data[2])
    assert r.totals == full.totals                   # (the count does not look at the table)
    # max_blocks of the legacy decode one short: the legacy item that no longer fits answers InvalidState and decides its
    # buffer; the others are left alone
    r = run(zl, gpu, buffers, legacy_decode_blocks=full.legacy_blocks - 1)
    assert r.result == [full.result[0], full.result[1], mg.INVALID_STATE] and r.data[:2] == full.data[:2]
    assert r.item_result == full.item_result[:5] + [mg.INVALID_STATE, 1]


def test_refusals_of_the_two_batch_calls(zl, gpu):
    import torch
    L = zl.lib()
    p = parts()
    buffers = [p.b.frame + p.l3 + p.sk, p.l4]
    d_src, src_off, src_len = zl._stage(buffers, gpu)
    st = zl._stream()
    ptr = lambda t: C.c_void_p(t.data_ptr())           # noqa: E731
    i64 = lambda n: torch.zeros(n, dtype=torch.int64, device=gpu)   # noqa: E731
    count, totals = i64(2), i64(4)
    assert L.zlz4f_batch_multiframe_split_ex(st, ptr(d_src), ptr(src_off), ptr(src_len), 2, ptr(count), ptr(totals), None, None,
                                             None, None, None, None, None, 1, None) == 0
    assert count.tolist() == [3, 1] and totals.tolist() == [4, 1, 2, 8]
    member, mem_off, mem_cap = torch.zeros((4, 3), dtype=torch.int64, device=gpu), i64(2), i64(2)
    mem_off[1], mem_cap[0], mem_cap[1] = 3, 3, 1
    item_first, item_off, item_len, sres, leg_len = i64(3), i64(4), i64(4), i64(2), i64(4)
    rec = (st, ptr(d_src), ptr(src_off), ptr(src_len), 2, ptr(count), ptr(totals), ptr(member), ptr(mem_off), ptr(mem_cap),
           ptr(item_first), ptr(item_off), ptr(item_len), ptr(sres), 1, ptr(leg_len))
    assert L.zlz4f_batch_multiframe_split_ex(*rec) == 0
    assert sres.tolist() == [3, 1] and item_first.tolist() == [0, 3, 4]
    assert item_len.tolist() == [len(p.b.frame), 0, 0, 0] and leg_len.tolist() == [0, len(p.l3), 0, len(p.l4)]
    a, b, out = i64(4), i64(4), i64(4)
    a += 10
    b += 20
    sel = (st, ptr(member), ptr(mem_off), ptr(sres), ptr(item_first), ptr(a), ptr(b), 2, ptr(out))
    assert L.zlz4f_batch_multiframe_select(*sel) == 0
    assert out.tolist() == [10, 20, 10, 20]
    sres2 = sres.clone()
    sres2[1] = mg.DST_TOO_SMALL                       # a buffer without a table copies the frame family's answers
    assert L.zlz4f_batch_multiframe_select(*(sel[:3] + (ptr(sres2),) + sel[4:])) == 0
    assert out.tolist() == [10, 20, 10, 10]

    def refused(fn, args, which):
        for k in which:
            bad = list(args)
            bad[k] = None
            assert fn(*bad) == mg.INVALID_STATE, (fn.__name__, k, "null")
            bad[k] = C.c_void_p(args[k].value + 4)
            assert fn(*bad) == mg.INVALID_STATE, (fn.__name__, k, "misaligned")

    tensors = (count, totals, member, item_first, item_off, item_len, sres, leg_len, out)
    before = [t.clone() for t in tensors]
    refused(L.zlz4f_batch_multiframe_split_ex, rec, (2, 3, 5, 6, 8, 9, 10, 11, 12, 13, 15))
    assert L.zlz4f_batch_multiframe_split_ex(*(rec[:1] + (None,) + rec[2:])) == mg.INVALID_STATE         # d_src
    bad = list(rec)
    bad[7] = C.c_void_p(rec[7].value + 4)
    assert L.zlz4f_batch_multiframe_split_ex(*bad) == mg.INVALID_STATE                                   # d_member misaligned
    for flags in (2, 0x80000000, 3):
        assert L.zlz4f_batch_multiframe_split_ex(*(rec[:14] + (flags,) + rec[15:])) == mg.PARAMETER_INVALID
        assert L.zlz4f_batch_multiframe_split_ex(*(rec[:6] + (None,) + rec[7:14] + (flags,) + rec[15:])) == mg.PARAMETER_INVALID
    refused(L.zlz4f_batch_multiframe_select, sel, (1, 2, 3, 4, 5, 6, 8))
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(before, tensors)), "a refused call wrote"
    # nbuf == 0: 0, four zeros
    totals.fill_(7)
    for flags in (0, 1):
        assert L.zlz4f_batch_multiframe_split_ex(st, None, None, None, 0, None, ptr(totals), None, None, None, None, None, None,
                                                 None, flags, None) == 0
        assert totals.tolist() == [0, 0, 0, 0]
        totals.fill_(7)
    assert L.zlz4f_batch_multiframe_select(st, None, None, None, None, None, None, 0, None) == 0
    assert zl.lz4f.decompressFiles([]) == [] and zl.lz4f.multiframeMembers([], legacy=True) == []
    with pytest.raises(zl.Lz4Error) as e:
        zl.lz4f.decompressMultiframes(buffers, flags=2, legacy=True)
    assert e.value.code == mg.PARAMETER_INVALID


def test_host_single_calls(zl, gpu):
    p = parts()
    (l0, d0) = mg.linked()[0]
    f = zl.lz4f
    three = [(p.l64 + p.a.frame + mg.skippable(11, b"seek table") + p.b.frame, p.text64 + p.a.content + p.b.content),
             (p.a.frame + p.l3 + MAGIC + l0, p.a.content + p.c3 + d0), (MAGIC, b"")]
    for buf, content in three:
        assert f.decompressFile(buf) == content
        assert f.multiframeDecompressedSize(buf, f.DECODE_LINKED, legacy=True) == len(content)
        assert f.decompressMultiframe(buf, f.DECODE_LINKED, legacy=True) == content
    # the first one answers FrameTypeUnknown without the flag, through the old calls and through the _ex calls with 0
    L = zl.lib()
    s, n = zl._in(three[0][0])
    for call in (f.decompressMultiframe, f.multiframeDecompressedSize):
        with pytest.raises(zl.Lz4Error) as e:
            call(three[0][0])
        assert e.value.code == mg.TYPE_UNKNOWN
    assert L.zlz4f_multiframe_decompressed_size_ex(C.addressof(s), n, 0, 0) == mg.TYPE_UNKNOWN
    assert f.decompressFile(b"") == b"" and f.decompressFile(p.sk) == b""
    # without legacy members the _ex calls answer what the calls without _ex answer
    plain = p.a.frame + p.sk + p.b.frame
    assert f.decompressMultiframe(plain, legacy=True) == f.decompressMultiframe(plain) == p.a.content + p.b.content
    for name, buf, code in defect_cases():
        if name.endswith("_middle") or name.startswith("content_checksum"):
            for call in ((f.decompressFile,) if name.startswith("content") else
                         (f.decompressFile, lambda b: f.multiframeDecompressedSize(b, legacy=True))):
                with pytest.raises(zl.Lz4Error) as e:
                    call(buf)
                assert e.value.code == code, name
    with pytest.raises(zl.Lz4Error) as e:
        f.decompressMultiframe(three[0][0], dst_cap=len(three[0][1]) - 1, legacy=True)
    assert e.value.code == mg.DST_TOO_SMALL
