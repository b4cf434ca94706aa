#!/usr/bin/env python3
"""Timing of whole-file decoding: legacy members in multiframe buffers (zlz4f_batch_multiframe_split_ex and
zlz4f_batch_multiframe_select around the frame calls and the legacy frame calls).

Input (bench.make_device_blocks, D-text, compressed on the device): --members chunks of 64 KiB, each written as a one-block
modern frame and -- for (b) every fourth, for (c) all of them -- as the blocks of legacy frames with 64 KiB blocks.

 a  the cost of the flag where it buys nothing: --per-buffer modern frames per buffer, the split (count, record) through
    zlz4f_batch_multiframe_split and through the _ex call with split_flags 0 and 1.
 b  the cost of the merge: the same content with every fourth member a legacy frame; the whole sequence (splits, two
    queries, select, plan, two decodes, select, finish) against its floor: the same members passed as separate items to the
    frame calls and to the legacy calls.
 c  the serial case: --serial BUFFERSxBLOCKS buffers of one legacy member each, where one lane walks all the blocks of a
    buffer; the floor is the legacy calls over the same frames.

The steps alternate inside one process: HIP events around each call, the stream synchronised after each, warm-up, --reps
alternations; median and spread (min .. max) per call.  Before timing, totals, results and every decoded byte are compared
with the input.  (profiles/r33_lz4_files.md)"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch
    import zig_lz4_amd as zl
    from bench import make_device_blocks
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=65536)
    ap.add_argument("--per-buffer", type=int, default=16)
    ap.add_argument("--serial", default="64x1024")
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    assert zl.device_available(), "needs a gfx950 device"
    lz4f = zl.lz4f
    n, bs, k = a.members, 65536, a.per_buffer
    assert n % k == 0 and k % 4 == 0
    LEG = lz4f.SPLIT_LEGACY

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def alternate(title, calls):
        for _ in range(a.warmup):
            for _, fn in calls:
                fn()
        torch.cuda.synchronize()
        times = [[] for _ in calls]
        for _ in range(a.reps):
            for t, (_, fn) in zip(times, calls):
                t.append(timed(fn))
        med = {}
        for (label, _), t in zip(calls, times):
            med[label] = statistics.median(t)
            print("%-4s %-40s %9.3f ms  (%.3f .. %.3f, %d runs)" % (title, label, med[label], min(t), max(t), len(t)), flush=True)
        return med

    def i64(m):
        return torch.zeros(max(1, m), dtype=torch.int64, device=dev)[:m]

    def full(m, v):
        return torch.full((m,), v, dtype=torch.int64, device=dev)

    def u8(m):
        return torch.empty(max(16, m), dtype=torch.uint8, device=dev)

    def pack(rows, lens):
        """the first lens[j] bytes of every row back to back -> (bytes, offsets, ends)"""
        stride = rows.shape[1]
        col = torch.arange(stride, dtype=torch.int64, device=dev)
        parts = []
        for lo in range(0, rows.shape[0], 2048):      # (a chunk at a time: the mask of all rows at once is large)
            hi = min(rows.shape[0], lo + 2048)
            parts.append(rows[lo:hi][col[None, :] < lens[lo:hi, None]])
        ends = torch.cumsum(lens, 0)
        return torch.cat(parts), ends - lens, ends

    ar = torch.arange(n, dtype=torch.int64, device=dev)
    raw = make_device_blocks("text", n, bs, dev, seed=1).reshape(-1)
    out = torch.empty(n * bs, dtype=torch.uint8, device=dev)
    lp = zl.LegacyPrefs(bs, 0)

    def sequence(src, src_off, src_len, nitems, frame_blocks, legacy_blocks):
        """the arrays and the steps of the whole sequence over nbuf buffers -> (steps, state)"""
        nbuf = src_len.numel()
        s = argparse.Namespace()
        s.count, s.totals, s.ptotals = i64(nbuf), i64(4), i64(2)
        s.member = torch.zeros((nitems, 3), dtype=torch.int64, device=dev)
        s.mem_off, s.mem_cap = i64(nbuf), i64(nbuf)
        s.item_first, s.item_off, s.item_len, s.leg_len, s.sres = i64(nbuf + 1), i64(nitems), i64(nitems), i64(nitems), i64(nbuf)
        s.size, s.lsize, s.dst_off, s.dst_cap, s.ires, s.lres = (i64(nitems) for _ in range(6))
        s.out_off, s.out_size, s.res = i64(nbuf), i64(nbuf), i64(nbuf)
        qws = u8(lz4f.frameDecompressedSizeBatchWorkspace(nitems, frame_blocks))
        dws = u8(lz4f.decompressFrameBatchWorkspace(nitems, frame_blocks))
        lqws = u8(lz4f.legacyFrameDecompressedSizeBatchWorkspace(nitems, legacy_blocks))
        ldws = u8(lz4f.decompressLegacyFrameBatchWorkspace(nitems, legacy_blocks))
        # the member table is laid out as the items are: the count fills mem_cap, its scan mem_off
        lz4f.multiframeSplitBatchEx(src, src_off, src_len, s.mem_cap, s.totals, split_flags=LEG)
        s.mem_off.copy_(torch.cumsum(s.mem_cap, 0) - s.mem_cap)
        steps = [
            ("count", lambda: lz4f.multiframeSplitBatchEx(src, src_off, src_len, s.count, s.totals, split_flags=LEG)),
            ("record (counts again)", lambda: lz4f.multiframeSplitBatchEx(
                src, src_off, src_len, s.count, s.totals, s.member, s.mem_off, s.mem_cap, s.item_first, s.item_off, s.item_len,
                s.sres, LEG, s.leg_len)),
            ("frame size query", lambda: lz4f.frameDecompressedSizeBatch(src, s.item_off, s.item_len, s.size, frame_blocks, qws)),
            ("legacy size query", lambda: lz4f.legacyFrameDecompressedSizeBatch(src, s.item_off, s.leg_len, s.lsize, None,
                                                                                legacy_blocks, lqws)),
            ("select sizes", lambda: lz4f.multiframeSelectBatch(s.member, s.mem_off, s.sres, s.item_first, s.size, s.lsize,
                                                                s.size)),
            ("plan", lambda: lz4f.multiframePlanBatch(s.size, s.item_first, s.dst_off, s.dst_cap, s.out_off, s.out_size,
                                                      s.ptotals, 0)),
            ("frame decode", lambda: lz4f.decompressFrameBatch(src, s.item_off, s.item_len, out, s.dst_off, s.dst_cap, s.ires,
                                                               frame_blocks, dws)),
            ("legacy decode", lambda: lz4f.decompressLegacyFrameBatch(src, s.item_off, s.leg_len, out, s.dst_off, s.dst_cap,
                                                                      s.lres, None, legacy_blocks, ldws)),
            ("select results", lambda: lz4f.multiframeSelectBatch(s.member, s.mem_off, s.sres, s.item_first, s.ires, s.lres,
                                                                  s.ires)),
            ("finish", lambda: lz4f.multiframeFinishBatch(s.member, s.mem_off, s.sres, s.item_first, s.size, s.ires, s.res)),
        ]
        return steps, s

    def report(title, med, steps, floor_labels):
        total = sum(med[label] for label, _ in steps)
        floor = sum(med[label] for label in floor_labels)
        print("%-4s floor %.3f ms; sequence %.3f ms = %.3f x; overhead %.3f ms = %.3f of the floor" %
              (title, floor, total, total / floor, total - floor, (total - floor) / floor), flush=True)

    parts = a.parts.split(",")
    if "a" in parts or "b" in parts:
        prefs = zl.Prefs()
        prefs.block_mode = 1
        fb = lz4f.compressFrameBound(bs, prefs)
        lb = lz4f.legacyCompressFrameBound(bs, lp)
        stride = max(fb, lb)
        rows = torch.empty((n, stride), dtype=torch.uint8, device=dev)
        cres = i64(n)
        lz4f.compressFrameBatch(raw, ar * bs, full(n, bs), rows.view(-1), ar * stride, full(n, stride), cres, prefs, 0, n)
        torch.cuda.synchronize()
        assert bool((cres > 0).all()), "compression failed"
        nbuf = n // k
        first = torch.arange(nbuf, dtype=torch.int64, device=dev) * k

    if "a" in parts:
        packed, frm_off, ends = pack(rows, cres)
        print("a: %d buffers of %d one-block frames of %d B D-text, %.1f MiB" % (nbuf, k, bs, packed.numel() / 2**20), flush=True)
        src_off = frm_off[first]
        src_len = ends[first + k - 1] - src_off
        count, t2, t4 = i64(nbuf), i64(2), i64(4)
        member = torch.zeros((n, 3), dtype=torch.int64, device=dev)
        mem_cap = full(nbuf, k)
        item_first, item_off, item_len, leg_len, sres = i64(nbuf + 1), i64(n), i64(n), i64(n), i64(nbuf)
        rec = (member, first, mem_cap, item_first, item_off, item_len, sres)
        calls = [("split: count", lambda: lz4f.multiframeSplitBatch(packed, src_off, src_len, count, t2)),
                 ("split: record", lambda: lz4f.multiframeSplitBatch(packed, src_off, src_len, count, t2, *rec))]
        for flags in (0, LEG):
            calls.append(("split_ex flags %d: count" % flags,
                          lambda flags=flags: lz4f.multiframeSplitBatchEx(packed, src_off, src_len, count, t4, split_flags=flags)))
            calls.append(("split_ex flags %d: record" % flags,
                          lambda flags=flags: lz4f.multiframeSplitBatchEx(packed, src_off, src_len, count, t4, *rec, flags, leg_len)))
        for _, fn in calls:
            item_off.zero_()
            fn()
            torch.cuda.synchronize()
            assert bool((count == k).all()), "counts"
        assert t2.tolist() == [n, n] and t4.tolist() == [n, n, 0, 0] and not bool(leg_len.any()), "totals"
        assert torch.equal(item_off, frm_off) and torch.equal(item_len, cres) and bool((sres == k).all()), "items"
        med = alternate("a", calls)
        old = med["split: count"] + med["split: record"]
        for flags in (0, LEG):
            ex = med["split_ex flags %d: count" % flags] + med["split_ex flags %d: record" % flags]
            print("a    count + record: split %.3f ms, split_ex flags %d %.3f ms = %+.3f ms" % (old, flags, ex, ex - old), flush=True)
        del packed, member

    if "b" in parts:
        q = ar[3::4].contiguous()
        nl = q.numel()
        lrows = torch.empty((nl, lb), dtype=torch.uint8, device=dev)
        lres = i64(nl)
        lz4f.compressLegacyFrameBatch(raw, q * bs, full(nl, bs), lrows.view(-1), torch.arange(nl, dtype=torch.int64, device=dev) * lb,
                                      full(nl, lb), lres, lp, nl)
        torch.cuda.synchronize()
        assert bool((lres > 0).all()), "legacy compression failed"
        rows[q, :lb] = lrows
        mlen = cres.clone()
        mlen[q] = lres
        del lrows
        packed, m_off, ends = pack(rows, mlen)
        print("b: %d buffers of %d members, every fourth a legacy frame, %.1f MiB" % (nbuf, k, packed.numel() / 2**20), flush=True)
        src_off = m_off[first]
        src_len = ends[first + k - 1] - src_off
        steps, s = sequence(packed, src_off, src_len, n, n - nl, nl)
        out.zero_()
        for _, fn in steps:
            fn()
        torch.cuda.synchronize()
        assert s.totals.tolist() == [n, n - nl, nl, nl] and bool((s.sres == k).all()), "split results"
        assert torch.equal(s.item_off, m_off) and torch.equal(s.item_len + s.leg_len, mlen), "the items are not the members"
        assert bool((s.leg_len[q] == lres).all()) and int(s.leg_len.count_nonzero()) == nl, "legacy items"
        assert s.ptotals.tolist() == [n * bs, n * bs] and bool((s.res == k * bs).all()) and torch.equal(out, raw), "decode"
        # the floor: the same members as separate items of the two families
        f = ar[ar % 4 != 3].contiguous()
        nf = f.numel()
        f_off, f_len, f_dst, f_cap, f_size, f_res = m_off[f].contiguous(), mlen[f].contiguous(), f * bs, full(nf, bs), i64(nf), i64(nf)
        l_off, l_len, l_dst, l_cap, l_size, l_res = m_off[q].contiguous(), mlen[q].contiguous(), q * bs, full(nl, bs), i64(nl), i64(nl)
        fq, fd = u8(lz4f.frameDecompressedSizeBatchWorkspace(nf, nf)), u8(lz4f.decompressFrameBatchWorkspace(nf, nf))
        lq, ld = u8(lz4f.legacyFrameDecompressedSizeBatchWorkspace(nl, nl)), u8(lz4f.decompressLegacyFrameBatchWorkspace(nl, nl))
        floor = [
            ("floor: frame size query, items", lambda: lz4f.frameDecompressedSizeBatch(packed, f_off, f_len, f_size, nf, fq)),
            ("floor: frame decode, items", lambda: lz4f.decompressFrameBatch(packed, f_off, f_len, out, f_dst, f_cap, f_res, nf, fd)),
            ("floor: legacy size query, items", lambda: lz4f.legacyFrameDecompressedSizeBatch(packed, l_off, l_len, l_size, None,
                                                                                              nl, lq)),
            ("floor: legacy decode, items", lambda: lz4f.decompressLegacyFrameBatch(packed, l_off, l_len, out, l_dst, l_cap, l_res,
                                                                                    None, nl, ld)),
        ]
        out.zero_()
        for _, fn in floor:
            fn()
        torch.cuda.synchronize()
        assert all(bool((t == bs).all()) for t in (f_size, f_res, l_size, l_res)) and torch.equal(out, raw), "the floor is wrong"
        med = alternate("b", steps + floor)
        report("b", med, steps, [label for label, _ in floor])
        del packed, s, steps, floor
    if "a" in parts or "b" in parts:
        del rows

    if "c" in parts:
        nbuf, blocks = (int(x) for x in a.serial.split("x"))
        assert nbuf * blocks == n, "--serial must use all members"
        cb = lz4f.legacyCompressFrameBound(blocks * bs, lp)
        frames = torch.empty(nbuf * cb, dtype=torch.uint8, device=dev)
        src_off = torch.arange(nbuf, dtype=torch.int64, device=dev) * cb
        src_len = i64(nbuf)
        lz4f.compressLegacyFrameBatch(raw, src_off // cb * (blocks * bs), full(nbuf, blocks * bs), frames, src_off, full(nbuf, cb),
                                      src_len, lp, n)
        torch.cuda.synchronize()
        assert bool((src_len > 0).all()), "legacy compression failed"
        print("c: %d buffers of one legacy member of %d blocks of %d B, %.1f MiB" % (nbuf, blocks, bs, int(src_len.sum()) / 2**20),
              flush=True)
        steps, s = sequence(frames, src_off, src_len, nbuf, 0, n)
        out.zero_()
        for _, fn in steps:
            fn()
        torch.cuda.synchronize()
        assert s.totals.tolist() == [nbuf, 0, nbuf, n] and torch.equal(s.leg_len, src_len), "split results"
        assert bool((s.res == blocks * bs).all()) and torch.equal(out, raw), "decode"
        l_dst, l_cap, l_size, l_res = src_off // cb * (blocks * bs), full(nbuf, blocks * bs), i64(nbuf), i64(nbuf)
        lq, ld = u8(lz4f.legacyFrameDecompressedSizeBatchWorkspace(nbuf, n)), u8(lz4f.decompressLegacyFrameBatchWorkspace(nbuf, n))
        floor = [
            ("floor: legacy size query, items", lambda: lz4f.legacyFrameDecompressedSizeBatch(frames, src_off, src_len, l_size,
                                                                                              None, n, lq)),
            ("floor: legacy decode, items", lambda: lz4f.decompressLegacyFrameBatch(frames, src_off, src_len, out, l_dst, l_cap,
                                                                                    l_res, None, n, ld)),
        ]
        out.zero_()
        for _, fn in floor:
            fn()
        torch.cuda.synchronize()
        assert bool((l_size == blocks * bs).all()) and bool((l_res == blocks * bs).all()) and torch.equal(out, raw), "the floor"
        med = alternate("c", steps + floor)
        report("c", med, steps, [label for label, _ in floor])


if __name__ == "__main__":
    main()
