#!/usr/bin/env python3
"""Timing of multiframe decoding (zlz4f_batch_multiframe_split / _plan / _finish around the frame size query and the frame
decode), step by step, against the yardstick: zlz4f_batch_frame_decompressed_size_ex +
zlz4f_batch_decompress_frame_ex over the SAME frames passed as separate items -- existing code, which has to know where every
frame starts.  What the multiframe calls add on top (count, record, plan, finish) is reported as a fraction of it.

Input (bench.make_device_blocks, D-text, compressed on the device): --frames one-block frames of 64 KiB, laid back to back
and cut into buffers by --groupings BUFFERSxMEMBERS (4096x16: many short buffers; 64x1024: the serial walk of the split,
1024 dependent hops on 64 lanes).  The steps alternate inside one process: HIP events around each call, the stream
synchronised after each, warm-up, --reps alternations; median and spread (min .. max) per call.  Before timing, the member
tables, the results and every decoded byte are compared with the input.  (profiles/r30_multiframe.md)"""
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
    ap.add_argument("--frames", type=int, default=65536)
    ap.add_argument("--groupings", default="4096x16,64x1024")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    groupings = [tuple(int(x) for x in gp.split("x")) for gp in a.groupings.split(",")]
    assert all(nb * k == a.frames for nb, k in groupings), "every grouping must use all frames"
    dev = torch.device("cuda:0")
    assert zl.device_available(), "needs a gfx950 device"
    lz4f = zl.lz4f

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
            print("%-10s %-34s %9.3f ms  (%.3f .. %.3f, %d runs)" % (title, label, med[label], min(t), max(t), len(t)))
        return med

    # ---- the frames: one block each, back to back
    n, bs = a.frames, 65536
    prefs = zl.Prefs()
    prefs.block_mode = 1
    ar = torch.arange(n, dtype=torch.int64, device=dev)
    raw = make_device_blocks("text", n, bs, dev, seed=1).reshape(-1)
    fb = lz4f.compressFrameBound(bs, prefs)
    slots = torch.empty(n * fb, dtype=torch.uint8, device=dev)
    cres = torch.empty(n, dtype=torch.int64, device=dev)
    lz4f.compressFrameBatch(raw, ar * bs, torch.full((n,), bs, dtype=torch.int64, device=dev), slots, ar * fb,
                            torch.full((n,), fb, dtype=torch.int64, device=dev), cres, prefs, 0, n)
    torch.cuda.synchronize()
    assert bool((cres > 0).all()), "compression failed"
    col = torch.arange(fb, dtype=torch.int64, device=dev)
    parts = []
    for lo in range(0, n, 2048):                      # (a chunk at a time: the mask of all slots at once is large)
        hi = min(n, lo + 2048)
        parts.append(slots[lo * fb:hi * fb].view(hi - lo, fb)[col[None, :] < cres[lo:hi, None]])
    packed = torch.cat(parts)
    del parts, slots
    ends = torch.cumsum(cres, 0)
    frm_off = ends - cres
    assert packed.numel() == int(ends[-1])
    print("%d one-block frames of %d B D-text, %.1f MiB back to back" % (n, bs, packed.numel() / 2**20))

    def i64(k):
        return torch.zeros(max(1, k), dtype=torch.int64, device=dev)[:k]

    # ---- the yardstick: the same frames as separate items
    y_size, y_res, y_off = i64(n), i64(n), ar * bs
    y_cap = torch.full((n,), bs, dtype=torch.int64, device=dev)
    out = torch.empty(n * bs, dtype=torch.uint8, device=dev)
    qws = torch.empty(max(16, lz4f.frameDecompressedSizeBatchWorkspace(n, n)), dtype=torch.uint8, device=dev)
    dws = torch.empty(max(16, lz4f.decompressFrameBatchWorkspace(n, n)), dtype=torch.uint8, device=dev)
    y_query = lambda: lz4f.frameDecompressedSizeBatch(packed, frm_off, cres, y_size, n, qws)  # noqa: E731
    y_decode = lambda: lz4f.decompressFrameBatch(packed, frm_off, cres, out, y_off, y_cap, y_res, n, dws)  # noqa: E731
    y_query()
    y_decode()
    torch.cuda.synchronize()
    assert bool((y_size == bs).all()) and bool((y_res == bs).all()) and torch.equal(out, raw), "the yardstick is wrong"

    for nbuf, k in groupings:
        title = "%dx%d" % (nbuf, k)
        first = torch.arange(nbuf, dtype=torch.int64, device=dev) * k
        src_off = frm_off[first]
        src_len = ends[first + k - 1] - src_off
        count, totals, ptotals = i64(nbuf), i64(2), i64(2)
        member = torch.zeros((n, 3), dtype=torch.int64, device=dev)
        mem_cap = torch.full((nbuf,), k, dtype=torch.int64, device=dev)
        item_first, item_off, item_len, sres = i64(nbuf + 1), i64(n), i64(n), i64(nbuf)
        size, dst_off, dst_cap, ires = i64(n), i64(n), i64(n), i64(n)
        out_off, out_size, res = i64(nbuf), i64(nbuf), i64(nbuf)
        steps = [
            ("count", lambda: lz4f.multiframeSplitBatch(packed, src_off, src_len, count, totals)),
            ("record (counts again)", lambda: lz4f.multiframeSplitBatch(packed, src_off, src_len, count, totals, member, first,
                                                                       mem_cap, item_first, item_off, item_len, sres)),
            ("size query", lambda: lz4f.frameDecompressedSizeBatch(packed, item_off, item_len, size, n, qws)),
            ("plan", lambda: lz4f.multiframePlanBatch(size, item_first, dst_off, dst_cap, out_off, out_size, ptotals, 0)),
            ("decode", lambda: lz4f.decompressFrameBatch(packed, item_off, item_len, out, dst_off, dst_cap, ires, n, dws)),
            ("finish", lambda: lz4f.multiframeFinishBatch(member, first, sres, item_first, size, ires, res)),
        ]
        out.zero_()
        for _, fn in steps:
            fn()
        torch.cuda.synchronize()
        assert totals.tolist() == [n, n] and bool((count == k).all()) and bool((sres == k).all()), "split results"
        assert torch.equal(item_off, frm_off) and torch.equal(item_len, cres), "the items are not the frames"
        assert torch.equal(member[:, 0], frm_off - src_off.repeat_interleave(k)) and torch.equal(member[:, 1], cres), "member table"
        assert ptotals.tolist() == [n * bs, n * bs] and torch.equal(dst_off, y_off), "plan"
        assert bool((res == k * bs).all()) and torch.equal(out, raw), "the multiframe decode is wrong"
        med = alternate(title, steps + [("yardstick: size query, items", y_query), ("yardstick: decode, items", y_decode)])
        yard = med["yardstick: size query, items"] + med["yardstick: decode, items"]
        added = med["count"] + med["record (counts again)"] + med["plan"] + med["finish"]
        total = added + med["size query"] + med["decode"]
        print("%-10s yardstick %.3f ms; multiframe %.3f ms = %.3f x; count + record + plan + finish %.3f ms = %.3f of the "
              "yardstick (count %.3f, record %.3f, plan %.3f, finish %.3f)" %
              (title, yard, total, total / yard, added, added / yard, med["count"] / yard,
               med["record (counts again)"] / yard, med["plan"] / yard, med["finish"] / yard))


if __name__ == "__main__":
    main()
