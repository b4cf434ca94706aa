#!/usr/bin/env python3
"""Timing of seek tables (zlz4f_batch_append_seek_table, zlz4f_batch_load_seek_table, zlz4f_batch_concat, DESIGN.md section
4.4l) against the calls whose work they store or follow, on the same files.

Input (bench.make_device_blocks, D-text): --frames chunks of 64 KiB, each compressed on the device as a one-block frame and
laid back to back (zlz4f_batch_concat) into files of the --groupings, e.g. 4096x16 = 4 096 files of 16 members.

 (a) load     count + record of zlz4f_batch_load_seek_table against what a reader without a table runs: the split (count +
              record) and zlz4f_batch_file_index; then 4 KiB of every file through either set of tables.
 (b) append   zlz4f_batch_append_seek_table against the index it follows.
 (c) write    what compressFiles adds to compressFrameBatch over the same chunks: concat, split, index, append.

The steps alternate inside one process: HIP events around each call, warm-up, --reps alternations; median and spread
(min .. max) per call.  Before timing, the loaded tables are compared with the computed ones and the decoded bytes with the
input.  Writes the table to --out (profiles/r35_seek_table.md)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import numpy as np
    import torch
    import zig_lz4_amd as zl
    from bench import make_device_blocks
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=65536)
    ap.add_argument("--groupings", default="4096x16,64x1024")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r35_seek_table.md"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    assert zl.device_available(), "needs a gfx950 device"
    lz4f = zl.lz4f
    n, bs = a.frames, 65536
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def alternate(calls):
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
            say("| %s | %.3f | %.3f .. %.3f | %d |" % (label, med[label], min(t), max(t), len(t)))
        return med

    def i64(m):
        return torch.zeros(max(1, m), dtype=torch.int64, device=dev)[:m]

    def full(m, v):
        return torch.full((m,), v, dtype=torch.int64, device=dev)

    def u8(m):
        return torch.empty(max(16, m), dtype=torch.uint8, device=dev)

    ar = torch.arange(n, dtype=torch.int64, device=dev)
    raw = make_device_blocks("text", n, bs, dev, seed=1).reshape(-1)
    prefs = zl.Prefs()
    prefs.block_mode = 1
    stride = lz4f.compressFrameBound(bs, prefs)
    frames = torch.empty(n * stride, dtype=torch.uint8, device=dev)
    f_off, f_cap, f_len, chunk_len = ar * stride, full(n, stride), i64(n), full(n, bs)
    cws = u8(lz4f.compressFrameBatchWorkspace(n, n, prefs))

    def compress():
        lz4f.compressFrameBatch(raw, ar * bs, chunk_len, frames, f_off, f_cap, f_len, prefs, 0, n, cws)

    compress()
    torch.cuda.synchronize()
    assert bool((f_len > 0).all()), "compression failed"
    say("# Seek tables on the MI355X (`tools/time_seek_table.py`)")
    say()
    say("%d chunks of 64 KiB of D-text, each a one-block frame; times in ms, median of %d alternations (min .. max)." % (n, a.reps))

    for grouping in a.groupings.split(","):
        nbuf, k = (int(x) for x in grouping.split("x"))
        assert nbuf * k == n
        T = lz4f.seekTableBound(k, k)
        first = torch.arange(nbuf + 1, dtype=torch.int64, device=dev) * k
        slot = (k * stride + T + 15) & ~15
        files = torch.zeros(nbuf * slot, dtype=torch.uint8, device=dev)
        file_off, file_cap = torch.arange(nbuf, dtype=torch.int64, device=dev) * slot, full(nbuf, slot)
        joined, kws = i64(nbuf), u8(lz4f.concatBatchWorkspace(n))

        def concat():
            lz4f.concatBatch(frames, f_off, f_len, first, files, file_off, file_cap, joined, kws)

        concat()
        torch.cuda.synchronize()
        assert bool((joined > 0).all()), "concat failed"
        LEG = lz4f.SPLIT_LEGACY
        count, totals = i64(nbuf), i64(4)
        member = torch.zeros((n + nbuf, 3), dtype=torch.int64, device=dev)
        item_first, item_off, item_len, leg_len, sres = i64(nbuf + 1), i64(n + nbuf), i64(n + nbuf), i64(n + nbuf), i64(nbuf)
        cap = n + nbuf
        index = torch.zeros((cap, 2), dtype=torch.int64, device=dev)
        idx_off, idx_n, ares = i64(nbuf + 1), i64(nbuf), i64(nbuf)
        src_len = joined.clone()
        state = {"k": k, "totals": (n, n, 0, 0)}
        iws = u8(max(lz4f.fileIndexBatchWorkspace(nbuf, (n, n, 0, 0)), lz4f.fileIndexBatchWorkspace(nbuf, (n + nbuf, n, 0, 0))))

        def split():
            mem_off = torch.arange(nbuf, dtype=torch.int64, device=dev) * state["k"]
            state["mem_off"] = mem_off
            lz4f.multiframeSplitBatchEx(files, file_off, src_len, count, totals, split_flags=LEG)
            lz4f.multiframeSplitBatchEx(files, file_off, src_len, count, totals, member, mem_off, full(nbuf, state["k"]),
                                        item_first, item_off, item_len, sres, LEG, leg_len)

        def file_index():
            lz4f.fileIndexBatch(files, file_off, src_len, member, state["mem_off"], sres, item_first, item_off, item_len, leg_len,
                                state["totals"], index, idx_off, idx_n, cap, iws)

        def append():
            lz4f.appendSeekTableBatch(files, file_off, joined, file_cap, member, state["mem_off"], sres, index, idx_off, idx_n, ares)

        split()
        file_index()
        append()
        torch.cuda.synchronize()
        assert bool((ares == joined + T).all()) and bool((idx_n == k).all()), "append"
        say()
        say("## %s: %d files of %d members, table %d bytes per file (%.2f %% of %.1f MiB compressed)" % (
            grouping, nbuf, k, T, 100.0 * nbuf * T / float(joined.sum()), float(joined.sum()) / 2**20))
        say()
        say("| call | median | min .. max | runs |")
        say("|---|---|---|---|")
        write = alternate([("(c) compressFrameBatch over the chunks", compress), ("(c) concat", concat),
                           ("(c) split: count + record, files without a table", split),
                           ("(b) file index, files without a table", file_index), ("(b) append", append)])
        # the files with their table: what a reader sees
        src_len = ares.clone()
        state["k"], state["totals"] = k + 1, (n + nbuf, n, 0, 0)
        split()
        file_index()
        torch.cuda.synchronize()
        assert bool((sres == k + 1).all()) and bool((idx_n == k).all()), "the split and index of the files with a table"
        l_count, l_totals = i64(nbuf), i64(2)
        l_member = torch.zeros((n + nbuf, 3), dtype=torch.int64, device=dev)
        l_index = torch.zeros((cap, 2), dtype=torch.int64, device=dev)
        l_idx_off, l_idx_n, l_sres = i64(nbuf + 1), i64(nbuf), i64(nbuf)
        l_mem_off, l_mem_cap = torch.arange(nbuf, dtype=torch.int64, device=dev) * (k + 1), full(nbuf, k + 1)

        def load():
            lz4f.loadSeekTableBatch(files, file_off, src_len, l_count, l_totals)
            lz4f.loadSeekTableBatch(files, file_off, src_len, l_count, l_totals, l_member, l_mem_off, l_mem_cap, l_sres, l_index,
                                    l_idx_off, l_idx_n, cap)

        load()
        torch.cuda.synchronize()
        assert l_totals.tolist() == [n + nbuf, n + nbuf], "the load's totals"
        assert torch.equal(l_member, member) and torch.equal(l_index, index) and torch.equal(l_idx_off, idx_off), "loaded == computed"
        assert torch.equal(l_idx_n, idx_n) and torch.equal(l_sres, sres)
        f = np.arange(nbuf, dtype=np.uint64)
        a0 = np.full(nbuf, (k // 2) * bs + 1000, dtype=np.uint64)
        rng = np.stack([f, a0, a0 + 4096], 1)
        d_range = torch.from_numpy(np.ascontiguousarray(rng).view(np.int64)).to(dev)
        r_off, r_cap, r_tot, skip, rres = i64(nbuf), i64(nbuf), i64(2), i64(nbuf), i64(nbuf)
        lz4f.planFrameRanges(l_index, l_idx_off, l_idx_n, d_range, r_off, r_cap, r_tot)
        arena, items = r_tot.tolist()
        r_dst, rws = u8(arena), u8(lz4f.decompressFileRangeBatchWorkspace(nbuf, items))

        def read_loaded():
            lz4f.planFrameRanges(l_index, l_idx_off, l_idx_n, d_range, r_off, r_cap, r_tot)
            lz4f.decompressFileRangeBatch(files, file_off, src_len, l_index, l_idx_off, l_idx_n, l_member, l_mem_off, l_sres, d_range,
                                          r_dst, r_off, r_cap, skip, rres, items, rws)

        read_loaded()
        torch.cuda.synchronize()
        assert bool((rres == 4096).all()), "r4k"
        for r in range(0, nbuf, max(1, nbuf // 64)):
            o = int(r_off[r]) + int(skip[r])
            lo = r * k * bs + int(a0[r])
            assert torch.equal(r_dst[o:o + 4096], raw[lo:lo + 4096]), r
        read = alternate([("(a) split: count + record, files with a table", split), ("(a) file index, files with a table", file_index),
                          ("(a) load: count + record", load), ("(a) 4 KiB of every file: plan + file range decode, loaded tables", read_loaded)])
        walk = read["(a) split: count + record, files with a table"] + read["(a) file index, files with a table"]
        ld, r4 = read["(a) load: count + record"], read["(a) 4 KiB of every file: plan + file range decode, loaded tables"]
        say()
        say("(a) open and read 4 KiB: %.3f ms through split + index, %.3f ms through the load (%.1fx); load / (split + index) = %.4f"
            % (walk + r4, ld + r4, (walk + r4) / (ld + r4), ld / walk))
        say("(b) append / index = %.4f" % (write["(b) append"] / write["(b) file index, files without a table"]))
        extra = sum(v for lbl, v in write.items() if not lbl.startswith("(c) compressFrameBatch"))
        say("(c) concat + split + index + append = %.3f ms = %.3f of compressFrameBatch" % (
            extra, extra / write["(c) compressFrameBatch over the chunks"]))
        del files, member, index, l_member, l_index
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
