#!/usr/bin/env python3
"""Timing of dictionary .lz4 files (zlz4f_batch_file_index_using_dict, zlz4f_batch_decompress_file_range_using_dict and the
dicts= keywords of lz4f.compressFiles / loadFileIndex) against the plain calls on the same inputs
written without a dictionary, in the same build and process.

 (a) the shape of tools/time_file_range.py and tools/time_seek_table.py: --frames chunks of 64 KiB of text (a pool of
     --pool distinct blocks of tests/datagen.py text, repeated on the device: a shared dictionary needs the shared
     vocabulary, which bench.make_device_blocks' per-block byte substitution takes away), each a one-block frame, --files
     files of frames/files members; one shared dictionary of 64 KiB of the same text.  Index, 4 KiB of every file, and
     ranges that cover every file, with and without the dictionary.
 (b) a record store: --records records of 4 KiB written by lz4f.compressFiles(frame_size=4096, dicts=...) as --stores files;
     file sizes with and without the dictionary; load table + one record per file against split + index + one record.

The steps alternate inside one process: HIP events (a) or the wall clock around synchronised calls (b: the Python one-liners
stage from host memory), warm-up, --reps alternations; median and spread (min .. max) per call.  Before timing, the decoded
bytes are compared with the input.  Writes the table to --out."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import numpy as np
    import torch
    import zig_lz4_amd as zl
    import datagen as dg
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=65536)
    ap.add_argument("--files", type=int, default=4096)
    ap.add_argument("--records", type=int, default=65536)
    ap.add_argument("--stores", type=int, default=64)
    ap.add_argument("--pool", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r36_file_dicts_timing.md"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    assert zl.device_available(), "needs a gfx950 device"
    lz4f = zl.lz4f
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

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def alternate(calls, clock=timed):
        for _ in range(a.warmup):
            for _, fn in calls:
                fn()
        torch.cuda.synchronize()
        times = [[] for _ in calls]
        for _ in range(a.reps):
            for t, (_, fn) in zip(times, calls):
                t.append(clock(fn))
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

    say("# Dictionary .lz4 files on the MI355X (`tools/time_file_dict.py`)")
    say()

    # ------------------------------------------------------------------ (a) files of one-block 64 KiB frames
    n, bs, nbuf = a.frames, 65536, a.files
    k = n // nbuf
    assert nbuf * k == n
    ar = torch.arange(n, dtype=torch.int64, device=dev)
    pool_host = dg.make_blocks("text", a.pool, bs, seed=1)
    pool = torch.from_numpy(np.ascontiguousarray(pool_host)).to(dev)
    raw = pool[ar % a.pool].reshape(-1)
    d_dict = torch.from_numpy(np.ascontiguousarray(dg.make_blocks("text", 1, bs, seed=2))).to(dev).reshape(-1)
    dict_off, dict_len = i64(1), torch.tensor([bs], dtype=torch.int32, device=dev)
    prefs = zl.Prefs()
    prefs.block_mode = 1
    stride = lz4f.compressFrameBound(bs, prefs)
    f_off, f_cap, chunk_len = ar * stride, full(n, stride), full(n, bs)
    first = torch.arange(nbuf + 1, dtype=torch.int64, device=dev) * k
    slot = (k * stride + 15) & ~15
    file_off, file_cap = torch.arange(nbuf, dtype=torch.int64, device=dev) * slot, full(nbuf, slot)
    f = np.arange(nbuf, dtype=np.uint64)
    a0 = np.full(nbuf, (k // 2) * bs + 1000, dtype=np.uint64)
    r4k = torch.from_numpy(np.ascontiguousarray(np.stack([f, a0, a0 + 4096], 1)).view(np.int64)).to(dev)
    rall = torch.from_numpy(np.ascontiguousarray(np.stack([f, a0 * 0, a0 * 0 + k * bs], 1)).view(np.int64)).to(dev)
    say("## (a) %d files of %d one-block 64 KiB text frames (a pool of %d distinct blocks, repeated), one shared dictionary "
        "of 64 KiB" % (nbuf, k, a.pool))
    say()
    say("times in ms, median of %d alternations (min .. max); HIP events around each call" % a.reps)
    say()
    calls, keep = [], []
    for with_dict in (False, True):
        tag = "dictionary" if with_dict else "plain"
        frames, f_len = torch.empty(n * stride, dtype=torch.uint8, device=dev), i64(n)
        if with_dict:
            lz4f.compressFrameUsingDictBatch(raw, ar * bs, chunk_len, frames, f_off, f_cap, f_len, d_dict, dict_off, dict_len,
                                             None, prefs, 0, n, max_src_len=bs)
        else:
            lz4f.compressFrameBatch(raw, ar * bs, chunk_len, frames, f_off, f_cap, f_len, prefs, 0, n)
        files, joined = torch.zeros(nbuf * slot, dtype=torch.uint8, device=dev), i64(nbuf)
        lz4f.concatBatch(frames, f_off, f_len, first, files, file_off, file_cap, joined)
        torch.cuda.synchronize()
        assert bool((joined > 0).all()), "compress / concat failed"
        say("%s files: %.1f MiB compressed (ratio %.3f)" % (tag, float(joined.sum()) / 2**20, float(joined.sum()) / (n * bs)))
        del frames
        sp = lz4f.splitStaged(files, file_off, joined, legacy=True)
        totals = (sp.nitems, sp.max_blocks, sp.nlegacy, sp.legacy_blocks)
        cap = n + nbuf
        index, idx_off, idx_n = torch.zeros((cap, 2), dtype=torch.int64, device=dev), i64(nbuf + 1), i64(nbuf)
        iws = u8(lz4f.fileIndexUsingDictBatchWorkspace(nbuf, totals))
        r_off, r_cap, r_tot, skip, rres = i64(nbuf), i64(nbuf), i64(2), i64(nbuf), i64(nbuf)

        def index_fn(sp=sp, totals=totals, index=index, idx_off=idx_off, idx_n=idx_n, iws=iws, with_dict=with_dict):
            if with_dict:
                lz4f.fileIndexUsingDictBatch(sp.d_src, sp.src_off, sp.src_len, sp.member, sp.mem_off, sp.result, sp.item_first,
                                             sp.item_off, sp.item_len, sp.leg_len, totals, index, idx_off, idx_n, dict_len, None,
                                             cap, iws)
            else:
                lz4f.fileIndexBatch(sp.d_src, sp.src_off, sp.src_len, sp.member, sp.mem_off, sp.result, sp.item_first,
                                    sp.item_off, sp.item_len, sp.leg_len, totals, index, idx_off, idx_n, cap, iws)

        index_fn()
        torch.cuda.synchronize()
        assert bool((idx_n == k).all()), "the index"
        calls.append(("file index, %s" % tag, index_fn))
        for name, d_range, want in (("4 KiB of every file", r4k, 4096), ("all of every file", rall, k * bs)):
            lz4f.planFrameRanges(index, idx_off, idx_n, d_range, r_off, r_cap, r_tot)
            arena, items = r_tot.tolist()
            r_dst = u8(arena)
            rws = u8(lz4f.decompressFileRangeUsingDictBatchWorkspace(nbuf, items))

            def read(sp=sp, index=index, idx_off=idx_off, idx_n=idx_n, d_range=d_range, r_dst=r_dst, rws=rws, items=items,
                     with_dict=with_dict):
                lz4f.planFrameRanges(index, idx_off, idx_n, d_range, r_off, r_cap, r_tot)
                if with_dict:
                    lz4f.decompressFileRangeUsingDictBatch(sp.d_src, sp.src_off, sp.src_len, index, idx_off, idx_n, sp.member,
                                                           sp.mem_off, sp.result, d_range, r_dst, r_off, r_cap, skip, rres,
                                                           items, d_dict, dict_off, dict_len, None, rws)
                else:
                    lz4f.decompressFileRangeBatch(sp.d_src, sp.src_off, sp.src_len, index, idx_off, idx_n, sp.member,
                                                  sp.mem_off, sp.result, d_range, r_dst, r_off, r_cap, skip, rres, items, rws)

            read()
            torch.cuda.synchronize()
            assert bool((rres == want).all()), name
            lo0 = int(d_range[0, 1])
            for r in range(0, nbuf, max(1, nbuf // 32)):
                o = int(r_off[r]) + int(skip[r])
                lo = r * k * bs + lo0
                assert torch.equal(r_dst[o:o + 4096], raw[lo:lo + 4096]), (name, r)
            calls.append(("%s: plan + file range decode, %s" % (name, tag), read))
            keep.append((r_dst, rws))
        keep.append((files, sp, index))
    say()
    say("| call | median | min .. max | runs |")
    say("|---|---|---|---|")
    med = alternate(calls)
    say()
    for what in ("file index", "4 KiB of every file: plan + file range decode", "all of every file: plan + file range decode"):
        p, d = med["%s, plain" % what], med["%s, dictionary" % what]
        say("%s: dictionary / plain = %.3f" % (what, d / p))
    del keep, calls, raw
    torch.cuda.empty_cache()

    # ------------------------------------------------------------------ (b) a record store of 4 KiB records
    nrec, nst, rs = a.records, a.stores, 4096
    per = nrec // nst
    assert per * nst == nrec
    text = pool_host.reshape(-1).tobytes()
    inputs = [(text[(s * per * rs) % len(text):] + text)[:per * rs] for s in range(nst)]
    dictionary = d_dict.cpu().numpy().tobytes()
    say()
    say("## (b) a record store: %d records of 4 KiB as %d files of %d members (`lz4f.compressFiles(frame_size=4096)`)" % (
        nrec, nst, per))
    say()
    stores = {}
    for tag, kw in (("plain", {}), ("dictionary", {"dicts": [dictionary]})):
        files = lz4f.compressFiles(inputs, prefs, rs, device=dev, **kw)
        assert all(isinstance(x, bytes) for x in files), tag
        stores[tag] = (files, kw)
        say("%s: %.2f MiB for %.0f MiB of input (ratio %.3f), seek tables included" % (
            tag, sum(map(len, files)) / 2**20, nrec * rs / 2**20, sum(map(len, files)) / (nrec * rs)))
    ranges = [(s, (per // 2) * rs, (per // 2 + 1) * rs) for s in range(nst)]
    want = [inputs[s][lo:hi] for s, lo, hi in ranges]
    calls = []
    for tag, (files, kw) in stores.items():
        def via_load(files=files, kw=kw):
            return lz4f.decompressFileRanges(lz4f.loadFileIndex(files, device=dev, **kw), ranges)

        def via_index(files=files, kw=kw):
            return lz4f.decompressFileRanges(lz4f.fileIndex(files, device=dev, **kw), ranges)

        assert via_load() == want and via_index() == want, tag
        calls += [("load table + one record per file, %s" % tag, via_load), ("split + index + one record per file, %s" % tag, via_index)]
    say()
    say("wall clock around synchronised calls, staging from host memory included; ms, median of %d (min .. max)" % a.reps)
    say()
    say("| call | median | min .. max | runs |")
    say("|---|---|---|---|")
    alternate(calls, wall)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
