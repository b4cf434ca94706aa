#!/usr/bin/env python3
"""Timing of linked-block frames on the GPU (profiles/r12_linked_frames.md): HIP events around
each batch call, warm-up, median of --reps.

Workload: --frames frames of --blocks x 64 KiB D-text each (64 distinct frames, repeated), compressed
  linked       zlz4f_batch_compress_frame with ZLZ4F_BATCH_LINK_BLOCKS, decoded by zlz4f_batch_decompress_frame_ex with
               ZLZ4F_DECODE_LINKED, sized by zlz4f_batch_frame_decompressed_size_ex with the flag
  independent  the yardstick: the same inputs through the unchanged zlz4f_batch_compress_frame /
               zlz4f_batch_decompress_frame / zlz4f_batch_frame_decompressed_size, block_mode 1, in the same process
Prints the compressed sizes, the ratio, and time and GiB/s (of decoded bytes) for both directions and the size query.
Nothing gates on these figures."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, warm, reps):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def main():
    import torch
    import datagen as dg
    import zig_lz4_amd as zl
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    nf, B = a.frames, 65536
    flen = a.blocks * B
    uniq = min(64, nf)
    raw = torch.from_numpy(np.ascontiguousarray(dg.make_blocks("text", uniq * a.blocks, B, seed=1)).reshape(-1)).to(dev)
    i64 = lambda x: torch.tensor(x, dtype=torch.int64, device=dev)  # noqa: E731
    s_off, s_len = i64([(f % uniq) * flen for f in range(nf)]), i64([flen] * nf)
    max_blocks = nf * a.blocks
    gib = nf * flen / 2**30
    d_out = torch.empty(nf * flen, dtype=torch.uint8, device=dev)
    o_off, o_cap = i64([f * flen for f in range(nf)]), i64([flen] * nf)
    print("%d frames of %d x 64 KiB D-text (%.2f GiB), median of %d" % (nf, a.blocks, gib, a.reps))
    rows = {}
    for name, mode, cflags, dflags in (("independent", 1, 0, 0), ("linked", 0, zl.lz4f.BATCH_LINK_BLOCKS, zl.lz4f.DECODE_LINKED)):
        p = zl.Prefs()
        p.block_mode = mode
        cap = zl.lz4f.compressFrameBound(flen, p)
        d_frm = torch.empty(nf * cap, dtype=torch.uint8, device=dev)
        f_off, f_cap = i64([f * cap for f in range(nf)]), i64([cap] * nf)
        cres = torch.empty(nf, dtype=torch.int64, device=dev)
        dres = torch.empty(nf, dtype=torch.int64, device=dev)
        qres = torch.empty(nf, dtype=torch.int64, device=dev)
        cws = torch.empty(zl.lz4f.compressFrameBatchWorkspace(nf, max_blocks, p, cflags), dtype=torch.uint8, device=dev)
        dws = torch.empty(zl.lz4f.decompressFrameBatchWorkspace(nf, max_blocks, dflags), dtype=torch.uint8, device=dev)
        qws = torch.empty(zl.lz4f.frameDecompressedSizeBatchWorkspace(nf, max_blocks, dflags), dtype=torch.uint8, device=dev)
        tc = timed(lambda: zl.lz4f.compressFrameBatch(raw, s_off, s_len, d_frm, f_off, f_cap, cres, p, cflags, max_blocks, cws),
                   a.warmup, a.reps)
        csum = int(cres.sum())
        assert int((cres < 0).sum()) == 0
        td = timed(lambda: zl.lz4f.decompressFrameBatch(d_frm, f_off, cres, d_out, o_off, o_cap, dres, max_blocks, dws,
                                                        flags=dflags), a.warmup, a.reps)
        assert bool((dres == flen).all()) and torch.equal(d_out[:uniq * flen], raw)
        tq = timed(lambda: zl.lz4f.frameDecompressedSizeBatch(d_frm, f_off, cres, qres, max_blocks, qws, flags=dflags),
                   a.warmup, a.reps)
        assert bool((qres == flen).all())
        rows[name] = (csum, tc, td, tq)
        print("%-11s  compressed %d bytes (ratio %.3f)  compress %.3f ms %.1f GiB/s  decode %.3f ms %.1f GiB/s  "
              "size query %.3f ms" % (name, csum, nf * flen / csum, tc, gib / tc * 1e3, td, gib / td * 1e3, tq))
        del d_frm, cws, dws, qws
    i, l = rows["independent"], rows["linked"]
    print("linked / independent: size %.3f  compress time %.2fx  decode time %.2fx  size query time %.2fx"
          % (l[0] / i[0], l[1] / i[1], l[2] / i[2], l[3] / i[3]))


if __name__ == "__main__":
    main()
