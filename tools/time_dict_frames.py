#!/usr/bin/env python3
"""Time the dictionary frame calls (zlz4f_batch_compress_frame_using_dict / zlz4f_batch_decompress_frame_using_dict) with HIP
events: 3 warm-up runs, then the median of 10 timed runs per measurement.

  (a) 65 536 records of 4 KiB D-text against ONE shared dictionary of 16 KiB, and of 64 KiB (independent-declared frames,
      max_src_len = 4096): frame compress and frame decode next to the block-level calls on the same records --
      zlz4_batch_compress_fast_using_dict after one zlz4_batch_load_dict, and zlz4_batch_decompress_safe_using_dict;
  (b) the same records as linked-declared frames (one block each: the same compressor launch, the one-wavefront-per-frame
      decoder);
  (c) 1 024 linked frames of 256 KiB against a 64 KiB dictionary, next to the linked calls without a dictionary
      (ZLZ4F_BATCH_LINK_BLOCKS / ZLZ4F_DECODE_LINKED).

  python tools/time_dict_frames.py [a|b|c|all]
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import datagen as dg
import zig_lz4_amd as zl

dev = torch.device("cuda:0")
WARM, RUNS = 3, 10


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(RUNS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def text_records(n, size):
    """n records of `size` bytes of D-text: a pool of 16 MiB of text (tests/datagen.py), repeated.  The dictionaries are text
    of the same generator, so the records find matches in them."""
    pool = min(n * size, 16 << 20)
    t = torch.from_numpy(dg.text_bytes(pool, 1)).to(dev)
    return t.repeat(n * size // pool)


class Setup:
    """n frames of `size` bytes back to back, one shared dictionary of `dsize` bytes (dsize 0: the calls without one)."""

    def __init__(self, n, size, dsize, block_mode, max_src_len):
        self.n, self.size, self.dsize = n, size, dsize
        self.p = zl.Prefs()
        self.p.block_mode = block_mode
        self.inp = text_records(n, size)
        self.dict = torch.from_numpy(dg.text_bytes(max(dsize, 16), 77)).to(dev)[:max(dsize, 1)]
        self.dict_off = torch.zeros(1, dtype=torch.int64, device=dev)
        self.dict_len = torch.full((1,), dsize, dtype=torch.int32, device=dev)
        ar = torch.arange(n, dtype=torch.int64, device=dev)
        fb = zl.lz4f.compressFrameBound(size, self.p)
        self.src_off, self.src_len = ar * size, torch.full((n,), size, dtype=torch.int64, device=dev)
        self.frm = torch.empty(n * fb, dtype=torch.uint8, device=dev)
        self.frm_off, self.frm_cap = ar * fb, torch.full((n,), fb, dtype=torch.int64, device=dev)
        self.out = torch.empty(n * size, dtype=torch.uint8, device=dev)
        self.cres = torch.empty(n, dtype=torch.int64, device=dev)
        self.dres = torch.empty(n, dtype=torch.int64, device=dev)
        self.mb = n * ((size + 65535) // 65536)
        self.max_src_len = max_src_len
        if dsize:
            self.cws = torch.empty(zl.lz4f.compressFrameUsingDictBatchWorkspace(n, self.mb, self.p, 0, 1, max_src_len, dsize),
                                   dtype=torch.uint8, device=dev)
            self.dws = torch.empty(zl.lz4f.decompressFrameUsingDictBatchWorkspace(n, self.mb), dtype=torch.uint8, device=dev)
        else:
            self.cws = torch.empty(zl.lz4f.compressFrameBatchWorkspace(n, self.mb, self.p, zl.lz4f.BATCH_LINK_BLOCKS),
                                   dtype=torch.uint8, device=dev)
            self.dws = torch.empty(zl.lz4f.decompressFrameBatchWorkspace(n, self.mb, zl.lz4f.DECODE_LINKED),
                                   dtype=torch.uint8, device=dev)

    def compress(self):
        if self.dsize:
            zl.lz4f.compressFrameUsingDictBatch(self.inp, self.src_off, self.src_len, self.frm, self.frm_off, self.frm_cap,
                                                self.cres, self.dict, self.dict_off, self.dict_len, None, self.p, 0, self.mb,
                                                self.max_src_len, self.dsize, self.cws)
        else:
            zl.lz4f.compressFrameBatch(self.inp, self.src_off, self.src_len, self.frm, self.frm_off, self.frm_cap, self.cres,
                                       self.p, zl.lz4f.BATCH_LINK_BLOCKS, self.mb, self.cws)

    def decompress(self):
        if self.dsize:
            zl.lz4f.decompressFrameUsingDictBatch(self.frm, self.frm_off, self.cres, self.out, self.src_off, self.src_len,
                                                  self.dres, self.dict, self.dict_off, self.dict_len, None, self.mb, self.dws)
        else:
            zl.lz4f.decompressFrameBatch(self.frm, self.frm_off, self.cres, self.out, self.src_off, self.src_len, self.dres,
                                         self.mb, self.dws, flags=zl.lz4f.DECODE_LINKED)

    def check(self):
        torch.cuda.synchronize()
        return bool((self.cres > 0).all()) and bool((self.dres == self.size).all()) and bool(torch.equal(self.out, self.inp))


def block_calls(s):
    """The records as plain blocks against the shared dictionary: load_dict once, then the dictionary compressor and the
    dictionary decoder (the calls of the parent commit: the yardstick)."""
    n, size = s.n, s.size
    slot = (zl.compressBound(size) + 15) // 16 * 16
    ar = torch.arange(n, dtype=torch.int64, device=dev)
    in_len = torch.full((n,), size, dtype=torch.int32, device=dev)
    comp = torch.empty(n * slot, dtype=torch.uint8, device=dev)
    cap = torch.full((n,), slot, dtype=torch.int32, device=dev)
    res = torch.empty(n, dtype=torch.int64, device=dev)
    out = torch.empty(n * size, dtype=torch.uint8, device=dev)
    dres = torch.empty(n, dtype=torch.int64, device=dev)
    dcap = torch.full((n,), size, dtype=torch.int32, device=dev)
    table = torch.empty(zl.STREAM_TABLE_ENTRIES, dtype=torch.int32, device=dev)
    lres = torch.empty(1, dtype=torch.int64, device=dev)
    d_off = torch.zeros(n, dtype=torch.int64, device=dev)
    d_len = torch.full((n,), s.dsize, dtype=torch.int32, device=dev)
    t_idx = torch.zeros(n, dtype=torch.int32, device=dev)

    def c():
        zl.batch_load_dict(s.dict, s.dict_off, s.dict_len, table, lres)
        zl.batch_compress_fast_using_dict(s.inp, ar * size, in_len, comp, ar * slot, cap, s.dict, d_off, d_len, table, t_idx, res,
                                          size, s.dsize, 1)
    tc = timed(c)
    clen = res.to(torch.int32)

    def d():
        zl.batch_decompress_safe_using_dict(comp, ar * slot, clen, out, ar * size, dcap, s.dict, d_off, d_len, dres)
    td = timed(d)
    return tc, td, bool(torch.equal(out, s.inp)), s.n * s.size / float(res.sum())


def report(tag, s, tc, td, ok):
    gib = s.n * s.size / 2**30
    print("%s: compress %.3f ms (%.1f GiB/s), decompress %.3f ms (%.1f GiB/s), round trip ok=%s, ratio %.3f"
          % (tag, tc, gib / tc * 1e3, td, gib / td * 1e3, ok, s.n * s.size / float(s.cres.sum())), flush=True)


def records(block_mode, tag):
    for dsize in (16384, 65536):
        s = Setup(65536, 4096, dsize, block_mode, 4096)
        tc, td = timed(s.compress), timed(s.decompress)
        report("%s 65536 x 4 KiB, %d KiB dictionary, frames" % (tag, dsize >> 10), s, tc, td, s.check())
        bc, bd, bok, ratio = block_calls(s)
        print("    block calls: compress %.3f ms, decompress %.3f ms (ok=%s, ratio %.3f) -> frame/block %.3f / %.3f"
              % (bc, bd, bok, ratio, tc / bc, td / bd), flush=True)
        del s
        torch.cuda.empty_cache()


def case_c():
    out = []
    for dsize in (65536, 0):
        s = Setup(1024, 262144, dsize, 0, 0)
        tc, td = timed(s.compress), timed(s.decompress)
        report("(c) 1024 x 256 KiB linked frames, %s" % ("64 KiB dictionary" if dsize else "no dictionary (the linked calls)"),
               s, tc, td, s.check())
        out.append((tc, td))
        del s
        torch.cuda.empty_cache()
    print("    with / without dictionary: compress %.3f, decompress %.3f" % (out[0][0] / out[1][0], out[0][1] / out[1][1]),
          flush=True)


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    print("device: %s" % torch.cuda.get_device_name(0), flush=True)
    if which in ("a", "all"):
        records(1, "(a) independent")
    if which in ("b", "all"):
        records(0, "(b) linked-declared")
    if which in ("c", "all"):
        case_c()
