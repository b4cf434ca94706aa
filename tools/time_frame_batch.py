#!/usr/bin/env python3
"""Time the batch frame calls (zlz4f_batch_compress_frame / zlz4f_batch_decompress_frame) with HIP events: 3 warm-up
runs, then the median of 10 timed runs per measurement.

  (a) configs[1] shape: 65 536 x 64 KiB D-text frames, compress and decompress, checksums off and on, next to
      zlz4_batch_compress_fast / zlz4_batch_decompress_safe on the same 64 KiB blocks;
  (b) 262 144 x 4 KiB D-text frames with block and content checksums (block batch on the same blocks for scale);
  (c) the per-frame cost of a loop of zlz4f_compress_frame_device / zlz4f_decompress_frame_device over 1 000 of the
      4 KiB frames of (b) (each call synchronises; wall clock), against the batch's cost per frame from (b).

  python tools/time_frame_batch.py [a|b|c|all]
"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import bench
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
    return statistics.median(ts), ts


def prefs(checksums):
    p = zl.Prefs()
    p.block_checksum = p.content_checksum = 1 if checksums else 0
    return p


class Setup:
    """n frames of `size` bytes back to back in one tensor; frame slots of compressFrameBound, decode slots of `size`."""

    def __init__(self, n, size, p):
        self.n, self.size, self.p = n, size, p
        self.inp = bench.make_device_blocks("text", n, size, dev, seed=1).reshape(-1)
        ar = torch.arange(n, dtype=torch.int64, device=dev)
        fb = zl.lz4f.compressFrameBound(size, p)
        self.src_off, self.src_len = ar * size, torch.full((n,), size, dtype=torch.int64, device=dev)
        self.frm = torch.empty(n * fb, dtype=torch.uint8, device=dev)
        self.frm_off, self.frm_cap = ar * fb, torch.full((n,), fb, dtype=torch.int64, device=dev)
        self.out = torch.empty(n * size, dtype=torch.uint8, device=dev)
        self.cres = torch.empty(n, dtype=torch.int64, device=dev)
        self.dres = torch.empty(n, dtype=torch.int64, device=dev)
        self.mb = n * ((size + 65535) // 65536)
        self.cws = torch.empty(zl.lz4f.compressFrameBatchWorkspace(n, self.mb, p), dtype=torch.uint8, device=dev)
        self.dws = torch.empty(zl.lz4f.decompressFrameBatchWorkspace(n, self.mb), dtype=torch.uint8, device=dev)

    def compress(self):
        zl.lz4f.compressFrameBatch(self.inp, self.src_off, self.src_len, self.frm, self.frm_off, self.frm_cap, self.cres,
                                   self.p, 0, self.mb, self.cws)

    def decompress(self):
        zl.lz4f.decompressFrameBatch(self.frm, self.frm_off, self.cres, self.out, self.src_off, self.src_len, self.dres,
                                     self.mb, self.dws)

    def check(self):
        torch.cuda.synchronize()
        return bool((self.cres > 0).all()) and bool((self.dres == self.size).all()) and bool(torch.equal(self.out, self.inp))


def block_batch(s):
    """zlz4_batch_compress_fast / zlz4_batch_decompress_safe on the frames' bytes as plain blocks."""
    n, size = s.n, s.size
    slot = (zl.compressBound(size) + 15) // 16 * 16
    ar = torch.arange(n, dtype=torch.int64, device=dev)
    in_len = torch.full((n,), size, dtype=torch.int32, device=dev)
    comp = torch.empty(n * slot, dtype=torch.uint8, device=dev)
    cap = torch.full((n,), slot, dtype=torch.int32, device=dev)
    res = torch.empty(n, dtype=torch.int64, device=dev)
    out = torch.empty(n * size, dtype=torch.uint8, device=dev)
    dres = torch.empty(n, dtype=torch.int64, device=dev)
    clen = torch.empty(n, dtype=torch.int32, device=dev)
    dcap = torch.full((n,), size, dtype=torch.int32, device=dev)

    def c():
        zl.batch_compress_fast(s.inp, ar * size, in_len, comp, ar * slot, cap, res, size, 1)
    tc, _ = timed(c)
    clen.copy_(res.to(torch.int32))

    def d():
        zl.batch_decompress_safe(comp, ar * slot, clen, out, ar * size, dcap, dres)
    td, _ = timed(d)
    ok = bool(torch.equal(out, s.inp))
    del comp, out
    return tc, td, ok


def report(tag, s, tc, td, bc=None, bd=None):
    gib = s.n * s.size / 2**30
    line = "%s: compress %.3f ms (%.1f GiB/s), decompress %.3f ms (%.1f GiB/s)" % (tag, tc, gib / tc * 1e3, td, gib / td * 1e3)
    if bc is not None:
        line += "; block batch %.3f / %.3f ms -> frame/block %.3f / %.3f" % (bc, bd, tc / bc, td / bd)
    print(line, flush=True)


def case_a():
    for cks in (False, True):
        s = Setup(65536, 65536, prefs(cks))
        tc, tcs = timed(s.compress)
        td, tds = timed(s.decompress)
        ok = s.check()
        bc, bd, bok = block_batch(s)
        report("(a) 65536 x 64 KiB D-text, checksums %s" % ("on" if cks else "off"), s, tc, td, bc, bd)
        print("    round trip ok=%s, block batch ok=%s, ratio %.3f; ms compress %s / decompress %s"
              % (ok, bok, s.n * s.size / float(s.cres.sum()), ["%.2f" % x for x in tcs], ["%.2f" % x for x in tds]), flush=True)
        del s
        torch.cuda.empty_cache()


def case_b():
    s = Setup(262144, 4096, prefs(True))
    tc, _ = timed(s.compress)
    td, _ = timed(s.decompress)
    ok = s.check()
    bc, bd, _ = block_batch(s)
    report("(b) 262144 x 4 KiB D-text, block + content checksums", s, tc, td, bc, bd)
    print("    round trip ok=%s; per frame: compress %.3f us, decompress %.3f us"
          % (ok, tc * 1e3 / s.n, td * 1e3 / s.n), flush=True)
    return s, tc, td


def case_c(s=None, tc=None, td=None):
    if s is None:
        s, tc, td = case_b()
    n, size, p = 1000, s.size, s.p
    fb = zl.lz4f.compressFrameBound(size, p)
    frm = torch.empty(n * fb, dtype=torch.uint8, device=dev)
    out = torch.empty(n * size, dtype=torch.uint8, device=dev)
    lens = [0] * n
    src = [s.inp[k * size:(k + 1) * size] for k in range(n)]
    fr = [frm[k * fb:(k + 1) * fb] for k in range(n)]
    dst = [out[k * size:(k + 1) * size] for k in range(n)]

    def loop_c():
        for k in range(n):
            lens[k] = zl.lz4f.compressFrameDevice(src[k], fr[k], p)

    def loop_d():
        for k in range(n):
            zl.lz4f.decompressFrameDevice(fr[k], lens[k], dst[k])

    def wall(fn):
        for _ in range(WARM):
            fn()
        ts = []
        for _ in range(RUNS):
            torch.cuda.synchronize()
            t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts)
    lc, ld = wall(loop_c), wall(loop_d)
    ok = bool(torch.equal(out, s.inp[:n * size]))
    bcf, bdf = tc * 1e3 / s.n, td * 1e3 / s.n
    print("(c) loop of %d single-frame device calls (4 KiB, checksums on): compress %.1f us / frame, decompress %.1f us / "
          "frame (ok=%s); batch of (b): %.3f / %.3f us / frame -> %.0fx / %.0fx"
          % (n, lc * 1e3 / n, ld * 1e3 / n, ok, bcf, bdf, lc * 1e3 / n / bcf, ld * 1e3 / n / bdf), flush=True)


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    print("device: %s" % torch.cuda.get_device_name(0), flush=True)
    if which in ("a", "all"):
        case_a()
    if which in ("b", "c", "all"):
        s, tc, td = case_b()
        if which in ("c", "all"):
            case_c(s, tc, td)
