#!/usr/bin/env python3
"""Time the batch compressDestSize (zlz4_batch_compress_dest_size) with HIP events: 3 warm-up runs, then the median of
10 timed runs per measurement.

  (a) 65 536 x 64 KiB D-text blocks with caps of 16 KiB and 4 KiB, timed alternately in one process against
      zlz4_batch_compress_fast on the same blocks;
  (b) 262 144 x 4 KiB D-text blocks with a 1 KiB cap, against zlz4_batch_compress_fast on the same blocks;
  (c) single-call latency of zlz4_compress_dest_size (host pointers, each call synchronises; wall clock) over 64 of the
      64 KiB blocks with a 16 KiB cap.  Run it with ZLZ4_AMD_LIB pointing at another build of the library to compare.

  python tools/time_dest_size.py [a|b|c|all]
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


def alternate(fns):
    """median of RUNS timed runs of every function, the functions taking turns run by run"""
    for fn in fns:
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(RUNS):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    return [statistics.median(t) for t in ts], ts


class Setup:
    """n D-text blocks of `size` bytes back to back; compressBound slots for the fast batch, `cap`-byte slots and a
    workspace for the dest-size batch"""

    def __init__(self, n, size):
        self.n, self.size = n, size
        self.inp = bench.make_device_blocks("text", n, size, dev, seed=1).reshape(-1)
        ar = torch.arange(n, dtype=torch.int64, device=dev)
        self.ar = ar
        self.in_off, self.in_len = ar * size, torch.full((n,), size, dtype=torch.int32, device=dev)
        slot = (zl.compressBound(size) + 15) // 16 * 16
        self.fslot = slot
        self.fout = torch.empty(n * slot, dtype=torch.uint8, device=dev)
        self.fcap = torch.full((n,), slot, dtype=torch.int32, device=dev)
        self.fres = torch.empty(n, dtype=torch.int64, device=dev)
        self.ws = torch.empty(zl.batch_compress_dest_size_workspace(n, size), dtype=torch.uint8, device=dev)
        self.res = torch.empty(n, dtype=torch.int64, device=dev)
        self.consumed = torch.empty(n, dtype=torch.int32, device=dev)
        self.out = None

    def fast(self):
        zl.batch_compress_fast(self.inp, self.in_off, self.in_len, self.fout, self.ar * self.fslot, self.fcap, self.fres,
                               self.size, 1)

    def dest_size_fn(self, cap):
        out = torch.empty(self.n * cap, dtype=torch.uint8, device=dev)
        out_off, out_cap = self.ar * cap, torch.full((self.n,), cap, dtype=torch.int32, device=dev)

        def run():
            zl.batch_compress_dest_size(self.inp, self.in_off, self.in_len, out, out_off, out_cap, self.res,
                                        self.consumed, self.size, self.ws)
        return run

    def summary(self, cap):
        torch.cuda.synchronize()
        r, c = self.res.cpu(), self.consumed.cpu().to(torch.int64)
        ok = bool(((r >= 0) & (r <= cap)).all()) and bool((c > 0).all())
        return ok, float(c.float().mean()), float(r.float().mean())


def case(tag, n, size, caps):
    s = Setup(n, size)
    gib = n * size / 2**30
    fns = [s.fast] + [s.dest_size_fn(c) for c in caps]
    meds, ts = alternate(fns)
    print("%s: compress_fast %.3f ms (%.1f GiB/s)" % (tag, meds[0], gib / meds[0] * 1e3), flush=True)
    for cap, m, t in zip(caps, meds[1:], ts[1:]):
        s.dest_size_fn(cap)()
        ok, mc, mr = s.summary(cap)
        print("    dest_size cap %d: %.3f ms (%.1f GiB/s of input, %.3f us / block) = %.3fx compress_fast; ok=%s, "
              "mean consumed %.0f, mean result %.0f; ms %s"
              % (cap, m, gib / m * 1e3, m * 1e3 / n, m / meds[0], ok, mc, mr, ["%.2f" % x for x in t]), flush=True)
    print("    compress_fast ms %s" % ["%.2f" % x for x in ts[0]], flush=True)
    del s
    torch.cuda.empty_cache()


def case_c():
    n, size, cap = 64, 65536, 16384
    blocks = bench.make_device_blocks("text", n, size, dev, seed=1).cpu().numpy()
    items = [bytes(b) for b in blocks]
    for b in items[:WARM]:
        zl.compressDestSize(b, cap)
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        for b in items:
            zl.compressDestSize(b, cap)
        ts.append((time.perf_counter() - t0) * 1e6 / n)
    print("(c) %s: single zlz4_compress_dest_size, 64 KiB D-text, cap %d: %.1f us / call (passes: %s)"
          % (os.path.basename(zl.LIB_PATH), cap, statistics.median(ts), ["%.1f" % x for x in ts]), flush=True)


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    print("device: %s" % torch.cuda.get_device_name(0), flush=True)
    if which in ("a", "all"):
        case("(a) 65536 x 64 KiB D-text", 65536, 65536, (16384, 4096))
    if which in ("b", "all"):
        case("(b) 262144 x 4 KiB D-text", 262144, 4096, (1024,))
    if which in ("c", "all"):
        case_c()
