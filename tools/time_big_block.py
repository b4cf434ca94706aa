#!/usr/bin/env python3
"""Device time of ONE block of 2^24 + 70 001 bytes of D-text (tests/bigblocks.py) in batch_compress_fast (acceleration 1)
and batch_compress_hc (levels 4 and 9): torch.cuda.Event around the batch call, the second of two runs.  Above 2^24 the
fast compressor's table has no tags and the level 3-9 search no counted runs; one block is one wavefront (fast) or one
workgroup (HC).
usage: python tools/time_big_block.py"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch, bigblocks as bb, zig_lz4_amd as zl
dev = torch.device("cuda:0")
text = bb.text()
n = len(text)
cap = zl.compressBound(n)
d_in = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(dev)
d_out = torch.empty(cap, dtype=torch.uint8, device=dev)
zero = torch.zeros(1, dtype=torch.int64, device=dev)
t_len = torch.tensor([n], dtype=torch.int32, device=dev)
t_cap = torch.tensor([cap], dtype=torch.int32, device=dev)
res = torch.empty(1, dtype=torch.int64, device=dev)
ws = torch.empty(zl.batch_compress_hc_workspace(1, n), dtype=torch.uint8, device=dev)
calls = [("compressFast(1)", lambda: zl.batch_compress_fast(d_in, zero, t_len, d_out, zero, t_cap, res, n, 1))]
for level in (4, 9):
    calls.append(("compressHC(%d)" % level, lambda level=level: zl.batch_compress_hc(d_in, zero, t_len, d_out, zero, t_cap, res, n, level, ws)))
for name, call in calls:
    ms = []
    for _ in range(2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record()
        torch.cuda.synchronize(); ms.append(e0.elapsed_time(e1))
    print("%-16s 1 x %d bytes: %9.1f ms (first run %.1f ms)  %6.3f GiB/s  -> %d bytes" % (
        name, n, ms[1], ms[0], n / 2**30 / ms[1] * 1e3, int(res[0])), flush=True)
