#!/usr/bin/env python3
"""Time dictionary frames at the HC levels (zlz4f_batch_compress_frame_using_dict_ex) with HIP
events: 3 warm-up runs per call, then 10 rounds that alternate between the call and its yardsticks in one process; the
median per call.

  (a) 65 536 records of 4 KiB D-text as independent frames against ONE shared dictionary of 60 KiB (max_src_len = 4096,
      max_dict_len = 61 440: LDS links);
  (b) the same against a 64 KiB dictionary (HBM links);
  (c) 1 024 linked frames of 256 KiB (four 64 KiB blocks) against a 64 KiB dictionary;
  each at the levels 3, 6 and 9.

Yardsticks: zlz4_batch_compress_hc_using_dict on the same records (c: on the frames' 64 KiB blocks) and the same dictionary
-- the block call, whose code the frame call runs and does not change: what the container is paid on top of; the fast
dictionary frames (zlz4f_batch_compress_frame_using_dict); for (c) also zlz4f_batch_compress_frame_ex(..,
ZLZ4F_BATCH_LINK_BLOCKS) at the same level without a dictionary.  The frames are decoded once with
zlz4f_batch_decompress_frame_using_dict and compared with the input.

The time per kernel (k_hc_dict_stage, k_hc_build_links, k_hc_seg_search, k_hc_parse_emit, the k_bf* container kernels) comes
from a kernel trace of one call in a run of its own:
  rocprofv3 --kernel-trace --stats -- python tools/time_dict_frames_hc.py a --level 9 --once

  python tools/time_dict_frames_hc.py [a|b|c|all] [--level L] [--once] [--scale K]
"""
import argparse
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
POOL = 16 << 20
SHAPES = {"a": (65536, 4096, 61440, 1, 4096), "b": (65536, 4096, 65536, 1, 4096), "c": (1024, 262144, 65536, 0, 0)}


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternated(calls):
    """{name: fn} -> {name: median ms}: WARM runs of each, then RUNS rounds over all of them"""
    for fn in calls.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in calls}
    for _ in range(RUNS):
        for k, fn in calls.items():
            ts[k].append(event_ms(fn))
    return {k: statistics.median(v) for k, v in ts.items()}


class Frames:
    """n frames of `size` bytes back to back, one shared dictionary of `dsize` bytes; destination slots of the frame bound"""

    def __init__(self, n, size, dsize, block_mode, max_src_len):
        self.n, self.size, self.dsize, self.block_mode, self.max_src_len = n, size, dsize, block_mode, max_src_len
        pool = min(n * size, POOL)
        self.inp = torch.from_numpy(dg.text_bytes(pool, 1)).to(dev).repeat(n * size // pool)
        self.dict = torch.from_numpy(dg.text_bytes(dsize, 77)).to(dev)
        self.dict_off = torch.zeros(1, dtype=torch.int64, device=dev)
        self.dict_len = torch.full((1,), dsize, dtype=torch.int32, device=dev)
        ar = torch.arange(n, dtype=torch.int64, device=dev)
        fb = zl.lz4f.compressFrameBound(size, self.prefs(0))
        self.src_off, self.src_len = ar * size, torch.full((n,), size, dtype=torch.int64, device=dev)
        self.frm = torch.empty(n * fb, dtype=torch.uint8, device=dev)
        self.frm_off, self.frm_cap = ar * fb, torch.full((n,), fb, dtype=torch.int64, device=dev)
        self.res = torch.empty(n, dtype=torch.int64, device=dev)
        self.mb = n * ((size + 65535) // 65536)

    def prefs(self, level):
        p = zl.Prefs()
        p.block_mode, p.compression_level = self.block_mode, level
        return p

    def dict_frames(self, level):
        """the _ex call at `level` (0: the fast dictionary frames, through the plain call) -> fn"""
        p = self.prefs(level)
        ws_fn = zl.lz4f.compressFrameUsingDictBatchWorkspaceEx if level else zl.lz4f.compressFrameUsingDictBatchWorkspace
        call = zl.lz4f.compressFrameUsingDictBatchEx if level else zl.lz4f.compressFrameUsingDictBatch
        ws = torch.empty(ws_fn(self.n, self.mb, p, 0, 1, self.max_src_len, self.dsize), dtype=torch.uint8, device=dev)
        print("    level %d: frame workspace %.2f GiB" % (level, ws.numel() / 2**30), flush=True)
        return lambda: call(self.inp, self.src_off, self.src_len, self.frm, self.frm_off, self.frm_cap, self.res, self.dict,
                            self.dict_off, self.dict_len, None, p, 0, self.mb, self.max_src_len, self.dsize, ws)

    def linked_frames(self, level):
        """zlz4f_batch_compress_frame_ex with ZLZ4F_BATCH_LINK_BLOCKS at `level`, no dictionary -> fn"""
        p = self.prefs(level)
        ws = torch.empty(zl.lz4f.compressFrameBatchWorkspace(self.n, self.mb, p, zl.lz4f.BATCH_LINK_BLOCKS), dtype=torch.uint8,
                         device=dev)
        return lambda: zl.lz4f.compressFrameBatch(self.inp, self.src_off, self.src_len, self.frm, self.frm_off, self.frm_cap,
                                                  self.res, p, zl.lz4f.BATCH_LINK_BLOCKS, self.mb, ws)

    def block_call(self, level):
        """zlz4_batch_compress_hc_using_dict over the frames' blocks against the shared dictionary -> (fn, results)"""
        block = min(self.size, 65536)
        nb = self.n * self.size // block
        slot = (zl.compressBound(block) + 15) // 16 * 16
        ar = torch.arange(nb, dtype=torch.int64, device=dev)
        in_len = torch.full((nb,), block, dtype=torch.int32, device=dev)
        out = torch.empty(nb * slot, dtype=torch.uint8, device=dev)
        cap = torch.full((nb,), slot, dtype=torch.int32, device=dev)
        res = torch.empty(nb, dtype=torch.int64, device=dev)
        d_off = torch.zeros(nb, dtype=torch.int64, device=dev)
        d_len = torch.full((nb,), self.dsize, dtype=torch.int32, device=dev)
        ws = torch.empty(zl.batch_compress_hc_using_dict_workspace(nb, block, self.dsize), dtype=torch.uint8, device=dev)
        in_off, out_off = ar * block, ar * slot
        return (lambda: zl.batch_compress_hc_using_dict(self.inp, in_off, in_len, out, out_off, cap, self.dict, d_off, d_len,
                                                        res, block, self.dsize, level, ws)), res

    def round_trip(self):
        """decodes the frames in self.frm (results in self.res) with the dictionary -> ok"""
        out = torch.empty(self.n * self.size, dtype=torch.uint8, device=dev)
        dres = torch.empty(self.n, dtype=torch.int64, device=dev)
        zl.lz4f.decompressFrameUsingDictBatch(self.frm, self.frm_off, self.res, out, self.src_off, self.src_len, dres, self.dict,
                                              self.dict_off, self.dict_len, None, self.mb)
        torch.cuda.synchronize()
        return bool((self.res > 0).all()) and bool((dres == self.size).all()) and bool(torch.equal(out, self.inp))


def run(key, levels, once, scale):
    n, size, dsize, block_mode, max_src_len = SHAPES[key]
    n //= scale
    s = Frames(n, size, dsize, block_mode, max_src_len)
    gib = n * size / 2**30
    print("(%s) %d x %d bytes, %s frames, %d-byte dictionary, %s links in launch A" %
          (key, n, size, "independent" if block_mode else "linked", dsize,
           "LDS" if dsize + min(size, 65536) <= 65536 and max_src_len else "HBM"), flush=True)
    if once:
        fn = s.dict_frames(levels[0])
        fn()
        torch.cuda.synchronize()
        return
    fast = s.dict_frames(0)
    for level in levels:
        frames = s.dict_frames(level)
        block, block_res = s.block_call(level)
        calls = {"frames_hc_dict": frames, "block_hc_dict": block, "frames_fast_dict": fast}
        if key == "c":
            calls["frames_hc_linked"] = s.linked_frames(level)
        t = alternated(calls)
        total = {}
        for k, fn in calls.items():                                    # sizes, and the round trip of the new frames last
            if k != "frames_hc_dict":
                fn()
                torch.cuda.synchronize()
                total[k] = int((block_res if k == "block_hc_dict" else s.res).sum())
        frames()
        ok = s.round_trip()
        total["frames_hc_dict"] = int(s.res.sum())
        print("  level %d (round trip ok=%s)" % (level, ok))
        for k in calls:
            print("    %-17s median %9.3f ms  %7.2f GiB/s  %12d bytes (ratio %.3f)" %
                  (k, t[k], gib / t[k] * 1e3, total[k], n * size / total[k]))
        print("    frames / block call %.3f; against the fast dictionary frames: time %.2f, size %.3f%s" %
              (t["frames_hc_dict"] / t["block_hc_dict"], t["frames_hc_dict"] / t["frames_fast_dict"],
               total["frames_hc_dict"] / total["frames_fast_dict"],
               "; against linked HC without a dictionary: time %.2f, size %.3f" %
               (t["frames_hc_dict"] / t["frames_hc_linked"], total["frames_hc_dict"] / total["frames_hc_linked"])
               if key == "c" else ""), flush=True)
        del frames, block, block_res, calls
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", default="all")
    ap.add_argument("--level", type=int, default=0)
    ap.add_argument("--once", action="store_true", help="one _ex call per shape and nothing else (for a kernel trace)")
    ap.add_argument("--scale", type=int, default=1, help="divide the number of frames by this")
    a = ap.parse_args()
    assert torch.cuda.is_available() and zl.device_available(), "needs a gfx950 device"
    print("device: %s" % torch.cuda.get_device_name(0), flush=True)
    for key in SHAPES:
        if a.what in (key, "all"):
            run(key, [a.level] if a.level else [3, 6, 9], a.once, a.scale)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
