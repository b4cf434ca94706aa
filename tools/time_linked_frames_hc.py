#!/usr/bin/env python3
"""Timing of linked-block frames at the HC levels on the GPU (profiles/r13_linked_frames_hc.md):
HIP events around each batch call, one warm-up per variant, then --reps passes that ALTERNATE between the variants in one
process; the best pass of each is reported.

Workload: --frames frames of --blocks x 64 KiB D-text each (64 distinct frames, repeated), per level of --levels:
  linked_hc    zlz4f_batch_compress_frame_ex with ZLZ4F_BATCH_LINK_BLOCKS at the level
  independent  yardstick: zlz4f_batch_compress_frame at the same level, block_mode 1 (every block alone)
  linked_fast  yardstick: zlz4f_batch_compress_frame with ZLZ4F_BATCH_LINK_BLOCKS at the fast level
The linked HC frames of the first pass are decoded with ZLZ4F_DECODE_LINKED and compared with the input.
--only NAME runs one variant alone (for a kernel trace).  Nothing gates on these figures."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch
    import datagen as dg
    import zig_lz4_amd as zl
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--levels", type=int, nargs="+", default=[3, 9])
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    L = zl.lib()
    nf, B = a.frames, 65536
    flen = a.blocks * B
    uniq = min(64, nf)
    raw = torch.from_numpy(np.ascontiguousarray(dg.make_blocks("text", uniq * a.blocks, B, seed=1)).reshape(-1)).to(dev)
    i64 = lambda x: torch.tensor(x, dtype=torch.int64, device=dev)  # noqa: E731
    s_off, s_len = i64([(f % uniq) * flen for f in range(nf)]), i64([flen] * nf)
    max_blocks = nf * a.blocks
    gib = nf * flen / 2**30
    cap = zl.lz4f.compressFrameBound(flen, None)
    d_frm = torch.empty(nf * cap, dtype=torch.uint8, device=dev)
    f_off, f_cap = i64([f * cap for f in range(nf)]), i64([cap] * nf)
    link = zl.lz4f.BATCH_LINK_BLOCKS
    print("%d frames of %d x 64 KiB D-text (%.2f GiB), best of %d alternating passes" % (nf, a.blocks, gib, a.reps))

    def variant(name, fn, level, mode, flags):
        p = zl.Prefs()
        p.compression_level, p.block_mode = level, mode
        ws = torch.empty(zl.lz4f.compressFrameBatchWorkspace(nf, max_blocks, p, flags), dtype=torch.uint8, device=dev)
        res = torch.empty(nf, dtype=torch.int64, device=dev)

        def run():
            rc = fn(zl._stream(), raw.data_ptr(), s_off.data_ptr(), s_len.data_ptr(), d_frm.data_ptr(), f_off.data_ptr(),
                    f_cap.data_ptr(), res.data_ptr(), nf, max_blocks, p, flags, ws.data_ptr(), ws.numel())
            assert rc == 0, (name, rc)
        return dict(name=name, run=run, res=res, ws_bytes=ws.numel(), keep=(p, ws), best=None)

    for level in a.levels:
        vs = [variant("linked_hc", L.zlz4f_batch_compress_frame_ex, level, 0, link),
              variant("independent", L.zlz4f_batch_compress_frame, level, 1, 0),
              variant("linked_fast", L.zlz4f_batch_compress_frame, 0, 0, link)]
        if a.only:
            vs = [v for v in vs if v["name"] == a.only]
        for v in vs:                                   # warm-up; the linked HC frames are checked once
            v["run"]()
            torch.cuda.synchronize()
            assert int((v["res"] < 0).sum()) == 0, v["name"]
            v["bytes"] = int(v["res"].sum())
            if v["name"] == "linked_hc":
                d_out = torch.empty(uniq * flen, dtype=torch.uint8, device=dev)
                dres = torch.empty(uniq, dtype=torch.int64, device=dev)
                zl.lz4f.decompressFrameBatch(d_frm, f_off[:uniq], v["res"][:uniq], d_out, i64([f * flen for f in range(uniq)]),
                                             i64([flen] * uniq), dres, uniq * a.blocks, flags=zl.lz4f.DECODE_LINKED)
                assert bool((dres == flen).all()) and torch.equal(d_out, raw), "the linked HC frames do not decode to the input"
                del d_out
        for _ in range(a.reps):
            for v in vs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                v["run"]()
                e1.record()
                e1.synchronize()
                t = e0.elapsed_time(e1)
                v["best"] = t if v["best"] is None else min(v["best"], t)
        for v in vs:
            print("level %d  %-11s  compressed %d bytes (ratio %.3f)  %.1f ms  %.2f GiB/s  workspace %.2f GiB"
                  % (level, v["name"], v["bytes"], nf * flen / v["bytes"], v["best"], gib / v["best"] * 1e3,
                     v["ws_bytes"] / 2**30))
        by = {v["name"]: v for v in vs}
        if len(by) == 3:
            h, i, f = by["linked_hc"], by["independent"], by["linked_fast"]
            print("level %d  linked_hc / independent: size %.3f  time %.2fx;  linked_hc / linked_fast: size %.3f  time %.2fx"
                  % (level, h["bytes"] / i["bytes"], h["best"] / i["best"], h["bytes"] / f["bytes"], h["best"] / f["best"]))
        del vs


if __name__ == "__main__":
    main()
