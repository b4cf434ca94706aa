#!/usr/bin/env python3
"""Timing of frame prefix decoding (zlz4f_batch_decompress_frame_prefix) against two baselines on
the same frames:

  full    zlz4f_batch_decompress_frame_ex(ZLZ4F_DECODE_LINKED): the whole frame, block table and workspace included.
          --parent-lib PATH takes it from a library built from the parent commit, loaded next to this one; without it
          the call is this build's (the same gfx950 code: profiles/r25_frame_prefix_so_diff.txt).
  block0  zlz4_batch_decompress_safe_prefix on block 0 of every frame (its data found on the host side of the tool, 11
          bytes into the frame): the wide prefix decoder, min(prefix, 65536) bytes -- what a follow-up that routes a
          frame's first block through k_decompress_safe<kPartial> could reach at best.

Inputs (bench.make_device_blocks, D-text, compressed on the device): `one` = 65 536 one-block frames of 64 KiB; `indep` /
`linked` = 4 096 frames of 16 x 64 KiB, declared independent / written with ZLZ4F_BATCH_LINK_BLOCKS.  Prefixes of 64 B,
4 KiB, 64 KiB and the full size.  The three calls alternate inside one process: HIP events around each call, the stream
synchronised after each, warm-up, --reps alternations; median and spread (min .. max) per call.  Before timing, every
prefix output is compared with the first bytes of the input and every result with min(size, prefix).
(profiles/r25_frame_prefix.md)"""
import argparse
import ctypes as C
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
    ap.add_argument("--inputs", default="one,indep,linked")
    ap.add_argument("--one-frames", type=int, default=65536)
    ap.add_argument("--multi-frames", type=int, default=4096)
    ap.add_argument("--prefixes", default="64,4096,65536")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    assert zl.device_available(), "needs a gfx950 device"
    P, plabel = zl.lib(), "this build"
    if a.parent_lib:
        P, plabel = C.CDLL(os.path.abspath(a.parent_lib)), "parent"
    P.zlz4f_batch_decompress_frame_ex.restype = C.c_int32
    P.zlz4f_batch_decompress_frame_workspace_ex.restype = C.c_size_t
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    fmt = "%-52s %9.3f ms  (%.3f .. %.3f, %d runs)"
    for kind in a.inputs.split(","):
        n, size = (a.one_frames, 65536) if kind == "one" else (a.multi_frames, 16 * 65536)
        prefs = zl.Prefs()
        prefs.block_mode = 0 if kind == "linked" else 1
        flags = zl.lz4f.BATCH_LINK_BLOCKS if kind == "linked" else 0
        ar = torch.arange(n, dtype=torch.int64, device=dev)
        raw = make_device_blocks("text", n * (size // 65536), 65536, dev, seed=1).reshape(-1)
        fb = zl.lz4f.compressFrameBound(size, prefs)
        frm = torch.empty(n * fb, dtype=torch.uint8, device=dev)
        frm_off, frm_cap = ar * fb, torch.full((n,), fb, dtype=torch.int64, device=dev)
        src_len = torch.full((n,), size, dtype=torch.int64, device=dev)
        cres = torch.empty(n, dtype=torch.int64, device=dev)
        mb = n * (size // 65536)
        zl.lz4f.compressFrameBatch(raw, ar * size, src_len, frm, frm_off, frm_cap, cres, prefs, flags, mb)
        torch.cuda.synchronize()
        assert bool((cres > 0).all()), "compression failed"
        cbytes = int(cres.sum())
        # block 0 of every frame: a 7-byte header, the block's 4-byte header, its data
        head = frm.view(n, fb)[:, 7:11].to(torch.int64)
        word = head[:, 0] | (head[:, 1] << 8) | (head[:, 2] << 16) | (head[:, 3] << 24)
        assert bool((word < (1 << 31)).all()), "a stored first block"
        b_off, b_len = frm_off + 11, word.to(torch.int32)

        full_out = torch.empty(n * size, dtype=torch.uint8, device=dev)
        full_res = torch.empty(n, dtype=torch.int64, device=dev)
        ws_bytes = P.zlz4f_batch_decompress_frame_workspace_ex(C.c_uint32(n), C.c_uint32(mb), C.c_uint32(zl.lz4f.DECODE_LINKED))
        ws = torch.empty(max(16, ws_bytes), dtype=torch.uint8, device=dev)
        full_off = ar * size

        def full():
            rc = P.zlz4f_batch_decompress_frame_ex(st(), p(frm), p(frm_off), p(cres), p(full_out), p(full_off), p(src_len),
                                                   p(full_res), C.c_uint32(n), C.c_uint32(mb),
                                                   C.c_uint32(zl.lz4f.DECODE_LINKED), p(ws), C.c_size_t(ws.numel()))
            assert rc == 0, rc

        full()
        torch.cuda.synchronize()
        assert bool((full_res == size).all()) and torch.equal(full_out, raw), "the full decode is wrong"
        print("%s: %d frames x %d B D-text (%d blocks each), %.1f MiB of frames; full decode: "
              "zlz4f_batch_decompress_frame_ex(LINKED) (%s), workspace %.1f MiB" %
              (kind, n, size, size // 65536, cbytes / 2**20, plabel, ws_bytes / 2**20))
        for want in sorted({int(x) for x in a.prefixes.split(",")} | {size}):
            out = torch.full((n * want,), 0xA5, dtype=torch.uint8, device=dev)
            off, cap = ar * want, torch.full((n,), want, dtype=torch.int64, device=dev)
            pres = torch.full((n,), -999, dtype=torch.int64, device=dev)
            w0 = min(want, 65536)
            out0 = torch.empty(n * w0, dtype=torch.uint8, device=dev)
            off0, cap0 = ar * w0, torch.full((n,), w0, dtype=torch.int32, device=dev)
            res0 = torch.empty(n, dtype=torch.int64, device=dev)
            pre = lambda: zl.batch_decompress_frame_prefix(frm, frm_off, cres, out, off, cap, pres)  # noqa: E731
            blk = lambda: zl.batch_decompress_safe_prefix(frm, b_off, b_len, out0, off0, cap0, res0)  # noqa: E731
            pre()
            blk()
            torch.cuda.synchronize()
            assert bool((pres == min(want, size)).all()), "wrong prefix results"
            assert torch.equal(out.view(n, want), raw.view(n, size)[:, :want]), "prefix bytes differ from the input"
            assert bool((res0 == w0).all()) and torch.equal(out0.view(n, w0), raw.view(n, size)[:, :w0]), "block 0 differs"
            for _ in range(a.warmup):
                pre()
                full()
                blk()
            torch.cuda.synchronize()
            tp, tf, tb = [], [], []
            for _ in range(a.reps):
                tp.append(timed(pre))
                tf.append(timed(full))
                tb.append(timed(blk))
            mp, mf, mb0 = statistics.median(tp), statistics.median(tf), statistics.median(tb)
            print(fmt % ("%s prefix %7d B  frame prefix (this build)" % (kind, want), mp, min(tp), max(tp), len(tp)))
            print(fmt % ("%s                   full frame decode (%s)" % (kind, plabel), mf, min(tf), max(tf), len(tf)))
            print(fmt % ("%s                   block 0 prefix, %d B (this build)" % (kind, w0), mb0, min(tb), max(tb), len(tb)))
            print("%s prefix %7d B  prefix / full = %.3f   prefix / block0 = %.2f   (prefix / frame = %.5f)" %
                  (kind, want, mp / mf, mp / mb0, want / size))
            del out, out0
        del raw, frm, full_out, ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
