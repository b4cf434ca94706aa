#!/usr/bin/env python3
"""Timing of the frame index and of frame range decoding (zlz4f_batch_frame_index, zlz4f_batch_decompress_frame_range,
DESIGN.md section 4.4g) against the calls that reach the same bytes without an index:

  query   zlz4f_batch_frame_decompressed_size: what the index call costs apart from its one new kernel.
  full    zlz4f_batch_decompress_frame: the whole frame.
  prefix  zlz4f_batch_decompress_frame_prefix with n = b: the only way to bytes [a, b) without decoding everything.

--parent-lib PATH takes the three baselines from a library built from the parent commit, loaded next to this one; without
it they are this build's.  Input (bench.make_device_blocks, D-text, compressed on the device): --frames independent frames
of 16 x 64 KiB.  Workloads: the index; one 4 KiB range per frame at decoded offset 512 KiB + 1000; one 64 KiB range per
frame straddling a block boundary; 16 ranges per frame covering it entirely.  The calls of a workload alternate inside one
process: HIP events around each call, the stream synchronised after each, warm-up, --reps alternations; median and spread
(min .. max) per call.  Before timing, every range output is compared with the input and the index with the size query.
(profiles/r26_frame_range.md)"""
import argparse
import ctypes as C
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
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    assert zl.device_available(), "needs a gfx950 device"
    P, plabel = zl.lib(), "this build"
    if a.parent_lib:
        P, plabel = C.CDLL(os.path.abspath(a.parent_lib)), "parent"
    for name, res in (("zlz4f_batch_decompress_frame", C.c_int32), ("zlz4f_batch_decompress_frame_workspace", C.c_size_t),
                      ("zlz4f_batch_frame_decompressed_size", C.c_int32),
                      ("zlz4f_batch_frame_decompressed_size_workspace", C.c_size_t),
                      ("zlz4f_batch_decompress_frame_prefix", C.c_int32)):
        getattr(P, name).restype = res
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    u32, sz = C.c_uint32, C.c_size_t

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def alternate(title, calls):
        for _ in range(a.warmup):
            for _, fn in calls:
                fn()
        torch.cuda.synchronize()
        times = [[] for _ in calls]
        for _ in range(a.reps):
            for t, (_, fn) in zip(times, calls):
                t.append(timed(fn))
        med = [statistics.median(t) for t in times]
        for (label, _), t, m in zip(calls, times, med):
            print("%-18s %-46s %9.3f ms  (%.3f .. %.3f, %d runs)" % (title, label, m, min(t), max(t), len(t)))
        print("%-18s %s" % (title, "   ".join("%s / %s = %.3f" % (calls[0][0].split(" (")[0], l.split(" (")[0], med[0] / m)
                                              for (l, _), m in list(zip(calls, med))[1:])))

    n, nblk, bs = a.frames, 16, 65536
    size, mb = nblk * bs, a.frames * nblk
    prefs = zl.Prefs()
    prefs.block_mode = 1
    ar = torch.arange(n, dtype=torch.int64, device=dev)
    raw = make_device_blocks("text", mb, bs, dev, seed=1).reshape(-1)
    fb = zl.lz4f.compressFrameBound(size, prefs)
    frm = torch.empty(n * fb, dtype=torch.uint8, device=dev)
    frm_off, frm_cap = ar * fb, torch.full((n,), fb, dtype=torch.int64, device=dev)
    src_len = torch.full((n,), size, dtype=torch.int64, device=dev)
    cres = torch.empty(n, dtype=torch.int64, device=dev)
    zl.lz4f.compressFrameBatch(raw, ar * size, src_len, frm, frm_off, frm_cap, cres, prefs, 0, mb)
    torch.cuda.synchronize()
    assert bool((cres > 0).all()), "compression failed"
    print("%d independent frames x %d B D-text (%d blocks each), %.1f MiB of frames; baselines: %s" %
          (n, size, nblk, int(cres.sum()) / 2**20, plabel))

    # ---- 1. the index against the size query
    qws = torch.empty(max(16, P.zlz4f_batch_frame_decompressed_size_workspace(u32(n), u32(mb))), dtype=torch.uint8, device=dev)
    iws = torch.empty(max(16, zl.lz4f.frameIndexBatchWorkspace(n, mb)), dtype=torch.uint8, device=dev)
    qres = torch.empty(n, dtype=torch.int64, device=dev)
    index = torch.zeros((n * (nblk + 1), 2), dtype=torch.int64, device=dev)
    idx_off, idx_cap = ar * (nblk + 1), torch.full((n,), nblk + 1, dtype=torch.int64, device=dev)
    idx_n = torch.empty(n, dtype=torch.int64, device=dev)

    def query():
        rc = P.zlz4f_batch_frame_decompressed_size(st(), p(frm), p(frm_off), p(cres), p(qres), u32(n), u32(mb), p(qws),
                                                   sz(qws.numel()))
        assert rc == 0, rc

    build = lambda: zl.lz4f.frameIndexBatch(frm, frm_off, cres, index, idx_off, idx_cap, idx_n, mb, iws)  # noqa: E731
    query()
    build()
    torch.cuda.synchronize()
    assert bool((qres == size).all()) and bool((idx_n == nblk).all()), "size query / index results"
    dec = index.view(n, nblk + 1, 2)[:, :, 1]
    assert torch.equal(dec, (torch.arange(nblk + 1, device=dev) * bs).expand(n, -1)), "index offsets"
    alternate("index", [("frame index (this build)", build), ("size query (%s)" % plabel, query)])

    # ---- the baselines of the range workloads
    full_out = torch.empty(n * size, dtype=torch.uint8, device=dev)
    full_res = torch.empty(n, dtype=torch.int64, device=dev)
    dws = torch.empty(max(16, P.zlz4f_batch_decompress_frame_workspace(u32(n), u32(mb))), dtype=torch.uint8, device=dev)
    full_off = ar * size

    def full():
        rc = P.zlz4f_batch_decompress_frame(st(), p(frm), p(frm_off), p(cres), p(full_out), p(full_off), p(src_len), p(full_res),
                                            u32(n), u32(mb), p(dws), sz(dws.numel()))
        assert rc == 0, rc

    full()
    torch.cuda.synchronize()
    assert bool((full_res == size).all()) and torch.equal(full_out, raw), "the full decode is wrong"
    rawf = raw.view(n, size)

    def ranges_workload(title, per_frame):
        """per_frame: [(a, b)] for every frame"""
        k = len(per_frame)
        rng = np.zeros((n * k, 3), dtype=np.uint64)
        rng[:, 0] = np.repeat(np.arange(n, dtype=np.uint64), k)
        rng[:, 1] = np.tile(np.array([x for x, _ in per_frame], dtype=np.uint64), n)
        rng[:, 2] = np.tile(np.array([y for _, y in per_frame], dtype=np.uint64), n)
        d_range = torch.from_numpy(rng.view(np.int64)).to(dev)
        nr = n * k
        dst_off = torch.empty(nr, dtype=torch.int64, device=dev)
        dst_cap = torch.empty(nr, dtype=torch.int64, device=dev)
        totals = torch.empty(2, dtype=torch.int64, device=dev)
        zl.lz4f.planFrameRanges(index, idx_off, idx_n, d_range, dst_off, dst_cap, totals, 16)
        arena, items = totals.cpu().tolist()
        out = torch.empty(max(1, arena), dtype=torch.uint8, device=dev)
        skip = torch.empty(nr, dtype=torch.int64, device=dev)
        res = torch.empty(nr, dtype=torch.int64, device=dev)
        rws = torch.empty(max(16, zl.lz4f.decompressFrameRangeBatchWorkspace(nr, items)), dtype=torch.uint8, device=dev)
        run = lambda: zl.lz4f.decompressFrameRangeBatch(frm, frm_off, cres, index, idx_off, idx_n, d_range, out, dst_off,  # noqa: E731
                                                        dst_cap, skip, res, items, rws)
        plan = lambda: zl.lz4f.planFrameRanges(index, idx_off, idx_n, d_range, dst_off, dst_cap, totals, 16)  # noqa: E731
        run()
        torch.cuda.synchronize()
        lens = torch.tensor([y - x for x, y in per_frame], dtype=torch.int64, device=dev).repeat(n)
        assert torch.equal(res, lens), "range results"
        o_h, s_h = dst_off.view(n, k).cpu(), skip.view(n, k).cpu()
        for j, (x, y) in enumerate(per_frame):                # bytes: frame by frame for a sample, all frames for one range
            for f in (range(n) if j == 0 else (0, n // 2, n - 1)):
                lo = int(o_h[f, j] + s_h[f, j])
                assert torch.equal(out[lo:lo + y - x], rawf[f, x:y]), "range bytes differ from the input"
        print("%-18s %d ranges, %d items, slots %.1f MiB, workspace %.1f MiB" % (title, nr, items, arena / 2**20, rws.numel() / 2**20))
        calls = [("range decode (this build)", run), ("full frame decode (%s)" % plabel, full)]
        bmax = max(y for _, y in per_frame)
        if k == 1:
            pout = torch.empty(n * bmax, dtype=torch.uint8, device=dev)
            poff, pcap = ar * bmax, torch.full((n,), bmax, dtype=torch.int64, device=dev)
            pres = torch.empty(n, dtype=torch.int64, device=dev)

            def prefix():
                rc = P.zlz4f_batch_decompress_frame_prefix(st(), p(frm), p(frm_off), p(cres), p(pout), p(poff), p(pcap), p(pres),
                                                           u32(n))
                assert rc == 0, rc
            prefix()
            torch.cuda.synchronize()
            assert bool((pres == bmax).all()), "prefix results"
            calls.append(("frame prefix n = %d (%s)" % (bmax, plabel), prefix))
        calls.append(("plan (this build)", plan))
        alternate(title, calls)

    ranges_workload("4 KiB mid-frame", [(8 * bs + 1000, 8 * bs + 1000 + 4096)])
    ranges_workload("64 KiB straddling", [(8 * bs + bs // 2, 9 * bs + bs // 2)])
    ranges_workload("16 ranges = frame", [(k * bs, (k + 1) * bs) for k in range(nblk)])


if __name__ == "__main__":
    main()
