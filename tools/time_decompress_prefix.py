#!/usr/bin/env python3
"""Timing of prefix decoding (zlz4_batch_decompress_safe_prefix) against the full decode of the same blocks
(zlz4_batch_decompress_safe): 65 536 x 64 KiB D-text blocks (bench.make_device_blocks, compressed on the device), the
first 64, 4096 and 32 768 bytes of every block and the full size.  Each prefix decode alternates with the full decode on
the same inputs inside one process: HIP events around each call, the stream synchronised after each, warm-up, --reps
alternations; median and spread (min .. max) per call.  Before timing, every prefix output is compared with the first
bytes of the full decode's output and every result with min(size, prefix).
--parent-lib PATH takes zlz4_batch_decompress_safe from a library built from another commit, loaded next to this one;
without it the full decode is this build's (the same gfx950 code: tools/diff_kernel_asm.py).
--dict runs the _using_dict pair instead, with one 64 KiB dictionary that no block refers to (the cost of the build).
(profiles/r24_prefix_decode.md)"""
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
    ap.add_argument("--blocks", type=int, default=65536)
    ap.add_argument("--block-size", type=int, default=65536)
    ap.add_argument("--prefixes", default="64,4096,32768")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--dict", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    assert zl.device_available(), "needs a gfx950 device"
    n, B = a.blocks, a.block_size
    P, plabel = zl.lib(), "this build"
    if a.parent_lib:
        P, plabel = C.CDLL(os.path.abspath(a.parent_lib)), "parent"
    full_name = "zlz4_batch_decompress_safe_using_dict" if a.dict else "zlz4_batch_decompress_safe"
    getattr(P, full_name).restype = C.c_int32
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    ar = torch.arange(n, dtype=torch.int64, device=dev)
    raw = make_device_blocks("text", n, B, dev, seed=1).reshape(-1)
    slot = (zl.compressBound(B) + 15) // 16 * 16
    comp = torch.empty(n * slot, dtype=torch.uint8, device=dev)
    in_off = ar * slot
    res = torch.empty(n, dtype=torch.int64, device=dev)
    zl.batch_compress_fast(raw, ar * B, torch.full((n,), B, dtype=torch.int32, device=dev), comp, in_off,
                           torch.full((n,), slot, dtype=torch.int32, device=dev), res, B)
    torch.cuda.synchronize()
    in_len = res.to(torch.int32)
    cbytes = int(res.sum())
    d_dict = torch.zeros(65536, dtype=torch.uint8, device=dev)
    d_off = torch.zeros(n, dtype=torch.int64, device=dev)
    d_len = torch.full((n,), 65536, dtype=torch.int32, device=dev)

    full_out = torch.empty(n * B, dtype=torch.uint8, device=dev)
    full_off, full_cap = ar * B, torch.full((n,), B, dtype=torch.int32, device=dev)
    full_res = torch.empty(n, dtype=torch.int64, device=dev)

    def full():
        if a.dict:
            rc = P.zlz4_batch_decompress_safe_using_dict(st(), p(comp), p(in_off), p(in_len), p(full_out), p(full_off),
                                                         p(full_cap), p(d_dict), p(d_off), p(d_len), p(full_res), n)
        else:
            rc = P.zlz4_batch_decompress_safe(st(), p(comp), p(in_off), p(in_len), p(full_out), p(full_off), p(full_cap),
                                              p(full_res), n)
        assert rc == 0, rc

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    full()
    torch.cuda.synchronize()
    assert bool((full_res == B).all()) and torch.equal(full_out, raw), "the full decode is wrong"
    del raw
    print("%d x %d B D-text, %.1f MiB compressed; full decode: %s (%s)%s" %
          (n, B, cbytes / 2**20, full_name, plabel, "; one unreferenced 64 KiB dictionary" if a.dict else ""))
    fmt = "%-44s %8.3f ms  (%.3f .. %.3f, %d runs)"
    for want in [int(x) for x in a.prefixes.split(",")] + [B]:
        out = torch.full((n * want,), 0xA5, dtype=torch.uint8, device=dev)
        off, cap = ar * want, torch.full((n,), want, dtype=torch.int32, device=dev)
        pres = torch.full((n,), -999, dtype=torch.int64, device=dev)
        if a.dict:
            pre = lambda: zl.batch_decompress_safe_prefix_using_dict(comp, in_off, in_len, out, off, cap, d_dict, d_off,  # noqa: E731
                                                                     d_len, pres)
        else:
            pre = lambda: zl.batch_decompress_safe_prefix(comp, in_off, in_len, out, off, cap, pres)  # noqa: E731
        pre()
        torch.cuda.synchronize()
        assert bool((pres == min(want, B)).all()), "wrong prefix results"
        assert torch.equal(out.view(n, want), full_out.view(n, B)[:, :want]), "prefix bytes differ from the full decode"
        for _ in range(a.warmup):
            pre()
            full()
        torch.cuda.synchronize()
        tp, tf = [], []
        for _ in range(a.reps):
            tp.append(timed(pre))
            tf.append(timed(full))
        mp, mf = statistics.median(tp), statistics.median(tf)
        print(fmt % ("prefix %6d B  (prefix decode, this build)" % want, mp, min(tp), max(tp), len(tp)))
        print(fmt % ("              (full decode, %s)" % plabel, mf, min(tf), max(tf), len(tf)))
        print("prefix %6d B  prefix / full = %.3f   (prefix / block = %.4f)" % (want, mp / mf, want / B))
        del out


if __name__ == "__main__":
    main()
