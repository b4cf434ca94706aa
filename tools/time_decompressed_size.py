#!/usr/bin/env python3
"""Timing of the decompressed-size queries on the GPU against the decode they precede: HIP events around each call,
warm-up, median of --reps, the calls of one case alternating inside one process (profiles/r09_decompressed_size.md).
Cases, every block distinct (bench.make_device_blocks), compressed on the device:
  text64k   65 536 x 64 KiB D-text      zlz4_batch_decompressed_size      vs zlz4_batch_decompress_safe
  text4k    262 144 x 4 KiB D-text      the same pair
  zero64k   16 384 x 64 KiB D-zero      the same pair, and the decoder's private size pass zlz4_launch_decompress_sizes
  frames    65 536 frames of 64 KiB D-text, without and with block checksums:
            zlz4f_batch_frame_decompressed_size vs zlz4f_batch_decompress_frame
  edge      one block that decodes to 0xFFFFFFFF bytes (a single run of ~16.8 M length bytes, 17 MB of input) between
            two small ones: the query alone
--alt-lib LABEL=PATH[,LABEL=PATH...] also times the block query of other builds of this library (A/B of a variation of
k_decompressed_size).
--parent-lib PATH times the decode calls (and the private size pass) in a library built from another commit, loaded next
to this one; without it they come from this build (the decoder's code objects are the same in both: tools/
diff_kernel_asm.py).  Every query result is checked against the known sizes.  Prints one line per call."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed_alternating(fns, warm, reps):
    """medians (ms) of the calls of `fns`, run in turn inside each repetition"""
    import torch
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b))
    return [statistics.median(t) for t in ts]


def main():
    import torch
    import zig_lz4_amd as zl
    from bench import make_device_blocks
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="text64k,text4k,zero64k,frames,edge")
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies every block count (rehearsals)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--alt-lib", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    assert zl.device_available(), "needs a gfx950 device"
    L = zl.lib()
    P, plabel = L, "this build"
    if a.parent_lib:
        P, plabel = C.CDLL(os.path.abspath(a.parent_lib)), "parent"
    for name in ("zlz4_batch_decompress_safe", "zlz4f_batch_decompress_frame", "zlz4_launch_decompress_sizes"):
        getattr(P, name).restype = C.c_int32
    alts = []
    for spec in filter(None, a.alt_lib.split(",")):
        lab, path = spec.split("=", 1)
        A = C.CDLL(os.path.abspath(path))
        A.zlz4_batch_decompressed_size.restype = C.c_int32
        alts.append((lab, A))
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    i64 = lambda x: torch.as_tensor(x, dtype=torch.int64).to(dev)  # noqa: E731
    u32 = lambda x: torch.as_tensor(x, dtype=torch.int64).to(torch.int32).to(dev)  # noqa: E731

    def blocks_case(label, dist, n, B):
        n = max(64, int(n * a.scale))
        raw = make_device_blocks(dist, n, B, dev, seed=1).reshape(-1)
        cap = zl.compressBound(B)
        comp = torch.empty(n * cap, dtype=torch.uint8, device=dev)
        in_off = torch.arange(n, dtype=torch.int64, device=dev) * cap
        res = torch.empty(n, dtype=torch.int64, device=dev)
        zl.batch_compress_fast(raw, torch.arange(n, dtype=torch.int64, device=dev) * B, u32([B]).repeat(n), comp, in_off,
                               u32([cap]).repeat(n), res, B)
        torch.cuda.synchronize()
        del raw
        in_len = res.to(torch.int32)
        cbytes = int(res.sum())
        d_out = torch.empty(n * B, dtype=torch.uint8, device=dev)
        out_off = torch.arange(n, dtype=torch.int64, device=dev) * B
        out_cap = u32([B]).repeat(n)
        result = torch.empty(n, dtype=torch.int64, device=dev)
        size = torch.empty(n, dtype=torch.int64, device=dev)
        zeros = torch.zeros(n, dtype=torch.int64, device=dev)
        full = torch.full((n,), -1, dtype=torch.int32, device=dev)          # 0xFFFFFFFF
        psize = torch.empty(n, dtype=torch.int64, device=dev)
        names = ["zlz4_batch_decompressed_size (this build)", "zlz4_batch_decompress_safe (%s)" % plabel]
        fns = [lambda: zl.batch_decompressed_size(comp, in_off, in_len, size),
               lambda: P.zlz4_batch_decompress_safe(st(), p(comp), p(in_off), p(in_len), p(d_out), p(out_off), p(out_cap),
                                                    p(result), n)]
        if dist == "zero":
            names.append("zlz4_launch_decompress_sizes (%s)" % plabel)
            fns.append(lambda: P.zlz4_launch_decompress_sizes(st(), p(comp), p(in_off), p(in_len), p(zeros), p(full),
                                                              p(psize), n))
        asizes = [torch.empty(n, dtype=torch.int64, device=dev) for _ in alts]
        for (lab, A), asz in zip(alts, asizes):
            names.append("zlz4_batch_decompressed_size (%s)" % lab)
            fns.append(lambda A=A, asz=asz: A.zlz4_batch_decompressed_size(st(), p(comp), p(in_off), p(in_len), None, p(asz), n))
        ms = timed_alternating(fns, a.warmup, a.reps)
        assert bool((size == B).all()) and bool((result == B).all()), "wrong sizes"
        assert all(bool((asz == B).all()) for asz in asizes), "wrong sizes"
        if dist == "zero":
            assert bool((psize == B).all())
        for nm, t in zip(names, ms):
            print("%-8s %7d x %6d B  in %8.1f MiB  %-48s %8.3f ms  %7.1f GiB/s of output  %6.1f GiB/s of input" %
                  (label, n, B, cbytes / 2**20, nm, t, n * B / 2**30 / t * 1e3, cbytes / 2**30 / t * 1e3))
        print("%-8s query / decode = %.3f" % (label, ms[0] / ms[1]) +
              ("   query / private size pass = %.3f" % (ms[0] / ms[2]) if dist == "zero" else ""))

    def frames_case(n, B, bc):
        n = max(64, int(n * a.scale))
        label = "frames" + ("+bc" if bc else "")
        raw = make_device_blocks("text", n, B, dev, seed=2).reshape(-1)
        prefs = zl.Prefs()
        prefs.block_checksum = bc
        fcap = zl.lz4f.compressFrameBound(B, prefs)
        d_frm = torch.empty(n * fcap, dtype=torch.uint8, device=dev)
        f_off = torch.arange(n, dtype=torch.int64, device=dev) * fcap
        flen = torch.empty(n, dtype=torch.int64, device=dev)
        zl.lz4f.compressFrameBatch(raw, torch.arange(n, dtype=torch.int64, device=dev) * B, i64([B]).repeat(n), d_frm, f_off,
                                   i64([fcap]).repeat(n), flen, prefs, 0, n)
        torch.cuda.synchronize()
        del raw
        assert int(flen.min()) > 0
        cbytes = int(flen.sum())
        d_out = torch.empty(n * B, dtype=torch.uint8, device=dev)
        o_off = torch.arange(n, dtype=torch.int64, device=dev) * B
        o_cap = i64([B]).repeat(n)
        result = torch.empty(n, dtype=torch.int64, device=dev)
        size = torch.empty(n, dtype=torch.int64, device=dev)
        qws = torch.empty(zl.lz4f.frameDecompressedSizeBatchWorkspace(n, n), dtype=torch.uint8, device=dev)
        dws = torch.empty(zl.lz4f.decompressFrameBatchWorkspace(n, n), dtype=torch.uint8, device=dev)
        names = ["zlz4f_batch_frame_decompressed_size (this build)", "zlz4f_batch_decompress_frame (%s)" % plabel]
        fns = [lambda: zl.lz4f.frameDecompressedSizeBatch(d_frm, f_off, flen, size, n, qws),
               lambda: P.zlz4f_batch_decompress_frame(st(), p(d_frm), p(f_off), p(flen), p(d_out), p(o_off), p(o_cap), p(result),
                                                      n, n, p(dws), C.c_size_t(dws.numel()))]
        ms = timed_alternating(fns, a.warmup, a.reps)
        assert bool((size == B).all()) and bool((result == B).all()), "wrong sizes"
        for nm, t in zip(names, ms):
            print("%-8s %7d x %6d B  in %8.1f MiB  %-48s %8.3f ms  %7.1f GiB/s of output  %6.1f GiB/s of input" %
                  (label, n, B, cbytes / 2**20, nm, t, n * B / 2**30 / t * 1e3, cbytes / 2**30 / t * 1e3))
        print("%-8s query / decode = %.3f" % (label, ms[0] / ms[1]))

    def edge_case():
        import sizegen
        items = [sizegen.edge_block(70000), sizegen.edge_block(0xFFFFFFFF), sizegen.edge_block(4096)]
        lens = [len(b) for b in items]
        offs = [0]
        for ln in lens[:-1]:
            offs.append((offs[-1] + ln + 15) & ~15)
        buf = torch.zeros(offs[-1] + lens[-1], dtype=torch.uint8)
        for o, b in zip(offs, items):
            buf[o:o + len(b)] = torch.frombuffer(bytearray(b), dtype=torch.uint8)
        comp, in_off, in_len = buf.to(dev), i64(offs), u32(lens)
        n = len(items)
        outs = [torch.empty(n, dtype=torch.int64, device=dev) for _ in range(1 + len(alts))]
        names = ["zlz4_batch_decompressed_size (this build)"] + ["zlz4_batch_decompressed_size (%s)" % lab for lab, _ in alts]
        fns = [lambda: zl.batch_decompressed_size(comp, in_off, in_len, outs[0])]
        for (lab, A), o in zip(alts, outs[1:]):
            fns.append(lambda A=A, o=o: A.zlz4_batch_decompressed_size(st(), p(comp), p(in_off), p(in_len), None, p(o), n))
        ms = timed_alternating(fns, a.warmup, a.reps)
        assert all(o.cpu().tolist() == [70000, 0xFFFFFFFF, 4096] for o in outs), "wrong sizes"
        for nm, t in zip(names, ms):
            print("%-8s %7d blocks       in %8.1f MiB  %-48s %8.3f ms  %6.1f GiB/s of input" %
                  ("edge", n, sum(lens) / 2**20, nm, t, sum(lens) / 2**30 / t * 1e3))

    want = a.cases.split(",")
    if "text64k" in want:
        blocks_case("text64k", "text", 65536, 65536)
    if "text4k" in want:
        blocks_case("text4k", "text", 262144, 4096)
    if "zero64k" in want:
        blocks_case("zero64k", "zero", 16384, 65536)
    if "frames" in want:
        frames_case(65536, 65536, 0)
        frames_case(65536, 65536, 1)
    if "edge" in want:
        edge_case()


if __name__ == "__main__":
    main()
