#!/usr/bin/env python3
"""Time the streaming compressor (zlz4_batch_compress_fast_continue, zlz4_batch_load_dict) with HIP events, as
tools/time_dict_decompress.py does.

  (a) configs[1] shape (65 536 x 64 KiB D-text): continue from zero tables (identity indexing, tables written) against
      zlz4_batch_compress_fast on the same blocks, alternated; the outputs must be identical;
  (b) 262 144 x 4 KiB D-text records against one loaded 64 KiB dictionary (every block points at table 0);
  (c) a two-step chained run: 16 384 streams, step 1 = 64 KiB blocks from zero tables, step 2 = the next 64 KiB of
      every stream continuing in place;
  (d) loadDict: one 64 KiB dictionary, one 64 KiB run of one repeated byte (all positions on one slot), and 4096
      dictionaries of 64 KiB in one batch.

  python tools/time_stream_compress.py [a|b|c|d|all]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import bench
import zig_lz4_amd as zl

dev = torch.device("cuda:0")


def timed(fn, iters=5):
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize(); ts.append(e0.elapsed_time(e1))
    return ts


def batch(nblocks, block):
    slot = (zl.compressBound(block) + 15) // 16 * 16
    ar = torch.arange(nblocks, dtype=torch.int64, device=dev)
    return dict(in_off=ar * block, in_len=torch.full((nblocks,), block, dtype=torch.int32, device=dev),
                out=torch.empty(nblocks * slot, dtype=torch.uint8, device=dev), out_off=ar * slot,
                cap=torch.full((nblocks,), slot, dtype=torch.int32, device=dev),
                res=torch.empty(nblocks, dtype=torch.int64, device=dev))


def case_a():
    nblocks, block = 65536, 65536
    inp = bench.make_device_blocks("text", nblocks, block, dev, seed=1)
    b = batch(nblocks, block)
    ref_out, ref_res = torch.empty_like(b["out"]), torch.empty_like(b["res"])
    tables = torch.zeros(nblocks * 4096, dtype=torch.int32, device=dev)

    def fast():
        zl.batch_compress_fast(inp, b["in_off"], b["in_len"], ref_out, b["out_off"], b["cap"], ref_res, block, 1)

    def cont():
        tables.zero_()      # (a fresh zero table per block, as a stream's first step; the fill is timed too)
        zl.batch_compress_fast_continue(inp, b["in_off"], b["in_len"], b["out"], b["out_off"], b["cap"], tables, None,
                                        tables, b["res"], block, 1)

    def cont_nofill():
        zl.batch_compress_fast_continue(inp, b["in_off"], b["in_len"], b["out"], b["out_off"], b["cap"], zeros, None,
                                        tables, b["res"], block, 1)
    zeros = torch.zeros(nblocks * 4096, dtype=torch.int32, device=dev)
    tf, tc, tn = [], [], []
    for _ in range(3):
        tf += timed(fast, 3); tc += timed(cont, 3); tn += timed(cont_nofill, 3)
    same = bool(torch.equal(ref_res, b["res"])) and bool(torch.equal(ref_out, b["out"]))
    gib = nblocks * block / 2**30
    f, c, n = min(tf), min(tc), min(tn)
    print("(a) configs[1] D-text: compressFast %.2f ms (%.1f GiB/s), continue from zero tables %.2f ms (%.1f GiB/s, "
          "ratio %.3f), same with separate zero input tables (no fill) %.2f ms (ratio %.3f), identical=%s"
          % (f, gib / f * 1e3, c, gib / c * 1e3, c / f, n, n / f, same))
    print("    ms fast %s / cont %s / nofill %s" % (["%.2f" % x for x in tf], ["%.2f" % x for x in tc], ["%.2f" % x for x in tn]))


def load_tables(dicts_u8, lens):
    n = len(lens)
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)).to(dev)
    t_len = torch.from_numpy(np.asarray(lens, np.int32)).to(dev)
    tabs = torch.empty(n * 4096, dtype=torch.int32, device=dev)
    res = torch.empty(n, dtype=torch.int64, device=dev)
    return offs, t_len, tabs, res


def case_b():
    nblocks, block = 262144, 4096
    inp = bench.make_device_blocks("text", nblocks, block, dev, seed=2)
    d = bench.make_device_blocks("text", 1, 65536, dev, seed=3).reshape(-1)
    offs, t_len, tab, r = load_tables(d, [65536])
    zl.batch_load_dict(d, offs, t_len, tab, r)
    b = batch(nblocks, block)
    idx = torch.zeros(nblocks, dtype=torch.int32, device=dev)
    tout = torch.empty(nblocks * 4096, dtype=torch.int32, device=dev)
    t = timed(lambda: zl.batch_compress_fast_continue(inp, b["in_off"], b["in_len"], b["out"], b["out_off"], b["cap"], tab,
                                                      idx, tout, b["res"], block, 1), 6)
    t2 = timed(lambda: zl.batch_compress_fast_continue(inp, b["in_off"], b["in_len"], b["out"], b["out_off"], b["cap"], tab,
                                                       idx, None, b["res"], block, 1), 6)
    ref_out, ref_res = torch.empty_like(b["out"]), torch.empty_like(b["res"])
    tf = timed(lambda: zl.batch_compress_fast(inp, b["in_off"], b["in_len"], ref_out, b["out_off"], b["cap"], ref_res,
                                              block, 1), 6)
    torch.cuda.synchronize()
    gib = nblocks * block / 2**30
    ratio = gib * 2**30 / float(b["res"].sum())
    print("(b) 262144 x 4 KiB D-text against one loaded 64 KiB dictionary: %.2f ms (%.1f GiB/s) with the final tables "
          "written, %.2f ms (%.1f GiB/s) without; compressFast (zero tables) %.2f ms; ratio %.3f (compressFast %.3f)"
          % (min(t), gib / min(t) * 1e3, min(t2), gib / min(t2) * 1e3, min(tf), ratio, gib * 2**30 / float(ref_res.sum())))


def case_c():
    nstreams, block = 16384, 65536
    data = bench.make_device_blocks("text", nstreams * 2, block, dev, seed=4)
    tables = torch.zeros(nstreams * 4096, dtype=torch.int32, device=dev)
    b = batch(nstreams, block)
    step_off = [b["in_off"] * 2, b["in_off"] * 2 + block]     # stream s = blocks 2s, 2s + 1

    def run():
        tables.zero_()
        for k in range(2):
            zl.batch_compress_fast_continue(data, step_off[k], b["in_len"], b["out"], b["out_off"], b["cap"], tables, None,
                                            tables, b["res"], block, 1)
    t = timed(run, 5)
    gib = 2 * nstreams * block / 2**30
    print("(c) two chained steps, 16384 streams x 2 x 64 KiB D-text, in place: %.2f ms (%.1f GiB/s)" % (min(t), gib / min(t) * 1e3))


def case_d():
    one = bench.make_device_blocks("text", 1, 65536, dev, seed=5).reshape(-1)
    rep = torch.full((65536,), 0x61, dtype=torch.uint8, device=dev)
    many = bench.make_device_blocks("text", 4096, 65536, dev, seed=6).reshape(-1)
    for name, d, n in (("one 64 KiB D-text dictionary", one, 1), ("one 64 KiB run of one byte", rep, 1),
                       ("4096 x 64 KiB D-text dictionaries", many, 4096)):
        offs, t_len, tab, r = load_tables(d, [65536] * n)
        t = timed(lambda: zl.batch_load_dict(d, offs, t_len, tab, r), 8)
        print("(d) loadDict, %s: %.3f ms (best of 8; median %.3f)" % (name, min(t), sorted(t)[len(t) // 2]))


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    for k, fn in (("a", case_a), ("b", case_b), ("c", case_c), ("d", case_d)):
        if what in (k, "all"):
            fn()
            torch.cuda.synchronize()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
