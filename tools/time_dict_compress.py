#!/usr/bin/env python3
"""Time the dictionary compressor (zlz4_batch_compress_fast_using_dict) with HIP events, as tools/time_stream_compress.py
does, against two yardsticks on the same records in the same process, alternated: zlz4_batch_compress_fast_continue from
the same loaded table (the same table load per block, no dictionary reach) and zlz4_batch_compress_fast.

  (a) 262 144 x 4 KiB D-text records against one shared 64 KiB dictionary (32-bit table: 69 632 positions);
  (b) the same records, each against the previous record (dictionaries inside the input; 16-bit table), with the
      zlz4_batch_load_dict call over all records timed separately;
  (c) 65 536 x 64 KiB D-text blocks against one shared 64 KiB dictionary.

The records are 32 MiB of distinct D-text (tests/datagen.py, one stream cut into records) tiled into separate memory, the
shared dictionary 64 KiB of D-text from another seed, as in tools/time_dict_decompress.py (bench.make_device_blocks gives
every repetition of its pool another byte alphabet, which no shared dictionary could serve).

Per case: best and median time of each call, compressed bytes with and without the dictionary, and -- from the C
restatement on the first records -- the share of match bytes whose source lies in the dictionary.  Every output of the
sample is compared with the restatement's.

  python tools/time_dict_compress.py [a|b|c|all]
"""
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import datagen as dg
import dictcgen
import zig_lz4_amd as zl

dev = torch.device("cuda:0")
SAMPLE = 256


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def batch(nblocks, block):
    slot = (zl.compressBound(block) + 15) // 16 * 16
    ar = torch.arange(nblocks, dtype=torch.int64, device=dev)
    return dict(in_off=ar * block, in_len=torch.full((nblocks,), block, dtype=torch.int32, device=dev),
                out=torch.empty(nblocks * slot, dtype=torch.uint8, device=dev), out_off=ar * slot, slot=slot,
                cap=torch.full((nblocks,), slot, dtype=torch.int32, device=dev),
                res=torch.empty(nblocks, dtype=torch.int64, device=dev))


def run_case(name, inp, nblocks, block, d_dict, dict_off, dict_len, tables, idx, max_dict, cref, rounds=4):
    b = batch(nblocks, block)
    o2, r2 = torch.empty_like(b["out"]), torch.empty_like(b["res"])
    o3, r3 = torch.empty_like(b["out"]), torch.empty_like(b["res"])
    calls = {
        "using_dict": lambda: zl.batch_compress_fast_using_dict(inp, b["in_off"], b["in_len"], b["out"], b["out_off"], b["cap"],
                                                                d_dict, dict_off, dict_len, tables, idx, b["res"], block,
                                                                max_dict, 1),
        "continue": lambda: zl.batch_compress_fast_continue(inp, b["in_off"], b["in_len"], o2, b["out_off"], b["cap"], tables,
                                                            idx, None, r2, block, 1),
        "fast": lambda: zl.batch_compress_fast(inp, b["in_off"], b["in_len"], o3, b["out_off"], b["cap"], r3, block, 1),
    }
    if max_dict + block > 65536 + 11:
        # what the table width alone costs the yardstick: the same call with max_in_len raised to the position count of the
        # dictionary call (a precondition only; it selects the 32-bit table, 10 wavefronts per CU in place of 20)
        calls["continue_u32"] = lambda: zl.batch_compress_fast_continue(inp, b["in_off"], b["in_len"], o2, b["out_off"], b["cap"],
                                                                        tables, idx, None, r2, block + max_dict, 1)
    for fn in calls.values():                         # warm-up: code objects, first touch of the outputs
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in calls}
    for _ in range(rounds):                           # alternated
        for k, fn in calls.items():
            ts[k].append(timed(fn))
    assert int((b["res"] <= 0).sum()) == 0 and int((r3 <= 0).sum()) == 0
    gib = nblocks * block / 2**30
    total = {"using_dict": int(b["res"].sum()), "continue": int(r2.sum()), "continue_u32": int(r2.sum()), "fast": int(r3.sum())}
    print("(%s) %d x %d bytes" % (name, nblocks, block))
    for k in calls:
        t = sorted(ts[k])
        print("    %-12s best %8.2f ms  median %8.2f ms  %7.1f GiB/s  compressed %d bytes (ratio %.3f)  all %s"
              % (k, t[0], t[len(t) // 2], gib / t[0] * 1e3, total[k], nblocks * block / total[k], ["%.2f" % x for x in ts[k]]))
    print("    time using_dict / continue %.2f, using_dict / fast %.2f; compressed size with / without dictionary %.3f"
          % (min(ts["using_dict"]) / min(ts["continue"]), min(ts["using_dict"]) / min(ts["fast"]),
             total["using_dict"] / total["fast"]))
    # the first records against the restatement: bytes, and where the match bytes come from
    k = min(SAMPLE, nblocks)
    h_in = inp.reshape(-1)[:k * block].cpu().numpy()
    h_out = b["out"][:k * b["slot"]].cpu().numpy()
    h_res = b["res"][:k].cpu().numpy()
    h_dict = d_dict.reshape(-1).cpu().numpy() if d_dict is not inp else None
    doff, dlen = dict_off[:k].cpu().numpy(), dict_len[:k].cpu().numpy()
    stats = np.zeros(2, np.uint64)
    for i in range(k):
        src = bytes(h_in[i * block:(i + 1) * block])
        arena = h_dict if h_dict is not None else h_in
        d = bytes(arena[int(doff[i]):int(doff[i]) + int(dlen[i])])
        r, out = cref.compress(src, d, 1, stats=stats)
        assert r == int(h_res[i]) and out == bytes(h_out[i * b["slot"]: i * b["slot"] + r]), "record %d differs from the restatement" % i
    print("    first %d records equal the C restatement; match bytes taken from the dictionary: %.1f %% (%d of %d)"
          % (k, 100.0 * int(stats[0]) / max(1, int(stats[1])), int(stats[0]), int(stats[1])))


POOL = 32 << 20


def records(nblocks, block):
    pool = torch.from_numpy(dg.text_bytes(POOL, 31)).to(dev)
    return pool.repeat(nblocks * block // POOL)


def shared_dict(nblocks, seed):
    d = torch.from_numpy(dg.text_bytes(65536, seed)).to(dev)
    tab = torch.empty(4096, dtype=torch.int32, device=dev)
    r = torch.empty(1, dtype=torch.int64, device=dev)
    zl.batch_load_dict(d, torch.zeros(1, dtype=torch.int64, device=dev), torch.full((1,), 65536, dtype=torch.int32, device=dev), tab, r)
    return (d, torch.zeros(nblocks, dtype=torch.int64, device=dev), torch.full((nblocks,), 65536, dtype=torch.int32, device=dev),
            tab, torch.zeros(nblocks, dtype=torch.int32, device=dev))


def case_a(cref):
    nblocks, block = 262144, 4096
    inp = records(nblocks, block)
    d, doff, dlen, tab, idx = shared_dict(nblocks, 32)
    run_case("a: shared 64 KiB dictionary", inp, nblocks, block, d, doff, dlen, tab, idx, 65536, cref)


def case_b(cref):
    nblocks, block = 262144, 4096
    inp = records(nblocks, block)
    ar = torch.arange(nblocks, dtype=torch.int64, device=dev)
    doff = (ar - 1).clamp(min=0) * block
    dlen = torch.full((nblocks,), block, dtype=torch.int32, device=dev)
    dlen[0] = 0
    tabs = torch.empty(nblocks * 4096, dtype=torch.int32, device=dev)
    r = torch.empty(nblocks, dtype=torch.int64, device=dev)
    flat = inp.reshape(-1)
    load = lambda: zl.batch_load_dict(flat, doff, dlen, tabs, r)
    load()
    torch.cuda.synchronize()
    t = sorted(timed(load) for _ in range(4))
    print("(b) zlz4_batch_load_dict over %d records of %d bytes: best %.2f ms, median %.2f ms" % (nblocks, block, t[0], t[2]))
    run_case("b: previous record as dictionary", flat, nblocks, block, flat, doff, dlen, tabs, None, block, cref)


def case_c(cref):
    nblocks, block = 65536, 65536
    inp = records(nblocks, block)
    d, doff, dlen, tab, idx = shared_dict(nblocks, 32)
    run_case("c: 64 KiB blocks, shared 64 KiB dictionary", inp, nblocks, block, d, doff, dlen, tab, idx, 65536, cref, rounds=3)


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    assert torch.cuda.is_available() and zl.device_available(), "needs a gfx950 device"
    with tempfile.TemporaryDirectory() as tmp:
        cref = dictcgen.ref(tmp)
        for k, fn in (("a", case_a), ("b", case_b), ("c", case_c)):
            if what in (k, "all"):
                fn(cref)
                torch.cuda.synchronize()
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
