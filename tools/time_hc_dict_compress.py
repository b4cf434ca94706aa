#!/usr/bin/env python3
"""Time the HC dictionary compressor (zlz4_batch_compress_hc_using_dict) with HIP events, as tools/time_dict_compress.py
does, against two yardsticks on the same records in the same process, alternated: zlz4_batch_compress_hc at the same
level without a dictionary, and zlz4_batch_compress_fast_using_dict.

  (a) 262 144 x 4 KiB D-text records against one shared 60 KiB dictionary (LDS links: 61 440 + 4 096 = 65 536);
  (b) the same records against one shared 64 KiB dictionary (HBM links);
  (c) the same records, each against the previous record (dictionaries inside the input; LDS links);
  (d) 65 536 x 64 KiB D-text blocks against one shared 64 KiB dictionary (HBM links).

Levels 3, 6 and 9 for each case.  The records are 32 MiB of distinct D-text tiled into separate memory and the shared
dictionary is D-text from another seed, as in tools/time_dict_compress.py.  Per case and level: best and median time of
each call, compressed bytes against both yardsticks; the first records are compared with the C restatement.

The time per kernel (k_hc_dict_stage, k_hc_build_links, k_hc_seg_search, k_hc_parse_emit) comes from a kernel trace of
one call:  rocprofv3 --kernel-trace --stats -- python tools/time_hc_dict_compress.py a --level 9 --once

  python tools/time_hc_dict_compress.py [a|b|c|d|all] [--level L] [--once] [--scale K]
"""
import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import datagen as dg
import hcdictcgen
import zig_lz4_amd as zl

dev = torch.device("cuda:0")
SAMPLE = 64
POOL = 32 << 20


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


def run_case(name, inp, nblocks, block, d_dict, dict_off, dict_len, max_dict, levels, cref, rounds, once):
    b = batch(nblocks, block)
    o2, r2 = torch.empty_like(b["out"]), torch.empty_like(b["res"])
    ws = torch.empty(zl.batch_compress_hc_using_dict_workspace(nblocks, block, max_dict), dtype=torch.uint8, device=dev)
    ws2 = torch.empty(zl.batch_compress_hc_workspace(nblocks, block), dtype=torch.uint8, device=dev)
    print("(%s) %d x %d bytes, links in %s, workspace %.2f GiB" % (name, nblocks, block, "LDS" if max_dict + block <= 65536 else "HBM",
                                                                   ws.numel() / 2**30))
    if once:
        zl.batch_compress_hc_using_dict(inp, b["in_off"], b["in_len"], b["out"], b["out_off"], b["cap"], d_dict, dict_off,
                                        dict_len, b["res"], block, max_dict, levels[0], ws)
        torch.cuda.synchronize()
        return
    # the fast dictionary call: one table per distinct dictionary offset is more than this yardstick needs; it is given one
    # table per block only where the dictionaries differ
    shared = bool((dict_off == dict_off[0]).all()) and bool((dict_len == dict_len[0]).all())
    nt = 1 if shared else nblocks
    tabs = torch.empty(nt * 4096, dtype=torch.int32, device=dev)
    lres = torch.empty(nt, dtype=torch.int64, device=dev)
    zl.batch_load_dict(d_dict, dict_off[:nt].contiguous(), dict_len[:nt].contiguous(), tabs, lres)
    idx = torch.zeros(nblocks, dtype=torch.int32, device=dev) if shared else None
    gib = nblocks * block / 2**30
    for level in levels:
        calls = {
            "hc_using_dict": lambda: zl.batch_compress_hc_using_dict(inp, b["in_off"], b["in_len"], b["out"], b["out_off"], b["cap"],
                                                                     d_dict, dict_off, dict_len, b["res"], block, max_dict, level, ws),
            "hc": lambda: zl.batch_compress_hc(inp, b["in_off"], b["in_len"], o2, b["out_off"], b["cap"], r2, block, level, ws2),
        }
        total = {}
        if level == levels[0]:
            o3, r3 = torch.empty_like(b["out"]), torch.empty_like(b["res"])
            calls["fast_using_dict"] = lambda: zl.batch_compress_fast_using_dict(inp, b["in_off"], b["in_len"], o3, b["out_off"],
                                                                                 b["cap"], d_dict, dict_off, dict_len, tabs, idx,
                                                                                 r3, block, max_dict, 1)
        for fn in calls.values():                     # warm-up: code objects, first touch of the outputs
            fn()
        torch.cuda.synchronize()
        ts = {k: [] for k in calls}
        for _ in range(rounds):                       # alternated
            for k, fn in calls.items():
                ts[k].append(timed(fn))
        assert int((b["res"] <= 0).sum()) == 0 and int((r2 <= 0).sum()) == 0
        total["hc_using_dict"], total["hc"] = int(b["res"].sum()), int(r2.sum())
        if "fast_using_dict" in calls:
            run_case.fast_total = int(r3.sum())
            del o3, r3
        total["fast_using_dict"] = run_case.fast_total
        print("  level %d" % level)
        for k in calls:
            t = sorted(ts[k])
            print("    %-16s best %9.2f ms  median %9.2f ms  %7.2f GiB/s  compressed %d bytes (ratio %.3f)  all %s"
                  % (k, t[0], t[len(t) // 2], gib / t[0] * 1e3, total[k], nblocks * block / total[k], ["%.2f" % x for x in ts[k]]))
        print("    time hc_using_dict / hc %.2f; size against hc %.3f, against fast_using_dict %.3f"
              % (min(ts["hc_using_dict"]) / min(ts["hc"]), total["hc_using_dict"] / total["hc"],
                 total["hc_using_dict"] / total["fast_using_dict"]))
        k = min(SAMPLE, nblocks)
        h_in = inp.reshape(-1)[:k * block].cpu().numpy()
        h_out = b["out"][:k * b["slot"]].cpu().numpy()
        h_res = b["res"][:k].cpu().numpy()
        arena = d_dict.reshape(-1).cpu().numpy() if d_dict is not inp else h_in
        doff, dlen = dict_off[:k].cpu().numpy(), dict_len[:k].cpu().numpy()
        for i in range(k):
            d = bytes(arena[int(doff[i]):int(doff[i]) + int(dlen[i])])
            r, out = cref.compress(bytes(h_in[i * block:(i + 1) * block]), d, level)
            assert r == int(h_res[i]) and out == bytes(h_out[i * b["slot"]: i * b["slot"] + r]), "record %d differs from the restatement" % i
        print("    first %d records equal the C restatement" % k)


def records(nblocks, block):
    pool = torch.from_numpy(dg.text_bytes(POOL, 31)).to(dev)
    total = nblocks * block
    return pool.repeat((total + POOL - 1) // POOL)[:total].contiguous()


def shared(nblocks, dl):
    d = torch.from_numpy(dg.text_bytes(dl, 32)).to(dev)
    return d, torch.zeros(nblocks, dtype=torch.int64, device=dev), torch.full((nblocks,), dl, dtype=torch.int32, device=dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", default="all")
    ap.add_argument("--level", type=int, default=0)
    ap.add_argument("--once", action="store_true", help="one hc_using_dict call per case and nothing else (for a kernel trace)")
    ap.add_argument("--scale", type=int, default=1, help="divide the number of records by this")
    a = ap.parse_args()
    assert torch.cuda.is_available() and zl.device_available(), "needs a gfx950 device"
    levels = [a.level] if a.level else [3, 6, 9]
    with tempfile.TemporaryDirectory() as tmp:
        cref = hcdictcgen.ref(tmp)
        for key, nblocks, block, dl in (("a", 262144, 4096, 61440), ("b", 262144, 4096, 65536), ("c", 262144, 4096, -1),
                                        ("d", 65536, 65536, 65536)):
            if a.what not in (key, "all"):
                continue
            nblocks //= a.scale
            inp = records(nblocks, block)
            if dl < 0:
                ar = torch.arange(nblocks, dtype=torch.int64, device=dev)
                d, doff, dlen = inp, (ar - 1).clamp(min=0) * block, torch.full((nblocks,), block, dtype=torch.int32, device=dev)
                dlen[0] = 0
                name, max_dict = "c: previous record as dictionary", block
            else:
                d, doff, dlen = shared(nblocks, dl)
                name, max_dict = "%s: shared %d KiB dictionary" % (key, dl // 1024), dl
            run_case(name, inp, nblocks, block, d, doff, dlen, max_dict, levels, cref, 3 if key == "d" else 4, a.once)
            del inp, d
            torch.cuda.synchronize()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
