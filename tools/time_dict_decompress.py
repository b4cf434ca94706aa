#!/usr/bin/env python3
"""Time the dictionary decoder (zlz4_batch_decompress_safe_using_dict) with HIP events, as tools/time_decompress.py does.

  (a) configs[1] streams (65 536 x 64 KiB D-text, compressDefault) with an EMPTY dictionary, against
      zlz4_batch_decompress_safe on the same streams;
  (b) 262 144 x 4 KiB D-text records, one shared 64 KiB D-text dictionary;
  (c) the same records, dictionary of record i = the plaintext of record i - 1.
For (b) / (c) 8192 distinct records (32 MiB of D-text) are encoded on the host by tests/dict_encoder.c and the streams
are tiled 32 times into separate memory (output slots and input copies are all distinct).  Reports output GiB/s and the
share of match bytes the encoder took from the dictionary; with liblz4 present, also LZ4_decompress_safe_usingDict on one
host core for (b) (ctypes per call: an upper bound of its time).

  python tools/time_dict_decompress.py [a|b|c|all]
"""
import ctypes as C
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import bench
import datagen as dg
import dictgen
import zig_lz4_amd as zl

dev = torch.device("cuda:0")
REC, NUNIQ, TILE = 4096, 8192, 32


def timed(fn, iters=5):
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize(); ts.append(e0.elapsed_time(e1))
    return ts


def case_a():
    nblocks, block = 65536, 65536
    slot = (zl.compressBound(block) + 15) // 16 * 16
    inp = bench.make_device_blocks("text", nblocks, block, dev, seed=1)
    ar = torch.arange(nblocks, dtype=torch.int64, device=dev)
    in_len = torch.full((nblocks,), block, dtype=torch.int32, device=dev)
    cap = torch.full((nblocks,), slot, dtype=torch.int32, device=dev)
    comp = torch.empty(nblocks * slot, dtype=torch.uint8, device=dev)
    res = torch.empty(nblocks, dtype=torch.int64, device=dev)
    zl.batch_compress_fast(inp, ar * block, in_len, comp, ar * slot, cap, res, block, 1)
    torch.cuda.synchronize()
    clen = res.to(torch.int32)
    out = torch.empty_like(inp); ds = torch.empty(nblocks, dtype=torch.int64, device=dev)
    d_dict = torch.zeros(16, dtype=torch.uint8, device=dev)
    z64 = torch.zeros(nblocks, dtype=torch.int64, device=dev)
    z32 = torch.zeros(nblocks, dtype=torch.int32, device=dev)
    plain = lambda: zl.batch_decompress_safe(comp, ar * slot, clen, out, ar * block, in_len, ds)
    dct = lambda: zl.batch_decompress_safe_using_dict(comp, ar * slot, clen, out, ar * block, in_len, d_dict, z64, z32, ds)
    ta, tb = [], []
    for _ in range(3):        # interleaved: the two kernels see the same clocks
        ta += timed(plain, 2); tb += timed(dct, 2)
    ok = bool((ds == block).all()) and torch.equal(out, inp)
    gib = nblocks * block / 2**30
    print("(a) configs[1] D-text, empty dict: decompressSafe %.2f ms (%.1f GiB/s), usingDict %.2f ms (%.1f GiB/s), "
          "ratio %.3f, roundtrip_ok=%s" % (min(ta), gib / min(ta) * 1e3, min(tb), gib / min(tb) * 1e3, min(tb) / min(ta), ok))


def records():
    pool = bytes(dg.text_bytes(NUNIQ * REC, 31))
    dict_shared = bytes(dg.text_bytes(65536, 32))
    return pool, dict_shared


def encode(pool, dct, shared, tmp):
    enc_lib = dictgen.encoder(tmp)          # compiles tests/dict_encoder.c
    lib = C.CDLL(os.path.join(tmp, "libdict_encoder.so"))
    lib.dict_encode_batch.restype = C.c_int64
    slot = REC + REC // 255 + 16
    src = (C.c_uint8 * len(pool)).from_buffer_copy(pool)
    d = (C.c_uint8 * len(dct)).from_buffer_copy(dct)
    dst = (C.c_uint8 * (slot * NUNIQ))()
    ln = (C.c_int64 * NUNIQ)()
    st = (C.c_uint64 * 4)()
    if shared:
        assert lib.dict_encode_batch(d, C.c_size_t(len(dct)), src, C.c_size_t(REC), C.c_size_t(NUNIQ), 1, dst,
                                     C.c_size_t(slot), ln, st) == 0
        streams = [bytes(dst[i * slot: i * slot + ln[i]]) for i in range(NUNIQ)]
        stats = list(st)
    else:   # record i with record i - 1 (cyclic: record 0 with the last one, as the tiling places it)
        streams, stats = [], [0, 0, 0, 0]
        for i in range(NUNIQ):
            prev = pool[((i - 1) % NUNIQ) * REC: ((i - 1) % NUNIQ + 1) * REC]
            s, t = enc_lib(prev, pool[i * REC: (i + 1) * REC])
            streams.append(s)
            stats = [a + b for a, b in zip(stats, t)]
    return streams, stats


def case_bc(shared, pool, dict_shared, tmp):
    streams, st = encode(pool, dict_shared, shared, tmp)
    n = NUNIQ * TILE
    buf, offs, lens = __import__("gpu_harness")._pack(streams)
    span = len(buf)
    d_in = torch.from_numpy(np.tile(buf, TILE)).to(dev)
    in_off = torch.from_numpy(np.concatenate([offs + k * span for k in range(TILE)])).to(dev)
    in_len = torch.from_numpy(np.tile(lens, TILE).astype(np.int32)).to(dev)
    out = torch.empty(n * REC, dtype=torch.uint8, device=dev)
    out_off = torch.arange(n, dtype=torch.int64, device=dev) * REC
    cap = torch.full((n,), REC, dtype=torch.int32, device=dev)
    res = torch.empty(n, dtype=torch.int64, device=dev)
    if shared:
        d_dict = torch.from_numpy(np.frombuffer(dict_shared, dtype=np.uint8).copy()).to(dev)
        d_off = torch.zeros(n, dtype=torch.int64, device=dev)
        d_len = torch.full((n,), len(dict_shared), dtype=torch.int32, device=dev)
    else:
        d_dict = torch.from_numpy(np.frombuffer(pool, dtype=np.uint8).copy()).to(dev)
        idx = (torch.arange(n, dtype=torch.int64, device=dev) - 1) % NUNIQ
        d_off = idx * REC
        d_len = torch.full((n,), REC, dtype=torch.int32, device=dev)
    run = lambda: zl.batch_decompress_safe_using_dict(d_in, in_off, in_len, out, out_off, cap, d_dict, d_off, d_len, res)
    ts = timed(run, 6)
    want = torch.from_numpy(np.frombuffer(pool, dtype=np.uint8).copy()).to(dev)
    ok = bool((res == REC).all()) and torch.equal(out.view(TILE, -1), want.unsqueeze(0).expand(TILE, -1))
    gib = n * REC / 2**30
    share = st[0] / max(1, st[0] + st[1])
    name = "(b) shared 64 KiB dict" if shared else "(c) per-block dict (previous record)"
    print("%s: %d x 4 KiB D-text, ratio %.2f, match bytes from the dictionary %.1f %% (%d wholly-in-dict, %d spanning "
          "matches per %d records): ms %s -> %.1f GiB/s output, ok=%s" % (
              name, n, NUNIQ * REC / sum(lens), 100 * share, st[2], st[3], NUNIQ, ["%.2f" % t for t in ts],
              gib / min(ts) * 1e3, ok))
    if shared:
        lz = dictgen.liblz4()
        if lz is None:
            print("(b) liblz4: not present")
            return
        fn = lz.fn
        obuf = (C.c_uint8 * REC)()
        dbuf = (C.c_uint8 * len(dict_shared)).from_buffer_copy(dict_shared)
        sb = [(C.c_uint8 * len(s)).from_buffer_copy(s) for s in streams]
        t0 = time.perf_counter()
        for s, b in zip(streams, sb):
            r = fn(b, obuf, len(s), REC, dbuf, len(dict_shared))
            assert r == REC
        dt = time.perf_counter() - t0
        print("(b) liblz4 LZ4_decompress_safe_usingDict, one host core, %d records: %.1f ms -> %.2f GiB/s (incl. ctypes)"
              % (NUNIQ, dt * 1e3, NUNIQ * REC / dt / 2**30))


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    if what in ("a", "all"):
        case_a()
        torch.cuda.empty_cache()
    if what in ("b", "c", "all"):
        pool, dict_shared = records()
        with tempfile.TemporaryDirectory() as tmp:
            if what in ("b", "all"):
                case_bc(True, pool, dict_shared, tmp)
            if what in ("c", "all"):
                case_bc(False, pool, dict_shared, tmp)


if __name__ == "__main__":
    main()
