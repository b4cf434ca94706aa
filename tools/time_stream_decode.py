#!/usr/bin/env python3
"""Timing of zlz4_batch_decompress_safe_continue (StreamDecode over whole streams) on the GPU: HIP events around the
batch call, warm-up, median of --reps.  Cases (profiles/r08_stream_decode.md):
  a  N x 64 KiB D-text blocks (compressDefault) as ONE run, against zlz4_batch_decompress_safe on the same blocks
  b  the same blocks as N one-call runs
  c  4 KiB records as runs of 64 with a shared 64 KiB dictionary pending at each run's start
  d  (a) with 1 % corrupt blocks
  e  per-call latency of zlz4_decompress_safe_continue against zlz4_decompress_safe (host buffers)
  w  the serial walk of k_sd_finish: 64 runs that open with 70 corrupt calls (more than k_sd_plan looks back), then 32 x
     (a corrupt call, a 64 KiB block); every block is re-decoded by its run's one wavefront
Prints one line per case."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, warm, reps):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def main():
    import torch
    import datagen as dg
    import zig_lz4_amd as zl
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=65536)
    ap.add_argument("--records", type=int, default=262144)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n, B = a.blocks, 65536
    # compress on the device (the flagship compressor), 64 distinct D-text blocks repeated
    uniq = 64
    raw = torch.from_numpy(np.ascontiguousarray(dg.make_blocks("text", uniq, B, seed=1)).reshape(-1)).to(dev)
    cap = zl.compressBound(B)
    comp = torch.empty(uniq * cap, dtype=torch.uint8, device=dev)
    i64 = lambda x: torch.tensor(x, dtype=torch.int64, device=dev)  # noqa: E731
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)  # noqa: E731
    res = torch.empty(uniq, dtype=torch.int64, device=dev)
    zl.batch_compress_fast(raw, i64([i * B for i in range(uniq)]), i32([B] * uniq), comp, i64([i * cap for i in range(uniq)]),
                           i32([cap] * uniq), res, B)
    clen = res.cpu().tolist()
    in_off = i64([(i % uniq) * cap for i in range(n)])
    in_len = i32([clen[i % uniq] for i in range(n)])
    d_out = torch.empty(n * B, dtype=torch.uint8, device=dev)
    out_off = i64([i * B for i in range(n)])
    out_cap = i32([B] * n)
    result = torch.empty(n, dtype=torch.int64, device=dev)
    gib = n * B / 2**30
    plain = timed(lambda: zl.batch_decompress_safe(comp, in_off, in_len, d_out, out_off, out_cap, result), a.warmup, a.reps)
    print("plain batch_decompress_safe: %d x 64 KiB  %.3f ms  %.1f GiB/s" % (n, plain, gib / plain * 1e3))

    def stream_case(name, run_start, in_len_t, ns, state_init=None):
        state = torch.zeros((ns, 4), dtype=torch.int64, device=dev)
        ws = torch.empty(zl.batch_decompress_safe_continue_workspace(n, ns), dtype=torch.uint8, device=dev)

        def go():
            if state_init is None:
                state.zero_()
            else:
                state.copy_(state_init)
            zl.batch_decompress_safe_continue(comp, in_off, in_len_t, d_out, out_off, out_cap, run_start, state, result, ws)
        t = timed(go, a.warmup, a.reps)
        r = result.cpu()
        print("%s: %.3f ms  %.1f GiB/s  %.3fx plain  (%d ok, %d failed)" % (name, t, gib / t * 1e3, t / plain,
                                                                            int((r >= 0).sum()), int((r < 0).sum())))
    stream_case("(a) one run", i32([0, n]), in_len, 1)
    stream_case("(b) %d one-call runs" % n, i32(list(range(n + 1))), in_len, n)
    rng = np.random.default_rng(3)
    bad = rng.random(n) < 0.01
    comp_bad_len = [1 if bad[i] else clen[i % uniq] for i in range(n)]   # a 1-byte stream with a literal run: corrupt
    stream_case("(d) one run, 1 % corrupt", i32([0, n]), i32(comp_bad_len), 1)

    # (w) the good blocks go to ascending slots, each behind a corrupt call whose slot lies above them all: a block's true
    # entry bound is 0, the guessed one (from the call in front of it) is not, and no plan round sees a success
    W, G = 64, 32
    per = 70 + 2 * G
    blk, slot = [], []
    for s in range(W):
        for j in range(per):
            good = j >= 70 and (j - 70) % 2 == 1
            blk.append((s * G + (j - 70) // 2) % uniq if good else -1)
            slot.append(s * G + (j - 70) // 2 if good else W * G)
    w_in_off = i64([max(b, 0) * cap for b in blk])
    w_in_len = i32([clen[b] if b >= 0 else 1 for b in blk])
    w_out = torch.empty((W * G + 1) * B, dtype=torch.uint8, device=dev)
    w_out_off, w_out_cap = i64([k * B for k in slot]), i32([B] * len(blk))
    w_res = torch.empty(len(blk), dtype=torch.int64, device=dev)
    w_state = torch.zeros((W, 4), dtype=torch.int64, device=dev)
    w_ws = torch.empty(zl.batch_decompress_safe_continue_workspace(len(blk), W), dtype=torch.uint8, device=dev)
    w_runs = i32([per * s for s in range(W + 1)])

    def gow():
        w_state.zero_()
        zl.batch_decompress_safe_continue(comp, w_in_off, w_in_len, w_out, w_out_off, w_out_cap, w_runs, w_state, w_res, w_ws)
    t = timed(gow, a.warmup, a.reps)
    wr = w_res.cpu()
    wgib = W * G * B / 2**30
    print("(w) %d runs of 70 corrupt calls + %d x (corrupt, 64 KiB), the serial walk: %.3f ms  %.2f GiB/s  (%d ok, %d failed)" %
          (W, G, t, wgib / t * 1e3, int((wr >= 0).sum()), int((wr < 0).sum())))

    # (c) 4 KiB records, runs of 64, a shared 64 KiB dictionary pending at each run's start.  The records are compressed
    # without the dictionary (no device dict encoder): the dictionary path is taken and consumed, bytes as plain.
    R, rl = a.records, 4096
    rraw = torch.from_numpy(np.ascontiguousarray(dg.make_blocks("text", 256, rl, seed=5)).reshape(-1)).to(dev)
    rcap = zl.compressBound(rl)
    rcomp = torch.empty(256 * rcap, dtype=torch.uint8, device=dev)
    rres = torch.empty(256, dtype=torch.int64, device=dev)
    zl.batch_compress_fast(rraw, i64([i * rl for i in range(256)]), i32([rl] * 256), rcomp,
                           i64([i * rcap for i in range(256)]), i32([rcap] * 256), rres, rl)
    rlen = rres.cpu().tolist()
    ns = R // 64
    dct = torch.from_numpy(np.ascontiguousarray(dg.make_blocks("text", 1, 65536, seed=9)).reshape(-1)).to(dev)
    st0 = torch.zeros((ns, 4), dtype=torch.int64, device=dev)
    st0[:, 0] = dct.data_ptr()
    st0[:, 1] = 65536
    r_in_off, r_in_len = i64([(i % 256) * rcap for i in range(R)]), i32([rlen[i % 256] for i in range(R)])
    r_out = torch.empty(R * rl, dtype=torch.uint8, device=dev)
    r_out_off, r_out_cap = i64([i * rl for i in range(R)]), i32([rl] * R)
    r_res = torch.empty(R, dtype=torch.int64, device=dev)
    state = torch.empty_like(st0)
    ws = torch.empty(zl.batch_decompress_safe_continue_workspace(R, ns), dtype=torch.uint8, device=dev)
    run_start = i32([64 * s for s in range(ns + 1)])

    def goc():
        state.copy_(st0)
        zl.batch_decompress_safe_continue(rcomp, r_in_off, r_in_len, r_out, r_out_off, r_out_cap, run_start, state, r_res, ws)
    t = timed(goc, a.warmup, a.reps)
    rr = r_res.cpu()
    rgib = R * rl / 2**30
    print("(c) %d x 4 KiB in %d runs of 64, dictionary pending: %.3f ms  %.1f GiB/s  (%d ok)" % (R, ns, t, rgib / t * 1e3,
                                                                                               int((rr >= 0).sum())))
    # (e) single-call latency on host buffers
    src = comp[:clen[0]].cpu().numpy().tobytes()
    dst = np.zeros(B, dtype=np.uint8)
    sd = zl.StreamDecode()
    lat = {}
    for name, fn in (("decompressSafe", lambda: zl.decompressSafe(src, B)),
                     ("decompressSafeContinue", lambda: sd.decompressSafeContinue(src, dst))):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(20):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        lat[name] = statistics.median(ts)
    print("(e) per call, one 64 KiB block: decompressSafe %.3f ms, decompressSafeContinue %.3f ms" %
          (lat["decompressSafe"], lat["decompressSafeContinue"]))


if __name__ == "__main__":
    main()
