#!/usr/bin/env python3
"""Timing of the legacy frame calls (zlz4f_batch_compress_legacy_frame, zlz4f_batch_legacy_frame_count,
zlz4f_batch_legacy_frame_decompressed_size, zlz4f_batch_decompress_legacy_frame) against the block
calls they contain, so that what the frame layer adds can be read off.

  big:  --frames frames of --frame-mib MiB of D-text (bench.make_device_blocks) at block sizes 8 MiB and 64 KiB, at the
        fast level and at level 9.  Yardstick of the compress call: zlz4_batch_compress_fast / zlz4_batch_compress_hc on the
        same chunks alone, into compressBound slots.  Yardstick of the size query and the decode: zlz4_batch_decompressed_size
        and zlz4_batch_decompress_safe on the same compressed blocks alone, with the decoded sizes known.
  many: --many frames of one 64 KiB block, against the modern zlz4f_batch_compress_frame / zlz4f_batch_frame_decompressed_size
        / zlz4f_batch_decompress_frame on the same inputs.

The calls of a comparison alternate inside one process: HIP events around each call, the stream synchronised after each,
warm-up, --reps alternations; median and spread (min .. max) per call.  Before timing, frame sizes are checked against the
block results and every decoded byte against the input.  (profiles/r32_legacy_frames.md)"""
import argparse
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
    ap.add_argument("--sections", default="big,many")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--frame-mib", type=int, default=64)
    ap.add_argument("--block-sizes", default="8388608,65536")
    ap.add_argument("--levels", default="0,9")
    ap.add_argument("--many", type=int, default=65536)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    assert zl.device_available(), "needs a gfx950 device"
    lz4f = zl.lz4f
    levels = [int(x) for x in a.levels.split(",")]

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
        med = {}
        for (label, _), t in zip(calls, times):
            med[label] = statistics.median(t)
            print("%-22s %-40s %10.3f ms  (%.3f .. %.3f, %d runs)" % (title, label, med[label], min(t), max(t), len(t)),
                  flush=True)
        return med

    def i64(k, v=0):
        return torch.full((max(1, k),), v, dtype=torch.int64, device=dev)[:k]

    def i32(k, v=0):
        return torch.full((max(1, k),), v, dtype=torch.int32, device=dev)[:k]

    def u8(k):
        return torch.empty(max(16, k), dtype=torch.uint8, device=dev)

    def ar(k):
        return torch.arange(k, dtype=torch.int64, device=dev)

    def added(title, what, legacy, yard):
        print("%-22s %s: legacy %.3f ms, yardstick %.3f ms, the frame layer adds %.3f ms = %.3f of the yardstick" %
              (title, what, legacy, yard, legacy - yard, (legacy - yard) / yard), flush=True)

    def legacy_side(title, raw, nf, flen, bs, level, decode):
        """compress nf frames of flen bytes at block size bs; with `decode`, the size query and the decode of those frames"""
        gib = nf * flen / 2**30
        per = (flen + bs - 1) // bs
        m = nf * per
        prefs = zl.LegacyPrefs(bs, level)
        bound = lz4f.legacyCompressFrameBound(flen, prefs)
        src_off, src_len = ar(nf) * flen, i64(nf, flen)
        dst, dst_off, dst_cap, res = u8(nf * bound), ar(nf) * bound, i64(nf, bound), i64(nf)
        ws = u8(lz4f.compressLegacyFrameBatchWorkspace(nf, m, prefs))
        slot = (zl.compressBound(bs) + 15) // 16 * 16
        starts = (ar(m) // per) * flen + (ar(m) % per) * bs
        lens = torch.minimum(i64(m, bs), (ar(m) // per) * flen + flen - starts).to(torch.int32)
        yslots, y_off, y_cap, cres = u8(m * slot), ar(m) * slot, i32(m, slot), i64(m)
        hws = u8(zl.batch_compress_hc_workspace(m, bs)) if level > 0 else None
        calls = [("legacy compress", lambda: lz4f.compressLegacyFrameBatch(raw, src_off, src_len, dst, dst_off, dst_cap, res,
                                                                          prefs, m, ws))]
        if level > 0:
            calls.append(("yardstick: batch_compress_hc", lambda: zl.batch_compress_hc(raw, starts, lens, yslots, y_off, y_cap,
                                                                                       cres, bs, level, hws)))
        else:
            calls.append(("yardstick: batch_compress_fast", lambda: zl.batch_compress_fast(raw, starts, lens, yslots, y_off,
                                                                                           y_cap, cres, bs, 1)))
        for _, fn in calls:
            fn()
        torch.cuda.synchronize()
        assert bool((cres > 0).all()) and bool((res > 0).all()), "compression failed"
        assert torch.equal(res, 4 + (cres + 4).view(nf, per).sum(1)), "frame sizes are not the blocks' sizes"
        print("%-22s %d frames of %d B, %d blocks of %d B, level %d, ratio %.3f" %
              (title, nf, flen, m, bs, level, nf * flen / float(res.sum())), flush=True)
        med = alternate(title, calls)
        added(title, "compress (%.2f GiB)" % gib, med[calls[0][0]], med[calls[1][0]])
        print("%-22s legacy compress %.1f GiB/s, yardstick %.1f GiB/s" %
              (title, gib / med[calls[0][0]] * 1e3, gib / med[calls[1][0]] * 1e3), flush=True)
        if not decode:
            return
        del ws, hws
        nblocks, totals, size, dres = i64(nf), i64(1), i64(nf), i64(nf)
        lz4f.legacyFrameCountBatch(dst, dst_off, res, nblocks, None, totals)
        assert int(totals.item()) == m and bool((nblocks == per).all()), "count"
        out, o_off, o_cap = u8(nf * flen), ar(nf) * flen, i64(nf, flen)
        qws = u8(lz4f.legacyFrameDecompressedSizeBatchWorkspace(nf, m))
        dws = u8(lz4f.decompressLegacyFrameBatchWorkspace(nf, m))
        clen, ysize, yres, blen = cres.to(torch.int32), i64(m), i64(m), lens.clone()
        calls = [
            ("legacy count", lambda: lz4f.legacyFrameCountBatch(dst, dst_off, res, nblocks, None, totals)),
            ("legacy size query", lambda: lz4f.legacyFrameDecompressedSizeBatch(dst, dst_off, res, size, None, m, qws)),
            ("legacy decode", lambda: lz4f.decompressLegacyFrameBatch(dst, dst_off, res, out, o_off, o_cap, dres, None, m, dws)),
            ("yardstick: batch_decompressed_size", lambda: zl.batch_decompressed_size(yslots, y_off, clen, ysize)),
            ("yardstick: batch_decompress_safe", lambda: zl.batch_decompress_safe(yslots, y_off, clen, out, starts, blen, yres)),
        ]
        out.zero_()
        for _, fn in calls[:3]:
            fn()
        torch.cuda.synchronize()
        assert bool((size == flen).all()) and bool((dres == flen).all()), "legacy decode results"
        assert torch.equal(out[:nf * flen], raw.reshape(-1)[:nf * flen]), "the legacy decode is wrong"
        out.zero_()
        for _, fn in calls[3:]:
            fn()
        torch.cuda.synchronize()
        assert torch.equal(ysize, lens.to(torch.int64)) and torch.equal(yres, ysize), "yardstick results"
        assert torch.equal(out[:nf * flen], raw.reshape(-1)[:nf * flen]), "the yardstick decode is wrong"
        med = alternate(title, calls)
        added(title, "size query", med["legacy size query"], med["yardstick: batch_decompressed_size"])
        # the decode call holds the size pass too: its yardstick is both block calls
        added(title, "decode", med["legacy decode"],
              med["yardstick: batch_decompressed_size"] + med["yardstick: batch_decompress_safe"])
        print("%-22s legacy decode %.1f GiB/s, yardstick: batch_decompress_safe alone %.1f GiB/s" %
              (title, gib / med["legacy decode"] * 1e3, gib / med["yardstick: batch_decompress_safe"] * 1e3), flush=True)

    if "big" in a.sections.split(","):
        flen = a.frame_mib << 20
        raw = make_device_blocks("text", a.frames * flen // 65536, 65536, dev, seed=1).reshape(-1)
        for bs in (int(x) for x in a.block_sizes.split(",")):
            for level in levels:
                legacy_side("big bs=%d L%d" % (bs, level), raw, a.frames, flen, bs, level, decode=(level == levels[0]))
                torch.cuda.empty_cache()
        del raw
        torch.cuda.empty_cache()

    if "many" in a.sections.split(","):
        n, bs = a.many, 65536
        raw = make_device_blocks("text", n, bs, dev, seed=2).reshape(-1)
        src_off, src_len = ar(n) * bs, i64(n, bs)
        for level in levels:
            title = "many x64KiB L%d" % level
            lp = zl.LegacyPrefs(bs, level)
            mp = zl.Prefs()
            mp.block_size_id, mp.block_mode, mp.compression_level = 4, 1, level
            lb, fb = lz4f.legacyCompressFrameBound(bs, lp), lz4f.compressFrameBound(bs, mp)
            ldst, lres, lws = u8(n * lb), i64(n), u8(lz4f.compressLegacyFrameBatchWorkspace(n, n, lp))
            mdst, mres, mws = u8(n * fb), i64(n), u8(lz4f.compressFrameBatchWorkspace(n, n, mp))
            l_off, l_cap, m_off, m_cap = ar(n) * lb, i64(n, lb), ar(n) * fb, i64(n, fb)
            calls = [
                ("legacy compress", lambda: lz4f.compressLegacyFrameBatch(raw, src_off, src_len, ldst, l_off, l_cap, lres, lp, n,
                                                                          lws)),
                ("modern compress_frame", lambda: lz4f.compressFrameBatch(raw, src_off, src_len, mdst, m_off, m_cap, mres, mp, 0,
                                                                          n, mws)),
            ]
            for _, fn in calls:
                fn()
            torch.cuda.synchronize()
            assert bool((lres > 0).all()) and bool((mres > 0).all()), "compression failed"
            # a modern frame of one compressed block: 7 header bytes, the block word, the block, the end mark
            assert torch.equal(lres - 8, mres - 15), "the two frames do not hold the same block"
            med = alternate(title, calls)
            print("%-22s compress: legacy %.3f ms = %.3f of the modern call" %
                  (title, med["legacy compress"], med["legacy compress"] / med["modern compress_frame"]), flush=True)
            if level != levels[0]:
                continue
            del lws, mws
            out, o_off, o_cap = u8(n * bs), ar(n) * bs, i64(n, bs)
            lsize, ldres, msize, mdres, nblocks, totals = i64(n), i64(n), i64(n), i64(n), i64(n), i64(1)
            lq, ld = u8(lz4f.legacyFrameDecompressedSizeBatchWorkspace(n, n)), u8(lz4f.decompressLegacyFrameBatchWorkspace(n, n))
            mq, md = u8(lz4f.frameDecompressedSizeBatchWorkspace(n, n)), u8(lz4f.decompressFrameBatchWorkspace(n, n))
            calls = [
                ("legacy count", lambda: lz4f.legacyFrameCountBatch(ldst, l_off, lres, nblocks, None, totals)),
                ("legacy size query", lambda: lz4f.legacyFrameDecompressedSizeBatch(ldst, l_off, lres, lsize, None, n, lq)),
                ("legacy decode", lambda: lz4f.decompressLegacyFrameBatch(ldst, l_off, lres, out, o_off, o_cap, ldres, None, n, ld)),
                ("modern size query", lambda: lz4f.frameDecompressedSizeBatch(mdst, m_off, mres, msize, n, mq)),
                ("modern decompress_frame", lambda: lz4f.decompressFrameBatch(mdst, m_off, mres, out, o_off, o_cap, mdres, n, md)),
            ]
            for k in (slice(0, 3), slice(3, 5)):
                out.zero_()
                for _, fn in calls[k]:
                    fn()
                torch.cuda.synchronize()
                assert torch.equal(out[:n * bs], raw), "decode is wrong"
            assert int(totals.item()) == n and bool((lsize == bs).all()) and bool((ldres == bs).all())
            assert bool((msize == bs).all()) and bool((mdres == bs).all())
            med = alternate(title, calls)
            print("%-22s size query: legacy %.3f of the modern call; decode: legacy %.3f of the modern call" %
                  (title, med["legacy size query"] / med["modern size query"],
                   med["legacy decode"] / med["modern decompress_frame"]), flush=True)
            del out, lq, ld, mq, md
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
