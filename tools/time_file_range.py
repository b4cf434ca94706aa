#!/usr/bin/env python3
"""Timing of the file index and of file range decoding (zlz4f_batch_file_index, zlz4f_batch_decompress_file_range, DESIGN.md
section 4.4k) against the calls that existed before them, on the same buffers.

Input (bench.make_device_blocks, D-text, compressed on the device): --files files of --per-file members, each member one
64 KiB chunk written as a one-block modern frame; shape "modern" keeps them all, shape "legacy4" writes every fourth member
as a legacy frame of one 64 KiB block.

 index   zlz4f_batch_file_index against what decompressFiles runs to learn the sizes: the frame size query, the legacy size
         query and the select over the split's items (the split itself is common to both and timed beside them).
 r4k     4 KiB per file at a mid-file offset: plan + range decode, against the full decode of decompressFiles (plan, the
         two decodes, select, finish).
 r64k    64 KiB per file across a member boundary (in legacy4: from a legacy member into a frame member).
 cover   --per-file ranges per file that cover it.

The steps alternate inside one process: HIP events around each call, the stream synchronised after each, warm-up, --reps
alternations; median and spread (min .. max) per call.  Before timing, every index entry and every decoded byte is compared
with the input.  Writes the table to --out (profiles/r34_file_ranges.md)."""
import argparse
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
    ap.add_argument("--files", type=int, default=4096)
    ap.add_argument("--per-file", type=int, default=16)
    ap.add_argument("--shapes", default="modern,legacy4")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r34_file_ranges.md"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    assert zl.device_available(), "needs a gfx950 device"
    lz4f = zl.lz4f
    nbuf, k, bs = a.files, a.per_file, 65536
    n = nbuf * k
    assert k % 4 == 0
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def alternate(calls):
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
            say("| %s | %.3f | %.3f .. %.3f | %d |" % (label, med[label], min(t), max(t), len(t)))
        return med

    def i64(m):
        return torch.zeros(max(1, m), dtype=torch.int64, device=dev)[:m]

    def full(m, v):
        return torch.full((m,), v, dtype=torch.int64, device=dev)

    def u8(m):
        return torch.empty(max(16, m), dtype=torch.uint8, device=dev)

    def pack(rows, lens):
        col = torch.arange(rows.shape[1], dtype=torch.int64, device=dev)
        parts = []
        for lo in range(0, rows.shape[0], 2048):
            hi = min(rows.shape[0], lo + 2048)
            parts.append(rows[lo:hi][col[None, :] < lens[lo:hi, None]])
        ends = torch.cumsum(lens, 0)
        return torch.cat(parts), ends - lens, ends

    ar = torch.arange(n, dtype=torch.int64, device=dev)
    raw = make_device_blocks("text", n, bs, dev, seed=1).reshape(-1)
    out = torch.empty(n * bs, dtype=torch.uint8, device=dev)
    lp = zl.LegacyPrefs(bs, 0)
    prefs = zl.Prefs()
    prefs.block_mode = 1
    fb, lb = lz4f.compressFrameBound(bs, prefs), lz4f.legacyCompressFrameBound(bs, lp)
    stride = max(fb, lb)
    rows = torch.empty((n, stride), dtype=torch.uint8, device=dev)
    cres = i64(n)
    lz4f.compressFrameBatch(raw, ar * bs, full(n, bs), rows.view(-1), ar * stride, full(n, stride), cres, prefs, 0, n)
    torch.cuda.synchronize()
    assert bool((cres > 0).all()), "compression failed"
    first = torch.arange(nbuf, dtype=torch.int64, device=dev) * k
    say("# File index and file range decoding on the MI355X (`tools/time_file_range.py`)")
    say()
    say("%d files of %d members, each member one 64 KiB chunk of D-text; times in ms, median of %d alternations (min .. max)."
        % (nbuf, k, a.reps))

    for shape in a.shapes.split(","):
        mlen = cres.clone()
        nl = 0
        if shape == "legacy4":
            q = ar[3::4].contiguous()
            nl = q.numel()
            lrows = torch.empty((nl, lb), dtype=torch.uint8, device=dev)
            lres = i64(nl)
            lz4f.compressLegacyFrameBatch(raw, q * bs, full(nl, bs), lrows.view(-1),
                                          torch.arange(nl, dtype=torch.int64, device=dev) * lb, full(nl, lb), lres, lp, nl)
            torch.cuda.synchronize()
            assert bool((lres > 0).all()), "legacy compression failed"
            rows[q, :lb] = lrows
            mlen[q] = lres
            del lrows
        packed, m_off, ends = pack(rows, mlen)
        src_off = m_off[first].contiguous()
        src_len = (ends[first + k - 1] - src_off).contiguous()
        say()
        say("## %s: %d of %d members legacy, %.1f MiB compressed, %.1f MiB content" % (shape, nl, n, packed.numel() / 2**20,
                                                                                        n * bs / 2**20))
        say()
        say("| call | median | min .. max | runs |")
        say("|---|---|---|---|")
        LEG, LINKED = lz4f.SPLIT_LEGACY, lz4f.DECODE_LINKED
        totals_h = (n, n - nl, nl, nl)
        count, totals, ptotals = i64(nbuf), i64(4), i64(2)
        member = torch.zeros((n, 3), dtype=torch.int64, device=dev)
        mem_cap = full(nbuf, k)
        item_first, item_off, item_len, leg_len, sres = i64(nbuf + 1), i64(n), i64(n), i64(n), i64(nbuf)
        size, lsize, dst_off, dst_cap, ires, lres2 = (i64(n) for _ in range(6))
        out_off, out_size, res = i64(nbuf), i64(nbuf), i64(nbuf)
        qws = u8(lz4f.frameDecompressedSizeBatchWorkspace(n, n - nl, LINKED))
        dws = u8(lz4f.decompressFrameBatchWorkspace(n, n - nl, LINKED))
        lqws = u8(lz4f.legacyFrameDecompressedSizeBatchWorkspace(n, nl))
        ldws = u8(lz4f.decompressLegacyFrameBatchWorkspace(n, nl))
        cap = n + nbuf
        index = torch.zeros((cap, 2), dtype=torch.int64, device=dev)
        idx_off, idx_n = i64(nbuf + 1), i64(nbuf)
        iws = u8(lz4f.fileIndexBatchWorkspace(nbuf, totals_h))

        def split():
            lz4f.multiframeSplitBatchEx(packed, src_off, src_len, count, totals, split_flags=LEG)
            lz4f.multiframeSplitBatchEx(packed, src_off, src_len, count, totals, member, first, mem_cap, item_first, item_off,
                                        item_len, sres, LEG, leg_len)

        def sizes():
            lz4f.frameDecompressedSizeBatch(packed, item_off, item_len, size, n - nl, qws, LINKED)
            if nl:
                lz4f.legacyFrameDecompressedSizeBatch(packed, item_off, leg_len, lsize, None, nl, lqws)
                lz4f.multiframeSelectBatch(member, first, sres, item_first, size, lsize, size)

        def decode():
            lz4f.multiframePlanBatch(size, item_first, dst_off, dst_cap, out_off, out_size, ptotals, 0)
            lz4f.decompressFrameBatch(packed, item_off, item_len, out, dst_off, dst_cap, ires, n - nl, dws, LINKED)
            if nl:
                lz4f.decompressLegacyFrameBatch(packed, item_off, leg_len, out, dst_off, dst_cap, lres2, None, nl, ldws)
                lz4f.multiframeSelectBatch(member, first, sres, item_first, ires, lres2, ires)
            lz4f.multiframeFinishBatch(member, first, sres, item_first, size, ires, res)

        def file_index():
            lz4f.fileIndexBatch(packed, src_off, src_len, member, first, sres, item_first, item_off, item_len, leg_len, totals_h,
                                index, idx_off, idx_n, cap, iws)

        split()
        sizes()
        out.zero_()
        decode()
        file_index()
        torch.cuda.synchronize()
        assert totals.tolist() == list(totals_h) and bool((res == k * bs).all()) and torch.equal(out, raw), "the full decode"
        assert bool((idx_n == k).all()) and idx_off.tolist() == [(k + 1) * s for s in range(nbuf + 1)], "the index"
        ix = index.view(nbuf, k + 1, 2)
        assert bool((ix[:, :, 1] == (torch.arange(k + 1, device=dev) * bs)[None, :]).all()), "dec"
        hdr = torch.where(leg_len > 0, 4, 7).view(nbuf, k)
        assert bool((ix[:, :k, 0] == (item_off.view(nbuf, k) - src_off[:, None] + hdr)).all()), "pos"

        def ranges_of(kind):
            f = np.arange(nbuf, dtype=np.uint64)
            if kind == "r4k":
                a0 = np.full(nbuf, (k // 2) * bs + 1000, dtype=np.uint64)
                return np.stack([f, a0, a0 + 4096], 1)
            if kind == "r64k":
                a0 = np.full(nbuf, 3 * bs + bs // 2, dtype=np.uint64)
                return np.stack([f, a0, a0 + bs], 1)
            j = np.arange(k, dtype=np.uint64)
            return np.stack([np.repeat(f, k), np.tile(j * bs, nbuf), np.tile((j + 1) * bs, nbuf)], 1)

        calls = [("split: count + record (common)", split), ("parent: size queries + select", sizes),
                 ("file index", file_index), ("parent: full decode (plan, decodes, select, finish)", decode)]
        checks = []
        for kind in ("r4k", "r64k", "cover"):
            rng = ranges_of(kind)
            nr = rng.shape[0]
            d_range = torch.from_numpy(np.ascontiguousarray(rng).view(np.int64)).to(dev)
            r_off, r_cap, r_tot, skip, rres = i64(nr), i64(nr), i64(2), i64(nr), i64(nr)
            lz4f.planFrameRanges(index, idx_off, idx_n, d_range, r_off, r_cap, r_tot)
            arena, items = r_tot.tolist()
            r_dst = u8(arena)
            rws = u8(lz4f.decompressFileRangeBatchWorkspace(nr, items))

            def run(d_range=d_range, r_off=r_off, r_cap=r_cap, r_tot=r_tot, skip=skip, rres=rres, r_dst=r_dst, rws=rws, items=items):
                lz4f.planFrameRanges(index, idx_off, idx_n, d_range, r_off, r_cap, r_tot)
                lz4f.decompressFileRangeBatch(packed, src_off, src_len, index, idx_off, idx_n, member, first, sres, d_range, r_dst,
                                              r_off, r_cap, skip, rres, items, rws)

            run()
            torch.cuda.synchronize()
            want = torch.from_numpy((rng[:, 2] - rng[:, 1]).astype(np.int64)).to(dev)
            assert torch.equal(rres, want), kind
            for r in range(0, nr, max(1, nr // 64)):                  # sampled ranges, byte for byte
                f, lo, hi = (int(x) for x in rng[r])
                o = int(r_off[r]) + int(skip[r])
                assert torch.equal(r_dst[o:o + hi - lo], raw[f * k * bs + lo:f * k * bs + hi]), (kind, r)
            calls.append(("%s: plan + file range decode (%d ranges, %d blocks, %.1f MiB arena)" % (kind, nr, items, arena / 2**20), run))
            checks.append(kind)
        med = alternate(calls)
        say()
        say("index / (size queries + select) = %.3f; against the full decode: r4k %.3f, r64k %.3f, cover %.3f" % (
            med["file index"] / med["parent: size queries + select"],
            *[[v for l, v in med.items() if l.startswith(kind + ":")][0] / med["parent: full decode (plan, decodes, select, finish)"]
              for kind in checks]))
        del packed, index, member
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
