"""k_compress_fast reads the window's bytes out of the ring's snapshot in one hop and ranks lanes with mbcnt / tests them
with the mask itself (see the kernel and DESIGN.md): every block byte for byte and status for status against the oracle,
at the smallest shapes where the new forms can go wrong -- every lane shift of the snapshot with its wrap past lane 63,
the ring's move and reload, the flush's extension bytes, the seeded and dictionary builds, the u32 builds, and the flush
under a short destination."""
import numpy as np
import pytest
import torch

import datagen as dg
import dictcgen as dc
import gpu_harness as gh
import streamgen as sg

pytestmark = pytest.mark.gpu

GENS = (dg.text_bytes, dg.reptext_bytes, dg.mixed_bytes)


def _compress_at(zl, items, offs, dev, caps=None, max_in=None):
    """batch_compress_fast with block i at byte offset offs[i] of one input tensor that ends where the last block ends;
    output slots with guard bands.  -> [(status, bytes)]"""
    total = max(o + len(b) for o, b in zip(offs, items))
    buf = np.zeros(total, dtype=np.uint8)
    for o, b in zip(offs, items):
        buf[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
    lens = np.array([len(b) for b in items], dtype=np.int64)
    caps = np.asarray([zl.compressBound(len(b)) for b in items] if caps is None else caps, dtype=np.int64)
    out_offs, guard_ends, out_total = gh._out_slots(caps)
    d_in = torch.from_numpy(buf).to(dev)
    d_out = torch.full((out_total,), 0xA5, dtype=torch.uint8, device=dev)
    res = torch.full((len(items),), -999, dtype=torch.int64, device=dev)
    zl.batch_compress_fast(d_in, torch.from_numpy(np.array(offs, dtype=np.int64)).to(dev),
                           torch.from_numpy(lens.astype(np.uint32).view(np.int32)).to(dev), d_out,
                           torch.from_numpy(out_offs).to(dev), torch.from_numpy(caps.astype(np.uint32).view(np.int32)).to(dev),
                           res, int(lens.max()) if max_in is None else max_in, 1)
    torch.cuda.synchronize()
    assert (d_in.cpu().numpy() == buf).all(), "the input arena changed"
    return gh._collect(res, d_out, out_offs, guard_ends, caps)


def _cmp(got, want, names):
    bad = []
    for name, (n, data), w in zip(names, got, want):
        if isinstance(w, int):
            if n != w:
                bad.append("%s: status %d, oracle %d" % (name, n, w))
        elif n != len(w) or data != w:
            bad.append("%s: size %d vs oracle %d" % (name, n, len(w)))
    assert not bad, "%d/%d mismatches: %s" % (len(bad), len(names), "; ".join(bad[:8]))


def _sequences(stream):
    """(literal run, match length) of every sequence of an LZ4 block; the last one has match length 0"""
    out, p = [], 0
    while p < len(stream):
        t = stream[p]; p += 1
        lit = t >> 4
        if lit == 15:
            while True:
                x = stream[p]; p += 1; lit += x
                if x != 255:
                    break
        p += lit
        if p >= len(stream):
            out.append((lit, 0))
            break
        p += 2
        ml = t & 15
        if ml == 15:
            while True:
                x = stream[p]; p += 1; ml += x
                if x != 255:
                    break
        out.append((lit, ml + 4))
    return out


def test_every_alignment_and_lane_shift(zl, oracle, gpu):
    """256 blocks of 2 KiB..9 KiB, block i at i % 4 bytes past a 4-byte boundary.  The ring is reloaded at rbase = A & ~127
    and moves by 256 bytes, so a window's lane shift is s0 = (A - rbase) >> 2 with A - rbase < 256 and rbase a multiple
    of 128.  Every window starts where a match of the parse ends (or at 0).  The lengths step through every residue
    modulo 256, each block holds tens to hundreds of matches, and the test counts the parse's match ends in every residue
    of A modulo 256 and every A & 3: some thousands of windows over the 64 values of s0, half of them past the wrap at
    lane 63 (s0 >= 36 with the last dword read), with the ring's move at 256 and (D-reptext: long matches make the
    anchor jump) its reload at 512."""
    items, offs, names, pos = [], [], [], 0
    for i in range(256):
        n = 2048 + ((i * 7177) % 7168 // 256) * 256 + i          # 2 KiB .. 9 KiB, n mod 256 = i
        b = bytes(GENS[i % 3](n, 700 + i))
        pos = (pos + 3) // 4 * 4 + i % 4
        items.append(b); offs.append(pos); names.append("%s/%d@%d" % (GENS[i % 3].__name__, n, i % 4))
        pos += n
    assert sorted(set(len(b) % 256 for b in items)) == list(range(256))
    want = [oracle.compress_default(b) for b in items]
    ends = np.zeros(256, dtype=np.int64)
    for w in want:
        a = 0
        for lit, ml in _sequences(w):
            a += lit + ml
            if ml:
                ends[a % 256] += 1
    assert ends.min() > 0 and all(ends[r::4].sum() > 0 for r in range(4))
    _cmp(_compress_at(zl, items, offs, gpu), want, names)


def _run_block(n, seed):
    """literal runs of 15..63 fresh bytes between matches of 19..47 bytes against a pool at the block's start"""
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 256, 768, dtype=np.uint8).tobytes()
    parts, total, k = [pool], len(pool), 0
    while total < n:
        lit = 15 + (k * 5 + seed) % 49
        ml = 19 + (k * 3 + seed) % 29
        s = int(rng.integers(0, len(pool) - ml))
        parts.append(rng.integers(0, 256, lit, dtype=np.uint8).tobytes() + pool[s:s + ml])
        total += lit + ml
        k += 1
    return b"".join(parts)[:n]


def test_extension_bytes_of_literal_runs_and_matches(zl, oracle, gpu):
    items = [_run_block(3000 + 517 * k, k) for k in range(24)]
    want = [oracle.compress_default(b) for b in items]
    seqs = [s for w in want for s in _sequences(w)]
    lits = set(l for l, m in seqs if m)
    mls = set(m for l, m in seqs)
    assert set(range(15, 64)) <= lits and set(range(19, 48)) <= mls        # what the test is about is in the parse
    offs = [k * 16384 + k % 4 for k in range(len(items))]               # (the longest block has 14 891 bytes)
    _cmp(_compress_at(zl, items, offs, gpu), want, ["runs/%d" % len(b) for b in items])


def test_seeded_batch(zl, gpu, tmp_path):
    """64 compressFastContinue blocks (the u16 seeded build) with planted seeds, against the C restatement"""
    cref = sg.ref(tmp_path)
    items, tabs = [], []
    for k in range(64):
        b, v, G = sg.planted(2500 + 97 * k, 9100 + k, r_off=(20, 63, 100)[k % 3])
        t = np.zeros(4096, np.uint32)
        t[sg.hash4(G)] = v
        items.append(b)
        tabs.append(t)
    tabs = np.stack(tabs)
    caps = [len(b) + len(b) // 255 + 16 for b in items]
    got = sg.run_continue(zl, items, caps, tabs, None, gpu, max_in=65547)
    want = cref.batch(tabs, None, items, caps, 1)
    assert list(got[0]) == list(want[0]) and got[1] == want[1]
    assert all(np.array_equal(got[2][i], want[2][i]) for i in range(len(items)))


def test_dictionary_batch(zl, gpu, tmp_path):
    """64 records against a shared dictionary (k_compress_fast_dict, u16 table), against the C restatement"""
    cref = dc.ref(tmp_path)
    text = bytes(dg.text_bytes(40000 + 64 * 3000, 78))
    d = text[:40000]
    recs = [text[40000 + 3000 * k: 40000 + 3000 * k + 2000 + 13 * k] for k in range(64)]
    got, want = dc.run_batch(zl, cref, recs, [dc.bound(len(r)) for r in recs], [d], [0] * 64, gpu)
    dc.check(got, want)


@pytest.mark.parametrize("max_in", [None, (1 << 24) + 1])
def test_u32_builds(zl, oracle, gpu, max_in):
    """one block of 65 548 bytes and one of 1 MiB: the u32 table with tags, and (declared bound above 2^24) without"""
    items = [bytes(dg.text_bytes(65548, 31)), bytes(dg.mixed_bytes(1 << 20, 32))]
    offs = [1, 65552 + 2]
    _cmp(_compress_at(zl, items, offs, gpu, max_in=max_in), [oracle.compress_default(b) for b in items], ["65548", "1MiB"])


def test_flush_under_a_short_destination(zl, oracle, gpu):
    """capacities that leave less than 512 bytes of room in the last windows (`tight`: every sequence takes the exact
    step), down to the first byte that does not fit"""
    items, caps, names = [], [], []
    for k, n in enumerate((2500, 5000, 9000)):
        for gen in GENS:
            b = bytes(gen(n, 60 + k))
            full = len(oracle.compress_default(b))
            for c in (full + 511, full + 300, full + 64, full + 1, full, full - 1, full - 200, 400):
                items.append(b); caps.append(c); names.append("%s/%d/cap%d" % (gen.__name__, n, c))
    want = [oracle.compress_default(b, cap=c) for b, c in zip(items, caps)]
    offs = [k * 9216 + k % 4 for k in range(len(items))]
    _cmp(_compress_at(zl, items, offs, gpu, caps=caps), want, names)
