"""Streaming compression on the GPU (zlz4_batch_load_dict, zlz4_batch_compress_fast_continue, the single-buffer
zlz4_stream_* calls behind zig_lz4_amd.Stream; reference src/lz4.zig:751-866): bytes, statuses and tables against
zlz4_batch_compress_fast, the C restatement (tests/stream_ref.c) and the Python one (tools/pyref/zig_lz4_stream.py)."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "pyref"))
import datagen as dg  # noqa: E402
import gpu_harness as gh  # noqa: E402
import streamgen as sg  # noqa: E402
import zig_lz4_stream as zs  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cref(tmp_path_factory):
    return sg.ref(tmp_path_factory.mktemp("streamref"))


@pytest.fixture(scope="module")
def text():
    return bytes(dg.text_bytes(24 << 20, 4711))


def _bound(n):
    return n + n // 255 + 16


def _cmp(got, want, what):
    gr, go, gt = got
    wr, wo, wt = want
    bad = [i for i in range(len(wr)) if gr[i] != wr[i] or go[i] != wo[i]]
    assert not bad, "%s: %d blocks differ, first %s (GPU %d vs %d)" % (what, len(bad), bad[:8], gr[bad[0]], wr[bad[0]])
    if gt is not None and wt is not None:
        tb = [i for i in range(len(wr)) if not np.array_equal(gt[i], wt[i])]
        assert not tb, "%s: %d tables differ, first %s" % (what, len(tb), tb[:8])


@pytest.mark.parametrize("accel", [1, 2, 7, 65537])
@pytest.mark.parametrize("size", [65536, 262144])
def test_zero_tables_equal_batch_compress_fast(zl, gpu, cref, text, size, accel):
    """continue from zero tables == compressFast, both table widths (max_in_len <= 65547 and above)"""
    rng = np.random.default_rng(size + accel)
    n = 96 if size == 65536 else 24
    items = []
    for i in range(n):
        m = size if i % 3 else int(rng.integers(1, size + 1))
        gen = (dg.text_bytes, dg.reptext_bytes, dg.mixed_bytes, dg.zero_bytes, dg.random_bytes)[i % 5]
        items.append(bytes(gen(m, 100 + i)))
    items[0] = items[0][:12]
    caps = [_bound(len(b)) for b in items]
    fast = gh.compress_fast(zl, items, gpu, caps, accel=accel)
    zeros = np.zeros((n, 4096), np.uint32)
    got = sg.run_continue(zl, items, caps, zeros, None, gpu, accel=accel, max_in=size)
    assert [r for r in got[0]] == [r for r, _ in fast]
    assert got[1] == [c for _, c in fast]
    _cmp(got, cref.batch(zeros, None, items, caps, accel), "zero tables")


def test_load_dict_batch_matches_restatement(zl, gpu, cref, text):
    sizes = (0, 1, 3, 4, 5, 13, 65535, 65536, 65537, 200000)
    dicts = [text[i * 1000: i * 1000 + n] for i, n in enumerate(sizes)]
    dicts += [b"\x61" * 65536, b"\x61" * 200000, bytes(dg.random_bytes(65536, 3)), b"ab" * 40000]
    res, tabs = sg.run_load_dict(zl, dicts, gpu)
    for i, d in enumerate(dicts):
        t, r = cref.load_dict(d)
        assert res[i] == r == min(len(d), 65536), i
        assert np.array_equal(tabs[i], t), "table of dictionary %d (%d bytes) differs" % (i, len(d))
    pt, _ = zs.load_dict(dicts[7])
    assert list(tabs[7]) == pt


@pytest.mark.parametrize("nblocks", [2048, 6144])
def test_shared_dictionary_records(zl, gpu, cref, text, nblocks):
    """one loaded 64 KiB dictionary, thousands of 4..64 KiB records pointing at it"""
    rng = np.random.default_rng(nblocks)
    _, dtab = sg.run_load_dict(zl, [text[:65536]], gpu)
    items, pos = [], 65536
    for i in range(nblocks):
        n = int(rng.integers(4096, 65537))
        if pos + n > len(text):
            pos = 65536
        items.append(text[pos:pos + n])
        pos += n
    caps = [_bound(len(b)) for b in items]
    idx = np.zeros(nblocks, np.uint32)
    got = sg.run_continue(zl, items, caps, dtab, idx, gpu, max_in=65536)
    want = cref.batch(dtab, idx, items, caps, 1)
    _cmp(got, want, "shared dictionary")
    # every block decodes with plain decompressSafe (no block refers to the dictionary)
    dec = gh.decompress(zl, got[1], [len(b) for b in items], gpu)
    assert all(d == b for (_, d), b in zip(dec, items))
    # (at acceleration 1 on text the loaded table practically never changes a block: a seed is only read by the first
    #  probe of its slot, and must then point below ip at the same 4 bytes of the CURRENT block)


def test_chained_streams_across_table_widths(zl, gpu, cref, text):
    """several streams, in-place steps of 256 KiB, then 64 KiB, then 256 KiB: positions >= 65536 written by the first
    step cannot be loaded into the 16-bit table of the second, must pass through it and reach the third (whose bytes and
    tables must equal the restatement's, which loads them)"""
    nstreams = 64
    rng = np.random.default_rng(17)
    tables = np.zeros((nstreams, 4096), np.uint32)
    ctabs = tables.copy()
    base = [int(rng.integers(0, len(text) - (1 << 20))) for _ in range(nstreams)]
    off = [0] * nstreams
    for step, size in enumerate((262144, 65536, 262144, 4096, 262144)):
        items = []
        for s in range(nstreams):
            items.append(text[base[s] + off[s]: base[s] + off[s] + size - (s % 7)])
            off[s] += size
        caps = [_bound(len(b)) for b in items]
        want = cref.batch(ctabs, None, items, caps, 1)
        got = sg.run_continue(zl, items, caps, tables, None, gpu, max_in=size, in_place=True)
        _cmp(got, want, "step %d" % step)
        if size == 65536:
            assert (got[2] >= 65536).any(), "no large seed survived the 64 KiB step"
        tables = got[2]
        ctabs = want[2]


@pytest.mark.parametrize("size", [5000, 65536, 200000])
def test_adversarial_tables(zl, gpu, cref, text, size):
    rng = np.random.default_rng(size)
    n = 40
    items = [text[1000 + i * 7919: 1000 + i * 7919 + size - (i % 5) * 3] for i in range(n)]
    tabs = []
    for i, b in enumerate(items):
        L = len(b) - 12
        k = i % 6
        if k == 0: t = rng.integers(0, 2 * len(b) + 1, 4096)
        elif k == 1: t = rng.integers(L, 1 << 32, 4096)
        elif k == 2: t = np.full(4096, len(b) - 1)
        elif k == 3: t = np.arange(4096) * 16 + 1               # values near many probe positions (= ip for some)
        elif k == 4: t = np.where(rng.random(4096) < 0.5, rng.integers(1, L, 4096), rng.integers(L, L + 64, 4096))
        else: t = rng.integers(0, 1 << 32, 4096)
        tabs.append(t.astype(np.uint32))
    tabs = np.stack(tabs)
    caps = [_bound(len(b)) for b in items]
    got = sg.run_continue(zl, items, caps, tabs, None, gpu, max_in=size)
    _cmp(got, cref.batch(tabs, None, items, caps, 1), "adversarial")
    got2 = sg.run_continue(zl, items, caps, tabs, None, gpu, accel=3, max_in=size)
    _cmp(got2, cref.batch(tabs, None, items, caps, 3), "adversarial accel 3")
    # the Python restatement on a few
    for i in range(0, n, 9):
        r, o, t = zs.compress_fast_continue([int(x) for x in tabs[i]], items[i], 1)
        assert r == got[0][i] and o == got[1][i] and list(got[2][i]) == t


def test_kat_on_gpu(zl, gpu):
    vs = json.load(open(os.path.join(ROOT, "tests", "golden", "stream_kat.json")))["vectors"]
    tabs = np.zeros((len(vs), 4096), np.uint32)
    for i, v in enumerate(vs):
        for k, x in v["seed"].items():
            tabs[i, int(k)] = x
    items = [bytes.fromhex(v["src_hex"]) for v in vs]
    for i, v in enumerate(vs):
        r, o, t = sg.run_continue(zl, [items[i]], [_bound(100)], tabs[i:i + 1], None, gpu, accel=v["acceleration"])
        final = np.zeros(4096, np.uint32)
        for k, x in v["final"].items():
            final[int(k)] = x
        assert r[0] == v["result"] and o[0].hex() == v["out_hex"] and np.array_equal(t[0], final), v["name"]


def test_statuses_leave_the_table(zl, gpu, cref, text):
    rng = np.random.default_rng(3)
    items, caps = [], []
    for i in range(60):
        k = i % 6
        b = text[i * 3000: i * 3000 + 6000]
        full = len(cref.cont(np.zeros(4096, np.uint32), b)[1])
        if k == 0: caps.append(full - int(rng.integers(1, 50)))          # OutputTooSmall
        elif k == 1: b = text[i: i + 7000]; caps.append(_bound(7000))   # longer than max_in_len: InvalidState
        elif k == 2: b = b""; caps.append(16)
        elif k == 3: b = b[:1 + i % 12]; caps.append(_bound(12))        # compressAsLiterals
        elif k == 4: b = b[:1 + i % 12]; caps.append(1 + i % 12)         # ... OutputTooSmall
        else: caps.append(full)                                          # exact fit
        items.append(b)
    tabs = rng.integers(0, 6000, (60, 4096)).astype(np.uint32)
    got = sg.run_continue(zl, items, caps, tabs, None, gpu, max_in=6000)
    want = cref.batch(tabs, None, items, caps, 1)
    for i in range(60):
        if i % 6 == 1:
            assert got[0][i] == -5 and np.array_equal(got[2][i], tabs[i]), i
            continue
        assert got[0][i] == want[0][i] and got[1][i] == want[1][i] and np.array_equal(got[2][i], want[2][i]), i
        if want[0][i] < 0 or len(items[i]) < 13:
            assert np.array_equal(got[2][i], tabs[i]), i
    assert sum(1 for r in got[0] if r == -1) >= 20
    # InputTooLarge needs a > 2 GiB block: the single-buffer call decides it on the host, the kernel does the same
    s = zl.Stream()
    s.hashTable[:] = 77
    with pytest.raises(zl.Lz4Error):
        s.compressFastContinue(b"x" * 20, 1, 3)
    assert (s.hashTable == 77).all() and s.currentOffset == 0


def test_single_buffer_stream_flow(zl, gpu, text):
    s = zl.createStream()
    d = text[5000:5000 + 80000]
    assert s.loadDict(d) == 65536 and s.dictSize == 65536 and s.dictionary == d[-65536:]
    pt, _ = zs.load_dict(d)
    assert list(s.hashTable) == pt
    total = 0
    for k, n in enumerate((30000, 7, 70000)):
        b = text[200000 + total: 200000 + total + n]
        total += n
        r, o, pt = zs.compress_fast_continue(pt, b, 1 + k)
        assert s.compressFastContinue(b, 1 + k) == o
        assert list(s.hashTable) == pt, k
        assert zl.decompressSafe(o, n) == b
    assert s.currentOffset == 100000                                  # the 7-byte block does not count (:825-827)
    buf = bytearray(100)
    assert s.saveDict(buf, 1000) == 100 and bytes(buf) == d[-100:]
    assert s.loadDict(b"") == 0 and not s.hashTable.any() and s.dictionary is None
    zl.freeStream(s)


def test_batch_continue_in_a_captured_graph(zl, gpu, cref, text):
    import torch
    n = 256
    items = [text[i * 4096: (i + 1) * 4096] for i in range(n)]
    caps = [_bound(4096)] * n
    _, dtab = sg.run_load_dict(zl, [text[-65536:]], gpu)
    buf, offs, lens = sg.pack(items)
    d_in = torch.from_numpy(buf).to(gpu)
    t_off = torch.from_numpy(offs).to(gpu)
    t_len = torch.from_numpy(lens.astype(np.int32)).to(gpu)
    out_off = torch.from_numpy((np.arange(n) * 4352).astype(np.int64)).to(gpu)
    out_cap = torch.full((n,), caps[0], dtype=torch.int32, device=gpu)
    d_out = torch.zeros(n * 4352, dtype=torch.uint8, device=gpu)
    tin = torch.from_numpy(dtab.reshape(-1).view(np.int32)).to(gpu)
    idx = torch.zeros(n, dtype=torch.int32, device=gpu)
    tout = torch.zeros(n * 4096, dtype=torch.int32, device=gpu)
    res = torch.zeros(n, dtype=torch.int64, device=gpu)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        zl.batch_compress_fast_continue(d_in, t_off, t_len, d_out, out_off, out_cap, tin, idx, tout, res, 4096, 1)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        zl.batch_compress_fast_continue(d_in, t_off, t_len, d_out, out_off, out_cap, tin, idx, tout, res, 4096, 1)
    res.fill_(-999)
    tout.fill_(0)
    g.replay()
    torch.cuda.synchronize()
    want = cref.batch(dtab, np.zeros(n, np.uint32), items, caps, 1)
    r = res.cpu().numpy()
    o = d_out.cpu().numpy()
    t = tout.cpu().numpy().view(np.uint32).reshape(n, 4096)
    for i in range(n):
        assert r[i] == want[0][i] and bytes(o[i * 4352: i * 4352 + r[i]]) == want[1][i] and np.array_equal(t[i], want[2][i])


# ------------------------------------------------------------------ seeds that must change the output
def _planted_batch(n, offs, seed0):
    items, tabs = [], []
    for k in range(12):
        off = offs[k % len(offs)]
        b, v, G = sg.planted(n - (k % 5), seed0 + k, r_off=off)
        t = np.zeros(4096, np.uint32)
        t[sg.hash4(G)] = v
        if k % 3 == 1:      # plus noise the block cannot use: every other slot at or above L
            noise = np.random.default_rng(seed0 + k).integers(len(b) - 12, 1 << 32, 4096).astype(np.uint32)
            noise[sg.hash4(G)] = v
            t = noise
        items.append(b)
        tabs.append(t)
    return items, np.stack(tabs)


@pytest.mark.parametrize("accel", [1, 64])
@pytest.mark.parametrize("n", [1024, 5000, 65547, 70000, 262144])
def test_planted_seeds_change_the_output(zl, gpu, cref, n, accel):
    """Blocks built so that a seed MUST produce a match (streamgen.planted): the window path (acceleration 1, probe
    20 or 63 lanes after an anchor, blocks > 192 bytes), the generic path (probe 100 positions on, or acceleration 64),
    the u16 table (<= 65 547 bytes) and the tagged u32 table (larger blocks).  The GPU must equal the restatement, and
    the restatement must differ from the zero-table output."""
    # (acceleration 64 probes E + 1, then E + 65, E + 66, ...: the seed's probe must lie on that schedule)
    items, tabs = _planted_batch(n, (20, 63, 100) if accel == 1 else (65, 100), 7000 + n + accel)
    caps = [_bound(len(b)) for b in items]
    got = sg.run_continue(zl, items, caps, tabs, None, gpu, accel=accel, max_in=n)
    want = cref.batch(tabs, None, items, caps, accel)
    _cmp(got, want, "planted")
    zero = cref.batch(np.zeros_like(tabs), None, items, caps, accel)
    same = [i for i in range(len(items)) if zero[1][i] == want[1][i]]
    assert not same, "a planted seed did not change blocks %s" % same
    dec = gh.decompress(zl, got[1], [len(b) for b in items], gpu)
    assert all(d == b for (_, d), b in zip(dec, items))
    # the single-buffer path on the first block
    s = zl.Stream()
    s.hashTable[:] = tabs[0]
    assert s.compressFastContinue(items[0], accel) == want[1][0] and np.array_equal(s.hashTable, want[2][0])


def test_chained_seeds_above_64k_pass_a_64k_step_and_are_used(zl, gpu, cref):
    """256 KiB, then 64 KiB, then 256 KiB steps of 16 streams, in place (streamgen.chained_planted): step 1 leaves a
    position v >= 65 536 in the table, the 64 KiB step (16-bit table) cannot load it and must pass it through, and
    step 3 must match it.  Step 3 must differ from the same step with every entry >= 65 536 dropped."""
    nstreams = 16
    streams = [sg.chained_planted(100000 + 4099 * s, 50 + s) for s in range(nstreams)]
    tables = np.zeros((nstreams, 4096), np.uint32)
    ctabs = tables.copy()
    for step in range(3):
        items = [st[step] for st in streams]
        caps = [_bound(len(b)) for b in items]
        size = max(len(b) for b in items)
        want = cref.batch(ctabs, None, items, caps, 1)
        got = sg.run_continue(zl, items, caps, tables, None, gpu, max_in=size, in_place=True)
        _cmp(got, want, "step %d" % step)
        if step == 1:
            for s in range(nstreams):
                v = 100000 + 4099 * s
                assert got[2][s][sg.hash4(streams[s][2][v:v + 4])] == v, "seed %d did not pass the 64 KiB step" % v
        if step == 2:
            dropped = cref.batch(np.where(ctabs >= 65536, 0, ctabs).astype(np.uint32), None, items, caps, 1)
            same = [s for s in range(nstreams) if dropped[1][s] == want[1][s]]
            assert not same, "step 3 did not use the seeds >= 65536 of streams %s" % same
            dec = gh.decompress(zl, got[1], [len(b) for b in items], gpu)
            assert all(d == b for (_, d), b in zip(dec, items))
        tables, ctabs = got[2], want[2]
