"""zlz4_batch_compress_fast_using_dict / zlz4_compress_fast_using_dict on the GPU: byte and status equality with the C
restatement tests/dict_compress_ref.c (never with the code under test), guard bands around every slot, arenas unchanged."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "pyref"))
import datagen as dg  # noqa: E402
import dictcgen as dc  # noqa: E402
import gpu_harness as gh  # noqa: E402

pytestmark = pytest.mark.gpu

DICT_LENS = (0, 1, 3, 4, 5, 100, 65535, 65536, 65537, 200000)
REC_LENS = (0, 1, 12, 13, 14, 37, 4096, 65536, 65548, 200000)
U16_MAX = 65536 + 11                                  # max_dict_len + max_in_len up to which the table is 16 bits wide


@pytest.fixture(scope="module")
def cref(tmp_path_factory):
    return dc.ref(tmp_path_factory.mktemp("dictcref"))


@pytest.fixture(scope="module")
def text():
    """400 000 bytes of D-text: a dictionary is the bytes in front of position 200 000, a record the bytes after it"""
    return bytes(dg.text_bytes(400000, 77))


def _pair(text, dl, n, k=0):
    cut = 200000 - 37 * k
    return text[cut - dl:cut], text[cut:cut + n]


def _tail(d):
    return min(len(d), 65536)


# ------------------------------------------------------------------ lengths, both table widths
def _groups():
    """the (dict, record) length grid split into launches: three whose positions fit the 16-bit table, one that needs 32"""
    g = [[], [], [], []]
    for dl in DICT_LENS:
        for n in REC_LENS:
            D = min(dl, 65536)
            k = 0 if (D <= 5 and n <= 65536) else 1 if (D <= 100 and n <= 4096) else 2 if (D <= 65535 and n <= 12) else 3
            g[k].append((dl, n))
    return g


@pytest.mark.parametrize("accel", [1, 8, 65537])
def test_length_grid_both_table_widths(zl, gpu, cref, text, accel):
    groups = _groups()
    assert sum(len(g) for g in groups) == len(DICT_LENS) * len(REC_LENS)
    for k, g in enumerate(groups):
        width = max(min(dl, 65536) for dl, _ in g) + max(n for _, n in g)
        assert (width <= U16_MAX) == (k < 3)
        dicts = [_pair(text, dl, 0)[0] for dl in DICT_LENS]
        recs = [_pair(text, dl, n)[1] for dl, n in g]
        idx = [DICT_LENS.index(dl) for dl, _ in g]
        got, want = dc.run_batch(zl, cref, recs, [dc.bound(len(r)) for r in recs], dicts, idx, gpu, accel=accel)
        dc.check(got, want, "group %d" % k)
        if accel == 1 and k == 3:                     # the dictionary is used at all
            plain = cref.compress(recs[-1], b"")[0]
            assert 0 < want[-1][0] < plain


# ------------------------------------------------------------------ capacities
def test_capacities(zl, gpu, cref, text):
    pairs = [_pair(text, dl, n, k) for k, (dl, n) in enumerate(((0, 13), (100, 37), (65536, 4096), (70000, 1000), (5, 12),
                                                                 (4096, 65536), (65536, 200000), (300, 1)))]
    sizes = [cref.compress(r, d)[0] for d, r in pairs]
    recs, dicts, caps = [], [], []
    for (d, r), s in zip(pairs, sizes):
        for c in (s, s - 1, 0, dc.bound(len(r)), s + 1, s // 2):
            recs.append(r); dicts.append(d); caps.append(max(c, 0))
    for accel in (1, 8):
        got, want = dc.run_batch(zl, cref, recs, caps, dicts, list(range(len(recs))), gpu, accel=accel, use_idx=False)
        dc.check(got, want)
        if accel == 1:
            for k, s in enumerate(sizes):
                assert want[6 * k][0] == s and want[6 * k + 1][0] == dc.OUTPUT_TOO_SMALL and want[6 * k + 2][0] == dc.OUTPUT_TOO_SMALL
                assert want[6 * k + 3][0] == s <= dc.bound(len(pairs[k][1]))


# ------------------------------------------------------------------ crafted records
def test_crafted_records(zl, gpu, cref):
    """dictcgen.crafted(): what each case is about is asserted on the restatement in tests/test_dict_compress_cpu.py"""
    cases = dc.crafted(cref)
    recs = [r for _, _, r in cases]
    dicts = [d for _, d, _ in cases]
    for accel in (1, 8):
        got, want = dc.run_batch(zl, cref, recs, [dc.bound(len(r)) for r in recs], dicts, list(range(len(recs))), gpu,
                                 accel=accel, use_idx=False)
        for (name, _, _), g, w in zip(cases, got, want):
            assert g == w, name


# ------------------------------------------------------------------ dictionary placement, table indexing, layouts
def _records(text, n, size, start=100000):
    return [text[start + i * size: start + (i + 1) * size] for i in range(n)]


@pytest.mark.parametrize("use_idx", [True, False])
def test_shared_dictionary(zl, gpu, cref, text, use_idx):
    recs = _records(text, 48, 4096)
    d = text[100000 - 65536:100000]
    got, want = dc.run_batch(zl, cref, recs, [dc.bound(4096)] * 48, [d], [0] * 48, gpu, use_idx=use_idx)
    dc.check(got, want)
    assert sum(w for w, _ in want) < sum(cref.compress(r, b"")[0] for r in recs)


@pytest.mark.parametrize("layout", [None, gh.Packed(seed=3), gh.Packed(seed=4, fill="cont", gaps=(0, 2))])
def test_per_block_dictionaries_and_packed_layouts(zl, gpu, cref, text, layout):
    rng = np.random.default_rng(11)
    recs, dicts = [], []
    for k in range(40):
        dl = int(rng.choice([0, 3, 7, 64, 1000, 4097, 30000, 65536, 66000]))
        n = int(rng.choice([0, 5, 13, 100, 1001, 4096, 9000, 70001]))
        d, r = _pair(text, dl, n, k)
        dicts.append(d); recs.append(r)
    for use_idx in (True, False):
        got, want = dc.run_batch(zl, cref, recs, [dc.bound(len(r)) for r in recs], dicts, list(range(40)), gpu, layout=layout,
                                 use_idx=use_idx, accel=1 if use_idx else 3)
        dc.check(got, want)


@pytest.mark.parametrize("size", [1000, 4096, 40000])
def test_previous_record_as_dictionary_inside_the_input(zl, gpu, cref, text, size):
    """record k against record k - 1, the dictionaries lying in d_in itself: one load_dict over the records, one batch"""
    n = 9
    recs = _records(text, n, size, start=0)
    buf, offs, lens = gh._pack(recs)
    prev = [(0, 0)] + [(int(offs[k - 1]), int(lens[k - 1])) for k in range(1, n)]
    got, want = dc.run_batch(zl, cref, recs, [dc.bound(size)] * n, None, None, gpu, in_input=prev)
    dc.check(got, want)
    for k in range(n):
        assert want[k] == cref.compress(recs[k], recs[k - 1] if k else b"")


# ------------------------------------------------------------------ preconditions
def test_over_max_lengths_get_invalid_state(zl, gpu, cref, text):
    pairs = [_pair(text, 100, 1000), _pair(text, 100, 1001), _pair(text, 101, 1000), _pair(text, 70000, 20),
             _pair(text, 0, 0), _pair(text, 101, 0), _pair(text, 50, 999)]
    recs = [r for _, r in pairs]
    dicts = [d for d, _ in pairs]
    got, want = dc.run_batch(zl, cref, recs, [dc.bound(len(r)) for r in recs], dicts, list(range(len(recs))), gpu,
                             max_in=1000, max_dict=100)
    dc.check(got, want)
    assert [want[k][0] for k in (1, 2, 3, 5)] == [dc.INVALID_STATE] * 4
    assert want[0][0] > 0 and want[4][0] == 0 and want[6][0] > 0


def test_misaligned_or_null_arrays_launch_nothing(zl, gpu, text):
    import torch
    d, r = _pair(text, 1000, 1000)
    a = lambda b: torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).to(gpu)
    z64 = torch.zeros(1, dtype=torch.int64, device=gpu)
    i32 = lambda v: torch.tensor([v], dtype=torch.int32, device=gpu)
    tab = torch.zeros(4096 + 4, dtype=torch.int32, device=gpu)
    out = torch.full((2000,), 0xA5, dtype=torch.uint8, device=gpu)
    res = torch.full((1,), -999, dtype=torch.int64, device=gpu)
    args = [a(r), z64, i32(1000), out, z64, i32(2000), a(d), z64, i32(1000), tab, None, res, 1000, 1000, 1]
    for k, bad in ((9, tab[1:]), (9, tab[2:]), (9, None), (7, None), (8, None), (1, None), (11, None), (6, None),
                   (8, torch.zeros(8, dtype=torch.uint8, device=gpu)[1:5])):
        b = list(args)
        b[k] = bad
        with pytest.raises(zl.Lz4Error) as e:
            zl.batch_compress_fast_using_dict(*b)
        assert e.value.name == "InvalidState"
    torch.cuda.synchronize()
    assert int(res.item()) == -999 and bool((out == 0xA5).all())
    zl.batch_compress_fast_using_dict(*args)          # (the same arguments, aligned: runs)
    torch.cuda.synchronize()
    assert int(res.item()) > 0


# ------------------------------------------------------------------ the single host call
def test_single_call_equals_the_batch(zl, gpu, cref, text):
    for k, (dl, n, accel) in enumerate(((0, 0, 1), (100, 5, 1), (0, 13, 1), (3, 14, 1), (100, 37, 8), (65536, 4096, 1),
                                        (70000, 4096, 65537), (200000, 70000, 1), (65535, 12, 1), (4096, 65548, 8))):
        d, r = _pair(text, dl, n, k)
        want = cref.compress(r, d, accel)
        assert zl.compressFastUsingDict(r, d, accel) == want[1]
        assert len(want[1]) == want[0]
        if want[0] > 1:
            with pytest.raises(zl.Lz4Error) as e:
                zl.compressFastUsingDict(r, d, accel, dst_cap=want[0] - 1)
            assert e.value.name == "OutputTooSmall"
            assert zl.compressFastUsingDict(r, d, accel, dst_cap=want[0]) == want[1]
        if n:
            assert zl.decompressSafeUsingDict(want[1], n, d) == r
    assert zl.compressFastUsingDict(text[:3000], b"") == zl.compressFast(text[:3000], 1)


# ------------------------------------------------------------------ fuzz
def _fuzz_batch(seed, nrec, ndict):
    rng = np.random.default_rng(seed)
    gens = (dg.text_bytes, dg.reptext_bytes, dg.mixed_bytes, dg.random_bytes)
    dicts = []
    for k in range(ndict):
        dl = int(rng.choice([0, int(rng.integers(1, 16)), int(rng.integers(16, 3000)), int(rng.integers(3000, 70000))],
                            p=[0.05, 0.15, 0.6, 0.2]))
        dicts.append(bytes(gens[int(rng.integers(0, 4))](dl, int(rng.integers(0, 1 << 30)))))
    recs, idx = [], []
    for k in range(nrec):
        di = int(rng.integers(0, ndict))
        d = dicts[di]
        n = int(rng.choice([int(rng.integers(0, 30)), int(rng.integers(30, 2000)), int(rng.integers(2000, 9000))], p=[0.2, 0.6, 0.2]))
        fresh = bytes(gens[int(rng.integers(0, 4))](n + 8, int(rng.integers(0, 1 << 30))))
        parts, left = [], n
        while left > 0:                               # pieces of the dictionary (its end above all) between fresh bytes
            take = min(left, int(rng.integers(1, 200)))
            if len(d) > 4 and rng.random() < 0.5:
                if rng.random() < 0.3:
                    s = max(0, len(d) - int(rng.integers(1, 40)))
                else:
                    s = int(rng.integers(0, len(d)))
                p = d[s:s + take] or b"\0"
            else:
                s = int(rng.integers(0, 8))
                p = fresh[s:s + take] or b"\0"
            parts.append(p)
            left -= len(p)
        recs.append(b"".join(parts)[:n])
        idx.append(di)
    return recs, dicts, idx


@pytest.mark.parametrize("seed,accel", [(1, 1), (2, 1), (3, 2), (4, 65), (5, 1)])
def test_fuzz_sweep(zl, gpu, cref, seed, accel):
    recs, dicts, idx = _fuzz_batch(1000 + seed, 700, 60)
    caps = [dc.bound(len(r)) for r in recs]
    if seed == 5:                                     # tight slots: OutputTooSmall at many points
        rng = np.random.default_rng(5)
        caps = [int(rng.integers(0, c + 1)) for c in caps]
    got, want = dc.run_batch(zl, cref, recs, caps, dicts, idx, gpu, accel=accel, use_idx=seed % 2 == 1)
    dc.check(got, want)


def test_foreign_tables_still_decode_and_equal_the_restatement(zl, gpu, cref):
    """tables that do not belong to the dictionaries (random u32; positions around the dictionary's end, whose 4-byte
    compare straddles it): the same bytes as the restatement run with the same table, and every stream decodes"""
    recs, dicts, idx = _fuzz_batch(77, 300, 30)
    rng = np.random.default_rng(78)
    tabs = np.empty((30, 4096), np.uint32)
    for k, d in enumerate(dicts):
        D = _tail(d)
        kind = k % 3
        if kind == 0:
            tabs[k] = rng.integers(0, 1 << 32, 4096, dtype=np.uint64).astype(np.uint32)
        elif kind == 1:
            tabs[k] = rng.integers(0, D + 3000, 4096)
        else:
            tabs[k] = np.clip(D - rng.integers(-4, 6, 4096), 0, None)
    got, want = dc.run_batch(zl, cref, recs, [dc.bound(len(r)) for r in recs], dicts, idx, gpu, tables=tabs)
    dc.check(got, want)
    assert zl.decompressBlocks([gb for _, gb in got], [dicts[k] for k in idx], device=gpu) == recs


# ------------------------------------------------------------------ end to end, graph capture
def test_round_trip_through_the_convenience_calls(zl, gpu, text):
    n, size = 8192, 300
    d = text[300000:304096]
    pool = text[300000 - 40000:300000] + text[304096:304096 + 40000]
    recs = [pool[(37 * i) % (len(pool) - size):][:size - i % 7] for i in range(n)]
    streams = zl.compressBlocksUsingDict(recs, [d], dict_index=[0] * n, device=gpu)
    assert all(isinstance(s, bytes) for s in streams)
    assert sum(map(len, streams)) < sum(map(len, zl.compressBlocksUsingDict(recs[:64], [b""], [0] * 64, device=gpu))) * (n // 64)
    back = zl.decompressBlocks(streams, [d] * n, device=gpu)
    assert back == recs
    # per-block dictionaries (dict_index None)
    s2 = zl.compressBlocksUsingDict(recs[1:40], recs[0:39], device=gpu)
    assert zl.decompressBlocks(s2, recs[0:39], device=gpu) == recs[1:40]


def test_batch_in_a_captured_graph(zl, gpu, cref, text):
    import torch
    n = 256
    recs = _records(text, n, 4096)
    d = text[100000 - 65536:100000]
    buf, offs, lens = gh._pack(recs)
    dbuf = np.frombuffer(d, dtype=np.uint8).copy()
    d_in = torch.from_numpy(buf).to(gpu)
    d_dict = torch.from_numpy(dbuf).to(gpu)
    t_off = torch.from_numpy(offs).to(gpu)
    t_len = torch.from_numpy(lens.astype(np.int32)).to(gpu)
    cap = dc.bound(4096)
    out_off = torch.from_numpy((np.arange(n) * 4352).astype(np.int64)).to(gpu)
    out_cap = torch.full((n,), cap, dtype=torch.int32, device=gpu)
    d_out = torch.zeros(n * 4352, dtype=torch.uint8, device=gpu)
    doff = torch.zeros(n, dtype=torch.int64, device=gpu)
    dlen = torch.full((n,), 65536, dtype=torch.int32, device=gpu)
    tab = torch.zeros(4096, dtype=torch.int32, device=gpu)
    lres = torch.zeros(1, dtype=torch.int64, device=gpu)
    idx = torch.zeros(n, dtype=torch.int32, device=gpu)
    res = torch.zeros(n, dtype=torch.int64, device=gpu)

    def both():
        zl.batch_load_dict(d_dict, doff[:1], dlen[:1], tab, lres)
        zl.batch_compress_fast_using_dict(d_in, t_off, t_len, d_out, out_off, out_cap, d_dict, doff, dlen, tab, idx, res,
                                          4096, 65536, 1)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        both()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        both()
    res.fill_(-999)
    tab.fill_(0)
    d_out.fill_(0)
    g.replay()
    torch.cuda.synchronize()
    r = res.cpu().numpy()
    o = d_out.cpu().numpy()
    for i in range(n):
        w, wb = cref.compress(recs[i], d)
        assert r[i] == w and bytes(o[i * 4352: i * 4352 + w]) == wb
