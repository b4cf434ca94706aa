"""Dictionary decoding on the GPU (zlz4_decompress_safe[_partial]_using_dict, zlz4_batch_decompress_safe_using_dict;
reference src/lz4.zig:960-969): bytes and statuses against the Python restatement (tools/pyref/zig_lz4_dict.py) or
the known plaintext, for both decoder builds (below / from 6144 blocks per batch)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "pyref"))
import datagen as dg  # noqa: E402
import dictgen  # noqa: E402
import gpu_harness as gh  # noqa: E402
import zig_lz4_dict as pd  # noqa: E402

pytestmark = pytest.mark.gpu


def _call(fn, *args):
    import zig_lz4_amd as zl
    try:
        out = fn(*args)
        return len(out), out
    except zl.Lz4Error as e:
        return e.code, b""


def _cmp(names, got, want):
    bad = []
    for name, (n, d), (wn, wd) in zip(names, got, want):
        if n != wn or (wn > 0 and d != wd):
            bad.append("%s: GPU %d vs %d%s" % (name, n, wn, " (bytes differ)" if n == wn else ""))
    assert not bad, "%d blocks differ:\n%s" % (len(bad), "\n".join(bad[:20]))


def test_crafted_single_calls(zl, gpu):
    names, got, want = [], [], []
    for name, s, dct, cap, target in dictgen.crafted_cases():
        keep = bytes(dct)
        if target is None:
            got.append(_call(zl.decompressSafeUsingDict, s, cap, dct))
            want.append(pd.decompress_safe_using_dict(s, cap, dct))
        else:
            got.append(_call(zl.decompressSafePartialUsingDict, s, cap, target, dct))
            want.append(pd.decompress_safe_partial_using_dict(s, cap, target, dct))
        assert dct == keep
        names.append(name)
    _cmp(names, got, want)
    assert len(names) > 100


@pytest.mark.parametrize("nblocks", [300, 7000])
def test_crafted_batch(zl, gpu, nblocks):
    cases = [c for c in dictgen.crafted_cases() if c[4] is None]
    dicts = []
    for c in cases:
        if not any(d is c[2] for d in dicts):
            dicts.append(c[2])
    items, caps, idx, names = [], [], [], []
    for i in range(nblocks):
        name, s, dct, cap, _ = cases[i % len(cases)]
        items.append(s); caps.append(cap); names.append("%d/%s" % (i, name))
        idx.append(next(k for k, d in enumerate(dicts) if d is dct))
    got = dictgen.run_batch(zl, items, caps, dicts, idx, gpu)
    want = [pd.decompress_safe_using_dict(s, cap, dicts[k]) for s, cap, k in zip(items, caps, idx)]
    _cmp(names, got, want)


def _malformed_batch(oracle, nblocks, seed):
    rng = np.random.default_rng(seed)
    names, comp, caps = [], [], []
    for i in range(nblocks):
        n = int(rng.integers(600, 6000))
        b = bytes((dg.text_bytes, dg.reptext_bytes, dg.mixed_bytes)[i % 3](n, 3000 + i))
        c = (oracle.compress_default(b), oracle.compress_fast(b, 5), oracle.compress_hc(b, 6))[(i // 3) % 3]
        cap, what = n, "ok"
        if i % 9 == 4:
            m = bytearray(c)
            pos = int(rng.integers(0, len(m)))
            k = (i // 9) % 4
            if k == 0: m[pos] ^= 1 << int(rng.integers(0, 8))
            elif k == 1: m[pos] = int(rng.integers(0, 256))
            elif k == 2: m[pos:pos + 2] = b"\x00\x00"
            else: m[pos:pos + 4] = b"\xff\xff\xff\xff"
            c, what = bytes(m), "corrupt%d@%d" % (k, pos)
        elif i % 9 == 7:
            cut = int(rng.integers(1, len(c)))
            c, what = c[:cut], "trunc%d" % cut
        elif i % 9 == 2:
            cap = max(0, n + int(rng.choice([-1, -4, -17, -31, -32, -33, -100, 1, 31, 32, -n // 2])))
            what = "cap%d" % cap
        names.append("blk%d/n%d/%s" % (i, n, what)); comp.append(c); caps.append(cap)
    return names, comp, caps


@pytest.mark.parametrize("nblocks", [2000, 7000])
def test_empty_dict_equals_batch_decompress_safe(zl, oracle, gpu, nblocks):
    """an empty dictionary behaves exactly like decompressSafe, every status included (src/lz4.zig:183 vs :190)"""
    names, comp, caps = _malformed_batch(oracle, nblocks, 77 + nblocks)
    ref = gh.decompress(zl, comp, caps, gpu)
    got = dictgen.run_batch(zl, comp, caps, [b""], [0] * nblocks, gpu)
    _cmp(names, got, ref)
    want = [oracle.decompress_safe(c, cap) for c, cap in zip(comp, caps)]
    _cmp(names, got, [(w, b"") if isinstance(w, int) else (len(w), w) for w in want])
    nerr = sum(isinstance(w, int) for w in want)
    assert nerr > nblocks // 10


@pytest.fixture(scope="module")
def enc(tmp_path_factory):
    return dictgen.encoder(tmp_path_factory.mktemp("dictenc"))


@pytest.fixture(scope="module")
def text():
    return bytes(dg.text_bytes(40 << 20, 4711))


@pytest.mark.parametrize("nblocks", [4096, 8192])
def test_shared_dictionary_records(zl, gpu, enc, text, nblocks):
    dct = text[:65536]
    recs = [text[65536 + 4096 * i: 65536 + 4096 * (i + 1)] for i in range(nblocks)]
    streams, st = [], [0, 0, 0, 0]
    for r in recs:
        s, t = enc(dct, r)
        streams.append(s)
        st = [a + b for a, b in zip(st, t)]
    assert st[2] > nblocks and st[3] > 0, st
    got = dictgen.run_batch(zl, streams, [4096] * nblocks, [dct], [0] * nblocks, gpu)
    _cmp(["rec%d" % i for i in range(nblocks)], got, [(4096, r) for r in recs])


@pytest.mark.parametrize("nblocks", [1024, 8192])
def test_per_block_dictionaries(zl, gpu, enc, text, nblocks):
    """dictionary of record i = the plaintext of record i - 1 (record 0: none)"""
    base = 1 << 20
    recs = [text[base + 4096 * i: base + 4096 * (i + 1)] for i in range(nblocks + 1)]
    streams = [enc(recs[i], recs[i + 1])[0] for i in range(nblocks)]
    dicts = recs[:nblocks]
    got = dictgen.run_batch(zl, streams, [4096] * nblocks, dicts, list(range(nblocks)), gpu)
    _cmp(["rec%d" % i for i in range(nblocks)], got, [(4096, recs[i + 1]) for i in range(nblocks)])


@pytest.mark.parametrize("nblocks", [48, 6200])
def test_big_blocks_with_long_dictionary(zl, gpu, enc, text, nblocks):
    """64 KiB blocks whose dictionary is longer than 64 KiB (only its last 64 KiB can be referenced)"""
    dlen = 100000
    items, dicts, plain = [], [], []
    ndict = min(nblocks, 48)
    for i in range(ndict):
        dicts.append(text[i * 65536: i * 65536 + dlen])
    for i in range(nblocks):
        k = i % ndict
        blk = text[k * 65536 + dlen: k * 65536 + dlen + 65536]
        plain.append(blk)
        if i < ndict:
            items.append(enc(dicts[k], blk)[0])
        else:
            items.append(items[k])
    got = dictgen.run_batch(zl, items, [65536] * nblocks, dicts, [i % ndict for i in range(nblocks)], gpu)
    _cmp(["blk%d" % i for i in range(nblocks)], got, [(65536, p) for p in plain])


def test_malformed_dict_streams_large_batch(zl, gpu, enc, text):
    """flipped offsets, damaged bytes, truncations and short capacities of dictionary streams, 6400 blocks in one call"""
    rng = np.random.default_rng(99)
    nblocks = 6400
    dct = text[(8 << 20): (8 << 20) + 65536]
    items, caps, names, want = [], [], [], []
    for i in range(nblocks):
        r = text[(9 << 20) + 4096 * i: (9 << 20) + 4096 * (i + 1)]
        s, _ = enc(dct, r)
        m, cap, what = bytearray(s), 4096, "ok"
        k = i % 5
        if k == 1:   # flip a bit of an offset's high byte: reaches into (or beyond) the dictionary
            pos = int(rng.integers(0, len(m)))
            m[pos] ^= 1 << int(rng.integers(0, 8))
            what = "flip@%d" % pos
        elif k == 2:
            m = m[:int(rng.integers(1, len(m)))]
            what = "trunc%d" % len(m)
        elif k == 3:
            cap = 4096 - int(rng.integers(1, 200))
            what = "cap%d" % cap
        items.append(bytes(m)); caps.append(cap); names.append("blk%d/%s" % (i, what))
        want.append(pd.decompress_safe_using_dict(bytes(m), cap, dct))
    nerr = sum(w[0] < 0 for w in want)
    assert nerr > nblocks // 5, nerr
    got = dictgen.run_batch(zl, items, caps, [dct], [0] * nblocks, gpu)
    _cmp(names, got, want)
