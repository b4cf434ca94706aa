"""Results must depend on the bytes of [in_off, in_off + in_len) only.  batch_compress_hc, batch_decompress_safe and
batch_decompress_safe_using_dict over blocks packed back to back at unaligned offsets, the input tensor ending where the
last block ends, output slots at odd offsets with odd capacities (gpu_harness.Packed).  Every batch runs twice: the gaps
hold zeros, then bytes that continue the block before them.  Both runs must equal each other and the oracle, byte for
byte and status for status.  The decoders run below and from kLaneCopyMinBlocks (6144) blocks, the two builds the
launcher picks."""
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

GENS = (dg.text_bytes, dg.reptext_bytes, dg.mixed_bytes, dg.zero_bytes, dg.random_bytes, dg.ramp_bytes)


def _odd(n):
    return n | 1


def _periodic(n, period, seed):
    unit = bytes(dg.random_bytes(period, seed))
    return (unit * (n // period + 1))[:n]


def _plain_blocks(count, seed, max_len):
    """odd-sized blocks of every distribution, periodic ones (their continuation extends the last match) and tiny ones"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        k = i % 8
        if k == 6:
            n = _odd(int(rng.integers(13, max_len)))
            out.append(_periodic(n, int(rng.integers(1, 70)), seed + i))
        elif k == 7:
            out.append(bytes(dg.text_bytes(int(rng.integers(1, 40)), seed + i)))
        else:
            out.append(bytes(GENS[k](_odd(int(rng.integers(13, max_len))), seed + i)))
    return out


def _both_fills(run, want, names, seed):
    got = {}
    for fill in ("zero", "cont"):
        got[fill] = run(gh.Packed(seed, fill))
        bad = []
        for name, (n, data), w in zip(names, got[fill], want):
            wn, wd = (w, b"") if isinstance(w, int) else (len(w), w)
            if n != wn or data != wd:
                bad.append("%s: %d vs %d%s" % (name, n, wn, " (bytes differ)" if n == wn else ""))
        assert not bad, "gaps %s: %d/%d blocks differ from the oracle: %s" % (fill, len(bad), len(names), "; ".join(bad[:8]))
    assert got["zero"] == got["cont"]


@pytest.mark.parametrize("wide", [False, True], ids=["le64k", "gt64k"])
@pytest.mark.parametrize("level", [2, 9, 12])
def test_compress_hc_packed(zl, oracle, gpu, level, wide):
    items = _plain_blocks(150, 40 + level, 65536)
    items.append(bytes(dg.text_bytes(65536 if not wide else 70001, 41)))
    items.append(_periodic(65535, 7, 42))                # the last block: ends at the last byte of the input tensor
    caps = []
    for i, b in enumerate(items):
        w = len(oracle.compress_hc(b, level))
        caps.append(_odd(zl.compressBound(len(b))) if i % 5 else _odd(w - 2))   # a fifth just under the bound size
    names = ["blk%d/n%d/cap%d" % (i, len(b), c) for i, (b, c) in enumerate(zip(items, caps))]
    want = [oracle.compress_hc_expected(b, level, c) for b, c in zip(items, caps)]
    assert sum(not isinstance(w, int) for w in want) > 100
    _both_fills(lambda lay: gh.compress_hc(zl, items, gpu, level, caps=caps, layout=lay), want, names, level)


def _streams(oracle, count, seed):
    """compressed blocks (compressDefault, compressFast(3), compressHC(9)) with odd capacities; every sixth one is
    truncated, every seventh given a capacity just short of its size"""
    rng = np.random.default_rng(seed)
    comp, caps, want, names = [], [], [], []
    for i, b in enumerate(_plain_blocks(count, seed, 20000)):
        c = (oracle.compress_default(b), oracle.compress_fast(b, 3), oracle.compress_hc(b, 9))[i % 3]
        cap, what = _odd(len(b)), "ok"
        if i % 6 == 5 and len(c) > 2:
            c = c[:int(rng.integers(1, len(c)))]
            what = "trunc"
        elif i % 7 == 3 and len(b) > 3:
            cap = _odd(len(b) - int(rng.integers(2, min(len(b), 40))))
            what = "short"
        comp.append(c); caps.append(cap); names.append("%d/n%d/%s" % (i, len(b), what))
        want.append(oracle.decompress_safe(c, cap))
    return comp, caps, want, names


@pytest.mark.parametrize("nblocks", [500, 6200])
def test_decompress_safe_packed(zl, oracle, gpu, nblocks):
    comp, caps, want, names = _streams(oracle, 400, 7)
    idx = [i % len(comp) for i in range(nblocks)]
    comp, caps, want = [comp[k] for k in idx], [caps[k] for k in idx], [want[k] for k in idx]
    names = ["blk%d/%s" % (i, names[k]) for i, k in enumerate(idx)]
    assert sum(isinstance(w, int) for w in want) > nblocks // 10
    _both_fills(lambda lay: gh.decompress(zl, comp, caps, gpu, layout=lay), want, names, nblocks)


@pytest.fixture(scope="module")
def enc(tmp_path_factory):
    return dictgen.encoder(tmp_path_factory.mktemp("dictenc"))


@pytest.mark.parametrize("nblocks", [500, 6200])
def test_decompress_safe_using_dict_packed(zl, gpu, enc, nblocks):
    """records encoded against dictionaries of 0 .. 70 001 bytes (packed the same way as the streams); a fifth of the
    streams truncated or given a short capacity"""
    text = bytes(dg.text_bytes(4 << 20, 4712))
    rng = np.random.default_rng(nblocks)
    dicts = [b"", text[:1001], text[5000:5000 + 65536], text[80000:150001]]
    uniq, ucaps, uidx, unames = [], [], [], []
    for i in range(300):
        k = i % len(dicts)
        n = _odd(int(rng.integers(1, 9000)))
        start = 200000 + 9000 * i
        rec = text[start:start + n]
        s, _ = enc(dicts[k], rec)
        cap, what = n, "ok"
        if i % 10 == 3 and len(s) > 2:
            s = s[:int(rng.integers(1, len(s)))]
            what = "trunc"
        elif i % 10 == 7 and n > 40:
            cap = n - 2 * int(rng.integers(1, 20))
            what = "short"
        uniq.append(s); ucaps.append(cap); uidx.append(k); unames.append("d%d/n%d/%s" % (len(dicts[k]), n, what))
    uwant = [pd.decompress_safe_using_dict(s, c, dicts[k]) for s, c, k in zip(uniq, ucaps, uidx)]
    sel = [i % len(uniq) for i in range(nblocks)]
    items, caps, dix = [uniq[j] for j in sel], [ucaps[j] for j in sel], [uidx[j] for j in sel]
    want = [uwant[j][0] if uwant[j][0] < 0 else uwant[j][1] for j in sel]
    names = ["blk%d/%s" % (i, unames[j]) for i, j in enumerate(sel)]
    assert sum(isinstance(w, int) for w in want) > nblocks // 20
    _both_fills(lambda lay: dictgen.run_batch(zl, items, caps, dicts, dix, gpu, layout=lay), want, names, nblocks)
