"""The window epilogue of k_compress_fast and of the dictionary compressor's copy of it (one covered mask accumulated by
the flushes and immediate emissions, one table write per lane): bytes, sizes and statuses against the oracle / the C
restatements on inputs that put the epilogue to work -- duplicate-hash groups with covered and uncovered members, matches
that end before, at and past lane 64, immediate emission followed by a run in one window, more than one flush per
window, the `tight` path near the end of the destination -- in the plain, the seeded (compressFastContinue) and the
dictionary (compressFastUsingDict) builds, 16- and 32-bit tables."""
import numpy as np
import pytest

import datagen as dg
import dictcgen as dc
import gpu_harness as gh
import streamgen as sg

pytestmark = pytest.mark.gpu

PERIODS = (1, 2, 3, 5, 8, 13, 37, 63, 64, 65)
SIZES = (300, 333, 511, 1000, 2065, 4096, 8192)
# destination capacity = the oracle's size + this (the window path is `tight` with < 512 bytes left); -1: OutputTooSmall
CAP_EXTRA = (-1, 0, 1, 7, 100, 300, 511, 512, 600)


def periodic(n, period, seed):
    """`period`-periodic bytes broken by one to three random literals every 20 to 90 bytes"""
    rng = np.random.default_rng(seed)
    unit = rng.integers(0, 256, period, dtype=np.uint8)
    b = np.tile(unit, n // period + 1)[:n].copy()
    p = int(rng.integers(20, 91))
    while p < n:
        k = int(rng.integers(1, 4))
        b[p:p + k] = rng.integers(0, 256, len(b[p:p + k]), dtype=np.uint8)
        p += int(rng.integers(20, 91))
    return b.tobytes()


def long_match(n, start, mlen, seed):
    """text whose bytes [start, start + mlen) repeat the bytes at [100, 100 + mlen): short sequences, then one match of
    about mlen >= 274 bytes that begins inside a window (emitted immediately, after a flush of the pending run), then
    short sequences again"""
    t = bytes(dg.text_bytes(n, seed))
    return (t[:start] + t[100:100 + mlen] + t[start:])[:n]


def _inputs():
    items, names = [], []
    for i, p in enumerate(PERIODS):                                     # (i)
        for k in range(3):
            n = SIZES[(3 * i + k) % len(SIZES)]
            items.append(periodic(n, p, 100 * p + k)); names.append("periodic%d/%d" % (p, n))
    items.append(periodic(65536, 37, 7)); names.append("periodic37/65536")
    for k, (start, mlen) in enumerate(((400, 320), (421, 330), (450, 335), (463, 529), (500, 1000), (517, 325), (535, 340),
                                       (600, 274 + 255))):            # (ii)
        n = (1500, 3000, 8000)[k % 3]
        items.append(long_match(n, start, mlen, 50 + k)); names.append("longmatch/%d+%d/%d" % (start, mlen, n))
    for k in range(3):                                                  # (iii)
        items.append(bytes(dg.text_bytes(4096, 900 + k))); names.append("text/4096/%d" % k)
        items.append(bytes(dg.reptext_bytes(4096, 900 + k))); names.append("reptext/4096/%d" % k)
    return items, names


def _big():
    return [bytes(dg.text_bytes(65548, 31)), periodic(100000, 13, 5) + long_match(104800, 450, 335, 9)], ["text/65548", "mix/204800"]


@pytest.fixture(scope="module")
def inputs(oracle):
    items, names = _inputs()
    return items, names, [oracle.compress_default(b) for b in items]


@pytest.fixture(scope="module")
def dictionary():
    """what the stream / dictionary builds start from: text, then a stretch of every periodic input's unit"""
    return bytes(dg.text_bytes(3000, 4242)) + b"".join(periodic(120, p, 100 * p) for p in PERIODS)


def _cmp(got, want, names):
    """sizes and statuses, and the bytes below the returned size"""
    bad = []
    for name, (n, data), w in zip(names, got, want):
        if isinstance(w, int):
            if n != w:
                bad.append("%s: status %d, oracle %d" % (name, n, w))
        elif n != len(w) or data[:n] != w:
            bad.append("%s: size %d vs oracle %d" % (name, n, len(w)))
    assert not bad, "%d/%d mismatches: %s" % (len(bad), len(names), "; ".join(bad[:8]))


def test_inputs_take_the_paths_they_are_meant_for(inputs):
    """(no GPU work) every block is long enough for the window path, and the long-match blocks hold a match that cannot
    join a run (length >= 274: its length field needs two extension bytes or more)"""
    items, names, want = inputs
    assert all(len(b) >= 300 for b in items)
    for b, name, w in zip(items, names, want):
        if name.startswith("longmatch"):
            i, longest = 0, 0
            while i < len(w):                                           # walk the sequences
                tok = w[i]; i += 1
                lit = tok >> 4
                if lit == 15:
                    while w[i] == 255: lit += 255; i += 1
                    lit += w[i]; i += 1
                i += lit
                if i >= len(w): break
                i += 2
                ml = tok & 15
                if ml == 15:
                    while w[i] == 255: ml += 255; i += 1
                    ml += w[i]; i += 1
                longest = max(longest, ml + 4)
            assert longest >= 274, name


def test_plain_blocks(zl, gpu, inputs):
    items, names, want = inputs
    _cmp(gh.compress_fast(zl, items, gpu), want, names)
    _cmp(gh.compress_fast(zl, items, gpu, layout=gh.Packed(11, gaps=(1, 3))), want, names)


def test_capacities_from_exact_to_600_more(zl, oracle, gpu, inputs):
    items, names, full = inputs
    its, caps, nms = [], [], []
    for b, name, w in zip(items, names, full):
        for d in CAP_EXTRA:
            its.append(b); caps.append(len(w) + d); nms.append("%s/cap+%d" % (name, d))
    want = [oracle.compress_default(b, cap=c) for b, c in zip(its, caps)]
    _cmp(gh.compress_fast(zl, its, gpu, caps=caps), want, nms)


def test_large_blocks_u32_tables(zl, oracle, gpu):
    items, names = _big()
    want = [oracle.compress_default(b) for b in items]
    _cmp(gh.compress_fast(zl, items, gpu), want, names)
    caps = [len(w) + d for w, d in zip(want, (100, 511))]
    _cmp(gh.compress_fast(zl, items, gpu, caps=caps), [oracle.compress_default(b, cap=c) for b, c in zip(items, caps)], names)


@pytest.mark.parametrize("big", [False, True])
def test_seeded_stream_blocks(zl, gpu, tmp_path, inputs, dictionary, big):
    """compressFastContinue from a loaded dictionary's table: outputs and the tables after the call.  Even blocks start
    from the table of their own first half (its entries are positions of the same bytes in the block, those inside
    matches included, which the block's own parse never puts: the seed changes the parse, and entries at or above a
    probe's position must be refused), odd blocks from the shared dictionary's."""
    cref = sg.ref(tmp_path)
    items = _big()[0] if big else inputs[0]
    dicts = [b[:len(b) // 2] if k % 2 == 0 else dictionary for k, b in enumerate(items)]
    _, loaded = sg.run_load_dict(zl, dicts, gpu)
    tabs = np.stack([cref.load_dict(d)[0] for d in dicts])
    assert np.array_equal(loaded, tabs)
    for extra in (None, 300):
        full = [len(b) + len(b) // 255 + 16 for b in items]
        caps = full if extra is None else [int(r) + extra for r in cref.batch(tabs, None, items, full, 1)[0]]
        got = sg.run_continue(zl, items, caps, tabs, None, gpu)
        want = cref.batch(tabs, None, items, caps, 1)
        assert list(got[0]) == list(want[0])
        assert all(g[:max(int(r), 0)] == w for g, w, r in zip(got[1], want[1], want[0]))
        assert all(np.array_equal(got[2][i], want[2][i]) for i in range(len(items)))


@pytest.mark.parametrize("big", [False, True])
def test_dictionary_blocks(zl, gpu, tmp_path, inputs, dictionary, big):
    """compressFastUsingDict: every second block against the dictionary, the others against their own first bytes"""
    cref = dc.ref(tmp_path)
    items = _big()[0] if big else inputs[0]
    dicts = [dictionary] + [b[:200 + 37 * (k % 5)] for k, b in enumerate(items)]
    idx = [0 if k % 2 == 0 else k + 1 for k in range(len(items))]
    full = [dc.bound(len(b)) for b in items]
    got, want = dc.run_batch(zl, cref, items, full, dicts, idx, gpu)
    dc.check(got, want)
    caps = [w + 300 if w > 0 else c for (w, _), c in zip(want, full)]
    got, want = dc.run_batch(zl, cref, items, caps, dicts, idx, gpu)
    dc.check(got, want)
