"""max_in_len is a bound, not the exact maximum: the bytes of a batch call must not depend on it.

The launchers pick a build from max_in_len -- k_compress_fast with a 16-bit table (<= 65 547), a 32-bit table with an
8-bit tag (<= 2^24) or a plain 32-bit table (above); the HC pipeline with its links in LDS (<= 65 536) or in HBM -- so a
caller who declares a loose bound over small records meets another build than one who passes the exact maximum.  Each
test runs one corpus under several declared bounds and compares every result with the oracle, status for status and
byte for byte.  Run on the GPU box: pytest -m gpu."""
import numpy as np
import pytest

import cases
import datagen as dg
import gpu_harness as gh
import streamgen as sg
from test_gpu_dest_size_batch import Batch
from test_gpu_dest_size_batch import _check as _check_dest_size
from test_gpu_packed_layout import _plain_blocks
from test_gpu_parity import _cmp

pytestmark = pytest.mark.gpu

U16_MAX = 65536 + 11                              # the largest block of the 16-bit table
T = 1 << 24                                       # the largest block of the tagged 32-bit table
LEGAL_MAX = 0x7E000000                            # the largest legal block
BOUNDS = [U16_MAX, U16_MAX + 1, T, T + 1, LEGAL_MAX]


def _corpus():
    c = [(n, b) for n, b in cases.reference_test_inputs() + cases.seeded_cases() if len(b) <= U16_MAX]
    for n in (65536, U16_MAX):
        c.append(("full text/%d" % n, bytes(dg.text_bytes(n, 300 + n))))
        c.append(("full mixed/%d" % n, bytes(dg.mixed_bytes(n, 300 + n))))
    return c


def _wide_extras():
    """blocks longer than the 16-bit table allows, for the bounds above it"""
    far = [(n, b) for n, b in cases.seeded_cases() if n == "random+copy-far"]
    assert len(far) == 1 and len(far[0][1]) > U16_MAX
    return [("text/65548", bytes(dg.text_bytes(65548, 1))), ("text/70001", bytes(dg.text_bytes(70001, 2)))] + far


@pytest.fixture(scope="module")
def corpus():
    return _corpus(), _wide_extras()


_want = {}


def _oracle_fast(oracle, sel, accel):
    """oracle.compress_fast of every block, computed once per acceleration"""
    out = []
    for name, b in sel:
        if (name, accel) not in _want:
            _want[(name, accel)] = oracle.compress_fast(b, accel)
        out.append(_want[(name, accel)])
    return out


@pytest.mark.parametrize("accel", [1, 7, 65537])
@pytest.mark.parametrize("max_in", BOUNDS)
def test_compress_fast_under_declared_bound(zl, oracle, gpu, corpus, max_in, accel):
    sel = corpus[0] + [(n, b) for n, b in corpus[1] if len(b) <= max_in]      # (at 65 548 only the 65 548-byte block fits)
    assert len(sel) > len(corpus[0]) or max_in == U16_MAX
    assert len({n for n, _ in sel}) == len(sel) and max(len(b) for _, b in sel) <= max_in
    got = gh.compress_fast(zl, [b for _, b in sel], gpu, accel=accel, max_in=max_in)
    _cmp([n for n, _ in sel], got, _oracle_fast(oracle, sel, accel))


def test_output_too_small_under_loose_bound(zl, oracle, gpu, corpus):
    """short destinations on the untagged 32-bit build: the same OutputTooSmall / success decision and the same bytes"""
    names, items, caps = [], [], []
    for n, b in corpus[0]:
        if not (13 <= len(b) <= 20000):
            continue
        full = len(oracle.compress_default(b))
        for cap in (full, full - 1, full // 2, 1, 0):
            names.append("%s/cap%d" % (n, cap)); items.append(b); caps.append(cap)
    assert len(items) > 500
    got = gh.compress_fast(zl, items, gpu, caps=caps, max_in=T + 1)
    want = [oracle.compress_default(b, cap=c) for b, c in zip(items, caps)]
    assert sum(isinstance(w, int) for w in want) > len(want) // 2
    _cmp(names, got, want)


@pytest.fixture(scope="module")
def cref(tmp_path_factory):
    return sg.ref(tmp_path_factory.mktemp("streamref"))


@pytest.mark.parametrize("accel", [1, 64])
@pytest.mark.parametrize("n", [5000, U16_MAX])
def test_stream_continue_under_declared_bound(zl, gpu, cref, n, accel):
    """seeded blocks (streamgen.planted: the seed must produce a match where its probe is on the schedule of the
    acceleration) through the three seeded builds: results, bytes and output tables equal the restatement's, and so
    each other's"""
    items, tabs = [], []
    for k, r_off in enumerate((20, 63, 100, 65) * 3):
        b, v, G = sg.planted(n - (k % 5), 9000 + n + 16 * accel + k, r_off=r_off)
        t = np.zeros(sg.ENTRIES, np.uint32)
        t[sg.hash4(G)] = v
        items.append(b); tabs.append(t)
    tabs = np.stack(tabs)
    caps = [len(b) + len(b) // 255 + 16 for b in items]
    wr, wo, wt = cref.batch(tabs, None, items, caps, accel)
    zero = cref.batch(np.zeros_like(tabs), None, items, caps, accel)
    assert sum(z != w for z, w in zip(zero[1], wo)) >= len(items) // 4, "the seeds changed too few blocks"
    for max_in in (n, T, T + 1):
        gr, go, gt = sg.run_continue(zl, items, caps, tabs, None, gpu, accel=accel, max_in=max_in)
        bad = [i for i in range(len(items)) if gr[i] != wr[i] or go[i] != wo[i]]
        assert not bad, "max_in %d: blocks %s differ (GPU %d vs %d)" % (max_in, bad[:8], gr[bad[0]], wr[bad[0]])
        tb = [i for i in range(len(items)) if not np.array_equal(gt[i], wt[i])]
        assert not tb, "max_in %d: tables %s differ" % (max_in, tb[:8])


def test_dest_size_batch_under_loose_bound(zl, oracle, gpu):
    """zlz4_batch_compress_dest_size with a 16 MiB + 1 bound over small blocks: its workspace slots are sized by the
    bound, its full-length pass runs the untagged build"""
    text = bytes(dg.text_bytes(50000, 1))
    rand, zeros = bytes(dg.random_bytes(30000, 2)), b"\0" * 40000
    pairs = [(text, 1000), (text, 10000), (text, len(text) + 200), (rand, 10000), (rand, 70000), (zeros, 100),
             (text[:100], 13), (b"", 0)]
    items, caps = [b for b, _ in pairs], [c for _, c in pairs]
    bt = Batch(zl, items, caps, gpu, max_in=T + 1)
    assert bt.ws.numel() >= 8 * zl.compressBound(T)
    bt.call()
    _check_dest_size(oracle, items, caps, bt.collect())
    del bt


@pytest.mark.parametrize("level", [2, 4, 9, 11])
@pytest.mark.parametrize("max_in", [65536, 65537])
def test_compress_hc_on_both_sides_of_the_lds_link_limit(zl, oracle, gpu, level, max_in):
    """the same blocks with their links in LDS (16-bit, max_in_len <= 65 536) and in HBM (32-bit)"""
    items = _plain_blocks(150, 40 + level, 65536)
    got = gh.compress_hc(zl, items, gpu, level, max_in=max_in)
    want = [oracle.compress_hc(b, level) for b in items]
    _cmp(["blk%d/n%d" % (i, len(b)) for i, b in enumerate(items)], got, want)
