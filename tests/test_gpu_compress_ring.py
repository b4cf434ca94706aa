"""k_compress_fast's input ring (the window path reads its bytes from three VGPRs loaded 256 bytes at a time, see the
kernel): bytes and statuses against the oracle where the ring's loads are most exposed -- blocks packed at odd byte
offsets with the last one ending at the end of the input buffer, sizes around the window path's exit (A + 192 >= L),
blocks > 64 KiB (u32 table with tags), and seeded stream blocks."""
import numpy as np
import pytest

import datagen as dg
import gpu_harness as gh
import streamgen as sg

pytestmark = pytest.mark.gpu

GENS = (dg.text_bytes, dg.reptext_bytes, dg.mixed_bytes, dg.zero_bytes, dg.random_bytes)


def _compress_tight(zl, items, dev, caps=None, seed=0):
    """batch_compress_fast over blocks packed back to back at odd offsets (gaps of 1..3 bytes), the input tensor ending
    exactly where the last block ends; output slots with guard bands (gpu_harness.Packed).  -> [(status, bytes)]"""
    return gh.compress_fast(zl, items, dev, caps=caps, layout=gh.Packed(seed, gaps=(1, 3)))


def _cmp(got, want, names):
    bad = []
    for name, (n, data), w in zip(names, got, want):
        if isinstance(w, int):
            if n != w:
                bad.append("%s: status %d, oracle %d" % (name, n, w))
        elif n != len(w) or data != w:
            bad.append("%s: size %d vs oracle %d" % (name, n, len(w)))
    assert not bad, "%d/%d mismatches: %s" % (len(bad), len(names), "; ".join(bad[:8]))


def test_odd_offsets_last_block_at_buffer_end(zl, oracle, gpu):
    rng = np.random.default_rng(5)
    items, names = [], []
    for i in range(120):
        n = int(rng.integers(13, 65548)) if i % 4 else 65536
        items.append(bytes(GENS[i % 5](n, 300 + i)))
        names.append("%s/%d" % (GENS[i % 5].__name__, n))
    items.append(bytes(dg.text_bytes(65547, 999)))     # the last block: ends at the last byte of the input tensor
    names.append("text_bytes/65547/last")
    _cmp(_compress_tight(zl, items, gpu, seed=1), [oracle.compress_default(b) for b in items], names)


@pytest.mark.parametrize("gen", [dg.text_bytes, dg.reptext_bytes, dg.mixed_bytes])
def test_sizes_around_the_window_exit(zl, oracle, gpu, gen):
    """src_size = 64 m + r, r = 13..400 (the last windows' A + 192 crosses L at every phase), and 65535 / 65536 / 65547"""
    sizes = [64 * m + r for m in (3, 64) for r in range(13, 401)] + [65535, 65536, 65547]
    items = [bytes(gen(n, 11 + k)) for k, n in enumerate(sizes)]
    names = ["%s/%d" % (gen.__name__, n) for n in sizes]
    _cmp(_compress_tight(zl, items, gpu, seed=2), [oracle.compress_default(b) for b in items], names)


def test_output_too_small_at_odd_offsets(zl, oracle, gpu):
    items, caps, names = [], [], []
    for k, n in enumerate((300, 4096 + 77, 65536)):
        b = bytes(dg.text_bytes(n, 40 + k))
        full = len(oracle.compress_default(b))
        for c in (full, full - 1, full // 2, 17):
            items.append(b); caps.append(c); names.append("%d/cap%d" % (n, c))
    want = [oracle.compress_default(b, cap=c) for b, c in zip(items, caps)]
    _cmp(_compress_tight(zl, items, gpu, caps=caps, seed=3), want, names)


def test_large_blocks_tagged_u32_table(zl, oracle, gpu):
    """64 x 256 KiB (max_in_len > 65547: the u32 table with 8-bit tags), odd offsets, last block at the buffer end"""
    items = [bytes(GENS[i % 3](262144 - (i % 7), 500 + i)) for i in range(64)]
    names = ["%s/%d" % (GENS[i % 3].__name__, len(b)) for i, b in enumerate(items)]
    _cmp(_compress_tight(zl, items, gpu, seed=4), [oracle.compress_default(b) for b in items], names)


@pytest.mark.parametrize("n", [5000, 65547, 262144])
def test_seeded_stream_batch(zl, gpu, tmp_path, n):
    """compressFastContinue blocks with planted seeds (streamgen.planted) against the C restatement"""
    cref = sg.ref(tmp_path)
    items, tabs = [], []
    for k in range(12):
        b, v, G = sg.planted(n - (k % 5), 8100 + n + k, r_off=(20, 63, 100)[k % 3])
        t = np.zeros(4096, np.uint32)
        t[sg.hash4(G)] = v
        items.append(b)
        tabs.append(t)
    tabs = np.stack(tabs)
    caps = [len(b) + len(b) // 255 + 16 for b in items]
    got = sg.run_continue(zl, items, caps, tabs, None, gpu, max_in=n)
    want = cref.batch(tabs, None, items, caps, 1)
    assert list(got[0]) == list(want[0]) and got[1] == want[1]
    assert all(np.array_equal(got[2][i], want[2][i]) for i in range(len(items)))
