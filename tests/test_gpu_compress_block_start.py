"""The start of a block in every build of k_compress_fast: the window path only runs behind a match (its lane 0 is the
anchor's pending put), so a block's first search takes the generic path and the window path takes over at the first
match.  Every block of the block-start corpus (tests/blockstartgen.py), bytes and returned sizes against the oracle, in
one batch per build: the u16 table, the u32 table with and without tags, and the three seeded builds, continued from
zero tables and from a loadDict table.  Acceleration 2 never takes the window path: it is the control.  Everything is
decoded again by batch_decompress_safe."""
import numpy as np
import pytest

import blockstartgen as bg
import gpu_harness as gh
import streamgen as sg

pytestmark = pytest.mark.gpu

# declared bound of the call -> build: u16 table; u32 with tags (the first size past the u16 table, and 1 MiB); u32
# without tags (positions may pass 2^24)
MAX_IN = (65536, 65548, 1 << 20, (1 << 24) + 1)
ACCELS = (1, 2)


@pytest.fixture(scope="module")
def blocks():
    c = bg.corpus()
    return [n for n, _ in c], [b for _, b in c]


@pytest.fixture(scope="module")
def want(oracle, blocks):
    """oracle output per acceleration, computed once"""
    return {a: [oracle.compress_fast(b, a) for b in blocks[1]] for a in ACCELS}


@pytest.fixture(scope="module")
def cref(tmp_path_factory):
    return sg.ref(tmp_path_factory.mktemp("stream_ref"))


def _same(names, got, want):
    bad = ["%s: size %d, oracle %d" % (n, k, len(w)) for n, (k, data), w in zip(names, got, want)
           if k != len(w) or data != w]
    assert not bad, "%d/%d mismatches: %s" % (len(bad), len(names), "; ".join(bad[:8]))


def _round_trip(zl, gpu, names, blocks, comp):
    dec = gh.decompress(zl, comp, [len(b) for b in blocks], gpu)
    bad = [n for n, b, (k, d) in zip(names, blocks, dec) if k != len(b) or d != b]
    assert not bad, "%d blocks do not decode to their input: %s" % (len(bad), ", ".join(bad[:8]))


def test_accel_1_is_the_default(oracle, blocks, want):
    assert all(w == oracle.compress_default(b) for b, w in zip(blocks[1][::7], want[1][::7]))


@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("max_in", MAX_IN)
def test_plain_builds(zl, gpu, blocks, want, max_in, accel):
    names, items = blocks
    got = gh.compress_fast(zl, items, gpu, accel=accel, max_in=max_in)
    _same(names, got, want[accel])
    _round_trip(zl, gpu, names, items, [c for _, c in got])


def _seeded(zl, gpu, cref, blocks, tables, idx, max_in, accel):
    names, items = blocks
    caps = [zl.compressBound(len(b)) for b in items]
    res, outs, tabs = sg.run_continue(zl, items, caps, tables, idx, gpu, accel=accel, max_in=max_in)
    w_res, w_outs, w_tabs = cref.batch(tables, idx, items, caps, accel)
    _same(names, list(zip((int(r) for r in res), outs)), w_outs)
    assert list(res) == list(w_res)
    bad = [n for i, n in enumerate(names) if not np.array_equal(tabs[i], w_tabs[i])]
    assert not bad, "%d final tables differ: %s" % (len(bad), ", ".join(bad[:8]))
    _round_trip(zl, gpu, names, items, outs)
    return outs


@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("max_in", MAX_IN[::2] + MAX_IN[3:])
def test_seeded_from_zero_tables(zl, gpu, cref, blocks, want, max_in, accel):
    """compressFastContinue from an empty table is compressFast: a seeded block starts with anchor 0 and no pending put
    like any other, and takes the same generic first step"""
    idx = np.zeros(len(blocks[0]), dtype=np.uint32)                 # every block starts from the one table
    outs = _seeded(zl, gpu, cref, blocks, np.zeros((1, 4096), dtype=np.uint32), idx, max_in, accel)
    assert outs == want[accel]


@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("max_in", MAX_IN[::2] + MAX_IN[3:])
def test_seeded_from_a_load_dict_table(zl, gpu, cref, blocks, want, max_in, accel):
    """block i continues from the table of a dictionary that is its own first 30 000 bytes: every entry is a position
    at which the block holds the hashed bytes, so the first search meets candidates from its first probe on -- most of
    them ahead of the probe (`match < ip` fails), the slot of position 0's bytes among them"""
    names, items = blocks
    tables = np.stack([cref.load_dict(b[:30000])[0] for b in items])
    outs = _seeded(zl, gpu, cref, blocks, tables, None, max_in, accel)
    assert sum(o != w for o, w in zip(outs, want[accel])) >= 32     # the seeds do change parses
