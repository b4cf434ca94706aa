"""The run masks of the window in every build that has the window path: a pending run keeps its end lanes in a scalar
mask beside its match lanes, the covered lanes and the literal starts of a flush come from those two masks, the fast-run
trip has one exit test and the exact step reads its lane from masks.  Every block of the run-mask corpus
(tests/runmaskgen.py: runs that end at lanes 62, 63, 64 and beyond, a fast run entered at lane 64, exact steps on
duplicate-hash lanes behind a pending run, long and immediate matches behind one, windows with little room), bytes and
returned sizes against the oracle, one batch per build: the u16 table, the u32 table with and without tags, the three
seeded builds, continued from zero tables and from a loadDict table (final tables against the stream reference), and
both dictionary kernels against the C restatement.  Acceleration 2 never takes the window path: it is the control.
Everything is decoded again, against its dictionary where it has one."""
import numpy as np
import pytest

import dictcgen as dc
import dictgen as dgen
import gpu_harness as gh
import runmaskgen as rg
import streamgen as sg

pytestmark = pytest.mark.gpu

# declared bound of the call -> build: u16 table; u32 with tags; u32 without tags (positions may pass 2^24)
MAX_IN = (65536, 1 << 20, (1 << 24) + 1)
ACCELS = (1, 2)


@pytest.fixture(scope="module")
def blocks():
    c = rg.corpus()
    return [n for n, _ in c], [b for _, b in c]


@pytest.fixture(scope="module")
def want(oracle, blocks):
    """oracle output per acceleration, computed once"""
    return {a: [oracle.compress_fast(b, a) for b in blocks[1]] for a in ACCELS}


@pytest.fixture(scope="module")
def cref(tmp_path_factory):
    return sg.ref(tmp_path_factory.mktemp("stream_ref"))


@pytest.fixture(scope="module")
def dref(tmp_path_factory):
    return dc.ref(tmp_path_factory.mktemp("dict_ref"))


def _same(names, got, want):
    bad = ["%s: size %d, oracle %d" % (n, k, len(w)) for n, (k, data), w in zip(names, got, want)
           if k != len(w) or data != w]
    assert not bad, "%d/%d mismatches: %s" % (len(bad), len(names), "; ".join(bad[:8]))


def _round_trip(zl, gpu, names, blocks, comp):
    dec = gh.decompress(zl, comp, [len(b) for b in blocks], gpu)
    bad = [n for n, b, (k, d) in zip(names, blocks, dec) if k != len(b) or d != b]
    assert not bad, "%d blocks do not decode to their input: %s" % (len(bad), ", ".join(bad[:8]))


def test_corpus_shows_every_event():
    assert rg.events() >= set(rg.ew.EVENTS)


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
@pytest.mark.parametrize("max_in", MAX_IN)
def test_seeded_from_zero_tables(zl, gpu, cref, blocks, want, max_in, accel):
    """compressFastContinue from an empty table is compressFast, and leaves the table compressFast would have left"""
    idx = np.zeros(len(blocks[0]), dtype=np.uint32)                 # every block starts from the one table
    outs = _seeded(zl, gpu, cref, blocks, np.zeros((1, 4096), dtype=np.uint32), idx, max_in, accel)
    assert outs == want[accel]


@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("max_in", MAX_IN)
def test_seeded_from_a_load_dict_table(zl, gpu, cref, blocks, want, max_in, accel):
    """block i continues from the table of a dictionary that is its own first 300 bytes: the windows meet candidates that
    lie ahead of the probe (`match < ip` fails) next to the ones the block put itself"""
    names, items = blocks
    tables = np.stack([cref.load_dict(b[:300])[0] for b in items])
    _seeded(zl, gpu, cref, blocks, tables, None, max_in, accel)


@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("max_in", (4096, 1 << 20))
def test_dictionary_kernels(zl, gpu, dref, blocks, want, max_in, accel):
    """k_compress_fast_dict with the 16-bit table (dictionary + record within 65 547 bytes) and with the 32-bit one:
    without a dictionary the oracle's bytes; against a dictionary (the head of another block of the corpus, so that a
    crafted block finds its copies in it as well) the C restatement's"""
    names, items = blocks
    caps = [dc.bound(len(b)) for b in items]
    got, ref = dc.run_batch(zl, dref, items, caps, [b""], [0] * len(items), gpu, accel=accel, max_in=max_in, max_dict=0)
    dc.check(got, ref, "no dictionary")
    _same(names, got, want[accel])
    dicts = [b[:460] for b in items]
    idx = [(i + 1) % len(items) if i % 2 else i for i in range(len(items))]
    got, ref = dc.run_batch(zl, dref, items, caps, dicts, idx, gpu, accel=accel, max_in=max_in, max_dict=460)
    dc.check(got, ref, "with a dictionary")
    dec = dgen.run_batch(zl, [c for _, c in got], [len(b) for b in items], dicts, idx, gpu)
    bad = [n for n, b, (k, d) in zip(names, items, dec) if k != len(b) or d != b]
    assert not bad, "%d blocks do not decode to their input: %s" % (len(bad), ", ".join(bad[:8]))
