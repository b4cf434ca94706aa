"""Prefix decoding without a GPU: the model (tools/pyref/zig_lz4_prefix.py) against liblz4's LZ4_decompress_safe_partial
and against the full-decode model (tools/pyref/zig_lz4_dict.py) over the corpus of tests/prefixgen.py, and the surface
(header, library, Python binding)."""
import ctypes as C
import os
import re

import pytest

import dictgen
import prefixgen as pg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORRUPTED = -3
NAMES = ("zlz4_decompress_safe_prefix", "zlz4_decompress_safe_prefix_using_dict", "zlz4_batch_decompress_safe_prefix",
         "zlz4_batch_decompress_safe_prefix_using_dict")


def test_the_corpus_is_what_the_gpu_test_needs():
    """more than 6144 items per call (the lane-copy build), every stream decodable, the long one past 7200 bytes"""
    assert len(pg.plain_items()) > 6144 and len(pg.dict_items()) > 6144
    for name, s, _ in pg.exhaustive_streams():
        assert 0 < pg.full_size(s) <= 1400, name
    assert pg.full_size(pg.long_stream()[1]) > 7200
    for name, s, p in pg.malformed_streams():
        assert pg.full_size(s) == CORRUPTED and pg.full_size(s, pg.DICT) == CORRUPTED, name


def test_model_against_liblz4():
    """every valid stream at every cap of the corpus: result and bytes of LZ4_decompress_safe_partial(src, dst, n, cap, cap)"""
    dec = dictgen.liblz4()
    if dec is None:
        pytest.skip("liblz4 does not load")
    fn = dec.lib.LZ4_decompress_safe_partial
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    items = pg.valid_items()
    assert len(items) > 6000
    bufs = {}
    for name, s, cap, _ in items:
        if s not in bufs:
            bufs[s] = (C.c_uint8 * len(s)).from_buffer_copy(s)
        o = (C.c_uint8 * (cap + 64)).from_buffer_copy(b"\xA5" * (cap + 64))
        r = fn(C.addressof(bufs[s]), C.addressof(o), len(s), cap, cap)
        wn, wd = pg.expected(s, cap, None)
        assert r == wn == min(pg.full_size(s), cap), name
        assert bytes(o[:r]) == wd, name
        assert bytes(o[cap:]) == b"\xA5" * 64, name


def test_model_against_the_full_decode_model():
    """cap >= S: the full decode's result and bytes; cap < S: its first cap bytes"""
    full = {}
    items = pg.plain_items() + pg.dict_items()
    for name, s, cap, d in items:
        key = (s, d)
        if key not in full:
            full[key] = pg.pd.decompress_generic(s, 1 << 24, 1 << 24, d)
        fn, fd = full[key]
        if fn < 0:
            continue                                  # (a dictionary too short for the stream: the test below)
        got = pg.expected(s, cap, d)
        assert got == (min(fn, cap), fd[:cap]), name
        if cap >= fn:
            assert got == pg.pd.decompress_generic(s, cap, cap, d), name
    assert sum(1 for k in full if full[k][0] >= 0) >= 40


def test_model_on_malformed_streams():
    """the full decode's error when the defect lies before the cut, cap when it lies behind: a defect met at output
    position p (after its sequence's literals) is reached iff cap > p"""
    for with_dict in (False, True):
        where = {s: p for _, s, p in pg.malformed_streams()}
        items = pg.malformed_items(with_dict)
        assert len(items) > 1000
        for name, s, cap, d in items:
            n, data = pg.expected(s, cap, d)
            if cap <= where[s]:
                assert n == cap and len(data) == cap, name
            else:
                assert n == CORRUPTED == pg.full_size(s, d), name
    # a dictionary shorter than the first match needs: CorruptedData once the match is reached, cap before
    seen, short, litend = 0, {}, {s: p for _, s, p in pg.dict_streams()}
    for name, s, cap, d in pg.dict_items():
        if (s, d) not in short:
            short[(s, d)] = pg.full_size(s, d) < 0
        if short[(s, d)]:
            n, _ = pg.expected(s, cap, d)
            assert n == (cap if cap <= litend[s] else CORRUPTED), name
            seen += 1
    assert seen > 1000
    # literals that end exactly at cap in front of an offset of 0: the offset is not read
    s = dictgen.seq(b"abcdef", 0, 4) + dictgen.seq(pg.TAIL)
    assert pg.expected(s, 6, None) == (6, b"abcdef") and pg.expected(s, 7, None)[0] == CORRUPTED
    assert pg.expected(b"", 5, None) == (0, b"") and pg.expected(s, 0, None) == (0, b"")


def test_surface_header_library_and_binding(zl):
    """the four calls are declared, exported and bound (fails before prefix decoding existed)"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zlz4_amd.h")).read(), flags=re.S)
    L = zl.lib()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), "%s is not declared" % name
        assert hasattr(L, name), "%s is not exported" % name
        assert name in zl.SYMBOLS, "%s is not bound" % name
    for fn in ("decompressSafePrefix", "decompressSafePrefixUsingDict", "batch_decompress_safe_prefix",
               "batch_decompress_safe_prefix_using_dict", "decompressBlockPrefixes"):
        assert callable(getattr(zl, fn, None)), fn
    # host-side argument checks need no device
    assert L.zlz4_decompress_safe_prefix(None, 0, None, 10) == 0
    assert L.zlz4_decompress_safe_prefix_using_dict(b"\x10A", 2, None, 0, None, 0) == 0
    buf = (C.c_uint8 * 8)()
    assert L.zlz4_decompress_safe_prefix_using_dict(b"\x10A", 2, C.addressof(buf), 8, None, 5) == -5
    assert L.zlz4_batch_decompress_safe_prefix(None, None, None, None, None, None, None, None, 0) == 0
    assert L.zlz4_batch_decompress_safe_prefix(None, None, None, None, None, None, None, None, 3) == -5
    assert L.zlz4_batch_decompress_safe_prefix_using_dict(None, None, None, None, None, None, None, None, None, None, None, 3) == -5
