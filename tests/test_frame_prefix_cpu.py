"""Frame prefix decoding without a GPU: the model tools/pyref/zig_lz4_frame_prefix.py against
liblz4's LZ4F_decompress(_usingDict) into a destination of n bytes, against the full-frame models on every consequence of
the specification, against results stated by hand for the defect and header cases, and the public surface (header, library,
Python binding, Zig and C++ mirrors).  Corpus: tests/frameprefixgen.py."""
import ctypes as C
import os
import re

import pytest

import dictframegen
import frameprefixgen as g
import linkedgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("zlz4f_batch_decompress_frame_prefix", "zlz4f_batch_decompress_frame_prefix_using_dict",
         "zlz4f_decompress_frame_prefix", "zlz4f_decompress_frame_prefix_using_dict")


def _all_cases():
    return g.small_cases() + g.dict_cases() + g.long_cases() + g.fixture_cases()


def test_the_corpus_is_what_the_gpu_test_needs():
    fam = {}
    for c in _all_cases():
        fam.setdefault(c.family, []).append(c)
    assert {"literals", "disjoint", "far", "doubling", "stored", "cross", "empty", "dict", "dictlen", "histcap", "big",
            "fixture"} <= set(fam)
    for c in g.small_cases() + g.dict_cases():        # every n of a small frame: at most 3 KiB of output each
        assert c.ns is None and g.full(c.frame, c.dict)[0] <= 3072, c.name
    assert any(g.full(c.frame)[0] > 2048 for c in fam["far"])          # n > offset >= 1024
    assert all(g.full(c.frame, c.dict)[0] > 65536 for c in fam["histcap"] if c.valid)
    assert {c.valid for c in fam["histcap"]} == {True, False}
    assert g.full(fam["big"][0].frame)[0] > 2 * 260000
    assert [g.full(c.frame)[0] for c in fam["empty"]] == [0, 0]
    # frame kinds: independent and linked, with and without checksums, dictionaries of every length class
    flgs = {c.frame[4] & 0x34 for c in _all_cases()}
    assert {0x00, 0x20, 0x14, 0x34} <= flgs
    assert {min(len(c.dict), 65537) for c in fam["dictlen"]} == {0, 499, 500, 65537}
    assert len(g.items(g.small_cases())) > 10000 and len(g.items(g.dict_cases())) > 3000


def _liblz4_prefix(lib, frame, n, dct):
    """what LZ4F_decompress_usingDict leaves in a destination of n bytes -> bytes, or None on an error"""
    SZ, VP = C.c_size_t, C.c_void_p
    ctx = VP()
    assert not lib.LZ4F_isError(lib.LZ4F_createDecompressionContext(C.byref(ctx), 100))
    try:
        src = (C.c_uint8 * max(1, len(frame))).from_buffer_copy(frame or b"\0")
        out = (C.c_uint8 * (n + 64)).from_buffer_copy(b"\xA5" * (n + 64))
        d = (C.c_uint8 * max(1, len(dct))).from_buffer_copy(dct or b"\0")
        sp = dp = 0
        while dp < n:
            ss, ds = SZ(len(frame) - sp), SZ(n - dp)
            r = lib.LZ4F_decompress_usingDict(ctx, C.addressof(out) + dp, C.byref(ds), C.addressof(src) + sp, C.byref(ss),
                                              C.addressof(d), len(dct), None)
            if lib.LZ4F_isError(r):
                return None
            sp += ss.value
            dp += ds.value
            if r == 0:
                break
            if ss.value == 0 and ds.value == 0:
                return None
        assert bytes(out[n:]) == b"\xA5" * 64
        return bytes(out[:dp])
    finally:
        lib.LZ4F_freeDecompressionContext(ctx)


def test_model_against_liblz4():
    """every valid corpus frame at every n of its case (the small frames: 0 .. S + 1): the bytes liblz4 leaves in a
    destination of n bytes are the model's, and their count is the model's result"""
    if linkedgen.liblz4f() is None or dictframegen.liblz4fd() is None:
        pytest.skip("liblz4 does not load")
    lib = C.CDLL("liblz4.so.1")
    SZ, VP = C.c_size_t, C.c_void_p
    lib.LZ4F_isError.restype, lib.LZ4F_isError.argtypes = C.c_uint, [SZ]
    lib.LZ4F_createDecompressionContext.restype, lib.LZ4F_createDecompressionContext.argtypes = SZ, [C.POINTER(VP), C.c_uint]
    lib.LZ4F_freeDecompressionContext.restype, lib.LZ4F_freeDecompressionContext.argtypes = SZ, [VP]
    lib.LZ4F_decompress_usingDict.restype = SZ
    lib.LZ4F_decompress_usingDict.argtypes = [VP, VP, C.POINTER(SZ), VP, C.POINTER(SZ), VP, SZ, VP]
    seen = 0
    for c in _all_cases():
        if not c.valid:
            continue
        S = g.full(c.frame, c.dict)[0]
        for name, f, n, d in g.items([c]):
            got = _liblz4_prefix(lib, f, n, d or b"")
            wn, wd = g.expected(f, n, d)
            assert got is not None and wn == min(S, n) and got == wd, name
            seen += 1
    assert seen > 15000


def test_model_against_the_full_frame_models():
    """the consequences of section 4.4f, on the whole corpus and on the defect cases"""
    lf, dfm = linkedgen.lf, g.dfm
    for c in _all_cases():
        R, data = g.full(c.frame, c.dict)
        if not c.dict:                                # D == 0: the linked decode
            assert (R, data) == lf.decompress_frame_linked(c.frame, g.BIG), c.name
        for name, f, n, d in g.items([c]):
            r, got = g.expected(f, n, d)
            if R >= 0:                                # min(S, n) and the first bytes of the full decode
                assert (r, got) == (min(R, n), data[:n]), name
                if n > R:                             # the full decode's own result into n bytes
                    assert (r, got) == dfm.decompress_frame_using_dict(f, n, d), name
            else:
                assert r == n or r == R, name         # cut in front of the defect, or the decode's own error
        assert g.expected(c.frame, 10 ** 7, c.dict) == (R, data), c.name       # with room to spare: R itself
    for c, want in g.defect_cases():
        R, _ = g.full(c.frame, c.dict)
        assert g.expected(c.frame, 100000, c.dict)[0] == R == want(100000), c.name
        assert g.expected(c.frame, 0, c.dict) == (0, b""), c.name


def test_defects_on_both_sides_of_the_cut():
    """results stated by hand (frameprefixgen.defect_cases): a defect is reported once n exceeds the bytes that decode in
    front of it, and not before; at n == S a bad content checksum, a missing end mark and a cut tail are not reported"""
    names = set()
    for c, want in g.defect_cases():
        names.add(c.name)
        prev = None
        for name, f, n, d in g.items([c]):
            r, data = g.expected(f, n, d)
            assert r == want(n), (name, r, want(n))
            if r >= 0:
                assert len(data) == r and (prev is None or data[:len(prev)] == prev), name
                prev = data
    assert {"defect_corrupt_block2", "defect_bad_block_cks_0", "defect_bad_block_cks_2", "defect_missing_block_cks_1",
            "defect_truncated_in_block2", "defect_no_end_mark", "defect_no_end_mark_cks", "defect_bad_content_cks",
            "defect_missing_content_cks"} <= names
    by = {c.name: (c, w) for c, w in g.defect_cases()}
    c, _ = by["defect_bad_content_cks"]
    assert g.expected(c.frame, 170)[0] == 170 and g.expected(c.frame, 171)[0] == g.CONTENT_CHECKSUM
    c, _ = by["defect_truncated_in_block2"]
    assert g.expected(c.frame, 126)[0] == 126 and g.expected(c.frame, 127)[0] == g.FRAME_SIZE_WRONG
    c, _ = by["defect_corrupt_block2"]
    assert g.expected(c.frame, 30)[0] == 30 and g.expected(c.frame, 139)[0] == g.FAILED


def test_header_errors_come_first():
    codes = set()
    for name, f, want in g.header_cases():
        for n in (0, 1, 5000):
            assert g.expected(f, n) == (want, b""), (name, n)
            assert g.expected(f, n, b"x" * 100) == (want, b""), (name, n)
        assert g.full(f)[0] == want, name
        codes.add(want)
    assert codes == {g.HEADER_INCOMPLETE, g.TYPE_UNKNOWN, g.VERSION_WRONG, g.RESERVED, g.MAX_BLOCK_SIZE, g.HEADER_CHECKSUM}
    ok = g.small_cases()[0].frame                     # after a good header n == 0 gives 0
    assert g.expected(ok, 0) == (0, b"")


def test_surface_header_library_binding_and_mirrors(zl):
    """the four calls are declared, exported, bound and mirrored (fails before frame prefix decoding existed)"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zlz4_amd.h")).read(), flags=re.S)
    zig = open(os.path.join(ROOT, "zig-lz4_amd", "zig", "root.zig")).read()
    hpp = open(os.path.join(ROOT, "zig-lz4_amd", "csrc", "host", "zlz4.hpp")).read()
    L = zl.lib()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), "%s is not declared" % name
        assert hasattr(L, name), "%s is not exported" % name
        assert name in zl.SYMBOLS, "%s is not bound" % name
        assert re.search(r'extern "c" fn %s\(' % name, zig), "%s: no Zig extern" % name
        assert len(re.findall(r"\b%s\(" % name, zig)) >= 2, "%s: no Zig entry" % name
        assert re.search(r"\b%s\(" % name, hpp), "%s: no C++ entry" % name
    for fn in ("decompressFramePrefix", "decompressFramePrefixUsingDict", "decompressFramePrefixBatch",
               "decompressFramePrefixBatchUsingDict"):
        assert re.search(r"pub fn %s\(" % fn, zig), fn
        assert re.search(r"inline Result %s\(" % fn, hpp), fn
    assert callable(zl.lz4f.decompressFramePrefix) and callable(zl.lz4f.decompressFramePrefixes)
    assert callable(zl.batch_decompress_frame_prefix)
    # host-side argument checks need no device
    nul9 = [None] * 8
    assert L.zlz4f_batch_decompress_frame_prefix(*nul9, 0) == 0
    assert L.zlz4f_batch_decompress_frame_prefix(*nul9, 3) == -5
    assert L.zlz4f_batch_decompress_frame_prefix_using_dict(*nul9, 0, None, None, None, 1, None) == 0
    assert L.zlz4f_batch_decompress_frame_prefix_using_dict(*nul9, 3, None, None, None, 1, None) == -5
    buf = (C.c_uint8 * 64)()
    for name, f, want in g.header_cases():            # a header error is the result, also when n == 0
        for cap in (0, 64):
            assert L.zlz4f_decompress_frame_prefix(f, len(f), C.addressof(buf), cap) == want, name
            assert L.zlz4f_decompress_frame_prefix_using_dict(f, len(f), C.addressof(buf), cap, b"abc", 3) == want, name
    ok = g.small_cases()[0].frame
    assert L.zlz4f_decompress_frame_prefix(ok, len(ok), None, 0) == 0  # a good header, n == 0
    assert L.zlz4f_decompress_frame_prefix_using_dict(ok, len(ok), C.addressof(buf), 64, None, 5) == -5
    assert L.zlz4f_decompress_frame_prefix(ok, len(ok), None, 64) == -5
    assert L.zlz4f_decompress_frame_prefix(None, 10, C.addressof(buf), 64) == -5
    assert zl.lz4f.decompressFramePrefixes([], 5) == []
