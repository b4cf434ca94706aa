"""Test-side helpers for lz4f dictionary frames (tests/test_dict_frame_cpu.py, tests/test_gpu_dict_frame.py,
tests/golden/gen_dict_frames.py, tools/time_dict_frames.py).

* `recipe_dict(recipe)` / `recipe_input(recipe)`: the dictionary and the input a fixture records -- a text dictionary, and
  an input made of the last `period` bytes of that dictionary, repeated, with every flip_every-th byte flipped: block 0
  matches into the dictionary's tail, later blocks into the dictionary (independent) or into the output (linked).
* `liblz4fd()`: LZ4F_createCDict, LZ4F_compressFrame_usingCDict and LZ4F_decompress_usingDict of the system liblz4 through
  ctypes, or None where `liblz4.so.1` or one of the symbols is missing.
* `fixtures()`: tests/golden/dict_frames.json, dictionaries and inputs rebuilt from their recipes and checked by sha256.
* `crafted_cases()`: hand-made dictionary frames for the edges of the history bound, with their expected results.
"""
import base64
import ctypes as C
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools", "pyref"))
import datagen as dg  # noqa: E402
import dictgen  # noqa: E402
import linkedgen  # noqa: E402

FIXTURES = os.path.join(HERE, "golden", "dict_frames.json")
_BIG = dict(dict_len=100000, dict_seed=11, period=60000, input_len=150000, flip_every=1000, block_size_id=4)
RECIPES = (
    dict(_BIG, name="l0_linked", level=0, linked=1, block_checksum=0, content_checksum=0, dict_id=0),
    dict(_BIG, name="l0_independent", level=0, linked=0, block_checksum=0, content_checksum=0, dict_id=0),
    dict(_BIG, name="l9_linked_checksums_dictid", level=9, linked=1, block_checksum=1, content_checksum=1,
         dict_id=0x1234ABCD),
    dict(_BIG, name="l9_independent", level=9, linked=0, block_checksum=0, content_checksum=0, dict_id=0),
    dict(name="l0_record_1000", dict_len=100000, dict_seed=11, period=3000, input_len=1000, flip_every=100,
         block_size_id=4, level=0, linked=1, block_checksum=0, content_checksum=0, dict_id=7),
)


def recipe_dict(r):
    return bytes(dg.text_bytes(r["dict_len"], r["dict_seed"]))


def recipe_input(r):
    """The last `period` bytes of the dictionary, repeated up to input_len, every flip_every-th byte XOR 0x55"""
    d = recipe_dict(r)[-r["period"]:]
    b = bytearray((d * (r["input_len"] // len(d) + 1))[:r["input_len"]])
    for i in range(0, len(b), r["flip_every"]):
        b[i] ^= 0x55
    return bytes(b)


def liblz4fd():
    """-> object with compress(data, dict, level, linked, block_size_id, block_checksum, content_checksum, dict_id) ->
    frame and decompress(frame, cap, dict) -> bytes or None (liblz4 reported an error, or the frame did not end); None
    where liblz4 or one of its dictionary calls is missing."""
    try:
        lib = C.CDLL("liblz4.so.1")
        lib.LZ4F_createCDict, lib.LZ4F_freeCDict, lib.LZ4F_compressFrame_usingCDict, lib.LZ4F_decompress_usingDict
        lib.LZ4F_createCompressionContext, lib.LZ4F_createDecompressionContext
    except (OSError, AttributeError):
        return None
    SZ, VP = C.c_size_t, C.c_void_p
    lib.LZ4F_compressFrameBound.restype, lib.LZ4F_compressFrameBound.argtypes = SZ, [SZ, VP]
    lib.LZ4F_isError.restype, lib.LZ4F_isError.argtypes = C.c_uint, [SZ]
    lib.LZ4F_createCDict.restype, lib.LZ4F_createCDict.argtypes = VP, [VP, SZ]
    lib.LZ4F_freeCDict.restype, lib.LZ4F_freeCDict.argtypes = None, [VP]
    lib.LZ4F_createCompressionContext.restype, lib.LZ4F_createCompressionContext.argtypes = SZ, [C.POINTER(VP), C.c_uint]
    lib.LZ4F_freeCompressionContext.restype, lib.LZ4F_freeCompressionContext.argtypes = SZ, [VP]
    lib.LZ4F_compressFrame_usingCDict.restype = SZ
    lib.LZ4F_compressFrame_usingCDict.argtypes = [VP, VP, SZ, VP, SZ, VP, VP]
    lib.LZ4F_createDecompressionContext.restype, lib.LZ4F_createDecompressionContext.argtypes = SZ, [C.POINTER(VP), C.c_uint]
    lib.LZ4F_freeDecompressionContext.restype, lib.LZ4F_freeDecompressionContext.argtypes = SZ, [VP]
    lib.LZ4F_decompress_usingDict.restype = SZ
    lib.LZ4F_decompress_usingDict.argtypes = [VP, VP, C.POINTER(SZ), VP, C.POINTER(SZ), VP, SZ, VP]

    def buf(b):
        return (C.c_uint8 * max(1, len(b))).from_buffer_copy(b or b"\0")

    class L:
        @staticmethod
        def compress(data, dict_bytes, level=0, linked=True, block_size_id=4, block_checksum=0, content_checksum=0,
                     dict_id=0):
            p = linkedgen._Preferences()
            p.frameInfo.blockSizeID = block_size_id
            p.frameInfo.blockMode = 0 if linked else 1
            p.frameInfo.contentChecksumFlag = content_checksum
            p.frameInfo.blockChecksumFlag = block_checksum
            p.frameInfo.dictID = dict_id
            p.compressionLevel = level
            d = buf(dict_bytes)
            cdict = lib.LZ4F_createCDict(C.addressof(d), len(dict_bytes))
            cctx = VP()
            assert cdict and not lib.LZ4F_isError(lib.LZ4F_createCompressionContext(C.byref(cctx), 100))
            try:
                cap = lib.LZ4F_compressFrameBound(len(data), C.addressof(p))
                out, src = (C.c_uint8 * cap)(), buf(data)
                r = lib.LZ4F_compressFrame_usingCDict(cctx, C.addressof(out), cap, C.addressof(src), len(data), cdict,
                                                      C.addressof(p))
                assert not lib.LZ4F_isError(r), "LZ4F_compressFrame_usingCDict failed"
                return bytes(out[:r])
            finally:
                lib.LZ4F_freeCompressionContext(cctx)
                lib.LZ4F_freeCDict(cdict)

        @staticmethod
        def decompress(frame, cap, dict_bytes):
            ctx = VP()
            assert not lib.LZ4F_isError(lib.LZ4F_createDecompressionContext(C.byref(ctx), 100))
            try:
                src, out, d = buf(frame), (C.c_uint8 * max(1, cap))(), buf(dict_bytes)
                sp = dp = 0
                while True:
                    ss, ds = SZ(len(frame) - sp), SZ(cap - dp)
                    r = lib.LZ4F_decompress_usingDict(ctx, C.addressof(out) + dp, C.byref(ds), C.addressof(src) + sp,
                                                      C.byref(ss), C.addressof(d), len(dict_bytes), None)
                    if lib.LZ4F_isError(r):
                        return None
                    sp += ss.value
                    dp += ds.value
                    if r == 0:
                        return bytes(out[:dp])
                    if ss.value == 0 and ds.value == 0:
                        return None                   # wants more input or more room than there is
            finally:
                lib.LZ4F_freeDecompressionContext(ctx)
    return L


_FIX = None


def fixtures():
    """-> list of dicts: name, recipe, frame, input, dict (bytes); built once and shared"""
    global _FIX
    if _FIX is None:
        out = []
        for e in json.load(open(FIXTURES))["frames"]:
            r = e["recipe"]
            d, data = recipe_dict(r), recipe_input(r)
            assert hashlib.sha256(d).hexdigest() == e["dict_sha256"], "datagen no longer gives the recorded dictionary"
            assert hashlib.sha256(data).hexdigest() == e["input_sha256"], "datagen no longer gives the recorded input"
            frame = base64.b64decode(e["frame_b64"])
            assert hashlib.sha256(frame).hexdigest() == e["frame_sha256"]
            out.append(dict(name=e["name"], recipe=r, frame=frame, input=data, dict=d))
        _FIX = out
    return _FIX


def crafted_cases():
    """-> list of (name, frame, dict, cap, expected result, expected bytes or None, liblz4_checks).  The expected values
    follow section 1 of the contract by hand (W = T ++ output), so the tests also pin the model.  liblz4_checks: the frame
    is valid and liblz4's LZ4F_decompress_usingDict must give the same bytes."""
    seq, pat, build = dictgen.seq, dictgen.pattern, linkedgen.build_frame
    cases = []
    dct = pat(500, 21)                                                 # D = 500
    a, b, c = pat(30, 22), pat(12, 23), pat(9, 24)
    e = pat(7, 27)
    # "linked2": the same block 0 in front of a second block of literals -- a linked-declared frame of two blocks is walked
    # by the one-wavefront decoder, one of one block goes with the independent frames
    for mode, tag, more in ((0, "linked", False), (0, "linked2", True), (1, "independent", False)):
        def frame(block0):
            return build([(block0, False)] + ([(seq(e), False)] if more else []), block_mode=mode)
        x = e if more else b""
        # block 0: 30 literals, then a match at op = 30
        first = frame(seq(a, 30 + 500, 8) + seq(c))                    # o = op + pos + D: T's first byte
        want = a + dct[0:8] + c + x
        cases.append(("%s_match_to_T_first_byte" % tag, first, dct, len(want), len(want), want, True))
        beyond = frame(seq(a, 30 + 501, 8) + seq(c))
        cases.append(("%s_match_one_byte_in_front_of_T" % tag, beyond, dct, len(want) + 8, -116, None, False))
        # starts 5 bytes in front of T's end and crosses into the output: T[-5:] then output[0:15]
        cross = frame(seq(a, 30 + 5, 20) + seq(c))
        want = a + dct[-5:] + a[0:15] + c + x
        cases.append(("%s_match_crosses_T_end" % tag, cross, dct, len(want), len(want), want, True))
        # the same running over itself: offset 3 < length 40 at op = 0 (3 bytes of T, then period 3)
        over = frame(seq(b"", 3, 40) + seq(c))
        want = (dct[-3:] * 14)[:40] + c + x
        cases.append(("%s_match_from_T_over_itself" % tag, over, dct, len(want), len(want), want, True))
        # offset 33 < length 50 at op = 30: 3 bytes of T, then the output from its first byte, then itself
        w = bytearray(dct[-3:] + a)
        for k in range(50):
            w.append(w[len(w) - 33])
        over2 = frame(seq(a, 33, 50) + seq(c))
        want = bytes(w[3:]) + c + x
        cases.append(("%s_match_crosses_and_overlaps" % tag, over2, dct, len(want), len(want), want, True))
        cases.append(("%s_capacity_one_short" % tag, over2, dct, len(want) - 1, -116, None, False))
        # a long match wholly inside T (the 16-byte copy loop), ending at T's last byte
        long_t = frame(seq(a, 30 + 300, 300) + seq(c))
        want = a + dct[-300:] + c + x
        cases.append(("%s_long_match_inside_T" % tag, long_t, dct, len(want), len(want), want, True))
    # block 1 of an independent frame reaches T (and cannot reach block 0)
    blk0 = seq(pat(300, 25))
    ind1 = build([(blk0, False), (seq(b, 12 + 500, 6) + seq(c), False)], block_mode=1)
    want = pat(300, 25) + b + dct[0:6] + c
    cases.append(("independent_block_1_reaches_T", ind1, dct, len(want), len(want), want, True))
    # block 1 of a linked frame with pos = 300, D = 65536, offset 65535 at op = 12: index D + 312 - 65535 = 313 of W
    big = pat(70000, 26)
    T = big[-65536:]
    lnk1 = build([(blk0, False), (seq(b, 65535, 10) + seq(c), False)], block_mode=0)
    want = pat(300, 25) + b + T[313:323] + c
    cases.append(("linked_block_1_pos300_offset_65535", lnk1, big, len(want), len(want), want, True))
    # the same offset from an independent block 1 (op = 12: index 65536 + 12 - 65535 = 13 of T)
    ind2 = build([(blk0, False), (seq(b, 65535, 10) + seq(c), False)], block_mode=1)
    want = pat(300, 25) + b + T[13:23] + c
    cases.append(("independent_block_1_offset_65535", ind2, big, len(want), len(want), want, True))
    # a stored block is history: block 1 reaches through it into T
    st = build([(a, True), (seq(b, 12 + 30 + 4, 10) + seq(c), False)], block_mode=0)
    want = a + b + dct[-4:] + a[0:6] + c
    cases.append(("stored_block_is_history", st, dct, len(want), len(want), want, True))
    # three blocks with block checksums; a checksum error in block 2; a truncated chain
    three = [(seq(a, 30 + 100, 8) + seq(c), False), (seq(b, 12 + 47 + 2, 6) + seq(c), False),
             (seq(b, 5, 7) + seq(c), False)]
    o0 = a + dct[-100:-92] + c
    o1 = b + (dct[-2:] + o0)[0:6] + c
    o2 = b + (b[7:] * 2)[0:7] + c
    want = o0 + o1 + o2
    cases.append(("three_blocks_checksums", build(three, True, want), dct, len(want), len(want), want, True))
    cases.append(("block_checksum_wrong_in_block_2", build(three, True, want, bad_block_cks=2), dct, len(want), -107, None,
                  False))
    cases.append(("chain_truncated", build(three, True, want)[:-(4 + 4 + 4 + 10)], dct, len(want), -114, None, False))
    cases.append(("content_checksum_wrong", build(three, True, want, bad_content_cks=True), dct, len(want), -118, None,
                  False))
    # D = 0: the linked decode (a match into block 0 decodes, one to T does not)
    d0 = build([(blk0, False), (seq(b, 12 + 300, 6) + seq(c), False)], block_mode=0)
    want = pat(300, 25) + b + pat(300, 25)[0:6] + c
    cases.append(("no_dictionary_linked", d0, b"", len(want), len(want), want, True))
    cases.append(("no_dictionary_match_in_front_of_frame", first, b"", 100, -116, None, False))
    return cases
