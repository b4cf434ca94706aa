"""Test-side helpers for linked-block frames (tests/test_linked_frame_cpu.py, tests/test_gpu_linked_frame.py,
tests/golden/gen_linked_frame_fixtures.py).

* `recipe_input(recipe)`: the input a fixture records -- text of period 40 000 (so that every block matches into the
  64 KiB in front of it) with every 1000th byte flipped (so that the matches are short enough to need many of them).
* `liblz4f()`: LZ4F_compressFrame / LZ4F_decompress of the system liblz4 through ctypes, or None where it does not load.
* `fixtures()`: tests/golden/linked_frames.json, inputs rebuilt from their recipes and checked against their sha256.
* `crafted_cases()`: hand-made linked frames for the edges of the history bound and the frame's error order.
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
import zig_lz4_linked_frame as lf  # noqa: E402
from zig_lz4_sizes import xxh32  # noqa: E402

FIXTURES = os.path.join(HERE, "golden", "linked_frames.json")
RECIPES = (
    dict(name="text160k_bs64k", period=40000, seed=5, repeats=4, flip_every=1000, block_size_id=4, block_checksum=0,
         content_checksum=0),
    dict(name="text160k_bs64k_checksums", period=40000, seed=5, repeats=4, flip_every=1000, block_size_id=4,
         block_checksum=1, content_checksum=1),
    dict(name="text600k_bs256k", period=40000, seed=5, repeats=15, flip_every=1000, block_size_id=5, block_checksum=0,
         content_checksum=0),
)


def recipe_input(r):
    """bytes(datagen.text_bytes(period, seed)) * repeats with every flip_every-th byte (0, flip_every, ...) XOR 0x55"""
    b = bytearray(bytes(dg.text_bytes(r["period"], r["seed"])) * r["repeats"])
    for i in range(0, len(b), r["flip_every"]):
        b[i] ^= 0x55
    return bytes(b)


class _FrameInfo(C.Structure):
    _fields_ = [("blockSizeID", C.c_int), ("blockMode", C.c_int), ("contentChecksumFlag", C.c_int), ("frameType", C.c_int),
                ("contentSize", C.c_ulonglong), ("dictID", C.c_uint), ("blockChecksumFlag", C.c_int)]


class _Preferences(C.Structure):
    _fields_ = [("frameInfo", _FrameInfo), ("compressionLevel", C.c_int), ("autoFlush", C.c_uint),
                ("favorDecSpeed", C.c_uint), ("reserved", C.c_uint * 3)]


def liblz4f():
    """-> object with compress(data, block_size_id, block_checksum, content_checksum, linked=True) -> frame and
    decompress(frame, cap) -> bytes or None (liblz4 reported an error, or the frame did not end); None without liblz4."""
    try:
        lib = C.CDLL("liblz4.so.1")
        lib.LZ4F_compressFrame, lib.LZ4F_decompress, lib.LZ4F_createDecompressionContext
    except (OSError, AttributeError):
        return None
    lib.LZ4F_compressFrameBound.restype = C.c_size_t
    lib.LZ4F_compressFrameBound.argtypes = [C.c_size_t, C.c_void_p]
    lib.LZ4F_compressFrame.restype = C.c_size_t
    lib.LZ4F_compressFrame.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.LZ4F_isError.restype = C.c_uint
    lib.LZ4F_isError.argtypes = [C.c_size_t]
    lib.LZ4F_createDecompressionContext.restype = C.c_size_t
    lib.LZ4F_createDecompressionContext.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    lib.LZ4F_freeDecompressionContext.restype = C.c_size_t
    lib.LZ4F_freeDecompressionContext.argtypes = [C.c_void_p]
    lib.LZ4F_decompress.restype = C.c_size_t
    lib.LZ4F_decompress.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p, C.POINTER(C.c_size_t),
                                    C.c_void_p]

    class L:
        @staticmethod
        def compress(data, block_size_id=4, block_checksum=0, content_checksum=0, linked=True):
            p = _Preferences()
            p.frameInfo.blockSizeID = block_size_id
            p.frameInfo.blockMode = 0 if linked else 1
            p.frameInfo.contentChecksumFlag = content_checksum
            p.frameInfo.blockChecksumFlag = block_checksum
            cap = lib.LZ4F_compressFrameBound(len(data), C.addressof(p))
            out = (C.c_uint8 * cap)()
            src = (C.c_uint8 * max(1, len(data))).from_buffer_copy(data or b"\0")
            r = lib.LZ4F_compressFrame(C.addressof(out), cap, C.addressof(src), len(data), C.addressof(p))
            assert not lib.LZ4F_isError(r), "LZ4F_compressFrame failed"
            return bytes(out[:r])

        @staticmethod
        def decompress(frame, cap):
            ctx = C.c_void_p()
            assert not lib.LZ4F_isError(lib.LZ4F_createDecompressionContext(C.byref(ctx), 100))
            try:
                src = (C.c_uint8 * max(1, len(frame))).from_buffer_copy(frame or b"\0")
                out = (C.c_uint8 * max(1, cap))()
                sp = dp = 0
                while True:
                    ss, ds = C.c_size_t(len(frame) - sp), C.c_size_t(cap - dp)
                    r = lib.LZ4F_decompress(ctx, C.addressof(out) + dp, C.byref(ds), C.addressof(src) + sp, C.byref(ss), None)
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


def fixtures():
    """-> list of dicts: name, recipe, frame (bytes), input (bytes)"""
    out = []
    for e in json.load(open(FIXTURES))["frames"]:
        data = recipe_input(e["recipe"])
        assert hashlib.sha256(data).hexdigest() == e["input_sha256"], "datagen no longer gives the recorded input"
        frame = base64.b64decode(e["frame_b64"])
        assert hashlib.sha256(frame).hexdigest() == e["frame_sha256"]
        out.append(dict(name=e["name"], recipe=e["recipe"], frame=frame, input=data))
    return out


def build_frame(blocks, block_checksum=False, content=None, end_mark=True, block_mode=0, bad_block_cks=None,
                bad_content_cks=False):
    """A frame from ready-made blocks: (payload, stored) pairs.  content: the bytes whose XXH32 ends the frame (None: no
    content checksum).  bad_block_cks: index of the block whose checksum is flipped."""
    out = bytearray(lf.encode_header(4, block_mode, 0 if content is None else 1, 1 if block_checksum else 0))
    for k, (body, stored) in enumerate(blocks):
        out += (len(body) | (0x80000000 if stored else 0)).to_bytes(4, "little") + body
        if block_checksum:
            out += (xxh32(body) ^ (1 if bad_block_cks == k else 0)).to_bytes(4, "little")
    if end_mark:
        out += b"\0\0\0\0"
    if content is not None:
        out += (xxh32(content) ^ (1 if bad_content_cks else 0)).to_bytes(4, "little")
    return bytes(out)


def crafted_cases():
    """-> list of (name, frame, cap, expected result, expected bytes or None).  The expected values are the model's
    (zig_lz4_linked_frame.decompress_frame_linked), stated here so that the tests also pin the model."""
    seq, pat = dictgen.seq, dictgen.pattern
    a, b, c = pat(300, 1), pat(40, 2), pat(25, 3)
    blk0 = seq(a)                                                      # block 0: 300 literals
    # block 1: 40 literals, then a match of 20 that starts `reach` bytes in front of the block (offset = 40 + reach)
    exact = seq(b, 40 + 300, 20) + seq(c)
    beyond = seq(b, 40 + 301, 20) + seq(c)
    want_exact = a + b + a[0:20] + c
    blk2 = seq(pat(10, 4), 10 + 385 + 0, 8) + seq(pat(6, 5))           # block 2: matches block 0's first bytes again
    want3 = want_exact + pat(10, 4) + a[0:8] + pat(6, 5)
    three = [(blk0, False), (exact, False), (blk2, False)]
    cases = [
        ("match_to_the_first_byte", build_frame([(blk0, False), (exact, False)]), len(want_exact), len(want_exact),
         want_exact),
        ("match_one_byte_before_the_frame", build_frame([(blk0, False), (beyond, False)]), len(want_exact) + 8, -116, None),
        ("three_blocks_checksums", build_frame(three, True, want3), len(want3), len(want3), want3),
        ("block_checksum_wrong_in_block_2", build_frame(three, True, want3, bad_block_cks=2), len(want3), -107, None),
        ("chain_truncated", build_frame(three, True, want3)[:-(4 + 4 + 4 + 10)], len(want3), -114, None),
        ("capacity_one_short", build_frame(three, True, want3), len(want3) - 1, -116, None),
        ("content_checksum_wrong", build_frame(three, True, want3, bad_content_cks=True), len(want3), -118, None),
        ("stored_block_is_history", build_frame([(a, True), (exact, False)]), len(want_exact), len(want_exact), want_exact),
        ("stored_block_too_large", build_frame([(blk0, False), (a, True)]), 599, -111, None),
    ]
    return cases
