"""The host-pointer entry points called directly (zl.lib()), with a destination that is larger than the capacity they
are told: a call writes dst[0:result) and nothing else, and a call that fails writes nothing.  The Python wrappers hand
the library a buffer of exactly `cap` bytes, so they cannot see either.  Results, bytes and error codes are the
wrappers' own; the decoders' bytes are also the plaintext.  One 4096-byte record of text, the 1024 bytes in front of
it as dictionary.  Run on the GPU box: pytest -m gpu."""
import ctypes as C

import numpy as np
import pytest

import datagen as dg

pytestmark = pytest.mark.gpu

FILL, PAD = 0xA5, 64
N, D = 4096, 1024


class _SdState(C.Structure):
    _fields_ = [("dict", C.c_uint64), ("dict_len", C.c_uint64), ("prefix", C.c_uint64), ("prefix_len", C.c_uint64)]


def _src(b):
    a = np.frombuffer(bytes(b), dtype=np.uint8)
    return a, C.c_void_p(a.ctypes.data), a.size


def _ptr(a, off=0):
    return C.c_void_p(a.ctypes.data + off)


class Case:
    """call(a, cap) -> the entry point's return value, a = the uint8 destination array (cap + PAD bytes of FILL);
    wrapper(cap) -> the Python wrapper's bytes for the same call, or its Lz4Error; cap = a sufficient capacity;
    short(result) = the capacity that is one byte short; plain = what a decoder must produce"""

    def __init__(self, call, wrapper, cap, short, plain=None):
        self.call, self.wrapper, self.cap, self.short, self.plain = call, wrapper, cap, short, plain
        self.side = {}                                # what a call / a wrapper leaves beside dst (the stream's table)


NAMES = ("compress_fast", "compress_hc", "decompress_safe", "decompress_safe_using_dict", "decompress_safe_continue",
         "stream_compress_fast_continue", "compress_fast_using_dict", "compress_hc_using_dict", "compress_frame",
         "compress_frame_ex_linked", "decompress_frame", "decompress_frame_ex_linked")


@pytest.fixture(scope="module")
def cases(zl, gpu):
    L = zl.lib()
    text = bytes(dg.text_bytes(D + N, 1601))
    dic, rec = text[:D], text[D:]
    keep_d, pd, nd = _src(dic)
    keep_r, pr, nr = _src(rec)
    bound = zl.compressBound(N)
    fbound = zl.lz4f.compressFrameBound(N)
    LINK, LINKED = zl.lz4f.BATCH_LINK_BLOCKS, zl.lz4f.DECODE_LINKED
    result_short, bound_short, n_short = (lambda r: r - 1), (lambda r: fbound - 1), (lambda r: N - 1)
    out = {"_keep": [keep_d, keep_r]}

    def compressor(name, fn, wrapper, cap=bound, short=result_short):
        out[name] = Case(lambda a, cap: fn(pr, nr, _ptr(a), cap), wrapper, cap, short)

    def decoder(name, block, fn, wrapper):
        keep, pb, nb = _src(block)
        out["_keep"].append(keep)
        out[name] = Case(lambda a, cap: fn(pb, nb, _ptr(a), cap), wrapper, N + 32, n_short, plain=rec)

    compressor("compress_fast", lambda s, n, d, c: L.zlz4_compress_fast(s, n, d, c, 1), lambda cap: zl.compressFast(rec, 1, cap))
    compressor("compress_hc", lambda s, n, d, c: L.zlz4_compress_hc(s, n, d, c, 9), lambda cap: zl.compressHC(rec, 9, cap))
    compressor("compress_fast_using_dict", lambda s, n, d, c: L.zlz4_compress_fast_using_dict(s, n, d, c, pd, nd, 1),
               lambda cap: zl.compressFastUsingDict(rec, dic, 1, cap))
    compressor("compress_hc_using_dict", lambda s, n, d, c: L.zlz4_compress_hc_using_dict(s, n, d, c, pd, nd, 9),
               lambda cap: zl.compressHCUsingDict(rec, dic, 9, cap))
    compressor("compress_frame", lambda s, n, d, c: L.zlz4f_compress_frame(s, n, d, c, None),
               lambda cap: zl.lz4f.compressFrame(rec, None, cap), fbound, bound_short)
    compressor("compress_frame_ex_linked", lambda s, n, d, c: L.zlz4f_compress_frame_ex(s, n, d, c, None, LINK),
               lambda cap: zl.lz4f.compressFrame(rec, None, cap, LINK), fbound, bound_short)

    block = zl.compressDefault(rec)
    decoder("decompress_safe", block, L.zlz4_decompress_safe, lambda cap: zl.decompressSafe(block, cap))
    with_dict = zl.compressFastUsingDict(rec, dic)
    decoder("decompress_safe_using_dict", with_dict, lambda s, n, d, c: L.zlz4_decompress_safe_using_dict(s, n, d, c, pd, nd),
            lambda cap: zl.decompressSafeUsingDict(with_dict, cap, dic))
    frame = zl.lz4f.compressFrame(rec)
    decoder("decompress_frame", frame, L.zlz4f_decompress_frame, lambda cap: zl.lz4f.decompressFrame(frame, cap))
    linked = zl.lz4f.compressFrame(rec, None, None, LINK)
    decoder("decompress_frame_ex_linked", linked, lambda s, n, d, c: L.zlz4f_decompress_frame_ex(s, n, d, c, LINKED),
            lambda cap: zl.lz4f.decompressFrame(linked, cap, LINKED))

    # StreamDecode: the first call leaves its 64 bytes one byte above dst, so the second call decodes with the bound
    # prefix - dst = 1 (DecompressBound): only a match that reaches output position 0 fails, and 0xFF never repeats
    first_plain, second_plain = rec[:64], b"\xff" + rec[:N - 1]
    first, second = zl.compressDefault(first_plain), zl.compressDefault(second_plain)
    keep_1, p1, n1 = _src(first)
    keep_2, p2, n2 = _src(second)
    out["_keep"] += [keep_1, keep_2]

    def continue_call(a, cap):
        st = _SdState()
        L.zlz4_stream_decode_init(C.byref(st))
        assert L.zlz4_decompress_safe_continue(C.byref(st), p1, n1, _ptr(a, 1), 64) == 64
        assert bytes(a[1:65]) == first_plain and st.prefix == a.ctypes.data + 1
        a[:] = FILL
        return L.zlz4_decompress_safe_continue(C.byref(st), p2, n2, _ptr(a), cap)

    def continue_wrapper(cap):
        b = np.zeros(cap + PAD, dtype=np.uint8)
        sd = zl.StreamDecode()
        assert sd.decompressSafeContinue(first, b[1:65]) == 64
        r = sd.decompressSafeContinue(second, b[:cap])
        return bytes(b[:r])

    out["decompress_safe_continue"] = Case(continue_call, continue_wrapper, N + 32, n_short, plain=second_plain)

    # Stream.compressFastContinue from the table loadDict(dic) leaves; the table comes back on every exit
    loaded = zl.Stream()
    loaded.loadDict(dic)
    stream_case = Case(None, None, bound, result_short)

    def stream_call(a, cap):
        table = loaded.hashTable.copy()
        r = L.zlz4_stream_compress_fast_continue(_ptr(table), pr, nr, _ptr(a), cap, 1)
        stream_case.side["call"] = table
        return r

    def stream_wrapper(cap):
        s = zl.Stream()
        s.hashTable[:] = loaded.hashTable
        try:
            return s.compressFastContinue(rec, 1, cap)
        finally:
            stream_case.side["wrapper"] = s.hashTable.copy()

    stream_case.call, stream_case.wrapper = stream_call, stream_wrapper
    out["stream_compress_fast_continue"] = stream_case
    return out


def _dst(cap):
    return np.full(cap + PAD, FILL, dtype=np.uint8)


@pytest.mark.parametrize("name", NAMES)
def test_sufficient_capacity_writes_result_bytes_only(zl, cases, name):
    c = cases[name]
    want = c.wrapper(c.cap)
    a = _dst(c.cap)
    r = c.call(a, c.cap)
    print("%s: cap %d -> %d" % (name, c.cap, r))
    assert r == len(want) and 0 < r <= c.cap
    assert bytes(a[:r]) == want
    if c.plain is not None:
        assert want == c.plain
    assert (a[r:] == FILL).all(), "%s wrote past its result" % name
    if c.side:
        assert (c.side["call"] == c.side["wrapper"]).all(), "%s: the table differs from the wrapper's" % name


@pytest.mark.parametrize("name", NAMES)
def test_capacity_one_byte_short_writes_nothing(zl, cases, name):
    c = cases[name]
    short = c.short(len(c.wrapper(c.cap)))
    with pytest.raises(zl.Lz4Error) as e:
        c.wrapper(short)
    a = _dst(short)
    r = c.call(a, short)
    print("%s: cap %d -> %d (%s)" % (name, short, r, zl.error_name(r)))
    assert r == e.value.code and r < 0
    assert (a == FILL).all(), "%s wrote to dst on an error exit" % name
    if c.side:
        assert (c.side["call"] == c.side["wrapper"]).all(), "%s: the table differs from the wrapper's" % name


def test_compress_dest_size_fits_its_capacity(zl, gpu):
    """no failing capacity: cap = 1000 takes the search branch (the batch pipeline as a batch of one)"""
    rec = bytes(dg.text_bytes(D + N, 1601))[D:]
    want, want_consumed = zl.compressDestSize(rec, 1000)
    keep, pr, nr = _src(rec)
    a = _dst(1000)
    ss = C.c_size_t(nr)
    r = zl.lib().zlz4_compress_dest_size(pr, _ptr(a), 1000, C.byref(ss))
    print("compress_dest_size: cap 1000 -> %d, consumed %d" % (r, ss.value))
    assert r == len(want) and 0 < r <= 1000 and ss.value == want_consumed and 0 < want_consumed < N
    assert bytes(a[:r]) == want
    assert (a[r:] == FILL).all(), "compress_dest_size wrote past its result"
