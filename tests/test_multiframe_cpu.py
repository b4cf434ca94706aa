"""Multiframe buffers without a GPU: the split model of tests/multiframegen.py against liblz4 (looping LZ4F_decompress over
a buffer consumes exactly the model's member boundaries and gives the model's bytes), the model's own edge table, and
the refusals of the host calls that come before the device check."""
import ctypes as C

import pytest

import dictframegen
import multiframegen as g


def _liblz4_loop(buf):
    """LZ4F_decompress over `buf`, frame after frame -> ([end of every frame it completed], bytes)"""
    lib = C.CDLL("liblz4.so.1")
    SZ, VP = C.c_size_t, C.c_void_p
    lib.LZ4F_isError.restype, lib.LZ4F_isError.argtypes = C.c_uint, [SZ]
    lib.LZ4F_createDecompressionContext.restype, lib.LZ4F_createDecompressionContext.argtypes = SZ, [C.POINTER(VP), C.c_uint]
    lib.LZ4F_freeDecompressionContext.restype, lib.LZ4F_freeDecompressionContext.argtypes = SZ, [VP]
    lib.LZ4F_decompress.restype = SZ
    lib.LZ4F_decompress.argtypes = [VP, VP, C.POINTER(SZ), VP, C.POINTER(SZ), VP]
    ctx = VP()
    assert not lib.LZ4F_isError(lib.LZ4F_createDecompressionContext(C.byref(ctx), 100))
    try:
        src = (C.c_uint8 * max(1, len(buf))).from_buffer_copy(buf or b"\0")
        cap = 1 << 20
        out = (C.c_uint8 * cap)()
        ends, got, sp = [], bytearray(), 0
        while sp < len(buf):
            ss, ds = C.c_size_t(len(buf) - sp), C.c_size_t(cap)
            r = lib.LZ4F_decompress(ctx, C.addressof(out), C.byref(ds), C.addressof(src) + sp, C.byref(ss), None)
            assert not lib.LZ4F_isError(r), "liblz4 refuses the buffer at %d" % sp
            assert ss.value or ds.value, "liblz4 makes no progress at %d" % sp
            sp += ss.value
            got += bytes(out[:ds.value])
            if r == 0:
                ends.append(sp)
        return ends, bytes(got)
    finally:
        lib.LZ4F_freeDecompressionContext(ctx)


def _valid_buffers():
    c = g.few()
    sk = [g.skippable(k, b"s" * n) for k, n in ((0, 0), (7, 1), (15, 65536), (9, 70000))]
    yield "one", c[3].frame
    yield "two", c[1].frame + c[6].frame
    yield "three", c[0].frame + c[5].frame + c[7].frame
    yield "five", b"".join(x.frame for x in c[:5])
    yield "skip_front_between_last", sk[1] + c[2].frame + sk[2] + c[4].frame + sk[0]
    yield "two_skips_in_a_row", c[1].frame + sk[3] + sk[0] + c[0].frame
    yield "only_skips", sk[0] + sk[1]
    yield "empty", b""


@pytest.mark.parametrize("name,buf", list(_valid_buffers()), ids=[n for n, _ in _valid_buffers()])
def test_model_against_liblz4(name, buf):
    if dictframegen.liblz4fd() is None:
        pytest.skip("liblz4 does not load")
    members = g.split(buf)
    assert not any(m.last for m in members)
    ends, data = _liblz4_loop(buf)
    assert ends == [m.pos + m.len for m in members]
    result, want, items = g.expected(buf)
    assert (result, want) == (len(data), data)


def test_model_edge_table():
    c = g.few()
    a, b = c[4], c[1]
    assert g.split(b"") == []
    assert g.table(a.frame) == [(0, len(a.frame), g.FRAME, 0)] and g.split(a.frame)[0].nb == 2
    assert [m.nb for m in g.split(b"".join(x.frame for x in c))] == [0, 1, 1, 1, 2, 4, 4, 2]
    for k in range(16):
        assert g.table(g.skippable(k, b"abc") + a.frame) == [(0, 11, g.SKIPPABLE, k), (11, len(a.frame), g.FRAME, 0)]
    # whatever cannot be delimited is the last member and reaches to the end
    for tail, rest in ((b"\x01", b.frame), (b"\x01" * 7, b.frame), (g.skippable(2)[:4], b""), (g.skippable(2)[:7], b""),
                       (g.skippable(2, b"abcd")[:-1], b""), (a.frame[:-1], b""), (a.frame[:-5], b""), (a.frame[:30], b.frame),
                       (b"\x02\x21\x4c\x18" + b"z" * 20, b.frame)):
        t = g.split(a.frame + tail + rest)
        assert len(t) == 2 and t[1].last and t[1].pos + t[1].len == len(a.frame + tail + rest), tail[:8]
    # (the split never judges: the bytes that follow a torn member complete it where they can)
    assert [m.last for m in g.split(a.frame[:-1] + b.frame)] == [False, True]
    assert g.split(g.skippable(2)[:7])[0].kind == g.SKIPPABLE_TRUNCATED
    assert g.table(g.skippable(2, b"abcd")[:-1]) == [(0, 11, g.SKIPPABLE_TRUNCATED, 2)]
    # the stated codes of the defects are the model's
    for name, buf, code, front in g.defects():
        result, data, items = g.expected(buf)
        assert result == code and data is None, name
        assert all(r is None or r >= 0 for r in items[:front]) and len(items) > front, name
        bad = items[front]
        assert (bad is None and g.split(buf)[front].kind == g.SKIPPABLE_TRUNCATED) or bad == code, name
    # a chain that merely lacks its end mark at the end of the buffer keeps its content
    plain = g.pick("text65536_bc0_cc0_cs0")[0]
    assert g.expected(plain.frame[:-4])[:2] == (65536, plain.content)
    assert g.expected(a.frame[:-4])[0] == g.SIZE_WRONG                # the content checksum word is missing
    # linked members need the flag
    frame, data = g.linked()[0]
    assert g.expected(b.frame + frame)[0] == g.FAILED
    assert g.expected(b.frame + frame, g.DECODE_LINKED)[:2] == (len(b.content) + len(data), b.content + data)


def test_host_refusals_come_before_the_device_check(zl):
    L = zl.lib()
    frame = g.few()[1].frame
    src = (C.c_uint8 * len(frame)).from_buffer_copy(frame)
    dst = (C.c_uint8 * 64)()
    for flags in (2, 4, 0x80000000, 3):
        assert L.zlz4f_multiframe_decompressed_size(C.addressof(src), len(frame), flags) == g.PARAMETER_INVALID
        assert L.zlz4f_decompress_multiframe(C.addressof(src), len(frame), C.addressof(dst), 64, flags) == g.PARAMETER_INVALID
        assert L.zlz4f_decompress_multiframe(None, 5, None, 5, flags) == g.PARAMETER_INVALID   # the flags come first
    assert L.zlz4f_multiframe_decompressed_size(None, 5, 0) == g.INVALID_STATE
    assert L.zlz4f_decompress_multiframe(None, 5, C.addressof(dst), 64, 1) == g.INVALID_STATE
    assert L.zlz4f_decompress_multiframe(C.addressof(src), len(frame), None, 64, 0) == g.INVALID_STATE
    with pytest.raises(zl.Lz4Error):
        zl.lz4f.decompressMultiframes([frame], flags=2, device="cpu")
