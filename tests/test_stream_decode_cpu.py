"""StreamDecode (lz4.StreamDecode, src/lz4.zig:870-957) without a GPU: the restatement tools/pyref/zig_lz4_stream_decode.py
against the oracle and zig_lz4_dict.py, its bound rule and state machine, and the new entry points' surface."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "pyref"))
import datagen as dg  # noqa: E402
import dictgen  # noqa: E402
import zig_lz4_dict as pd  # noqa: E402
import zig_lz4_stream_decode as psd  # noqa: E402

NEW = ("zlz4_stream_decode_init", "zlz4_set_stream_decode", "zlz4_decompress_safe_continue",
       "zlz4_decoder_ring_buffer_size", "zlz4_batch_decompress_safe_continue_workspace",
       "zlz4_batch_decompress_safe_continue")


def _blocks(oracle):
    out = []
    for d in ("text", "mixed", "zero", "random", "ramp"):
        for b in dg.make_blocks(d, 2, 3000, seed=3):
            out.append((bytes(b), oracle.compress_default(bytes(b))))
    return out


def test_symbols_declared_exported_and_bound(zl):
    hdr = open(os.path.join(ROOT, "include", "zlz4_amd.h")).read()
    L = C.CDLL(zl.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(L, name) and name in zl.SYMBOLS, name
    assert "WARNING (a defect of the reference" in hdr
    root = open(os.path.join(ROOT, "zig-lz4_amd", "zig", "root.zig")).read()
    for name in ("StreamDecode", "createStreamDecode", "freeStreamDecode", "decoderRingBufferSize",
                 "decompressSafeContinueBatch"):
        assert re.search(r"pub (const|fn) %s\b" % name, root), name
    for name in ("setStreamDecode", "decompressSafeContinue", "pub fn create", "pub fn destroy", "pub fn init"):
        assert name in root, name
    hpp = open(os.path.join(ROOT, "zig-lz4_amd", "csrc", "host", "zlz4.hpp")).read()
    for name in ("StreamDecode", "decompressSafeContinue", "decoderRingBufferSize"):
        assert name in hpp, name
    for name in ("StreamDecode", "createStreamDecode", "freeStreamDecode", "decoderRingBufferSize",
                 "batch_decompress_safe_continue", "decompressStreams"):
        assert hasattr(zl, name), name


def test_decoder_ring_buffer_size(zl):
    for n in (0, 1, 4096, 65536, 4 << 20):
        exp = 0 if n == 0 else 65536 + 14 + n                  # src/lz4.zig:954-957
        assert zl.decoderRingBufferSize(n) == exp == psd.decoder_ring_buffer_size(n)


def test_mode_a_and_low_prefix_below_dst_equal_decompress_safe(oracle):
    blocks = _blocks(oracle)
    for raw, comp in blocks:
        for cap in (len(raw), len(raw) - 1, 17, 0):
            exp = oracle.decompress_safe(comp, cap)
            exp_r = exp if isinstance(exp, int) else len(exp)
            for lp in (0, -1, -5000):
                r, out = psd.decompress_generic(comp, cap, lp, None)
                assert r == (exp_r if not isinstance(exp, int) else exp)
                if r > 0:
                    assert out == exp
            sd = psd.StreamDecode()
            r, out = sd.decompress_safe_continue(comp, 1000, cap)        # mode A
            if r > 0:
                assert out == exp
            sd2 = psd.StreamDecode(0, 0, 1000 - 4096, 9)               # mode B, prefix below dst
            assert sd2.decompress_safe_continue(comp, 1000, cap)[0] == r


def test_dict_mode_equals_dict_pyref(tmp_path):
    enc = dictgen.encoder(tmp_path)
    dct = bytes(dg.make_blocks("text", 1, 70000, seed=8)[0])
    for i in range(6):
        raw = dct[3000 * i:3000 * i + 900] + dct[65000 + 200 * i:65000 + 200 * i + 700]
        comp, _ = enc(dct, raw)
        for cap in (len(raw), len(raw) - 3):
            sd = psd.StreamDecode()
            sd.set_stream_decode(1 << 40, dct)
            r, out = sd.decompress_safe_continue(comp, 1 << 30, cap)
            er, eb = pd.decompress_safe_using_dict(comp, cap, dct)
            assert r == er and (r <= 0 or out == eb)
            if r >= 0:
                assert sd.state() == (0, 0, 1 << 30, r)
            else:
                assert sd.state() == (1 << 40, len(dct), 0, 0)          # a failed call leaves it pending


def _first_match(comp):
    """(op, offset, ml) of the first match of a block."""
    ip, op = 0, 0
    while True:
        t = comp[ip]; ip += 1
        lit = t >> 4
        if lit == 15:
            while True:
                s = comp[ip]; ip += 1; lit += s
                if s != 255:
                    break
        ip += lit; op += lit
        off = comp[ip] | (comp[ip + 1] << 8); ip += 2
        ml = t & 15
        if ml == 15:
            while True:
                s = comp[ip]; ip += 1; ml += s
                if s != 255:
                    break
        return op, off, ml + 4


def test_bound_rule_edges(oracle):
    """A match at op with offset o passes iff op - o >= L = prefix - dst: checked at L and L + 1, and after the match's
    OutputTooSmall (:174)."""
    raw = b"abcdefgh" * 40 + bytes(range(200))
    comp = oracle.compress_default(raw)
    op, off, ml = _first_match(comp)
    L = op - off
    dst = 1 << 20
    r_ok, out = psd.StreamDecode(0, 0, dst + L, 5).decompress_safe_continue(comp, dst, len(raw))
    assert r_ok == len(raw) and out == raw
    r_bad, _ = psd.StreamDecode(0, 0, dst + L + 1, 5).decompress_safe_continue(comp, dst, len(raw))
    assert r_bad == psd.CORRUPTED
    # the same match without room for it: OutputTooSmall comes first
    r_small, _ = psd.StreamDecode(0, 0, dst + L + 1, 5).decompress_safe_continue(comp, dst, op + ml - 1)
    assert r_small == psd.OUTPUT_TOO_SMALL


def test_state_machine_walk(oracle):
    raw, comp = _blocks(oracle)[0]
    sd = psd.StreamDecode()
    sd.set_stream_decode(5000, b"D" * 100)
    assert sd.state() == (5000, 100, 0, 0)
    assert sd.decompress_safe_continue(b"\x1f", 1 << 20, 100)[0] == psd.CORRUPTED    # error: still pending
    assert sd.state() == (5000, 100, 0, 0)
    assert sd.decompress_safe_continue(b"", 1 << 20, 100) == (0, b"")                 # empty src consumes it
    assert sd.state() == (0, 0, 1 << 20, 0)
    assert sd.kind(1 << 21) == ("A",)                                                 # prefix_len 0: mode A
    sd.set_stream_decode(5000, b"D" * 100)
    assert sd.decompress_safe_continue(comp, 1 << 21, 0) == (0, b"")                  # capacity 0 consumes it too
    assert sd.state() == (0, 0, 1 << 21, 0)
    r, _ = sd.decompress_safe_continue(comp, 1 << 22, len(raw))                       # mode A
    assert r == len(raw) and sd.state() == (0, 0, 1 << 22, r)
    assert sd.kind((1 << 22) - 100) == ("bound", 100)
    sd.set_stream_decode(0, None)
    assert sd.state() == (0, 0, 0, 0)
    # mode A keeps a dictionary address of length 0
    sd = psd.StreamDecode(777, 0, 0, 0)
    sd.decompress_safe_continue(comp, 1 << 22, len(raw))
    assert sd.state() == (777, 0, 1 << 22, len(raw))
    # both a dictionary and a prefix: InvalidState, untouched
    sd = psd.StreamDecode(777, 10, 1 << 22, 0, b"x" * 10)
    assert sd.decompress_safe_continue(comp, 1 << 23, len(raw))[0] == psd.INVALID_STATE
    assert sd.state() == (777, 10, 1 << 22, 0)


def test_entry_points_without_device_or_trivially(zl):
    if zl.device_available():
        pytest.skip("a device is present: covered by tests/test_gpu_stream_decode.py")
    L = zl.lib()
    st = (C.c_uint64 * 4)(1, 2, 3, 4)
    L.zlz4_stream_decode_init(st)
    assert list(st) == [0, 0, 0, 0]
    buf = (C.c_uint8 * 16)()
    L.zlz4_set_stream_decode(st, buf, 16)
    assert list(st) == [C.addressof(buf), 16, 0, 0]
    L.zlz4_set_stream_decode(st, None, 16)
    assert list(st) == [0, 0, 0, 0]
    src = (C.c_uint8 * 4)(0x10, 65, 0, 0)
    out = (C.c_uint8 * 64)()
    assert L.zlz4_decompress_safe_continue(st, src, 2, out, 64) == zl.ERR_DEVICE
    assert list(st) == [0, 0, 0, 0]
    assert L.zlz4_decompress_safe_continue(None, src, 2, out, 64) == -5
    # trivial calls decide on the host: empty src is a success and records the prefix
    assert L.zlz4_decompress_safe_continue(st, src, 0, out, 64) == 0
    assert list(st) == [0, 0, C.addressof(out), 0]
    # both a dictionary and a prefix
    bad = (C.c_uint64 * 4)(C.addressof(buf), 16, C.addressof(out), 0)
    assert L.zlz4_decompress_safe_continue(bad, src, 2, out, 64) == -5
    assert list(bad) == [C.addressof(buf), 16, C.addressof(out), 0]
    ws = L.zlz4_batch_decompress_safe_continue_workspace(100, 10)
    assert ws >= 100 * 32
    wsb = (C.c_uint8 * (ws + 16))()
    wsp = (C.addressof(wsb) + 15) & ~15
    rs = (C.c_uint32 * 11)()
    sts = (C.c_uint64 * 40)()
    res = (C.c_int64 * 100)()
    args = [None, None, None, None, None, None, None, rs, sts, res, 100, 10]
    assert L.zlz4_batch_decompress_safe_continue(*args, wsp, ws) == zl.ERR_DEVICE
    assert L.zlz4_batch_decompress_safe_continue(*args, wsp, ws - 1) == -5          # workspace too small
    assert L.zlz4_batch_decompress_safe_continue(*args, wsp + 8, ws) == -5          # misaligned
    assert L.zlz4_batch_decompress_safe_continue(*args, None, ws) == -5
    with pytest.raises(zl.Lz4Error) as e:
        zl.StreamDecode().decompressSafeContinue(b"\x10A", np.zeros(8, np.uint8))
    assert e.value.code == zl.ERR_DEVICE
