"""Test-side helpers for the dictionary decoder (tests/test_dict_*.py, tools/time_dict_decompress.py).

* `encoder(dirpath)`: compiles tests/dict_encoder.c with cc into `dirpath` and returns a callable
  encode(dict, block) -> (stream, stats) -- valid LZ4 blocks whose matches may reach into the dictionary.
* `liblz4()`: the system liblz4 (LZ4_decompress_safe_usingDict) if it loads, else None -- an optional cross-check.
* `crafted_cases()`: hand-made streams for the edge cases of the dict branch (src/lz4.zig:181-225).
"""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def encoder(dirpath):
    so = os.path.join(str(dirpath), "libdict_encoder.so")
    if not os.path.exists(so):
        subprocess.check_call(["cc", "-O2", "-std=c11", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "dict_encoder.c")])
    lib = C.CDLL(so)
    lib.dict_encode.restype = C.c_int64
    lib.dict_encode.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                C.POINTER(C.c_uint64)]

    def encode(dict_bytes, block):
        d = (C.c_uint8 * max(1, len(dict_bytes))).from_buffer_copy(dict_bytes or b"\0")
        s = (C.c_uint8 * max(1, len(block))).from_buffer_copy(block or b"\0")
        cap = len(block) + len(block) // 255 + 16
        o = (C.c_uint8 * cap)()
        st = (C.c_uint64 * 4)()
        r = lib.dict_encode(C.addressof(d), len(dict_bytes), C.addressof(s), len(block), C.addressof(o), cap, st)
        assert r >= 0, "dict_encode failed"
        return bytes(o[:r]), tuple(st)
    return encode


def liblz4():
    try:
        lib = C.CDLL("liblz4.so.1")
        fn = lib.LZ4_decompress_safe_usingDict
    except (OSError, AttributeError):
        return None
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]

    def decode(src, cap, dict_bytes):
        """-> decoded bytes, or None when liblz4 reports an error"""
        s = (C.c_uint8 * max(1, len(src))).from_buffer_copy(src or b"\0")
        d = (C.c_uint8 * max(1, len(dict_bytes))).from_buffer_copy(dict_bytes or b"\0")
        o = (C.c_uint8 * max(1, cap))()
        r = fn(C.addressof(s), C.addressof(o), len(src), cap, C.addressof(d), len(dict_bytes))
        return bytes(o[:r]) if r >= 0 else None
    decode.fn = fn
    decode.lib = lib
    return decode


def _len_ext(v):
    out = bytearray()
    while v >= 255:
        out.append(255)
        v -= 255
    out.append(v)
    return bytes(out)


def seq(lit, off=None, ml=None):
    """one sequence: literals `lit`, then (unless off is None) a match of length ml at offset off"""
    ln = len(lit)
    mc = 0 if off is None else ml - 4
    tok = (min(ln, 15) << 4) | min(mc, 15)
    out = bytes([tok]) + (_len_ext(ln - 15) if ln >= 15 else b"") + bytes(lit)
    if off is not None:
        out += bytes([off & 255, off >> 8]) + (_len_ext(mc - 15) if mc >= 15 else b"")
    return out


def pattern(n, seed=1):
    """n bytes without short repeats (so that crafted offsets decide what is copied)"""
    import random
    r = random.Random(seed)
    return bytes(r.randrange(256) for _ in range(n))


def crafted_cases():
    """-> list of (name, stream, dict, dst_cap, target); target None = the full call"""
    cases = []
    tail = b"ENDOFBLOCKLITS"
    for dl in (0, 1, 3, 4, 65535, 65536, 65537, 200000):
        dct = pattern(dl, seed=dl)
        lit = b"0123456789"
        # offset == op + dict.len (the dictionary's first byte, valid) and op + dict.len + 1 (:190, CorruptedData)
        for extra, name in ((0, "first"), (1, "beyond")):
            off = len(lit) + dl + extra
            if 0 < off <= 65535:
                cases.append(("dl%d_%s" % (dl, name), seq(lit, off, 4) + seq(tail), dct, 64, None))
        # a dict match ending exactly at the dictionary's end (offset = op + ml) and one of 40 bytes (long path)
        for ml in (4, 7, 16, 18, 40, 300):
            if ml <= dl:
                cases.append(("dl%d_end_ml%d" % (dl, ml), seq(lit, len(lit) + ml, ml) + seq(tail), dct, 400, None))
        # spanning matches: 2 dict bytes then in-block (offset < ml: periodic), and a long one with restSize > offset
        if dl >= 3:
            cases.append(("dl%d_span_short" % dl, seq(lit, len(lit) + 2, 9) + seq(tail), dct, 64, None))
            cases.append(("dl%d_span_long" % dl, seq(lit, len(lit) + 3, 200) + seq(tail), dct, 300, None))
            cases.append(("dl%d_span_rle" % dl, seq(b"", 1, 50) + seq(tail), dct, 80, None))
        # a match reaching the largest offset, far into a big dictionary
        if dl >= 65535 - 20:
            cases.append(("dl%d_off65535" % dl, seq(lit, 65535, 20) + seq(tail), dct, 64, None))
        # OutputTooSmall (:174) wins over CorruptedData (:190) when both apply
        cases.append(("dl%d_ots_over_corrupt" % dl, seq(lit, len(lit) + dl + 1 if len(lit) + dl + 1 <= 65535 else 65535, 40)
                      + seq(tail), dct, len(lit) + 10, None))
        # partial decoding: target cuts inside a dictionary match, target == 0
        if dl >= 40:
            s = seq(lit, len(lit) + 40, 30) + seq(lit, 5, 20) + seq(tail)
            for t in (0, 5, len(lit), len(lit) + 1, len(lit) + 17, len(lit) + 30, 200):
                cases.append(("dl%d_partial%d" % (dl, t), s, dct, 200, t))
            cases.append(("dl%d_cap0" % dl, s, dct, 0, None))
            cases.append(("dl%d_src0" % dl, b"", dct, 64, None))
            cases.append(("dl%d_trunc" % dl, s[:len(s) - len(tail) - 3], dct, 200, None))
    return cases


def run_batch(zl, items, caps, dicts, dict_index, dev, layout=None):
    """zlz4_batch_decompress_safe_using_dict on one batch: block i decodes items[i] into a slot of capacity caps[i]
    with the dictionary dicts[dict_index[i]] (dicts are stored once each: equal indices share one copy).  Checks that
    no slot is written past its capacity and that the input and dictionary arenas are unchanged.  `layout`
    (gpu_harness.Packed) packs the streams, the dictionaries and the output slots at unaligned offsets.
    -> [(result, bytes)]"""
    import numpy as np
    import torch
    import gpu_harness as gh
    buf, offs, lens = gh._pack(items, layout=layout)
    dbuf, doffs, dlens = gh._pack(dicts, layout=layout)
    caps = np.asarray(caps, dtype=np.int64)
    out_offs, guard_ends, total = gh._out_slots(caps, layout)
    idx = np.asarray(dict_index, dtype=np.int64)
    d_in = torch.from_numpy(buf).to(dev)
    d_dict = torch.from_numpy(dbuf).to(dev)
    d_out = torch.full((total,), 0xA5, dtype=torch.uint8, device=dev)
    res = torch.full((len(items),), -999, dtype=torch.int64, device=dev)
    u32 = lambda a: torch.from_numpy(np.asarray(a).astype(np.uint32).view(np.int32)).to(dev)
    zl.batch_decompress_safe_using_dict(d_in, torch.from_numpy(offs).to(dev), u32(lens), d_out,
                                        torch.from_numpy(out_offs).to(dev), u32(caps), d_dict,
                                        torch.from_numpy(doffs[idx]).to(dev), u32(dlens[idx]), res)
    torch.cuda.synchronize()
    assert (d_dict.cpu().numpy() == dbuf).all(), "the dictionary arena changed"
    assert (d_in.cpu().numpy() == buf).all(), "the input arena changed"
    return gh._collect(res, d_out, out_offs, guard_ends, caps)
