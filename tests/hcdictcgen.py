"""Test-side helpers for the HC dictionary compressor (tests/test_hc_dict_cpu.py, tests/test_gpu_hc_dict.py,
tools/time_hc_dict_compress.py).

* `ref(dirpath)`: compiles tests/hc_dict_ref.c with cc into `dirpath` and returns its ctypes handle with
  compress(src, dict, level, cap) -> (result, bytes) and batch(...) (the C restatement of zlz4_compress_hc_using_dict,
  the checker of the GPU tests).
* `run_batch(zl, ...)`: one zlz4_batch_compress_hc_using_dict call on packed records and dictionaries with 0xA5 guard
  bands; checks that the input and dictionary arenas are unchanged and that InvalidState wrote nothing.
* `sequences(stream)`: the (literal length, match length, offset) triples of a block.
* `crafted()`: the edge cases of the dictionary reach, each with what it is about.
"""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
INVALID_STATE, OUTPUT_TOO_SMALL, UNSUPPORTED = -5, -1, -8
SRC = os.path.join(HERE, "hc_dict_ref.c")


def bound(n):
    return n + n // 255 + 16                          # compressBound, src/lz4.zig:80-83


def _cbuf(b):
    return (C.c_uint8 * max(1, len(b))).from_buffer_copy(bytes(b) or b"\0")


class Ref:
    def __init__(self, so):
        L = C.CDLL(so)
        L.hd_compress.restype = C.c_int64
        L.hd_compress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int]
        L.hd_compress_batch.restype = C.c_int32
        L.hd_compress_batch.argtypes = [C.c_void_p] * 10 + [C.c_uint32] * 3 + [C.c_int]
        self.L = L

    def compress(self, src, dict_bytes, level, cap=None):
        """-> (result, bytes); dict_bytes None = the null dictionary"""
        src = bytes(src)
        cap = bound(len(src)) if cap is None else cap
        s, o = _cbuf(src), (C.c_uint8 * max(1, cap))()
        d = None if dict_bytes is None else _cbuf(dict_bytes)
        r = self.L.hd_compress(C.addressof(s), len(src), C.addressof(o), cap, None if d is None else C.addressof(d),
                               0 if dict_bytes is None else len(dict_bytes), level)
        return r, (bytes(o[:r]) if r > 0 else b"")

    def batch(self, buf, offs, lens, caps, dbuf, doffs, dlens, max_in, max_dict, level):
        """The batch on packed arenas (numpy) -> (call status, results int64[n], outputs list of bytes)"""
        n = len(lens)
        caps = np.asarray(caps, dtype=np.uint32)
        out_offs = np.zeros(n, dtype=np.uint64)
        out_offs[1:] = np.cumsum(caps.astype(np.uint64))[:-1]
        out = np.zeros(max(1, int(caps.astype(np.uint64).sum())), dtype=np.uint8)
        res = np.full(n, -999, dtype=np.int64)
        a = [np.ascontiguousarray(buf), np.asarray(offs).astype(np.uint64), np.asarray(lens).astype(np.uint32),
             np.ascontiguousarray(dbuf), np.asarray(doffs).astype(np.uint64), np.asarray(dlens).astype(np.uint32)]
        rc = self.L.hd_compress_batch(a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, out.ctypes.data,
                                      out_offs.ctypes.data, caps.ctypes.data, a[3].ctypes.data, a[4].ctypes.data,
                                      a[5].ctypes.data, res.ctypes.data, n, max_in, max_dict, level)
        return rc, res, [bytes(out[int(o):int(o) + int(r)]) if r > 0 else b"" for o, r in zip(out_offs, res)]


def ref(dirpath):
    so = os.path.join(str(dirpath), "libhc_dict_ref.so")
    if not os.path.exists(so):
        subprocess.check_call(["cc", "-O2", "-std=c11", "-fPIC", "-shared", "-o", so, SRC])
    return Ref(so)


def _t32(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.uint32)).view(np.int32)).to(dev)


def run_batch(zl, cref, records, caps, dicts, dict_index, dev, level, layout=None, max_in=None, max_dict=None,
              in_input=None, workspace=None):
    """Record i is compressed into a slot of caps[i] bytes against dicts[dict_index[i]] (each dictionary is stored once).
    in_input: list of (offset, length) per block -- dictionaries taken from the INPUT arena (d_dict = d_in; dicts /
    dict_index are ignored).  layout: gpu_harness.Packed.  workspace: a uint8 tensor to use (default: the size the
    workspace function gives).  -> (gpu [(result, bytes)], ref [(result, bytes)])"""
    import torch
    import gpu_harness as gh
    n = len(records)
    buf, offs, lens = gh._pack(records, layout=layout)
    caps = np.asarray(caps, dtype=np.int64)
    out_offs, guard_ends, total = gh._out_slots(caps, layout)
    d_in = torch.from_numpy(buf).to(dev)
    if in_input is None:
        dbuf, doffs, dlens = gh._pack(dicts, layout=layout)
        idx = np.asarray(dict_index, dtype=np.int64)
        d_dict = torch.from_numpy(dbuf).to(dev)
        b_doff, b_dlen = doffs[idx], dlens[idx]
    else:
        dbuf, d_dict = buf, d_in
        b_doff = np.asarray([o for o, _ in in_input], dtype=np.int64)
        b_dlen = np.asarray([k for _, k in in_input], dtype=np.int64)
    d_out = torch.full((total,), 0xA5, dtype=torch.uint8, device=dev)
    res = torch.full((n,), -999, dtype=torch.int64, device=dev)
    max_in = (int(lens.max()) if n else 0) if max_in is None else max_in
    max_dict = (int(min(b_dlen.max(), 65536)) if n else 0) if max_dict is None else max_dict
    if workspace is None:
        workspace = torch.empty(max(16, zl.batch_compress_hc_using_dict_workspace(n, max_in, max_dict)), dtype=torch.uint8,
                                device=dev)
    zl.batch_compress_hc_using_dict(d_in, torch.from_numpy(offs).to(dev), _t32(lens, dev), d_out,
                                    torch.from_numpy(out_offs).to(dev), _t32(caps, dev), d_dict,
                                    torch.from_numpy(b_doff).to(dev), _t32(b_dlen, dev), res, max_in, max_dict, level,
                                    workspace)
    torch.cuda.synchronize()
    assert (d_in.cpu().numpy() == buf).all(), "the input arena changed"
    assert (d_dict.cpu().numpy() == dbuf).all(), "the dictionary arena changed"
    got = gh._collect(res, d_out, out_offs, guard_ends, caps)
    o = d_out.cpu().numpy()
    for i, (r, _) in enumerate(got):                  # InvalidState writes nothing
        if r == INVALID_STATE:
            assert (o[out_offs[i]:out_offs[i] + int(caps[i])] == 0xA5).all(), "block %d wrote into its slot" % i
    rc, rres, routs = cref.batch(buf, offs, lens, caps, dbuf, b_doff, b_dlen, max_in, max_dict, level)
    assert rc == 0
    return got, list(zip([int(r) for r in rres], routs))


def check(got, want, tag=""):
    """byte and status equality; a failed block's slot contents are unspecified"""
    assert len(got) == len(want)
    for i, ((g, gb), (w, wb)) in enumerate(zip(got, want)):
        assert g == w, "%s block %d: result %d, restatement %d" % (tag, i, g, w)
        if w > 0:
            assert gb == wb, "%s block %d: bytes differ" % (tag, i)


def sequences(stream):
    """-> [(output position of the match, literal length, match length, offset)] of an LZ4 block (the last literals have
    no entry)"""
    out, ip, op, n = [], 0, 0, len(stream)
    while ip < n:
        tok = stream[ip]
        ip += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                b = stream[ip]
                ip += 1
                lit += b
                if b != 255:
                    break
        ip += lit
        op += lit
        if ip >= n:
            break
        off = stream[ip] | stream[ip + 1] << 8
        ip += 2
        ml = tok & 15
        if ml == 15:
            while True:
                b = stream[ip]
                ip += 1
                ml += b
                if b != 255:
                    break
        ml += 4
        out.append((op, lit, ml, off))
        op += ml
    return out


def crafted():
    """-> [(name, dictionary, record)]"""
    import datagen as dg
    rnd = lambda n, s: bytes(dg.random_bytes(n, s))
    out = []
    d1 = rnd(65536, 1)
    out.append(("equals_tail_4k", d1, d1[-4096:]))
    per = b"abcdefg" * 40
    out.append(("period_7_from_dict", rnd(500, 3) + per[:75], (per * 30)[75:75 + 3000] + rnd(40, 4)))
    out.append(("period_1_from_dict_64k", b"a" * 65536, b"a" * 5000 + rnd(100, 16) + b"a" * 100))
    out.append(("period_1_from_dict_9", b"a" * 9, b"a" * 300 + rnd(20, 17)))
    # record byte j pairs with tail byte j + 1 at offset 65535; one byte further back (offset 65536) is out of range
    d = rnd(300, 7) + bytes(65536 - 300)
    out.append(("offset_65535_only", d, rnd(19, 8) + d[20:80] + rnd(30, 9)))
    out.append(("offset_65536_none", d, rnd(20, 10) + d[20:80] + rnd(30, 11)))
    G = b"\x01\xfe\x02\xfd"
    clean = lambda b: b.replace(b"\x01", b"\x03")     # no other 4-gram starts like G
    body = clean(rnd(96, 13))
    rec = clean(rnd(30, 14)) + G + clean(rnd(30, 15))
    out.append(("only_at_v_pos_0", G + body, rec))
    out.append(("at_v_pos_1", b"\x07" + G + body, rec))
    x = rnd(300, 18)
    out.append(("first_byte_starts_match", x, x[100:170] + rnd(20, 19)))
    out.append(("match_ends_at_dict_end", x, x[-40:] + rnd(40, 20)))
    out.append(("match_spans_dict_end", x, x[-40:] + x[-40:] + rnd(40, 21)))
    out.append(("thirteen_bytes", x, x[50:63]))
    out += [(name, d, r) for name, d, r, _ in traced()]
    return out


def traced():
    """-> [(name, dictionary, record, level)]: the two hand traces of tests/golden/gen_hc_dict_kat.py that need more than
    a few bytes (the attempt budget and the pattern step)"""
    # Attempt budget (level 3: four attempts).  The record starts with K = "QRST" + 12 bytes that continue as in the
    # dictionary's ONE long occurrence; between that occurrence and the record lie five occurrences of "QRST" followed by
    # other bytes -- one more at the dictionary's end and four at the head of the record's own prefix.  The chain from
    # the search position visits the nearest first: four short candidates (length 4) use up the attempts, the long
    # dictionary candidate is never compared.  At level 4 (eight attempts) it is.
    long_occ = b"QRSTlong-match-in-dict!"
    shorts = b"".join(b"QRST" + bytes([0x80 + k]) * 3 for k in range(4))
    dict_a = b"\x90" * 7 + long_occ + b"\x91" * 30 + b"QRST\x92\x93\x94"
    rec_a = shorts + long_occ + b"\x95\x96\x97\x98\x99" * 3
    # Pattern step (level 9: 256 attempts, patternAnalysis).  D = 120: the tail ends in 100 'z', the record is 300 'z',
    # one other byte, 350 'z', noise.  The search at record position 301 (the second run) walks the chain of "zzzz" down
    # from the end of the first run: candidate D+296 matches 4 bytes, every further one a byte more, until candidate
    # D+43 matches 257 > 256 and the walk leaves by the early exit (:613) with m = D+43, whose link is 1.  The pattern
    # step takes cand = D+42: forward 258 bytes of 'z' (to the end of the first run), backward 42 in the record and on
    # through the tail's 100, so the segment is 400 >= 350 = the run at the search position, and the match is placed at
    # its end: cand + 258 - 350 = D - 50, a match of 350 bytes at offset 351 that STARTS IN THE TAIL.  A level L below 9
    # (A = 1 << (L - 1) attempts, no pattern step) leaves by the same exit at A + 1 bytes, offset A + 2.
    dict_p = b"\xa0\xa1\xa2\xa3\xa4" * 4 + b"z" * 100
    rec_p = b"z" * 300 + b"\xb0" + b"z" * 350 + b"\xb1\xb2\xb3\xb4\xb5\xb6\xb7\xb8" * 3
    return [("attempt_budget", dict_a, rec_a, 3), ("pattern_into_tail", dict_p, rec_p, 9)]
