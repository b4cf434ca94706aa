"""Test-side helpers for the dictionary compressor (tests/test_dict_compress_cpu.py, tests/test_gpu_dict_compress.py,
tools/time_dict_compress.py).

* `ref(dirpath)`: compiles tests/dict_compress_ref.c with cc into `dirpath` and returns its ctypes handle with
  load_dict(dict) -> table, compress(src, dict, accel, cap, table) -> (result, bytes) and batch(...) (the C restatement
  of zlz4_compress_fast_using_dict, the checker of the GPU tests).
* `run_batch(zl, ...)`: one zlz4_batch_load_dict + one zlz4_batch_compress_fast_using_dict call on packed records,
  dictionaries and tables, with 0xA5 guard bands; checks that the input, dictionary and table arenas are unchanged.
"""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ENTRIES = 4096
INVALID_STATE, OUTPUT_TOO_SMALL = -5, -1


def bound(n):
    return n + n // 255 + 16                          # compressBound, src/lz4.zig:80-83


def _cbuf(b):
    return (C.c_uint8 * max(1, len(b))).from_buffer_copy(bytes(b) or b"\0")


class Ref:
    def __init__(self, so):
        L = C.CDLL(so)
        L.dc_load_dict.restype = C.c_int64
        L.dc_load_dict.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.dc_compress_with_table.restype = C.c_int64
        L.dc_compress_with_table.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                             C.c_size_t, C.c_uint32, C.c_void_p]
        L.dc_compress_batch.restype = None
        L.dc_compress_batch.argtypes = [C.c_void_p] * 12 + [C.c_uint32] * 4
        self.L = L

    def load_dict(self, d):
        t = np.zeros(ENTRIES, dtype=np.uint32)
        b = _cbuf(d)
        self.L.dc_load_dict(t.ctypes.data, C.addressof(b), len(d))
        return t

    def compress(self, src, dict_bytes, accel=1, cap=None, table=None, stats=None):
        """-> (result, bytes); table None = the dictionary's own; stats: a uint64[2] array that is added to"""
        src, dict_bytes = bytes(src), bytes(dict_bytes)
        t = self.load_dict(dict_bytes) if table is None else np.ascontiguousarray(table, dtype=np.uint32)
        cap = bound(len(src)) if cap is None else cap
        s, d, o = _cbuf(src), _cbuf(dict_bytes), (C.c_uint8 * max(1, cap))()
        r = self.L.dc_compress_with_table(t.ctypes.data, C.addressof(s), len(src), C.addressof(o), cap, C.addressof(d),
                                          len(dict_bytes), accel, None if stats is None else stats.ctypes.data)
        return r, (bytes(o[:r]) if r > 0 else b"")

    def batch(self, buf, offs, lens, caps, dbuf, doffs, dlens, tables, idx, max_in, max_dict, accel):
        """The batch on packed arenas (numpy) -> (results int64[n], outputs list of bytes)"""
        n = len(lens)
        caps = np.asarray(caps, dtype=np.uint32)
        out_offs = np.zeros(n, dtype=np.uint64)
        out_offs[1:] = np.cumsum(caps.astype(np.uint64))[:-1]
        out = np.zeros(max(1, int(caps.astype(np.uint64).sum())), dtype=np.uint8)
        res = np.zeros(n, dtype=np.int64)
        tables = np.ascontiguousarray(tables, dtype=np.uint32)
        ix = None if idx is None else np.ascontiguousarray(idx, dtype=np.uint32)
        a = [np.ascontiguousarray(buf), np.asarray(offs).astype(np.uint64), np.asarray(lens).astype(np.uint32),
             np.ascontiguousarray(dbuf), np.asarray(doffs).astype(np.uint64), np.asarray(dlens).astype(np.uint32)]
        self.L.dc_compress_batch(a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, out.ctypes.data, out_offs.ctypes.data,
                                 caps.ctypes.data, a[3].ctypes.data, a[4].ctypes.data, a[5].ctypes.data, tables.ctypes.data,
                                 None if ix is None else ix.ctypes.data, res.ctypes.data, n, max_in, max_dict, accel)
        return res, [bytes(out[int(o):int(o) + int(r)]) if r > 0 else b"" for o, r in zip(out_offs, res)]


def ref(dirpath):
    so = os.path.join(str(dirpath), "libdict_compress_ref.so")
    if not os.path.exists(so):
        subprocess.check_call(["cc", "-O2", "-std=c11", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "dict_compress_ref.c")])
    return Ref(so)


def _t32(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.uint32)).view(np.int32)).to(dev)


def run_batch(zl, cref, records, caps, dicts, dict_index, dev, accel=1, layout=None, use_idx=True, max_in=None,
              max_dict=None, tables=None, in_input=None):
    """Record i is compressed into a slot of caps[i] bytes against dicts[dict_index[i]] (each dictionary is stored once).
    use_idx: one table per dictionary and d_table_idx = dict_index; else one table per block and d_table_idx NULL.
    tables: uint32[ndicts, 4096] to use in place of what zlz4_batch_load_dict computes (which is checked against the C
    restatement's).  in_input: list of (offset, length) per block -- dictionaries taken from the INPUT arena (d_dict =
    d_in; dicts / dict_index are ignored, one table per block).  layout: gpu_harness.Packed.
    -> (gpu [(result, bytes)], ref [(result, bytes)])"""
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
        t_doff, t_dlen = doffs, dlens                 # per dictionary
        b_doff, b_dlen = doffs[idx], dlens[idx]       # per block
    else:
        dbuf, d_dict = buf, d_in
        b_doff = np.asarray([o for o, _ in in_input], dtype=np.int64)
        b_dlen = np.asarray([k for _, k in in_input], dtype=np.int64)
        t_doff, t_dlen, idx, use_idx = b_doff, b_dlen, np.arange(n), False
    nt = len(t_dlen)
    # tables: one zlz4_batch_load_dict call, behind 4 guard entries in front (still 16-byte aligned) and one guard table
    d_tab = torch.full(((nt + 1) * ENTRIES + 4,), 0x5A5A5A5A, dtype=torch.int64, device=dev).to(torch.int32)
    tview = d_tab[4:]
    lres = torch.full((nt,), -999, dtype=torch.int64, device=dev)
    zl.batch_load_dict(d_dict, torch.from_numpy(t_doff).to(dev), _t32(t_dlen, dev), tview, lres)
    torch.cuda.synchronize()
    loaded = tview.cpu().numpy().view(np.uint32).reshape(-1, ENTRIES)[:nt].copy()
    for k in range(nt):
        d = bytes(dbuf[int(t_doff[k]):int(t_doff[k]) + int(t_dlen[k])])
        assert (loaded[k] == cref.load_dict(d)).all(), "zlz4_batch_load_dict table %d" % k
    if tables is not None:
        loaded = np.ascontiguousarray(tables, dtype=np.uint32).reshape(nt, ENTRIES)
        tview[:nt * ENTRIES] = _t32(loaded.reshape(-1), dev)
    if use_idx:
        tabs, t_idx, ref_idx = loaded, _t32(idx, dev), idx
    else:
        tabs = loaded[idx] if in_input is None else loaded          # one table per block
        d_tab = torch.cat([d_tab[:4], _t32(tabs.reshape(-1), dev), d_tab[-ENTRIES:]])
        tview, t_idx, ref_idx = d_tab[4:], None, None
    tab_before = d_tab.cpu().numpy().copy()
    d_out = torch.full((total,), 0xA5, dtype=torch.uint8, device=dev)
    res = torch.full((n,), -999, dtype=torch.int64, device=dev)
    max_in = (int(lens.max()) if n else 0) if max_in is None else max_in
    max_dict = (int(min(b_dlen.max(), 65536)) if n else 0) if max_dict is None else max_dict
    zl.batch_compress_fast_using_dict(d_in, torch.from_numpy(offs).to(dev), _t32(lens, dev), d_out,
                                      torch.from_numpy(out_offs).to(dev), _t32(caps, dev), d_dict,
                                      torch.from_numpy(b_doff).to(dev), _t32(b_dlen, dev), tview, t_idx, res, max_in,
                                      max_dict, accel)
    torch.cuda.synchronize()
    assert (d_in.cpu().numpy() == buf).all(), "the input arena changed"
    assert (d_dict.cpu().numpy() == dbuf).all(), "the dictionary arena changed"
    assert (d_tab.cpu().numpy() == tab_before).all(), "the table arena changed"
    got = gh._collect(res, d_out, out_offs, guard_ends, caps)
    o = d_out.cpu().numpy()
    for i, (r, _) in enumerate(got):                  # InvalidState writes nothing
        if r == INVALID_STATE:
            assert (o[out_offs[i]:out_offs[i] + int(caps[i])] == 0xA5).all(), "block %d wrote into its slot" % i
    rres, routs = cref.batch(buf, offs, lens, caps, dbuf, b_doff, b_dlen, tabs, ref_idx, max_in, max_dict, accel)
    return got, list(zip([int(r) for r in rres], routs))


def check(got, want, tag=""):
    """byte and status equality; a failed block's slot contents are unspecified"""
    assert len(got) == len(want)
    for i, ((g, gb), (w, wb)) in enumerate(zip(got, want)):
        assert g == w, "%s block %d: result %d, restatement %d" % (tag, i, g, w)
        if w > 0:
            assert gb == wb, "%s block %d: bytes differ" % (tag, i)


def crafted(cref):
    """-> [(name, dictionary, record)]: the edge cases of the dictionary reach.  `cref` picks dictionary positions that
    own their table slot (Stream.loadDict keeps the LAST position of every slot)."""
    import datagen as dg
    rnd = lambda n, s: bytes(dg.random_bytes(n, s))
    out = []
    d1 = rnd(65536, 1)
    out.append(("equals_tail_4k", d1, d1[-4096:]))
    out.append(("equals_tail_4k_long_dict", rnd(3000, 2) + d1, d1[-4096:]))
    per = b"abcdefg" * 40
    out.append(("period_from_dict", rnd(500, 3) + per[:75], (per * 30)[75:75 + 3000] + rnd(40, 4)))
    out.append(("period_1_from_dict", rnd(50, 5) + b"zzzzz", b"z" * 700 + rnd(20, 6)))
    # a 64 KiB dictionary whose first 300 bytes own their slots: record byte j pairs with tail byte j + 1 at offset
    # 65535; the same column one byte further back (offset 65536) is out of range
    d = rnd(300, 7) + bytes(65536 - 300)
    t = cref.load_dict(d)
    h = lambda b4: ((int.from_bytes(b4, "little") * 2654435761) & 0xFFFFFFFF) >> 20
    own = lambda d, t, lo, hi: next(q for q in range(lo, hi) if all(int(t[h(d[q + k:q + k + 4])]) == q + k for k in range(4)))
    p = own(d, t, 8, 200)
    out.append(("offset_65535_only", d, rnd(p - 1, 8) + d[p:p + 60] + rnd(30, 9)))
    out.append(("offset_65536_none", d, rnd(p, 10) + d[p:p + 60] + rnd(30, 11)))
    out.append(("offset_65535_from_start", d, d[1:1 + 200] + rnd(30, 12)))
    G = b"\x01\xfe\x02\xfd"
    clean = lambda b: b.replace(b"\x01", b"\x03")        # no other 4-gram starts like G
    body = clean(rnd(96, 13))
    rec = clean(rnd(30, 14)) + G + clean(rnd(30, 15))
    out.append(("only_at_dict_pos_0", G + body, rec))
    out.append(("at_dict_pos_1", b"\x07" + G + body, rec))
    out.append(("one_byte_dict_64k", b"a" * 65536, b"a" * 5000 + rnd(100, 16) + b"a" * 100))
    out.append(("one_byte_dict_short", b"a" * 9, b"a" * 300 + rnd(20, 17)))
    x = rnd(300, 18)
    q = own(x, cref.load_dict(x), 50, 200)
    out.append(("first_byte_starts_match", x, x[q:q + 70] + rnd(20, 19)))
    out.append(("match_ends_at_dict_end", x, x[-40:] + rnd(40, 20)))
    out.append(("match_spans_dict_end", x, x[-40:] + x[-40:] + rnd(40, 21)))
    return out
