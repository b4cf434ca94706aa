"""Test-side helpers for the streaming compressor (tests/test_stream_cpu.py, tests/test_gpu_stream.py,
tools/time_stream_compress.py).

* `ref(dirpath)`: compiles tests/stream_ref.c with cc into `dirpath` and returns its ctypes handle with
  load_dict(dict) -> (table, dictSize), cont(table, src, accel, cap) -> (result, bytes, table) and
  batch(...) (the C restatement, fast enough for large GPU batches).
* `run_continue(zl, ...)`: one zlz4_batch_compress_fast_continue call on packed blocks and tables, with guard bands.
* `run_load_dict(zl, dicts, dev)`: one zlz4_batch_load_dict call.
"""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ENTRIES = 4096


class Ref:
    def __init__(self, so):
        L = C.CDLL(so)
        L.sr_load_dict.restype = C.c_int64
        L.sr_load_dict.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.sr_compress_continue.restype = C.c_int64
        L.sr_compress_continue.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint32]
        L.sr_compress_continue_batch.restype = None
        L.sr_compress_continue_batch.argtypes = [C.c_void_p] * 10 + [C.c_uint32, C.c_uint32]
        self.L = L

    def load_dict(self, d):
        d = bytes(d)
        t = np.zeros(ENTRIES, dtype=np.uint32)
        b = (C.c_uint8 * max(1, len(d))).from_buffer_copy(d or b"\0")
        r = self.L.sr_load_dict(t.ctypes.data, C.addressof(b), len(d))
        return t, r

    def cont(self, table, src, accel=1, cap=None):
        src = bytes(src)
        t = np.array(table, dtype=np.uint32)
        cap = len(src) + len(src) // 255 + 16 if cap is None else cap
        s = (C.c_uint8 * max(1, len(src))).from_buffer_copy(src or b"\0")
        o = (C.c_uint8 * max(1, cap))()
        r = self.L.sr_compress_continue(t.ctypes.data, C.addressof(s), len(src), C.addressof(o), cap, accel)
        return r, (bytes(o[:r]) if r > 0 else b""), t

    def batch(self, tables_in, idx, items, caps, accel):
        """-> (results int64[n], outputs list of bytes, tables_out uint32[n, 4096])"""
        n = len(items)
        tables_in = np.ascontiguousarray(tables_in, dtype=np.uint32)
        buf, offs, lens = pack(items)
        caps = np.asarray(caps, dtype=np.uint32)
        out_offs = np.zeros(n, dtype=np.uint64)
        out_offs[1:] = np.cumsum(caps.astype(np.uint64))[:-1]
        out = np.zeros(max(1, int(caps.astype(np.uint64).sum())), dtype=np.uint8)
        res = np.zeros(n, dtype=np.int64)
        tout = np.zeros((n, ENTRIES), dtype=np.uint32)
        ix = None if idx is None else np.ascontiguousarray(idx, dtype=np.uint32)
        offs64, lens32 = offs.astype(np.uint64), lens.astype(np.uint32)    # (kept alive for the duration of the call)
        self.L.sr_compress_continue_batch(tables_in.ctypes.data, None if ix is None else ix.ctypes.data, tout.ctypes.data,
                                          buf.ctypes.data, offs64.ctypes.data, lens32.ctypes.data, out.ctypes.data,
                                          out_offs.ctypes.data, caps.ctypes.data, res.ctypes.data, n, accel)
        outs = [bytes(out[int(o):int(o) + int(r)]) if r > 0 else b"" for o, r in zip(out_offs, res)]
        return res, outs, tout


def ref(dirpath):
    so = os.path.join(str(dirpath), "libstream_ref.so")
    if not os.path.exists(so):
        subprocess.check_call(["cc", "-O2", "-std=c11", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "stream_ref.c")])
    return Ref(so)


def pack(items, align=16):
    offs, lens, pos = [], [], 0
    for b in items:
        offs.append(pos)
        lens.append(len(b))
        pos += (len(b) + align - 1) // align * align + align
    buf = np.zeros(max(pos, align), dtype=np.uint8)
    for o, b in zip(offs, items):
        if len(b):
            buf[o:o + len(b)] = np.frombuffer(bytes(b), dtype=np.uint8)
    return buf, np.array(offs, dtype=np.int64), np.array(lens, dtype=np.int64)


def _t32(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(dev)


def run_continue(zl, items, caps, tables_in, idx, dev, accel=1, max_in=None, in_place=False, write_tables=True):
    """zlz4_batch_compress_fast_continue -> (results, outputs, tables_out uint32[n, 4096] or None).  The output slots are
    separated by 64-byte guard bands, and the table arena by one guard table, which must stay untouched."""
    import torch
    n = len(items)
    buf, offs, lens = pack(items)
    caps = np.asarray(caps, dtype=np.int64)
    out_offs = np.zeros(n, dtype=np.int64)
    pos = 0
    for i, c in enumerate(caps):
        out_offs[i] = pos
        pos += (int(c) + 15) // 16 * 16 + 64
    d_in = torch.from_numpy(buf).to(dev)
    d_out = torch.full((max(pos, 16),), 0xA5, dtype=torch.uint8, device=dev)
    t_in_off = torch.from_numpy(offs).to(dev)
    t_in_len = _t32(lens, dev)
    t_out_off = torch.from_numpy(out_offs).to(dev)
    t_out_cap = _t32(caps, dev)
    res = torch.full((n,), -999, dtype=torch.int64, device=dev)
    tin = np.ascontiguousarray(tables_in, dtype=np.uint32).reshape(-1, ENTRIES)
    guard = np.full((1, ENTRIES), 0x5A5A5A5A, dtype=np.uint32)
    d_tin = _t32(np.concatenate([tin, guard]).reshape(-1), dev)
    d_idx = None if idx is None else _t32(np.asarray(idx), dev)
    if in_place:
        d_tout = d_tin
    elif write_tables:
        d_tout = _t32(np.concatenate([np.full((n, ENTRIES), 0xDEADBEEF, dtype=np.uint32), guard]).reshape(-1), dev)
    else:
        d_tout = None
    max_in = int(lens.max()) if max_in is None and n else (max_in or 0)
    zl.batch_compress_fast_continue(d_in, t_in_off, t_in_len, d_out, t_out_off, t_out_cap, d_tin, d_idx, d_tout, res,
                                    max_in, accel)
    torch.cuda.synchronize()
    r = res.cpu().numpy()
    o = d_out.cpu().numpy()
    outs = []
    for i in range(n):
        k = int(r[i])
        g = o[out_offs[i] + int(caps[i]): out_offs[i] + (int(caps[i]) + 15) // 16 * 16 + 64]
        assert (g == 0xA5).all(), "block %d wrote past its capacity" % i
        outs.append(bytes(o[out_offs[i]: out_offs[i] + k]) if k > 0 else b"")
    tout = None
    if d_tout is not None:
        ta = d_tout.cpu().numpy().view(np.uint32).reshape(-1, ENTRIES)
        assert (ta[-1] == 0x5A5A5A5A).all(), "the guard table was written"
        tout = ta[:-1] if not in_place else ta[:-1]
    if not in_place:
        ti = d_tin.cpu().numpy().view(np.uint32).reshape(-1, ENTRIES)
        assert (ti[:-1] == tin).all() and (ti[-1] == 0x5A5A5A5A).all(), "the input tables were written"
    return r, outs, tout


def run_load_dict(zl, dicts, dev):
    """zlz4_batch_load_dict -> (results int64[n], tables uint32[n, 4096])"""
    import torch
    n = len(dicts)
    buf, offs, lens = pack(dicts)
    d_dict = torch.from_numpy(buf).to(dev)
    t_off = torch.from_numpy(offs).to(dev)
    t_len = _t32(lens, dev)
    tables = torch.full(((n + 1) * ENTRIES,), 0x5A5A5A5A, dtype=torch.int64, device=dev).to(torch.int32)
    res = torch.full((n,), -999, dtype=torch.int64, device=dev)
    zl.batch_load_dict(d_dict, t_off, t_len, tables, res)
    torch.cuda.synchronize()
    t = tables.cpu().numpy().view(np.uint32).reshape(-1, ENTRIES)
    assert (t[-1] == 0x5A5A5A5A).all(), "the guard table was written"
    return res.cpu().numpy(), t[:-1]


# ---------------------------------------------------------------- blocks in which a seed must produce a match
def hash4(b4):
    return ((int.from_bytes(bytes(b4), "little") * 2654435761) & 0xFFFFFFFF) >> 20


def planted(n, seed, run_end=200, r_off=20):
    """A block whose parse reads a seed: bytes [0, E) are one repeated byte c (E = run_end), so the match found at 2
    (offset 1) covers positions 3 .. E - 1 and none of them is probed or put (src/lz4.zig:730-736).  The 4-gram
    G = c c X0 X1 at v = E - 2 straddles the end of that match, so it never enters the table.  G is written again at
    r = E + r_off, the first probe of slot hash4(G) after the match (r_off < 64: the acceleration-1 window path; larger:
    the generic path).  A table with table[hash4(G)] = v makes that probe match v (offset r - v); a zero table cannot.
    -> (block, v, G)."""
    rng = np.random.default_rng(seed)
    c = int(rng.integers(1, 256))
    b = bytearray(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
    b[0:run_end] = bytes([c]) * run_end
    while b[run_end] == c:
        b[run_end] = int(rng.integers(0, 256))
    G = bytes(b[run_end - 2:run_end + 2])
    r = run_end + r_off
    b[r:r + 4] = G
    while b[r + 4] == b[run_end + 2]:                    # the match at r is exactly 4 bytes long
        b[r + 4] = int(rng.integers(0, 256))
    # no position probed before r may share G's slot (it would put itself there first): re-draw the colliding bytes
    hg = hash4(G)
    assert hash4(bytes([c]) * 4) != hg, "choose another seed"
    p = run_end
    while p < r:
        if hash4(b[p:p + 4]) == hg:
            k = p + 3 if p + 3 < r else p                # (never one of E, E + 1: they are X0 X1 of G)
            b[k] = (b[k] + 1) & 255
            p = max(run_end, k - 3)
            continue
        p += 1
    return bytes(b), run_end - 2, G


def chained_planted(v, seed, n1=262144, n2=65536, n3=262144):
    """Three steps of one stream in which step 3 must use a seed >= 65536 that step 1 wrote and step 2 passed through:
      step 1: zeros up to v, then c c X0 X1 X2 .. X7, then zeros -- the zero match ends at v, so anchor v is put at
              hash4(c c X0 X1) (:730-736), and the zeros after it are one more long match (few puts);
      step 2: n2 zeros -- it touches only the slot of 0000 (a 16-bit table cannot even load v, so v must pass through);
      step 3: planted() with the run of c ending at v + 2: its window probe at v + 22 matches v.
    -> (block1, block2, block3)."""
    rng = np.random.default_rng(seed)
    c = int(rng.integers(1, 256))
    X = bytes(int(x) for x in rng.integers(1, 256, 8))
    b1 = bytearray(n1)
    b1[v] = c
    b1[v + 1] = c
    b1[v + 2:v + 10] = X
    b3 = bytearray(rng.integers(0, 256, n3, dtype=np.uint8).tobytes())
    E = v + 2
    b3[0:E] = bytes([c]) * E
    b3[E:E + 8] = X
    r = E + 20
    b3[r:r + 4] = bytes([c, c]) + X[:2]
    while b3[r + 4] == X[2]:
        b3[r + 4] = int(rng.integers(0, 256))
    return bytes(b1), bytes(n2), bytes(b3)
