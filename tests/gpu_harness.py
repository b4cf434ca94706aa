"""Helpers for the -m gpu parity tests: pack byte strings into device batches and call the C ABI."""
import numpy as np
import torch


class Packed:
    """Layout option of the batch helpers: blocks packed back to back at unaligned byte offsets (the first at offset 1,
    then gaps of gaps[0]..gaps[1] bytes), the input tensor ending exactly where the last block ends; output slots at odd
    offsets, each followed by an odd-sized guard band of 63..65 bytes.  `fill` is what the gaps hold: "zero", or
    "cont" -- bytes that continue the block before the gap (its own first bytes for even blocks, for odd blocks the
    bytes that followed the last earlier occurrence of its final 8 bytes, i.e. what would extend its last match).
    A result must not depend on either."""

    def __init__(self, seed=0, fill="zero", gaps=(0, 3)):
        assert fill in ("zero", "cont")
        self.seed, self.fill, self.gaps = seed, fill, gaps


def _continuation(b, k, i):
    src = b
    if i % 2:
        j = b.rfind(b[-8:], 0, len(b) - 1)
        if j >= 0 and len(b) >= 8:
            src = b[j + 8:] + b
    return (src * (k // len(src) + 1))[:k]


def _pack(items, align=16, layout=None):
    if layout is not None:
        return _pack_packed(items, layout)
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


def _pack_packed(items, layout):
    rng = np.random.default_rng(layout.seed)
    offs, pos = [], 1
    for b in items:
        offs.append(pos)
        pos += len(b) + int(rng.integers(layout.gaps[0], layout.gaps[1] + 1))
    total = offs[-1] + len(items[-1]) if items else 1
    buf = np.zeros(max(total, 1), dtype=np.uint8)
    for i, (o, b) in enumerate(zip(offs, items)):
        if len(b):
            buf[o:o + len(b)] = np.frombuffer(bytes(b), dtype=np.uint8)
        if layout.fill == "cont":
            end = offs[i + 1] if i + 1 < len(items) else total
            gap = end - (o + len(b))
            if gap > 0 and len(b):
                buf[o + len(b):end] = np.frombuffer(_continuation(bytes(b), gap, i), dtype=np.uint8)
    if layout.fill == "cont" and items and len(items[0]):
        buf[0] = bytes(items[0])[-1]                  # the byte before the first block
    return buf, np.array(offs, dtype=np.int64), np.array([len(b) for b in items], dtype=np.int64)


def _out_slots(caps, layout=None):
    """-> (slot offsets, guard band ends, arena size): aligned slots with a 64-byte guard band, or (Packed) odd offsets"""
    offs, ends, pos = [], [], 1 if layout is not None else 0
    for c in caps:
        c = int(c)
        offs.append(pos)
        if layout is None:
            pos += (c + 15) // 16 * 16 + 64          # 64 B guard band between slots
        else:
            pos += c + 63
            pos += 1 if pos % 2 == 0 else 2          # the next slot starts at an odd offset: 64 or 65 guard bytes
        ends.append(pos)
    return np.array(offs, dtype=np.int64), ends, max(pos, 16)


def _run(zl, kind, items, caps, dev, layout=None, max_in=None, **kw):
    buf, offs, lens = _pack(items, layout=layout)
    caps = np.asarray(caps, dtype=np.int64)
    out_offs, guard_ends, total = _out_slots(caps, layout)
    d_in = torch.from_numpy(buf).to(dev)
    d_out = torch.full((total,), 0xA5, dtype=torch.uint8, device=dev)
    t_in_off = torch.from_numpy(offs).to(dev)
    t_in_len = torch.from_numpy(lens.astype(np.uint32).view(np.int32)).to(dev)
    t_out_off = torch.from_numpy(out_offs).to(dev)
    t_out_cap = torch.from_numpy(caps.astype(np.uint32).view(np.int32)).to(dev)
    res = torch.full((len(items),), -999, dtype=torch.int64, device=dev)
    if max_in is None:                                # the declared bound defaults to the exact maximum
        max_in = int(lens.max()) if len(lens) else 0
    if kind == "fast":
        zl.batch_compress_fast(d_in, t_in_off, t_in_len, d_out, t_out_off, t_out_cap, res, max_in, kw.get("accel", 1))
    elif kind == "hc":
        ws = torch.empty(max(16, zl.batch_compress_hc_workspace(len(items), max_in)), dtype=torch.uint8, device=dev)
        zl.batch_compress_hc(d_in, t_in_off, t_in_len, d_out, t_out_off, t_out_cap, res, max_in, kw["level"], ws)
    elif kind == "dec":
        zl.batch_decompress_safe(d_in, t_in_off, t_in_len, d_out, t_out_off, t_out_cap, res)
    else:
        raise ValueError(kind)
    torch.cuda.synchronize()
    if layout is not None:
        assert (d_in.cpu().numpy() == buf).all(), "the input arena changed"
    return _collect(res, d_out, out_offs, guard_ends, caps)


def _collect(res, d_out, out_offs, guard_ends, caps):
    r = res.cpu().numpy()
    o = d_out.cpu().numpy()
    outs = []
    for i in range(len(caps)):
        n = int(r[i])
        # guard band must be untouched (no write past the slot capacity)
        guard = o[out_offs[i] + int(caps[i]): guard_ends[i]]
        assert (guard == 0xA5).all(), "block %d wrote past its capacity" % i
        outs.append((n, bytes(o[out_offs[i]: out_offs[i] + n]) if n > 0 else b""))
    if len(caps):
        assert (o[:out_offs[0]] == 0xA5).all(), "a block wrote before the first slot"
    return outs


def compress_fast(zl, items, dev, caps=None, accel=1, layout=None, max_in=None):
    caps = [zl.compressBound(len(b)) for b in items] if caps is None else caps
    return _run(zl, "fast", items, caps, dev, layout=layout, max_in=max_in, accel=accel)


def compress_hc(zl, items, dev, level, caps=None, layout=None, max_in=None):
    caps = [zl.compressBound(len(b)) for b in items] if caps is None else caps
    return _run(zl, "hc", items, caps, dev, layout=layout, max_in=max_in, level=level)


def decompress(zl, items, caps, dev, layout=None):
    return _run(zl, "dec", items, caps, dev, layout=layout)
