"""Model of the frame index and of frame range decoding (include/zlz4_amd.h: zlz4f_batch_frame_index,
zlz4f_batch_plan_frame_ranges, zlz4f_batch_decompress_frame_range): bytes [a, b) of an lz4f frame through a table of
(position, decoded offset) per block.

Composed from the models that exist: the header parse and XXH32 of zig_lz4_sizes (src/lz4f.zig:483-538), its block size walk
(the index is what frame_size adds up, kept), decompressSafe of zig_lz4_dict (src/lz4.zig:89-251) for a block wanted in full
and P(block, cap) of zig_lz4_prefix (section 4.2e) for the block that b cuts.  Test infrastructure like the other files here:
written from the specification, independent of the kernels, never imported by the product, the bench or smoke().

An index is a list of (pos, dec) pairs, nb + 1 of them; idx_n is the block count or the frame's negative code.  The range
decode does NOT trust the index: it is given as data, and a wrong one has a stated result.
"""
import functools

from zig_lz4_dict import decompress_generic
from zig_lz4_prefix import decompress_prefix
from zig_lz4_sizes import (F_BLOCK_CHECKSUM_INVALID, F_DECOMPRESSION_FAILED, F_FRAME_SIZE_WRONG, _parse_header, block_size,
                           frame_size, xxh32)

INVALID_STATE = -5                                    # include/zlz4_amd.h ZLZ4_ERR_INVALID_STATE
F_DST_MAX_SIZE_TOO_SMALL = -111                       # lz4f.Error (src/lz4f.zig:31-55): -(100 + declaration index)
BLOCK_SIZES = {0: 64 << 10, 4: 64 << 10, 5: 256 << 10, 6: 1 << 20, 7: 4 << 20}   # BlockSizeID.toBlockSize, :64-79
U64 = (1 << 64) - 1


@functools.lru_cache(maxsize=4096)
def _full(data, cap):
    """decompressSafe(block, dst) with dst.len == cap (the tests ask for many ranges over few blocks: kept)"""
    return decompress_generic(data, cap, cap, None)


@functools.lru_cache(maxsize=4096)
def _cut(data, want):
    return decompress_prefix(data, want)


@functools.lru_cache(maxsize=4096)
def _header(src):
    return _parse_header(src)


@functools.lru_cache(maxsize=4096)
def _hash(data):
    return xxh32(data)


def _size_alone(data, dec):
    """a compressed block sized on its own, wherever it starts: the view of the size query with flags 0"""
    return block_size(data)


def frame_index(frame, idx_cap=None, sizer=_size_alone):
    """zlz4f_batch_frame_index for one frame -> (idx_n, entries).  The walk, the checks and their order are frame_size's
    (zig_lz4_sizes._frame_walk, src/lz4f.zig:541-638); an error writes no entry.  `sizer` sizes a compressed block; the
    call uses the plain one (every block on its own) -- a test that wants the history-aware view of a linked frame passes
    its own."""
    src = bytes(frame)
    ph = _parse_header(src)                                            # :547
    if not isinstance(ph, tuple):
        return ph, []
    flg, pos = ph
    n, dec, entries = len(src), 0, []
    while pos < n:                                                     # :563
        if pos + 4 > n:                                                # :565
            return F_FRAME_SIZE_WRONG, []
        h = int.from_bytes(src[pos:pos + 4], "little")
        if h == 0:                                                     # :573: entry nb stands on the end mark
            break
        size = h & 0x7FFFFFFF
        if pos + 4 + size > n:                                         # :582
            return F_FRAME_SIZE_WRONG, []
        data = src[pos + 4:pos + 4 + size]
        nxt = pos + 4 + size
        if flg & 0x10:                                                 # :590-598
            if nxt + 4 > n:
                return F_FRAME_SIZE_WRONG, []
            if int.from_bytes(src[nxt:nxt + 4], "little") != xxh32(data):
                return F_BLOCK_CHECKSUM_INVALID, []
            nxt += 4
        entries.append((pos, dec))
        if h & 0x80000000:                                             # :603-608 stored
            dec += size
        else:                                                          # :610-613
            s = sizer(data, dec)
            if s < 0:
                return F_DECOMPRESSION_FAILED, []
            dec += s
        pos = nxt
    if flg & 0x04 and (pos + 4 if pos < n else pos) + 4 > n:           # :626 (behind the end mark, when there is one)
        return F_FRAME_SIZE_WRONG, []
    entries.append((pos, dec))
    if idx_cap is not None and len(entries) > idx_cap:
        return F_DST_MAX_SIZE_TOO_SMALL, []
    return len(entries) - 1, entries


def block_of(entries, nb, t):
    """The block that holds decoded byte t: the last entry k of 0..nb with dec[k] <= t, by the bisection the kernels use
    (stated step by step: on an index that is not sorted the result is whatever these steps give).  -1: entry 0 is above t."""
    lo, hi = 0, nb + 1
    while lo < hi:
        mid = lo + (hi - lo) // 2
        if entries[mid][1] <= t:
            lo = mid + 1
        else:
            hi = mid
    return lo - 1


def _span(entries, idx_n, nframes_ok, a, b):
    """-> (a', b', k0, k1, found)"""
    if not nframes_ok or a > b or idx_n < 0:
        return 0, 0, 0, 0, False
    nb = idx_n
    S = entries[nb][1]
    a1, b1 = min(a, S), min(b, S)
    if a1 == b1:
        return a1, b1, 0, 0, False
    k0, k1 = block_of(entries, nb, a1), block_of(entries, nb, b1 - 1)
    found = 0 <= k0 < nb and 0 <= k1 < nb and k0 <= k1 and entries[k0][1] <= a1
    return a1, b1, k0, k1, found


def plan_range(entries, idx_n, a, b, frame_ok=True):
    """zlz4f_batch_plan_frame_ranges for one range -> (slot bytes, items)"""
    a1, b1, k0, k1, found = _span(entries, idx_n, frame_ok, a, b)
    if not found:
        return 0, 0
    return b1 - entries[k0][1], k1 - k0 + 1


def plan(ranges, align=0):
    """the packed layout: ranges = [(slot bytes, items)] -> (offsets, arena bytes, items)"""
    al = max(1, align)
    offs, pos = [], 0
    for cap, _ in ranges:
        offs.append(pos)
        pos += (cap + al - 1) & ~(al - 1)
    return offs, pos, sum(i for _, i in ranges)


def _admit(frame, entries, idx_n, a, b, dst_cap, reserved, frame_ok):
    """statuses 1-3 -> (status, None) for a range that ends here (0: the empty range), else (None, (flg, a', b', k0, k1))"""
    # 1. the range itself, the index status, the header, entry 0, the chain k0..k1+1
    if not frame_ok or a > b or reserved != 0:
        return INVALID_STATE, None
    if idx_n < 0:
        return idx_n, None
    src = bytes(frame)
    ph = _header(src)
    if not isinstance(ph, tuple):
        return ph, None
    flg, hsize = ph
    bs = BLOCK_SIZES[(src[5] >> 4) & 7]
    n = len(src)
    a1, b1, k0, k1, found = _span(entries, idx_n, True, a, b)
    if entries[0][0] != hsize:
        return INVALID_STATE, None
    if a1 == b1:                                                       # 2.
        return 0, None
    if not found:
        return INVALID_STATE, None
    for k in range(k0, k1 + 1):
        (p, d), (q, e) = entries[k], entries[k + 1]
        if q <= p or p + 4 > n or q > n or e < d or e - d > bs:
            return INVALID_STATE, None
    if entries[k1][1] >= b1 or entries[k1 + 1][1] < b1:
        return INVALID_STATE, None
    need = b1 - entries[k0][1]
    if (need if dst_cap is None else dst_cap) < need:                  # 3.
        return F_DST_MAX_SIZE_TOO_SMALL, None
    return None, (flg, a1, b1, k0, k1)


def range_items(frame, entries, idx_n, a, b, dst_cap=None, reserved=0, frame_ok=True):
    """the items the range takes of max_items: k1 - k0 + 1 once statuses 1-3 are passed, else 0"""
    st, go = _admit(frame, entries, idx_n, a, b, dst_cap, reserved, frame_ok)
    return 0 if go is None else go[4] - go[3] + 1


def decompress_frame_range(frame, entries, idx_n, a, b, dst_cap=None, reserved=0, frame_ok=True, fits=True):
    """zlz4f_batch_decompress_frame_range for one range -> (result, skip, slot bytes).  dst_cap None: what the plan gives.
    fits False: the range's items lie past max_items.  On an error skip is 0 and the slot is b""."""
    st, go = _admit(frame, entries, idx_n, a, b, dst_cap, reserved, frame_ok)
    if go is None:
        return st, 0, b""
    if not fits:                                                       # 4.
        return INVALID_STATE, 0, b""
    src = bytes(frame)
    flg, a1, b1, k0, k1 = go
    d0 = entries[k0][1]
    slot = bytearray()
    for k in range(k0, k1 + 1):                                        # 5. the first failing block in block order
        (p, d), (q, e) = entries[k], entries[k + 1]
        w = int.from_bytes(src[p:p + 4], "little")
        sz = w & 0x7FFFFFFF
        if w == 0 or p + 4 + sz + (4 if flg & 0x10 else 0) != q:       # the end mark is no block
            return INVALID_STATE, 0, b""
        data = src[p + 4:p + 4 + sz]
        if flg & 0x10 and int.from_bytes(src[p + 4 + sz:p + 8 + sz], "little") != _hash(data):
            return F_BLOCK_CHECKSUM_INVALID, 0, b""
        step, want = e - d, min(e - d, b1 - d)
        assert len(slot) == d - d0
        if w >> 31:
            if sz != step:
                return INVALID_STATE, 0, b""
            slot += data[:want]
        elif want == step:                                             # wanted in full: the safe decoder, exact capacity
            r, out = _full(data, step)
            if r != step:
                return F_DECOMPRESSION_FAILED, 0, b""
            slot += out
        else:                                                          # the block that b' cuts
            r, out = _cut(data, want)
            if r != want:
                return F_DECOMPRESSION_FAILED, 0, b""
            slot += out
    return b1 - a1, a1 - d0, bytes(slot)                               # 6.


def frame_range(frame, a, b):
    """The host call zlz4f_decompress_frame_range -> (result, bytes): exactly bytes [a', b')."""
    src = bytes(frame)
    ph = _header(src)
    if not isinstance(ph, tuple):
        return ph, b""
    if a > b:
        return INVALID_STATE, b""
    idx_n, entries = frame_index(src)
    if idx_n < 0:
        return idx_n, b""
    r, skip, slot = decompress_frame_range(src, entries, idx_n, a, b)
    return (r, slot[skip:skip + r]) if r >= 0 else (r, b"")


__all__ = ["frame_index", "block_of", "plan_range", "plan", "range_items", "decompress_frame_range", "frame_range", "frame_size"]
