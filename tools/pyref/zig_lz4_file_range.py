"""Model of the file index and of file range decoding (include/zlz4_amd.h: zlz4f_batch_file_index,
zlz4f_batch_decompress_file_range, zlz4f_decompress_file_range): bytes [a, b) of a whole .lz4 file -- frame, skippable and
legacy members in any order -- through one table of (position in the file, offset in its content) per block.

Composed from the models that exist: the frame index of zig_lz4_frame_range (one frame member is one frame), block_size of
zig_lz4_sizes for a legacy block, the block decoders that zig_lz4_frame_range caches.  The split into members is written
here from the formats.  Test infrastructure like the other files of this directory: independent of the kernels, never
imported by the product, the bench or smoke().

A member is (pos, len, kind); an index is a list of (pos, dec) pairs, nb + 1 of them; idx_n is the block count or the
file's negative code.  The range decode does NOT trust the index: a wrong one has a stated result.
"""
import functools

import zig_lz4_frame_range as fr
from zig_lz4_sizes import (F_BLOCK_CHECKSUM_INVALID, F_DECOMPRESSION_FAILED, F_FRAME_HEADER_INCOMPLETE, F_FRAME_SIZE_WRONG,
                           block_size)

FRAME, SKIPPABLE, SKIPPABLE_TRUNCATED, LEGACY = 1, 2, 3, 4
LEGACY_MAGIC, SKIP_MAGIC = 0x184C2102, 0x184D2A50
LEGACY_BLOCK_SIZE, LEGACY_BLOCK_BOUND = 8 << 20, 8421520
INVALID_STATE, F_DST_MAX_SIZE_TOO_SMALL, F_PARAMETER_INVALID = fr.INVALID_STATE, fr.F_DST_MAX_SIZE_TOO_SMALL, -104


def _u32(b, pos):
    return int.from_bytes(b[pos:pos + 4], "little")


# ----------------------------------------------------------------------------- members
def legacy_walk(b):
    """the legacy frame at b[0]: -> (verdict, [(offset of the size word, size)], consumed)"""
    n = len(b)
    pos, blocks = 4, []
    while True:
        if pos == n:
            return 0, blocks, n
        if n - pos < 4:
            return F_FRAME_SIZE_WRONG, blocks, n
        w = _u32(b, pos)
        if w > LEGACY_BLOCK_BOUND:                     # the next member
            return 0, blocks, pos
        if w == 0:
            return F_DECOMPRESSION_FAILED, blocks, n
        if pos + 4 + w > n:
            return F_FRAME_SIZE_WRONG, blocks, n
        blocks.append((pos, w))
        pos += 4 + w


def _frame_len(b):
    """the length of the frame member at b[0], or None where it cannot be delimited"""
    ph = fr._header(bytes(b[:19]))
    if not isinstance(ph, tuple):
        return None
    flg, pos = ph
    n = len(b)
    while True:
        if pos + 4 > n:
            return None
        w = _u32(b, pos)
        pos += 4
        if w == 0:
            break
        pos += w & 0x7FFFFFFF
        if pos > n:
            return None
        if flg & 0x10:
            if pos + 4 > n:
                return None
            pos += 4
    if flg & 0x04:
        if pos + 4 > n:
            return None
        pos += 4
    return pos


def split(buf, legacy=True):
    """-> [(pos, len, kind)]: what cannot be delimited is the last member and reaches to the end"""
    buf = bytes(buf)
    n, pos, out = len(buf), 0, []
    while pos < n:
        rest = n - pos
        magic = _u32(buf, pos) if rest >= 4 else None
        if magic is not None and (magic & 0xFFFFFFF0) == SKIP_MAGIC:
            if rest < 8 or 8 + _u32(buf, pos + 4) > rest:
                out.append((pos, rest, SKIPPABLE_TRUNCATED))
                break
            ln = 8 + _u32(buf, pos + 4)
            out.append((pos, ln, SKIPPABLE))
        elif legacy and magic == LEGACY_MAGIC:
            verdict, _, consumed = legacy_walk(buf[pos:])
            out.append((pos, consumed, LEGACY))
            if verdict < 0:
                break
            ln = consumed
        else:
            ln = _frame_len(buf[pos:])
            out.append((pos, rest if ln is None else ln, FRAME))
            if ln is None:
                break
        pos += ln
    return out


# ----------------------------------------------------------------------------- the index
@functools.lru_cache(maxsize=4096)
def _frame_member(body):
    """the frame index of one frame member (the tests build many files from few members: kept)"""
    return fr.frame_index(body)


@functools.lru_cache(maxsize=4096)
def _legacy_block(data):
    return block_size(data)


def file_index(buf, legacy=True, idx_cap=None, frame_member=None):
    """zlz4f_batch_file_index for one buffer -> (idx_n, entries).  The first member in member order that is not OK decides;
    the capacity is the last check; an error writes no entry.  frame_member: what indexes one frame member (body -> (n,
    entries)); the dictionary model (zig_lz4_file_dict) passes its own."""
    frame_member = frame_member or _frame_member
    buf = bytes(buf)
    entries, dec, end = [], 0, 0
    for pos, ln, kind in split(buf, legacy):
        body = buf[pos:pos + ln]
        if kind == FRAME:
            n, ents = frame_member(body)
            if n < 0:
                return n, []
            entries += [(pos + p, dec + d) for p, d in ents[:n]]
            end, dec = pos + ents[n][0], dec + ents[n][1]
        elif kind == LEGACY:
            verdict, blocks, _ = legacy_walk(body)
            for p, w in blocks:
                s = _legacy_block(body[p + 4:p + 4 + w])
                if s < 0 or s > LEGACY_BLOCK_SIZE:
                    return F_DECOMPRESSION_FAILED, []
                entries.append((pos + p, dec))
                dec += s
            if verdict < 0:
                return verdict, []
            end = pos + ln
        elif kind == SKIPPABLE_TRUNCATED:
            return (F_FRAME_HEADER_INCOMPLETE if ln < 8 else F_FRAME_SIZE_WRONG), []
    entries.append((end, dec))
    if idx_cap is not None and len(entries) > idx_cap:
        return F_DST_MAX_SIZE_TOO_SMALL, []
    return len(entries) - 1, entries


# ----------------------------------------------------------------------------- ranges
def member_of(buf, members, pos):
    """The member an item takes for the block word at `pos`, by the bisection the kernels use -> (end, bound, block
    checksums, legacy) or None: no member starts at or in front of pos, it is no frame or legacy member, it leaves the
    buffer, its header is none, pos lies inside the header or fewer than 4 bytes in front of the member's end."""
    lo, hi = 0, len(members)
    while lo < hi:
        mid = lo + (hi - lo) // 2
        if members[mid][0] <= pos:
            lo = mid + 1
        else:
            hi = mid
    if lo == 0:
        return None
    mpos, mlen, kind = members[lo - 1]
    n = len(buf)
    if mlen > n or mpos > n - mlen:
        return None
    if kind == FRAME:
        ph = fr._header(bytes(buf[mpos:mpos + min(mlen, 19)]))
        if not isinstance(ph, tuple):
            return None
        first = mpos + ph[1]
        out = (mpos + mlen, fr.BLOCK_SIZES[(buf[mpos + 5] >> 4) & 7], bool(ph[0] & 0x10), False)
    elif kind == LEGACY:
        if mlen < 4 or _u32(buf, mpos) != LEGACY_MAGIC:
            return None
        first = mpos + 4
        out = (mpos + mlen, LEGACY_BLOCK_SIZE, False, True)
    else:
        return None
    if pos < first or pos > out[0] or out[0] - pos < 4:
        return None
    return out


def _admit(buf, members, entries, idx_n, a, b, dst_cap, reserved, buf_ok):
    """the statuses in front of max_items -> (status, None) for a range that ends here, else (None, (a', b', k0, k1))"""
    if not buf_ok or a > b or reserved != 0:
        return INVALID_STATE, None
    if idx_n < 0:
        return idx_n, None
    a1, b1, k0, k1, found = fr._span(entries, idx_n, True, a, b)
    if a1 == b1:
        return 0, None
    if not found or not members:
        return INVALID_STATE, None
    for k in range(k0, k1 + 1):
        (p, d), (q, e) = entries[k], entries[k + 1]
        m = member_of(buf, members, p)
        if m is None or q <= p or e < d or e - d > m[1]:
            return INVALID_STATE, None
    if entries[k1][1] >= b1 or entries[k1 + 1][1] < b1:
        return INVALID_STATE, None
    need = b1 - entries[k0][1]
    if (need if dst_cap is None else dst_cap) < need:
        return F_DST_MAX_SIZE_TOO_SMALL, None
    return None, (a1, b1, k0, k1)


def range_items(buf, members, entries, idx_n, a, b, dst_cap=None, reserved=0, buf_ok=True):
    """the items the range takes of max_items"""
    st, go = _admit(bytes(buf), members, entries, idx_n, a, b, dst_cap, reserved, buf_ok)
    return 0 if go is None else go[3] - go[2] + 1


def decompress_file_range(buf, members, entries, idx_n, a, b, dst_cap=None, reserved=0, buf_ok=True, fits=True,
                          block_dict=None):
    """zlz4f_batch_decompress_file_range for one range -> (result, skip, slot bytes).  dst_cap None: what the plan gives.
    fits False: the range's items lie past max_items.  On an error skip is 0 and the slot is b"".  block_dict: pos -> the
    dictionary bytes the block at pos is decoded with (b"": none); the dictionary model (zig_lz4_file_dict) passes it."""
    buf = bytes(buf)
    st, go = _admit(buf, members, entries, idx_n, a, b, dst_cap, reserved, buf_ok)
    if go is None:
        return st, 0, b""
    if not fits:
        return INVALID_STATE, 0, b""
    a1, b1, k0, k1 = go
    d0 = entries[k0][1]
    slot = bytearray()
    for k in range(k0, k1 + 1):                                        # the first failing block in block order
        (p, d), (q, e) = entries[k], entries[k + 1]
        end, bound, bc, legacy = member_of(buf, members, p)
        w = _u32(buf, p)
        if legacy:
            sz, stored = w, False
            if w == 0 or w > LEGACY_BLOCK_BOUND:
                return INVALID_STATE, 0, b""
        else:
            sz, stored = w & 0x7FFFFFFF, bool(w >> 31)
            if w == 0:                                                 # the end mark is no block
                return INVALID_STATE, 0, b""
        nxt = p + 4 + sz + (4 if bc else 0)
        if nxt > end:
            return INVALID_STATE, 0, b""
        if q <= end:                                                   # k + 1 in the same member
            ok = nxt == q
        elif legacy:
            ok = nxt == end
        else:                                                          # the frame member's last block
            ok = nxt == end or (end - nxt >= 4 and _u32(buf, nxt) == 0)
        if not ok:
            return INVALID_STATE, 0, b""
        data = buf[p + 4:p + 4 + sz]
        if bc and _u32(buf, p + 4 + sz) != fr._hash(data):
            return F_BLOCK_CHECKSUM_INVALID, 0, b""
        step, want = e - d, min(e - d, b1 - d)
        assert len(slot) == d - d0
        if stored:
            if sz != step:
                return INVALID_STATE, 0, b""
            slot += data[:want]
        elif block_dict is not None and block_dict(p):                 # the decoders that take a dictionary
            T = block_dict(p)
            r, out = fr.decompress_generic(data, step, step, T) if want == step else fr.decompress_prefix(data, want, T)
            if r != want:
                return F_DECOMPRESSION_FAILED, 0, b""
            slot += out
        elif want == step:                                             # wanted in full: the safe decoder, exact capacity
            r, out = fr._full(data, step)
            if r != step:
                return F_DECOMPRESSION_FAILED, 0, b""
            slot += out
        else:                                                          # the block that b' cuts
            r, out = fr._cut(data, want)
            if r != want:
                return F_DECOMPRESSION_FAILED, 0, b""
            slot += out
    return b1 - a1, a1 - d0, bytes(slot)


def plan_range(entries, idx_n, a, b, buf_ok=True):
    """the plan is the frame range plan"""
    return fr.plan_range(entries, idx_n, a, b, buf_ok)


def file_range(buf, a, b, legacy=True, split_flags=None):
    """The host call zlz4f_decompress_file_range -> (result, bytes): exactly bytes [a', b')."""
    if split_flags is not None:
        if split_flags & ~1:
            return F_PARAMETER_INVALID, b""
        legacy = bool(split_flags & 1)
    if a > b:
        return INVALID_STATE, b""
    buf = bytes(buf)
    idx_n, entries = file_index(buf, legacy)
    if idx_n < 0:
        return idx_n, b""
    r, skip, slot = decompress_file_range(buf, split(buf, legacy), entries, idx_n, a, b)
    return (r, slot[skip:skip + r]) if r >= 0 else (r, b"")


__all__ = ["split", "legacy_walk", "file_index", "member_of", "plan_range", "range_items", "decompress_file_range",
           "file_range"]
