"""Model of seek tables (include/zlz4_amd.h: zlz4f_seek_table_bound, zlz4f_batch_append_seek_table,
zlz4f_batch_load_seek_table, zlz4f_batch_concat): the last, skippable member of a seekable .lz4 file, which stores the
file's member table and block index.

Written from the format as the header states it, not from the kernels.  The members and the index that a table stores are
those of the file range model (zig_lz4_file_range: split, file_index).  Test infrastructure like the other files of this
directory: never imported by the product, the bench or smoke().

A member row is (pos, len, kind) with kind = MEMBER_* | nibble << 8; an entry is (pos, dec).

    T = 40 + 24*nm + 16*(nb + 1)
    0          u32 0x184D2A5C, u32 P = T - 8
    8          nm     x { u64 pos, u64 len, u32 kind, u32 0 }      the table's own row is the last
    8 + 24*nm  nb + 1 x { u64 pos, u64 dec }
    T - 32     u64 nm, u64 nb, u64 file_len, u32 version = 1, u32 0x4B53345A
"""
import struct

import zig_lz4_file_range as ff

MAGIC, FOOTER_MAGIC, VERSION = 0x184D2A5C, 0x4B53345A, 1
SELF_KIND = ff.SKIPPABLE | 0xC << 8
INVALID_STATE, UNSUPPORTED, F_DST_MAX_SIZE_TOO_SMALL = -5, -8, -111
U64 = (1 << 64) - 1


def table_bytes(nm, nb):
    """T for nm member rows (the table's own among them) and nb + 1 entries"""
    return 40 + 24 * nm + 16 * (nb + 1)


def bound(nmembers, nblocks):
    """zlz4f_seek_table_bound: T for nmembers + 1 rows, 0 when P does not fit a u32"""
    T = table_bytes(nmembers + 1, nblocks)
    return T if T - 8 <= 0xFFFFFFFF else 0


def members(buf, legacy=True):
    """the rows of the record-mode split: (pos, len, kind | nibble << 8)"""
    buf = bytes(buf)
    out = []
    for pos, ln, kind in ff.split(buf, legacy):
        nib = (buf[pos] & 15) << 8 if kind in (ff.SKIPPABLE, ff.SKIPPABLE_TRUNCATED) else 0
        out.append((pos, ln, kind | nib))
    return out


def pack(rows, entries, file_len, nm=None, nb=None, version=VERSION, magic=MAGIC, payload=None, footer_magic=FOOTER_MAGIC,
         reserved=None):
    """The bytes of a table from its fields.  The defaults are the well-formed values; every argument overrides one field,
    which is how the tests make tables that are out of shape.  reserved: {row: word}."""
    nm = len(rows) if nm is None else nm
    nb = len(entries) - 1 if nb is None else nb
    T = 8 + 24 * len(rows) + 16 * len(entries) + 32
    out = struct.pack("<II", magic, T - 8 if payload is None else payload)
    for k, (pos, ln, kind) in enumerate(rows):
        out += struct.pack("<QQII", pos & U64, ln & U64, kind & 0xFFFFFFFF, (reserved or {}).get(k, 0))
    for pos, dec in entries:
        out += struct.pack("<QQ", pos & U64, dec & U64)
    return out + struct.pack("<QQQII", nm & U64, nb & U64, file_len & U64, version, footer_magic)


def append_refusal(buf, legacy=True, cap=None):
    """why zlz4f_batch_append_seek_table refuses the file (0: it does not).  A host split has no capacity, so its result
    is never negative; cap = the room of the buffer."""
    buf = bytes(buf)
    idx_n, entries = ff.file_index(buf, legacy)
    if idx_n < 0:
        return idx_n
    rows = members(buf, legacy)
    if rows and rows[-1][2] & 0xFF == ff.FRAME and entries[idx_n][0] + 4 > rows[-1][0] + rows[-1][1]:
        return INVALID_STATE                           # the chain lacks its end mark
    T = table_bytes(len(rows) + 1, idx_n)
    if T - 8 > 0xFFFFFFFF:
        return UNSUPPORTED
    if cap is not None and len(buf) + T > cap:
        return F_DST_MAX_SIZE_TOO_SMALL
    return 0


def table(buf, legacy=True, cap=None):
    """the table member that the append writes behind `buf` -> bytes, or the refusal's code"""
    buf = bytes(buf)
    why = append_refusal(buf, legacy, cap)
    if why:
        return why
    idx_n, entries = ff.file_index(buf, legacy)
    rows = members(buf, legacy)
    T = table_bytes(len(rows) + 1, idx_n)
    out = pack(rows + [(len(buf), T, SELF_KIND)], entries, len(buf) + T)
    assert len(out) == T
    return out


def _footer(buf):
    """-> None (no table), "malformed", or (nm, nb, T)"""
    n = len(buf)
    if n < 80 or int.from_bytes(buf[n - 4:], "little") != FOOTER_MAGIC:
        return None
    nm, nb, file_len, version = struct.unpack("<QQQI", buf[n - 32:n - 4])
    T = table_bytes(nm, nb)
    if version != VERSION or nm == 0 or T > U64 or T > n or file_len != n:
        return "malformed"
    if struct.unpack("<II", buf[n - T:n - T + 8]) != (MAGIC, T - 8):
        return "malformed"
    return nm, nb, T


def load(buf, mem_cap=None, idx_cap=None):
    """zlz4f_batch_load_seek_table for one file -> (split_result, rows, idx_n, entries); rows and entries are [] unless the
    split result is positive.  SHAPE ONLY is checked.  idx_cap: the entries left in the index for this file."""
    buf = bytes(buf)
    n = len(buf)
    f = _footer(buf)
    if f is None:
        return 0, [], INVALID_STATE, []
    bad = (INVALID_STATE, [], INVALID_STATE, [])
    if f == "malformed":
        return bad
    nm, nb, T = f
    if (mem_cap is not None and nm > mem_cap) or (idx_cap is not None and nb + 1 > idx_cap):
        return F_DST_MAX_SIZE_TOO_SMALL, [], F_DST_MAX_SIZE_TOO_SMALL, []
    at = n - T + 8
    raw = [struct.unpack("<QQII", buf[at + 24 * k:at + 24 * k + 24]) for k in range(nm)]
    at += 24 * nm
    entries = [struct.unpack("<QQ", buf[at + 16 * k:at + 16 * k + 16]) for k in range(nb + 1)]
    for k, (pos, ln, kind, rsv) in enumerate(raw):
        if rsv != 0 or ln == 0 or (k == 0 and pos != 0):
            return bad
        if k == nm - 1:
            if (pos, ln, kind) != (n - T, T, SELF_KIND):
                return bad
        elif kind & ~0xFFF or kind & 0xFF not in (ff.FRAME, ff.SKIPPABLE, ff.LEGACY) or pos + ln > U64 or pos + ln != raw[k + 1][0]:
            return bad
    for k, (pos, dec) in enumerate(entries):
        if pos > n - T or (k < nb and (entries[k + 1][0] <= pos or entries[k + 1][1] < dec)):
            return bad
    return nm, [r[:3] for r in raw], nb, entries


def rooms(buf):
    """count mode: (nm, room) of the file: (0, 0) without a well-formed footer"""
    f = _footer(bytes(buf))
    return (f[0], f[1] + 1) if isinstance(f, tuple) else (0, 0)


def concat(items, cap=None):
    """zlz4f_batch_concat for one file: items are bytes, or a negative int where the compress call failed -> bytes, or the
    first negative item in item order, or DstMaxSizeTooSmall against cap"""
    for it in items:
        if isinstance(it, int) and it < 0:
            return it
    out = b"".join(bytes(it) for it in items)
    if cap is not None and len(out) > cap:
        return F_DST_MAX_SIZE_TOO_SMALL
    return out


__all__ = ["bound", "members", "pack", "append_refusal", "table", "load", "rooms", "concat"]
