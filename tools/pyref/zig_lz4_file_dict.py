"""Model of the dictionary forms of the file calls (include/zlz4_amd.h:
zlz4f_batch_file_index_using_dict, zlz4f_batch_decompress_file_range_using_dict, zlz4f_decompress_file_range_using_dict).

ONE RULE.  A file has at most one dictionary; T is its last D = min(len, 65536) bytes.  Which blocks see T:
  - a legacy member: none;
  - a frame member whose FLG has the block-independence bit (0x20) set: every block;
  - a frame member with the bit clear: block 0 only, the block whose word stands at the end of the member's header; the
    later blocks are sized and decoded as independent blocks without a dictionary, as the plain file calls do.
With D == 0 everything here equals zig_lz4_file_range.

Written from that rule on top of zig_lz4_file_range (the split, the fold over the members, the range checks) and
zig_lz4_dict / zig_lz4_prefix / zig_lz4_sizes (the block decoders and the size pass with a dictionary).  Test
infrastructure like the other files of this directory: never imported by the product, the bench or smoke().
"""
import functools

import zig_lz4_file_range as ff
import zig_lz4_frame_range as fr
from zig_lz4_sizes import block_size

HISTORY = 65536
INVALID_STATE = ff.INVALID_STATE


def tail(dict_bytes):
    """T: the part of the dictionary an offset can reach"""
    return bytes(dict_bytes or b"")[-HISTORY:]


@functools.lru_cache(maxsize=4096)
def _frame_member(body, D):
    """the frame index of one frame member whose blocks see a dictionary of D bytes where the rule says so"""
    ph = fr._header(bytes(body[:19]))
    if not isinstance(ph, tuple):
        return fr.frame_index(body)
    flg, first = ph
    independent = bool(flg & 0x20)
    word = int.from_bytes(body[first:first + 4], "little") if first + 4 <= len(body) else 0
    state = {"next": 1 if word >> 31 else 0}          # the block the next call of the sizer is for, when it is block 0
                                                      # (a stored block is not sized: block 0 stored -> no call is block 0)

    def sizer(data, dec):
        k0 = state["next"] == 0
        state["next"] += 1
        return block_size(data, D) if independent or k0 else block_size(data)
    return fr.frame_index(body, sizer=sizer)


def file_index(buf, dict_len=0, legacy=True, idx_cap=None):
    """zlz4f_batch_file_index_using_dict for one buffer whose dictionary has dict_len bytes -> (idx_n, entries)"""
    D = min(int(dict_len), HISTORY)
    if D == 0:
        return ff.file_index(buf, legacy, idx_cap)
    return ff.file_index(buf, legacy, idx_cap, frame_member=lambda body: _frame_member(body, D))


def sees(buf, members, pos):
    """SEES for the block whose word stands at `pos` (a position k_ffr_range has accepted): the member by the kernels'
    bisection, then the rule"""
    lo, hi = 0, len(members)
    while lo < hi:
        mid = lo + (hi - lo) // 2
        if members[mid][0] <= pos:
            lo = mid + 1
        else:
            hi = mid
    if lo == 0:
        return False
    mpos, mlen, kind = members[lo - 1]
    if kind != ff.FRAME:
        return False
    ph = fr._header(bytes(buf[mpos:mpos + min(mlen, 19)]))
    if not isinstance(ph, tuple):
        return False
    return bool(ph[0] & 0x20) or pos == mpos + ph[1]


def decompress_file_range(buf, members, entries, idx_n, a, b, dict_bytes=b"", dst_cap=None, reserved=0, buf_ok=True,
                          fits=True, dict_ok=True):
    """zlz4f_batch_decompress_file_range_using_dict for one range -> (result, skip, slot bytes).  dict_ok False: the
    range's file names no dictionary (d_dict_idx >= ndicts), a refusal of step 1."""
    if not dict_ok:
        return INVALID_STATE, 0, b""
    T = tail(dict_bytes)
    buf = bytes(buf)
    hook = (lambda pos: T if sees(buf, members, pos) else b"") if T else None
    return ff.decompress_file_range(buf, members, entries, idx_n, a, b, dst_cap, reserved, buf_ok, fits, block_dict=hook)


def file_range(buf, a, b, dict_bytes=b"", legacy=True, split_flags=None):
    """The host call zlz4f_decompress_file_range_using_dict without a seek table -> (result, bytes)"""
    if split_flags is not None:
        if split_flags & ~1:
            return ff.F_PARAMETER_INVALID, b""
        legacy = bool(split_flags & 1)
    if a > b:
        return INVALID_STATE, b""
    buf = bytes(buf)
    idx_n, entries = file_index(buf, len(dict_bytes or b""), legacy)
    if idx_n < 0:
        return idx_n, b""
    r, skip, slot = decompress_file_range(buf, ff.split(buf, legacy), entries, idx_n, a, b, dict_bytes)
    return (r, slot[skip:skip + r]) if r >= 0 else (r, b"")


def file_content(buf, dict_bytes=b"", legacy=True):
    """the whole content under the model's index: the range [0, S) -> (result, bytes)"""
    return file_range(buf, 0, 1 << 62, dict_bytes, legacy)


__all__ = ["tail", "file_index", "sees", "decompress_file_range", "file_range", "file_content"]
