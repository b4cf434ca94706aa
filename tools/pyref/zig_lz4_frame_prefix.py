"""Model of frame prefix decoding, FP(frame, n, T) of DESIGN.md section 4.4f -- what zlz4f_decompress_frame_prefix(_using_dict)
and the two batch calls return: the first n bytes of an lz4f frame, history-aware, by a walk that ends at the cut.

Composed from the models that exist: the header parse and XXH32 of zig_lz4_sizes (src/lz4f.zig:483-538), the history rule of
zig_lz4_dict_frame (T = the dictionary's last 65536 bytes; FLG bit 0x20 set: every block sees T alone, clear: the last 65536
bytes of T ++ output) and P(block, cap, hist) of zig_lz4_prefix (section 4.2e).  The walk is written out here with the
reference's line cites, because the stop rule stands inside it.  Test infrastructure like the other files here: written from
the specification, independent of the kernel, never imported by the product, the bench or smoke().

Results: (number of bytes, bytes) or (a negative code of the C ABI, b"").  Never DstMaxSizeTooSmall, never OutputTooSmall.
"""
from zig_lz4_dict_frame import _history, _tail
from zig_lz4_linked_frame import F_CONTENT_CHECKSUM_INVALID, HISTORY
from zig_lz4_prefix import decompress_prefix
from zig_lz4_sizes import (F_BLOCK_CHECKSUM_INVALID, F_DECOMPRESSION_FAILED, F_FRAME_SIZE_WRONG, _parse_header, xxh32)


def decompress_frame_prefix(frame, n, dict_bytes=None):
    """-> (result, bytes): the first `n` bytes of the frame's content.  dict_bytes None or b"" = no dictionary (D = 0)."""
    src, T = bytes(frame), _tail(dict_bytes)
    ph = _parse_header(src)                                            # 1. :547; a header error also when n == 0
    if not isinstance(ph, tuple):
        return ph, b""
    flg, pos = ph
    linked = not (flg & 0x20)
    end, dst = len(src), bytearray()
    while True:
        if len(dst) == n:                                              # 2. the stop rule: nothing behind is read
            return n, bytes(dst)
        if pos >= end:                                                 # 3. :563 input ends at a block boundary
            break
        if pos + 4 > end:                                              # :565
            return F_FRAME_SIZE_WRONG, b""
        h = int.from_bytes(src[pos:pos + 4], "little")
        pos += 4
        if h == 0:                                                     # :573 the end mark
            break
        size = h & 0x7FFFFFFF
        if pos + size > end:                                           # :582
            return F_FRAME_SIZE_WRONG, b""
        block = src[pos:pos + size]
        pos += size
        if flg & 0x10:                                                 # 4. :590-598: the whole block, before the decode
            if pos + 4 > end:
                return F_FRAME_SIZE_WRONG, b""
            if int.from_bytes(src[pos:pos + 4], "little") != xxh32(block):
                return F_BLOCK_CHECKSUM_INVALID, b""
            pos += 4
        room = n - len(dst)
        if h & 0x80000000:                                             # 5. :603-608 stored: what fits; history
            dst += block[:room]
        else:                                                          # 6. :610-613
            hist = _history(T, bytes(dst[-HISTORY:]) if linked else None)
            r, got = decompress_prefix(block, min(room, 0xFFFFFFFF), hist)
            if r < 0:
                return F_DECOMPRESSION_FAILED, b""                     # :611
            dst += got
    if flg & 0x04:                                                     # 7. the whole frame is out: :625-635
        if pos + 4 > end:
            return F_FRAME_SIZE_WRONG, b""
        if int.from_bytes(src[pos:pos + 4], "little") != xxh32(dst):
            return F_CONTENT_CHECKSUM_INVALID, b""
    return len(dst), bytes(dst)
