"""Python model of linked-block lz4f frames (include/zlz4_amd.h: ZLZ4F_BATCH_LINK_BLOCKS, ZLZ4F_DECODE_LINKED; DESIGN.md
section 4.4c).  The reference has no counterpart (its block_mode is a header bit only, src/lz4f.zig:159-161, :610), so the
model is two statements over pieces that do have one:

  compress   block k of a frame = compress_fast_using_dict(block_k, dict = input[max(0, k * bs - 65536) : k * bs]),
             everything else as lz4f.compressFrame (src/lz4f.zig:354-446);
  decode     a frame whose FLG has the block-independence bit (0x20) clear: block k =
             decompress_safe_using_dict(block_k, dst[pos:cap], dict = dst[max(0, pos - 65536) : pos]);
             a frame with the bit set: lz4f.decompressFrame (src/lz4f.zig:541-638), every block on its own.

Composed from zig_lz4_sizes (header parse, XXH32, block sizes), zig_lz4_dict (the dictionary decoder) and
zig_lz4_dict_compress (the dictionary compressor).  Test infrastructure like the other files here: never imported by the
product, the bench or smoke().  Results: bytes, or the negative code of the C ABI.
"""
from zig_lz4_dict import decompress_safe_using_dict
from zig_lz4_dict_compress import compress_fast_using_dict
from zig_lz4_sizes import (F_BLOCK_CHECKSUM_INVALID, F_DECOMPRESSION_FAILED, F_FRAME_SIZE_WRONG, MAGIC, _parse_header,
                           block_size, xxh32)

F_DST_MAX_SIZE_TOO_SMALL, F_CONTENT_CHECKSUM_INVALID = -111, -118        # src/lz4f.zig:31-55
HISTORY = 64 * 1024
BLOCK_SIZES = {0: 64 << 10, 4: 64 << 10, 5: 256 << 10, 6: 1 << 20, 7: 4 << 20}   # BlockSizeID.toBlockSize, :64-79


def encode_header(block_size_id=0, block_mode=0, content_checksum=0, block_checksum=0, content_size=0, dict_id=0):
    """encodeFrameHeader, src/lz4f.zig:304-351 (block_size_id 0 is written as 4, :64-79)."""
    flg = (1 << 6) | ((block_mode & 1) << 5) | ((block_checksum & 1) << 4) | ((1 if content_size else 0) << 3) \
        | ((content_checksum & 1) << 2) | (1 if dict_id else 0)
    bd = ((block_size_id or 4) & 7) << 4
    desc = bytes([flg, bd])
    if content_size:
        desc += content_size.to_bytes(8, "little")
    if dict_id:
        desc += dict_id.to_bytes(4, "little")
    return MAGIC.to_bytes(4, "little") + desc + bytes([(xxh32(desc) >> 8) & 0xFF])


def compress_frame_linked(data, prefs=None):
    """The frame zlz4f_batch_compress_frame writes for `data` with ZLZ4F_BATCH_LINK_BLOCKS.  prefs: a dict of
    block_size_id, content_checksum, block_checksum, content_size, dict_id (block_mode is 0: linked)."""
    data = bytes(data)
    p = dict(prefs or {})
    bs = BLOCK_SIZES[p.get("block_size_id", 0)]
    bc, cc = p.get("block_checksum", 0) == 1, p.get("content_checksum", 0) == 1
    out = bytearray(encode_header(p.get("block_size_id", 0), 0, 1 if cc else 0, 1 if bc else 0, p.get("content_size", 0),
                                  p.get("dict_id", 0)))
    for start in range(0, len(data), bs):                              # :379-430
        block = data[start:start + bs]
        r, comp = compress_fast_using_dict(block, data[max(0, start - HISTORY):start], 1)
        assert r == len(comp) and r > 0
        if r >= len(block):                                            # :407 stored (the input stays the dictionary)
            body, head = block, len(block) | 0x80000000
        else:
            body, head = comp, r
        out += head.to_bytes(4, "little") + body
        if bc:                                                         # :417-421
            out += xxh32(body).to_bytes(4, "little")
    out += b"\0\0\0\0"                                                 # :433
    if cc:                                                             # :437-441
        out += xxh32(data).to_bytes(4, "little")
    return bytes(out)


def _walk(frame, cap, decode):
    """src/lz4f.zig:541-638 -> (result, output).  decode(block, room, history) -> (size or a negative code, bytes); cap
    None = a destination that is never too small, without the content checksum (the size query)."""
    src = bytes(frame)
    ph = _parse_header(src)                                            # :547
    if not isinstance(ph, tuple):
        return ph, b""
    flg, pos = ph
    linked = not (flg & 0x20)
    n, dst = len(src), bytearray()
    while pos < n:                                                     # :563
        if pos + 4 > n:                                                # :565
            return F_FRAME_SIZE_WRONG, b""
        h = int.from_bytes(src[pos:pos + 4], "little")
        pos += 4
        if h == 0:                                                     # :573
            break
        size = h & 0x7FFFFFFF
        if pos + size > n:                                             # :582
            return F_FRAME_SIZE_WRONG, b""
        block = src[pos:pos + size]
        pos += size
        if flg & 0x10:                                                 # :590-598
            if pos + 4 > n:
                return F_FRAME_SIZE_WRONG, b""
            if int.from_bytes(src[pos:pos + 4], "little") != xxh32(block):
                return F_BLOCK_CHECKSUM_INVALID, b""
            pos += 4
        room = None if cap is None else cap - len(dst)
        if h & 0x80000000:                                             # :603-608 stored: history for later blocks
            if room is not None and size > room:
                return F_DST_MAX_SIZE_TOO_SMALL, b""
            dst += block
        else:                                                          # :610-613
            r, got = decode(block, room, bytes(dst[-HISTORY:]) if linked and dst else (b"" if linked else None))
            if r < 0:
                return F_DECOMPRESSION_FAILED, b""
            dst += got
    if flg & 0x04:                                                     # :625-635
        if pos + 4 > n:
            return F_FRAME_SIZE_WRONG, b""
        if cap is not None and int.from_bytes(src[pos:pos + 4], "little") != xxh32(dst):
            return F_CONTENT_CHECKSUM_INVALID, b""
    return len(dst), bytes(dst)                                        # :637


def decompress_frame_linked(frame, cap):
    """What zlz4f_batch_decompress_frame_ex(ZLZ4F_DECODE_LINKED) gives for `frame` into `cap` bytes -> (result, bytes)."""
    def decode(block, room, history):
        return decompress_safe_using_dict(block, room, history)        # (history None: decompressSafe)
    return _walk(frame, cap, decode)


def frame_size_linked(frame):
    """What zlz4f_batch_frame_decompressed_size_ex(ZLZ4F_DECODE_LINKED) gives for `frame`: the walk without output, block k
    by its size under dict_len = min(pos, 65536); the content checksum is not verified."""
    def decode(block, room, history):
        r = block_size(block, None if history is None else len(history))
        return r, (b"\0" * r if r > 0 else b"")
    return _walk(frame, None, decode)[0]
