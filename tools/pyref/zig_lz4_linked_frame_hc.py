"""Python model of linked-block lz4f frames at the HC levels 3..9 (include/zlz4_amd.h: zlz4f_batch_compress_frame_ex with
ZLZ4F_BATCH_LINK_BLOCKS).  One statement over pieces that have a model of their own:

  block k of a frame = compress_hc_using_dict(block_k, dict = input[max(0, k * bs - 65536) : k * bs], level)
                       (zig_lz4_hc_dict.py), whether or not block k - 1 ended up stored;
  everything else as lz4f.compressFrame (src/lz4f.zig:354-446): the stored-block rule, the checksums, the header
  (zig_lz4_linked_frame.encode_header with block_mode 0) and the end mark.

Decoding is zig_lz4_linked_frame.decompress_frame_linked.  Test infrastructure like the other files here: never imported by
the product, the bench or smoke().
"""
from zig_lz4_hc_dict import ERR_UNSUPPORTED, compress_hc_using_dict, level_of
from zig_lz4_linked_frame import BLOCK_SIZES, HISTORY, encode_header
from zig_lz4_sizes import xxh32


def frame_level(level):
    """prefs.compression_level as the frame calls read it: <= 0 is the fast level (0), 1 becomes 9, above 12 becomes 12"""
    if level <= 0:
        return 0
    return 9 if level < 2 else min(level, 12)


def compress_frame_linked_hc(data, level, prefs=None, compress_block=None):
    """The frame zlz4f_batch_compress_frame_ex writes for `data` with ZLZ4F_BATCH_LINK_BLOCKS at an HC level, or
    ERR_UNSUPPORTED (-8) for the levels the dictionary compressor does not take (2, 10..12).  prefs: a dict of
    block_size_id, content_checksum, block_checksum, content_size, dict_id (block_mode is 0: linked).
    compress_block(block, dictionary, level) -> bytes: another statement of compress_hc_using_dict (the C restatement of
    the tests); default: the Python one."""
    data = bytes(data)
    level = frame_level(level)
    if level == 0 or level_of(level) == 0:
        return ERR_UNSUPPORTED
    if compress_block is None:
        compress_block = compress_hc_using_dict
    p = dict(prefs or {})
    bs = BLOCK_SIZES[p.get("block_size_id", 0)]
    bc, cc = p.get("block_checksum", 0) == 1, p.get("content_checksum", 0) == 1
    out = bytearray(encode_header(p.get("block_size_id", 0), 0, 1 if cc else 0, 1 if bc else 0, p.get("content_size", 0),
                                  p.get("dict_id", 0)))
    for start in range(0, len(data), bs):                              # :379-430
        block = data[start:start + bs]
        comp = compress_block(block, data[max(0, start - HISTORY):start], level)
        assert isinstance(comp, bytes) and len(comp) > 0
        if len(comp) >= len(block):                                    # :407 stored (the input stays the dictionary)
            body, head = block, len(block) | 0x80000000
        else:
            body, head = comp, len(comp)
        out += head.to_bytes(4, "little") + body
        if bc:                                                         # :417-421
            out += xxh32(body).to_bytes(4, "little")
    out += b"\0\0\0\0"                                                 # :433
    if cc:                                                             # :437-441
        out += xxh32(data).to_bytes(4, "little")
    return bytes(out)


def blocks_of(frame):
    """-> [(payload, stored)] of a frame this model wrote (no error handling: test helper)"""
    frame = bytes(frame)
    flg = frame[4]
    pos = 7 + (8 if flg & 0x08 else 0) + (4 if flg & 0x01 else 0)
    out = []
    while True:
        h = int.from_bytes(frame[pos:pos + 4], "little")
        pos += 4
        if h == 0:
            return out
        size = h & 0x7FFFFFFF
        out.append((frame[pos:pos + size], bool(h & 0x80000000)))
        pos += size + (4 if flg & 0x10 else 0)
