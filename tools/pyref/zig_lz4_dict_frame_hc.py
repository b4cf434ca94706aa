"""Python model of lz4f dictionary frames at the HC levels 3..9 (include/zlz4_amd.h: the zlz4f_*_using_dict_ex compress
calls).  What `lz4 -9 -D dict` and LZ4F_compressFrame_usingCDict with a level produce in liblz4;
the reference has no counterpart.  The loop of zig_lz4_dict_frame.compress_frame_using_dict with the block compressor of
zig_lz4_hc_dict.py.  T = the last min(len(dict), 65536) bytes of the dictionary:

  block_mode 1: block k = compress_hc_using_dict(block_k, dict = T, level) for every k;
  block_mode 0: block 0 the same, block k >= 1 against input[k * bs - 65536 : k * bs] (compress_frame_linked_hc: block
                sizes are >= 64 KiB, so T is out of reach from block 1 on);
  header (with prefs' dict_id), stored-block rule, checksums and end mark as lz4f.compressFrame.

Decoding is zig_lz4_dict_frame.decompress_frame_using_dict.  Test infrastructure like the other files here: never imported
by the product, the bench or smoke().  Results: bytes, or the negative code of the C ABI.
"""
from zig_lz4_hc_dict import ERR_UNSUPPORTED, compress_hc_using_dict, level_of
from zig_lz4_linked_frame import BLOCK_SIZES, HISTORY, encode_header
from zig_lz4_linked_frame_hc import frame_level
from zig_lz4_sizes import xxh32


def block_dict(data, dict_bytes, start, independent):
    """the dictionary of the block that starts at input position `start`"""
    if independent or start == 0:
        return bytes(dict_bytes or b"")[-HISTORY:]
    return bytes(data[start - HISTORY:start])


def compress_frame_using_dict_hc(data, dict_bytes, level, prefs=None, compress_block=None):
    """The frame zlz4f_batch_compress_frame_using_dict_ex writes for `data` at an HC level, or ERR_UNSUPPORTED (-8) for
    the levels the dictionary compressor does not take (2, 10..12).  `level` is prefs.compression_level as given (1 becomes
    9); the fast level (<= 0) is zig_lz4_dict_frame.compress_frame_using_dict's business and is refused here too.  prefs: a
    dict of block_size_id, block_mode, content_checksum, block_checksum, content_size, dict_id.
    compress_block(block, dictionary, level) -> bytes: another statement of compress_hc_using_dict (the C restatement of the
    tests); default: the Python one."""
    data = bytes(data)
    level = frame_level(level)
    if level == 0 or level_of(level) == 0:
        return ERR_UNSUPPORTED
    if compress_block is None:
        compress_block = compress_hc_using_dict
    p = dict(prefs or {})
    bs = BLOCK_SIZES[p.get("block_size_id", 0)]
    independent = p.get("block_mode", 0) == 1
    bc, cc = p.get("block_checksum", 0) == 1, p.get("content_checksum", 0) == 1
    out = bytearray(encode_header(p.get("block_size_id", 0), 1 if independent else 0, 1 if cc else 0, 1 if bc else 0,
                                  p.get("content_size", 0), p.get("dict_id", 0)))
    for start in range(0, len(data), bs):                              # src/lz4f.zig:379-430
        block = data[start:start + bs]
        comp = compress_block(block, block_dict(data, dict_bytes, start, independent), level)
        assert isinstance(comp, bytes) and len(comp) > 0
        if len(comp) >= len(block):                                    # :407 stored
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
