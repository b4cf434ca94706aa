"""Python model of lz4f dictionary frames (include/zlz4_amd.h: the zlz4f_*_using_dict calls).
The reference has no counterpart; liblz4 has (LZ4F_compressFrame_usingCDict, LZ4F_decompress_usingDict), and the model is
two statements over pieces that are modelled already.  T = the last min(len(dict), 65536) bytes of the dictionary:

  decode     a frame whose FLG has the block-independence bit (0x20) set: block k =
             decompress_safe_using_dict(block_k, dst[pos:cap], dict = T) -- every block sees the dictionary;
             a frame with the bit clear: dict = the last 65536 bytes of T ++ dst[0:pos].
             Everything else is the walk of zig_lz4_linked_frame (src/lz4f.zig:541-638); the header's dictID is not read.
  compress   block_mode 1: block k = compress_fast_using_dict(block_k, dict = T) for every k;
             block_mode 0: block 0 the same, block k >= 1 against input[k * bs - 65536 : k * bs] (compress_frame_linked);
             header (with prefs' dict_id), stored-block rule, checksums and end mark as lz4f.compressFrame.

With an empty dictionary the two are decompress_frame_linked and compress_frame_linked / compressFrame.  Test
infrastructure like the other files here: never imported by the product, the bench or smoke().  Results: bytes, or the
negative code of the C ABI.
"""
from zig_lz4_dict import decompress_safe_using_dict
from zig_lz4_dict_compress import compress_fast_using_dict
from zig_lz4_linked_frame import BLOCK_SIZES, HISTORY, _walk, encode_header
from zig_lz4_sizes import block_size, xxh32


def _tail(dict_bytes):
    return bytes(dict_bytes or b"")[-HISTORY:]


def _history(T, history):
    """The dictionary a block decodes with; `history` is _walk's: None for an independent frame, else the last 65536
    bytes of the frame's output so far."""
    if history is None:
        return T if T else None                                        # (no dictionary: decompressSafe)
    return (T + history)[-HISTORY:]


def decompress_frame_using_dict(frame, cap, dict_bytes):
    """What zlz4f_batch_decompress_frame_using_dict gives for `frame` into `cap` bytes -> (result, bytes)."""
    T = _tail(dict_bytes)

    def decode(block, room, history):
        return decompress_safe_using_dict(block, room, _history(T, history))
    return _walk(frame, cap, decode)


def frame_size_using_dict(frame, dict_len):
    """What zlz4f_batch_frame_decompressed_size_using_dict gives: the walk without output, a block by its size under the
    length of its dictionary; the content checksum is not verified."""
    T = b"\0" * min(int(dict_len), HISTORY)

    def decode(block, room, history):
        h = _history(T, history)
        r = block_size(block, None if h is None else len(h))
        return r, (b"\0" * r if r > 0 else b"")
    return _walk(frame, None, decode)[0]


def compress_frame_using_dict(data, dict_bytes, prefs=None):
    """The frame zlz4f_batch_compress_frame_using_dict writes for `data`.  prefs: a dict of block_size_id, block_mode,
    content_checksum, block_checksum, content_size, dict_id (the fast level)."""
    data, T = bytes(data), _tail(dict_bytes)
    p = dict(prefs or {})
    bs = BLOCK_SIZES[p.get("block_size_id", 0)]
    independent = p.get("block_mode", 0) == 1
    bc, cc = p.get("block_checksum", 0) == 1, p.get("content_checksum", 0) == 1
    out = bytearray(encode_header(p.get("block_size_id", 0), 1 if independent else 0, 1 if cc else 0, 1 if bc else 0,
                                  p.get("content_size", 0), p.get("dict_id", 0)))
    for start in range(0, len(data), bs):                              # src/lz4f.zig:379-430
        block = data[start:start + bs]
        d = T if independent or start == 0 else data[start - HISTORY:start]
        r, comp = compress_fast_using_dict(block, d, 1)
        assert r == len(comp) and r > 0
        if r >= len(block):                                            # :407 stored
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
