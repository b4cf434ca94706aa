"""Python restatement of lz4.StreamDecode (reference src/lz4.zig:870-957) with the decompressGeneric it calls
(:89-251), written from the Zig source (line cites per step).  Test infrastructure like zig_lz4_dict.py: never imported
by the product, the bench or smoke().

Addresses are modelled as integers.  decompress_generic takes lowPrefix as a SIGNED position relative to dst
(lowPrefix - dst.ptr), so a prefix above dst is a positive number.  Results: bytes produced, or the negative lz4.Error
code of the C ABI (-1 OutputTooSmall, -3 CorruptedData, -5 InvalidState).
"""
OUTPUT_TOO_SMALL, CORRUPTED, INVALID_STATE = -1, -3, -5
MINMATCH, ML_MASK, RUN_MASK = 4, 15, 15               # src/lz4.zig:12-21


def decompress_generic(src, dst_cap, low_prefix=0, dict_bytes=None, target=None):
    """decompressGeneric(src, dst, target, dst.ptr + low_prefix, dict) -> (result, bytes); dict_bytes None = null."""
    src = bytes(src)
    target = dst_cap if target is None else target
    if len(src) == 0:                                 # :97
        return 0, b""
    if dst_cap == 0:                                  # :98
        return 0, b""
    if target > dst_cap:                              # :99
        return OUTPUT_TOO_SMALL, b""
    have_dict = dict_bytes is not None                # :103
    dct = bytes(dict_bytes) if have_dict else b""
    dict_size = len(dct)                              # :104
    dst = bytearray()
    ip, iend, oend = 0, len(src), target
    while True:
        if ip >= iend:                                # :113
            break
        token = src[ip]; ip += 1                      # :116-117
        lit = token >> 4                              # :120
        if lit == RUN_MASK:                           # :123-131
            while True:
                if ip >= iend:
                    return CORRUPTED, b""
                s = src[ip]; ip += 1
                lit += s
                if s != 255:
                    break
        if lit > 0:                                   # :134-144
            if ip + lit > iend:
                return CORRUPTED, b""
            if len(dst) + lit > oend:
                return OUTPUT_TOO_SMALL, b""
            dst += src[ip:ip + lit]
            ip += lit
        if ip >= iend:                                # :146
            break
        if ip + 2 > iend:                             # :149
            return CORRUPTED, b""
        offset = src[ip] | (src[ip + 1] << 8); ip += 2   # :150-151
        if offset == 0:                               # :154
            return CORRUPTED, b""
        ml = token & ML_MASK                          # :157
        if ml == ML_MASK:                             # :160-168
            while True:
                if ip >= iend:
                    return CORRUPTED, b""
                s = src[ip]; ip += 1
                ml += s
                if s != 255:
                    break
        ml += MINMATCH                                # :171
        op = len(dst)
        if op + ml > oend:                            # :174
            return OUTPUT_TOO_SMALL, b""
        match = op - offset                           # :178-179 (relative to dst)
        if match < low_prefix:                        # :181
            if not have_dict:                         # :183-186
                return CORRUPTED, b""
            prefix_offset = op - low_prefix           # :189
            if offset > prefix_offset + dict_size:    # :190-192
                return CORRUPTED, b""
            lpo = low_prefix - match                  # :195
            start = dict_size - lpo                   # :196 dictEnd - lowPrefixOffset
            if ml <= lpo:                             # :199-202
                dst += dct[start:start + ml]
            else:                                     # :203-224
                dst += dct[start:]
                rest = ml - lpo
                rest_start = low_prefix               # :210
                for i in range(rest):                 # (both branches copy dst[restStart + i] in order)
                    dst.append(dst[rest_start + i])
        else:
            if offset > op:                           # :229-231
                return CORRUPTED, b""
            for i in range(ml):                       # :234-247
                dst.append(dst[match + i])
    return len(dst), bytes(dst)                       # :250


def decompress_safe(src, dst_cap):
    return decompress_generic(src, dst_cap)           # :257-259


class StreamDecode:
    """:870-951 over integer addresses.  `dicts` maps a dictionary address to its bytes (the model's memory)."""

    def __init__(self, dict_addr=0, dict_len=0, prefix=0, prefix_len=0, dict_bytes=None):
        self.dict, self.dict_len, self.prefix, self.prefix_len = dict_addr, dict_len, prefix, prefix_len
        self.dict_bytes = dict_bytes                  # the bytes at self.dict (any length >= dict_len)

    def state(self):
        return (self.dict, self.dict_len, self.prefix, self.prefix_len)

    def set_stream_decode(self, dict_addr, dict_bytes):
        """:904-909; dict_addr 0 = null (dict_bytes ignored)."""
        self.dict = dict_addr
        self.dict_bytes = bytes(dict_bytes) if dict_addr else None
        self.dict_len = len(self.dict_bytes) if dict_addr else 0
        self.prefix, self.prefix_len = 0, 0

    def kind(self, dst):
        """How the next call at dst decodes: ("A",), ("dict",), ("bound", lo) or ("invalid",)."""
        if self.prefix_len == 0 and self.dict_len == 0:   # :914
            return ("A",)
        if self.dict_len > 0 and self.prefix != 0:
            return ("invalid",)                       # (restStart underflow, :213)
        if self.dict_len > 0 and self.dict != 0:
            return ("dict",)
        low = self.prefix if self.prefix else dst     # :921-924
        return ("bound", low - dst)

    def decompress_safe_continue(self, src, dst, dst_cap):
        """:912-939 -> (result, bytes); the state changes only on success."""
        k = self.kind(dst)
        if k[0] == "A":
            r, out = decompress_safe(src, dst_cap)    # :916
            if r >= 0:
                self.prefix, self.prefix_len = dst, r   # :918-919
            return r, out
        if k[0] == "invalid":
            return INVALID_STATE, b""
        if k[0] == "dict":                            # lowPrefix = dst (prefix null), dict = externalDict (:924-930)
            r, out = decompress_generic(src, dst_cap, 0, self.dict_bytes[:self.dict_len])
        else:
            r, out = decompress_generic(src, dst_cap, k[1], None)
        if r >= 0:                                    # :933-938
            self.prefix, self.prefix_len = dst, r
            self.dict, self.dict_len, self.dict_bytes = 0, 0, None
        return r, out


def decoder_ring_buffer_size(max_block_size):         # :954-957
    return 0 if max_block_size == 0 else 65536 + 14 + max_block_size


def replay(state, calls):
    """state: StreamDecode; calls: [(src, dst_addr, dst_cap)] -> [(result, bytes)] (state updated)."""
    return [state.decompress_safe_continue(s, d, c) for s, d, c in calls]
