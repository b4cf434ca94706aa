"""Python restatement of decompressGeneric WITH its dictionary branch (reference src/lz4.zig:89-251), i.e. of
lz4.decompressSafeUsingDict (:960-962) and lz4.decompressSafePartialUsingDict (:967-969).

Test infrastructure like zig_lz4_pyref.py: written from the Zig source (line cites per step), never imported by the
product, the bench or smoke().  The tests use it for the expected bytes and statuses of dictionary streams, malformed
ones included.  Results: the number of bytes produced, or the negative lz4.Error code of the C ABI (-1 OutputTooSmall,
-3 CorruptedData).  What lies in `dst` after an error is unspecified in the reference and not returned here.
"""
OUTPUT_TOO_SMALL, CORRUPTED = -1, -3                  # lz4.Error order, src/lz4.zig:48-55 (include/zlz4_amd.h)
MINMATCH, ML_BITS, ML_MASK, RUN_MASK = 4, 4, 15, 15   # src/lz4.zig:12-21


def decompress_generic(src, dst_cap, target, dict_bytes):
    """-> (result, bytes).  `dict_bytes` None = no dictionary (decompressSafe); b"" = an empty one (dictEnd set,
    dictSize 0).  bytes is dst[:result] on success, b"" on an error."""
    src = bytes(src)
    if len(src) == 0:                                 # :97
        return 0, b""
    if dst_cap == 0:                                  # :98
        return 0, b""
    if target > dst_cap:                              # :99
        return OUTPUT_TOO_SMALL, b""
    have_dict = dict_bytes is not None                # :103 dictEnd
    dct = bytes(dict_bytes) if have_dict else b""
    dict_size = len(dct)                              # :104
    dst = bytearray()
    ip, iend, oend = 0, len(src), target              # :106-109
    while True:
        if ip >= iend:                                # :113
            break
        token = src[ip]                               # :116
        ip += 1
        lit = token >> ML_BITS                        # :120
        if lit == RUN_MASK:                           # :123-131
            while True:
                if ip >= iend:
                    return CORRUPTED, b""
                s = src[ip]
                ip += 1
                lit += s
                if s != 255:
                    break
        if lit > 0:                                   # :134
            if ip + lit > iend:                       # :136
                return CORRUPTED, b""
            if len(dst) + lit > oend:                 # :137
                return OUTPUT_TOO_SMALL, b""
            dst += src[ip:ip + lit]                   # :140
            ip += lit
        if ip >= iend:                                # :146
            break
        if ip + 2 > iend:                             # :149
            return CORRUPTED, b""
        offset = src[ip] | (src[ip + 1] << 8)         # :150
        ip += 2
        if offset == 0:                               # :154
            return CORRUPTED, b""
        ml = token & ML_MASK                          # :157
        if ml == ML_MASK:                             # :160-168
            while True:
                if ip >= iend:
                    return CORRUPTED, b""
                s = src[ip]
                ip += 1
                ml += s
                if s != 255:
                    break
        ml += MINMATCH                                # :171
        op = len(dst)
        if op + ml > oend:                            # :174
            return OUTPUT_TOO_SMALL, b""
        if offset > op:                               # :181 matchPtr < lowPrefix (lowPrefix == dst.ptr)
            if not have_dict:                         # :183
                return CORRUPTED, b""
            if offset > op + dict_size:               # :189-192
                return CORRUPTED, b""
            low = offset - op                         # :195 lowPrefixOffset
            dm = dict_size - low                      # :196 dictMatchPtr
            if ml <= low:                             # :199-202 wholly in the dictionary
                dst += dct[dm:dm + ml]
            else:                                     # :203-225 spans the dictionary end
                dst += dct[dm:dict_size]
                rest = ml - low
                op = len(dst)
                for i in range(rest):                 # :213-217 byte by byte (the memcpy of :220 is the same bytes)
                    dst.append(dst[i])
        else:                                         # :226-248
            mp = op - offset
            if offset >= ml:                          # :244-247 disjoint
                dst += dst[mp:mp + ml]
            else:                                     # :235-241 overlap, byte by byte
                for i in range(ml):
                    dst.append(dst[mp + i])
    return len(dst), bytes(dst)                       # :250


def decompress_safe_using_dict(src, dst_cap, dict_bytes):
    """lz4.decompressSafeUsingDict, src/lz4.zig:960-962."""
    return decompress_generic(src, dst_cap, dst_cap, dict_bytes)


def decompress_safe_partial_using_dict(src, dst_cap, target, dict_bytes):
    """lz4.decompressSafePartialUsingDict, src/lz4.zig:967-969."""
    return decompress_generic(src, dst_cap, target, dict_bytes)
