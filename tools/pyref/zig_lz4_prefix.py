"""Model of prefix decoding, P(src, cap, hist): decompressGeneric (reference src/lz4.zig:89-251) with oend = cap and the
named changes of DESIGN.md section 4.2e -- what zlz4_decompress_safe_prefix(_using_dict) and the two batch calls return.

Test infrastructure like zig_lz4_dict.py: written from the specification with the reference's line cites, independent of
the kernel, never imported by the product, the bench or smoke().  Results: the number of bytes produced, or -3
(CorruptedData); never OutputTooSmall.  On an error the bytes produced so far are not returned.

A single literal or match length saturates at 0xFFFF0000 in the device decoders; the model counts exactly, so it states
the contract for streams in which no single length passes that value.
"""
CORRUPTED = -3                                        # lz4.Error order, src/lz4.zig:48-55 (include/zlz4_amd.h)
MINMATCH, ML_BITS, ML_MASK, RUN_MASK = 4, 4, 15, 15   # src/lz4.zig:12-21


def decompress_prefix(src, cap, dict_bytes=None):
    """-> (result, bytes): the first `cap` bytes of the block.  dict_bytes None or b"" = no reachable dictionary (hist
    0); else hist = min(len(dict_bytes), 65536), the tail that an offset <= 65535 can reach."""
    src = bytes(src)
    if len(src) == 0:                                 # :97
        return 0, b""
    if cap == 0:                                      # :98
        return 0, b""
    dct = bytes(dict_bytes or b"")[-65536:]
    hist = len(dct)
    out = bytearray()
    ip, iend = 0, len(src)
    while True:
        if ip >= iend:                                # :113
            break
        if len(out) == cap:                           # stop rule, at the top of the loop
            break
        token = src[ip]                               # :116
        ip += 1
        lit = token >> ML_BITS                        # :120
        if lit == RUN_MASK:                           # :123-131, unchanged
            while True:
                if ip >= iend:
                    return CORRUPTED, b""
                s = src[ip]
                ip += 1
                lit += s
                if s != 255:
                    break
        if lit > 0:                                   # :134
            if ip + lit > iend:                       # :136, unchanged: even when the cut falls inside the run
                return CORRUPTED, b""
            n = min(lit, cap - len(out))              # :137 becomes: the literals that fit
            out += src[ip:ip + n]                     # :140
            ip += lit
            if len(out) == cap:                       # stop rule, right after the literal copy: nothing behind is read
                break
        if ip >= iend:                                # :146
            break
        if ip + 2 > iend:                             # :149
            return CORRUPTED, b""
        offset = src[ip] | (src[ip + 1] << 8)         # :150
        ip += 2
        if offset == 0:                               # :154
            return CORRUPTED, b""
        ml = token & ML_MASK                          # :157
        if ml == ML_MASK:                             # :160-168, unchanged
            while True:
                if ip >= iend:
                    return CORRUPTED, b""
                s = src[ip]
                ip += 1
                ml += s
                if s != 255:
                    break
        ml += MINMATCH                                # :171
        op = len(out)                                 # (:174 is dropped)
        if offset > op + hist:                        # :181-192 / :231 on the full offset
            return CORRUPTED, b""
        n = min(ml, cap - op)
        j0 = hist + op - offset                       # out[op + k] = W[j0 + k], W = dict tail ++ out, byte by byte
        if j0 >= hist and offset >= n:                # (source and destination disjoint, all in out: the same as a slice)
            out += out[j0 - hist:j0 - hist + n]
        else:
            for k in range(n):
                j = j0 + k
                out.append(dct[j] if j < hist else out[j - hist])
        # stop rule, right after the match copy: the test at the top of the loop
    return len(out), bytes(out)                       # :250, or cap
