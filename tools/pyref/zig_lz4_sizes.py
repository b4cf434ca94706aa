"""Python restatement of the decompressed-size queries: what lz4.decompressSafe / decompressSafeUsingDict (reference
src/lz4.zig:89-251, :257-259, :960-962) and lz4f.decompressFrame (src/lz4f.zig:541-638) RETURN, computed without an
output buffer.

Test infrastructure like zig_lz4_pyref.py and zig_lz4_dict.py: written from the Zig source (line cites per step), never
imported by the product, the bench or smoke().  It shares no code with those two files (the decoders there build the
output; this walk only counts), so the tests can hold them against each other.  Results: a size, or the negative code of
the C ABI (include/zlz4_amd.h).

Block query: decompressGeneric into a destination of BLOCK_CAP = 0xFFFFFFFF bytes, the library's per-block limit.  A
dictionary takes part by its length alone (:189-192 is the only place it is consulted before a byte is copied).
Frame query: decompressFrame into a destination that is never too small, with ONE stated exception: the content
checksum (:629-633) is a hash of the decoded bytes and is not verified -- a frame whose only defect is a wrong content
checksum reports its size.
"""
OUTPUT_TOO_SMALL, CORRUPTED = -1, -3                  # lz4.Error order, src/lz4.zig:48-55
BLOCK_CAP = 0xFFFFFFFF                                # capacities are 32-bit

# lz4f.Error (src/lz4f.zig:31-55): -(100 + 1-based declaration index)
F_MAX_BLOCK_SIZE_INVALID, F_HEADER_VERSION_WRONG, F_BLOCK_CHECKSUM_INVALID, F_RESERVED_FLAG_SET = -102, -106, -107, -108
F_FRAME_HEADER_INCOMPLETE, F_FRAME_TYPE_UNKNOWN, F_FRAME_SIZE_WRONG, F_DECOMPRESSION_FAILED = -112, -113, -114, -116
F_HEADER_CHECKSUM_INVALID = -117
MAGIC = 0x184D2204                                    # src/lz4f.zig:12


def _length(src, ip, iend, n):
    """The 255-run after a saturated nibble (:123-131 / :160-168) -> (value, ip), or (None, ip) when the input ends."""
    while True:
        if ip >= iend:                                # :125 / :162
            return None, ip
        s = src[ip]
        ip += 1
        n += s
        if s != 255:
            return n, ip


def block_size(src, dict_len=None, cap=BLOCK_CAP, reach=None):
    """What decompressSafe(src, dst) returns for dst.len == cap (dict_len None), or decompressSafeUsingDict with a
    dictionary of dict_len bytes.  `reach` (a list) receives offset - op of every match that starts in front of dst and
    passes :189-192: max(reach) is the shortest dictionary the stream decodes with."""
    src = bytes(src)
    iend = len(src)
    if iend == 0:                                     # :97
        return 0
    if cap == 0:                                      # :98
        return 0
    ip = op = 0
    while True:
        if ip >= iend:                                # :113
            break
        token = src[ip]                               # :116
        ip += 1
        lit = token >> 4                              # :120
        if lit == 15:
            lit, ip = _length(src, ip, iend, lit)
            if lit is None:
                return CORRUPTED
        if lit > 0:                                   # :134
            if ip + lit > iend:                       # :136
                return CORRUPTED
            if op + lit > cap:                        # :137
                return OUTPUT_TOO_SMALL
            ip += lit                                 # :140-142 (nothing is copied here)
            op += lit
        if ip >= iend:                                # :146
            break
        if ip + 2 > iend:                             # :149
            return CORRUPTED
        offset = src[ip] | (src[ip + 1] << 8)         # :150
        ip += 2
        if offset == 0:                               # :154
            return CORRUPTED
        ml = token & 15                               # :157
        if ml == 15:
            ml, ip = _length(src, ip, iend, ml)
            if ml is None:
                return CORRUPTED
        ml += 4                                       # :171
        if op + ml > cap:                             # :174
            return OUTPUT_TOO_SMALL
        if offset > op:                               # :181 the match starts in front of dst
            if dict_len is None:                      # :183
                return CORRUPTED
            if offset > op + dict_len:                # :189-192
                return CORRUPTED
            if reach is not None:
                reach.append(offset - op)
        op += ml                                      # :199-248 produce exactly ml bytes
    return op                                         # :250


# ---- XXH32 (the spec's reference algorithm; std.hash.XxHash32 in the reference) ----
_P1, _P2, _P3, _P4, _P5 = 2654435761, 2246822519, 3266489917, 668265263, 374761393
_M = 0xFFFFFFFF


def _rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & _M


def xxh32(data, seed=0):
    data = bytes(data)
    n, i = len(data), 0
    if n >= 16:
        v = [(seed + _P1 + _P2) & _M, (seed + _P2) & _M, seed & _M, (seed - _P1) & _M]
        while i + 16 <= n:
            for k in range(4):
                w = int.from_bytes(data[i + 4 * k:i + 4 * k + 4], "little")
                v[k] = (_rotl((v[k] + w * _P2) & _M, 13) * _P1) & _M
            i += 16
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & _M
    else:
        h = (seed + _P5) & _M
    h = (h + n) & _M
    while i + 4 <= n:
        h = (_rotl((h + int.from_bytes(data[i:i + 4], "little") * _P3) & _M, 17) * _P4) & _M
        i += 4
    while i < n:
        h = (_rotl((h + data[i] * _P5) & _M, 11) * _P1) & _M
        i += 1
    h ^= h >> 15
    h = (h * _P2) & _M
    h ^= h >> 13
    h = (h * _P3) & _M
    h ^= h >> 16
    return h


def _parse_header(src):
    """parseFrameHeader (src/lz4f.zig:483-538) -> (flg, header size) or a negative code."""
    if len(src) < 7:                                  # :484 HEADER_SIZE_MIN
        return F_FRAME_HEADER_INCOMPLETE
    if int.from_bytes(src[0:4], "little") != MAGIC:   # :489-492
        return F_FRAME_TYPE_UNKNOWN
    flg = src[4]
    if (flg >> 6) & 3 != 1:                           # decodeFLG :191-194
        return F_HEADER_VERSION_WRONG
    if flg & 0x02:                                    # :197-199
        return F_RESERVED_FLAG_SET
    bd = src[5]
    if bd & 0x8F:                                     # decodeBD :237-239
        return F_RESERVED_FLAG_SET
    if (bd >> 4) & 7 not in (0, 4, 5, 6, 7):          # :241-248
        return F_MAX_BLOCK_SIZE_INVALID
    pos = 6
    if flg & 0x08:                                    # :509-515
        if len(src) < pos + 8:
            return F_FRAME_HEADER_INCOMPLETE
        pos += 8
    if flg & 0x01:                                    # :518-524
        if len(src) < pos + 4:
            return F_FRAME_HEADER_INCOMPLETE
        pos += 4
    if len(src) < pos + 1:                            # :527-529
        return F_FRAME_HEADER_INCOMPLETE
    if src[pos] != (xxh32(src[4:pos]) >> 8) & 0xFF:   # :530-534, headerChecksum :138-141
        return F_HEADER_CHECKSUM_INVALID
    return flg, pos + 1


def frame_size(src, room=None):
    """What decompressFrame(src, dst) returns for a dst that is never too small; the content checksum is not verified.
    `room` (a list) receives dstPos at the exit: a dst of that many bytes is large enough for this frame, error or not
    (the position only moves past blocks that decoded)."""
    result, total = _frame_walk(bytes(src))
    if room is not None:
        room.append(total)
    return result


def _frame_walk(src):
    """-> (result, dstPos at the exit)"""
    ph = _parse_header(src)                           # :547
    if not isinstance(ph, tuple):
        return ph, 0
    flg, pos = ph
    n, total = len(src), 0
    while pos < n:                                    # :563
        if pos + 4 > n:                               # :565
            return F_FRAME_SIZE_WRONG, total
        h = int.from_bytes(src[pos:pos + 4], "little")
        pos += 4
        if h == 0:                                    # :573
            break
        size = h & 0x7FFFFFFF                         # :578-579
        if pos + size > n:                            # :582
            return F_FRAME_SIZE_WRONG, total
        data = src[pos:pos + size]
        pos += size
        if flg & 0x10:                                # :590
            if pos + 4 > n:                           # :591
                return F_FRAME_SIZE_WRONG, total
            if int.from_bytes(src[pos:pos + 4], "little") != xxh32(data):   # :594-598
                return F_BLOCK_CHECKSUM_INVALID, total
            pos += 4
        if h & 0x80000000:                            # :603-608 stored
            total += size
        else:                                         # :610-613
            s = block_size(data)
            if s < 0:
                return F_DECOMPRESSION_FAILED, total
            total += s
    if flg & 0x04:                                    # :625
        if pos + 4 > n:                               # :626
            return F_FRAME_SIZE_WRONG, total
        # :629-633 ContentChecksumInvalid needs the decoded bytes: not verified by a size query
    return total, total                               # :637
