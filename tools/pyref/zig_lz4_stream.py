"""Python restatement of the reference's streaming compressor (src/lz4.zig:751-866): Stream.loadDict (:798-820) and
Stream.compressFastContinue (:822-836) with compressFastWithHashTable (:624-748).

Test infrastructure like zig_lz4_pyref.py: written from the Zig source (line cites per step), never imported by the
product, the bench or smoke().  A table is a list of 4096 ints (Stream.hashTable, LZ4_HASH_SIZE_U32 = 4096, :33); the
functions return a NEW table and leave the argument alone.  Results: bytes written, or the negative lz4.Error code of
the C ABI (-1 OutputTooSmall, -2 InputTooLarge).

compressFastWithHashTable is compressFast's loop statement for statement, except that the table starts from the given
state.  Every entry is read as a position in the CURRENT block (:656-659), so a loaded dictionary only changes which
in-block matches the greedy parse finds: no output block refers to the dictionary.
"""
from zig_lz4_pyref import (DIST_MAX, HASH_MUL, LASTLITERALS, M32, MFLIMIT, MINMATCH, ML_BITS, ML_MASK, RUN_MASK,
                           _last_literals, _put_len, rd32)

TABLE_ENTRIES = 4096                                  # LZ4_HASH_SIZE_U32, src/lz4.zig:33
MAX_INPUT = 0x7E000000                                # src/lz4.zig:23
OUTPUT_TOO_SMALL, INPUT_TOO_LARGE = -1, -2            # lz4.Error order, src/lz4.zig:48-55


def _hash4(seq):                                      # :75-77
    return ((seq * HASH_MUL) & M32) >> 20


def load_dict(dict_bytes):
    """Stream.loadDict on a fresh stream -> (table, dictSize)."""
    table = [0] * TABLE_ENTRIES                       # resetFast, :799 (:786-795)
    d = bytes(dict_bytes)
    if len(d) == 0:                                   # :801
        return table, 0
    size = min(len(d), 64 * 1024)                     # :804
    start = len(d) - size                             # :805
    if size >= MINMATCH:                              # :810
        for i in range(size - MINMATCH):              # :812 (i < dictSize - MINMATCH)
            table[_hash4(rd32(d, start + i))] = i     # :813-814 (last writer wins)
    return table, size


def compress_with_table(table, src, acceleration=1):
    """compressFastWithHashTable (:624-748) on a copy of `table` -> (output bytes, final table); dst unbounded."""
    t = list(table)
    src = bytes(src)
    n = len(src)
    out = bytearray()
    ip, anchor = 0, 0
    L = n - MFLIMIT                                   # :630
    match_limit = n - LASTLITERALS                    # :631
    ip += 1                                           # :633
    while ip < L:                                     # :635
        accel = min(max(acceleration, 1), 65537)      # :636
        step = accel
        search_nb = accel
        forward = ip
        while True:                                   # :643
            ip = forward
            forward += step
            step = search_nb >> 6
            search_nb += 1
            if forward > L:                           # :649-650
                _last_literals(out, src, anchor)
                return bytes(out), t
            seq = rd32(src, ip)
            h = _hash4(seq)                           # :653
            match = t[h]
            valid = match > 0 and match < ip and match + DIST_MAX >= ip and rd32(src, match) == seq   # :656-659
            t[h] = ip                                 # :661
            if valid:
                break
        lit = ip - anchor                             # :668
        token_pos = len(out)
        out.append(0)
        if lit >= RUN_MASK:                           # :673-687
            out[token_pos] = RUN_MASK << ML_BITS
            _put_len(out, lit - RUN_MASK)
        else:
            out[token_pos] = lit << ML_BITS
        out += src[anchor:ip]                         # :689-692
        out += (ip - match).to_bytes(2, "little")     # :695-699
        ip += MINMATCH
        match += MINMATCH
        ml = 0
        while ip < match_limit and src[ip] == src[match]:   # :701-712
            ip += 1
            match += 1
            ml += 1
        if ml >= ML_MASK:                             # :714-727
            out[token_pos] |= ML_MASK
            _put_len(out, ml - ML_MASK)
        else:
            out[token_pos] |= ml
        anchor = ip                                   # :730
        if ip < L:                                    # :732-736
            t[_hash4(rd32(src, ip))] = ip
            ip += 1
    _last_literals(out, src, anchor)                  # :739
    return bytes(out), t


def compress_fast_continue(table, src, acceleration=1, dst_cap=None):
    """Stream.compressFastContinue (:822-836) -> (result, output bytes, table after the call).  dst_cap None =
    unbounded.  The table is replaced only when a >= 13-byte block compresses; every other exit leaves it as it was."""
    src = bytes(src)
    n = len(src)
    if n > MAX_INPUT:                                 # :823
        return INPUT_TOO_LARGE, b"", list(table)
    if n == 0:                                        # :824
        return 0, b"", list(table)
    if n < MFLIMIT + 1:                               # :825-827 compressAsLiterals (:449-482)
        out = bytearray()
        _last_literals(out, src, 0)
        if dst_cap is not None and len(out) > dst_cap:
            return OUTPUT_TOO_SMALL, b"", list(table)
        return len(out), bytes(out), list(table)
    out, t = compress_with_table(table, src, acceleration)   # :830-831
    # every OutputTooSmall test of :673-737 compares the running output position with dst.len, and the output only
    # grows, so the call fails iff the whole output is longer than dst; `try` then returns before the store (:832)
    if dst_cap is not None and len(out) > dst_cap:
        return OUTPUT_TOO_SMALL, b"", list(table)
    return len(out), out, t


def save_dict(dictionary, safe_len, max_dict_size):
    """Stream.saveDict (:839-855) on the stream's `dictionary` slice (None = none loaded) -> the bytes it copies to the
    front of a safeBuffer of safe_len bytes.  It copies the tail of the LOADED dictionary, never compressed history."""
    if max_dict_size == 0:                            # :840
        return b""
    if dictionary is None:                            # :841
        return b""
    d = bytes(dictionary)
    size = min(min(len(d), max_dict_size), 64 * 1024)   # :844
    if size > safe_len:                               # :846-850
        copy = min(size, safe_len)
        return d[len(d) - copy:]
    return d[len(d) - size:]                          # :852-853
