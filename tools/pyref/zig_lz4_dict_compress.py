"""Python restatement of zlz4_compress_fast_using_dict (include/zlz4_amd.h): the dictionary
compressor.  It has no counterpart in the reference; its definition is anchored to it at both ends:

  tail = the last D = min(len(dict), 65536) bytes of the dictionary, V = tail ++ src, n = len(src)
  entry checks of Stream.compressFastContinue (src/lz4.zig:823-827), which do not depend on the dictionary;
  then compressFastWithHashTable's loop (:624-740) statement for statement on V, with
    1. the table starting as Stream.loadDict(dict) leaves it (:798-820),
    2. anchor = D and ip = max(D, 1) at entry (in place of anchor = 0; ip = 1, :626-633),
    3. mflimitPlusOne = D + n - 12, matchLimit = D + n - 5, every position a position in V,
    4. nothing else changed.

Test infrastructure like zig_lz4_stream.py: written from the specification with line cites, never imported by the
product, the bench or smoke().  Results: bytes written, or the negative lz4.Error code of the C ABI.
"""
from zig_lz4_pyref import DIST_MAX, LASTLITERALS, MFLIMIT, MINMATCH, ML_BITS, ML_MASK, RUN_MASK, _last_literals, _put_len, rd32
from zig_lz4_stream import INPUT_TOO_LARGE, MAX_INPUT, OUTPUT_TOO_SMALL, _hash4, load_dict


def compress_with_table(table, src, dict_bytes, acceleration=1, stats=None):
    """The loop on V from `table` (any 4096 ints; only load_dict(dict)'s gives the specified bytes) -> output bytes, dst
    unbounded.  len(src) >= 13.  stats (a list of two ints) += [match bytes taken from the dictionary, all match bytes]."""
    d = bytes(dict_bytes)
    D = min(len(d), 64 * 1024)                        # :804
    V = d[len(d) - D:] + bytes(src)
    t = list(table)
    out = bytearray()
    L = len(V) - MFLIMIT                              # :630 on V
    match_limit = len(V) - LASTLITERALS               # :631 on V
    anchor = D                                        # :628 (the record starts at D)
    ip = max(D, 1)                                    # :633
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
                _last_literals(out, V, anchor)
                return bytes(out)
            seq = rd32(V, ip)
            h = _hash4(seq)                           # :653
            match = t[h]
            valid = match > 0 and match < ip and match + DIST_MAX >= ip and rd32(V, match) == seq   # :656-659
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
        out += V[anchor:ip]                           # :689-692 (anchor >= D: record bytes)
        out += (ip - match).to_bytes(2, "little")     # :695-699
        m0 = match
        ip += MINMATCH
        match += MINMATCH
        ml = 0
        while ip < match_limit and V[ip] == V[match]:   # :704-712 (may run from the dictionary into the record)
            ip += 1
            match += 1
            ml += 1
        if stats is not None:
            stats[1] += ml + MINMATCH
            if m0 < D:
                stats[0] += min(ml + MINMATCH, D - m0)
        if ml >= ML_MASK:                             # :714-728
            out[token_pos] |= ML_MASK
            _put_len(out, ml - ML_MASK)
        else:
            out[token_pos] |= ml
        anchor = ip                                   # :730
        if ip < L:                                    # :732-736
            t[_hash4(rd32(V, ip))] = ip
            ip += 1
    _last_literals(out, V, anchor)                    # :739
    return bytes(out)


def compress_fast_using_dict(src, dict_bytes, acceleration=1, dst_cap=None, table=None, stats=None):
    """-> (result, output bytes).  dst_cap None = unbounded; table None = Stream.loadDict(dict)'s."""
    src = bytes(src)
    n = len(src)
    if n > MAX_INPUT:                                 # :823
        return INPUT_TOO_LARGE, b""
    if n == 0:                                        # :824
        return 0, b""
    if n < MFLIMIT + 1:                               # :825-827 compressAsLiterals (:449-482)
        out = bytearray()
        _last_literals(out, src, 0)
        out = bytes(out)
    else:
        if table is None:
            table, _ = load_dict(dict_bytes)          # :798-820
        out = compress_with_table(table, src, dict_bytes, acceleration, stats)
    # every OutputTooSmall test compares the running output position with dst.len and the output only grows, so the call
    # fails iff the whole output is longer than dst (as in zig_lz4_stream.compress_fast_continue)
    if dst_cap is not None and len(out) > dst_cap:
        return OUTPUT_TOO_SMALL, b""
    return len(out), out
