"""Python restatement of zlz4_compress_hc_using_dict (include/zlz4_amd.h): compressHashChain
(src/lz4hc.zig:976-1064) on V = tail ++ src with a fresh context and ip = anchor = D, built from the helpers of
zig_lz4_pyref.py (insertHC, insertAndGetWiderMatch, encodeSequence are used as they are: they address bytes as
src[position], and the position of a byte is its position in V).

Results are ints for errors (lz4.Error order) and bytes for streams."""
from zig_lz4_pyref import (LASTLITERALS, MFLIMIT, MINMATCH, _Ctx, _encode_literals, _encode_sequence, _insert_hc,
                           _wider_match)

MAX_INPUT = 0x7E000000
ERR_OUTPUT_TOO_SMALL, ERR_INPUT_TOO_LARGE, ERR_INVALID_STATE, ERR_UNSUPPORTED = -1, -2, -5, -8


def compress_bound(n):
    return 0 if n > MAX_INPUT else n + n // 255 + 16


def level_of(level):
    """the level compressHC runs (:1446-1452), or 0 where the dictionary call has none (2: lz4mid, 10..12: lz4opt)"""
    if level < 2:
        level = 9
    if level > 12:
        level = 12
    return level if 3 <= level <= 9 else 0


def _ext(v):
    return 1 + (v - 15) // 255 if v >= 15 else 0


def compress_hc_using_dict(src, dict_bytes, level, dst_cap=None, sequences=None):
    """-> bytes or an error code.  dict_bytes None = the null dictionary (dict == NULL, dict_len == 0).  sequences: a list
    that receives (position in V, literal length, match length, offset, D) per sequence."""
    src = bytes(src)
    n = len(src)
    level = level_of(level)
    if level == 0:
        return ERR_UNSUPPORTED
    if n > MAX_INPUT:
        return ERR_INPUT_TOO_LARGE                    # :1442
    if n == 0:
        return b""                                    # :1443
    cap = compress_bound(n) if dst_cap is None else dst_cap
    if cap == 0:
        return ERR_OUTPUT_TOO_SMALL                   # :1461
    if n < MFLIMIT + 1:                               # :995-998
        return ERR_OUTPUT_TOO_SMALL if cap < n + 1 + n // 255 else _encode_literals(src)   # :1395
    d = bytes(dict_bytes or b"")
    tail = d[-65536:] if len(d) > 65536 else d
    D = len(tail)
    v = tail + src
    N = D + n
    max_attempts = 1 << (level - 1)
    ctx = _Ctx()                                      # Context.init; nextToUpdate = 0
    out = bytearray()
    ip = anchor = D
    mflimit, matchlimit = N - MFLIMIT, N - LASTLITERALS
    while ip <= mflimit:                              # :1009
        _insert_hc(ctx, v, ip)
        mlen, off = _wider_match(ctx, v, ip, matchlimit, MINMATCH - 1, max_attempts, max_attempts > 128)
        if mlen < MINMATCH or off == 0:
            ip += 1
            continue
        lit = ip - anchor
        op = len(out)
        if op + lit // 255 + lit + (2 + 1 + LASTLITERALS) > cap:                     # :320-325
            return ERR_OUTPUT_TOO_SMALL
        if op + 1 + _ext(lit) + lit + 2 + (mlen - MINMATCH) // 255 + (1 + LASTLITERALS) > cap:   # :355-359
            return ERR_OUTPUT_TOO_SMALL
        if sequences is not None:
            sequences.append((ip, lit, mlen, off, D))
        ip = anchor = _encode_sequence(out, v, ip, anchor, mlen, off)
    fl = N - anchor                                   # :1035
    if fl > 0:
        op = len(out)
        # :1037, and the refusal where the reference would write its length bytes past the end (k_hc_parse_emit)
        if op + fl + 1 > cap or op + 1 + _ext(fl) + fl > cap:
            return ERR_OUTPUT_TOO_SMALL
        out += _encode_literals(v[anchor:])
    return bytes(out)


def batch(records, dicts, level, caps=None, max_in_len=None, max_dict_len=None):
    """zlz4_batch_compress_hc_using_dict over Python lists -> an error code for the call, or a list of results."""
    if not records:
        return []
    if level_of(level) == 0:
        return ERR_UNSUPPORTED
    max_in = max(len(r) for r in records) if max_in_len is None else max_in_len
    max_d = 65536 if max_dict_len is None else max_dict_len
    res = []
    for i, r in enumerate(records):
        d = dicts[i] or b""
        if len(r) > MAX_INPUT:
            res.append(ERR_INPUT_TOO_LARGE)
        elif len(r) > max_in or min(len(d), 65536) > max_d:
            res.append(ERR_INVALID_STATE)
        else:
            res.append(compress_hc_using_dict(r, d, level, None if caps is None else caps[i]))
    return res
