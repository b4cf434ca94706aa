"""A model of k_hc_mid_serial's loop (zig-lz4_amd/csrc/zlz4_compress_hc_serial.hip), with switches.

`compress(b)` walks a block the way the kernel does -- the entries of the next probed position read before the
current probe writes its own and patched afterwards, both candidates decided from one 8-byte load each, the length
clamped to matchlimit - ip, the end-of-match fills as index comparisons -- and gives the level-2 stream.  It is written
from the kernel and from DESIGN.md 4.3b, not from the reference, and is slow on purpose: plain integers, one byte at a
time.

`compress(b, defect=NAME)` is the same walk with ONE operator of the kernel changed.  tests/test_mid_corpus_cpu.py
requires every defect of DEFECTS to give other bytes on a case of the family it belongs to (tests/midgen.py), and every
defect of EQUIVALENT to give the same bytes everywhere: those change a comparison that no input can put on its edge.
"""
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
HASH_MUL, HASH_MUL_64 = 2654435761, 58295818150454627       # zlz4_device.hpp kHashMul, zlz4_compress_hc_serial.hip:30
MID_HASH_LOG = 14
MFLIMIT, LAST_LITERALS, MIN_MATCH, MAX_DIST = 12, 5, 4, 65535

# defect -> the family of tests/midgen.py that has to notice it
DEFECTS = {
    "no_patch8": "pf_patch",            # pf8 = n8, also when the next position shares the slot of h8
    "no_patch4": "pf_patch",            # pf4 = n4
    "pf_survives_match": "pf_patch",    # have_pf is not dropped after a taken match
    "pf_survives_match8": "pf_patch",   # ... after a match taken through h8 only
    "pf_survives_match4": "pf_patch",   # ... through h4 only
    "no_clamp": "end_clamp",            # the length is not clamped to matchlimit - ip
    "probe_lt_mflimit": "end_clamp",    # while (ip < mflimit)
    "ml2_ge": "next_longer",            # ml2 >= match_len moves
    "lookup_at_mflimit": "next_longer",  # the ip + 1 lookup also at ip == mflimit
    "no_lookup_before_mflimit": "next_longer",   # the ip + 1 lookup only while ip + 1 < mflimit
    "h8n_read_early": "next_longer",    # the lookup's entry is read before this probe has stored h8[hh8] = ip
    "no_h8n_write": "moved_index",      # a moved match does not store h8[h8n] = ip_index + 1
    "moved_index_exact": "moved_index",  # the begin-of-match fills store the moved index
    "no_b1_h8": "fill_end", "no_b2_h8": "fill_end", "no_b1_h4": "fill_end",      # a begin-of-match entry is missing
    "no_e5": "fill_end", "no_e3": "fill_end", "no_e2_h8": "fill_end", "no_e2_h4": "fill_end", "no_e1": "fill_end",
    "e1_h8_too": "fill_end",            # e - 1 also goes into h8
    "dist_le_65536": "reach",           # every distance test one too wide
    "dist8_le_65536": "reach", "dist4_le_65536": "reach", "dist2_le_65536": "reach",   # one of the three
    "dist_lt_65535": "reach",           # every distance test one too narrow
    "pos_ge_0": "reach",                # position 0 is a source
    "step_from_ip": "step",             # the step counts from the block's start, not from the anchor
    "step_shift_8": "step",             # >> 8
    "step_off_by_one": "step",          # (ip - anchor + 1) >> 9
}
# Equivalent by construction: a taken match has a source pos >= 1 and pos < ip, so ip >= 2 and its end e >= 6, and e - 5 = 1
# has been probed anyway; and with e - 2 == ilimit the match ends at n - 6 > mflimit, so no probe follows that could read
# what the fill wrote.  The `<= ilimit` tests inside the guard follow from the guard itself (e - 2 < ilimit).
EQUIVALENT = ("e_gt_4", "fill_guard_le", "no_inner_guards", "no_begin_guards")


def _rd(b, i, k):
    return int.from_bytes(b[i:i + k], "little")


def hash_mid4(b, i):
    return ((_rd(b, i, 4) * HASH_MUL) & M32) >> (32 - MID_HASH_LOG)


def hash_mid8(b, i):
    """the low 7 bytes of an 8-byte read decide it"""
    return ((((_rd(b, i, 8) << 8) & M64) * HASH_MUL_64) & M64) >> (64 - MID_HASH_LOG)


def _count(b, a, c, limit):
    k = 0
    while a < limit and b[a] == b[c]:
        a += 1; c += 1; k += 1
    return k


def _put_len(out, v):
    while v >= 255:
        out.append(255); v -= 255
    out.append(v)


def _sequence(out, b, anchor, ip, mlen, off):
    lit, mc = ip - anchor, mlen - MIN_MATCH
    out.append((min(lit, 15) << 4) | min(mc, 15))
    if lit >= 15:
        _put_len(out, lit - 15)
    out += b[anchor:ip]
    out += bytes((off & 255, (off >> 8) & 255))         # (the kernel stores two bytes of it)
    if mc >= 15:
        _put_len(out, mc - 15)


def compress(b, defect=None, trace=None):
    """-> the stream; `trace`, a list, receives (event, position) for "probe", "pf" (a probe served by prefetch),
    "move" and "clamp" """
    assert defect is None or defect in DEFECTS or defect in EQUIVALENT, defect
    d = defect
    n = len(b)
    if n == 0:
        return b""
    if n < MFLIMIT + 1:
        return bytes([n << 4]) + bytes(b)
    out = bytearray()
    h4, h8 = {}, {}                                  # zeroed tables
    mflimit, matchlimit, ilimit = n - MFLIMIT, n - LAST_LITERALS, n - 8
    far8 = MAX_DIST + (d in ("dist_le_65536", "dist8_le_65536")) - (d == "dist_lt_65535")
    far4 = MAX_DIST + (d in ("dist_le_65536", "dist4_le_65536")) - (d == "dist_lt_65535")
    far2 = MAX_DIST + (d in ("dist_le_65536", "dist2_le_65536")) - (d == "dist_lt_65535")
    low = -1 if d == "pos_ge_0" else 0

    def eight(i):                                    # ld64 (the arena continues behind the block; the kernel never
        return _rd(b, i, 8) if i + 8 <= n else None  # loads past ip + 8 <= matchlimit + 1, so None is never compared)

    def first8(ip, pos):
        x = eight(ip) ^ eight(pos)
        if x:
            return ((x & -x).bit_length() - 1) >> 3
        return 8 + _count(b, ip + 8, pos + 8, matchlimit)

    def fill_begin(ip, idx):
        g = d != "no_begin_guards"
        if (not g or ip + 1 <= ilimit) and d != "no_b1_h8":
            h8[hash_mid8(b, ip + 1)] = idx + 1
        if (not g or ip + 2 <= ilimit) and d != "no_b2_h8":
            h8[hash_mid8(b, ip + 2)] = idx + 2
        if (not g or ip + 1 <= ilimit) and d != "no_b1_h4":
            h4[hash_mid4(b, ip + 1)] = idx + 1

    def fill_end(e):
        g = d != "no_inner_guards"
        if e - 2 < ilimit or (d == "fill_guard_le" and e - 2 == ilimit):
            if e > (4 if d == "e_gt_4" else 5) and (not g or e - 5 <= ilimit) and d != "no_e5":
                h8[hash_mid8(b, e - 5)] = e - 5
            if (not g or e - 3 <= ilimit) and d != "no_e3":
                h8[hash_mid8(b, e - 3)] = e - 3
            if not g or e - 2 <= ilimit:
                if d != "no_e2_h8":
                    h8[hash_mid8(b, e - 2)] = e - 2
                if d != "no_e2_h4":
                    h4[hash_mid4(b, e - 2)] = e - 2
            if (not g or e - 1 <= ilimit) and d != "no_e1":
                h4[hash_mid4(b, e - 1)] = e - 1
                if d == "e1_h8_too":
                    h8[hash_mid8(b, e - 1)] = e - 1

    ip = anchor = 0
    have_pf, pf8, pf4, pfh8, pfh4 = False, 0, 0, 0, 0
    while (ip < mflimit) if d == "probe_lt_mflimit" else (ip <= mflimit):
        idx = ip
        if trace is not None:
            trace.append(("pf" if have_pf else "probe", ip))
        hh8 = pfh8 if have_pf else hash_mid8(b, ip)
        hh4 = pfh4 if have_pf else hash_mid4(b, ip)
        pos8 = pf8 if have_pf else h8.get(hh8, 0)
        pos4 = pf4 if have_pf else h4.get(hh4, 0)
        since = ip if d == "step_from_ip" else ip - anchor + (d == "step_off_by_one")
        nip = ip + 1 + (since >> (8 if d == "step_shift_8" else 9))
        nvalid = nip <= mflimit
        nh8 = nh4 = n8 = n4 = 0
        if nvalid:
            nh8, nh4 = hash_mid8(b, nip), hash_mid4(b, nip)
            n8, n4 = h8.get(nh8, 0), h4.get(nh4, 0)
        ok8 = pos8 > low and idx - pos8 <= far8 and pos8 < ip
        ok4 = pos4 > low and idx - pos4 <= far4 and pos4 < ip
        taken = False
        h8[hh8] = idx
        if ok8:
            mlt = first8(ip, pos8)
            if mlt > matchlimit - ip and d != "no_clamp":
                mlt = matchlimit - ip
                if trace is not None:
                    trace.append(("clamp", ip))
            if mlt >= MIN_MATCH:
                fill_begin(ip, idx)
                _sequence(out, b, anchor, ip, mlt, idx - pos8)
                ip += mlt; anchor = ip
                fill_end(ip)
                taken = True
                keep = d in ("pf_survives_match", "pf_survives_match8")
        if not taken:
            h4[hh4] = idx
            if ok4:
                mlen = first8(ip, pos4)
                if mlen > matchlimit - ip and d != "no_clamp":
                    mlen = matchlimit - ip
                    if trace is not None:
                        trace.append(("clamp", ip))
                if mlen >= MIN_MATCH:
                    dist = idx - pos4
                    look = ip <= mflimit if d == "lookup_at_mflimit" else \
                        ip + 1 < mflimit if d == "no_lookup_before_mflimit" else ip < mflimit
                    if look:
                        h8n = hash_mid8(b, ip + 1)
                        pos8n = pos8 if (d == "h8n_read_early" and h8n == hh8) else h8.get(h8n, 0)
                        m2 = idx + 1 - pos8n
                        if m2 <= far2 and pos8n > low and pos8n < ip + 1:
                            ml2 = _count(b, ip + 1, pos8n, matchlimit)
                            if ml2 > mlen or (d == "ml2_ge" and ml2 == mlen):
                                if d != "no_h8n_write":
                                    h8[h8n] = idx + 1
                                ip += 1
                                mlen, dist = ml2, m2
                                if trace is not None:
                                    trace.append(("move", ip))
                    fill_begin(ip, ip if d == "moved_index_exact" else idx)
                    _sequence(out, b, anchor, ip, mlen, dist)
                    ip += mlen; anchor = ip
                    fill_end(ip)
                    taken = True
                    keep = d in ("pf_survives_match", "pf_survives_match4")
        if taken:
            if not keep:
                have_pf = False
            continue
        pf8 = idx if (nh8 == hh8 and d != "no_patch8") else n8
        pf4 = idx if (nh4 == hh4 and d != "no_patch4") else n4
        pfh8, pfh4 = nh8, nh4
        have_pf = nvalid
        ip = nip
    fl = n - anchor
    if fl:
        out.append(min(fl, 15) << 4)
        if fl >= 15:
            _put_len(out, fl - 15)
        out += b[anchor:]
    return bytes(out)
