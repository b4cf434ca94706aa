#!/usr/bin/env python3
"""Lane-level Python emulation of k_compress_fast's window path + generic path (debug aid).
Mirrors the window logic of zig-lz4_amd/csrc/zlz4_compress_fast.hip as it was when the window path was brought up
(12-byte in-register compare, hand-over at lane 49, one flush per sequence): the later refinements of the kernel
(48-byte compare levels, extension bytes in the run flush, precomputed fast-run steps, hand-over at lane 64) change
how many sequences a window resolves and how they are emitted, not the bytes, so the emulator still produces the
oracle's output and remains the place to try a change of the lane logic on the CPU first.

The window's epilogue is written the way the kernel has it: the lanes strictly inside a match are one mask (cov_acc)
that every flush and every immediate emission ORs its own lanes into (run_cover / imm_cover), `ins` comes from that
mask without another pass over the match lanes, and the table is settled by one write per lane (commit_one_write).
tests/test_window_commit_model_cpu.py checks both against the definitions they replaced.

A window only starts behind a match (has_ins: lane 0 is the anchor's pending put), so every lane of a window reads,
puts and reads back its slot; the block's first search, where position 0 is neither probed nor put, runs on the generic
path (tests/test_window_entry_model_cpu.py).  ins_mask and commit_one_write keep their general forms (a mask / list of
the written lanes) for the checks of their definitions; the window passes all 64 lanes.

compress_run_masks() further down is the window in its present form (48-byte compare levels, runs with extension bytes,
precomputed fast-run steps, hand-over at lane 64) with the pending run's masks in scalar form, every new form next to the
one it replaced (tests/test_window_run_masks_model_cpu.py)."""
import sys, os
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1
ALL_LANES = [True] * 64
def rd32(b, p): return int.from_bytes(b[p:p+4], "little")
def hash4(x): return ((x * 2654435761) & M32) >> 20
def ext_len_bytes(v): return 1 + (v - 15) // 255 if v >= 15 else 0
def ext_bytes(v):
    r = v - 15; return bytes([255] * (r // 255) + [r % 255])
def ctz(x): return (x & -x).bit_length() - 1
def msb(x): return x.bit_length() - 1
def S(x):
    q, r = x >> 6, x & 63; return 32 * q * (q - 1) + q * r

def extend(src, m_pos, m_cand, mlen, match_limit):
    ip, mt = m_pos + 4 + mlen, m_cand + 4 + mlen
    while ip < match_limit and src[ip] == src[mt]:
        ip += 1; mt += 1; mlen += 1
    return mlen

def run_cover(mm_run, v_end):
    """ballot(cov) of a flush: the lanes strictly inside a match of the run mm_run (lane i: the nearest match lane of the
    run below it ends above it).  v_end[j] = anchor lane after a match at lane j (may be >= 64)."""
    m, rest = 0, mm_run
    while rest:
        j = ctz(rest); rest &= rest - 1
        top = min(v_end[j], ctz(rest) + 1 if rest else 64, 64)      # lanes j+1 .. top-1 (the next match lane looks at j too)
        if top > j + 1: m |= ((1 << top) - 1) & ~((2 << j) - 1)
    return m

def imm_cover(j, e):
    """lanes j+1 .. e-1 of a match at lane j that was emitted immediately (e = its anchor lane, may be >= 64)"""
    return ((1 << min(e, 64)) - 1) & ~((2 << j) - 1)

def ins_mask(wrmask, cov_acc, f_end):
    """lanes the serial loop put(): written at all, below the frontier, not strictly inside a match"""
    return wrmask & ~cov_acc & ((1 << min(f_end, 64)) - 1)

def commit_one_write(table, h, mine, old, wr, grp, ins):
    """Leave `table` as the serial loop would have, one write per lane: with gi = grp & ins, a written lane of a group
    without an `ins` lane puts its old value back, the highest `ins` lane of a group stores its own entry, every other
    lane writes nothing.  Returns [(lane, slot, value)], the writes in lane order (all lanes of a group read the same
    old value before any put, so writes to one slot carry one value)."""
    writes = []
    for i in range(64):
        gi = grp[i] & ins
        if wr[i] and gi == 0: writes.append((i, h[i], old[i]))
        elif (ins >> i) & 1 and (gi >> i) >> 1 == 0: writes.append((i, h[i], mine[i]))
    for _, slot, v in writes: table[slot] = v
    return writes

def compress(src, accel=1, dst_len=None, RESTART=48, trace=False):
    n = len(src)
    if n == 0: return b""
    if n < 13:
        return bytes([min(n,15) << 4]) + (ext_bytes(n) if n >= 15 else b"") + src
    dst_len = dst_len if dst_len is not None else n + n // 255 + 16
    table = [0] * 4096
    L, match_limit = n - 12, n - 5
    anchor, op, F0, has_ins = 0, 0, 1, False
    out = bytearray(dst_len + 64)
    cbase = max(64, accel); s_cbase = S(cbase)
    def emit_general(lit_src_pos, lit, offset, mlen):
        nonlocal op
        tok = (min(lit, 15) << 4) | min(mlen, 15)
        b = bytes([tok]) + (ext_bytes(lit) if lit >= 15 else b"") + src[lit_src_pos:lit_src_pos+lit] + offset.to_bytes(2, "little") + (ext_bytes(mlen) if mlen >= 15 else b"")
        out[op:op+len(b)] = b; op += len(b)
    while F0 < L:
        ub = -1
        if accel == 1 and F0 == anchor + 1 and has_ins and anchor + 192 < L:
            A = anchor
            pos = [A + i for i in range(64)]
            fwd = [[rd32(src, pos[i] + 4*k) for k in range(4)] for i in range(64)]
            h = [hash4(fwd[i][0]) for i in range(64)]
            old = [table[h[i]] for i in range(64)]
            for i in range(64):
                table[h[i]] = pos[i]                # race winner: any; emulate "last lane wins"
            by_hash = {}
            for i in range(64): by_hash[h[i]] = by_hash.get(h[i], 0) | (1 << i)
            grp = [by_hash[h[i]] for i in range(64)]    # the lanes of the window that share lane i's hash
            old_ok = [old[i] > 0 and old[i] + 65535 >= pos[i] for i in range(64)]
            cold = [[rd32(src, old[i] + 4*k) for k in range(4)] if old_ok[i] else [0]*4 for i in range(64)]
            vo = [old_ok[i] and cold[i][0] == fwd[i][0] for i in range(64)]
            mlo = []
            for i in range(64):
                x1, x2, x3 = fwd[i][1]^cold[i][1], fwd[i][2]^cold[i][2], fwd[i][3]^cold[i][3]
                mlo.append(ctz(x1)>>3 if x1 else (4+(ctz(x2)>>3) if x2 else (8+(ctz(x3)>>3) if x3 else 12)))
            single = [grp[i] == (1 << i) for i in range(64)]
            cfast = sum(1 << i for i in range(64) if vo[i] and mlo[i] < 12)
            slow = sum(1 << i for i in range(64) if (((not single[i]) and not (vo[i] and mlo[i] < 12)) or (vo[i] and mlo[i] >= 12)))
            nsing = sum(1 << i for i in range(64) if not single[i])
            def first_ge(mask, i):
                m = mask >> i
                return i + ctz(m) if m else 64
            J = [first_ge(cfast, i) for i in range(64)]
            Sx = [first_ge(slow, i) for i in range(64)]
            v_end = [i + 4 + mlo[i] for i in range(64)]
            E = [v_end[J[i] & 63] for i in range(64)]
            f, a, nseq, cov_acc = 1, 0, 0, 0
            continue_generic = False
            tight = dst_len - op < 512
            while True:
                # ---- fast run: collect match lanes with a minimal scalar loop ----
                a0, op0, mm_run = a, op, 0
                while f < 64 and (f < 49 or (nseq == 0 and mm_run == 0)):
                    j, sl = J[f], Sx[f]
                    if tight or sl <= j or j - a >= 15 or (nsing >> j) & 1: break
                    mm_run |= 1 << j
                    e = v_end[j]; a = e; f = e + 1
                if mm_run:
                    # ---- vector flush of the run ----
                    jlast = msb(mm_run)
                    litmask = 0
                    info = []
                    for i in range(64):
                        mb = mm_run & ((1 << i) - 1)
                        has_prev = mb != 0
                        pend = v_end[msb(mb)] if has_prev else a0
                        cov = has_prev and i < pend
                        is_m = (mm_run >> i) & 1
                        is_lit = i >= a0 and i < jlast and not cov and not is_m
                        if is_lit: litmask |= 1 << i
                        info.append((pend, is_m, is_lit))
                    for i in range(64):
                        pend, is_m, is_lit = info[i]
                        k = bin(mm_run & ((1 << i) - 1)).count("1")
                        Lb = bin(litmask & ((1 << i) - 1)).count("1")
                        if is_lit: out[op0 + 3 * k + Lb + 1] = fwd[i][0] & 0xFF
                        if is_m:
                            lit_k = i - pend
                            out[op0 + 3 * k + Lb - lit_k] = (lit_k << 4) | mlo[i]
                            o2 = op0 + 3 * k + Lb + 1
                            out[o2:o2 + 2] = ((pos[i] - old[i]) & 0xFFFF).to_bytes(2, "little")
                            if trace: print("  fast seq A=%d j=%d cand=%d lit=%d mlen=%d" % (A, i, old[i], lit_k, mlo[i]))
                    op = op0 + 3 * bin(mm_run).count("1") + bin(litmask).count("1")
                    cov_acc |= run_cover(mm_run, v_end)
                    nseq += bin(mm_run).count("1")
                if f >= 64 or (f >= 49 and nseq > 0):
                    if nseq == 0: continue_generic = True
                    break
                # ---- exact step for the search at probe lane f ----
                j, sl = J[f], Sx[f]
                x = sl if sl < j else j
                if x >= 64:
                    if nseq == 0: continue_generic = True
                    break
                pm = 0
                if (nsing >> x) & 1:
                    pm = grp[x] & ~cov_acc & ((1 << x) - 1)      # (no run is pending here)
                if pm:
                    pr = msb(pm); ok = fwd[pr][0] == fwd[x][0]; m_cand = A + pr; c = fwd[pr]
                else:
                    ok = vo[x]; m_cand = old[x]; c = cold[x]
                if not ok:
                    f = x + 1; continue
                j = x; m_pos = A + j
                xa = ((fwd[j][2] ^ c[2]) << 32) | (fwd[j][1] ^ c[1]); xb = fwd[j][3] ^ c[3]
                if xa: mlen = ctz(xa) >> 3
                elif xb: mlen = 8 + (ctz(xb) >> 3)
                else: mlen = extend(src, m_pos, m_cand, 12, match_limit)
                lit = j - a
                if trace: print("  slow seq A=%d j=%d cand=%d lit=%d mlen=%d" % (A, j, m_cand, lit, mlen))
                emit_general(A + a, lit, m_pos - m_cand, mlen)
                e = j + 4 + mlen
                cov_acc |= imm_cover(j, e)
                nseq += 1
                a = e
                if e >= 64: break
                f = e + 1
            anchor = A + a
            f_end = 64 if continue_generic else (64 if a >= 64 else a + 1)
            ins = ins_mask(M64, cov_acc, f_end)
            commit_one_write(table, h, pos, old, ALL_LANES, grp, ins)
            if not continue_generic:
                if anchor < L: has_ins, F0 = True, anchor + 1
                else: has_ins, F0 = False, L
                continue
            ub = 63
        # generic (serial emulation of one search from probe index ub)
        found = False
        u = ub
        while True:
            if u < 0:
                if has_ins:
                    p = F0 - 1; table[hash4(rd32(src, p))] = p
                u = 0; continue
            if u == 0: pos_, st = F0, accel
            elif u == 1: pos_, st = F0 + accel, accel >> 6
            else:
                x = cbase + u - 1; pos_, st = F0 + accel + S(x) - s_cbase, x >> 6
            if pos_ + st > L: break
            hh = hash4(rd32(src, pos_)); cand = table[hh]
            valid = cand > 0 and cand < pos_ and cand + 65535 >= pos_ and rd32(src, cand) == rd32(src, pos_)
            table[hh] = pos_
            if valid: found = True; break
            u += 1
        if not found: break
        mlen = extend(src, pos_, cand, 0, match_limit)
        if trace: print("  generic seq pos=%d cand=%d lit=%d mlen=%d" % (pos_, cand, pos_ - anchor, mlen))
        emit_general(anchor, pos_ - anchor, pos_ - cand, mlen)
        end = pos_ + 4 + mlen; anchor = end
        if end < L: has_ins, F0 = True, end + 1
        else: has_ins, F0 = False, L
    lit = n - anchor
    if lit:
        b = bytes([min(lit,15) << 4]) + (ext_bytes(lit) if lit >= 15 else b"") + src[anchor:]
        out[op:op+len(b)] = b; op += len(b)
    return bytes(out[:op])


# ---------------------------------------------------------------------------------------------------------------------
# The window as the kernel has it now (48-byte compare levels, runs with extension bytes, precomputed fast-run steps,
# hand-over at lane 64), with the run masks in scalar form: E_run beside mm_run, covered lanes by subtraction, pend from
# the end-lane mask, one exit test per fast-run trip, the exact step's inputs from masks.  Every new form stands next to
# the form it replaced; compress_run_masks(check=True) evaluates both wherever the kernel evaluates one and asserts that
# they agree (tests/test_window_run_masks_model_cpu.py), and records which events a block's windows went through
# (tests/runmaskgen.py builds its corpus from that).
# ---------------------------------------------------------------------------------------------------------------------
def bits(m):
    while m:
        yield ctz(m); m &= m - 1

def first_ge(mask, i):
    m = mask >> i
    return i + ctz(m) if m else 64

def ends_mask(mm_run, v_end):
    """E_run: bit e for every match of the run whose end lane e = v_end[j] is below 64"""
    return sum(1 << v_end[j] for j in bits(mm_run) if v_end[j] < 64)

def cover_sub(E_run, mm_run):
    """the lanes strictly inside the matches of a run: every match is 2^e - 2^(j+1); a last end >= 64 has no bit and wraps"""
    return (E_run - (mm_run << 1)) & M64

def pend_permute(mm_run, v_end, a0, i):
    """first lane of lane i's literal run, the form with the permute: the end of the nearest match lane below i, else a0"""
    mb = mm_run & ((1 << i) - 1)
    return v_end[msb(mb)] if mb else a0

def pend_ends(E_run, a0, i):
    """the same from the end-lane mask: the highest bit of E_run | bit(a0) at or below lane i"""
    return msb((E_run | (1 << a0) | 1) & ((2 << i) - 1))

def litmask_ballot(mm_run, v_end, a0):
    jlast, m = msb(mm_run), 0
    for i in range(64):
        mb = mm_run & ((1 << i) - 1)
        cov = mb != 0 and i < v_end[msb(mb)]
        if i >= a0 and not (i >= jlast or cov or (mm_run >> i) & 1): m |= 1 << i
    return m

def litmask_scalar(mm_run, E_run, a0):
    jlast = msb(mm_run)
    return ((1 << jlast) - 1) & ~((1 << a0) - 1) & ~(cover_sub(E_run, mm_run) | mm_run) & M64

def steps_old(cfast, slow, nsing, vom, mlo, v_end):
    """J / S / XP / Q / PK per lane, as the vector code built them: PK = j | (v_end[j] << 6) or ~0"""
    PK, XP, Q = [], [], []
    for i in range(64):
        J, Sx = first_ge(cfast, i), first_ge(slow, i)
        xm = min(J, Sx)
        XP.append(xm | (((nsing >> (xm & 63)) & 1) << 7))
        Q.append(((vom >> i) & 1) | (mlo[i] << 1))
        ok = J < 64 and Sx > J and not (nsing >> (J & 63)) & 1
        PK.append(J | (v_end[J & 63] << 6) if ok else M32)
    return PK, XP, Q

def steps_new(cfast, slow, nsing, vom, mlo, v_end):
    """PK from fastm / stopm: j | ((v_end[j] + 1) << 6) | bit 31 if the step ends the window, or ~0; X = the first lane
    >= i that can match at all; Q = the lane's own bits: vo | nsing << 1 | mlo << 2 (no lane looks up another lane's bit)"""
    fastm, stopm = cfast & ~nsing & M64, slow | (cfast & nsing)
    PK, X, Q = [], [], []
    for i in range(64):
        J, Sx = first_ge(fastm, i), first_ge(stopm, i)
        PK.append(J | ((v_end[J] + 1) << 6) | (0x80000000 if v_end[J] >= 63 else 0) if J < Sx else M32)
        X.append(min(J, Sx))
        Q.append(((vom >> i) & 1) | (((nsing >> i) & 1) << 1) | (mlo[i] << 2))
    return PK, X, Q

def exact_inputs_old(XP, Q, f):
    """-> (x, nsing bit of x, vo of x, mlo of x); x = 64: nothing can match from f on"""
    x = XP[f] & 127
    return (64, 0, 0, 0) if x >= 64 else (x, XP[f] >> 7, Q[x] & 1, Q[x] >> 1)

def exact_inputs_new(X, Q, f):
    x = X[f]
    return (64, 0, 0, 0) if x >= 64 else (x, (Q[x] >> 1) & 1, Q[x] & 1, Q[x] >> 2)

def fast_run_two_tests(PK, f, a, mm_run):
    """the trip with `f > 63` and `pk == ~0`: -> (f, a, mm_run, [(j, e)] consumed)"""
    seqs = []
    while f < 64:
        pk = PK[f]
        if pk == M32: break
        j = pk & 63; a = pk >> 6; f = a + 1
        mm_run |= 1 << j; seqs.append((j, a))
    return f, a, mm_run, seqs

def fast_run_one_test(PK, f, a, mm_run, E_run):
    """the trip with one test of bit 31; entered with f < 64 only: -> (f, a, mm_run, E_run, [(j, e)] consumed)"""
    seqs = []
    if f < 64:
        while True:
            pk = PK[f]
            if pk & 0x80000000: break
            f = pk >> 6; j = pk & 63; mm_run |= 1 << j; a = f - 1; E_run |= 1 << a
            seqs.append((j, a))
        if pk != M32:                   # the step that ends the window, consumed once
            j = pk & 63; mm_run |= 1 << j; f = (pk >> 6) & 127; a = f - 1
            if a == 63: E_run |= 1 << 63
            seqs.append((j, a))
    return f, a, mm_run, E_run, seqs

# (a sequence without literals cannot occur inside a run: the search behind a match starts at its end lane + 1 (Q6), so
#  the nearest match lane is e + 1, one literal.  compress_run_masks asserts that; the identities hold for e == j all the
#  same, and tests/test_window_run_masks_model_cpu.py checks them there on made-up runs.)
EVENTS = ("end62", "end63", "end64", "end65+", "enter_f64", "first_trip_terminal", "one_lit_in_run", "ownm",
          "dup_exact_pending_covered", "dup_exact_pending_not_covered", "long44_after_pending", "imm270_after_pending",
          "tight", "generic_a0")

def compress_run_masks(src, dst_len=None, events=None, check=True):
    """LZ4 fast compression (acceleration 1) with the window path in its present form.  -> bytes, None if dst_len is too
    small.  events: a set that receives the names (EVENTS) of what the windows went through."""
    n = len(src)
    ev = events if events is not None else set()
    if n == 0: return b""
    bound = n + n // 255 + 16
    dst_len = dst_len if dst_len is not None else bound
    if n < 13:
        b = bytes([min(n, 15) << 4]) + (ext_bytes(n) if n >= 15 else b"") + src
        return b if len(b) <= dst_len else None
    table = [0] * 4096
    L, match_limit = n - 12, n - 5
    anchor, op, F0, has_ins = 0, 0, 1, False
    out = bytearray(bound + 600)
    def emit_general(lit_src_pos, lit, offset, mlen):
        nonlocal op
        tok = (min(lit, 15) << 4) | min(mlen, 15)
        b = bytes([tok]) + (ext_bytes(lit) if lit >= 15 else b"") + src[lit_src_pos:lit_src_pos+lit] + offset.to_bytes(2, "little") + (ext_bytes(mlen) if mlen >= 15 else b"")
        if op + len(b) > dst_len: return False
        out[op:op+len(b)] = b; op += len(b)
        return True
    while F0 < L:
        ub = -1
        if F0 == anchor + 1 and has_ins and anchor + 192 < L:
            A = anchor
            pos = [A + i for i in range(64)]
            w0 = [rd32(src, pos[i]) for i in range(64)]
            h = [hash4(w0[i]) for i in range(64)]
            old = [table[h[i]] for i in range(64)]
            by_hash = {}
            for i in range(64): by_hash[h[i]] = by_hash.get(h[i], 0) | (1 << i)
            grp = [by_hash[h[i]] for i in range(64)]
            vom, mlo = 0, []
            for i in range(64):
                ok = old[i] > 0 and old[i] + 65535 >= pos[i] and rd32(src, old[i]) == w0[i]
                if ok: vom |= 1 << i
                k = 0
                if ok:
                    while k < 44 and src[pos[i] + 4 + k] == src[old[i] + 4 + k]: k += 1
                mlo.append(k)
            nsing = sum(1 << i for i in range(64) if grp[i] & ((1 << i) - 1))
            lt44 = sum(1 << i for i in range(64) if mlo[i] < 44)
            cfast = vom & lt44
            slow = (nsing & ~cfast & M64) | (vom & ~lt44 & M64)
            v_end = [i + 4 + mlo[i] for i in range(64)]
            mlo_e, off_e = list(mlo), [pos[i] - old[i] for i in range(64)]
            PK, X, Q = steps_new(cfast, slow, nsing, vom, mlo, v_end)
            if check: PKo, XPo, Qo = steps_old(cfast, slow, nsing, vom, mlo, v_end)
            ends_of = {}                       # match lane -> end lane, of the pending run (the permute form's v_end)
            f, a, cov_acc = 1, 0, 0
            nseq = 0                           # (check only)
            continue_generic = failed = False
            tight = dst_len - op < 512
            if tight: ev.add("tight")
            a0, op0, mm_run, E_run = a, op, 0, 0
            first_trip = True
            def flush_run():
                nonlocal op, cov_acc, mm_run, E_run
                assert op0 == op                # op does not move while a run is pending: the kernel keeps no op0
                covm = cover_sub(E_run, mm_run)
                jlast = msb(mm_run)
                litmask = litmask_scalar(mm_run, E_run, a0)
                if check:
                    ve = [ends_of.get(i, v_end[i]) for i in range(64)]
                    assert E_run == ends_mask(mm_run, ve)
                    assert covm == run_cover(mm_run, ve), (hex(mm_run), hex(E_run))
                    assert litmask == litmask_ballot(mm_run, ve, a0)
                    for i in range(64):
                        if ((mm_run | litmask) >> i) & 1: assert pend_ends(E_run, a0, i) == pend_permute(mm_run, ve, a0, i)
                last_e = ends_of[jlast]
                ev.add("end62" if last_e == 62 else "end63" if last_e == 63 else "end64" if last_e == 64 else "end65+" if last_e > 64 else "end<62")
                extm = sum(1 << j for j in bits(mm_run) if mlo_e[j] >= 15)
                pend = [pend_ends(E_run, a0, i) for i in range(64)]
                ownm = 0
                for i in range(64):
                    above = mm_run >> i
                    my_m = i + ctz(above) if above else i
                    if my_m - pend[i] >= 15: ownm |= 1 << i
                lextm = mm_run & ownm
                if lextm: ev.add("ownm")
                def rank(m, i): return bin(m & ((1 << i) - 1)).count("1")
                for i in range(64):
                    own_l = (ownm >> i) & 1
                    o1 = op0 + 3 * rank(mm_run, i) + rank(litmask, i) + 1 + rank(extm, i) + rank(lextm, i) + own_l
                    if (litmask >> i) & 1: out[o1] = w0[i] & 0xFF
                    if (mm_run >> i) & 1:
                        lit_k = i - pend[i]
                        assert lit_k >= 1 or i == a0 == 0 or not mm_run & ((1 << i) - 1)
                        if lit_k == 1 and mm_run & ((1 << i) - 1): ev.add("one_lit_in_run")
                        tk = o1 - 1 - lit_k - own_l
                        out[tk] = (min(lit_k, 15) << 4) | min(mlo_e[i], 15)
                        if own_l: out[tk + 1] = lit_k - 15
                        out[o1:o1 + 2] = (off_e[i] & 0xFFFF).to_bytes(2, "little")
                        if mlo_e[i] >= 15: out[o1 + 2] = mlo_e[i] - 15
                op = op0 + 3 * bin(mm_run).count("1") + bin(litmask).count("1") + bin(extm).count("1") + bin(lextm).count("1")
                cov_acc |= covm
                mm_run = E_run = 0
                ends_of.clear()
            while True:
                if mm_run == 0: a0, op0 = a, op
                if f == 64: ev.add("enter_f64")
                if not tight:
                    if check:
                        f2, a2, mm2, seqs2 = fast_run_two_tests(PKo, f, a, mm_run)
                    f, a, mm_run, E_run, seqs = fast_run_one_test(PK, f, a, mm_run, E_run)
                    if check: assert (f2, a2, mm2, seqs2) == (f, a, mm_run, seqs), (seqs2, seqs)
                    if first_trip and len(seqs) == 1 and seqs[0][1] >= 63: ev.add("first_trip_terminal")
                    for j, e in seqs: ends_of[j] = e
                    nseq += len(seqs)
                first_trip = False
                if check: assert (a == 0) == (nseq == 0)
                if f >= 64:
                    if a == 0: continue_generic = True
                    break
                x, ns_x, vo_x, ml_x = exact_inputs_new(X, Q, f)
                if check: assert (x, ns_x, vo_x, ml_x) == exact_inputs_old(XPo, Qo, f)
                if x >= 64:
                    if a == 0: continue_generic = True
                    break
                pm = 0
                if ns_x:
                    covered = cov_acc | cover_sub(E_run, mm_run)
                    if check:
                        ve = [ends_of.get(i, v_end[i]) for i in range(64)]
                        assert covered == cov_acc | (run_cover(mm_run, ve) if mm_run else 0)
                    pm = grp[x] & ~covered & ((1 << x) - 1)
                    if mm_run:
                        near = msb(grp[x] & ((1 << x) - 1))
                        ev.add("dup_exact_pending_covered" if (covered >> near) & 1 else "dup_exact_pending_not_covered")
                j = x; m_pos = A + j
                joined = False
                if pm:
                    pr = msb(pm)
                    if w0[pr] != w0[x]: f = x + 1; continue
                    m_cand = A + pr
                    mlen = extend(src, m_pos, m_cand, 0, match_limit)
                else:
                    if not vo_x: f = x + 1; continue
                    mlen = ml_x
                    if mlen < 44 and not tight:
                        mm_run |= 1 << j; a = j + 4 + mlen; ends_of[j] = a; nseq += 1
                        if a < 64: E_run |= 1 << a
                        if a >= 64: break
                        f = a + 1; continue
                    m_cand = old[x]
                    if mlen >= 44: mlen = extend(src, m_pos, m_cand, 44, match_limit)
                lit, offset, e = j - a, m_pos - m_cand, j + 4 + mlen
                if not tight and mlen < 270:
                    if mm_run and mlen >= 44: ev.add("long44_after_pending")
                    mlo_e[j], off_e[j] = mlen, offset
                    mm_run |= 1 << j; ends_of[j] = e; nseq += 1
                    if e < 64: E_run |= 1 << e
                    a = e
                    if e >= 64: break
                    f = e + 1; continue
                if mm_run:
                    if mlen >= 270: ev.add("imm270_after_pending")
                    flush_run()
                if not emit_general(A + a, lit, offset, mlen): failed = True; break
                cov_acc |= imm_cover(j, e)
                nseq += 1
                a = e
                if e >= 64: break
                f = e + 1
            if check: assert (a == 0) == (nseq == 0)
            if failed: return None
            if mm_run: flush_run()
            anchor = A + a
            f_end = 64 if continue_generic else (64 if a >= 64 else a + 1)
            ins = ins_mask(M64, cov_acc, f_end)
            commit_one_write(table, h, pos, old, ALL_LANES, grp, ins)
            if not continue_generic:
                if anchor < L: has_ins, F0 = True, anchor + 1
                else: has_ins, F0 = False, L
                continue
            ev.add("generic_a0")
            ub = 63
        found = False
        u = ub
        while True:
            if u < 0:
                if has_ins:
                    p = F0 - 1; table[hash4(rd32(src, p))] = p
                u = 0; continue
            if u == 0: pos_, st = F0, 1
            elif u == 1: pos_, st = F0 + 1, 0
            else:
                x = 64 + u - 1; pos_, st = F0 + 1 + S(x) - S(64), x >> 6
            if pos_ + st > L: break
            hh = hash4(rd32(src, pos_)); cand = table[hh]
            valid = cand > 0 and cand < pos_ and cand + 65535 >= pos_ and rd32(src, cand) == rd32(src, pos_)
            table[hh] = pos_
            if valid: found = True; break
            u += 1
        if not found: break
        mlen = extend(src, pos_, cand, 0, match_limit)
        if not emit_general(anchor, pos_ - anchor, pos_ - cand, mlen): return None
        end = pos_ + 4 + mlen; anchor = end
        if end < L: has_ins, F0 = True, end + 1
        else: has_ins, F0 = False, L
    lit = n - anchor
    if lit:
        b = bytes([min(lit, 15) << 4]) + (ext_bytes(lit) if lit >= 15 else b"") + src[anchor:]
        if op + len(b) > dst_len: return None
        out[op:op+len(b)] = b; op += len(b)
    return bytes(out[:op])

if __name__ == "__main__":
    import cases
    from oracle import binding as o
    bad = 0
    allc = cases.reference_test_inputs() + list(cases.kat_inputs().items()) + cases.seeded_cases()
    for name, b in allc:
        if len(b) > 20000: continue
        w = o.compress_default(b); g = compress(b)
        if g != w:
            bad += 1
            first = next((i for i, (x, y) in enumerate(zip(g, w)) if x != y), min(len(g), len(w)))
            print("MISMATCH", name, len(g), len(w), "first diff", first)
    print("bad", bad, "of", len(allc))
