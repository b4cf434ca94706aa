"""Python restatement of lz4.compressDestSize (reference src/lz4.zig:551-616) on top of ONE full-length compression.

Test infrastructure like zig_lz4_pyref.py: never imported by the product, the bench or smoke().  It states the rules
that the batch kernel k_dest_size_plan (zig-lz4_amd/csrc/zlz4_dest_size.hip) follows:

compressDefault (:292-447) depends on the input length only through mflimitPlusOne = srcSize - 12 and matchLimit =
srcSize - 5 (:313-314).  So the stream of compressDefault(src[:m]) equals the stream of compressDefault(src) up to the
first sequence that notices the shorter length, followed by a short re-encoded tail.  Per sequence j of the full
stream: a = literal start, p = match position, e = match end, O = stream offset of its token and f = the forwardIp of
the attempt that found the match (:327-333; with acceleration 1 the attempts from s = a + 1 visit s, then s + 1 + S(t)
for t >= 1, S(t) = sum_{y < t} (y >> 6), and the step taken after attempt t is 1 for t = 0, else t >> 6).

Sequence j is reproduced unchanged in compressDefault(src[:m]) iff f_i <= m - 12 and e_i <= m - 13 for all i <= j.
With c_j = max(f_j + 12, e_j + 13) and C_j its running maximum, the shared sequences are k(m) = #{j : C_j <= m}.

compressDestSize replays the reference's search probe for probe: fits(m) is NOT monotone in m.
"""
from zig_lz4_pyref import ML_BITS, RUN_MASK, _put_len

MFLIMIT, LASTLITERALS, MINMATCH = 12, 5, 4            # src/lz4.zig:12-15


def compress_bound(n):                                # :80-83
    return n + n // 255 + 16


def step_after(lit):
    """sigma(t) of the attempt that found a match `lit` bytes after its literal start a (the search starts at a + 1)"""
    d = lit - 1                                       # p - s
    if d == 0:
        return 1                                      # attempt 0: step = acceleration
    if d == 1:
        return 0                                      # attempt 1 (attempts 1..64 all visit s + 1)
    D, q = d - 1, 1                                   # s + 1 + S(t) = p: the first such t is 64 q + r, step q
    while 32 * (q + 1) * q <= D:
        q += 1
    return q


def parse(stream, n):
    """sequences of a compressDefault stream of an n-byte input (n >= 13): [(O, a, lit, p, e, off, f)] and the offset of
    the last-literals token"""
    seqs, O, a = [], 0, 0
    while True:
        tok = stream[O]
        q, lit = O + 1, tok >> 4
        if lit == 15:
            while True:
                b = stream[q]
                q += 1
                lit += b
                if b != 255:
                    break
        q += lit
        if q >= len(stream):
            assert a + lit == n
            return seqs, O
        off = stream[q] | stream[q + 1] << 8
        q += 2
        ml = tok & 15
        if ml == 15:
            while True:
                b = stream[q]
                q += 1
                ml += b
                if b != 255:
                    break
        p = a + lit
        e = p + ml + MINMATCH
        seqs.append((O, a, lit, p, e, off, p + step_after(lit)))
        O, a = q, e


def _len_bytes(v):                                    # token nibble + 255-run for a length v
    return 0 if v < 15 else 1 + (v - 15) // 255


def _last_lits_size(lit):
    return 0 if lit == 0 else 1 + _len_bytes(lit) + lit


class Plan:
    """the full stream of src, parsed once; size(m) / derive(m) answer for every prefix length m"""

    def __init__(self, src, full_stream):
        self.src, self.full, self.n = bytes(src), bytes(full_stream), len(src)
        self.seqs, self.last_O = parse(self.full, self.n) if self.n >= 13 else ([], 0)
        self.C, c = [], 0
        for (_, _, _, _, e, _, f) in self.seqs:
            c = max(c, f + MFLIMIT, e + MFLIMIT + 1)
            self.C.append(c)

    def _tail(self, m):
        """(prefix length of the full stream, sequence to re-emit or None, anchor of the last literals)"""
        lo, hi = 0, len(self.C)                       # k = #{j : C_j <= m}
        while lo < hi:
            mid = (lo + hi) // 2
            if self.C[mid] <= m:
                lo = mid + 1
            else:
                hi = mid
        k = lo
        if k == len(self.seqs):
            return self.last_O, None, self.seqs[-1][4] if k else 0
        O, a, lit, p, e, off, f = self.seqs[k]
        if f <= m - MFLIMIT:                          # tail case 1: found again, extension stops at m - 5
            e2 = min(e, m - LASTLITERALS)
            return O, (a, lit, p, e2, off), e2
        return O, None, a                             # tail case 2: the search bails, a = e_k

    def size(self, m):
        if m == 0:
            return 0
        if m < MFLIMIT + 1:
            return 1 + _len_bytes(m) + m              # compressAsLiterals
        O, seq, anchor = self._tail(m)
        s = O + _last_lits_size(m - anchor)
        if seq:
            a, lit, p, e2, off = seq
            s += 1 + _len_bytes(lit) + lit + 2 + _len_bytes(e2 - p - MINMATCH)
        return s

    def derive(self, m):
        """the bytes of compressDefault(src[:m])"""
        if m == 0:
            return b""
        out = bytearray()
        if m < MFLIMIT + 1:
            anchor = 0
        else:
            O, seq, anchor = self._tail(m)
            out += self.full[:O]
            if seq:
                a, lit, p, e2, off = seq
                ml = e2 - p - MINMATCH
                out.append((min(lit, 15) << ML_BITS) | min(ml, 15))
                if lit >= RUN_MASK:
                    _put_len(out, lit - RUN_MASK)
                out += self.src[a:p]
                out += bytes((off & 255, off >> 8))
                if ml >= 15:
                    _put_len(out, ml - 15)
        lit = m - anchor
        out.append(min(lit, 15) << ML_BITS)
        if lit >= RUN_MASK:
            _put_len(out, lit - RUN_MASK)
        out += self.src[anchor:m]
        return bytes(out)


def search(n, cap, size):
    """the reference's search (:567-612) with size(m) = len(compressDefault(src[:m])): -> (result, consumed)"""
    if n == 0:                                        # :553-556
        return 0, 0
    if cap >= compress_bound(n):                      # :559-564
        return size(n), n
    low, high, best, best_c = 1, n, 0, 0
    if cap <= n:                                      # :573-586: first probe at m = cap (cap == 0: m = 0 fits)
        s = size(cap)
        if s <= cap:
            best, best_c, low = cap, s, cap + 1
        else:
            high = cap - 1
    while low <= high:                                # :589-612
        mid = low + (high - low) // 2
        if mid == 0 or mid > n:
            break
        s = size(mid)
        if s <= cap:
            best, best_c = mid, s
            if mid == n:
                break
            low = mid + 1
        else:
            high = mid - 1
        if low > n:
            break
    return best_c, best


def compress_dest_size(src, cap, full_stream):
    """-> (result, consumed, output bytes), full_stream = compressDefault(src)"""
    plan = Plan(src, full_stream)
    r, consumed = search(len(src), cap, plan.size)
    return r, consumed, plan.derive(consumed)
