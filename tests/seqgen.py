"""Crafted LZ4 block streams at the sequence level, and a model of the wave decoder's grouping (test infrastructure).

* `corpus()` / `dict_corpus()`: seeded, deterministic streams built from (literals, offset, match length) lists with
  dictgen.seq.  Every valid stream comes with the plaintext the generator built itself (an expectation that does not
  come from the oracle); malformed ones carry None and are judged by the reference restatements.  Each family aims at
  one branch of the batch path of k_decompress_safe (zig-lz4_amd/csrc/zlz4_decompress.hip).
* `model()`: restates the kernel's batch path (the window parse, the token walk with its `room` limit, the `viol` cuts,
  cap_short(), the copy phases) and the single-sequence path in between, and counts what each stream goes through.
  Line cites (:N) are those of zlz4_decompress.hip; src/lz4.zig is the reference decoder.  The -DZLZ4_STAMPS build
  counts the same events in g_zlz4_dstamps (tools/decoder_census.py compares the two).
"""
import random

from dictgen import seq

OUTPUT_TOO_SMALL, CORRUPTED = -1, -3
CAP_DELTAS = (0, -1, -4, 1, 31, 32, 33)        # every valid stream is also decoded at cap = n + d


class Item:
    """One decode: stream `src` into a slot of `cap` bytes; `plain` = the generator's plaintext (None: malformed).
    `dict_bytes` is set for the dictionary families."""
    __slots__ = ("name", "src", "cap", "plain", "dict_bytes")

    def __init__(self, name, src, cap, plain, dict_bytes=None):
        self.name, self.src, self.cap, self.plain, self.dict_bytes = name, src, cap, plain, dict_bytes

    def expected(self):
        """-> bytes, or the status; None when only a reference decoder can tell (malformed streams)"""
        if self.plain is None:
            return None
        if self.cap == 0 and self.src:
            return 0                                  # src/lz4.zig:98
        return self.plain if self.cap >= len(self.plain) else OUTPUT_TOO_SMALL


class _Builder:
    """A stream and the plaintext it decodes to (over the virtual buffer dict ++ output, src/lz4.zig:181-225)."""

    def __init__(self, rng, dict_bytes=b""):
        self.rng, self.d = rng, bytes(dict_bytes)
        self.s, self.out, self.valid, self.ends_with_match = bytearray(), bytearray(), True, False

    @property
    def op(self):
        return len(self.out)

    def lits(self, n):
        return bytes(self.rng.getrandbits(8) for _ in range(n))

    def add(self, lit, off=None, ml=None):
        if isinstance(lit, int):
            lit = self.lits(lit)
        self.s += seq(lit, off, ml)
        self.out += lit
        self.ends_with_match = off is not None
        if off is None or not self.valid:
            return
        if off == 0 or off > self.op + len(self.d) or off > 65535:
            self.valid = False
            return
        for _ in range(ml):                           # byte by byte: overlaps repeat the period (:235-241)
            p = self.op - off
            self.out.append(self.out[p] if p >= 0 else self.d[len(self.d) + p])

    def free_off(self, ml, limit):
        """an offset whose source lies wholly in front of output position `limit` (so no batch grouping can make the
        match read the output of a match of its own batch)"""
        lo = max(0, self.op - 65535)
        hi = limit - ml
        assert hi >= lo, (hi, lo)
        return self.op - self.rng.randint(lo, hi)

    def tail(self):
        """the last literals (0..40 bytes), or nothing: the stream then ends right after a match"""
        if self.rng.random() < 0.3:
            return
        self.add(self.rng.randint(0, 40))

    def item(self, name):
        return name, bytes(self.s), (bytes(self.out) if self.valid else None)


def _short_ml(rng, mix):
    u = rng.random()
    if mix >= 1 and u < 0.25:
        return rng.randint(19, 32)                    # mlc = 15, extension 0..13: a 4-byte sequence
    if mix >= 2 and u < 0.4:
        return rng.randint(33, 48)                    # long: the 16-byte pieces beside the lane copy
    return rng.randint(4, 18)                         # a 3-byte sequence


def _short_runs(rng, k):
    """17..40 sequences without literals after a preamble: only cap_short() (:343-356) cuts their phases"""
    b = _Builder(rng)
    b.add(rng.randint(200, 900), rng.randint(1, 150), rng.randint(4, 18))
    mix = k % 3
    for _ in range(rng.randint(1, 4)):
        start = b.op
        b.add(rng.randint(0, 3), b.free_off(8, start) if b.op >= 8 else 1, 4)
        start = b.op - 4
        for _ in range(rng.randint(17, 40)):
            ml = _short_ml(rng, mix)
            b.add(b"", b.free_off(ml, start), ml)
        b.add(rng.randint(20, 120), b.free_off(6, start), 6)
    b.tail()
    return b.item("short_runs%d" % mix)


def _dep_chains(rng, k):
    """matches that read the output of the match just before (:320 / :444): phase after phase, up to the limit of six
    (:438); some cutting tokens overlap their own output (:446), and some runs end with < min_phase_tokens left (:441)"""
    b = _Builder(rng)
    b.add(rng.randint(200, 600), rng.randint(1, 100), rng.randint(4, 18))
    variant = k % 4
    for _ in range(rng.randint(1, 3)):
        start = b.op
        prev = None                                   # output position / length of the previous match
        n = rng.randint(12, 40)
        for j in range(n):
            lit = 0 if rng.random() < 0.8 else rng.randint(1, 3)
            if variant == 0:
                dep = j % 3 == 0 and j > 0            # [dep, free, free] x 7 per window: six cuts
            elif variant == 1:
                dep = j % 2 == 1                      # [free, dep]
            else:
                dep = j > 0 and rng.random() < (0.3 if variant == 2 else 0.6)
            if dep and prev is not None:
                pm, pl = prev
                self_ov = rng.random() < 0.15
                ml = rng.randint(4, min(18, pl)) if not self_ov else rng.randint(4, 18)
                off = b.op + lit - pm                 # the source starts at the previous match
                if self_ov:
                    off = rng.randint(1, 3) if rng.random() < 0.5 else max(1, min(off, ml - 1))
                b.add(lit, off, ml)
            else:
                ml = rng.randint(4, 18)
                b.add(lit, b.free_off(ml, start), ml)
            prev = (b.op - ml, ml)
        b.add(rng.randint(20, 100), b.free_off(5, start), 5)
    b.tail()
    return b.item("dep_chains%d" % variant)


def _self_overlap(rng, k):
    """off < ml inside a window, right after batched sequences: the single path's overlap branches (:506-509, :589-611)"""
    b = _Builder(rng)
    b.add(rng.randint(300, 1500), rng.randint(1, 200), rng.randint(4, 18))
    for _ in range(rng.randint(2, 8)):
        start = b.op
        for _ in range(rng.randint(2, 12)):
            ml = rng.randint(4, 18)
            b.add(rng.randint(0, 4), b.free_off(ml, start), ml)
        oc = rng.randint(0, 3)
        off = (rng.randint(1, 3), rng.randint(4, 15), rng.randint(16, 63), rng.randint(64, 300))[oc]
        mlc = rng.randint(0, 3)
        ml = (rng.randint(4, 18), rng.randint(19, 32), rng.randint(33, 64), rng.randint(65, 700))[mlc]
        if ml <= off:
            ml = off + rng.randint(1, 40)
        b.add(rng.randint(0, 3), off, ml)
    b.tail()
    return b.item("self_overlap")


_EDGE_LIT = (0, 1, 14, 15, 16, 269, 270)
_EDGE_ML = (4, 7, 8, 15, 16, 17, 18, 19, 31, 32, 33, 273, 274)


def _edges(rng, k):
    """literal runs 0..16 / 269 / 270 (15 and 270 carry the extension bytes 0 and 255, 0), match lengths around every
    class limit (19 and 274: extension byte 0 after the nibble / after 255), offsets that reach output byte 0 exactly"""
    b = _Builder(rng)
    b.add(rng.randint(100, 400), rng.randint(1, 90), rng.randint(4, 18))
    for _ in range(rng.randint(20, 90)):
        lit = rng.choice(_EDGE_LIT) if rng.random() < 0.15 else rng.randint(0, 16)
        ml = rng.choice(_EDGE_ML) if rng.random() < 0.3 else rng.randint(4, 40)
        pr, v = b.op + lit, rng.random()
        if v < 0.1:
            off = pr                                  # the match starts at output byte 0
        elif v < 0.15:
            off = 1
        else:
            off = rng.randint(ml, pr) if pr >= ml else pr
        b.add(lit, off, ml)
    b.tail()
    return b.item("edges")


def _far(rng, k):
    """offsets of 65535 (the largest): the output first grows past 64 KiB with long matches"""
    b = _Builder(rng)
    b.add(3000, rng.randint(1, 3000), 4)
    while b.op < 66000:
        b.add(rng.randint(0, 2), rng.randint(1, min(b.op, 65535)), rng.choice((274, 273, 1000)))
    for _ in range(rng.randint(10, 40)):
        ml = rng.randint(4, 32)
        b.add(rng.randint(0, 3), 65535 if rng.random() < 0.5 else rng.randint(ml, 65535), ml)
    b.tail()
    return b.item("far")


def _exact_len(rng, k):
    """streams of 66..70 bytes: around the ip + 68 <= iend switch (:181)"""
    L = 66 + k % 5
    b = _Builder(rng)
    b.add(8, rng.randint(1, 8), 4)
    while len(b.s) < L - 12:
        ml = rng.randint(4, 8)
        b.add(rng.randint(0, 1), b.free_off(ml, 8), ml)
    if rng.random() < 0.5:
        while len(b.s) + 3 <= L:
            ml = rng.randint(4, 8)
            b.add(b"", b.free_off(ml, 8), ml)
    rest = L - len(b.s)
    if rest > 0:
        b.add(max(0, rest - 1 - (1 if rest - 1 >= 15 else 0)))
    name, s, p = b.item("exact_len")
    return name + str(len(s)), s, p


def _end_at_cap(rng, k):
    """a batch of short sequences that ends with the stream and ends with a match: at cap = n the room test's 32-byte
    slack (:225-227) cuts the walk and the single path finishes"""
    b = _Builder(rng)
    b.add(rng.randint(64, 300), rng.randint(1, 60), rng.randint(4, 18))
    start = b.op
    for _ in range(rng.randint(20, 80)):
        ml = rng.randint(4, 40)
        b.add(rng.randint(0, 2), b.free_off(ml, start), ml)
    return b.item("end_at_cap")


def _malformed(rng, k):
    """offset 0 or offset > op as the 17th sequence of a short run, or inside a later phase; or a match-length
    extension cut off by the end of the stream (that one always lies in the last 68 bytes: only the single path sees it)"""
    b = _Builder(rng)
    b.add(rng.randint(200, 700), rng.randint(1, 150), rng.randint(4, 18))
    start = b.op
    kind, where = k % 3, (k // 3) % 2
    pm = None
    n = 16 if where == 0 else rng.randint(4, 9)
    for j in range(n):
        if where == 1 and j % 3 == 2 and pm is not None:
            ml = 4
            b.add(b"", b.op - pm, ml)                 # depends on the match before: a later phase begins
        else:
            ml = rng.randint(4, 18)
            b.add(b"", b.free_off(ml, start), ml)
        pm = b.op - ml
    op = b.op
    if kind == 0:
        b.s += bytes([rng.randint(0, 14)]) + b"\0\0"                              # offset 0 (:154)
    elif kind == 1:
        off = rng.randint(op + 1, min(65535, op + 3000))
        b.s += bytes([rng.randint(0, 14), off & 255, off >> 8])                  # offset > op (:181-186)
    else:
        b.s += bytes([0x0F, 4, 0])                                               # ml extension missing (:162)
        b.valid = False
        return "malformed%d_%d" % (kind, where), bytes(b.s), None
    b.valid = False
    for _ in range(rng.randint(0, 25)):
        ml = rng.randint(4, 18)
        b.s += seq(b"", 5, ml)
    b.s += seq(b.lits(rng.randint(0, 30)))
    return "malformed%d_%d" % (kind, where), bytes(b.s), None


def _one_past(rng, k):
    """offset = op + 1 exactly (:181-186 / :311, one byte in front of the slot: CorruptedData) as the 17th sequence of a
    short run, inside a later phase, or on the single path (after a literal run too long for the window)"""
    b = _Builder(rng)
    b.add(rng.randint(200, 700), rng.randint(1, 150), rng.randint(4, 18))
    start = b.op
    where = k % 3
    pm = None
    for j in range(16 if where == 0 else (rng.randint(4, 9) if where == 1 else rng.randint(0, 5))):
        if where == 1 and j % 3 == 2 and pm is not None:
            ml = 4
            b.add(b"", b.op - pm, ml)                 # depends on the match before: a later phase begins
        else:
            ml = rng.randint(4, 18)
            b.add(b"", b.free_off(ml, start), ml)
        pm = b.op - ml
    lit = rng.randint(0, 3) if where < 2 else rng.randint(62, 200)
    b.add(lit, b.op + lit + 1, rng.randint(4, 18))
    assert not b.valid
    for _ in range(rng.randint(0, 25)):
        b.s += seq(b"", 5, rng.randint(4, 18))
    b.s += seq(b.lits(rng.randint(0, 30)))
    return "one_past%d" % where, bytes(b.s), None


_FAMILIES = ((_short_runs, 260), (_dep_chains, 260), (_self_overlap, 90), (_edges, 120), (_far, 6),
             (_exact_len, 30), (_end_at_cap, 100))


def corpus(seed=2026, scale=1.0):
    """-> [Item]: every valid stream at every capacity of CAP_DELTAS, then the malformed streams (cap = 4 KiB)"""
    items = []
    for fi, (fam, count) in enumerate(_FAMILIES):
        rng = random.Random(seed * 1000 + fi)
        for k in range(max(1, int(count * scale))):
            name, s, plain = fam(rng, k)
            n = len(plain)
            for d in CAP_DELTAS:
                if n + d >= 0:
                    items.append(Item(name, s, n + d, plain))
    rng = random.Random(seed * 1000 + 99)
    for k in range(max(6, int(120 * scale))):
        name, s, _ = _malformed(rng, k)
        items.append(Item(name, s, 4096, None))
    rng = random.Random(seed * 1000 + 98)
    for k in range(max(3, int(60 * scale))):
        name, s, _ = _one_past(rng, k)
        items.append(Item(name, s, 4096, None))
    return items


# ------------------------------------------------------------------------------------------------ dictionary families
def _dict_stream(rng, k, dct):
    """matches into a dictionary: its first reachable byte, matches that end exactly at its end (off - pr = need,
    need - 1, need + 1 with need = ml or 16, :316-317) and matches that span its end"""
    b = _Builder(rng, dct)
    dl = min(len(dct), 65536)
    for _ in range(rng.randint(10, 40)):
        lit = rng.randint(0, 3)
        ml = rng.randint(4, 40) if rng.random() < 0.8 else rng.randint(41, 300)
        pr = b.op + lit
        u = rng.random()
        if u < 0.15:
            off = pr + dl                             # the first byte the block can reach
        elif u < 0.75:
            need = rng.choice((ml, max(ml, 16), 16))
            off = pr + need + rng.choice((-1, 0, 0, 1))   # ends at / just before / just across the dictionary's end
        elif u < 0.9:
            off = pr + rng.randint(1, max(1, ml - 1)) if ml > 1 else pr + 1   # spans the end
        else:
            off = pr + rng.randint(1, dl)
        off = max(1, min(off, pr + dl, 65535))
        b.add(lit, off, ml)
    if k % 7 == 3:                                    # one byte too far (:190): CorruptedData
        lit = rng.randint(0, 3)
        off = b.op + lit + 1 + dl
        if off <= 65535:
            b.add(lit, off, 4)
            b.add(10, 5, 4)
    b.tail()
    return b.item("dict%d" % dl)


def dict_corpus(seed=7, count=300):
    """-> [Item] with dict_bytes set; dictionaries of 5, 64, 1000, 65536 and 70000 bytes"""
    rng = random.Random(seed)
    dicts = [bytes(rng.getrandbits(8) for _ in range(n)) for n in (5, 64, 1000, 65536, 70000)]
    items = []
    for k in range(count):
        dct = dicts[k % len(dicts)]
        name, s, plain = _dict_stream(rng, k, dct)
        if plain is None:
            items.append(Item(name, s, 8192, None, dct))
        else:
            d = CAP_DELTAS[k % len(CAP_DELTAS)]
            items.append(Item(name, s, max(0, len(plain) + d), plain, dct))
    return items


# ------------------------------------------------------------------------------------------------ the model
class Counts:
    FIELDS = ("batches", "batch_seqs", "later_phases", "cap_cuts", "phase_limit", "room_cuts", "single_seqs",
              "ends_with_match", "phases3")

    def __init__(self):
        for f in self.FIELDS:
            setattr(self, f, 0)
        self.ml_hist, self.lit_hist = {}, {}

    def add(self, o):
        for f in self.FIELDS:
            setattr(self, f, getattr(self, f) + getattr(o, f))
        for h, oh in ((self.ml_hist, o.ml_hist), (self.lit_hist, o.lit_hist)):
            for k, v in oh.items():
                h[k] = h.get(k, 0) + v

    def row(self):
        return {f: getattr(self, f) for f in self.FIELDS}


def _parse(src, ip, i):
    """lane i of the window parse (:206-222) -> (ok, nxt, lit, ml, off, ol); bytes up to ip + 66 exist (ip + 68 <= iend)"""
    b0 = src[ip + i]
    lit, hl, cx = b0 >> 4, 1, False
    if lit == 15:                                     # :212, one extension byte
        b1 = src[ip + i + 1]
        cx = b1 == 255
        lit += b1
        hl = 2
    mpos = i + hl + lit                               # :213
    mlc, slen = b0 & 15, hl + lit + 2
    off = 0
    if mpos <= 63:
        off = src[ip + mpos] | (src[ip + mpos + 1] << 8)   # :214-215
        if mlc == 15:                                 # :217
            e2 = src[ip + mpos + 2]
            cx = cx or e2 == 255
            mlc += e2
            slen += 1
    ml = mlc + 4
    nxt = i + slen
    ok = (not cx) and mpos <= 63 and nxt <= 64 and off != 0   # :220
    return ok, nxt, lit, ml, off, lit + ml


def _single(src, ip, op, oend, dlen, lo):
    """one sequence through the single-sequence paths (:483-612, the reference's order of checks) -> (ip, op, err)"""
    iend = len(src)
    token = src[ip]; ip += 1
    lit = token >> 4
    if lit == 15:
        while True:
            if ip >= iend:
                return ip, op, CORRUPTED
            s = src[ip]; ip += 1
            lit += s
            if s != 255:
                break
    if lit > 0:
        if lit > iend - ip:
            return ip, op, CORRUPTED
        if lit > oend - op:
            return ip, op, OUTPUT_TOO_SMALL
        ip += lit; op += lit
    if ip >= iend:
        return ip, op, "end"
    if iend - ip < 2:
        return ip, op, CORRUPTED
    off = src[ip] | (src[ip + 1] << 8); ip += 2
    if off == 0:
        return ip, op, CORRUPTED
    ml = token & 15
    if ml == 15:
        while True:
            if ip >= iend:
                return ip, op, CORRUPTED
            s = src[ip]; ip += 1
            ml += s
            if s != 255:
                break
    ml += 4
    if ml > oend - op:
        return ip, op, OUTPUT_TOO_SMALL
    if off > op:
        if off - op > dlen:
            return ip, op, CORRUPTED
    elif off + lo > op:
        return ip, op, CORRUPTED
    return ip, op + ml, None


def model(src, cap, lane_copy, phases, min_phase_tokens=3, write=True, dlen=0, lo=0):
    """k_decompress_safe<write, lane_copy, phases, dlen > 0 (kDict), lo > 0 (kBound)> on one stream -> (result, Counts).
    dlen = the reachable dictionary length (kDict), lo = the StreamDecode bound (kBound)."""
    c = Counts()
    src = bytes(src)
    iend, oend = len(src), cap
    ip = op = 0
    kdict = dlen > 0
    short_max = 32 if lane_copy else 0
    if iend == 0 or oend == 0:                        # :112
        return 0, c
    last_match = False
    while True:
        if ip >= iend:                                # :170
            break
        if ip + 68 <= iend:                           # :181
            while True:
                P = {}

                def lane(i):
                    if i not in P:
                        P[i] = _parse(src, ip, i)
                    return P[i]
                orem = oend - op                      # :225-227
                room0 = (orem - 32 if orem >= 32 else 0) if write else orem
                room = min(room0, 4095)
                fast = room0 >= 7100 and lane(0)[0]   # :239: the walk without the room test
                # the walk (:231): take tokens while they are ok and (slow walk) fit in room
                R, T, pos, room_cut = [], 0, 0, False
                while pos < 64:
                    ok, nxt, lit, ml, off, ol = lane(pos)
                    if not ok:
                        break
                    if not fast and T + ol > room:
                        room_cut = True
                        break
                    R.append(pos)
                    T += ol
                    pos = nxt
                R_walk, T_walk, pos_walk = list(R), T, pos
                relv, acc = {}, 0                     # :307 output offset of each token inside the batch
                for t in R:
                    relv[t] = acc
                    acc += lane(t)[5]
                op0 = op
                viol_err = {}
                if R:
                    lit0 = lane(0)[2]
                    viol = []
                    for t in R:
                        ok, nxt, lit, ml, off, ol = lane(t)
                        ve = off + lo > op0 + relv[t] + lit                          # :311
                        if kdict:                                                   # :312-318
                            pr = op0 + relv[t] + lit
                            need = ml if lane_copy else max(ml, 16)
                            ve = ve and (((off - pr) & 0xFFFFFFFF) < need or ((off - pr) & 0xFFFFFFFF) > dlen)
                        viol_err[t] = ve
                        viol.append(ve or (write and off + lit0 < relv[t] + ol))    # :319-320
                    fb = next((t for t, v in zip(R, viol) if v), None)              # :321-327
                    if fb is not None:
                        R = [t for t in R if t < fb]
                        T = relv[fb]
                        pos = fb
                if not R:                             # :333
                    break
                if room_cut:
                    c.room_cuts += 1
                c.batches += 1

                def cap_short(R, T, pos):             # :343-356
                    if write and lane_copy and len(R) > 16:
                        S = [t for t in R if lane(t)[3] <= short_max]
                        if len(S) > 16:
                            fb = S[16]
                            c.cap_cuts += 1
                            return [t for t in R if t < fb], relv[fb], fb
                    return R, T, pos

                def take(R):
                    c.batch_seqs += len(R)
                    for t in R:
                        _, _, lit, ml, _, _ = lane(t)
                        c.ml_hist[ml] = c.ml_hist.get(ml, 0) + 1
                        c.lit_hist[lit] = c.lit_hist.get(lit, 0) + 1
                R, T, pos = cap_short(R, T, pos)      # :431
                take(R)
                nphases = 1
                if write and phases:                  # :437-462
                    phase = 1
                    while phase < 6 and pos != pos_walk:
                        first, tbase = pos, T
                        Rn = [t for t in R_walk if t >= first]
                        if len(Rn) < min_phase_tokens:                               # :441
                            break
                        lit_f = lane(first)[2]
                        vmn = [t for t in Rn if viol_err[t] or lane(t)[4] + lit_f < (relv[t] - tbase) + lane(t)[5]]
                        if vmn and vmn[0] == first:                                  # :446
                            break
                        if vmn:
                            fb = vmn[0]
                            R, T, pos = [t for t in Rn if t < fb], relv[fb], fb
                        else:
                            R, T, pos = Rn, T_walk, pos_walk
                        c.later_phases += 1
                        R, T, pos = cap_short(R, T, pos)                             # :458
                        take(R)
                        nphases += 1
                        phase += 1
                    if phase == 6 and pos != pos_walk:
                        c.phase_limit += 1
                if nphases >= 3:
                    c.phases3 += 1
                last_match = True
                op += T                               # :463-464
                ip += pos
                if ip + 68 > iend:
                    break
            if ip >= iend:                            # :476
                break
        c.single_seqs += 1                            # :479
        ip, op, err = _single(src, ip, op, oend, dlen, lo)
        if err == "end":                              # literals only: the last sequence (:146)
            last_match = False
        elif err is not None:
            return err, c
        else:
            last_match = True
    c.ends_with_match = int(last_match)
    return op, c
