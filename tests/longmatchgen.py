"""Crafted LZ4 block streams around the LONG matches of the wave decoder's batch path (test infrastructure).

k_decompress_safe (zig-lz4_amd/csrc/zlz4_decompress.hip) copies a batched match of more than 32 bytes (lane-copy build;
32 or more in the sequence-lane build) in 16-byte pieces held by the token's lane and by the two lanes above it, up to
96 bytes; what is longer keeps a load -> store loop.  Every stream here is built with the builder of tests/seqgen.py and
puts such matches at chosen window lanes: after a preamble that only the single-sequence path takes (a literal run
whose first extension byte is 255), the next token is lane 0 of a 64-byte window, 3-byte sequences (plus literals) fill
the window up to the wanted lane, and a literal tail keeps the stream >= 68 bytes past the window's start but too short
for a second window -- so a stream is ONE batch, and the long match is in it.

A match of 19..273 bytes takes a 4-byte sequence (token, offset, one extension byte), so two such tokens are at least
four lanes apart and the highest lane of one is 60; at lane 61 the token does not fit the window and opens the next one.

`shorten=True` builds the twin of a stream: the same sequences, every match of 32 bytes or more replaced by one of
19..31 (the same 4-byte sequence), offsets recomputed from the same anchors.  The grouping the decoder makes must not
depend on it (tests/test_long_match_corpus_cpu.py)."""
import random

from seqgen import Item, _Builder

MLS = (31, 32, 33, 34, 47, 48, 49, 63, 64, 65, 79, 80, 81, 95, 96, 97, 112, 273)
LANES = (0, 13, 14, 15, 16, 29, 30, 31, 32, 45, 46, 47, 48, 60, 61)
ROOMY = 7200            # cap - n from which the walk runs without its room test (room0 >= 7100, :239)
LONG = 32               # a match longer than this takes the helper lanes in both builds; the sequence-lane build's old
                        # copy loop also ran for exactly 32, so the twins shorten from 32 on


class _W:
    """one stream: preamble, one window of sequences, tail"""

    def __init__(self, rng, shorten, dict_bytes=b""):
        self.rng, self.shorten = rng, shorten
        self.b = b = _Builder(rng, dict_bytes)
        b.add(rng.randint(300, 420), rng.randint(1, 200), rng.randint(4, 18))   # 15, 255, x: the single path's
        self.start = b.op                             # output position of the window
        self.ws = len(b.s)                            # stream position of the window
        self.first_match = None                       # output position of the window's first match

    @property
    def lane(self):
        return len(self.b.s) - self.ws

    def ml(self, ml):
        return 19 + ml % 13 if self.shorten and ml >= LONG else ml

    def match(self, lit, ml, src_end=None):
        """a match of ml bytes whose source ends at output position src_end (default: somewhere in the preamble)"""
        b, ml = self.b, self.ml(ml)
        r = self.rng.randint(274, self.start)          # (drawn whatever ml is: the twin draws the same)
        if src_end is None:
            src_end = r
        pos = b.op + lit
        if self.first_match is None:
            self.first_match = pos
        b.add(lit, pos - (src_end - ml), ml)
        return pos, ml

    def fill(self, lane):
        """sequences of three bytes and a literal or two (matches of 4..18) up to window lane `lane`: at most 15, so that
        with the matches behind them a window holds no more than 16 and cap_short() (:343-356) cuts neither a stream nor
        its twin"""
        todo = lane - self.lane
        assert todo == 0 or todo >= 3, todo
        k = max(1, todo // 4) if todo else 0
        lits = [0] * k
        for j in range(todo - 3 * k):
            lits[j % k] += 1
        for lit in lits:
            self.match(lit, self.rng.randint(4, 18))
        assert self.lane == lane, (self.lane, lane)

    def new_window(self):
        self.ws, self.start, self.first_match = len(self.b.s), self.b.op, None

    def close(self, name, tail=None):
        """short sequences up to lane >= 40, then literals that end the stream 68..(lane + 67) bytes past the window"""
        while self.lane < 40:
            self.match(0, self.rng.randint(4, 18))
        p = self.lane
        assert p <= 64, p
        t = max(6, 68 - p) + self.rng.randint(0, 8) if tail is None else tail
        t += t == 16                                  # (15 literals take a second header byte)
        assert p + t >= 68 and t < 68
        self.b.add(t - (1 if t - 1 < 15 else 2))
        assert len(self.b.s) - self.ws == p + t
        return self.b.item(name)


def _ml_lane(rng, shorten, ml, lane):
    w = _W(rng, shorten)
    w.fill(lane)
    if lane > 60:                                     # the token does not fit: it is lane 0 of the next window
        w.new_window()
    w.match(0, ml)
    return w.close("ml%d_lane%d" % (ml, lane))


def _pair(rng, shorten, ml1, ml2, lane, lead_short):
    """two long matches in sequences back to back (lanes t and t + 4), or behind a 3-byte sequence (t, t + 3, t + 7)"""
    w = _W(rng, shorten)
    w.fill(lane)
    if lead_short:
        w.match(0, rng.randint(4, 18))
    w.match(0, ml1)
    w.match(0, ml2)
    return w.close("pair%d_%d_lane%d%s" % (ml1, ml2, lane, "s" if lead_short else ""))


def _beside_short(rng, shorten, ml, lane):
    """a long match between matches the lane copy moves: 3-byte sequences and a 4-byte one of 19..32"""
    w = _W(rng, shorten)
    w.fill(lane)
    w.match(0, rng.randint(19, 32))
    w.match(0, ml)
    w.match(0, rng.randint(19, 32))
    w.match(1, rng.randint(4, 18))
    return w.close("beside_short%d_lane%d" % (ml, lane))


def _phases(rng, shorten, ml2, ml3):
    """a long match in the second and in the third copy phase: a phase ends in front of a match that reads the match just
    before it (:320 / :444); the cutting match and two more tokens open the next one (min_phase_tokens = 3)"""
    w = _W(rng, shorten)
    w.match(rng.randint(0, 2), rng.randint(8, 18))
    prev, pml = w.match(0, rng.randint(8, 18))
    for ml in (ml2, ml3):
        p, m = w.match(0, 4 + rng.randint(0, 4), src_end=prev + pml)   # reads the match before: the phase ends here
        w.match(0, ml)
        w.match(rng.randint(0, 1), rng.randint(4, 18))
        prev, pml = w.match(0, rng.randint(8, 18))
    return w.close("phases%d_%d" % (ml2, ml3))


def _src_edge(rng, shorten, ml, lane, d):
    """the long match's source ends at the phase's first match + d (d = 1: it reads that match's first byte, :320)"""
    w = _W(rng, shorten)
    w.fill(lane) if lane else w.match(rng.randint(0, 3), rng.randint(4, 18))
    fm = w.first_match
    w.match(0, ml, src_end=fm + d)
    return w.close("src_edge%d_lane%d_d%d" % (ml, lane, d))


def _near_end(rng, shorten, ml, tail):
    """the long match at lane 60 (57 with a 3-byte sequence behind it), then `tail` < 32 bytes of output"""
    w = _W(rng, shorten)
    w.fill(60)
    w.match(0, ml)
    return w.close("near_end%d_tail%d" % (ml, tail), tail=tail + 1)


def streams(seed=2027, shorten=False):
    """-> [(name, stream, plaintext)], the same list for the same seed; shorten: the twins (see the module's text)"""
    out = []
    rng = random.Random(seed)
    for ml in MLS:
        for lane in LANES:
            out.append(_ml_lane(rng, shorten, ml, lane))
    for ml1, ml2 in ((33, 96), (64, 65), (97, 49), (273, 34), (80, 81), (48, 112), (96, 97), (95, 33), (34, 64), (65, 79),
                     (49, 48), (63, 273)):
        for lane in (0, 12, 13, 14, 28, 29, 44, 52):
            for lead in (False, True):
                out.append(_pair(rng, shorten, ml1, ml2, lane, lead))
    for ml in (33, 48, 49, 64, 65, 80, 81, 96, 97, 273):
        for lane in (0, 9, 12, 27, 42):
            out.append(_beside_short(rng, shorten, ml, lane))
    for ml2 in (33, 49, 65, 81, 96, 97):
        for ml3 in (34, 64, 80, 95, 112, 273):
            out.append(_phases(rng, shorten, ml2, ml3))
    for ml in (33, 48, 65, 96, 97):
        for lane in (0, 13, 30, 47):
            for d in (-1, 0, 1):
                out.append(_src_edge(rng, shorten, ml, lane, d))
    for ml in (33, 64, 96, 112):
        for tail in (5, 16, 31):
            out.append(_near_end(rng, shorten, ml, tail))
    return out


# capacities beside the plaintext's length n: roomy (the walk without its room test), then the room-tested walk -- the
# match within the last 7100 bytes of the slot -- down to the slot that ends with the stream
CAP_DELTAS = (ROOMY, ROOMY + 1, 7000, 100, 33, 32, 31, 0)


def damage(rng, s):
    """one byte flipped (not in the preamble's literals: past them the bytes are tokens, offsets and lengths) or the end
    cut off"""
    s = bytearray(s)
    if rng.random() < 0.25:
        return bytes(s[:rng.randint(len(s) - 80, len(s) - 1)])
    i = rng.randint(len(s) - 110, len(s) - 1)
    s[i] ^= 1 << rng.randrange(8)
    return bytes(s)


def corpus(seed=2027, min_items=6144):
    """-> [Item]: every stream at every capacity of CAP_DELTAS, then damaged copies at the roomy capacity (plain = None:
    the oracle judges them) until there are min_items"""
    base = streams(seed)
    items = [Item(name, s, len(p) + d, p) for name, s, p in base for d in CAP_DELTAS]
    rng = random.Random(seed + 1)
    k = 0
    while len(items) < min_items or k < 2 * len(base):
        name, s, p = base[k % len(base)]
        items.append(Item(name + "_damaged", damage(rng, s), len(p) + ROOMY, None))
        k += 1
    return items


def dict_streams(seed, shorten=False):
    """the long match with its source wholly in the dictionary (ending at its last byte, and earlier), wholly in dst, and
    across the dictionary's end (the single path) -> [(name, stream, plaintext, dictionary)]"""
    rng = random.Random(seed)
    dicts = [bytes(rng.getrandbits(8) for _ in range(n)) for n in (300, 4096, 70000)]
    out = []
    for ml in MLS:
        for lane in (0, 14, 31, 48):
            for where in ("dict_end", "dict", "dst", "span"):
                dct = dicts[(ml + lane) % 3]
                w = _W(rng, shorten, dct)
                w.fill(lane)
                m = w.ml(ml)
                u = rng.random()                       # (one draw whatever m is: the twin draws the same)
                back = {"dict_end": m, "dict": m + int(u * (min(len(dct), 60000) - m)), "dst": None,
                        "span": 1 + int(u * (m - 1))}[where]
                w.match(0, ml, src_end=None if back is None else m - back)
                name, s, p = w.close("%s%d_lane%d" % (where, ml, lane))
                out.append((name, s, p, dct))
    return out


def dict_corpus(seed=11, min_items=6144):
    base = dict_streams(seed)
    items = [Item(name, s, len(p) + d, p, dct) for name, s, p, dct in base for d in (ROOMY, 100, 32, 0)]
    rng = random.Random(seed + 1)
    k = 0
    while len(items) < min_items:
        name, s, p, dct = base[k % len(base)]
        if k < len(base):
            items.append(Item(name + "_damaged", damage(rng, s), len(p) + ROOMY, None, dct))
        else:
            items.append(Item(name, s, len(p) + ROOMY + 1 + k % 7, p, dct))
        k += 1
    return items
