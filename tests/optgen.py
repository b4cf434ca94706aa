"""Blocks built on the edges of the level 10-12 price parser (compressOptimal, src/lz4hc.zig:1068-1391) for
tests/test_opt_corpus_cpu.py and tests/test_gpu_opt_corpus.py: windows of 1000 records and more, the early-encode exits,
price ties and the ends of a block.  On the GPU the parse runs in k_hc_opt_parse_wave (blocks <= 64 KiB), which keeps
records 0..999 of opt[] packed in LDS and the rest as structs in HBM, or in k_hc_opt_parse<uint64_t>.

A pure generator: no GPU, no oracle.  `cases()` gives [(family, name, bytes, meta)].  meta holds

  levels    the levels the case is meant for
  witness   {counter: value} the oracle's counters (oracle.binding.OPT_STATS) must show at every such level, by
            construction; a value may be a (lo, hi) range
  decodes   whether the oracle's stream decodes back to the block (False: the early-encode exit walked forward without
            the reverse traversal; None: the oracle returns OutputTooSmall because that walk left the
            anchor past the end of the input)
  twin      the name of the case on the other side of the edge, where there is one
  probe / parse   (price family) the region of the block and the (position - probe start, match length) pairs of the
            sequences that must start in it

The building block is the chain.  R is random without a zero byte, a_i = 100 i + 10.  Part one is R, then for every i
the bridge  00 00 R[a_i + 10 : a_i + len_i] R[a_(i+1) : a_(i+1) + 25].  Part two is the pieces R[a_i : a_i + len_i]
back to back (len_i = 50 but for the first and the last).  At a piece's start the search finds the piece, ten bytes on
the bridge, which ends 25 bytes into the next piece: last_match_pos always lies ahead of cur, and ONE window grows by 50
records per piece, through accepted updates only.  (a_0 is not 0: position 0 is never a match source.)

In front of a window lie literals only if every window before it was a literal one, and those are 3 records long
(firstMatch.len == 3): a window's llen is a multiple of 3.  A literal run of F bytes in front of part two therefore
gives llen = F - F % 3, and the first piece is found at cur = F % 3 with the literal length F.

No case holds a run of one byte longer than 8 (level 12 is slow inside runs), and every byte is fixed by a seed.
"""
import numpy as np

SPLIT = 1000                                          # kOptLds: the first record k_hc_opt_parse_wave keeps in HBM
OPT_NUM = 4096
LEVELS = (10, 11, 12)
SUFFICIENT = {10: 64, 11: 128, 12: 4095}              # level -> sufficient_len (targetLength, clamped to OPT_NUM - 1)

WINDOW_SIZES = tuple(range(996, 1004)) + (1063, 1064, 1065, 1500, 2047, 2048, 2049)
WINDOW_FIRST = (47, 48, 49)                           # a first piece this long puts a piece boundary on 997, 998, 999
OPTNUM_FRONTS = (0, 14, 15, 270)
OPTNUM_SEEDS = (1, 2)
LONG_PAIR_Q = {4095: 1996, 4096: 1995}                # len + cur at the decisive position -> len(Q)
ENDS_CUT = (12, 13, 20)
PRICE_LLEN = (14, 15, 16, 269, 270, 271)
PRICE_MLEN = (18, 19, 20, 273, 274)


def rnd(n, seed):
    return np.random.default_rng(seed).integers(1, 256, n, dtype=np.uint8).tobytes()


def lit_price(ll):                                    # literalsPrice :466-472
    return ll + (1 + (ll - 15) // 255 if ll >= 15 else 0)


def seq_price(ll, ml):                                # sequencePrice :476-486
    return 3 + lit_price(ll) + (1 + (ml - 19) // 255 if ml >= 19 else 0)


def chain_parts(n, seed, first=50, last=50, bridge=25, last_bridge=None):
    """-> (part one, part two) of a chain of n pieces; last_bridge: how far the last bridge but one reaches into the
    last piece (which has no bridge of its own to anything)"""
    r = rnd(max(100 * (n + 1) + 60, 100 * n + 20 + max(last, bridge)), seed)
    a = [100 * i + 10 for i in range(n + 1)]
    ln = [50] * n
    ln[0], ln[-1] = first, last
    br = [bridge] * n
    if last_bridge is not None:
        br[n - 2] = last_bridge
    one = r + b"".join(b"\0\0" + r[a[i] + 10:a[i] + ln[i]] + r[a[i + 1]:a[i + 1] + br[i]] for i in range(n))
    return one, b"".join(r[a[i]:a[i] + ln[i]] for i in range(n))


def front_run(f, seed):
    """the f literals in front of part two: none, or 00 00 00 and random bytes"""
    assert f == 0 or f >= 3
    return b"" if f == 0 else b"\0\0\0" + rnd(f - 3, seed + 2000)


def chain(n, seed=1, first=50, last=50, front=3, tail=40, cut=None):
    """part one, `front` literals, part two, `tail` random bytes; `cut` keeps only the first `cut` bytes of part two and
    no tail"""
    one, two = chain_parts(n, seed, first, last)
    if cut is not None:
        return one + front_run(front, seed) + two[:cut]
    return one + front_run(front, seed) + two + rnd(tail, seed + 1000)


def tie_chain(m, front):
    """A chain whose last piece, m bytes, lies on records 990 .. 990 + m and is reached by nothing else (the bridge
    before it ends on record 1000): whether it is taken whole or as a literal and m - 1 bytes is decided by comparing
    a price computed from records below the split with one stored above it (choice()).  -> (block, probe)"""
    one, two = chain_parts(21, 81, first=40, last=m, last_bridge=10)
    head = one + front
    return head + two + rnd(40, 82), (len(head) + 990, len(head) + 990 + m)


def _pieces_for(t):
    """(pieces, length of the last) of a chain whose window ends at record t"""
    rem = t % 50
    return (t // 50, 50 + rem) if rem < 13 else (t // 50 + 1, rem)


def _window():
    out = []
    for t in WINDOW_SIZES:
        n, last = _pieces_for(t)
        w = dict(max_window=t, exit_optnum=0, exit_sufficient=0, first_sufficient=0)
        if t >= SPLIT:                                # the last piece's update writes records on both sides, the
            w.update(x_match=(1, 99), x_hop=1)        # traversal starts beyond and hops back across
        elif t + 3 >= SPLIT:
            w.update(x_trail=(1, 99) if t + 1 < SPLIT else 0, hi_trail=(1, 99), hi_match=0, hi_hop=0)
        else:
            w.update(hi_trail=0, hi_match=0)
        if t >= 1063:
            w.update(hi_back=(1, 999), hi_hop=(2, 999))
        out.append(("window", "window/t%d" % t, chain(n, seed=1, last=last),
                    dict(levels=LEVELS, witness=w, decodes=True, pieces=n)))
    for first in WINDOW_FIRST:                        # the boundary on 997 .. 999: the literal pass, the trailing
        w = dict(max_window=1150 + first, exit_optnum=0, exit_sufficient=0, x_hop=1, x_match=(1, 99))   # literals and
        w.update({47: dict(x_lit=2, x_trail=(1, 99), x_back=0),                                          # opt[cur - ll]
                  48: dict(x_lit=1, x_trail=(1, 99), x_back=1),
                  49: dict(x_lit=0, x_trail=0, x_back=2)}[first])
        out.append(("window", "window/first%d" % first, chain(24, seed=1, first=first),
                    dict(levels=LEVELS, witness=w, decodes=True, pieces=24)))
    for m in (18, 19, 20):                            # a price tie across the split decides the last sequence
        b, probe = tie_chain(m, b"\0\0\0")
        k = choice(0, m, 3)
        out.append(("window", "window/tie/m%d" % m, b,
                    dict(levels=LEVELS, witness=dict(max_window=990 + m, exit_optnum=0, exit_sufficient=0, x_hop=1),
                         decodes=True, probe=probe, parse=[(k, m - k)], twin="window/tie/m%d" % (19 if m != 19 else 18))))
    return out


def long_pair(lq, c=1038, seed=5):
    """P 000 P[c:] Q 000 rnd(7) P Q rnd(40): the window starts with P (2100 records); at cur = c + 3 - (the three
    literal records in front) the search finds P[c:] Q, whose end is record 2100 + len(Q)"""
    p, q = rnd(2100, seed), rnd(lq, seed + 1)
    return p + b"\0\0\0" + p[c:] + q + b"\0\0\0" + rnd(7, seed + 2) + p + q + rnd(40, seed + 3)


def _optnum():
    out = []
    for seed in OPTNUM_SEEDS:
        for f in OPTNUM_FRONTS:
            llen = f - f % 3
            w = dict(exit_optnum=1, exit_sufficient=0, max_optnum_llen=llen, max_window_llen=llen,
                     max_window=4075 + f % 3, min_optnum_sum=4100 + f % 3, hi_match=(3000, 9999), x_match=(1, 99))
            out.append(("optnum", "optnum/chain100/s%d/f%d" % (seed, f), chain(100, seed=seed, front=f),
                        dict(levels=LEVELS, witness=w, decodes=False, front=f)))
    for total, lq in LONG_PAIR_Q.items():
        if total < OPT_NUM:                           # the window grows to 4095: records up to 4098 are written
            w = dict(exit_optnum=0, max_window=4095, max_noexit_sum=4095, x_hop=(1, 9))
            dec = True
        else:                                         # the exit; its forward walk leaves the anchor past the input
            w = dict(exit_optnum=1, min_optnum_sum=4096, max_window=(2100, 2101))
            dec = None
        out.append(("optnum", "optnum/long_pair/sum%d" % total, long_pair(lq),
                    dict(levels=(12,), witness=w, decodes=dec, twin="optnum/long_pair/sum%d" % (8191 - total))))
    return out


def sufficient_first(level, ln, pre):
    """X rnd(pre) X[100 : 100 + ln] rnd(60): a copy of exactly ln bytes.  The literal windows before it are 3 long, so
    (len(X) + pre) % 3 says whether the copy is a window's first match (0) or found at cur = 1 or 2"""
    s = SUFFICIENT[level]
    x = rnd(s + 300, 9 + level)
    return x + rnd(pre, 10 + level) + x[100:100 + ln] + rnd(60, 11 + level)


def sufficient_chained(level, ln):
    """a chain of two pieces whose bridge match is ln bytes long where the parser looks for it: at cur = 18, the first
    position of the piece's match whose successor is dearer (records of one price are passed over, :1190).  The forward
    walk of the exit then has sequences to emit"""
    s = SUFFICIENT[level]
    one, two = chain_parts(2, 20 + level, last=s - 10, bridge=ln - 32)
    return one + b"\0\0\0" + two + rnd(40, 21 + level)


def _sufficient():
    out = []
    for level, s in SUFFICIENT.items():
        for pre in (50, 51, 52):
            at = "first" if (s + 300 + pre) % 3 == 0 else "cur"
            for ln in (s, s + 1):
                if ln <= s:
                    w = dict(first_sufficient=0, exit_sufficient=0)
                    if at == "first" or level < 12:
                        w.update(exit_optnum=0, max_window=ln + (s + 300 + pre) % 3 if at == "cur" else ln)
                    else:                             # level 12, cur > 0: 4095 + cur >= OPT_NUM comes first
                        w.update(exit_optnum=1, min_optnum_sum=4095 + (s + 300 + pre) % 3)
                else:
                    w = dict(first_sufficient=1 if at == "first" else 0, exit_sufficient=0 if at == "first" else 1,
                             exit_optnum=0, max_window=3)
                out.append(("sufficient", "sufficient/l%d/%s/pre%d/len%d" % (level, at, pre, ln),
                            sufficient_first(level, ln, pre),
                            dict(levels=(level,), witness=w, decodes=True,
                                 twin="sufficient/l%d/%s/pre%d/len%d" % (level, at, pre, 2 * s + 1 - ln))))
    for level in LEVELS:
        s = SUFFICIENT[level]
        for ln in (s, s + 1):
            w = dict(first_sufficient=0, exit_optnum=0, exit_sufficient=int(ln > s))
            if ln <= s and level < 12:
                w.update(max_window=s + 40)
            elif ln <= s:                             # level 12: 4095 + 18 >= OPT_NUM, the other exit
                w.update(exit_optnum=1, min_optnum_sum=s + 18)
            out.append(("sufficient", "sufficient/l%d/chained/len%d" % (level, ln), sufficient_chained(level, ln),
                        dict(levels=(level,), witness=w, decodes=ln <= s and level < 12,
                             twin="sufficient/l%d/chained/len%d" % (level, 2 * s + 1 - ln))))
    return out


def choice(ll, m, tries):
    """A copy of m bytes found after ll literals, alone in its window: the parser prices it at ll literals + m bytes,
    then at ll + 1 literals + m - 1 bytes, ... (`tries` positions), and a later candidate replaces an earlier one if
    its price is NOT HIGHER (:1293).  -> k, the literals it adds"""
    best, k = seq_price(ll, m), 0
    for j in range(1, tries):
        p = seq_price(ll + j, m - j)
        if p <= best:
            best, k = p, j
    return k


def price_llen_block(ll, m):
    """Y 000 rnd(ll - 3) Y[40 : 40 + m] rnd(40); the literal run begins behind a match (the second 000 is one byte short
    of one: it begins with the tail of a 24-byte copy)"""
    y = rnd(700, 31)
    head = y + b"\0\0" + y[600:624]
    b = head + b"\0\0\0" + rnd(ll - 3, 32 + ll) + y[40:40 + m] + rnd(40, 33)
    p = len(head) + ll
    return b, (p, p + m)


def price_mlen_block(m):
    """a chain of two pieces, the first 30 bytes long, the second m: the copy of m bytes is found at cur = 30 of a
    window, where opt[30] is a match record and opt[31], opt[32] the literals behind it"""
    r = rnd(900, 41)
    one = r + b"\0\0" + r[20:40] + r[300:308]
    b = one + b"\0\0\0" + r[10:40] + r[300:300 + m] + rnd(40, 42)
    p = len(one) + 3 + 30
    return b, (p, p + m)


def price_tie_block(b):
    """W = rnd(b + 2) behind six literals; sources W[0 : 10] (A, the first match) and W[2 : ] (B, b bytes, found at
    cur = 2).  At cur = 10, the end of A, the search finds W[10 : ] (C).  A + C costs two sequences, two literals + B
    one sequence and two bytes: B is cheaper -- unless b >= 19, where its length costs a byte more, the prices tie
    and C, found later, wins (:1293)"""
    w = rnd(b + 2, 51)
    head = rnd(300, 52) + b"\0\0" + w[:10] + b"\0\0" + w[2:] + b"\0\0"
    head += head[100:124] + rnd(6, 53)
    blk = head + w + rnd(40, 54)
    return blk, (len(head), len(head) + len(w))


def _price():
    out = []
    for ll in PRICE_LLEN:
        for m in (18, 19):
            b, probe = price_llen_block(ll, m)
            k = choice(ll, m, 3 - ll % 3)
            out.append(("price", "price/llen%d/m%d" % (ll, m), b,
                        dict(levels=LEVELS, witness=dict(max_llen=(ll - ll % 3, 9999)), decodes=True, probe=probe,
                             parse=[(k, m - k)], twin="price/llen%d/m%d" % (ll, 37 - m))))
    for m in PRICE_MLEN + (275,):
        b, probe = price_mlen_block(m)
        k = choice(0, m, 3)
        twin = {18: 19, 19: 18, 20: 19, 273: 274, 274: 273, 275: 274}[m]
        out.append(("price", "price/mlen%d" % m, b,
                    dict(levels=(12,) if m > 128 else (11, 12) if m > 64 else LEVELS, witness=dict(), decodes=True,
                         probe=probe, parse=[(k, m - k)], twin="price/mlen%d" % twin)))
    for q2 in (18, 19):
        b, probe = price_tie_block(q2)
        parse = [(2, 18)] if q2 == 18 else [(0, 10), (10, 11)]
        out.append(("price", "price/tie/b%d" % q2, b,
                    dict(levels=LEVELS, witness=dict(ties=(1, 9999)), decodes=True, probe=probe, parse=parse,
                         twin="price/tie/b%d" % (37 - q2))))
    return out


FULL = 65536
FAR_LLEN = 60003


def ends_full_block():
    c = chain(21, seed=61)
    return rnd(FULL - len(c), 62) + c


def ends_far_block():
    """part one, 60 003 literals, part two: the window's records carry a 17-bit literal length and 18-bit prices, the
    pieces lie 62 000 .. 65 000 bytes behind their sources"""
    one, two = chain_parts(21, 63)
    return one + b"\0\0\0" + rnd(FAR_LLEN - 3, 64) + two + rnd(40, 65)


def _ends():
    out = []
    for d in ENDS_CUT:                                # the block ends d bytes into piece 23 of 24
        w = dict(max_break_cur=1150 + d - 12 + 1, exit_optnum=0, exit_sufficient=0, max_window=1150 + d - 5)
        out.append(("ends", "ends/cut%d" % d, chain(24, seed=1, cut=1150 + d),
                    dict(levels=LEVELS, witness=w, decodes=True)))
    out.append(("ends", "ends/full", ends_full_block(),
                dict(levels=LEVELS, witness=dict(max_window=1050, x_hop=1), decodes=True, big=True)))
    out.append(("ends", "ends/far_llen", ends_far_block(),
                dict(levels=LEVELS, witness=dict(max_window=1050, max_window_llen=FAR_LLEN, max_llen=FAR_LLEN, x_hop=1,
                                                 max_price=(FAR_LLEN + 237, 70000)), decodes=True, big=True)))
    for m in (18, 19, 20):                            # the same tie with prices of 60 000 and more on both sides
        b, probe = tie_chain(m, b"\0\0\0" + rnd(FAR_LLEN - 3, 66))
        k = choice(0, m, 3)
        out.append(("ends", "ends/far_llen/tie/m%d" % m, b,
                    dict(levels=LEVELS, witness=dict(max_window=990 + m, max_window_llen=FAR_LLEN, x_hop=1,
                                                     max_price=(FAR_LLEN + 237, 70000)),
                         decodes=True, big=True, probe=probe, parse=[(k, m - k)],
                         twin="ends/far_llen/tie/m%d" % (19 if m != 19 else 18))))
    return out


WIDE = 70001


def _wide():
    """two blocks of 70 001 bytes, for k_hc_opt_parse<uint64_t> by their size: a window of 1500 records that begins
    past offset 65 536, and a chain of 100 pieces whose OPT_NUM exit lies past it"""
    c = chain(30, seed=71)
    a = rnd(WIDE - len(c), 72) + c
    c = chain(100, seed=73)
    b = rnd(WIDE - len(c), 74) + c
    assert WIDE - 1500 - 40 > 65536
    return [("wide", "wide/window1500", a, dict(levels=LEVELS, witness=dict(max_window=1500, exit_optnum=0, x_hop=1),
                                                decodes=True)),
            ("wide", "wide/optnum", b, dict(levels=LEVELS, witness=dict(exit_optnum=1, min_optnum_sum=4100,
                                                                        max_window=4075), decodes=False))]


_cases = None


def cases():
    """-> [(family, name, bytes, meta)]; built once"""
    global _cases
    if _cases is None:
        _cases = _window() + _optnum() + _sufficient() + _price() + _ends() + _wide()
        assert len({n for _, n, _, _ in _cases}) == len(_cases)
    return _cases


def longest_run(b):
    """the longest run of one byte value"""
    a = np.frombuffer(b, dtype=np.uint8)
    edges = np.flatnonzero(np.diff(a) != 0)
    return int(np.diff(np.concatenate(([-1], edges, [len(a) - 1]))).max())


def wave(cs=None):
    """the cases of at most 65 536 bytes: k_hc_opt_parse_wave under their natural bound"""
    return [c for c in (cases() if cs is None else cs) if len(c[2]) <= 65536]


def for_level(cs, level):
    return [c for c in cs if level in c[3]["levels"]]
