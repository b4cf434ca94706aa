"""Blocks built on the decision edges of level 2 (lz4mid, k_hc_mid_serial; tests/test_mid_corpus_cpu.py,
tests/test_gpu_mid_corpus.py).  The same shape as tests/edgegen.py: a pure generator, no GPU, no oracle, fixed seeds.

`cases()` gives [(family, name, bytes, meta)].  Every case puts ONE comparison of the level-2 walk on its edge and names
a twin on the other side.  `meta` carries "probe" (lo, hi), the region where the decision shows; "expect", the sequences
[(position, offset, length)] that start inside the probe, WORKED OUT FROM THE CONSTRUCTION (the comments of each builder
say how); "accept", the side of the edge; "twin"; and the builder's parameters.

What the walk does, as far as the constructions use it (n = block length, mflimit = n - 12, matchlimit =
n - 5, ilimit = n - 8):
  * positions are probed from the anchor with step 1 + ((ip - anchor) >> 9); a probe at ip reads h8[hash of 7 bytes], stores
    ip there, takes a match of >= 4 bytes from a source in 1 .. ip - 1 at most 65535 back; else the same with h4[hash of 4
    bytes]; an h4 match at ip < mflimit looks h8 up for ip + 1 and moves there if that match is LONGER;
  * a taken match at ip (index ix: ip before a move) stores ix + 1 in h8 and h4 and ix + 2 in h8 under the hashes at
    ip + 1 / ip + 2, and, ending at e, stores e - 5 and e - 3 in h8, e - 2 in both, e - 1 in h4.  Nothing else inside a match
    is entered: e - 3 is an h8-only position, e - 1 an h4-only one, e - 4 in neither table.

Families: pf_patch (the next probe falls into the slot the current one writes), next_longer (the ip + 1 lookup),
moved_index (the entries one byte early behind a moved match), fill_end (which entries a match leaves), reach (65535 /
65536 for h8, h4 and the lookup, position 0 as a source), end_clamp (a copy at mflimit - 1, mflimit, mflimit + 1), step (a
copy on a probed / skipped position behind 511 .. 1025 literals).

Collisions (two different strings in one slot) are found by a seeded search here, and the equality is asserted.  `rnd()`
has no zero byte, so runs of zeros never continue into it.
"""
from edgegen import MAX_DIST, in_probe, rnd, walk      # noqa: F401  (walk / in_probe: re-exported for the tests)

M32, M64 = (1 << 32) - 1, (1 << 64) - 1
FAR_D = (65534, 65535, 65536, 65537)
STEP_K = (511, 512, 513, 1023, 1024, 1025)
VARIANTS = 3                                          # every small construction is built from three sets of seeds
FAMILIES = ("pf_patch", "next_longer", "moved_index", "fill_end", "reach", "end_clamp", "step")


def hash_mid4(b, i):                                  # zlz4_compress_hc_serial.hip:36
    return ((int.from_bytes(b[i:i + 4], "little") * 2654435761) & M32) >> 18


def hash_mid8(b, i):                                  # :37-39: the low 7 bytes of the 8-byte read
    return ((((int.from_bytes(b[i:i + 8], "little") << 8) & M64) * 58295818150454627) & M64) >> 50


def probed(k):
    """the first probed offset >= k of a literal run that starts at offset 0 (the anchor)"""
    j = 0
    while j < k:
        j += 1 + (j >> 9)
    return j


class _Seeds:
    def __init__(self, var):
        self.var = var

    def __call__(self, n, s):
        return rnd(n, 7000 + 1000 * self.var + s)


def _case(out, fam, name, b, probe, expect, accept, twin, **kw):
    assert 0 <= probe[0] < probe[1] <= len(b), name
    out.append((fam, name, bytes(b), dict(probe=probe, expect=expect, accept=accept, twin=twin, **kw)))


def _quiet(b, lo, hi, at8=(), at4=()):
    """no position of [lo, hi) holds OTHER bytes in a table slot of the positions whose entries a construction relies on"""
    s8, s4 = {}, {}
    for i in at8:
        s8.setdefault(hash_mid8(b, i), set()).add(b[i:i + 7])
    for i in at4:
        s4.setdefault(hash_mid4(b, i), set()).add(b[i:i + 4])
    return not any(b[i:i + 7] not in s8.get(hash_mid8(b, i), (b[i:i + 7],)) or b[i:i + 4] not in s4.get(hash_mid4(b, i), (b[i:i + 4],))
                   for i in range(lo, hi))


def _other(*xs):
    """a byte that is none of xs and not zero"""
    return bytes([min(set(range(1, 256)) - set(xs))])


def _gadget(r, k):
    """x H(8) R(3) H: a match of 8 bytes through h8 that ends at e -> (bytes, e).  What follows must differ from R(3)[0]."""
    h = r(8, 10 + k)
    b = b"\x07" + h + r(3, 11 + k) + h
    return b, len(b)


# ------------------------------------------------------------------------------------------------ end_clamp
def _end_clamp(r, v):
    out, fam = [], "end_clamp"
    if v == 0:
        # 13 bytes: mflimit = 1, positions 0 and 1 are probed and neither has a source.  14 bytes: the run is found at 2
        # from 1, 11 bytes are equal, matchlimit - ip = 7 count.  20 bytes, mflimit = 8: a run of period 7 / 6 / 8 repeats
        # at 8 / 7 / 9 = mflimit / mflimit - 1 / mflimit + 1.
        g = r(8, 1)
        _case(out, fam, "end_clamp/n13/run", b"\x07" + b"a" * 12, (0, 13), [], False, "end_clamp/n14/run", n=13)
        _case(out, fam, "end_clamp/n14/run", b"\x07" + b"a" * 13, (0, 14), [(2, 1, 7)], True, "end_clamp/n13/run", n=14)
        _case(out, fam, "end_clamp/n20/at", b"\x07" + (g[:7] * 3)[:19], (0, 20), [(8, 7, 7)], True, "end_clamp/n20/after", n=20)
        _case(out, fam, "end_clamp/n20/before", b"\x07" + (g[:6] * 4)[:19], (0, 20), [(7, 6, 8)], True, "end_clamp/n20/at", n=20)
        _case(out, fam, "end_clamp/n20/after", b"\x07" + (g[:8] * 3)[:19], (0, 20), [], False, "end_clamp/n20/at", n=20)
    for via in ("h8", "h4"):
        for arrive in ("pf", "match"):
            for ext in ("eight", "end"):
                for delta in (-1, 0, 1):
                    # the copy starts at p = mflimit + delta, so 12 - delta bytes follow p; "eight": 8 equal bytes and a
                    # foreign rest, "end": equal to the block's end.  At mflimit - 1 eight bytes lie before matchlimit,
                    # at mflimit seven, and mflimit + 1 is not probed.
                    k = r(8, 20)                                     # arrive == "match": a copy of K ends at p
                    if via == "h8":                                  # G at 1, every position of it probed
                        g = r(13, 21)
                        b = b"\x07" + g + (k if arrive == "match" else b"") + r(9, 22)
                        src = 1
                    else:                                            # G starts on the LAST byte of a match: h4 only
                        head, e = _gadget(r, 0)
                        g = head[-1:] + r(12, 21)
                        b = head + g[1:] + (k if arrive == "match" else b"") + r(9, 22)
                        src = e - 1
                    if arrive == "match":
                        b += k
                    p = len(b)
                    assert via == "h8" or b[e] != b[9]                # the gadget's match ends after 8 bytes
                    assert arrive == "pf" or g[0] != b[p - 17]         # ... and so does the copy of K
                    rest = 12 - delta
                    b += g[:8] + r(rest - 8, 23) if ext == "eight" else g[:rest]
                    assert len(b) - 12 + delta == p and b[src:src + 8] == b[p:p + 8]
                    assert ext == "end" or b[p + 8] != g[8]
                    want = [(p, p - src, 7 - delta)] if delta <= 0 else []
                    name = "end_clamp/%s/%s/%s/v%d/m%+d" % (via, arrive, ext, v, delta)
                    twin = "end_clamp/%s/%s/%s/v%d/m%+d" % (via, arrive, ext, v, 0 if delta else 1)
                    _case(out, fam, name, b, (p, len(b)), want, delta <= 0, twin, via=via, arrive=arrive, delta=delta, src=src)
    return out


# ------------------------------------------------------------------------------------------------ step
def _step(r, v):
    out, fam = [], "step"
    for anchor in ("start", "match"):
        for k in STEP_K:
            # S (16 bytes) at 1, every position of it probed; its copy k bytes behind the anchor (the block's start, or
            # the end of a match).  The first probed offset j >= k finds S[j - k:] through h8.
            for attempt in range(40):
                s = r(16, 30)
                if anchor == "start":
                    b = b"\x07" + s + r(k - 17, 31 + 50 * attempt)
                    a = 0
                else:
                    hh = r(8, 32)
                    b = b"\x07" + s + hh + r(4, 33) + hh
                    a = len(b)
                    b += r(k, 31 + 50 * attempt)
                    assert b[a] != b[a - 12]
                p = a + k
                b += s + r(20, 34)
                if _quiet(b, 17, p, at8=(1, 2, 3)):
                    break
            else:
                raise AssertionError("no quiet filler")
            j = probed(k)
            want = [(a + j, p - 1, 16 - (j - k))]
            other = {511: 513, 512: 513, 513: 512, 1023: 1024, 1024: 1025, 1025: 1024}[k]
            _case(out, fam, "step/%s/v%d/k%d" % (anchor, v, k), b, (p, p + 16), want, j == k,
                  "step/%s/v%d/k%d" % (anchor, v, other), k=k, anchor=a)
    return out


# ------------------------------------------------------------------------------------------------ reach
def _reach():
    out, fam = [], "reach"
    r = _Seeds(9)
    for d in FAR_D:
        ok = d <= MAX_DIST
        tw = d + 2 if ok else d - 2
        # every filler is a run of zeros: position z0 + 1 matches z0 and one match swallows the run (four table writes)
        g = r(12, 40)
        z = d - 17
        b = b"\x07" + g + r(3, 41) + bytes(z) + r(2, 42)
        p = len(b)
        b += g + r(16, 43)
        assert p - 1 == d
        _case(out, fam, "reach/h8/d%d" % d, b, (p, p + 12), [(p, d, 12)] if ok else [], ok, "reach/h8/d%d" % tw, d=d)
        for ln in (4, 5, 6, 7):                      # G[:ln] and a foreign byte: up to 6 bytes h8 (7 bytes hashed) finds
            g = r(7, 44)                             # nothing and h4 gives the copy; 7 equal bytes come through h8
            z = d - 12
            b = b"\x07" + g + r(3, 45) + bytes(z) + r(2, 46)
            p = len(b)
            b += g[:ln] + r(20, 47)
            assert p - 1 == d and b[p + ln] != (g + b[8:9])[ln]
            _case(out, fam, "reach/h4/l%d/d%d" % (ln, d), b, (p, p + ln), [(p, d, ln)] if ok else [], ok,
                  "reach/h4/l%d/d%d" % (ln, tw), d=d, ln=ln)
        # the lookup: c F0 F1 F2 y at q gives 4 bytes at p through h4; F (10 bytes) at 1 is d bytes behind p + 1
        f, c = r(10, 48), b"\x09"
        z = d - 24
        b = b"\x07" + f + r(3, 49) + bytes(z) + r(2, 50)
        q = len(b)
        b += c + f[:3] + bytes([f[3] ^ 0x55 or 1]) + r(3, 51)
        p = len(b)
        b += c + f + r(16, 52)
        assert p == d and b[q + 4] != f[3]
        _case(out, fam, "reach/m2/d%d" % d, b, (p, p + 11), [(p + 1, d, 10)] if ok else [(p, p - q, 4)], ok,
              "reach/m2/d%d" % tw, d=d)
    # position 0 is no source (pos > 0): the same block with and without a byte in front
    for v in range(VARIANTS):
        r = _Seeds(v)
        for pad in (0, 1):
            x = b"\x07" * pad
            tw = 1 - pad
            g = r(12, 53)
            b = x + g + r(20, 54)
            p = len(b)
            b += g + r(16, 55)
            _case(out, fam, "reach/pos%d/h8/v%d" % (pad, v), b, (p, p + 12), [(p, p - pad, 12)] if pad else [(p + 1, p, 11)],
                  bool(pad), "reach/pos%d/h8/v%d" % (tw, v))
            for ln in (4, 6):                        # ln = 4: G[1:4] is too short for a match from position 1
                g = r(6, 56)
                b = x + g + r(20, 57)
                p = len(b)
                b += g[:ln] + r(16, 58)
                want = [(p, p - pad, ln)] if pad else ([(p + 1, p, ln - 1)] if ln > 4 else [])
                _case(out, fam, "reach/pos%d/h4/l%d/v%d" % (pad, ln, v), b, (p, p + ln), want, bool(pad),
                      "reach/pos%d/h4/l%d/v%d" % (tw, ln, v), ln=ln)
            # the lookup's source at 0: the 4-byte match stays, and F[3:] is found from position 3 behind it
            f, c = r(10, 59), b"\x09"
            b = x + f + r(8, 60)
            q = len(b)
            b += c + f[:3] + bytes([f[3] ^ 0x55 or 1]) + r(3, 61)
            p = len(b)
            b += c + f + r(16, 62)
            want = [(p + 1, p + 1 - pad, 10)] if pad else [(p, p - q, 4), (p + 4, p + 1, 7)]
            _case(out, fam, "reach/pos%d/m2/v%d" % (pad, v), b, (p, p + 11), want, bool(pad), "reach/pos%d/m2/v%d" % (tw, v))
    return out


# ------------------------------------------------------------------------------------------------ pf_patch
STEP_AT = {1: 30, 2: 600, 3: 1030}                   # a probed offset behind the anchor at which the step is 1 / 2 / 3


def _collide(r, kind, step, fixed):
    """-> (v, rest): hash(v + W) == hash(W) over 7 (h8) or 4 (h4) bytes for W = fixed + rest, v of `step` bytes, and the
    other table's slots differ"""
    ha, hb = (hash_mid8, hash_mid4) if kind == "h8" else (hash_mid4, hash_mid8)
    k = 10 - len(fixed)
    pool, heads = r(k * 4000, 100 + step), r(2 * 4000, 101 + step)      # candidates, drawn once
    for seed in range(4000):
        rest = pool[k * seed:k * seed + k]
        w = fixed + rest
        t, tb = ha(w, 0), hb(w, 0)
        head = heads[2 * seed:2 * seed + step - 1]
        for x in range(1, 256):
            vv = head + bytes([x])
            if ha(vv + w, 0) == t and hb(vv + w, 0) != tb and vv[-1] != w[0]:
                return vv, rest
    raise AssertionError("no collision found")


def _pf_patch(r, v):
    out, fam = [], "pf_patch"
    for step in (1, 2, 3):
        # a fresh run of period `step`, n bytes, at a probed position p: p finds nothing, the next probe p + step finds p
        # when the hashes are equal -- 4 bytes need n >= step + 4, 7 bytes n >= step + 7.  With n = step + 3 nothing.
        pat = bytes(range(step))                      # zeros, 00 01, 00 01 02
        for n in (step + 3, step + 4, step + 5, step + 6, step + 7, 20):
            for attempt in range(40):
                b = b"\x07" + r(STEP_AT[step] - 1, 70 + 50 * attempt)
                p = len(b)
                b += (pat * 30)[:n] + r(20, 71)
                if b[p - 1] != pat[-1] and b[p + n] != (pat * 30)[n] and all(x for x in b[p - 8:p]):
                    break
            want = [(p + step, step, n - step)] if n >= step + 4 else []
            slots = "h4" if n < step + 7 else "both"
            _case(out, fam, "pf_patch/same/s%d/v%d/n%d" % (step, v, n), b, (p, p + n), want, n >= step + 4,
                  "pf_patch/same/s%d/v%d/n%d" % (step, v, step + 3 if n >= step + 4 else step + 4), step=step, n=n, slots=slots)
        # different bytes in one slot: W (10 bytes) begins on an h8-only position (e - 3) or an h4-only one (e - 1) of a
        # match that ends at e; v + W stands at p, STEP_AT bytes behind the anchor e.  The probe at p takes W's slot; the
        # probe at p + step reads p, fails, and W[step:] is found one probe later from w + step.  The twin's v does not
        # collide and W is found at p + step.
        for kind in ("h8", "h4"):
            head, e = _gadget(r, 0)
            back = 3 if kind == "h8" else 1
            vv, rest = _collide(r, kind, step, head[-back:])
            w = e - back
            assert rest[0] != head[9]
            for side in ("hit", "miss"):
                v2 = vv if side == "hit" else vv[:-1] + bytes([vv[-1] ^ 0x2A or 1])
                for attempt in range(40):
                    b = head + rest + r(STEP_AT[step] - len(rest), 72 + 50 * attempt)
                    p = len(b)
                    b += v2 + head[-back:] + rest + r(20, 73)
                    if _quiet(b, e, p + step, at8=(w, w + 1, w + 2, w + 3, p), at4=(w, w + 1, w + 2, w + 3, p)):
                        break
                else:
                    raise AssertionError("no quiet filler")
                ha = hash_mid8 if kind == "h8" else hash_mid4
                hb = hash_mid4 if kind == "h8" else hash_mid8
                assert (ha(b, p) == ha(b, p + step)) == (side == "hit") and hb(b, p) != hb(b, p + step)
                assert b[w:w + 10] == b[p + step:p + step + 10] and b[w + 10] != b[p + step + 10] and p - e == STEP_AT[step]
                d = p + step - w
                want = [(p + 2 * step, d, 10 - step)] if side == "hit" else [(p + step, d, 10)]
                _case(out, fam, "pf_patch/diff/%s/s%d/v%d/%s" % (kind, step, v, side), b, (p, p + step + 10), want,
                      side == "miss", "pf_patch/diff/%s/s%d/v%d/%s" % (kind, step, v, "miss" if side == "hit" else "hit"),
                      step=step, slots=kind, w=w)
    # a taken match between two probes: what the probe before it fetched is not for the position behind it.  A (8 bytes:
    # taken through h8; 5 bytes: through h4) and C are copied back to back, or with one byte between them.
    for la in (8, 5):
        a, c = r(la, 74), r(8, 75)
        for gap in (0, 1):
            b = b"\x07" + a + r(3, 76) + c + r(10, 77)
            p = len(b)
            b += a + r(gap, 78) + c + r(20, 79)
            assert b[p + la] != b[1 + la] and b[p + la + gap + 8] != b[la + 12]
            p2 = p + la + gap
            _case(out, fam, "pf_patch/after_match/a%d/v%d/g%d" % (la, v, gap), b, (p, p2 + 8), [(p, p - 1, la), (p2, p2 - la - 4, 8)],
                  gap == 0, "pf_patch/after_match/a%d/v%d/g%d" % (la, v, 1 - gap), gap=gap, la=la)
    return out


# ------------------------------------------------------------------------------------------------ next_longer, moved_index
def _longer_block(r, ln):
    """x F(ln) R(3) | H R(3) H | F[:6] y R(10) | c F Z(16), c = the last byte of H.
    The near source c F[:6] y starts on the last byte of the match of H (e - 1: h4 only), so c F ... at p is found through
    h4 with 7 bytes; the lookup at p + 1 finds F at 1 with ln bytes.  (Behind the match of H, F[:6] at e matches F at 1.)
    -> (block, p, e)"""
    f = r(ln, 80)
    h = r(8, 81)
    for attempt in range(40):
        b = b"\x07" + f + r(3, 82) + h + r(3, 83) + h
        e = len(b)
        b += f[:6] + bytes([f[6] ^ 0x55 or 1]) + r(10, 84 + 50 * attempt)
        p = len(b)
        z = r(16, 85 + 50 * attempt)
        b += h[-1:] + f + z
        watch = tuple(range(1, 1 + ln)) + tuple(range(e - 1, e + 7)) + tuple(range(p, p + 12))
        if _quiet(b + bytes(8), 0, len(b), at8=watch, at4=watch):
            break
    else:
        raise AssertionError("no quiet filler")
    assert z[0] != b[1 + ln] and b[e + 6] != f[6] and f[0] != b[e - 11]
    return b, p, e


def _next_longer(r, v):
    out, fam = [], "next_longer"
    for ln in (7, 8, 9, 12):                         # ml2 == match_len stays; one more moves
        b, p, e = _longer_block(r, ln)
        b += r(20, 86)
        want = [(p, p - e + 1, 7)] if ln == 7 else [(p + 1, p, ln)]
        _case(out, fam, "next_longer/ml2/v%d/l%d" % (v, ln), b, (p, p + 1 + ln), want, ln > 7,
              "next_longer/ml2/v%d/l%d" % (v, 8 if ln == 7 else 7), ln=ln)
    for at in (0, -1):                               # the match of 4 bytes at mflimit (no lookup) / mflimit - 1
        f, c = r(7, 87), b"\x09"
        b = b"\x07" + f + r(3, 88)
        q = len(b)
        b += c + f[:3] + bytes([f[3] ^ 0x55 or 1]) + r(6, 89)
        p = len(b)
        b += c + f + r(4 - at, 90)
        assert len(b) - 12 + at == p
        want = [(p, p - q, 4)] if at == 0 else [(p + 1, p, 7)]
        _case(out, fam, "next_longer/mflimit/v%d/m%+d" % (v, at), b, (p, len(b)), want, at < 0,
              "next_longer/mflimit/v%d/m%+d" % (v, -1 - at), at=at)
    # h8[hash(ip + 1)] is the slot this probe has just written: 0000 y at q, six zeros u v at p with
    # hash8(000000u) == hash8(00000uv) (searched).  p matches q with 4 bytes, the lookup reads p itself: distance 1,
    # 5 bytes, longer.  The twin's v does not collide.
    base = b"\x07" + r(6, 91) + b"\x11"
    q = len(base)
    base += bytes(4) + r(9, 92) + b"\x22"               # (the bytes before the two runs differ)
    p = len(base)
    uv = None
    for u in range(1 + v, 256):                       # (another pair per variant)
        for w in range(1, 256):
            t = bytes(6) + bytes([u, w]) + b"\x01"
            if hash_mid8(t, 0) == hash_mid8(t, 1):
                uv = (u, w)
                break
        if uv:
            break
    assert uv, "no collision found"
    for side in ("hit", "miss"):
        w = uv[1] if side == "hit" else (uv[1] ^ 0x2A or 1)
        b = base + bytes(6) + bytes([uv[0], w]) + r(16, 93)
        assert (hash_mid8(b, p) == hash_mid8(b, p + 1)) == (side == "hit")
        want = [(p + 1, 1, 5)] if side == "hit" else [(p, p - q, 4)]
        _case(out, fam, "next_longer/own_slot/v%d/%s" % (v, side), b, (p, p + 8), want, side == "hit",
              "next_longer/own_slot/v%d/%s" % (v, "miss" if side == "hit" else "hit"))
    return out


def _moved_index(r, v):
    """The block of next_longer/ml2 and a later copy C of the text behind p.  ln = 8: the match moves to p + 1 (index p), so
    the text at p + 2 is entered as p + 1 (h8 and h4) and the text at p + 3 as p + 2 (h8): a copy of either is compared
    with a candidate one byte early and fails.  ln = 7: no move, exact entries."""
    out, fam = [], "moved_index"
    for kind, lo, n in (("h8_0", 1, 10), ("h8_1", 2, 10), ("h4_1", 2, 5), ("h8_2", 3, 7)):
        for ln in (8, 7) if lo > 1 else (8,):
            b, p, e = _longer_block(r, ln)
            b += _other(b[p + lo - 1])
            rr = len(b)
            b += b[p + lo:p + lo + n] + r(20, 94)
            assert b[rr + n] != b[p + lo + n]
            if kind == "h8_0":
                # the moved match's own start is entered exactly (h8[hash(ip + 1)] = index + 1): F and two bytes more from
                # p + 1, not F alone from 1.  Its other side is h8_1, the entry one byte early.
                _case(out, fam, "moved_index/h8_0/v%d/l8" % v, b, (rr, rr + n), [(rr, rr - p - 1, 10)], False,
                      "moved_index/h8_1/v%d/l8" % v, kind=kind, ln=ln)
                continue
            if kind == "h8_1":
                # moved: r and r + 1 fail on the early candidates (h8: p + 1, p + 2; h4: p + 1); h4 at r + 1 finds F[2:] at 3
                # with 6 bytes, and the lookup at r + 2 finds p + 4 (e - 5 of the moved match, exact) with 8.
                want = [(rr + 2, rr - p - 2, 8)] if ln == 8 else [(rr, rr - p - 2, 10)]
            elif kind == "h4_1":
                # moved: h4 at r gives p + 1 and fails; r + 1 finds F[2:6] at 3.  Not moved: F[1:6] from e + 1, the entry
                # the match of F[:6] at e left.
                want = [(rr + 1, rr - 2, 4)] if ln == 8 else [(rr, rr - e - 1, 5)]
            else:
                # moved: h8 at r gives p + 2 and fails, h4 finds F[2:8] at 3.  Not moved: p + 3 was never entered, h4 finds
                # F[2:7] at 3.
                want = [(rr, rr - 3, 6)] if ln == 8 else [(rr, rr - 3, 5)]
            _case(out, fam, "moved_index/%s/v%d/l%d" % (kind, v, ln), b, (rr, rr + n), want, ln == 8,
                  "moved_index/%s/v%d/l%d" % (kind, v, 15 - ln), kind=kind, ln=ln)
    return out


# ------------------------------------------------------------------------------------------------ fill_end
def _fill_end(r, v):
    """x T X(3) | T Y(16) | C foreign(4) [C[:4]] R(20): the copy of T at q is one match ending at e = q + len(T); C is
    a piece of the block that only ONE table entry of that match leads to (or none: the twins e4 / b3)."""
    out, fam = [], "fill_end"
    for via, tl in (("h8", 20), ("h4", 6)):
        t = r(tl, 95)
        b0 = b"\x07" + t + r(3, 96)
        q = len(b0)
        b0 += t + r(16, 97)
        e = q + tl
        assert b0[e] != b0[1 + tl]
        rr = len(b0)
        # name -> (start, length, again, expected offset base, expected length); again: C[:4] stands once more behind C
        spec = {
            "e3": (e - 3, 7, False), "e2_h8": (e - 2, 7, True), "e2_h4": (e - 2, 4, False), "e1": (e - 1, 4, False),
            "e1_long": (e - 1, 7, True), "b2_h8": (q + 2, 7, False), "b1_h4": (q + 1, 4, False),
        }
        if via == "h8":
            spec.update({"e5": (e - 5, 7, False), "e4": (e - 4, 7, False), "b1_h8": (q + 1, 7, False), "b3": (q + 3, 7, False)})
        for name, (lo, n, again) in spec.items():
            c = b0[lo:lo + n]
            b = b0 + _other(b0[lo - 1]) + c + r(4, 98)
            rr = len(b0) + 1
            b += _other(b[rr - 1], b0[lo - 1])
            r2 = len(b)
            b += (c[:4] if again else b"") + r(20, 99)
            assert b[rr + n] != b0[lo + n]
            if name == "e4":                         # no entry: h4 finds T[16:20] at 17, 4 bytes
                want = [(rr, rr - 17, 4)]
            elif name == "b3":                       # no entry: T[3:10] from the first T
                want = [(rr, rr - 4, 7)]
            elif name == "e2_h8":                    # taken through h8, so h4 still holds e - 2 for the second copy
                want = [(rr, rr - lo, 7), (r2, r2 - lo, 4)]
            elif name == "e1_long":                  # e - 1 is in h4 only: taken through h4, which then holds r
                want = [(rr, rr - lo, 7), (r2, r2 - rr, 4)]
            else:
                want = [(rr, rr - lo, n)]
            twin = "b3" if name[0] == "b" and name != "b3" else "b1_h8" if name == "b3" else "e5" if name == "e4" else "e4"
            _case(out, fam, "fill_end/%s/v%d/%s" % (via, v, name), b, (rr, r2 + 4), want, name not in ("e4", "b3"),
                  "fill_end/h8/v%d/%s" % (v, twin), via=via, entry=name, e=e, q=q)
    return out


_cases = None


def cases():
    """-> [(family, name, bytes, meta)]; built once.  Twins are neighbours."""
    global _cases
    if _cases is None:
        out = _reach()
        for v in range(VARIANTS):
            r = _Seeds(v)
            out += _pf_patch(r, v) + _next_longer(r, v) + _moved_index(r, v) + _fill_end(r, v) + _end_clamp(r, v) + _step(r, v)
        by = {c[1]: c for c in out}
        assert len(by) == len(out)
        for c in out:
            assert c[3]["twin"] in by and by[c[3]["twin"]][0] == c[0], c[1]
        _cases = sorted(out, key=lambda c: (FAMILIES.index(c[0]), min(c[1], c[3]["twin"]), c[1]))
    return _cases


def small(cs=None):
    return [c for c in (cases() if cs is None else cs) if len(c[2]) <= 4096]


def large(cs=None):
    return [c for c in (cases() if cs is None else cs) if len(c[2]) > 4096]
