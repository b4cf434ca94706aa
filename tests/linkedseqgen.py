"""Crafted lz4f frames at the sequence level for the serial wave decoder (test infrastructure): linked-declared frames
and dictionary frames whose blocks are cut out of one sequence stream, for decode_block_wave (zig-lz4_amd/csrc/
zlz4_device.hpp) behind k_bfl_decode (zig-lz4_amd/csrc/zlz4_frame_linked.hip).

* One seqgen._Builder(rng, T) spans a whole frame: its plaintext is the frame's plaintext over T ++ output, an expectation
  that comes from neither the CPU model nor the kernel.  The stream is cut into blocks at sequence boundaries only; a
  literal-only sequence stands only directly in front of a cut.
* `corpus()` -> [Item], seeded and deterministic.  Families: `overlap` (offset < length, placed four ways), `runs` (copy
  lengths around the 16-byte pieces and the 1 KiB chunks of copy_bytes), `hist` (accepted / refused pairs at the history
  bound), `slide` (more than 64 KiB of output), `ends` (block ends, stored blocks), `independent` (a few frames that
  declare independent blocks, for the mixed batch), then the variants: checksums, one-block twins of the dictionary
  frames, short capacities (`caps`) and `damaged` copies.
  About 1350 frames and 3.7 MB of plaintext, most frames a few KiB: an (offset, length) pair that starts in T needs a
  frame of its own, and each such frame brings its twin and two damaged copies.
* `census(items)` counts, from the sequence lists alone, how many matches fall into each class of the decoder's copy.
"""
import random

import linkedgen
from dictgen import seq
from seqgen import _Builder

lf = linkedgen.lf
HISTORY = 65536
FAILED, STORED_TOO_LARGE, BLOCK_CHECKSUM = -116, -111, -107
OVERLAP_OFFSETS = (1, 2, 3, 4, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 1023, 1024, 1025, 1039, 2047, 2048)
RUN_LENGTHS = (0, 1, 14, 15, 16, 269, 270, 1023, 1024, 1025, 1039, 1040, 2063, 5000)
HIST_PAIRS = ((0, 300), (500, 0), (500, 300))         # (D, pos)


def overlap_lengths(o):
    """the match lengths of the `overlap` family at offset o: only ml > o (and a match is four bytes at least)"""
    return sorted({ml for ml in (o + 1, 2 * o, 2 * o + 1, 1024, 1025, 2000, 4111) if ml > o and ml >= 4})


class Item:
    """One decode of `frame` into `cap` bytes; dict_bytes None = a plain linked call (ZLZ4F_DECODE_LINKED), else the
    dictionary call.  `plain`: the generator's plaintext of the whole frame, None where only the model can judge (a
    damaged frame, or one with a refused match).  `liblz4_ok`: the frame is valid, decoded at its exact size, and every
    block decodes to at most 65536 bytes and ends in five or more literals, so liblz4 must give the same bytes.  `status`: the result stated by the generator where it pins one (n,
    -116, -111, -107), else None.  `seqs`: the match records of a base frame (census), None on a variant.  `twin_of`:
    the name of the multi-block frame whose block 0 this frame is."""
    __slots__ = ("name", "family", "frame", "dict_bytes", "cap", "plain", "liblz4_ok", "status", "seqs", "twin_of")

    def __init__(self, name, family, frame, dict_bytes, cap, plain, liblz4_ok=False, status=None, seqs=None, twin_of=None):
        self.name, self.family, self.frame, self.dict_bytes, self.cap = name, family, frame, dict_bytes, cap
        self.plain, self.liblz4_ok, self.status, self.seqs, self.twin_of = plain, liblz4_ok, status, seqs, twin_of

    def expected(self):
        """-> bytes, or None when only the model can tell (damaged, refused or short of capacity)"""
        return self.plain if self.plain is not None and self.cap >= len(self.plain) else None


def assemble(blocks, bsid=4, block_checksum=False, content=None, block_mode=0):
    f = linkedgen.build_frame(blocks, block_checksum, content, block_mode=block_mode)
    if bsid != 4:                                     # build_frame writes block size id 4: the header is 7 bytes
        f = lf.encode_header(bsid, block_mode, 0 if content is None else 1, 1 if block_checksum else 0) + f[7:]
    return f


_FRAME = object()


class _Frame:
    """The blocks of one frame over one _Builder; `dict_bytes` None = a plain linked frame."""

    def __init__(self, rng, name, family, dict_bytes=None, bsid=4, block_mode=0):
        self.name, self.family, self.dict, self.bsid, self.block_mode = name, family, dict_bytes, bsid, block_mode
        self.D = min(len(dict_bytes or b""), HISTORY)
        self.b = _Builder(rng, (dict_bytes or b"")[-HISTORY:])
        self.blocks, self.cuts, self.seqs = [], [], []
        self.s0 = self.pos = 0
        self.lit_only = None                          # length of a pending literal-only sequence
        self.ok = True
        self.bad_block = None                         # the first block with a refused match
        self.stored_at = []                           # (output position, length) of the stored blocks

    @property
    def op(self):
        return self.b.op - self.pos

    def add(self, lit, off=None, ml=None, probe=False):
        assert self.lit_only is None, "a literal-only sequence stands only directly in front of a cut"
        n = lit if isinstance(lit, int) else len(lit)
        if off is None:
            self.lit_only = n
        else:
            self.seqs.append(dict(k=len(self.blocks), pos=self.pos, op=self.op + n, off=off, ml=ml, lit=n, D=self.D,
                                  probe=probe))
        self.b.add(lit, off, ml)
        if not self.b.valid and self.bad_block is None:
            self.bad_block = len(self.blocks)

    def cut(self):
        body = bytes(self.b.s[self.s0:])
        assert body
        if self.op > HISTORY or self.lit_only is None or self.lit_only < 5:
            self.ok = False
        self.blocks.append((body, False))
        self._end()

    def stored(self, n):
        assert self.s0 == len(self.b.s) and n > 0
        data = self.b.lits(n)
        self.stored_at.append((self.pos, n))
        self.b.out += data
        self.blocks.append((data, True))
        self._end()

    def _end(self):
        self.s0, self.pos, self.lit_only = len(self.b.s), self.b.op, None
        self.cuts.append(self.pos)

    def close(self, lo=5, hi=9):
        """the block's last literals (five or more keep liblz4 content), then the cut"""
        self.add(self.b.rng.randint(lo, hi))
        self.cut()

    @property
    def plain(self):
        return bytes(self.b.out) if self.b.valid else None

    def item(self, name=None, blocks=None, plain=_FRAME, cap=None, status=None, seqs=True, family=None, twin_of=None,
             block_checksum=False, content=False, ok=None):
        plain = self.plain if plain is _FRAME else plain
        blocks = self.blocks if blocks is None else blocks
        # (a frame with a refused match never reaches its content checksum: any value will do)
        frame = assemble(blocks, self.bsid, block_checksum,
                         (plain if plain is not None else bytes(self.b.out)) if content else None, self.block_mode)
        if cap is None:
            cap = len(plain) if plain is not None else self.b.op + 64
        ok = (self.ok if ok is None else ok) and plain is not None and cap == len(plain)
        return Item(name or self.name, family or self.family, frame, self.dict, cap, plain, ok, status,
                    self.seqs if seqs else None, twin_of)


# ------------------------------------------------------------------------------------------------ families
def _overlap(rng, dicts):
    out = []
    dct = dicts["d3000"]
    for o in OVERLAP_OFFSETS:
        f = _Frame(rng, "overlap_ab_o%d" % o, "overlap")
        f.add(max(o, 16) + rng.randint(0, 9))
        f.cut()
        for ml in overlap_lengths(o):
            f.add(rng.randint(0, min(o - 1, 12)), o, ml)            # (b) op < o: the source starts in the block before
            f.close()
            f.add(o + rng.randint(0, 3), o, ml)                       # (a) the source lies inside the block
            f.close()
        out.append(f)
        for j, ml in enumerate(overlap_lengths(o)):
            a = (1, max(1, o // 2), o)[j % 3]                         # bytes of the source inside T
            f = _Frame(rng, "overlap_c_o%d_ml%d" % (o, ml), "overlap", dct)
            f.add(o - a, o, ml)                                       # (c) block 0: from T across its end, over itself
            f.close()
            f.add(rng.randint(1, 4), rng.randint(1, 9), rng.randint(4, 12))
            f.close()
            out.append(f)
            if o < 2:
                continue                                              # (d) needs 0 < inframe < offset
            f = _Frame(rng, "overlap_d_o%d_ml%d" % (o, ml), "overlap", dct)
            p0 = min(o - 1, 5 + j)
            f.add(p0)
            f.cut()
            f.add(rng.randint(0, min(o - 1 - p0, 8)), o, ml)          # (d) block 1: across T ++ block 0, over itself
            f.close()
            out.append(f)
    return out


def _runs(rng, dicts):
    out = []
    for dct in (None, dicts["d65536"]):
        f = _Frame(rng, "runs_" + ("linked" if dct is None else "dict"), "runs", dct)
        if dct is None:
            f.stored(40000)
            f.stored(40000)
        else:
            f.add(20)
            f.cut()
        for L in RUN_LENGTHS:
            f.add(L, 65535, L if L >= 4 else 4)                       # a literal run of L, a far match of L
            f.close()
            if L >= 4:
                f.add(L, L, L)                                        # touching: offset == ml
                f.close()
        out.append(f)
    return out


def _hist(rng, dicts):
    out = []

    def probe(f, lit, off):
        f.add(lit, off, 8, probe=True)
        f.close(6, 9)

    def start(tag, dct, pos):
        f = _Frame(rng, "hist_" + tag, "hist", dct)
        if pos >= HISTORY:
            for _ in range(pos // 40000):
                f.stored(40000)
        elif pos:
            f.add(pos)
            f.cut()
        return f

    for D, pos in HIST_PAIRS:
        for extra, word in ((0, "accepted"), (1, "refused")):
            f = start("D%d_pos%d_%s" % (D, pos, word), dicts["d500"] if D else None, pos)
            probe(f, 12, 12 + pos + D + extra)
            if pos == 0:
                f.add(3, 2, 6)                                        # a second block: the frame goes the serial way
                f.close()
            out.append(f)
    for pos, lit, word in ((534, 0, "refused"), (534, 1, "accepted"), (535, 0, "accepted")):
        f = start("D65000_pos%d_op%d_%s" % (pos, lit, word), dicts["d65000"], pos)
        probe(f, lit, 65535)
        out.append(f)
    for pos in (0, 10):                               # D = 70 000: T is the dictionary's last 65 536 bytes
        f = start("D70000_pos%d" % pos, dicts["d70000"], pos)
        probe(f, 0, 65535)
        f.add(2, 65535, 9)
        f.close()
        out.append(f)
    f = start("D500_pos80000", dicts["d500"], 80000)   # pos >= 65536: offset 65535 at op = 0 reads the frame, never T
    probe(f, 0, 65535)
    out.append(f)
    return out


def _slide(rng, dicts):
    out = []
    for dct in (None, dicts["d500"]):
        f = _Frame(rng, "slide_short_blocks_" + ("linked" if dct is None else "dict"), "slide", dct)
        f.add(2000)
        f.cut()
        while f.pos < 70000:
            for _ in range(rng.randint(2, 5)):
                reach = min(f.b.op + f.D, 65535)
                u = rng.random()
                if u < 0.4:
                    off, ml = rng.randint(max(1, reach - 2000), reach), rng.randint(20, 400)   # far
                elif u < 0.7:
                    off, ml = rng.randint(1, 200), rng.randint(4, 500)                        # near, often overlapping
                else:
                    off, ml = rng.randint(1, reach), rng.randint(4, 300)
                f.add(rng.randint(0, 20), off, ml)
            f.close()
        out.append(f)
    f = _Frame(rng, "slide_one_block_past_64k", "slide", None, bsid=5)
    f.add(3000, 1500, 40)
    while f.op < 66000:
        f.add(rng.randint(0, 3), rng.randint(1, min(f.op, 65535)), rng.choice((274, 1000, 3000)))
    for _ in range(12):
        f.add(rng.randint(0, 3), 65535, rng.randint(4, 40))
        f.add(rng.randint(0, 3), rng.randint(1, 65535), rng.randint(4, 40))
    f.close()
    out.append(f)
    return out


def _ends(rng, dicts):
    out = []
    for dct in (None, dicts["d500"]):
        f = _Frame(rng, "ends_" + ("linked" if dct is None else "dict"), "ends", dct)
        f.add(40, 7, 30)                                              # block 0 ends right after a match
        f.cut()
        f.add(3, 60, 20)                                              # so does block 1, its source in block 0
        f.cut()
        f.add(33)                                                     # one literal run
        f.cut()
        f.add(b"")                                                    # the one-byte block 00
        f.cut()
        f.stored(100)
        f.add(2, 50, 40)                                              # the stored block is history
        f.close()
        f.stored(17)
        f.add(1, 17, 300)                                             # placement (b) right behind a stored block
        f.close()
        f.stored(1)
        f.add(b"", 1, 1025)
        f.close()
        f.stored(1100)
        f.add(5, 1029, 2100)                                          # offset >= 1024 across the stored block, over itself
        f.close()
        out.append(f)
    return out


def _independent(rng, dicts):
    """frames that declare independent blocks: k_bfl_mask leaves them to the parallel decode of the same call"""
    out = []
    for k in range(4):
        f = _Frame(rng, "independent_%d" % k, "independent", None, block_mode=1)
        for _ in range(1 + k):
            lit = rng.randint(20, 90)
            f.add(lit, rng.randint(1, lit), rng.randint(4, 60))       # (every match stays inside its block)
            for _ in range(rng.randint(3, 12)):
                lit = rng.randint(0, 6)
                f.add(lit, rng.randint(1, f.op + lit), rng.randint(4, 60))
            f.close()
        out.append(f)
    return out


_FAMILIES = (_overlap, _runs, _hist, _slide, _ends, _independent)
_CAP_FRAMES = ("overlap_ab_o17", "overlap_ab_o1024", "overlap_d_o33_ml2000", "runs_linked", "hist_D500_pos300_accepted",
               "ends_linked", "ends_dict", "slide_short_blocks_linked")
_CKS_FLIPS = ("overlap_ab_o3", "overlap_c_o64_ml1025", "runs_dict", "ends_linked", "hist_D0_pos300_accepted",
              "slide_short_blocks_dict")


def make_dicts(seed):
    rng = random.Random(seed * 1000 + 77)
    return {"d%d" % n: bytes(rng.getrandbits(8) for _ in range(n)) for n in (500, 3000, 65000, 65536, 70000)}


def _block_spans(frame, block_checksum=False):
    """-> [(payload start, payload length)] of a frame built here (7-byte header)"""
    spans, p = [], 7
    while True:
        h = int.from_bytes(frame[p:p + 4], "little")
        if h == 0:
            return spans
        spans.append((p + 4, h & 0x7FFFFFFF))
        p += 4 + (h & 0x7FFFFFFF) + (4 if block_checksum else 0)


def _flip(rng, frame, block_checksum=False):
    spans = _block_spans(frame, block_checksum)
    s, n = spans[rng.randrange(len(spans))]
    # the flip window: the first bytes of a payload are tokens and lengths (a flip there mostly breaks the block), the
    # rest is mostly literals (a flip there decodes)
    at = s + (rng.randrange(min(n, 3)) if rng.random() < 0.25 else rng.randrange(n))
    b = bytearray(frame)
    b[at] ^= 1 << rng.randrange(8)
    return bytes(b)


def corpus(seed=2027):
    """-> [Item]: the base frames (capacity n, no checksums), their variants, the `caps` and the `damaged` items"""
    dicts = make_dicts(seed)
    frames = []
    for fi, fam in enumerate(_FAMILIES):
        frames += fam(random.Random(seed * 1000 + fi), dicts)
    items = []
    for f in frames:
        refused = f.plain is None
        items.append(f.item(status=(FAILED if refused else len(f.plain)) if f.family == "hist" else None))
        if f.dict is None:
            items.append(f.item(f.name + "+checksums", seqs=False, block_checksum=True, content=True,
                                status=(FAILED if refused else len(f.plain)) if f.family == "hist" else None))
        if f.dict is not None and f.family in ("overlap", "hist") and len(f.blocks) > 1:
            good = f.bad_block is None or f.bad_block > 0
            first = f.blocks[0]
            ok0 = first[1] or (f.cuts[0] <= HISTORY and f.ok)
            items.append(f.item(f.name + "+twin", blocks=[first], plain=bytes(f.b.out[:f.cuts[0]]) if good else None,
                                seqs=False, twin_of=f.name, ok=ok0,
                                status=(FAILED if not good else f.cuts[0]) if f.family == "hist" else None))
    by_name = {f.name: f for f in frames}
    for name in _CAP_FRAMES:
        f = by_name[name]
        n = len(f.plain)
        last_lits = n - max(s["pos"] + s["op"] + s["ml"] for s in f.seqs if s["k"] == len(f.blocks) - 1)
        inside = next(s for s in f.seqs if s["k"] >= 1 and s["ml"] >= 8)
        caps = [(n - 1, None), (n - max(1, last_lits // 2), None), (inside["pos"] + inside["op"] + inside["ml"] // 2, None),
                (0, None)]
        if f.stored_at:
            at, ln = f.stored_at[-1]
            caps.append((at + ln // 2, STORED_TOO_LARGE))
        for cap, status in caps:
            items.append(f.item("%s@cap%d" % (name, cap), cap=cap, status=status, seqs=False, family="caps"))
    rng = random.Random(seed * 1000 + 99)
    for f in frames:
        if f.family == "independent":
            continue
        base = f.item()
        cap = f.b.op + 64
        items.append(Item(f.name + "~flip", "damaged", _flip(rng, base.frame), f.dict, cap, None))
        spans = _block_spans(base.frame)
        if rng.random() < 0.5:                        # cut at a block's end: the chain just stops there
            s, n = spans[rng.randrange(len(spans))]
            cut = s + n
        else:
            cut = rng.randrange(8, len(base.frame) - 1)
        items.append(Item(f.name + "~cut", "damaged", base.frame[:cut], f.dict, cap, None))
    for name in _CKS_FLIPS:                           # the block checksum fails before any decode
        f = by_name[name]
        frame = _flip(rng, f.item(block_checksum=True).frame, True)
        items.append(Item(name + "~cksflip", "damaged", frame, f.dict, f.b.op + 64, None, status=BLOCK_CHECKSUM))
    return items


# ------------------------------------------------------------------------------------------------ census
def classify(s):
    """One match record -> the facts of its copy in decode_block_wave, from (pos, op, offset, ml, D) alone."""
    inframe = min(s["pos"], HISTORY)
    hist = min(inframe + s["D"], HISTORY)
    op, off, ml = s["op"], s["off"], s["ml"]
    c = dict(hist=hist, accepted=not (off > op and off - op > hist), a=0, rest=ml, inframe=inframe)
    if not c["accepted"]:
        return c
    if off > op + inframe:                            # starts in T
        c["a"] = off - op - inframe
        c["rest"] = max(0, ml - c["a"])
    c["doubling"] = 0 < off < c["rest"] and off < 1024
    c["far_overlap"] = off >= 1024 and c["rest"] > off
    return c


def census(items):
    """Counts over the base frames' sequence lists (no decoder involved) -> dict"""
    n = dict(doubling_lt64=0, doubling_64_1023=0, far_overlap=0, inside_T=0, crosses_T=0, crosses_T_overlaps=0,
             crosses_T_overlaps_inframe=0, earlier_block=0, crosses_block_overlapping=0, run_mod16={0: 0, 1: 0, 15: 0})
    place = dict(a=set(), b=set(), c=set(), d=set())
    hist = {}
    for it in items:
        for s in it.seqs or ():
            c = classify(s)
            if s["probe"] and s["off"] - s["op"] in (c["hist"], c["hist"] + 1):
                hist.setdefault(c["hist"], [0, 0])[0 if c["accepted"] else 1] += 1
            if s["lit"] >= 1024 and s["lit"] % 16 in (0, 1, 15):
                n["run_mod16"][s["lit"] % 16] += 1
            if not c["accepted"]:
                continue
            op, off, ml, k = s["op"], s["off"], s["ml"], s["k"]
            if c["doubling"]:
                n["doubling_lt64" if off < 64 else "doubling_64_1023"] += 1
            n["far_overlap"] += c["far_overlap"]
            if c["a"]:
                n["inside_T"] += ml <= c["a"]
                n["crosses_T"] += ml > c["a"]
                n["crosses_T_overlaps"] += c["rest"] > off
                n["crosses_T_overlaps_inframe"] += c["rest"] > off and c["inframe"] > 0
            elif off > op:
                n["earlier_block"] += 1
                n["crosses_block_overlapping"] += ml > off
            if ml <= off or c["far_overlap"]:         # one copy_bytes call of ml bytes (or of the part after T)
                for run in ((min(c["a"], ml), c["rest"]) if c["a"] else (ml,)):
                    if run >= 1024 and run % 16 in (0, 1, 15):
                        n["run_mod16"][run % 16] += 1
            if it.family == "overlap" and ml > off:
                if c["a"]:
                    place["c" if k == 0 else "d"].add(off)
                elif k >= 1:
                    place["b" if off > op else "a"].add(off)
    n["place"], n["hist"] = place, hist
    return n
