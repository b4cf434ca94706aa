"""Corpus and batch runner for frame prefix decoding (tests/test_frame_prefix_cpu.py, tests/test_gpu_frame_prefix.py;
DESIGN.md section 4.4f).  Test infrastructure: frames are built from the helpers of linkedgen, linkedseqgen and dictframegen
and from the fixtures of tests/golden/; expectations come from tools/pyref/zig_lz4_frame_prefix.py (cached per process) and,
for the defect cases, from statements made here by hand.

A Case is one frame with its dictionary and the cuts to try: `ns` None = every n in 0 .. S + 1 (S = the full decode's size,
the frames of at most 3 KiB), else the listed ones (the long frames: each model run decodes up to the cut in Python).
items(cases) -> [(name, frame, n, dict)], one per cut.
"""
import functools
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools", "pyref"))
import dictframegen  # noqa: E402
import dictgen  # noqa: E402
import linkedgen  # noqa: E402
import linkedseqgen  # noqa: E402
import zig_lz4_dict_frame as dfm  # noqa: E402
import zig_lz4_frame_prefix as fp  # noqa: E402

seq, pat, build = dictgen.seq, dictgen.pattern, linkedgen.build_frame
FRAME_SIZE_WRONG, BLOCK_CHECKSUM, FAILED, CONTENT_CHECKSUM, INVALID_STATE = -114, -107, -116, -118, -5
HEADER_INCOMPLETE, TYPE_UNKNOWN, VERSION_WRONG, RESERVED, MAX_BLOCK_SIZE, HEADER_CHECKSUM = -112, -113, -106, -108, -102, -117
TAIL = pat(9, 33)                                     # a block's last literals (five or more keep liblz4 content)
BIG = 1 << 30


class Case:
    __slots__ = ("name", "family", "frame", "dict", "ns", "valid")

    def __init__(self, name, family, frame, dct=None, ns=None, valid=True):
        self.name, self.family, self.frame, self.dict, self.ns, self.valid = name, family, frame, dct, ns, valid


@functools.lru_cache(maxsize=None)
def full(frame, dct=None):
    """the full decode model into a destination that is large enough -> (R, bytes)"""
    return dfm.decompress_frame_using_dict(frame, BIG, dct)


@functools.lru_cache(maxsize=None)
def expected(frame, n, dct=None):
    return fp.decompress_frame_prefix(frame, n, dct)


def _both(name, family, blocks, mode, dct=None):
    """the frame without checksums and the same blocks with block and content checksums"""
    plain = build(blocks, block_mode=mode)
    r, data = full(plain, dct)
    assert r >= 0, name
    return [Case(name, family, plain, dct), Case(name + "_cks", family, build(blocks, True, data, block_mode=mode), dct)]


@functools.lru_cache(maxsize=None)
def small_cases():
    """Crafted frames of at most 3 KiB of output, one or two per place a cut can fall (the issue's list), independent and
    linked, with and without checksums; every n in 0 .. S + 1."""
    out = []
    # literal runs: 1100 literals (the 16-byte pieces, the 1 KiB chunk of copy_bytes, the byte tail), 17, 9
    lit = [(seq(pat(1100, 31), 1000, 40) + seq(pat(17, 32), 60, 33) + seq(TAIL), False)]
    out += _both("literals_indep", "literals", lit, 1)
    out.append(Case("literals_linked", "literals", build(lit, block_mode=0)))
    # disjoint matches
    out += _both("disjoint", "disjoint", [(seq(pat(50, 34), 40, 30) + seq(pat(20, 35), 90, 64) + seq(TAIL), False)], 0)
    # a far overlapping match: offset >= 1024 (one copy_bytes call over itself), n > offset
    out.append(Case("far_overlap", "far", build([(seq(pat(1100, 36), 1030, 1500) + seq(TAIL), False)], block_mode=1)))
    # the doubling copy
    for o in (1, 2, 3, 7, 63):
        out.append(Case("double_o%d" % o, "doubling", build([(seq(pat(70, 40 + o), o, 300) + seq(TAIL), False)], block_mode=0)))
    out.append(Case("double_o1023", "doubling", build([(seq(pat(1030, 39), 1023, 1900) + seq(TAIL), False)], block_mode=1)))
    # stored blocks: cut inside one; a match that starts in one, crosses into its own block and runs over itself
    st = [(pat(100, 50), True), (seq(pat(10, 51), 60, 80) + seq(TAIL), False), (pat(40, 52), True)]
    out += _both("stored_linked", "stored", st, 0)
    out += _both("stored_indep", "stored", [(pat(100, 53), True), (seq(pat(30, 54), 20, 8) + seq(TAIL), False)], 1)
    # linked frames: a match across the block boundary (overlapping, offset < length; and disjoint), three blocks
    b0 = (seq(pat(300, 55)), False)
    out += _both("cross_block_overlap", "cross", [b0, (seq(pat(10, 56), 30, 60) + seq(TAIL), False)], 0)
    out += _both("cross_block_disjoint", "cross", [b0, (seq(pat(10, 57), 10 + 250, 100) + seq(TAIL), False),
                                                  (seq(pat(5, 58), 5 + 300, 12) + seq(TAIL), False)], 0)
    out.append(Case("empty_frame", "empty", build([])))
    out.append(Case("empty_frame_cks", "empty", build([], True, b"")))
    return out


@functools.lru_cache(maxsize=None)
def dict_cases():
    """Dictionary frames: the valid crafted frames of dictframegen (matches that end in T, cross T's end, run over
    themselves; independent, linked, one block and two), every n; then one frame under dictionaries of length 0, one byte
    short, exact and above 64 KiB."""
    out = []
    for name, frame, dct, cap, want, data, ok in dictframegen.crafted_cases():
        if want >= 0 and ok:
            assert full(frame, dct) == (want, data), name
            out.append(Case("dict_" + name, "dict", frame, dct))
    dct = pat(500, 21)
    a = pat(30, 22)
    for mode, tag in ((0, "linked"), (1, "indep")):
        frame = build([(seq(a, 30 + 500, 8) + seq(TAIL), False), (seq(pat(7, 27), 7 + 47 + 3, 12) + seq(TAIL), False)],
                      block_mode=mode)
        over = pat(69500, 9) + dct                    # only the last 64 KiB count: the same bytes as with dct
        for dn, d, ok in (("d0", b"", False), ("short", dct[1:], False), ("exact", dct, True), ("d70000", over, True)):
            assert (full(frame, d)[0] >= 0) == ok
            out.append(Case("dictlen_%s_%s" % (tag, dn), "dictlen", frame, d, valid=ok))
    return out


def _around(*points, lo=0, hi=None):
    ns = set()
    for p in points:
        ns.update(range(p - 2, p + 3))
    return sorted(n for n in ns if n >= lo and (hi is None or n <= hi))


@functools.lru_cache(maxsize=None)
def long_cases():
    """Frames past 64 KiB of output (the history cap, an accepted and a refused offset exactly at the bound) and one frame
    of two 256 KiB blocks; sampled cuts."""
    out = []
    asm = linkedseqgen.assemble
    c = TAIL
    # block 0 stored, pos = 65530: at op = 0 offset 65530 is the frame's first byte, 65531 lies in front of it
    s0 = pat(65530, 60)
    for off, tag, ok in ((65530, "accepted", True), (65531, "refused", False)):
        frame = asm([(s0, True), (seq(b"", off, 20) + seq(c), False)], bsid=5)
        ns = _around(1, 65530, 65531, 65550, 65559)
        out.append(Case("pos65530_off_%s" % tag, "histcap", frame, None, ns, ok))
    # pos = 65236, D = 200: hist = 65436 -- offset 65436 is T's first byte; D = 500: hist = 65536 (the cap), offset 65535
    s1 = pat(65236, 61)
    d200, d500 = pat(200, 62), pat(500, 63)
    for off, dct, tag, ok in ((65436, d200, "T_first_byte", True), (65437, d200, "in_front_of_T", False),
                              (65535, d500, "cap_into_T", True)):
        frame = asm([(s1, True), (seq(b"", off, 400) + seq(c), False)], bsid=5)
        out.append(Case("pos65236_%s" % tag, "histcap", frame, dct, _around(65236, 65237, 65436, 65536, 65645), ok))
    # pos = 70000 > 65536: the dictionary is out of reach, offset 65535 at op = 0 reaches the output alone
    s2 = pat(70000, 64)
    frame = asm([(s2, True), (seq(b"", 65535, 30) + seq(c), False), (seq(pat(12, 65), 12 + 39 + 65000, 10) + seq(c), False)], bsid=5)
    out.append(Case("pos70000_off65535", "histcap", frame, d500, _around(69999, 70030, 70039, 70061, 70070)))
    # two blocks of 256 KiB each: long literal runs, a long match over itself, block 1 reaching back 65535 bytes
    blk0 = seq(pat(50000, 66), 30000, 212000) + seq(pat(135, 67))
    blk1 = seq(pat(100, 68), 65535, 150000) + seq(pat(60000, 69), 7, 52000) + seq(pat(35, 70))
    two = asm([(blk0, False), (blk1, False)], bsid=5, block_mode=0)
    r, data = full(two)
    assert r == 2 * 262135, r
    out.append(Case("two_256k_blocks", "big", two, None, [64, 50001, 262136, 300000, r, r + 1]))
    out.append(Case("two_256k_blocks_cks", "big", asm([(blk0, False), (blk1, False)], 5, True, data, 0), None, [r + 1]))
    return out


@functools.lru_cache(maxsize=None)
def fixture_cases():
    """liblz4's frames of tests/golden (linked_frames.json, dict_frames.json); sampled cuts"""
    out = []
    for fx in linkedgen.fixtures():
        size = len(fx["input"])
        ns = [1, 70001, size, size + 1] if size < 300000 else [300000, size]
        out.append(Case("fx_" + fx["name"], "fixture", fx["frame"], None, ns))
    for fx in dictframegen.fixtures():
        size = len(fx["input"])
        out.append(Case("fxd_" + fx["name"], "fixture", fx["frame"], fx["dict"], [13, 66000, size + 1] if size > 66000 else
                        [13, size, size + 1]))
    return out


def fixture_inputs():
    """frame -> the input liblz4 compressed"""
    m = {fx["frame"]: fx["input"] for fx in linkedgen.fixtures()}
    m.update({fx["frame"]: fx["input"] for fx in dictframegen.fixtures()})
    return m


@functools.lru_cache(maxsize=None)
def defect_cases():
    """-> [(Case, want)]: frames with a defect, every n; want(n) is the result stated by hand.  Three blocks of 64, 62 and
    44 bytes (S = 170): b0 = [0, 64), b1 = [64, 126), b2 = [126, 170)."""
    a, b, c = pat(46, 80), pat(20, 81), pat(12, 82)
    blk0 = seq(a, 20, 9) + seq(TAIL)                 # 46 + 9 + 9 = 64
    blk1 = seq(b, 20 + 50, 33) + seq(TAIL)                             # 20 + 33 + 9 = 62: reaches block 0 (linked)
    blk2 = seq(c, 5, 23) + seq(TAIL)                                   # 12 + 23 + 9 = 44
    three = [(blk0, False), (blk1, False), (blk2, False)]
    r, data = full(build(three))
    assert r == 170
    S = r
    out = []

    def add(name, frame, want, dct=None):
        out.append((Case("defect_" + name, "defect", frame, dct, None, False), want))

    # a corrupt block 2 (its match has offset 0, met at output 126 + 12): cut at or before that point gives n
    bad2 = seq(c, 0, 23) + seq(TAIL)
    add("corrupt_block2", build(three[:2] + [(bad2, False)]), lambda n: n if n <= 138 else FAILED)
    # block checksums: a bad one is met when the block is reached, i.e. once n > the output in front of it
    good = build(three, True, data)
    for k, start in ((0, 0), (1, 64), (2, 126)):
        add("bad_block_cks_%d" % k, build(three, True, data, bad_block_cks=k), lambda n, s=start: n if n <= s else BLOCK_CHECKSUM)
    # the checksum word of block 1 is missing: the source ends right behind block 1's data
    hdr = 7
    end_b0 = hdr + 4 + len(blk0) + 4
    end_b1_data = end_b0 + 4 + len(blk1)
    add("missing_block_cks_1", good[:end_b1_data], lambda n: n if n <= 64 else FRAME_SIZE_WRONG)
    add("missing_block_cks_1_partly", good[:end_b1_data + 3], lambda n: n if n <= 64 else FRAME_SIZE_WRONG)
    # a source truncated inside block 2's data (:582), inside block 2's header (:565)
    plain = build(three)
    p_b2 = hdr + 4 + len(blk0) + 4 + len(blk1)
    add("truncated_in_block2", plain[:p_b2 + 4 + 10], lambda n: n if n <= 126 else FRAME_SIZE_WRONG)
    add("truncated_in_header2", plain[:p_b2 + 2], lambda n: n if n <= 126 else FRAME_SIZE_WRONG)
    # a missing end mark: the input ends at a block boundary, which ends the loop; with a content checksum, :626
    add("no_end_mark", build(three, end_mark=False), lambda n: min(n, S))
    add("no_end_mark_cks", build(three, True, data)[:-8], lambda n: n if n <= S else FRAME_SIZE_WRONG)
    add("end_mark_cut", plain[:-2], lambda n: n if n <= S else FRAME_SIZE_WRONG)
    # the content checksum: wrong, missing
    add("bad_content_cks", build(three, True, data, bad_content_cks=True), lambda n: n if n <= S else CONTENT_CHECKSUM)
    add("missing_content_cks", build(three, True, data)[:-1], lambda n: n if n <= S else FRAME_SIZE_WRONG)
    # the same chain declared independent: block 1's match reaches in front of its block
    add("independent_reach", build(three, block_mode=1), lambda n: n if n <= 84 else FAILED)
    return out


@functools.lru_cache(maxsize=None)
def header_cases():
    """-> [(name, frame, want)]: every header error (src/lz4f.zig:483-538), the result for n == 0 and n > 0 alike"""
    good = build([(seq(pat(20, 90)), False)])
    enc = linkedgen.lf.encode_header

    def with_flg(flg, bd=0x40):
        return b"\x04\x22\x4d\x18" + bytes([flg, bd, 0]) + good[7:]
    cs = enc(4, 0, 0, 0, content_size=20)
    return [
        ("empty_source", b"", HEADER_INCOMPLETE),
        ("six_bytes", good[:6], HEADER_INCOMPLETE),
        ("bad_magic", b"\x05" + good[1:], TYPE_UNKNOWN),
        ("version_0", with_flg(0x00), VERSION_WRONG),
        ("version_2", with_flg(0x80), VERSION_WRONG),
        ("reserved_flg", with_flg(0x42), RESERVED),
        ("reserved_bd", with_flg(0x40, 0x41), RESERVED),
        ("reserved_bd_high", with_flg(0x40, 0xC0), RESERVED),
        ("block_size_id_3", with_flg(0x40, 0x30), MAX_BLOCK_SIZE),
        ("header_checksum", good[:6] + bytes([good[6] ^ 1]) + good[7:], HEADER_CHECKSUM),
        ("content_size_incomplete", cs[:10], HEADER_INCOMPLETE),
        ("dict_id_incomplete", enc(4, 0, 0, 0, dict_id=5)[:9], HEADER_INCOMPLETE),
        ("no_header_checksum_byte", cs[:14], HEADER_INCOMPLETE),
    ]


def items(cases):
    out = []
    for c in cases:
        ns = c.ns
        if ns is None:
            r = full(c.frame, c.dict)[0]
            if r < 0:                                 # (a failing frame: up to the size it has when undamaged, or 200)
                r = 200
            ns = range(0, r + 2)
        out += [("%s@%d" % (c.name, n), c.frame, n, c.dict) for n in ns]
    return out


def compare(its, got):
    """results, and bytes [0, result), against the model"""
    bad = []
    for (name, f, n, d), (r, data) in zip(its, got):
        wr, wd = expected(f, n, d)
        if r != wr or (wr > 0 and data != wd):
            bad.append("%s: GPU %d vs model %d%s" % (name, r, wr, " (bytes differ)" if r == wr else ""))
    assert not bad, "%d of %d items differ:\n%s" % (len(bad), len(its), "\n".join(bad[:20]))


def stage(its, dev, dict_index=None, dicts=None):
    """The device arrays of one batch over `its`: distinct frames and dictionaries are stored once, every output slot is
    exactly n bytes between guard bands (gpu_harness).  -> dict of tensors and host copies"""
    import numpy as np
    import torch
    import gpu_harness as gh
    frames, fidx, dl, didx = [], {}, list(dicts or []), {}
    for k, d in enumerate(dl):
        didx.setdefault(d, k)
    for _, f, _, d in its:
        if f not in fidx:
            fidx[f] = len(frames); frames.append(f)
        d = d or b""
        if dicts is None and d not in didx:
            didx[d] = len(dl); dl.append(d)
    buf, offs, lens = gh._pack(frames)
    dbuf, doffs, dlens = gh._pack(dl)
    fi = np.array([fidx[it[1]] for it in its], dtype=np.int64)
    di = np.array([didx[it[3] or b""] for it in its] if dict_index is None else dict_index, dtype=np.int64)
    caps = np.array([it[2] for it in its], dtype=np.int64)
    out_offs, guard_ends, total = gh._out_slots(caps)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    return dict(buf=buf, dbuf=dbuf, caps=caps, out_offs=out_offs, guard_ends=guard_ends,
                d_src=t(buf), src_off=t(offs[fi]), src_len=t(lens[fi]),
                d_dst=torch.full((total,), 0xA5, dtype=torch.uint8, device=dev), dst_off=t(out_offs), dst_cap=t(caps),
                d_dict=t(dbuf), dict_off=t(doffs), dict_len=t(dlens.astype(np.uint32).view(np.int32)),
                dict_idx=t(di.astype(np.uint32).view(np.int32)),
                result=torch.full((len(its),), -999, dtype=torch.int64, device=dev))


def collect(its, s):
    """after the call: arenas unchanged, guard bands and the bytes of every slot behind a result >= 0 untouched
    -> [(result, bytes)]"""
    import torch
    import gpu_harness as gh
    torch.cuda.synchronize()
    assert (s["d_src"].cpu().numpy() == s["buf"]).all(), "the source arena changed"
    assert (s["d_dict"].cpu().numpy() == s["dbuf"]).all(), "the dictionary arena changed"
    got = gh._collect(s["result"], s["d_dst"], s["out_offs"], s["guard_ends"], s["caps"])
    o = s["d_dst"].cpu().numpy()
    for i, (n, _) in enumerate(got):
        assert n <= s["caps"][i], "%s: result past the slot" % its[i][0]
        if n >= 0:                                    # (a frame that fails may have written what decoded before the defect)
            lo = s["out_offs"][i] + n
            assert (o[lo: s["out_offs"][i] + s["caps"][i]] == 0xA5).all(), "%s wrote behind its result" % its[i][0]
    return got


def run_batch(zl, its, dev, use_dict=None):
    """One zlz4f_batch_decompress_frame_prefix call over `its` (or _using_dict when any item has a dictionary; use_dict
    overrides) -> [(result, bytes)]"""
    if use_dict is None:
        use_dict = any(it[3] for it in its)
    s = stage(its, dev)
    a = (s["d_src"], s["src_off"], s["src_len"], s["d_dst"], s["dst_off"], s["dst_cap"], s["result"])
    if use_dict:
        zl.batch_decompress_frame_prefix(*a, s["d_dict"], s["dict_off"], s["dict_len"], s["dict_idx"])
    else:
        zl.batch_decompress_frame_prefix(*a)
    return collect(its, s)
