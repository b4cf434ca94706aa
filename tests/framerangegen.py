"""Corpus and batch runner for the frame index and frame range decoding (tests/test_frame_range_cpu.py,
tests/test_gpu_frame_range.py).  Test infrastructure: frames are built with linkedgen.build_frame and
the dictgen seq / pattern helpers, as frameprefixgen does, and taken from tests/golden/; expectations come from
tools/pyref/zig_lz4_frame_range.py and, for the defect and wrong-index cases, from statements made here by hand.

A View is a frame together with AN index (entries, idx_n) -- the index is the caller's data, so a view may pair a frame with
an index that is not its own.  An Item is one range of one view: (name, view, a, b, reserved, cap_delta, frame_override).
"""
import functools
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools", "pyref"))
import dictgen  # noqa: E402
import frameprefixgen  # noqa: E402
import linkedgen  # noqa: E402
import linkedseqgen  # noqa: E402
import zig_lz4_frame_range as fr  # noqa: E402
import zig_lz4_sizes as zs  # noqa: E402

seq, pat, build, asm = dictgen.seq, dictgen.pattern, linkedgen.build_frame, linkedseqgen.assemble
INVALID_STATE, DST_TOO_SMALL, FAILED, BLOCK_CHECKSUM = -5, -111, -116, -107
TAIL = pat(9, 33)
BIG = 1 << 63


class View:
    __slots__ = ("name", "family", "frame", "entries", "idx_n", "valid")

    def __init__(self, name, family, frame, index=None, valid=True):
        """index None: the frame's own (the model's frame_index); valid: every range of it is bytes [a, b) of the full decode"""
        self.name, self.family, self.frame, self.valid = name, family, frame, valid
        self.idx_n, self.entries = fr.frame_index(frame) if index is None else index

    @property
    def size(self):
        return self.entries[self.idx_n][1] if self.idx_n >= 0 else 0

    @property
    def bounds(self):
        return [e[1] for e in self.entries] if self.idx_n >= 0 else []


@functools.lru_cache(maxsize=None)
def full(frame):
    """the full linked decode model into a destination that is large enough -> (R, bytes)"""
    return linkedgen.lf.decompress_frame_linked(frame, 1 << 30)


def c(n, seed):
    """a compressed block that decodes to n >= 30 bytes: literals, a match inside the block, the last literals"""
    lit = n // 2
    return seq(pat(lit, seed), lit // 2 + 1, n - lit - 9) + seq(TAIL)


FIVE = [(c(300, 1), False), (seq(pat(17, 2)), False), (c(1100, 3), False), (b"\x00", False), (c(40, 4), False)]
FIVE_STORED = [(c(300, 1), False), (pat(17, 5), True), (c(1100, 3), False), (b"", True), (c(40, 4), False), (pat(70, 6), True)]
THREE = [(c(64, 80), False), (c(62, 81), False), (c(44, 82), False)]       # b0 = [0, 64), b1 = [64, 126), b2 = [126, 170)


def _cks(blocks, mode=1):
    plain = build(blocks, block_mode=mode)
    r, data = full(plain)
    assert r >= 0
    return build(blocks, True, data, block_mode=mode)


@functools.lru_cache(maxsize=None)
def small_views():
    """independent frames of at most 3 KiB: 1-6 blocks of unequal, short sizes, a block that decodes to nothing, stored
    blocks (one of 0 bytes), with and without checksums, the empty frame, a one-block frame"""
    return [View("five", "small", build(FIVE, block_mode=1)),
            View("five_stored_cks", "small", _cks(FIVE_STORED)),
            View("five_cks", "small", _cks(FIVE)),
            View("five_no_end_mark", "small", build(FIVE, end_mark=False, block_mode=1)),
            View("empty", "small", build([], block_mode=1)),
            View("empty_cks", "small", build([], True, b"", block_mode=1)),
            View("one_block", "small", build([(c(333, 7), False)], block_mode=1)),
            View("one_stored_cks", "small", _cks([(pat(45, 8), True)])),
            View("linked_declared_no_refs", "small", build(FIVE, block_mode=0))]


def _b64k(seed):
    """65536 bytes: 20000 literals, three matches that do not run over themselves, one that does not either, the tail"""
    return seq(pat(20000, seed), 15000, 15000) + seq(b"", 15000, 15000) * 2 + seq(b"", 15000, 527) + seq(TAIL)


def _b256k(seed):
    """262144 bytes: 50000 literals, 5 x 40000 copied from 40000 back, 12135 more, the tail"""
    return seq(pat(50000, seed), 40000, 40000) + seq(b"", 40000, 40000) * 4 + seq(b"", 40000, 12135) + seq(TAIL)


@functools.lru_cache(maxsize=None)
def long_views():
    """3 x 64 KiB + a short block; 2 x 256 KiB; 4 MiB block size with short blocks, as a flushing writer leaves them"""
    b256 = [(_b256k(20 + k), False) for k in range(2)]
    flush = [(c(5000, 23), False), (seq(pat(30000, 24), 20000, 20000) + seq(b"", 20000, 19991) + seq(TAIL), False),
             (pat(100, 25), True),
             (c(100, 26), False)]
    three64 = [(_b64k(10), False), (_b64k(11), False), (_b64k(12), False), (c(1000, 13), False)]
    return [View("three_64k_and_short", "long", build(three64, block_mode=1)),
            View("three_64k_and_short_cks", "long", _cks(three64)),
            View("two_256k", "long", asm(b256, bsid=5, block_mode=1)),
            View("bs4m_short_blocks", "long", asm(flush, bsid=7, block_mode=1))]


def _history_sizer(data, dec):
    return zs.block_size(data, dict_len=min(dec, 65536))


@functools.lru_cache(maxsize=None)
def linked_views():
    """a linked frame whose second block reaches into the first: the index call answers DecompressionFailed for it (the
    plain size query's view); with the history-aware index a caller may hold, ranges in block 0 are fine and a range that
    takes block 1 behind its 10 literals fails.  Also liblz4's linked frames of tests/golden."""
    ref = build([(seq(pat(300, 55)), False), (seq(pat(10, 56), 30, 60) + seq(TAIL), False)], block_mode=0)
    out = [View("linked_ref", "linked", ref, valid=False),
           View("linked_ref_history_index", "linked", ref, fr.frame_index(ref, sizer=_history_sizer), valid=False)]
    for fx in linkedgen.fixtures():
        if len(fx["input"]) < 300000:
            out.append(View("fx_" + fx["name"], "linked", fx["frame"], valid=False))
            out.append(View("fx_" + fx["name"] + "_history_index", "linked", fx["frame"],
                            fr.frame_index(fx["frame"], sizer=_history_sizer), valid=False))
    return out


@functools.lru_cache(maxsize=None)
def defect_views():
    """-> [(View, want)]: want(a', b') states by hand what a non-empty range gives: None = success, else the code.  The
    index is that of the undamaged frame (the defects keep every block's length)."""
    good, good_cks = build(THREE, block_mode=1), _cks(THREE)
    gi, gci = fr.frame_index(good), fr.frame_index(good_cks)
    r, data = full(good)
    assert r == 170 and gi[0] == 3
    lit = 44 // 2                                                      # block 2: 22 literals, then the match
    bad2 = seq(pat(lit, 82), 0, 44 - lit - 9) + seq(TAIL)              # offset 0, met once the cut lies behind the literals
    assert len(bad2) == len(THREE[2][0])
    return [
        (View("corrupt_block2", "defect", build(THREE[:2] + [(bad2, False)], block_mode=1), gi, False),
         lambda a, b: FAILED if b > 126 + lit else None),
        (View("bad_block_cks_1", "defect", build(THREE, True, data, block_mode=1, bad_block_cks=1), gci, False),
         lambda a, b: BLOCK_CHECKSUM if a < 126 and b > 64 else None),
        (View("bad_content_cks", "defect", build(THREE, True, data, block_mode=1, bad_content_cks=True), None, False),
         lambda a, b: None),
        (View("good_three", "defect", good), lambda a, b: None),
    ]


@functools.lru_cache(maxsize=None)
def header_views():
    """every header error of frameprefixgen.header_cases(): with the status the index call leaves (that code), and with an
    index that claims one block (the range decode parses the header itself: the same code)"""
    out = []
    for name, frame, want in frameprefixgen.header_cases():
        assert fr.frame_index(frame)[0] == want
        out.append((View("hdr_" + name, "header", frame, valid=False), want))
        out.append((View("hdr_" + name + "_claimed", "header", frame, (1, [(7, 0), (max(8, len(frame)), 20)]), False), want))
    return out


def _mod(entries, k, dpos=0, ddec=0, upto=None):
    return [(p + dpos, d + ddec) if (i >= k and (upto is None or i < upto)) else (p, d) for i, (p, d) in enumerate(entries)]


@functools.lru_cache(maxsize=None)
def wrong_index_views():
    """-> [(View, ranges, want)]: the frame `five` (blocks at decoded 0, 300, 317, 1417, 1417, S = 1457) under indexes that
    are not its own; want = the status stated by hand for each of `ranges` (None: success)"""
    five = small_views()[0]
    f, E, nb = five.frame, five.entries, five.idx_n
    assert [d for _, d in E] == [0, 300, 317, 1417, 1417, 1457] and nb == 5
    other = fr.frame_index(build(THREE, block_mode=1))
    swapped = list(E)
    swapped[1], swapped[2] = (E[1][0], E[2][1]), (E[2][0], E[1][1])       # dec: 0, 317, 300, ...
    more = E + [(E[5][0] + 4, 1467), (E[5][0] + 5, 1477)]
    inside0, whole, blk2 = (5, 100), (0, BIG), (317, 1417)
    V = lambda name, idx, frame=f: View("wrong_" + name, "wrong", frame, idx, False)    # noqa: E731
    st = small_views()[1]                                              # five_stored_cks: block 1 is stored, [300, 317)
    return [
        (V("other_frames_index", other), [(0, 64), (70, 100)], INVALID_STATE),
        (V("pos_shifted_by_one", (nb, _mod(E, 0, dpos=1))), [inside0, whole], INVALID_STATE),
        (V("pos2_shifted_by_one", (nb, _mod(E, 2, dpos=1, upto=3))), [(300, 310), blk2, whole], INVALID_STATE),
        (V("pos2_shifted_by_one", (nb, _mod(E, 2, dpos=1, upto=3))), [inside0], None),
        (V("pos_past_src_len", (nb, _mod(E, 3, dpos=len(f) + 100))), [blk2, whole], INVALID_STATE),
        (V("pos_past_src_len", (nb, _mod(E, 3, dpos=len(f) + 100))), [inside0, (300, 317)], None),
        (V("dec_not_monotonic", (nb, swapped)), [whole, (0, 1000)], INVALID_STATE),
        # (the bisection finds block 0 for both ends; its step says 317, the block holds 300: the cut decode comes up short)
        (V("dec_not_monotonic", (nb, swapped)), [(0, 310), (300, 310)], FAILED),
        (V("dec_step_above_block_size", (nb, _mod(E, 3, ddec=70000))), [(317, 2000), (400, 401)], INVALID_STATE),
        (V("dec_step_above_block_size", (nb, _mod(E, 3, ddec=70000))), [inside0], None),
        (V("dec_too_small_for_block2", (nb, _mod(E, 3, ddec=-1))), [(317, 1416), whole], FAILED),
        (V("dec_too_large_for_block2", (nb, _mod(E, 3, ddec=1))), [(317, 1418), whole], FAILED),
        (V("dec_too_large_for_block2", (nb, _mod(E, 3, ddec=1))), [inside0, (317, 1000)], None),
        (V("dec_too_large_for_stored", (st.idx_n, _mod(st.entries, 2, ddec=1)), st.frame), [(300, 318)], INVALID_STATE),
        (V("idx_n_above_the_count", (nb + 2, more)), [inside0, (0, 1457)], None),
        (V("idx_n_above_the_count", (nb + 2, more)), [(1450, 1460), (1460, 1470), whole], INVALID_STATE),
        (V("idx_n_below_the_count", (3, E[:4])), [(0, BIG)], None),        # a shorter index is a shorter frame: S = 1417
    ]


def small_ranges(view, every_a=True):
    """every a in 0 .. S + 1 (or, every_a False, around the block boundaries) with b in { a, a + 1, a + 17, each block
    boundary - 1 / 0 / + 1, S, S + 1, 2^63 }"""
    S, bounds = view.size, view.bounds
    ends = {S, S + 1, BIG}
    for d in bounds:
        ends.update((d - 1, d, d + 1))
    starts = range(0, S + 2) if every_a else sorted({x for d in bounds + [0, S] for x in (d - 1, d, d + 1, d + 7) if 0 <= x <= S + 1})
    out = []
    for a in starts:
        for b in sorted(ends | {a, a + 1, a + 17}):
            if b >= a:
                out.append((a, b))
    return out


def long_ranges(view):
    """sampled a, b around every block boundary and S"""
    S, bounds = view.size, sorted(set(view.bounds))
    out = []
    for i, d in enumerate(bounds):
        nxt = bounds[i + 1] if i + 1 < len(bounds) else S
        for a in (d - 1, d, d + 1):
            if 0 <= a <= S + 1:
                for b in (a, a + 1, a + 4096, nxt - 1, nxt, nxt + 1, S, S + 1):
                    if b >= a:
                        out.append((a, b))
    out += [(0, S), (0, BIG), (S // 2, S // 2 + 65536)]
    return sorted(set(out))


def items_of(views, ranges_of):
    """-> (views, items): every range of every view"""
    items = []
    for v, view in enumerate(views):
        for a, b in ranges_of(view):
            items.append(("%s[%d,%d)" % (view.name, a, min(b, 1 << 40)), v, a, b, 0, None, None))
    return list(views), items


def _args(views, item):
    name, v, a, b, reserved, cap_delta, frame_over = item
    view = views[v]
    need = fr.plan_range(view.entries, view.idx_n, a, b)[0]
    cap = need if cap_delta is None else max(0, need + cap_delta)
    return view.frame, view.entries, view.idx_n, a, b, cap, reserved, frame_over is None


def item_counts(views, items):
    """the items every range takes of max_items (0 for a range that statuses 1-3 end)"""
    return [fr.range_items(*_args(views, it)) for it in items]


def expect(views, items, max_items=None):
    """the model over one batch -> [(result, skip, slot bytes)], `fits` decided by the items the ranges in front take"""
    out, base = [], 0
    for it, n in zip(items, item_counts(views, items)):
        fits = max_items is None or n == 0 or base + n <= max_items
        base += n
        out.append(fr.decompress_frame_range(*_args(views, it), fits=fits))
    return out


# ----------------------------------------------------------------------------- the GPU side
def stage(views, items, dev, spare_views=0):
    """the device arrays of one batch: distinct frames stored once, every view's index with two spare entries behind it,
    every slot exactly the planned size (+ cap_delta) between guard bands -> dict"""
    import numpy as np
    import torch
    import gpu_harness as gh
    frames, fidx = [], {}
    for v in views:
        if v.frame not in fidx:
            fidx[v.frame] = len(frames); frames.append(v.frame)
    buf, offs, lens = gh._pack(frames)
    fi = np.array([fidx[v.frame] for v in views], dtype=np.int64)
    ents, idx_off = [], []
    for v in views:
        idx_off.append(len(ents))
        ents += list(v.entries) + [(0, 0), (0, 0)]
    index = np.array(ents or [(0, 0)], dtype=np.uint64).reshape(-1, 2)
    idx_n = np.array([v.idx_n for v in views], dtype=np.int64)
    rng = np.zeros((max(1, len(items)), 3), dtype=np.uint64)
    caps = []
    for i, (name, v, a, b, reserved, cap_delta, frame_over) in enumerate(items):
        rng[i] = ((v if frame_over is None else frame_over) | (reserved << 32), a, b)
        need = fr.plan_range(views[v].entries, views[v].idx_n, a, b)[0]
        caps.append(need if cap_delta is None else max(0, need + cap_delta))
    caps = np.array(caps, dtype=np.int64)
    out_offs, guard_ends, total = gh._out_slots(caps)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    nv = len(views) - spare_views
    return dict(buf=buf, caps=caps, out_offs=out_offs, guard_ends=guard_ends, nframes=nv,
                d_src=t(buf), src_off=t(offs[fi]), src_len=t(lens[fi]), index=t(index.view(np.int64)),
                idx_off=t(np.array(idx_off, dtype=np.int64)), idx_n=t(idx_n)[:nv], ranges=t(rng.view(np.int64))[:len(items)],
                d_dst=torch.full((total,), 0xA5, dtype=torch.uint8, device=dev), dst_off=t(out_offs), dst_cap=t(caps),
                skip=torch.full((len(items),), -999, dtype=torch.int64, device=dev),
                result=torch.full((len(items),), -999, dtype=torch.int64, device=dev))


def run(zl, views, items, dev, max_items=None, spare_views=0):
    """one zlz4f_batch_decompress_frame_range call -> [(result, skip, slot bytes[0, planned size))]; the source arena is
    unchanged and every guard band is intact, whatever the range's status"""
    import torch
    s = stage(views, items, dev, spare_views)
    if max_items is None:
        max_items = sum(fr.plan_range(views[v].entries, views[v].idx_n, a, b)[1] for _, v, a, b, _, _, _ in items)
    zl.lz4f.decompressFrameRangeBatch(s["d_src"], s["src_off"], s["src_len"], s["index"], s["idx_off"], s["idx_n"], s["ranges"],
                                      s["d_dst"], s["dst_off"], s["dst_cap"], s["skip"], s["result"], max_items)
    torch.cuda.synchronize()
    assert (s["d_src"].cpu().numpy() == s["buf"]).all(), "the source arena changed"
    o = s["d_dst"].cpu().numpy()
    res, skip = s["result"].cpu().tolist(), s["skip"].cpu().tolist()
    out = []
    if len(items):
        assert (o[:s["out_offs"][0]] == 0xA5).all(), "a range wrote in front of the first slot"
    for i in range(len(items)):
        lo, cap = int(s["out_offs"][i]), int(s["caps"][i])
        assert (o[lo + cap:s["guard_ends"][i]] == 0xA5).all(), "%s wrote past its slot" % items[i][0]
        out.append((res[i], skip[i], bytes(o[lo:lo + cap])))
    return out


def compare(views, items, got, want):
    bad = []
    for it, (r, sk, slot), (wr, wsk, wslot) in zip(items, got, want):
        if r != wr or sk != wsk or (wr >= 0 and slot[:len(wslot)] != wslot):
            bad.append("%s: GPU (%d, skip %d) vs model (%d, skip %d)%s" % (it[0], r, sk, wr, wsk,
                                                                             " (bytes differ)" if (r, sk) == (wr, wsk) else ""))
        elif wr >= 0 and views[it[1]].valid:
            a = min(it[2], views[it[1]].size)
            assert slot[sk:sk + r] == full(views[it[1]].frame)[1][a:a + r], it[0]
    assert not bad, "%d of %d ranges differ:\n%s" % (len(bad), len(items), "\n".join(bad[:20]))
