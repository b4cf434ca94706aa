"""Corpus and batch runner for the file index and file range decoding (tests/test_file_range_cpu.py,
tests/test_gpu_file_range.py).  Test infrastructure: it composes lz4filegen (the model of whole
files), legacygen (hand-made legacy frames), multiframegen (skippable frames, preferences) and framerangegen (hand-made
frames); expectations come from tools/pyref/zig_lz4_file_range.py, from lz4filegen.expected sliced [a:b], and -- for the
stated cases -- from figures written here by hand.

A View is a file together with AN index (entries, idx_n) -- the index is the caller's data, so a view may pair a file with
an index that is not its own.  An Item is one range of one view: (name, view, a, b, reserved, cap_delta, buf_override).
"""
import functools
import itertools
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools", "pyref"))
import framerangegen as frg  # noqa: E402
import legacygen as lg  # noqa: E402
import lz4filegen as fg  # noqa: E402
import multiframegen as mg  # noqa: E402
import zig_lz4_file_range as ff  # noqa: E402
from oracle import binding as oracle  # noqa: E402

seq, pat, build, c = frg.seq, frg.pat, frg.build, frg.c
INVALID_STATE, DST_TOO_SMALL, FAILED, BLOCK_CHECKSUM = -5, -111, -116, -107
PARAMETER_INVALID = -104
BIG = 1 << 63
MAGIC = lg.le32(lg.MAGIC)


@functools.lru_cache(maxsize=None)
def members():
    """the eight kinds of member, every block decoding to 0..300 bytes -> dict"""
    text = lg.text(300 * 64, 7)
    return dict(
        F=build(frg.THREE, block_mode=1),                                          # three blocks: 64, 62, 44 bytes
        FC=oracle.compress_frame(text[:250], mg._prefs(1, 1, 250)),                # block checksums, content size and checksum
        FS=build([(c(120, 31), False), (pat(33, 32), True), (c(90, 33), False)], block_mode=1),      # a stored block
        FE=build([], block_mode=1),                                                # the empty frame
        SK=mg.skippable(5, b"seek table"),
        L3=lg.build(lg.small_blocks(3, 5)[0]),                                     # legacy, three blocks
        LM=MAGIC,                                                                  # the legacy magic alone
        LZ=lg.build([lg.literal_block(b"ab" * 20), lg.EMPTY, lg.literal_block(b"c" * 7)]),    # a block of 0 bytes
    )


def join(*names):
    m = members()
    return b"".join(m[n] for n in names)


@functools.lru_cache(maxsize=None)
def content(buf, legacy=True):
    """what decompressFiles gives for the file (flags 0: no linked member here) -> bytes, or the code"""
    r, data, _ = fg.expected(buf, 0, legacy)
    return data if r >= 0 else r


class View:
    __slots__ = ("name", "buf", "entries", "idx_n", "valid", "members")

    def __init__(self, name, buf, index=None, valid=True, legacy=True):
        self.name, self.buf, self.valid = name, bytes(buf), valid
        self.idx_n, self.entries = ff.file_index(self.buf, legacy) if index is None else index
        self.members = ff.split(self.buf, legacy)

    @property
    def size(self):
        return self.entries[self.idx_n][1] if self.idx_n >= 0 else 0

    @property
    def bounds(self):
        return [e[1] for e in self.entries] if self.idx_n >= 0 else []


def orderings():
    """every ordering of the eight members -> [bytes]"""
    names = sorted(members())
    return [join(*perm) for perm in itertools.permutations(names)]


@functools.lru_cache(maxsize=None)
def tiny_views():
    """files whose content is at most 80 bytes, for every (a, b): tiny frames (one with checksums, one with a stored block),
    a tiny legacy frame with a block of 0 bytes, a skippable frame, the empty frame, the magic alone"""
    tf = build([(seq(pat(7, 1)), False), (pat(5, 2), True), (seq(pat(9, 3)), False)], block_mode=1)
    tc = frg._cks([(seq(pat(6, 4)), False), (seq(pat(11, 5)), False)])
    tl = lg.build([lg.literal_block(b"abcdef"), lg.EMPTY, lg.literal_block(b"ghi")])
    m = members()
    sk, fe = m["SK"], m["FE"]
    return [View("tiny_frame_frame", tf + tc), View("tiny_frame_legacy_frame", tf + tl + tc),
            View("tiny_legacy_skip_frame", tl + sk + tf), View("tiny_empty_between", tc + fe + MAGIC + tl + sk),
            View("tiny_legacy_legacy", tl + tl), View("tiny_one_frame", tf), View("tiny_nothing", b""),
            View("tiny_skippable_alone", sk), View("tiny_not_legacy", tf + tc, legacy=False)]


def all_ranges(view):
    S = view.size
    return [(a, b) for a in range(S + 2) for b in list(range(a, S + 2)) + [BIG]]


@functools.lru_cache(maxsize=None)
def range_views():
    """files for the ranges of the GPU test: every kind of crossing"""
    return [View("f_fc_l3_fs", join("F", "FC", "L3", "FS")),                      # frame->frame, frame->legacy, legacy->frame
            View("l3_sk_f_fe_lz_lm_fc", join("L3", "SK", "F", "FE", "LZ", "LM", "FC")),    # across a skippable, an empty member
            View("lz_l3_sk", join("LZ", "L3", "SK")),                             # legacy->legacy, a skippable last
            View("one_frame", join("FS"))]


@functools.lru_cache(maxsize=None)
def bound_views():
    """a legacy block of 70 000 zeros next to a frame whose bound is 64 KiB: the bound is the member's, not the range's"""
    z = lg.build([lg.zeros_block(70000)])
    return [View("zeros70k_then_frame", z + members()["F"]), View("frame_then_zeros70k", members()["F"] + z)]


def bound_ranges(view):
    S, out = view.size, []
    for d in view.bounds:
        out += [(max(0, d - 3), min(S, d + 5)), (d, d + 1)]
    return out + [(0, S), (69990, 70010), (100, BIG)]


@functools.lru_cache(maxsize=None)
def lane_edge_views():
    """the 64-lane loop edges: one legacy member and one frame member of 130 tiny blocks, one file of 70 members"""
    blocks = [lg.literal_block(pat(1 + k % 5, 100 + k)) for k in range(130)]
    m = members()
    seventy = b"".join((m["F"], m["L3"], m["SK"], m["LZ"], m["FC"], m["FE"], m["LM"])[k % 7] for k in range(70))
    return [View("legacy_130_blocks", m["SK"] + lg.build(blocks) + m["F"]),
            View("frame_130_blocks", m["L3"] + build([(seq(pat(1 + k % 5, 300 + k)), False) for k in range(130)], block_mode=1)),
            View("seventy_members", seventy)]


def _mod(entries, k, dpos=0, ddec=0, upto=None):
    return frg._mod(entries, k, dpos, ddec, upto)


@functools.lru_cache(maxsize=None)
def wrong_index_views():
    """-> [(View, ranges)]: the file F SK L3 FC (blocks 0-2 in F, 3-5 in L3, 6 in FC) under indexes that are not its own;
    every one of `ranges` touches what is wrong"""
    m = members()
    buf = join("F", "SK", "L3", "FC")
    n, E = ff.file_index(buf)
    assert n == 7
    D = [d for _, d in E]
    f_end, sk_end = len(m["F"]), len(m["F"]) + len(m["SK"])
    l3_end = sk_end + len(m["L3"])
    whole, blk1, blk4, cross = (0, BIG), (D[1], D[2]), (D[4], D[5]), (D[2], D[4])
    V = lambda name, idx: View("wrong_" + name, buf, idx, False)          # noqa: E731
    swapped = list(E)
    swapped[3], swapped[4] = (E[3][0], E[4][1]), (E[4][0], E[3][1])
    out = []
    for d in (1, -1, 4, -4):
        out.append((V("all_pos_shifted_%+d" % d, (n, _mod(E, 0, dpos=d))), [whole, blk1, blk4]))
        out.append((V("pos1_shifted_%+d" % d, (n, _mod(E, 1, dpos=d, upto=2))), [whole, blk1, (D[0], D[1])]))
        out.append((V("pos4_shifted_%+d" % d, (n, _mod(E, 4, dpos=d, upto=5))), [whole, blk4, (D[3], D[4])]))
    out += [
        (V("into_skippable_payload", (n, _mod(E, 3, dpos=f_end + 10 - E[3][0], upto=4))), [whole, (D[3], D[4]), cross]),
        (V("into_skippable_header", (n, _mod(E, 2, dpos=f_end - E[2][0], upto=3))), [whole, (D[2], D[3])]),
        (V("two_bytes_in_front_of_member_end", (n, _mod(E, 5, dpos=l3_end - 2 - E[5][0], upto=6))), [whole, (D[5], D[6])]),
        (V("across_member_end", (n, _mod(E, 2, dpos=sk_end + 4 - E[2][0], upto=3))), [whole, (D[2], D[3])]),
        (V("into_frame_header", (n, _mod(E, 6, dpos=-3, upto=7))), [whole, (D[6], D[7])]),
        (V("past_the_buffer", (n, _mod(E, 4, dpos=len(buf) + 100))), [whole, blk4, (D[3], D[4])]),
        (V("swapped_pair", (n, swapped)), [whole, (D[3], D[5])]),
        (V("dec_step_above_frame_bound", (n, _mod(E, 2, ddec=70000))), [(D[1], D[1] + 70001), (D[1] + 5, D[1] + 6)]),
        (V("dec_step_above_legacy_bound", (n, _mod(E, 5, ddec=9 << 20))), [(D[4], D[4] + 5)]),
        (V("dec_one_too_small", (n, _mod(E, 5, ddec=-1))), [whole, (D[4], D[5] - 1)]),
        (V("dec_one_too_large", (n, _mod(E, 5, ddec=1))), [whole, (D[4], D[5] + 1)]),
        (V("dec_one_too_large_in_frame", (n, _mod(E, 2, ddec=1))), [whole, (D[1], D[2] + 1)]),
    ]
    return out


# ----------------------------------------------------------------------------- the model over a batch
def items_of(views, ranges_of):
    items = []
    for v, view in enumerate(views):
        for a, b in ranges_of(view):
            items.append(("%s[%d,%d)" % (view.name, a, min(b, 1 << 40)), v, a, b, 0, None, None))
    return list(views), items


def _args(views, item):
    name, v, a, b, reserved, cap_delta, buf_over = item
    view = views[v]
    need = ff.plan_range(view.entries, view.idx_n, a, b)[0]
    cap = need if cap_delta is None else max(0, need + cap_delta)
    return view.buf, view.members, view.entries, view.idx_n, a, b, cap, reserved, buf_over is None


def item_counts(views, items):
    return [ff.range_items(*_args(views, it)) for it in items]


def expect(views, items, max_items=None):
    """the model over one batch -> [(result, skip, slot bytes)], `fits` decided by the items the ranges in front take"""
    out, base = [], 0
    for it, n in zip(items, item_counts(views, items)):
        fits = max_items is None or n == 0 or base + n <= max_items
        base += n
        out.append(ff.decompress_file_range(*_args(views, it), fits=fits))
    return out


# ----------------------------------------------------------------------------- the GPU side
def gpu_index(zl, bufs, dev, legacy=True):
    """lz4f.fileIndex -> (FileIndex, [(idx_n, entries)] read back; entries [] for a file that failed)"""
    ix = zl.lz4f.fileIndex(bufs, device=dev, legacy=legacy)
    rows = ix.index.cpu().tolist()
    off = ix.idx_off.cpu().tolist()
    out = []
    for s, n in enumerate(ix.results):
        out.append((n, [tuple(e) for e in rows[off[s]:off[s] + n + 1]] if n >= 0 else []))
    return ix, out


def run(zl, views, items, dev, max_items=None, legacy=True):
    """one zlz4f_batch_decompress_file_range call over the GPU split of the views' files and the VIEWS' indexes ->
    [(result, skip, slot bytes[0, planned size))]; the source arena is unchanged and every guard band is intact"""
    import numpy as np
    import torch
    import gpu_harness as gh
    sp = zl.lz4f.splitMultiframes([v.buf for v in views], dev, legacy)
    before = sp.d_src.clone()
    ents, idx_off = [], []
    for v in views:
        idx_off.append(len(ents))
        ents += list(v.entries) + [(0, 0), (0, 0)]
    index = np.array(ents or [(0, 0)], dtype=np.uint64).reshape(-1, 2)
    rng = np.zeros((max(1, len(items)), 3), dtype=np.uint64)
    caps, planned = [], 0
    for i, (name, v, a, b, reserved, cap_delta, buf_over) in enumerate(items):
        rng[i] = ((v if buf_over is None else buf_over) | (reserved << 32), a, b)
        need, n = ff.plan_range(views[v].entries, views[v].idx_n, a, b)
        planned += n
        caps.append(need if cap_delta is None else max(0, need + cap_delta))
    caps = np.array(caps, dtype=np.int64)
    out_offs, guard_ends, total = gh._out_slots(caps)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)       # noqa: E731
    d_dst = torch.full((total,), 0xA5, dtype=torch.uint8, device=dev)
    skip = torch.full((len(items),), -999, dtype=torch.int64, device=dev)
    result = torch.full((len(items),), -999, dtype=torch.int64, device=dev)
    idx_n = t(np.array([v.idx_n for v in views], dtype=np.int64))
    zl.lz4f.decompressFileRangeBatch(sp.d_src, sp.src_off, sp.src_len, t(index.view(np.int64)),
                                     t(np.array(idx_off, dtype=np.int64)), idx_n, sp.member, sp.mem_off, sp.result,
                                     t(rng.view(np.int64))[:len(items)], d_dst, t(out_offs), t(caps), skip, result,
                                     planned if max_items is None else max_items)
    torch.cuda.synchronize()
    assert torch.equal(sp.d_src, before), "the source arena changed"
    o = d_dst.cpu().numpy()
    res, sk = result.cpu().tolist(), skip.cpu().tolist()
    out = []
    if len(items):
        assert (o[:out_offs[0]] == 0xA5).all(), "a range wrote in front of the first slot"
    for i in range(len(items)):
        lo, cap = int(out_offs[i]), int(caps[i])
        assert (o[lo + cap:guard_ends[i]] == 0xA5).all(), "%s wrote past its slot" % items[i][0]
        out.append((res[i], sk[i], bytes(o[lo:lo + cap])))
    assert (o[guard_ends[-1] if len(items) else 0:] == 0xA5).all(), "the arena's end changed"
    return out


def compare(views, items, got, want):
    bad = []
    for it, (r, sk, slot), (wr, wsk, wslot) in zip(items, got, want):
        if r != wr or sk != wsk or (wr >= 0 and slot[:len(wslot)] != wslot):
            bad.append("%s: GPU (%d, skip %d) vs model (%d, skip %d)%s" % (it[0], r, sk, wr, wsk,
                                                                             " (bytes differ)" if (r, sk) == (wr, wsk) else ""))
        elif wr >= 0 and views[it[1]].valid:
            a = min(it[2], views[it[1]].size)
            assert slot[sk:sk + r] == content(views[it[1]].buf)[a:a + r], it[0]
    assert not bad, "%d of %d ranges differ:\n%s" % (len(bad), len(items), "\n".join(bad[:20]))
