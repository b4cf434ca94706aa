"""Corpus and batch runners for dictionary .lz4 files (tests/test_file_dict_cpu.py, tests/test_gpu_file_dict.py; DESIGN.md
section 4.4m).  Test infrastructure in the style of filerangegen: members are hand-built with the existing generators
(framerangegen / linkedgen.build_frame, dictgen.seq, legacygen), their blocks from sequences whose offsets are chosen
against the dictionary's tail T; expectations come from tools/pyref/zig_lz4_file_dict.py and, for every accept / refuse
twin, from the code written here by hand (View.want).

A View is a file, the dictionary it is READ with, and AN index (entries, idx_n): both are the caller's data, so a view may
pair a file with an index or a dictionary that is not its own.  An Item is one range of one view, as in filerangegen:
(name, view, a, b, reserved, cap_delta, buf_override).
"""
import functools
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools", "pyref"))
import filerangegen as frg2  # noqa: E402
import framerangegen as frg  # noqa: E402
import legacygen as lg  # noqa: E402
import zig_lz4_file_dict as fd  # noqa: E402
import zig_lz4_file_range as ff  # noqa: E402

seq, pat, build, c = frg.seq, frg.pat, frg.build, frg.c
INVALID_STATE, DST_TOO_SMALL, FAILED = -5, -111, -116
BIG = 1 << 63
DICT_LENS = (0, 1, 5, 65535, 65536, 65537, 70000)
_BASE = pat(70000, 4242)


def dic(n):
    """the dictionary of n bytes (the first n of one base, so the tails of two lengths differ)"""
    return _BASE[:n]


# ----------------------------------------------------------------------------- blocks against T
def dblock(D, seed, beyond=0):
    """A block for a dictionary tail of D >= 1 bytes.  Sequence 1: 8 literals, then a match that STARTS IN T, m = min(D, 20)
    bytes in front of its end, runs across the end into the block's own 8 literals and over itself (length m + 14).
    Sequence 2: 5 literals, then a match of 4 at offset op + D exactly -- the first byte of T -- where 16 bits can say so
    (else 65535); `beyond` is added to that offset: 1 gives the twin that reaches one byte in front of T.  Then 9 literals."""
    m = min(D, 20)
    s1 = seq(pat(8, seed), 8 + m, m + 14)
    op = 8 + m + 14 + 5
    s2 = seq(pat(5, seed + 1), min(op + D, 65535) + beyond, 4)
    return s1 + s2 + seq(frg.TAIL)


DBLOCK_CUT = 8 + 3                                     # a content offset inside the match that comes from T


def big_block(D, seed):
    """a block of 60 000 literals and a far match into T (for the file of some 60 KiB)"""
    return seq(pat(60000, seed), min(60000 + D, 65535), 40) + seq(frg.TAIL)


@functools.lru_cache(maxsize=None)
def members(D):
    """the members whose blocks are written against a tail of D bytes -> dict (D == 0: offsets that reach in front of the
    block, which nothing serves)"""
    d = max(D, 1)
    m = dict(frg2.members())
    m.update(
        DI3=build([(dblock(d, 10), False), (dblock(d, 20), False), (dblock(d, 30), False)], block_mode=1),
        DIC=build([(dblock(d, 40), False), (pat(21, 41), True), (dblock(d, 42), False)], True, None, block_mode=1),
        DL1=build([(dblock(d, 50), False)], block_mode=0),                         # linked, one block: T is its history
        DL2=build([(dblock(d, 60), False), (c(60, 61), False)], block_mode=0),     # the second block is self-contained
        DL2T=build([(dblock(d, 70), False), (dblock(d, 71), False)], block_mode=0),              # the second refers to T
        DL2H=build([(dblock(d, 80), False), (seq(pat(6, 81), 6 + 3, 5) + seq(frg.TAIL), False)], block_mode=0),   # to block 0
        LEGT=lg.build([dblock(d, 90)]),                                            # a legacy block that needs T
        BIG=build([(big_block(d, 95), False)], block_mode=1),
    )
    if d < 60000:                                      # (16 bits cannot say an offset one past a tail of 64 KiB)
        m["DI3X"] = build([(dblock(d, 10), False), (dblock(d, 20, beyond=1), False), (dblock(d, 30), False)], block_mode=1)
    return m


def join(D, *names):
    m = members(D)
    return b"".join(m[n] for n in names)


class View:
    __slots__ = ("name", "buf", "dict", "entries", "idx_n", "valid", "members", "want")

    def __init__(self, name, buf, dict_bytes, index=None, valid=True, want=None, index_dict_len=None):
        """want: the index result written by hand -- None = accepted, else the code; index_dict_len: the length the index
        is built with (None: the dictionary's own)"""
        self.name, self.buf, self.dict, self.valid, self.want = name, bytes(buf), bytes(dict_bytes), valid, want
        dl = len(self.dict) if index_dict_len is None else index_dict_len
        self.idx_n, self.entries = fd.file_index(self.buf, dl) if index is None else index
        self.members = ff.split(self.buf, True)

    @property
    def size(self):
        return self.entries[self.idx_n][1] if self.idx_n >= 0 else 0

    @property
    def bounds(self):
        return [e[1] for e in self.entries] if self.idx_n >= 0 else []


MIXED = ("SK", "DI3", "L3", "DL1", "FE", "DIC", "FS", "DL2", "FC")


@functools.lru_cache(maxsize=None)
def accepted_views():
    """one file of every kind of member -- dictionary frames beside a legacy member, a skippable one, the empty frame,
    stored blocks, block checksums -- per dictionary length >= 1, a file of some 60 KiB, and the plain members under
    a dictionary of 0 bytes"""
    out = [View("mixed_D%d" % n, join(min(n, 65536), *MIXED), dic(n)) for n in DICT_LENS if n]
    out.append(View("big_D65536", join(65536, "BIG", "DI3"), dic(65536)))
    out.append(View("plain_D0", frg2.join("F", "FC", "L3", "FS"), dic(0)))
    out.append(View("linked_one_block_D5", join(5, "DL1"), dic(5)))
    out.append(View("linked_two_blocks_D300", join(300, "DL2"), dic(300)))
    return out


@functools.lru_cache(maxsize=None)
def refused_views():
    """the refuse twins; every code is written here by hand"""
    out = []
    for n in (1, 5, 300):
        out.append(View("offset_one_past_T_D%d" % n, join(n, "SK", "DI3X"), dic(n), want=FAILED))
    out += [View("linked_second_block_refers_to_T", join(300, "DL2T"), dic(300), want=FAILED),
            View("linked_second_block_refers_to_block0", join(300, "DL2H"), dic(300), want=FAILED),
            View("legacy_block_needs_T", join(300, "DI3", "LEGT"), dic(300), want=FAILED),
            View("dictionary_frame_without_dictionary", join(300, "DI3"), dic(0), want=FAILED),
            View("dictionary_too_short", join(300, "DI3"), dic(299), want=FAILED)]
    return out


@functools.lru_cache(maxsize=None)
def tiny_view():
    """a file whose content is 100-odd bytes, for every (a, b): an independent and a linked dictionary member round a
    tiny legacy one"""
    tl = lg.build([lg.literal_block(b"abcdef"), lg.EMPTY, lg.literal_block(b"ghi")])
    m = members(5)
    one = build([(dblock(5, 10), False)], block_mode=1)
    return View("tiny_D5", one + tl + m["DL1"], dic(5))


@functools.lru_cache(maxsize=None)
def foreign_views():
    """pairings that are not the file's own -> [(View, ranges)]: the decoder, not the index, is the judge"""
    buf = join(65536, *MIXED)
    own = fd.file_index(buf, 65536)
    other = fd.file_index(join(5, *MIXED), 5)
    plain = ff.file_index(buf)
    assert own[0] > 0 and other[0] > 0 and plain[0] == FAILED
    whole = (0, BIG)
    d1 = own[1][1][1]
    return [(View("index_D65536_read_with_100_bytes", buf, dic(100), own, valid=False), [whole, (0, 5), (d1, d1 + 12)]),
            (View("index_of_another_file", buf, dic(65536), other, valid=False), [whole, (0, 5), (40, 60)]),
            (View("plain_index_of_the_same_file", buf, dic(65536), plain, valid=False), [whole, (0, 5)]),
            (View("own_index_without_dictionary", buf, dic(0), own, valid=False), [whole, (0, 5)])]


def all_ranges(view):
    S = view.size
    return [(a, b) for a in range(S + 2) for b in list(range(a, S + 2)) + [BIG]]


def edge_ranges(view):
    """cuts one byte either side of every block and member boundary, a cut inside a match that comes from T, the whole"""
    S, out = view.size, [(0, BIG), (0, view.size)]
    for d in view.bounds:
        out += [(max(0, d - 1), min(S, d + 1)), (d, min(S, d + 1)), (max(0, d - 1), d), (d, min(S, d + DBLOCK_CUT)),
                (max(0, d - 40), min(S, d + DBLOCK_CUT + 2))]
    return sorted(set(out))


# ----------------------------------------------------------------------------- files written by the lz4 tool
@functools.lru_cache(maxsize=None)
def golden():
    """tests/golden/dict_files.json (written by tests/golden/gen_dict_files.py with `lz4 -D`) -> (dictionary, [(name, file,
    content, linked_multiblock)]); every content is checked against its SHA-256 here"""
    import base64
    import hashlib
    import json
    import zlib
    j = json.load(open(os.path.join(HERE, "golden", "dict_files.json")))
    unz = lambda s: zlib.decompress(base64.b64decode(s))                  # noqa: E731
    dictionary = unz(j["dictionary"])
    assert hashlib.sha256(dictionary).hexdigest() == j["dictionary_sha256"]
    contents = {}
    for k, rec in j["contents"].items():
        contents[k] = unz(rec["zlib"])
        assert len(contents[k]) == rec["size"] and hashlib.sha256(contents[k]).hexdigest() == rec["sha256"], k
    files = {k: base64.b64decode(v) for k, v in j["files"].items()}
    cases = [(cs["name"], b"".join(files[p] for p in cs["parts"]), b"".join(contents[p] for p in cs["contents"]),
              cs["linked_multiblock"]) for cs in j["cases"]]
    return dictionary, cases


# ----------------------------------------------------------------------------- the model over a batch
def items_of(views, ranges_of):
    items = []
    for v, view in enumerate(views):
        for a, b in ranges_of(view):
            items.append(("%s[%d,%d)" % (view.name, a, min(b, 1 << 40)), v, a, b, 0, None, None))
    return list(views), items


def _need(view, a, b):
    return ff.plan_range(view.entries, view.idx_n, a, b)


def expect(views, items, max_items=None, no_dict=()):
    """the model over one batch -> [(result, skip, slot bytes)]; no_dict: the views whose file names no dictionary"""
    out, base = [], 0
    for name, v, a, b, reserved, cap_delta, buf_over in items:
        view = views[v]
        need = _need(view, a, b)[0]
        cap = need if cap_delta is None else max(0, need + cap_delta)
        ok = buf_over is None
        n = 0 if v in no_dict else ff.range_items(view.buf, view.members, view.entries, view.idx_n, a, b, cap, reserved, ok)
        fits = max_items is None or n == 0 or base + n <= max_items
        base += n
        out.append(fd.decompress_file_range(view.buf, view.members, view.entries, view.idx_n, a, b, view.dict, cap, reserved,
                                            ok, fits, dict_ok=v not in no_dict))
    return out


@functools.lru_cache(maxsize=None)
def content(view):
    """the whole content of an accepted view under the model"""
    r, data = fd.file_content(view.buf, view.dict)
    assert r >= 0, (view.name, r)
    return data


# ----------------------------------------------------------------------------- the GPU side
def dict_table(views, extra=()):
    """the distinct dictionaries of the views (and `extra`) -> (list of bytes, per-view index)"""
    table, idx = [], []
    for d in [v.dict for v in views] + list(extra):
        if d not in table:
            table.append(d)
    for v in views:
        idx.append(table.index(v.dict))
    return table, idx


def stage(zl, bufs, dev, lead=0):
    """the files in one arena with `lead` bytes in front and an odd gap between them -> the record-mode split"""
    import numpy as np
    import torch
    parts, offs, pos = [b"\xEE" * lead], [], lead
    for k, b in enumerate(bufs):
        offs.append(pos)
        gap = b"\xEE" * (1 + k % 3) if lead else b""
        parts += [bytes(b), gap]
        pos += len(b) + len(gap)
    arena = np.frombuffer(b"".join(parts) or b"\0", dtype=np.uint8).copy()
    t = lambda x: torch.tensor(x, dtype=torch.int64, device=dev)          # noqa: E731
    return zl.lz4f.splitStaged(torch.from_numpy(arena).to(dev), t(offs), t([len(b) for b in bufs]), legacy=True)


def gpu_index(zl, sp, dev, dict_lens, dict_idx, idx_cap=None):
    """zlz4f_batch_file_index_using_dict over a split -> (results, idx_off, rows)"""
    import torch
    nbuf = sp.src_len.numel()
    cap = sp.max_blocks + sp.legacy_blocks + nbuf
    index = torch.full((max(1, cap), 2), -7, dtype=torch.int64, device=dev)
    idx_off = torch.zeros(nbuf + 1, dtype=torch.int64, device=dev)
    idx_n = torch.full((nbuf,), -999, dtype=torch.int64, device=dev)
    dl = torch.tensor(list(dict_lens), dtype=torch.int32, device=dev)
    di = None if dict_idx is None else torch.tensor(list(dict_idx), dtype=torch.int32, device=dev)
    zl.lz4f.fileIndexUsingDictBatch(sp.d_src, sp.src_off, sp.src_len, sp.member, sp.mem_off, sp.result, sp.item_first,
                                    sp.item_off, sp.item_len, sp.leg_len,
                                    (sp.nitems, sp.max_blocks, sp.nlegacy, sp.legacy_blocks), index, idx_off, idx_n, dl, di,
                                    cap if idx_cap is None else idx_cap)
    torch.cuda.synchronize()
    return idx_n.cpu().tolist(), idx_off.cpu().tolist(), [tuple(r) for r in index.cpu().tolist()]


def run(zl, views, items, dev, max_items=None, lead=0, plain=False, no_dict=()):
    """one zlz4f_batch_decompress_file_range_using_dict call (plain: the plain call) over the GPU split of the views' files
    and the VIEWS' indexes and dictionaries -> [(result, skip, slot bytes[0, planned size))]; the source arena and the
    dictionaries are unchanged and every guard band is intact.  no_dict: the views that get a dictionary index past the
    table."""
    import numpy as np
    import torch
    import gpu_harness as gh
    sp = stage(zl, [v.buf for v in views], dev, lead)
    before = sp.d_src.clone()
    table, didx = dict_table(views)
    didx = [len(table) + 3 if v in no_dict else k for v, k in enumerate(didx)]
    fdicts = zl.lz4f.stageFileDicts(table, didx, dev)
    dict_before = fdicts.d_dict.clone()
    ents, idx_off = [], []
    for v in views:
        idx_off.append(len(ents))
        ents += list(v.entries) + [(0, 0), (0, 0)]
    index = np.array(ents or [(0, 0)], dtype=np.uint64).reshape(-1, 2)
    rng = np.zeros((max(1, len(items)), 3), dtype=np.uint64)
    caps, planned = [], 0
    for i, (name, v, a, b, reserved, cap_delta, buf_over) in enumerate(items):
        rng[i] = ((v if buf_over is None else buf_over) | (reserved << 32), a, b)
        need, n = _need(views[v], a, b)
        planned += n
        caps.append(need if cap_delta is None else max(0, need + cap_delta))
    caps = np.array(caps, dtype=np.int64)
    out_offs, guard_ends, total = gh._out_slots(caps)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)       # noqa: E731
    d_dst = torch.full((total,), 0xA5, dtype=torch.uint8, device=dev)
    skip = torch.full((len(items),), -999, dtype=torch.int64, device=dev)
    result = torch.full((len(items),), -999, dtype=torch.int64, device=dev)
    idx_n = t(np.array([v.idx_n for v in views], dtype=np.int64))
    args = (sp.d_src, sp.src_off, sp.src_len, t(index.view(np.int64)), t(np.array(idx_off, dtype=np.int64)), idx_n, sp.member,
            sp.mem_off, sp.result, t(rng.view(np.int64))[:len(items)], d_dst, t(out_offs), t(caps), skip, result,
            planned if max_items is None else max_items)
    if plain:
        zl.lz4f.decompressFileRangeBatch(*args)
    else:
        zl.lz4f.decompressFileRangeUsingDictBatch(*args, fdicts.d_dict, fdicts.dict_off, fdicts.dict_len, fdicts.idx)
    torch.cuda.synchronize()
    assert torch.equal(sp.d_src, before), "the source arena changed"
    assert torch.equal(fdicts.d_dict, dict_before), "a dictionary changed"
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
            assert slot[sk:sk + r] == content(views[it[1]])[a:a + r], it[0]
    assert not bad, "%d of %d ranges differ:\n%s" % (len(bad), len(items), "\n".join(bad[:20]))
