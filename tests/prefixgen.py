"""Corpus and batch runner of the prefix-decoding tests (tests/test_prefix_cpu.py, tests/test_gpu_prefix.py).

Every item is (name, stream, cap, dict): `stream` decoded to its first `cap` bytes with the dictionary `dict` (None =
the call without one).  The streams are crafted with dictgen.seq so that every copy path of the single-sequence half of
k_decompress_safe (zig-lz4_amd/csrc/zlz4_decompress.hip) is cut at every byte; what a result must be comes from the model
tools/pyref/zig_lz4_prefix.py, computed once per (stream, cap, dict) and shared (`expected`).

"valid" streams end as the LZ4 block format asks (a last sequence of >= 12 literals without a match), so liblz4 decodes
them; the others end in a match or carry a defect and are compared with the models only.
"""
import functools
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools", "pyref"))
import dictgen  # noqa: E402
import zig_lz4_dict as pd  # noqa: E402
import zig_lz4_prefix as pp  # noqa: E402

seq, pattern = dictgen.seq, dictgen.pattern
TAIL = b"ENDOFBLOCKLITS"                              # 14 literals: a valid last sequence


class _Builder:
    """sequences appended one by one; op is the output position so far (offsets are chosen against it)"""

    def __init__(self, seed):
        self.r = random.Random(seed)
        self.s = bytearray()
        self.op = 0

    def lits(self, n):
        return bytes(self.r.randrange(256) for _ in range(n))

    def add(self, nlit, off=None, ml=None):
        self.s += seq(self.lits(nlit), off, ml)
        self.op += nlit + (ml or 0)
        return self

    def short(self, count):
        """`count` sequences that fit the decoder's batch path: <= 14 literals, matches of 4..18 bytes, no extension bytes,
        sources old enough not to overlap their own output"""
        for _ in range(count):
            nlit, ml = self.r.randrange(0, 9), self.r.randrange(4, 19)
            hi = self.op + nlit
            self.add(nlit, self.r.randrange(ml, hi + 1) if hi >= ml else None, ml if hi >= ml else None)
        return self

    def done(self, tail=True):
        return bytes(self.s) + (seq(TAIL) if tail else b"")


def full_size(stream, dct=None):
    """decoded size by the full-decode model (zig_lz4_dict.decompress_generic), or its error code"""
    return pd.decompress_generic(stream, 1 << 24, 1 << 24, dct)[0]


@functools.lru_cache(maxsize=None)
def exhaustive_streams():
    """-> [(name, stream, valid)]: decoded sizes up to ~1300, each to be cut at every cap in 1 .. S + 1"""
    out = []
    # short sequences only: the batch path, then a fast-path end
    out.append(("short", _Builder(1).add(12, 8, 6).short(80).done(), True))
    out.append(("short2", _Builder(2).add(9, 4, 5).short(60).done(), True))
    # literal runs of 14 (the longest without an extension byte), 15, 16, 64 (the last one stored from the window), 65, 300
    b = _Builder(3)
    for n in (14, 15, 16, 64, 65, 300):
        b.add(n, 7, 8)
    out.append(("litruns", b.done(), True))
    # a disjoint match of 300 bytes
    out.append(("disjoint300", _Builder(4).add(400, 350, 300).done(), True))
    # overlapping matches with offsets 1, 2, 3, 63: short ones (the fast path's 18 lanes) and long ones (the RLE path)
    b = _Builder(5).add(4, 1, 10).add(3, 2, 15).add(5, 3, 18).add(70, 63, 18)
    b.add(70, 1, 100).add(5, 2, 90).add(5, 3, 100).add(70, 63, 200)
    out.append(("rle", b.done(), True))
    # overlapping matches with a period of 64 and of 100 bytes, 1200 long (the period path)
    out.append(("period64", _Builder(6).add(100, 64, 1200).done(), True))
    out.append(("period100", _Builder(7).add(120, 100, 1200).done(), True))
    # a far match (offset >= 1024 overlapping nothing) behind a long literal run, then short sequences again
    out.append(("far", _Builder(8).add(1100, 1050, 40).short(8).done(), True))
    # blocks whose last sequence has no match (every stream above) / is a match (the walk ends at :113)
    out.append(("endsinmatch", _Builder(9).add(20, 10, 30).done(tail=False), False))
    out.append(("endsinmatch_short", _Builder(10).add(12, 8, 6).short(30).done(tail=False), False))
    # literal-only blocks: 100 bytes, one byte
    out.append(("litonly", seq(pattern(100, 11)), True))
    out.append(("onebyte", seq(b"Z"), True))
    return out


@functools.lru_cache(maxsize=None)
def long_stream():
    """-> (name, stream, caps): more than 7200 bytes of short sequences.  With cap - op - 32 >= 7100 the batch walk runs
    without its room test and hands over to the one with it further on, before the cut.  Cut around that threshold and
    at the end of the block (every cap would be 7400 items of up to 7400 bytes)."""
    s = _Builder(20).add(12, 8, 6).short(760).done()
    size = full_size(s)
    assert size > 7300
    caps = sorted(set(list(range(7120, 7150)) + [7200, 7201] + list(range(size - 70, size + 2))))
    return "long", s, caps


DICT = pattern(200, 31)


@functools.lru_cache(maxsize=None)
def dict_streams():
    """-> [(name, stream, p)]: the first match that reaches in front of the output starts in a dictionary of 200 bytes (DICT),
    at output position p (where the literals in front of it end)"""
    lit = pattern(10, 32)
    pre = _Builder(34).add(12, 8, 6).short(40)
    out = [
        ("inside", seq(lit, 10 + 150, 100) + seq(TAIL), 10),                 # dict[50, 150)
        ("to_end", seq(lit, 10 + 100, 100) + seq(TAIL), 10),                 # dict[100, 200)
        ("span", seq(lit, 10 + 50, 58) + seq(TAIL), 10),                     # 50 dictionary bytes, then out[0, 8)
        ("span_self", seq(lit, 10 + 3, 200) + seq(TAIL), 10),                # 3 dictionary bytes, then period 13 over itself
        ("span_self64", seq(pattern(80, 33), 80 + 5, 300) + seq(TAIL), 80),  # ... period 85 (the period path)
        # the same four with matches of <= 18 bytes and no extension byte: the fast path's lanes
        ("inside_s", seq(lit, 10 + 150, 18) + seq(TAIL), 10),
        ("to_end_s", seq(lit, 10 + 12, 12) + seq(TAIL), 10),
        ("span_s", seq(lit, 10 + 9, 16) + seq(TAIL), 10),
        ("span_self_s", seq(lit, 10 + 2, 18) + seq(TAIL), 10),
        # behind a run of batch-path sequences: 9 dictionary bytes, then out[0, 7)
        ("batch_then_span", bytes(pre.s) + seq(lit, pre.op + 10 + 9, 16) + seq(TAIL), pre.op + 10),
    ]
    return out


@functools.lru_cache(maxsize=None)
def dict_variants():
    """-> [(name, dict)]: the full dictionary, none reachable, one shorter than the offsets need, one longer than 64 KiB
    whose tail is DICT (only the tail counts)"""
    return [("d200", DICT), ("d0", b""), ("d20", DICT[-20:]), ("d70000", pattern(70000 - 200, 35) + DICT)]


@functools.lru_cache(maxsize=None)
def malformed_streams():
    """-> [(name, stream, p)]: one defect each, met at output position p (after the literals of its sequence): cap <= p
    cuts in front of it, cap > p meets it.  Each defect comes behind a short valid start and (long_) behind a run of
    batch-path sequences."""
    out = []
    for pname, pre in (("", _Builder(40).add(20, 10, 8)), ("long_", _Builder(41).add(12, 8, 6).short(60))):
        base, op = bytes(pre.s), pre.op
        lit = pattern(6, 42)
        rest = _Builder(43).add(8, 4, 12).short(12).done()             # what follows a defect in the middle of a stream
        out.append((pname + "offset0", base + seq(lit, 0, 8) + rest, op + 6))
        out.append((pname + "offset0_ext", base + seq(lit, 0, 40) + rest, op + 6))
        out.append((pname + "offset_gt_op", base + seq(lit, op + 6 + 300, 8) + rest, op + 6))
        out.append((pname + "offset_gt_op_ext", base + seq(pattern(20, 44), op + 20 + 300, 40) + rest, op + 20))
        # match-length extension bytes that run out (:162), literal-length ones (:125)
        out.append((pname + "ml_ext_runs_out", base + seq(lit, 3, 19 + 255 * 2)[:-1], op + 6))
        out.append((pname + "lit_ext_runs_out", base + bytes([0xF0, 255, 255]), op))
        # literals that pass the end of the input (:136): 12 announced, 5 present; 300 announced, 40 present
        out.append((pname + "lits_pass_end", base + seq(pattern(12, 45))[:6], op))
        out.append((pname + "long_lits_pass_end", base + seq(pattern(300, 46))[:43], op))
        # one offset byte missing (:149)
        out.append((pname + "offset_byte_missing", base + seq(lit, 3, 8)[:-1], op + 6))
    return out


def _cuts(stream):
    """every cap in 1 .. S + 1"""
    return range(1, full_size(stream) + 2)


@functools.lru_cache(maxsize=None)
def plain_items():
    """section 1 of the GPU test: every exhaustive stream at every cap, then the long stream at its caps; no dictionary"""
    items = [(n + "@%d" % c, s, c, None) for n, s, _ in exhaustive_streams() for c in _cuts(s)]
    n, s, caps = long_stream()
    return items + [(n + "@%d" % c, s, c, None) for c in caps]


@functools.lru_cache(maxsize=None)
def valid_items():
    """the items of plain_items() whose stream liblz4 decodes (the block format's end conditions hold)"""
    ok = {s for _, s, v in exhaustive_streams() if v} | {long_stream()[1]}
    return [it for it in plain_items() if it[1] in ok]


@functools.lru_cache(maxsize=None)
def dict_items():
    """section 2: every dictionary stream under every dictionary variant at every cap up to the size it has with the full
    dictionary + 1 (under a shorter dictionary the match is CorruptedData once reached)"""
    items = []
    for sn, s, _ in dict_streams():
        size = full_size(s, DICT)
        assert size > 0, sn
        for dn, d in dict_variants():
            items += [("%s/%s@%d" % (sn, dn, c), s, c, d) for c in range(1, size + 2)]
    big = dict_variants()[3][1]
    far = seq(pattern(10, 36), 65535, 20) + seq(TAIL)                   # the farthest reachable byte of a long dictionary
    return items + [("far/d70000@%d" % c, far, c, big) for c in range(1, 46)]


@functools.lru_cache(maxsize=None)
def malformed_items(with_dict):
    """section 3: every malformed stream at every cap from 1 to 40 bytes behind its defect -- both sides of it, and every
    cut inside the sequence that carries it"""
    d = DICT if with_dict else None
    return [("%s@%d" % (n, c), s, c, d) for n, s, p in malformed_streams() for c in range(1, p + 41)]


@functools.lru_cache(maxsize=None)
def expected(stream, cap, dct):
    return pp.decompress_prefix(stream, cap, dct)


def compare(items, got):
    """results and bytes [0, result) against the model"""
    bad = []
    for (name, s, cap, d), (n, data) in zip(items, got):
        wn, wd = expected(s, cap, d)
        if n != wn or (wn > 0 and data != wd):
            bad.append("%s: GPU %d vs model %d%s" % (name, n, wn, " (bytes differ)" if n == wn else ""))
    assert not bad, "%d of %d items differ:\n%s" % (len(bad), len(items), "\n".join(bad[:20]))


def run_batch(zl, items, dev, use_dict=None, layout=None, call=None):
    """One prefix batch call over `items`: zlz4_batch_decompress_safe_prefix, or _using_dict when any item has a
    dictionary (use_dict overrides).  Distinct streams and dictionaries are stored once; every output slot is exactly cap
    bytes, fenced by a guard band that must stay untouched (gpu_harness), and bytes of the slot behind the result must
    keep their fill.  `call` replaces the library call (the full decoders, for comparison).  -> [(result, bytes)]"""
    import numpy as np
    import torch
    import gpu_harness as gh
    if use_dict is None:
        use_dict = any(it[3] is not None for it in items)
    streams, sidx, dicts, didx = [], {}, [], {}
    for _, s, _, d in items:
        if s not in sidx:
            sidx[s] = len(streams); streams.append(s)
        d = d or b""
        if d not in didx:
            didx[d] = len(dicts); dicts.append(d)
    buf, offs, lens = gh._pack(streams, layout=layout)
    dbuf, doffs, dlens = gh._pack(dicts, layout=layout)
    si = np.array([sidx[it[1]] for it in items], dtype=np.int64)
    di = np.array([didx[it[3] or b""] for it in items], dtype=np.int64)
    caps = np.array([it[2] for it in items], dtype=np.int64)
    out_offs, guard_ends, total = gh._out_slots(caps, layout)
    u32 = lambda a: torch.from_numpy(np.asarray(a).astype(np.uint32).view(np.int32)).to(dev)
    d_in, d_dict = torch.from_numpy(buf).to(dev), torch.from_numpy(dbuf).to(dev)
    d_out = torch.full((total,), 0xA5, dtype=torch.uint8, device=dev)
    res = torch.full((len(items),), -999, dtype=torch.int64, device=dev)
    a = (d_in, torch.from_numpy(offs[si]).to(dev), u32(lens[si]), d_out, torch.from_numpy(out_offs).to(dev), u32(caps))
    if use_dict:
        (call or zl.batch_decompress_safe_prefix_using_dict)(*a, d_dict, torch.from_numpy(doffs[di]).to(dev), u32(dlens[di]), res)
    else:
        (call or zl.batch_decompress_safe_prefix)(*a, res)
    torch.cuda.synchronize()
    assert (d_in.cpu().numpy() == buf).all(), "the input arena changed"
    assert (d_dict.cpu().numpy() == dbuf).all(), "the dictionary arena changed"
    got = gh._collect(res, d_out, out_offs, guard_ends, caps)
    o = d_out.cpu().numpy()
    for i, (n, _) in enumerate(got):
        if 0 <= n < caps[i]:
            assert (o[out_offs[i] + n: out_offs[i] + caps[i]] == 0xA5).all(), "%s wrote behind its result" % items[i][0]
    return got
