"""The file index and file range decoding without a GPU: the model
tools/pyref/zig_lz4_file_range.py against lz4filegen.expected sliced [a:b], its index of a one-frame file against the frame
range model's, results stated by hand for three files, the refusals of the new calls that need no device, and the public
surface.  Corpus: tests/filerangegen.py."""
import ctypes as C
import os

import filerangegen as g
import legacygen as lg
import lz4filegen as fg

ff, fr = g.ff, g.frg.fr
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("zlz4f_batch_file_index_workspace", "zlz4f_batch_file_index", "zlz4f_batch_decompress_file_range_workspace",
         "zlz4f_batch_decompress_file_range", "zlz4f_decompress_file_range")
PY_NAMES = ("fileIndexBatchWorkspace", "fileIndexBatch", "decompressFileRangeBatchWorkspace", "decompressFileRangeBatch",
            "FileIndex", "fileIndex", "decompressFileRanges", "decompressFileRange", "decompressFilePrefixes")


def test_model_split_is_the_file_models_split():
    bufs = [v.buf for v in g.tiny_views() + g.range_views() + g.lane_edge_views()] + g.orderings()[::997]
    for buf in bufs:
        for legacy in (True, False):
            assert ff.split(buf, legacy) == [(m.pos, m.len, m.kind) for m in fg.split(buf, legacy)]


def test_model_bytes_are_the_file_decode_sliced():
    """every (a, b) of every small file: the result is b' - a', the wanted bytes are [a, b) of what the file model decodes,
    the slot starts on a block boundary"""
    seen = 0
    for view in g.tiny_views():
        legacy = view.name != "tiny_not_legacy"
        data = g.content(view.buf, legacy)
        S = len(data)
        assert view.idx_n >= 0 and view.size == S <= 80, view.name
        for a, b in g.all_ranges(view):
            r, skip, slot = ff.decompress_file_range(view.buf, view.members, view.entries, view.idx_n, a, b)
            a1, b1 = min(a, S), min(b, S)
            assert r == b1 - a1 and slot[skip:skip + r] == data[a1:b1], (view.name, a, b)
            assert a1 == b1 or a1 - skip in view.bounds, (view.name, a, b)
            assert len(slot) == ff.plan_range(view.entries, view.idx_n, a, b)[0]
            if seen % 16 == 0:                        # the host call's form: the index built anew, exactly [a', b')
                assert ff.file_range(view.buf, a, b, legacy) == (r, data[a1:b1]), (view.name, a, b)
            seen += 1
    assert seen > 4000
    for view in g.range_views() + g.lane_edge_views():
        data = g.content(view.buf)
        assert view.size == len(data)
        for a, b in g.frg.small_ranges(view, every_a=False)[::23]:
            r, skip, slot = ff.decompress_file_range(view.buf, view.members, view.entries, view.idx_n, a, b)
            assert slot[skip:skip + r] == data[a:b], (view.name, a, b)


def test_index_of_a_one_frame_file_is_the_frame_index():
    frames = [g.members()[k] for k in ("F", "FC", "FS", "FE")] + [v.frame for v in g.frg.small_views() + g.frg.long_views()[:1]]
    frames += [v.frame for v, _ in g.frg.header_views()[:6]] + [g.frg.linked_views()[0].frame]
    for f in frames:
        if not len(f):                                 # (no byte is no member: a file of nothing, S = 0)
            continue
        assert ff.file_index(f) == fr.frame_index(f)
        assert ff.file_index(f, legacy=False) == fr.frame_index(f)
    assert ff.file_index(g.frg.linked_views()[0].frame)[0] == g.FAILED       # a linked member with history


def test_every_ordering_has_the_same_blocks():
    """the corpus of the GPU index test: 8! files of the same 13 blocks, 8 members each"""
    files = g.orderings()
    assert len(files) == 40320 and len(set(files)) == 40320
    m = g.members()
    assert m["FC"][4] & 0x1C == 0x1C and len(m["FE"]) == 11           # block checksums, content size, content checksum
    assert [m["FS"][p + 3] >> 7 for p, _ in ff.file_index(m["FS"])[1][:3]] == [0, 1, 0]      # the stored block
    for buf in files[::1009]:
        n, e = ff.file_index(buf)
        assert n == 13 and e[-1][1] == len(g.content(buf)) == 64 + 62 + 44 + 250 + 243 + len(lg.small_blocks(3, 5)[1]) + 47
        assert [k for _, _, k in ff.split(buf)].count(ff.LEGACY) == 3


def test_results_stated_by_hand():
    tiny = {v.name: v for v in g.tiny_views()}
    tf = tiny["tiny_one_frame"].buf                    # header 7, blocks of 8 / 5 (stored) / 10 bytes, end mark at 42
    tl = lg.build([lg.literal_block(b"abcdef"), lg.EMPTY, lg.literal_block(b"ghi")])
    sk = g.members()["SK"]
    assert (len(tf), len(tl), len(sk)) == (46, 28, 18)
    # 1. a frame, then a legacy frame with a block of 0 bytes
    one = tf + tl
    assert ff.file_index(one) == (6, [(7, 0), (19, 7), (28, 12), (50, 21), (61, 27), (66, 27), (74, 30)])
    assert ff.split(one) == [(0, 46, ff.FRAME), (46, 28, ff.LEGACY)]
    data = g.content(one)
    n, e = ff.file_index(one)
    assert ff.decompress_file_range(one, ff.split(one), e, n, 5, 25) == (20, 5, data[:25])
    assert ff.decompress_file_range(one, ff.split(one), e, n, 27, 29) == (2, 0, b"gh")       # the empty block holds no byte
    assert ff.decompress_file_range(one, ff.split(one), e, n, 30, 40) == (0, 0, b"")
    assert ff.decompress_file_range(one, ff.split(one), e, n, 9, 8) == (g.INVALID_STATE, 0, b"")
    assert ff.plan_range(e, n, 5, 25) == (25, 4) and ff.plan_range(e, n, 20, 22) == (10, 2)
    # 2. skippable frames around a frame: positions count from the file's first byte
    two = sk + tf + sk
    assert ff.file_index(two) == (3, [(25, 0), (37, 7), (46, 12), (60, 21)])
    # 3. no block at all: the magic alone, a skippable frame, the empty frame -- entry 0 stands on its end mark
    three = g.MAGIC + sk + g.members()["FE"]
    assert ff.file_index(three) == (0, [(29, 0)]) and ff.file_range(three, 0, 10) == (0, b"")
    assert ff.file_index(three, legacy=False)[0] == lg.TYPE_UNKNOWN
    assert ff.file_index(b"") == (0, [(0, 0)])
    # defects: the first member that is not OK decides
    assert ff.file_index(tf + sk[:6])[0] == lg.HEADER_INCOMPLETE and ff.file_index(tf + sk[:-1])[0] == lg.SIZE_WRONG
    assert ff.file_index(tl + b"\x07")[0] == lg.SIZE_WRONG and ff.file_index(lg.build([lg.CORRUPT]) + b"\x07")[0] == lg.FAILED
    assert ff.file_index(one, idx_cap=6)[0] == g.DST_TOO_SMALL and ff.file_index(one, idx_cap=7)[0] == 6
    # a wrong index: block 3's position moved into the frame in front of it; a dec step that is wrong but in bound
    wrong = list(e)
    wrong[3] = (40, 21)
    assert ff.decompress_file_range(one, ff.split(one), wrong, n, 22, 24)[0] == g.INVALID_STATE
    assert ff.decompress_file_range(one, ff.split(one), wrong, n, 0, 12)[0] == 12
    wrong = [(p, d + (1 if k >= 4 else 0)) for k, (p, d) in enumerate(e)]
    assert ff.decompress_file_range(one, ff.split(one), wrong, n, 21, 28)[0] == g.FAILED


def test_wrong_index_cases_are_wrong():
    """every case of the GPU test's wrong-index table gives INVALID_STATE or DECOMPRESSION_FAILED for each of its ranges"""
    for view, ranges in g.wrong_index_views():
        for a, b in ranges:
            r = ff.decompress_file_range(view.buf, view.members, view.entries, view.idx_n, a, b)[0]
            assert r in (g.INVALID_STATE, g.FAILED), (view.name, a, b, r)


def test_host_call_refusals_need_no_device(zl):
    L = zl.lib()
    src = (C.c_uint8 * 16)()
    dst = (C.c_uint8 * 16)()
    s, d = C.addressof(src), C.addressof(dst)
    assert L.zlz4f_decompress_file_range(s, 16, 0, 4, d, 16, 2) == g.PARAMETER_INVALID
    assert L.zlz4f_decompress_file_range(None, 0, 9, 4, None, 0, 6) == g.PARAMETER_INVALID      # in front of a > b
    assert L.zlz4f_decompress_file_range(None, 16, 0, 4, d, 16, 1) == g.INVALID_STATE
    assert L.zlz4f_decompress_file_range(s, 16, 0, 4, None, 16, 0) == g.INVALID_STATE
    assert L.zlz4f_decompress_file_range(s, 16, 5, 4, d, 16, 1) == g.INVALID_STATE
    # the batch calls: nothing to do, then null arrays and totals that are none, all in front of the device check
    totals = (C.c_uint64 * 4)(1, 1, 0, 0)
    huge = (C.c_uint64 * 4)(1 << 32, 1, 0, 0)
    assert L.zlz4f_batch_file_index(*([None] * 4), 0, *([None] * 10), 0, None, None, 0) == 0
    assert L.zlz4f_batch_file_index(*([None] * 4), 1, *([None] * 7), totals, None, None, 8, None, None, 0) == g.INVALID_STATE
    assert L.zlz4f_batch_file_index(*([None] * 4), 1, *([None] * 10), 8, None, None, 0) == g.INVALID_STATE
    assert L.zlz4f_batch_file_index_workspace(1, huge) == 0 and L.zlz4f_batch_file_index_workspace(1, None) == 0
    assert L.zlz4f_batch_file_index_workspace(3, totals) >= L.zlz4f_batch_frame_index_workspace(1, 1)
    assert L.zlz4f_batch_decompress_file_range(*([None] * 7), 1, *([None] * 9), 0, 0, None, 0) == 0
    assert L.zlz4f_batch_decompress_file_range(*([None] * 7), 1, *([None] * 9), 1, 0, None, 0) == g.INVALID_STATE
    assert L.zlz4f_batch_decompress_file_range_workspace(5, 9) == L.zlz4f_batch_decompress_frame_range_workspace(5, 9)


def test_public_surface_names_the_new_calls(zl):
    def text(*p):
        return open(os.path.join(ROOT, *p)).read()

    header, mirror, zig = text("include", "zlz4_amd.h"), text("zig-lz4_amd", "csrc", "host", "zlz4.hpp"), text("zig-lz4_amd", "zig", "root.zig")
    for name in NAMES:
        assert name in header and name in zl.SYMBOLS and hasattr(zl.lib(), name), name
        assert name in zig and name in mirror and name in text("INTEGRATION.md"), name
    for name in PY_NAMES:
        assert hasattr(zl.lz4f, name), name
    for name in ("fileIndexBatch", "decompressFileRangeBatch", "decompressFileRange("):
        assert name in mirror and name in zig, name
    for name in ("lz4f.fileIndex(", "lz4f.decompressFileRanges(", "lz4f.decompressFileRange(", "lz4f.decompressFilePrefixes("):
        assert name in text("INTEGRATION.md"), name
    assert "4.4k" in text("DESIGN.md") and "decompressFileRanges" in text("README.md")
