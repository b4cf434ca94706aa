"""Dictionary .lz4 files without a GPU: the model tools/pyref/zig_lz4_file_dict.py against the
plain file model (dict_len 0), against the dictionary frame model member by member, against the codes written by hand in
the corpus and against files written by the `lz4` tool with -D; the refusals of the new calls that need no device, and
the public surface.  Corpus: tests/filedictgen.py."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import pytest

import filedictgen as g
import filerangegen as rg
import legacygen as lg
import zig_lz4_dict_frame as df

fd, ff = g.fd, g.ff
NAMES = ("zlz4f_batch_file_index_using_dict_workspace", "zlz4f_batch_file_index_using_dict",
         "zlz4f_batch_decompress_file_range_using_dict_workspace", "zlz4f_batch_decompress_file_range_using_dict",
         "zlz4f_batch_multiframe_item_dicts", "zlz4f_decompress_file_range_using_dict")
PY_NAMES = ("fileIndexUsingDictBatchWorkspace", "fileIndexUsingDictBatch", "decompressFileRangeUsingDictBatchWorkspace",
            "decompressFileRangeUsingDictBatch", "multiframeItemDictsBatch", "FileDicts", "stageFileDicts")


def test_model_without_a_dictionary_is_the_plain_model():
    """every view and item of filerangegen: index, range result, skip and slot"""
    views = rg.tiny_views() + rg.range_views() + rg.bound_views() + rg.lane_edge_views()
    seen = 0
    for view in views:
        legacy = view.name != "tiny_not_legacy"
        assert fd.file_index(view.buf, 0, legacy) == ff.file_index(view.buf, legacy), view.name
        ranges = rg.all_ranges(view)[::7] if view.size <= 80 else rg.bound_ranges(view)
        for a, b in ranges:
            want = ff.decompress_file_range(view.buf, view.members, view.entries, view.idx_n, a, b)
            assert fd.decompress_file_range(view.buf, view.members, view.entries, view.idx_n, a, b, b"") == want
            seen += 1
    for view, ranges in rg.wrong_index_views():
        for a, b in ranges:
            want = ff.decompress_file_range(view.buf, view.members, view.entries, view.idx_n, a, b)
            assert fd.decompress_file_range(view.buf, view.members, view.entries, view.idx_n, a, b, b"") == want
            seen += 1
    assert seen > 1000
    assert fd.file_range(views[0].buf, 3, 40, b"") == ff.file_range(views[0].buf, 3, 40)


def _by_members(buf, dict_bytes):
    """the content member by member: the dictionary frame model for a frame member, the legacy reader for a legacy one"""
    out = b""
    for pos, ln, kind in ff.split(buf, True):
        body = buf[pos:pos + ln]
        if kind == ff.FRAME:
            r, data = df.decompress_frame_using_dict(body, 1 << 30, dict_bytes)
            assert r >= 0, r
            out += data
        elif kind == ff.LEGACY:
            rd = lg.read(body)
            assert rd.result >= 0
            out += rd.content
    return out


def test_accepted_files_decode_as_their_members_do():
    for view in g.accepted_views() + [g.tiny_view()]:
        assert view.want is None and view.idx_n >= 0, (view.name, view.idx_n)
        data = g.content(view)
        assert len(data) == view.size > 0
        assert data == _by_members(view.buf, view.dict), view.name
    sizes = sorted(len(v.buf) for v in g.accepted_views())
    assert sizes[0] < 1000 and 50000 < sizes[-1] < 100 << 10


def test_twins_answer_as_constructed():
    """the expected code of every refused file is written in the corpus by hand; its accepted twin stands beside it"""
    for view in g.refused_views():
        assert view.idx_n == view.want == g.FAILED, (view.name, view.idx_n)
        assert fd.file_range(view.buf, 0, 10, view.dict)[0] == g.FAILED
    # the twins: the same members with the offset one smaller, the second block self-contained, the block in a frame
    for n in (1, 5, 300):
        assert fd.file_index(g.join(n, "SK", "DI3"), n)[0] == 3
        assert fd.file_index(g.join(n, "SK", "DI3X"), n + 1)[0] == 3          # one more byte of dictionary serves it
    assert fd.file_index(g.join(300, "DL2"), 300)[0] == 2 and fd.file_index(g.join(300, "DL1"), 300)[0] == 1
    assert fd.file_index(g.join(300, "DL1"), 299)[0] == g.FAILED
    assert fd.file_index(g.join(300, "DI3"), 70000)[0] == 3                    # a longer dictionary reaches as far
    # SEES: block 0 of a linked member and every block of an independent one, no block of a legacy member
    v = g.View("sees", g.join(300, "DL2", "DI3", "L3"), g.dic(300))
    pos = [p for p, _ in v.entries[:v.idx_n]]
    assert [fd.sees(v.buf, v.members, p) for p in pos] == [True, False, True, True, True, False, False, False]


def test_tiny_file_every_range():
    view = g.tiny_view()
    data = g.content(view)
    S = len(data)
    assert S == view.size and view.idx_n == 5
    for a, b in g.all_ranges(view)[::3]:
        r, skip, slot = fd.decompress_file_range(view.buf, view.members, view.entries, view.idx_n, a, b, view.dict)
        a1, b1 = min(a, S), min(b, S)
        assert r == b1 - a1 and slot[skip:skip + r] == data[a1:b1], (a, b)


def test_foreign_pairings_are_answered_by_the_decoder():
    for view, ranges in g.foreign_views():
        results = [fd.decompress_file_range(view.buf, view.members, view.entries, view.idx_n, a, b, view.dict)[0]
                   for a, b in ranges]
        if view.name == "index_D65536_read_with_100_bytes":
            # the whole needs the far offsets; five literals are right bytes; a cut in front of the far offset is served
            # from the 100 bytes there are (other bytes than the writer's: a dictionary of another length is another one)
            assert results == [g.FAILED, 5, 12]
        else:                                          # (the other file's blocks stand at the same places and decode to
                                                       # other sizes: the decoder's exact-size check answers)
            assert results[0] == g.FAILED


def test_files_written_by_the_lz4_tool():
    dictionary, cases = g.golden()
    assert len(dictionary) == 70000 and len(cases) >= 8
    for name, buf, content, linked_multiblock in cases:
        assert _by_members(buf, dictionary) == content, name
        n, entries = fd.file_index(buf, len(dictionary))
        if linked_multiblock:                          # linked members with history are not served by the index
            assert n == g.FAILED, name
            continue
        assert n >= 1 and entries[n][1] == len(content), name
        assert fd.file_content(buf, dictionary) == (len(content), content), name
        assert ff.file_index(buf)[0] == g.FAILED, name                          # what the plain index says today
        S = len(content)
        for a, b in ((0, 1), (S // 2, S // 2 + 4096), (65535, 65537), (S - 1, S + 5)):
            r, data = fd.file_range(buf, a, b, dictionary)
            assert data == content[min(a, S):min(b, S)] and r == len(data), (name, a, b)


def test_lz4_tool_agrees_on_the_hand_built_files(tmp_path):
    tool = os.environ.get("LZ4") or shutil.which("lz4") or ("/opt/conda/bin/lz4" if os.path.exists("/opt/conda/bin/lz4") else None)
    if not tool:
        pytest.skip("no lz4 command line tool")
    for k, view in enumerate(g.accepted_views()):
        if not len(view.dict):
            continue
        dpath, fpath, opath = (str(tmp_path / ("%s%d" % (n, k))) for n in ("d", "f", "o"))
        open(dpath, "wb").write(view.dict)
        open(fpath, "wb").write(view.buf)
        subprocess.check_call([tool, "-d", "-f", "-q", "-D", dpath, fpath, opath])
        assert open(opath, "rb").read() == g.content(view), view.name


def test_refusals_without_a_device(zl):
    L = zl.lib()
    totals = (C.c_uint64 * 4)(1, 1, 0, 0)
    huge = (C.c_uint64 * 4)(1 << 33, 1, 0, 0)
    p = C.addressof((C.c_uint8 * 64)())
    assert L.zlz4f_batch_file_index_using_dict(*([None] * 4), 0, *([None] * 10), 0, None, None, 0, None, None, 0) == 0
    assert L.zlz4f_batch_file_index_using_dict(*([None] * 4), 1, *([None] * 10), 8, None, None, 1, None, None, 0) == g.INVALID_STATE
    assert L.zlz4f_batch_file_index_using_dict_workspace(1, huge) == 0
    assert L.zlz4f_batch_file_index_using_dict_workspace(1, None) == 0
    assert L.zlz4f_batch_file_index_using_dict_workspace(3, totals) > L.zlz4f_batch_file_index_workspace(3, totals)
    assert L.zlz4f_batch_decompress_file_range_using_dict(*([None] * 7), 1, *([None] * 9), 0, 0, None, None, None, 0, None, None,
                                                          0) == 0
    assert L.zlz4f_batch_decompress_file_range_using_dict(*([None] * 7), 1, *([None] * 9), 1, 0, None, None, None, 0, None, None,
                                                          0) == g.INVALID_STATE
    assert (L.zlz4f_batch_decompress_file_range_using_dict_workspace(5, 9) >
            L.zlz4f_batch_decompress_file_range_workspace(5, 9))
    assert L.zlz4f_batch_decompress_file_range_using_dict_workspace(5, 0) == L.zlz4f_batch_decompress_file_range_workspace(5, 0)
    assert L.zlz4f_batch_multiframe_item_dicts(None, None, 0, 4, None, None) == 0
    assert L.zlz4f_batch_multiframe_item_dicts(None, None, 2, 4, None, None) == g.INVALID_STATE
    assert L.zlz4f_batch_multiframe_item_dicts(None, p + 1, 2, 4, None, p) == g.INVALID_STATE
    # the host call: flags, then the null checks (the dictionary among them), all before the device check
    f = L.zlz4f_decompress_file_range_using_dict
    assert f(None, 16, 9, 4, None, 16, 2, 1, None, 5) == rg.PARAMETER_INVALID
    assert f(p, 16, 0, 4, p, 16, 1, 2, p, 5) == rg.PARAMETER_INVALID
    assert f(None, 16, 0, 4, p, 16, 1, 1, p, 5) == g.INVALID_STATE
    assert f(p, 16, 0, 4, None, 16, 1, 0, p, 5) == g.INVALID_STATE
    assert f(p, 16, 0, 4, p, 16, 1, 0, None, 5) == g.INVALID_STATE
    assert f(p, 16, 5, 4, p, 16, 1, 1, p, 5) == g.INVALID_STATE
    assert f(p, 16, 5, 4, p, 16, 1, 0, None, 0) == g.INVALID_STATE            # dict_len 0: the _ex call's refusal


def test_public_surface(zl):
    for n in NAMES:
        assert n in zl.SYMBOLS and hasattr(zl.lib(), n), n
    for n in PY_NAMES:
        assert hasattr(zl.lz4f, n), n
    sig = lambda f: list(inspect.signature(f).parameters)                 # noqa: E731
    assert sig(zl.lz4f.fileIndex) == ["buffers", "device", "legacy", "dicts", "dict_index"]
    assert sig(zl.lz4f.indexSplit)[-2:] == sig(zl.lz4f.loadFileIndex)[-2:] == ["dicts", "dict_index"]
    assert sig(zl.lz4f.decompressFilePrefixes)[-2:] == ["dicts", "dict_index"]
    assert sig(zl.lz4f.decompressFileRange) == ["src", "a", "b", "legacy", "seek_table", "dict"]
    assert sig(zl.lz4f.decompressFilesUsingDict) == ["buffers", "dicts", "dict_index", "align", "device"]
    assert sig(zl.lz4f.decodeMultiframes)[-1] == "dicts"
    assert sig(zl.lz4f.compressFiles) == ["items", "prefs", "frame_size", "seek_table", "batch_flags", "device", "dicts",
                                          "dict_index"]
    assert sig(zl.lz4f.appendSeekTables) == ["buffers", "legacy", "device", "dicts", "dict_index"]
    with pytest.raises(ValueError):
        zl.lz4f.compressFiles([b"x"], None, 1 << 20, dicts=[b"abc"])         # linked blocks, frame_size above the block size
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mirror = open(os.path.join(root, "zig-lz4_amd", "csrc", "host", "zlz4.hpp")).read()
    zig = open(os.path.join(root, "zig-lz4_amd", "zig", "root.zig")).read()
    for n in NAMES:
        assert n in mirror and n in zig, n
