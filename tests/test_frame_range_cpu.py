"""The frame index and frame range decoding without a GPU: the model
tools/pyref/zig_lz4_frame_range.py against liblz4's full LZ4F_decompress and the full-frame model sliced [a:b], its index
against the size-query model, the plan invariants, the results stated by hand for the defect, header and wrong-index cases,
and the refusals of the three batch calls that need no device.  Corpus: tests/framerangegen.py."""
import ctypes as C
import os
import re

import pytest

import framerangegen as g
import linkedgen

fr, zs = g.fr, g.zs
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("zlz4f_batch_frame_index_workspace", "zlz4f_batch_frame_index", "zlz4f_batch_plan_frame_ranges",
         "zlz4f_batch_decompress_frame_range_workspace", "zlz4f_batch_decompress_frame_range", "zlz4f_decompress_frame_range")


def _valid_views():
    return [v for v in g.small_views() + g.long_views() if v.valid] + [v for v, _ in g.defect_views() if v.valid]


def _ranges(view):
    return g.small_ranges(view) if view.family == "small" else g.long_ranges(view) if view.family == "long" else \
        g.small_ranges(view, every_a=False)


def test_the_corpus_is_what_the_gpu_test_needs():
    small, long_ = g.small_views(), g.long_views()
    assert all(v.size <= 3072 and 0 <= v.idx_n <= 6 for v in small)
    five = small[0]
    assert [b - a for a, b in zip(five.bounds, five.bounds[1:])] == [300, 17, 1100, 0, 40]   # unequal, short, one empty
    assert {v.frame[4] & 0x34 for v in small} >= {0x20, 0x34, 0x00}       # independent, with checksums, linked-declared
    assert [v.size for v in small if v.name.startswith("empty")] == [0, 0]
    stored = small[1]
    words = [int.from_bytes(stored.frame[p:p + 4], "little") for p, _ in stored.entries[:-1]]
    assert [w >> 31 for w in words] == [0, 1, 0, 1, 0, 1] and words[3] == 0x80000000       # a stored block of 0 bytes
    sizes = {v.name: [b - a for a, b in zip(v.bounds, v.bounds[1:])] for v in long_}
    assert sizes["three_64k_and_short"] == [65536] * 3 + [1000] and sizes["two_256k"] == [262144] * 2
    assert sizes["bs4m_short_blocks"] == [5000, 70000, 100, 100] and long_[3].frame[5] >> 4 == 7
    assert len(g.items_of(small, g.small_ranges)[1]) > 50000
    lv = {v.name: v for v in g.linked_views()}
    assert lv["linked_ref"].idx_n == g.FAILED and lv["linked_ref_history_index"].idx_n == 2
    assert any(v.name.startswith("fx_") and v.idx_n > 1 for v in lv.values())


def test_model_bytes_are_the_full_decode_sliced():
    """every valid frame and range: the result is b' - a', the wanted bytes are [a, b) of the full-frame model's output, the
    slot starts on a block boundary; and the full-frame model's output is liblz4's (checked once per frame below)"""
    seen = 0
    for view in _valid_views():
        S, data = g.full(view.frame)
        assert S == view.size == zs.frame_size(view.frame), view.name
        for a, b in _ranges(view):
            r, skip, slot = fr.decompress_frame_range(view.frame, view.entries, view.idx_n, a, b)
            a1, b1 = min(a, S), min(b, S)
            assert r == b1 - a1 and slot[skip:skip + r] == data[a1:b1], (view.name, a, b)
            if seen % 64 == 0:                        # the host call's form: the index built anew, exactly [a', b')
                assert fr.frame_range(view.frame, a, b) == (r, data[a1:b1]), (view.name, a, b)
            if r:
                assert a1 - skip in view.bounds and slot == data[a1 - skip:b1], (view.name, a, b)
            seen += 1
    assert seen > 50000


def test_full_decode_is_liblz4s():
    lib = linkedgen.liblz4f()
    if lib is None:
        pytest.skip("liblz4 does not load")
    for view in _valid_views() + [v for v in g.linked_views() if v.idx_n >= 0]:
        if "no_end_mark" in view.name:                # (the reference's decoder takes the end of the input; liblz4 does not)
            continue
        S, data = g.full(view.frame)
        assert lib.decompress(view.frame, S + 64) == data, view.name


def test_index_against_the_size_query_model():
    """dec[nb] is the size query's answer, errors are its errors, the pos chain re-walks the frame, dec is the running sum"""
    views = g.small_views() + g.long_views() + g.linked_views() + [v for v, _ in g.header_views()]
    frames = {v.frame for v in views} | {v.frame for v, _ in g.defect_views()}
    frames |= {fp_case[0].frame for fp_case in g.frameprefixgen.defect_cases()}
    errors = set()
    for f in frames:
        n, ent = fr.frame_index(f)
        q = zs.frame_size(f)
        if q < 0:
            assert (n, ent) == (q, []), f[:16]
            errors.add(q)
            continue
        assert n >= 0 and len(ent) == n + 1 and ent[n][1] == q
        flg, pos = zs._parse_header(f)
        assert ent[0] == (pos, 0)
        for k in range(n):
            w = int.from_bytes(f[pos:pos + 4], "little")
            assert w != 0 and ent[k][0] == pos
            pos += 4 + (w & 0x7FFFFFFF) + (4 if flg & 0x10 else 0)
            assert ent[k + 1][1] >= ent[k][1]
        assert ent[n][0] == pos and (pos == len(f) or f[pos:pos + 4] == b"\0\0\0\0")
        assert fr.frame_index(f, idx_cap=n + 1)[0] == n and fr.frame_index(f, idx_cap=n) == (fr.F_DST_MAX_SIZE_TOO_SMALL, [])
    assert {g.FAILED, g.BLOCK_CHECKSUM, -114, -112, -113, -106, -108, -102, -117} <= errors


def test_plan_invariants():
    for view in g.small_views() + g.long_views() + [v for v, _, _ in g.wrong_index_views()]:
        bs = fr.BLOCK_SIZES[(view.frame[5] >> 4) & 7]
        for a, b in _ranges(view) + [(7, 3)]:
            cap, items = fr.plan_range(view.entries, view.idx_n, a, b)
            r, skip, slot = fr.decompress_frame_range(view.frame, view.entries, view.idx_n, a, b)
            if r > 0:
                S = view.size
                k0 = fr.block_of(view.entries, view.idx_n, min(a, S))
                assert cap == min(b, S) - view.entries[k0][1] == len(slot) and skip < bs and cap >= r + skip
                assert items >= 1
            if min(a, view.size) == min(b, view.size) or a > b:
                assert (cap, items) == (0, 0)
    assert fr.plan([(5, 1), (0, 0), (64, 2), (65, 1)], 64) == ([0, 64, 64, 128], 256, 4)
    assert fr.plan([(5, 1), (0, 0), (64, 2)], 0) == ([0, 5, 5], 69, 3)


def test_results_stated_by_hand():
    for view, want in g.defect_views():
        for a, b in g.small_ranges(view):
            r = fr.decompress_frame_range(view.frame, view.entries, view.idx_n, a, b)[0]
            a1, b1 = min(a, 170), min(b, 170)
            w = want(a1, b1) if a1 < b1 else None
            assert r == (b1 - a1 if w is None else w), (view.name, a, b, r)
    assert zs.frame_size(g.defect_views()[2][0].frame) == 170             # a bad content checksum is never reported
    for view, want in g.header_views():
        for a, b in ((0, 0), (0, 10), (5, g.BIG)):
            assert fr.decompress_frame_range(view.frame, view.entries, view.idx_n, a, b)[0] == want, view.name
            assert fr.frame_range(view.frame, a, b)[0] == want
    for view, ranges, want in g.wrong_index_views():
        for a, b in ranges:
            r = fr.decompress_frame_range(view.frame, view.entries, view.idx_n, a, b)[0]
            assert (r == min(b, view.size) - min(a, view.size)) if want is None else (r == want), (view.name, a, b, r)
    five = g.small_views()[0]
    E, n = five.entries, five.idx_n
    assert fr.decompress_frame_range(five.frame, E, n, 9, 3)[0] == g.INVALID_STATE
    assert fr.decompress_frame_range(five.frame, E, n, 3, 9, reserved=1)[0] == g.INVALID_STATE
    assert fr.decompress_frame_range(five.frame, E, n, 3, 9, frame_ok=False)[0] == g.INVALID_STATE
    assert fr.decompress_frame_range(five.frame, E, n, 310, 400, dst_cap=99)[0] == g.DST_TOO_SMALL    # needs 400 - 300
    assert fr.decompress_frame_range(five.frame, E, n, 310, 400, dst_cap=100)[0] == 90
    assert fr.decompress_frame_range(five.frame, E, n, 310, 400, fits=False)[0] == g.INVALID_STATE
    assert fr.decompress_frame_range(five.frame, E, n, 2000, 3000, dst_cap=0, fits=False)[:2] == (0, 0)
    lv = {v.name: v for v in g.linked_views()}["linked_ref_history_index"]
    run = lambda a, b: fr.decompress_frame_range(lv.frame, lv.entries, lv.idx_n, a, b)[0]   # noqa: E731
    assert run(0, 300) == 300 and run(17, 40) == 23 and run(0, 379) == g.FAILED and run(290, 311) == g.FAILED
    assert run(300, 310) == 10                         # (the cut lies in block 1's literals: nothing behind it is read)


def test_refusals_that_need_no_device(zl):
    L = zl.lib()
    buf = (C.c_uint64 * 16)()
    p = (C.addressof(buf) + 15) & ~15                  # 16-byte aligned; never dereferenced: every call below is refused
    iws, rws = zl.lz4f.frameIndexBatchWorkspace, zl.lz4f.decompressFrameRangeBatchWorkspace
    assert iws(3, 17) == zl.lz4f.frameDecompressedSizeBatchWorkspace(3, 17) and iws(1, 100) > iws(1, 10) > 0
    assert rws(10, 100) > rws(10, 10) > rws(1, 0) > 0 and rws(100, 10) > rws(10, 10)
    index = lambda *a: L.zlz4f_batch_frame_index(None, *a)                # noqa: E731
    good = [p, p, p, p, p, p, p, 1, 4, p, iws(1, 4)]
    assert index(*[None] * 7, 0, 0, None, 0) == 0                         # nframes == 0
    for k in range(7):                                                    # a null array, a misaligned 64-bit array
        assert index(*[None if i == k else x for i, x in enumerate(good)]) == -5, k
        if k in (3, 4, 5):
            assert index(*[p + 4 if i == k else x for i, x in enumerate(good)]) == -5, k
    assert index(*good[:9], None, iws(1, 4)) == -5 and index(*good[:9], p + 8, iws(1, 4)) == -5
    assert index(*good[:9], p, iws(1, 4) - 1) == -5
    plan = lambda *a: L.zlz4f_batch_plan_frame_ranges(None, *a)          # noqa: E731
    good = [p, p, p, 1, p, 1, 0, p, p, p]
    for align in (3, 6, 24, 8192, 4097):
        assert plan(*good[:6], align, p, p, p) == -5, align
    for k in (0, 1, 2, 4, 7, 8, 9):
        assert plan(*[None if i == k else x for i, x in enumerate(good)]) == -5, k
        assert plan(*[p + 4 if i == k else x for i, x in enumerate(good)]) == -5, k
    rng = lambda *a: L.zlz4f_batch_decompress_frame_range(None, *a)      # noqa: E731
    good = [p, p, p, p, p, p, 1, p, p, p, p, p, p, 1, 4, p, rws(1, 4)]
    assert rng(*[None] * 6, 0, *[None] * 6, 0, 0, None, 0) == 0           # nranges == 0
    for k in (0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12):
        assert rng(*[None if i == k else x for i, x in enumerate(good)]) == -5, k
        if k not in (0, 8):                                               # (the byte arrays have no alignment)
            assert rng(*[p + 4 if i == k else x for i, x in enumerate(good)]) == -5, k
    assert rng(*good[:15], None, rws(1, 4)) == -5 and rng(*good[:15], p + 8, rws(1, 4)) == -5
    assert rng(*good[:15], p, rws(1, 4) - 1) == -5
    # the host call: header errors and a > b need no device
    for name, frame, want in g.frameprefixgen.header_cases():
        with pytest.raises(zl.Lz4Error) as e:
            zl.lz4f.decompressFrameRange(frame, 0, 10)
        assert e.value.code == want, name
    with pytest.raises(zl.Lz4Error) as e:
        zl.lz4f.decompressFrameRange(g.small_views()[0].frame, 9, 3)
    assert e.value.code == g.INVALID_STATE


def test_the_public_surface_names_the_calls(zl):
    header = open(os.path.join(ROOT, "include", "zlz4_amd.h")).read()
    zig = open(os.path.join(ROOT, "zig-lz4_amd", "zig", "root.zig")).read()
    hpp = open(os.path.join(ROOT, "zig-lz4_amd", "csrc", "host", "zlz4.hpp")).read()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in zl.SYMBOLS and hasattr(zl.lib(), name), name
        assert name in zig and name in hpp, name
    assert "zlz4f_index_entry" in header and "zlz4f_range" in header
    assert C.sizeof(C.c_uint64) * 2 == 16
    packed = zl.lz4f.packRanges([(3, 5, 1 << 63)])
    assert packed.tobytes() == (3).to_bytes(4, "little") + bytes(4) + (5).to_bytes(8, "little") + (1 << 63).to_bytes(8, "little")
