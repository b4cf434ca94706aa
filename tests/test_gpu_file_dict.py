"""Dictionary .lz4 files on the GPU (zlz4f_batch_file_index_using_dict, zlz4f_batch_decompress_file_range_using_dict,
zlz4f_batch_multiframe_item_dicts, zlz4f_decompress_file_range_using_dict and the dicts= keywords of the Python file
functions) against the model tools/pyref/zig_lz4_file_dict.py.  Corpus and runners:
tests/filedictgen.py (files written by the `lz4` tool: tests/golden/dict_files.json).  Every output region stands between
canary bytes."""
import pytest

import filedictgen as g
import filerangegen as rg

pytestmark = pytest.mark.gpu
fd, ff = g.fd, g.ff
INVALID = g.INVALID_STATE


def _corpus():
    return g.accepted_views() + g.refused_views() + [g.tiny_view()]


# ----------------------------------------------------------------------------- 1. the index
def test_index_against_the_model(zl, gpu):
    """one batch that mixes every corpus file over the table of their dictionaries, at two placements of the arena: results,
    d_idx_off and entries; one file names a dictionary past the table; then a NULL d_dict_idx with one dictionary, and
    idx_cap one short"""
    views = _corpus()
    table, didx = g.dict_table(views)
    assert 2 <= len(table) and len(views) < 300
    bad = 4                                             # this file's dictionary index lies past the table
    didx[bad] = len(table)
    want = [(INVALID, []) if s == bad else (v.idx_n, v.entries) for s, v in enumerate(views)]
    for lead in (0, 5):
        sp = g.stage(zl, [v.buf for v in views], gpu, lead)
        results, idx_off, rows = g.gpu_index(zl, sp, gpu, [len(d) for d in table], didx)
        for s, (v, (n, entries)) in enumerate(zip(views, want)):
            assert results[s] == n, (v.name, results[s], n)
            if n >= 0:
                assert rows[idx_off[s]:idx_off[s] + n + 1] == entries, v.name
                assert idx_off[s + 1] - idx_off[s] == n + 1, v.name
        assert results[bad] == INVALID and views[bad].idx_n >= 0       # its neighbours are untouched (the loop above)
        assert idx_off[bad + 1] - idx_off[bad] == views[bad].idx_n + 1  # and its room is kept
    # a NULL index with ndicts = 1: every file uses dictionary 0
    same = [v for v in views if v.dict == g.dic(300)]
    assert len(same) >= 5
    sp = g.stage(zl, [v.buf for v in same], gpu, 3)
    results, idx_off, rows = g.gpu_index(zl, sp, gpu, [300], None)
    assert results == [v.idx_n for v in same]
    # idx_cap one short: the last file that would be written answers DstMaxSizeTooSmall, the others stand
    last = max(s for s, v in enumerate(same) if v.idx_n >= 0)
    short, off2, rows2 = g.gpu_index(zl, sp, gpu, [300], None, idx_cap=idx_off[last + 1] - 1)
    assert off2 == idx_off
    for s, v in enumerate(same):
        ends_behind = idx_off[s + 1] > idx_off[last + 1] - 1
        assert short[s] == (g.DST_TOO_SMALL if ends_behind and v.idx_n >= 0 else v.idx_n), v.name


# ----------------------------------------------------------------------------- 2. identity
def test_identity_without_dictionaries(zl, gpu):
    """all dictionary lengths 0: both batch calls equal the plain calls on filerangegen's views -- entries, results, bytes,
    d_skip"""
    plain_views = rg.tiny_views() + rg.range_views() + rg.bound_views() + rg.lane_edge_views()
    sp = g.stage(zl, [v.buf for v in plain_views], gpu, 0)
    ix = zl.lz4f.indexSplit(sp)
    for lens, didx in (([0], None), ([0, 0, 0], [s % 3 for s in range(len(plain_views))])):
        results, idx_off, rows = g.gpu_index(zl, sp, gpu, lens, didx)
        assert results == ix.results and idx_off == ix.idx_off.cpu().tolist()
        prows = [tuple(r) for r in ix.index.cpu().tolist()]
        for s, n in enumerate(results):
            if n >= 0:
                assert rows[idx_off[s]:idx_off[s] + n + 1] == prows[idx_off[s]:idx_off[s] + n + 1]
    views = [g.View(v.name, v.buf, b"", (v.idx_n, v.entries)) for v in plain_views if v.name != "tiny_not_legacy"]
    views += [g.View(v.name, v.buf, b"", (v.idx_n, v.entries), valid=False) for v, _ in rg.wrong_index_views()]
    ranges = {}
    for v in plain_views:
        ranges[v.name] = rg.all_ranges(v)[::11] if v.size <= 80 else rg.bound_ranges(v)
    for v, r in rg.wrong_index_views():
        ranges[v.name] = r
    views, items = g.items_of(views, lambda v: ranges[v.name])
    items.append(("cap_one_short", 1, 0, g.BIG, 0, -1, None))
    assert 300 < len(items)
    got = g.run(zl, views, items, gpu)
    assert got == g.run(zl, views, items, gpu, plain=True)
    assert [(r, sk) for r, sk, _ in got] == [(r, sk) for r, sk, _ in g.expect(views, items)]


# ----------------------------------------------------------------------------- 3. ranges
def test_ranges_against_the_model(zl, gpu):
    """every file of the corpus under its own index and dictionary: cuts one byte either side of every block and member
    boundary (the spans cross members with and without the dictionary), cuts inside a match that comes from T -- the cut
    block goes through the prefix decoder with a dictionary --, the refused files' codes; at two placements"""
    views, items = g.items_of(_corpus()[:-1], g.edge_ranges)
    assert 400 < len(items) < 4000
    want = g.expect(views, items)
    assert sum(1 for r, _, _ in want if r > 0) > 300
    for lead in (0, 9):
        g.compare(views, items, g.run(zl, views, items, gpu, lead=lead), want)


def test_every_range_of_a_tiny_file(zl, gpu):
    views, items = g.items_of([g.tiny_view()], g.all_ranges)
    assert len(items) > 1500
    g.compare(views, items, g.run(zl, views, items, gpu), g.expect(views, items))


def test_foreign_pairings_capacity_and_refusals(zl, gpu):
    """an index built with D = 65 536 read with 100 bytes, the index of another file, the plain index, no dictionary; slots
    one byte short; max_items one short; a file that names no dictionary"""
    pairs = g.foreign_views()
    views, items = g.items_of([v for v, _ in pairs], lambda v: dict((p.name, r) for p, r in pairs)[v.name])
    own = g.accepted_views()[0]
    views.append(own)
    k = len(views) - 1
    S = own.size
    items += [("own_whole", k, 0, g.BIG, 0, None, None), ("own_one_short", k, 0, g.BIG, 0, -1, None),
              ("own_cut_one_short", k, 3, S - 2, 0, -1, None), ("own_reserved", k, 0, 5, 1, None, None),
              ("own_no_buffer", k, 0, 5, 0, None, 99), ("own_empty", k, 7, 7, 0, None, None)]
    want = g.expect(views, items)
    assert [w[0] for w in want[-6:]] == [S, g.DST_TOO_SMALL, g.DST_TOO_SMALL, INVALID, INVALID, 0]
    g.compare(views, items, g.run(zl, views, items, gpu), want)
    total = sum(ff.range_items(views[v].buf, views[v].members, views[v].entries, views[v].idx_n, a, b)
                for _, v, a, b, res, cd, bo in items if res == 0 and cd is None and bo is None)
    want = g.expect(views, items, max_items=total - 1)
    assert any(w[0] == INVALID for w in want[-6:-5])
    g.compare(views, items, g.run(zl, views, items, gpu, max_items=total - 1), want)
    # the range's file names no dictionary: InvalidState in step 1, the other files are served
    views2, items2 = g.items_of(g.accepted_views()[:3], lambda v: [(0, g.BIG), (5, 40)])
    want = g.expect(views2, items2, no_dict=(1,))
    assert [w[0] for w in want[2:4]] == [INVALID, INVALID] and want[0][0] > 0 and want[4][0] > 0
    g.compare(views2, items2, g.run(zl, views2, items2, gpu, no_dict=(1,)), want)


# ----------------------------------------------------------------------------- 4. what fails without the feature
def test_files_written_with_lz4_dash_D(zl, gpu):
    """tests/golden/dict_files.json: without dictionaries the index refuses the dictionary files; with dicts= every range
    is the stored content sliced and decompressFiles gives the stored contents.  A linked file of several blocks (-BD, 200 000
    bytes) is decoded whole; its index stays DecompressionFailed (linked members with history are not served)."""
    dictionary, cases = g.golden()
    files = [buf for _, buf, _, _ in cases]
    plain = zl.lz4f.fileIndex(files, device=gpu)
    assert all(r == g.FAILED for r in plain.results), plain.results
    ix = zl.lz4f.fileIndex(files, device=gpu, dicts=[dictionary])
    ranges, want = [], []
    for s, (name, buf, content, linked_multiblock) in enumerate(cases):
        if linked_multiblock:
            assert ix.results[s] == g.FAILED, name
            continue
        assert ix.results[s] == fd.file_index(buf, len(dictionary))[0] >= 1, name
        S = len(content)
        for a, b in ((0, g.BIG), (0, 1), (S // 2, S // 2 + 4096), (65535, 65537), (S - 1, S + 5), (S // 3, S // 3 + 70000)):
            ranges.append((s, a, b))
            want.append(content[a:b])
    assert zl.lz4f.decompressFileRanges(ix, ranges) == want
    assert zl.lz4f.decompressFilesUsingDict(files, [dictionary], device=gpu) == [c for _, _, c, _ in cases]
    two = zl.lz4f.decompressFilesUsingDict(files[:3], [b"", dictionary], [1, 0, 1], device=gpu)
    assert two[0] == cases[0][2] and two[1] == g.FAILED and two[2] == cases[2][2]
    assert zl.lz4f.decompressFilePrefixes(files[:2], 100, device=gpu, dicts=[dictionary]) == [c[:100] for _, _, c, _ in cases[:2]]
    with pytest.raises(ValueError):
        zl.lz4f.decompressFilesUsingDict(files[:2], [dictionary], [0, 1], device=gpu)
    # the hand-built files too: whole-file decoding against the model's content
    views = g.accepted_views()
    table, didx = g.dict_table(views)
    assert zl.lz4f.decompressFilesUsingDict([v.buf for v in views], table, didx, device=gpu) == [g.content(v) for v in views]


# ----------------------------------------------------------------------------- 5. the writer
def _text(n, seed):
    """word text over ONE vocabulary (the dictionary and the inputs share it), the words drawn by `seed`"""
    import random
    v = random.Random(0)
    words = [bytes(v.randrange(97, 123) for _ in range(v.randint(2, 9))) for _ in range(150)]
    r = random.Random(seed)
    out = b""
    while len(out) < n:
        out += r.choice(words) + b" "
    return out[:n]


@pytest.mark.parametrize("level", [0, 3, 9])
def test_writer_round_trip(zl, gpu, level):
    dictionary = _text(70000, 1)
    inputs = [b"", b"x", _text(300, 2), _text(5000, 3), _text(70001, 4)]
    prefs = zl.Prefs()
    prefs.block_mode, prefs.compression_level = 1, level
    for frame_size in (256, 4096, 65537):
        files = zl.lz4f.compressFiles(inputs, prefs, frame_size, device=gpu, dicts=[dictionary])
        assert all(isinstance(f, bytes) for f in files), files
        loaded = zl.lz4f.loadFileIndex(files, device=gpu, dicts=[dictionary])
        built = zl.lz4f.fileIndex(files, device=gpu, dicts=[dictionary])
        assert loaded.results == built.results and min(built.results) >= 0
        assert loaded.idx_off.cpu().tolist() == built.idx_off.cpu().tolist()
        assert loaded.index.cpu().tolist()[:sum(built.results) + len(files)] == \
            built.index.cpu().tolist()[:sum(built.results) + len(files)]
        ranges = [(s, a, b) for s, d in enumerate(inputs) for a, b in ((0, g.BIG), (len(d) // 2, len(d) // 2 + 300), (255, 257))]
        assert zl.lz4f.decompressFileRanges(loaded, ranges) == [inputs[s][a:b] for s, a, b in ranges]
        assert zl.lz4f.decompressFilesUsingDict(files, [dictionary], device=gpu) == inputs
        # every frame is compressFramesUsingDict's on the same chunk
        chunks = [d[o:o + frame_size] for d in inputs for o in range(0, max(1, len(d)), frame_size)]
        frames = zl.lz4f.compressFramesUsingDict(chunks, [dictionary], None, prefs, device=gpu)
        members = zl.lz4f.multiframeMembers(files, device=gpu, legacy=True)
        got = [f[pos:pos + ln] for f, ms in zip(files, members) for pos, ln, kind, _ in ms if kind == zl.lz4f.MEMBER_FRAME]
        assert got == frames
        without = zl.lz4f.compressFiles(inputs, prefs, frame_size, device=gpu)
        assert len(files[2]) < len(without[2]) and len(files[3]) < len(without[3]), frame_size
        assert zl.lz4f.decompressFiles(without, device=gpu) == inputs
    with pytest.raises(ValueError):
        p0 = zl.Prefs()
        zl.lz4f.compressFiles(inputs, p0, 1 << 20, device=gpu, dicts=[dictionary])


# ----------------------------------------------------------------------------- 6. the host call
def test_host_call(zl, gpu):
    dictionary, cases = g.golden()
    name, buf, content, _ = cases[0]
    big = next(cs for cs in cases if cs[0] == "big_legacy_big")
    S = len(big[2])
    for seek in (False, True):
        assert zl.lz4f.decompressFileRange(buf, 10, 200, seek_table=seek, dict=dictionary) == content[10:200]
        assert zl.lz4f.decompressFileRange(big[1], 199990, 205010, seek_table=seek, dict=dictionary) == big[2][199990:205010]
        assert zl.lz4f.decompressFileRange(big[1], S - 5, S + 100, seek_table=seek, dict=dictionary) == big[2][S - 5:]
        assert zl.lz4f.decompressFileRange(big[1], 100, g.BIG, seek_table=seek, dict=dictionary) == big[2][100:]   # a far b
    with pytest.raises(zl.Lz4Error):                    # three bytes of dictionary: the offsets reach in front of them
        zl.lz4f.decompressFileRange(buf, 0, 200, dict=b"abc")
    # a file with a seek table: written with the dictionary, read through the table
    prefs = zl.Prefs()
    prefs.block_mode = 1
    data = _text(20000, 9)
    seekable = zl.lz4f.compressFiles([data], prefs, 4096, device=gpu, dicts=[dictionary])[0]
    for seek in (False, True):
        assert zl.lz4f.decompressFileRange(seekable, 4000, 9000, seek_table=seek, dict=dictionary) == data[4000:9000]
    # dict_len == 0 is the _ex call
    v = rg.range_views()[0]
    for seek in (False, True):
        assert zl.lz4f.decompressFileRange(v.buf, 3, 300, seek_table=seek, dict=b"") == \
            zl.lz4f.decompressFileRange(v.buf, 3, 300, seek_table=seek)
