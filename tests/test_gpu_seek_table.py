"""Seek tables on the GPU (zlz4f_batch_append_seek_table, zlz4f_batch_load_seek_table, zlz4f_batch_concat, the two host
calls and the Python one-liners) against the model tools/pyref/zig_lz4_seek_table.py, byte for
byte.  Corpus and runners: tests/seektablegen.py.  Every output region stands between canary bytes or rows: nothing outside
[n, n + T), the rows of the files that loaded and the slots of the files that joined may change."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import datagen as dg
import seektablegen as sg

pytestmark = pytest.mark.gpu
st, ff, g, frg = sg.st, sg.ff, sg.g, sg.frg
LZ4_CLI = shutil.which("lz4") or ("/opt/conda/bin/lz4" if os.path.exists("/opt/conda/bin/lz4") else None)


def _all_files():
    return [b for _, b in sg.cpu_files() + sg.shape_files()] + [b for _, b, _ in sg.refused_files()]


def _with_tables():
    """every accepted file with its table -> [G]"""
    return [F + st.table(F) for _, F in sg.cpu_files() + sg.shape_files()]


# ----------------------------------------------------------------------------- append
def test_append_against_the_model(zl, gpu):
    """one batch that mixes every case, at two placements of the arena: the table bytes, the result, nothing else changed"""
    files = _all_files()
    files += [files[0] + st.table(files[0])]                           # a second table behind the first
    want = [st.table(F) for F in files]
    assert sum(isinstance(w, int) for w in want) == len(sg.refused_files())
    for pad in (0, 3):
        got = sg.run_append(zl, files, gpu, pad=pad)
        for s, (F, w, (r, slot)) in enumerate(zip(files, want, got)):
            if isinstance(w, int):
                assert r == w and slot == F, (s, r, w)
            else:
                assert r == len(F) + len(w) and slot == F + w, (s, r, len(F) + len(w))


def test_append_capacity_one_short(zl, gpu):
    files = [b for _, b in sg.cpu_files()[:12]] + [b for n, b in sg.shape_files() if n.startswith("aligned_")][:4]
    short = {s: -1 for s in range(0, len(files), 2)}
    got = sg.run_append(zl, files, gpu, cap_delta=short, pad=5)
    for s, (F, (r, slot)) in enumerate(zip(files, got)):
        if s in short:
            assert r == sg.DST_TOO_SMALL and slot == F, s              # (run_append: the buffer and the canaries untouched)
        else:
            assert slot == F + st.table(F), s
    # without legacy members a legacy magic is FrameTypeUnknown, and that code is the append's
    L3 = g.members()["L3"]
    assert sg.run_append(zl, [L3, g.members()["F"]], gpu, legacy=False)[0] == (sg.lg.TYPE_UNKNOWN, L3)


# ----------------------------------------------------------------------------- load
def test_load_against_the_model(zl, gpu):
    """files with a table, files without, every mutation, in one batch"""
    files = _with_tables() + _all_files()[::3] + [b for _, b, _ in sg.mutations()]
    counts, totals, loaded, idx_off = sg.run_load(zl, files, gpu)
    sg.check_loaded(files, loaded)
    rooms = [st.rooms(f) for f in files]
    assert counts == [r[0] for r in rooms] and totals == [sum(r[0] for r in rooms), sum(r[1] for r in rooms)]
    assert idx_off == [sum(r[1] for r in rooms[:s]) for s in range(len(files) + 1)]
    for (name, buf, code), got in zip(sg.mutations(), loaded[-len(sg.mutations()):]):
        assert got[0] == code, (name, got[0], code)


def test_load_capacities_one_short(zl, gpu):
    files = _with_tables()[:40] + [sg.mutations()[0][1], sg.mutations()[30][1]]
    short = set(range(0, len(files), 3))
    _, totals, loaded, idx_off = sg.run_load(zl, files, gpu, mem_short=short)
    for s, (f, got) in enumerate(zip(files, loaded)):
        want = st.load(f, mem_cap=st.rooms(f)[0] - (1 if s in short else 0))
        assert got[0] == want[0] and got[2] == want[2], (s, got[0], want[0])
        assert got[0] == sg.DST_TOO_SMALL or s not in short
    # the index one entry short: every file whose room ends behind idx_cap, and no other
    _, totals, loaded, idx_off = sg.run_load(zl, files, gpu, idx_short=1)
    hit = [s for s in range(len(files)) if idx_off[s + 1] > totals[1] - 1 and st.rooms(files[s])[1]]
    assert hit and [s for s, got in enumerate(loaded) if got[0] == sg.DST_TOO_SMALL] == hit
    for s, (f, got) in enumerate(zip(files, loaded)):
        if s not in hit:
            assert tuple(got) == st.load(f), s


def test_loaded_equals_computed(zl, gpu):
    lz = zl.lz4f
    files = _with_tables()
    a, b = lz.loadFileIndex(files, device=gpu), lz.fileIndex(files, device=gpu)
    n = a.split.nitems
    assert n == b.split.nitems == sum(st.rooms(f)[0] for f in files)
    assert a.split.member[:n].cpu().tolist() == b.split.member[:n].cpu().tolist()
    assert a.idx_off.cpu().tolist() == b.idx_off.cpu().tolist() and a.idx_n.cpu().tolist() == b.idx_n.cpu().tolist()
    rows = a.idx_off.cpu().tolist()[-1]
    assert a.index[:rows].cpu().tolist() == b.index[:rows].cpu().tolist()
    assert a.results == b.results and a.split.results == b.split.results and min(a.results) >= 0
    assert a.split.mem_off.cpu().tolist() == b.split.mem_off.cpu().tolist()
    # the range sets of the file range tests, through either
    views = g.range_views() + [v for v in g.tiny_views() if v.name != "tiny_not_legacy"]
    files = [v.buf + st.table(v.buf) for v in views]
    ranges = [(s, a_, b_) for s, v in enumerate(views)
              for a_, b_ in (frg.small_ranges(v, every_a=False) if s < len(g.range_views()) else g.all_ranges(v)[::5])]
    assert len(ranges) > 1500
    via_load = lz.decompressFileRanges(lz.loadFileIndex(files, device=gpu), ranges)
    assert via_load == lz.decompressFileRanges(lz.fileIndex(files, device=gpu), ranges)
    for (s, a_, b_), got in zip(ranges, via_load):
        data = g.content(views[s].buf)
        assert got == data[min(a_, len(data)):min(b_, len(data))], (views[s].name, a_, b_)
    # a file without a table keeps its code
    mixed = lz.loadFileIndex([files[0], views[0].buf, b"", files[1]], device=gpu)
    assert mixed.results[1] == mixed.results[2] == sg.INVALID_STATE and mixed.split.results[1:3] == [0, 0]
    assert lz.decompressFileRanges(mixed, [(0, 3, 9), (1, 3, 9), (3, 0, 5)]) == \
        [g.content(views[0].buf)[3:9], sg.INVALID_STATE, g.content(views[1].buf)[:5]]


def test_untrusted_tables(zl, gpu):
    """a file under the well-shaped table of ANOTHER file of the same length: it loads, and the range call answers what the
    model answers for those tables -- InvalidState, a decode error or the right bytes, never other bytes"""
    lz = zl.lz4f
    files = g.orderings()[::2500][:12]
    assert len(files) >= 10 and len({len(f) for f in files}) == 1
    paired = [files[k] + st.table(files[(k + 1) % len(files)]) for k in range(len(files))]
    ix = lz.loadFileIndex(paired, device=gpu)
    assert ix.split.results == [9] * len(paired) and ix.results == [13] * len(paired)
    ranges, want, refused, right = [], [], 0, 0
    for s, G in enumerate(paired):
        sr, rows, idx_n, entries = st.load(G)
        data = g.content(files[s])
        for d in [e[1] for e in entries[:-1]]:
            for a, b in ((d, d + 1), (max(0, d - 2), d + 40), (d, g.BIG)):
                r, skip, slot = ff.decompress_file_range(G, rows, entries, idx_n, a, b)
                ranges.append((s, a, b))
                want.append(slot[skip:skip + r] if r >= 0 else r)
                if r >= 0:
                    assert want[-1] == data[min(a, len(data)):min(b, len(data))]
                    right += 1
                else:
                    assert r in (sg.INVALID_STATE, g.FAILED, g.BLOCK_CHECKSUM), (s, a, b, r)
                    refused += 1
    assert refused > 50 and right > 20
    assert lz.decompressFileRanges(ix, ranges) == want


# ----------------------------------------------------------------------------- concat, compressFiles
def test_concat_fails_a_file_alone(zl, gpu):
    import torch
    lz = zl.lz4f
    rng = np.random.default_rng(5)
    groups = [[1, 7, 0, 300], [], [5000, 33], [9, 8, 7], [16], [64] * 70, [3, 4], [0]]       # item lengths per file
    bad = {2: (1, -111), 3: (0, -5), 5: (66, -114)}                    # file -> (item, code); file 3 has a second one behind
    items, first, lens = [], [0], []
    for s, grp in enumerate(groups):
        for k, n in enumerate(grp):
            items.append(bytes(rng.integers(0, 256, n, dtype=np.uint8)))
            lens.append(n)
            if s in bad and k == bad[s][0]:
                lens[-1] = bad[s][1]
            if s == 3 and k == 2:
                lens[-1] = -116
        first.append(len(items))
    want = [st.concat([it if ln >= 0 else ln for it, ln in zip(items[first[s]:first[s + 1]], lens[first[s]:first[s + 1]])])
            for s in range(len(groups))]
    want[6] = st.concat(items[first[6]:first[7]], cap=6)               # one byte short
    assert [w for w in want if isinstance(w, int)] == [-111, -5, -114, sg.DST_TOO_SMALL]
    d_src, item_off, _ = zl._stage(items, gpu)
    d_src = torch.cat([torch.zeros(3, dtype=torch.uint8, device=gpu), d_src])       # the items at odd addresses
    caps = [sum(len(it) for it in items[first[s]:first[s + 1]]) - (1 if s == 6 else 0) for s in range(len(groups))]
    offs, pos = [], 5
    for c in caps:
        offs.append(pos)
        pos += c + 13
    t = lambda v: torch.tensor(v, dtype=torch.int64, device=gpu)      # noqa: E731
    d_dst = torch.full((pos,), sg.CANARY, dtype=torch.uint8, device=gpu)
    result = torch.full((len(groups),), -999, dtype=torch.int64, device=gpu)
    lz.concatBatch(d_src, item_off + 3, t(lens), t(first), d_dst, t(offs), t(caps), result)
    torch.cuda.synchronize()
    got, res = d_dst.cpu().numpy().tobytes(), result.cpu().tolist()
    expect = bytearray([sg.CANARY]) * pos
    for s, w in enumerate(want):
        if isinstance(w, int):
            assert res[s] == w, (s, res[s], w)
        else:
            assert res[s] == len(w), (s, res[s], len(w))
            expect[offs[s]:offs[s] + len(w)] = w
    assert got == bytes(expect)                                        # the joins, and every other byte a canary


def test_compress_files(zl, gpu):
    lz = zl.lz4f
    fs = 4096
    text = bytes(dg.text_bytes(3 * fs + 7, 21))
    inputs = [b"", text[:1], text[:fs - 1], text[:fs], text[:fs + 1], text]
    files = lz.compressFiles(inputs, frame_size=fs, device=gpu)
    plain = lz.compressFiles(inputs, frame_size=fs, seek_table=False, device=gpu)
    chunks = [[d[o:o + fs] for o in range(0, len(d), fs)] or [b""] for d in inputs]
    assert [len(c) for c in chunks] == [1, 1, 1, 1, 2, 4]
    frames = lz.compressFrames([c for cs in chunks for c in cs], device=gpu)
    at = 0
    for d, cs, G, P in zip(inputs, chunks, files, plain):
        join = b"".join(frames[at:at + len(cs)])
        at += len(cs)
        assert P == join and G[:len(join)] == join, len(d)
        assert G[len(join):] == st.table(join) and st.load(G)[0] == len(cs) + 1, len(d)
    assert lz.decompressFiles(files, device=gpu) == inputs == lz.decompressFiles(plain, device=gpu)
    ix = lz.loadFileIndex(files, device=gpu)
    assert ix.results == [0, 1, 1, 1, 2, 4]
    ranges = [(5, fs - 3, fs + 3), (5, 2 * fs - 1, 3 * fs + 1), (5, 0, g.BIG), (4, fs - 1, fs + 1), (4, fs, g.BIG), (0, 0, 5),
              (1, 0, 1), (3, fs - 1, fs + 9), (5, 3 * fs, 3 * fs + 7)]
    assert lz.decompressFileRanges(ix, ranges) == [inputs[s][a:b] for s, a, b in ranges]
    assert lz.appendSeekTables(plain, device=gpu) == files
    if LZ4_CLI is not None:
        import tempfile
        with tempfile.TemporaryDirectory() as td:
            for d, G in zip(inputs, files):
                a, b = os.path.join(td, "a.lz4"), os.path.join(td, "a.out")
                open(a, "wb").write(G)
                subprocess.check_call([LZ4_CLI, "-d", "-f", "-q", a, b])
                assert open(b, "rb").read() == d


# ----------------------------------------------------------------------------- host calls
def test_host_calls(zl, gpu):
    lz = zl.lz4f
    for name, F in sg.cpu_files()[:10] + sg.shape_files()[:8] + [("empty", b"")]:
        assert lz.seekTable(F) == st.table(F), name
    for name, F, code in sg.refused_files():
        with pytest.raises(zl.Lz4Error) as e:
            lz.seekTable(F)
        assert e.value.code == code, name
    view = g.range_views()[0]
    F, data = view.buf, g.content(view.buf)
    G = F + st.table(F)
    broken = dict((n, b) for n, b, _ in sg.mutations())["entry_dec4_below_dec3"]
    whole = g.content(sg.mutation_base()[0])
    for buf, content in ((G, data), (F, data), (broken, whole)):       # a table, none, a malformed one: it falls back
        for a, b in ((0, 10), (60, 70), (100, 400), (len(content) - 5, g.BIG), (7, 7)):
            got = lz.decompressFileRange(buf, a, b, seek_table=True)
            assert got == lz.decompressFileRange(buf, a, b) == content[a:b], (len(buf), a, b)
