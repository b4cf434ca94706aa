"""Seek tables without a GPU: the model tools/pyref/zig_lz4_seek_table.py against the models of the
file range calls (the central property: a table loads to what split and index compute for the file WITH the table),
figures stated by hand for three files, every single-field mutation of a valid table, the host build of the shared
footer parse and row checks under the address and undefined-behaviour sanitizers, the refusals of the new calls that need
no device, and the public surface.  Corpus: tests/seektablegen.py.

"Cut by one byte" and "one byte added" are read as a byte taken from or put in front of the footer, so that the tail magic
still stands and the table is malformed; a byte taken from or added at the very END removes the tail magic, and by the
format's own rule such a file has no table (split result 0).  Both readings are in the mutation table."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import lz4filegen as fg
import seektablegen as sg

st, ff, g = sg.st, sg.ff, sg.g
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("zlz4f_seek_table_bound", "zlz4f_batch_append_seek_table", "zlz4f_batch_load_seek_table",
         "zlz4f_batch_concat_workspace", "zlz4f_batch_concat", "zlz4f_seek_table", "zlz4f_decompress_file_range_ex")
PY_NAMES = ("seekTableBound", "appendSeekTableBatch", "loadSeekTableBatch", "concatBatchWorkspace", "concatBatch",
            "appendSeekTables", "loadFileIndex", "seekTable", "compressFiles", "splitStaged", "indexSplit")


def test_a_table_loads_to_what_split_and_index_compute():
    accepted = 0
    for name, F in sg.cpu_files():
        tab = st.table(F)
        assert not isinstance(tab, int), (name, tab)
        accepted += 1
        G = F + tab
        assert len(tab) == st.bound(len(ff.split(F)), ff.file_index(F)[0])
        assert ff.split(G) == ff.split(F) + [(len(F), len(tab), ff.SKIPPABLE)], name
        assert [(m.pos, m.len, m.kind | m.nibble << 8) for m in fg.split(G)] == st.members(G), name
        sr, rows, idx_n, entries = st.load(G)
        assert (sr, rows) == (len(rows), st.members(G)) and (idx_n, entries) == ff.file_index(G), name
        assert (idx_n, entries) == ff.file_index(F), name              # a skippable member adds no entry
        assert fg.expected(G)[:2] == fg.expected(F)[:2], name          # the table is invisible to the decode
        # a second table lists the first as an ordinary member, and the loader uses the last
        GG = G + st.table(G)
        assert st.load(GG)[1] == st.members(GG) and st.load(GG)[0] == sr + 1, name
    assert accepted == len(sg.cpu_files()) == 56
    for name, F in sg.shape_files():
        G = F + st.table(F)
        sr, rows, idx_n, entries = st.load(G)
        assert (sr, rows) == (len(rows), st.members(G)) and (idx_n, entries) == ff.file_index(G), name


def test_ranges_through_the_loaded_tables_are_the_content():
    seen = 0
    for view in g.tiny_views():
        if view.name == "tiny_not_legacy":
            continue
        G = view.buf + st.table(view.buf)
        data = g.content(view.buf)
        sr, rows, idx_n, entries = st.load(G)
        for a, b in g.all_ranges(view):
            r, skip, slot = ff.decompress_file_range(G, rows, entries, idx_n, a, b)
            a1, b1 = min(a, len(data)), min(b, len(data))
            assert r == b1 - a1 and slot[skip:skip + r] == data[a1:b1], (view.name, a, b)
            seen += 1
    assert seen > 3000


def test_refused_files_are_refused_for_the_stated_reason():
    refused = sg.refused_files()
    assert len(refused) == 8
    for name, F, code in refused:
        assert st.append_refusal(F) == code == st.table(F), name
    # the chain without its end mark is the one refusal that the index does not make
    assert [ff.file_index(F)[0] >= 0 for _, F, _ in refused] == [True, True] + [False] * 6
    F = sg.cpu_files()[0][1]
    T = len(st.table(F))
    assert st.table(F, cap=len(F) + T - 1) == sg.DST_TOO_SMALL and st.table(F, cap=len(F) + T) == st.table(F)
    assert st.bound(0, (1 << 28) - 5) == (1 << 32) and st.bound(0, (1 << 28) - 4) == 0 == st.bound(1 << 28, 0)
    assert st.bound(0, 0) == 80


def test_figures_stated_by_hand():
    # 1. the empty file: the table alone
    t = st.table(b"")
    assert len(t) == 80 and st.load(t) == (1, [(0, 80, 0xC02)], 0, [(0, 0)])
    assert t == struct.pack("<II", 0x184D2A5C, 72) + struct.pack("<QQII", 0, 80, 0xC02, 0) + struct.pack("<QQ", 0, 0) + \
        struct.pack("<QQQII", 1, 0, 80, 1, 0x4B53345A)
    assert t[-4:] == b"Z4SK" and ff.split(t) == [(0, 80, ff.SKIPPABLE)] and ff.file_index(t) == (0, [(0, 0)])
    # 2. one three-block frame: header 7, blocks of 8 / 5 (stored) / 10 bytes, the end mark at 42, 46 bytes
    tf = {v.name: v for v in g.tiny_views()}["tiny_one_frame"].buf
    t = st.table(tf)
    assert len(t) == 40 + 24 * 2 + 16 * 4 == 152
    assert st.load(tf + t) == (2, [(0, 46, 1), (46, 152, 0xC02)], 3, [(7, 0), (19, 7), (28, 12), (42, 21)])
    assert struct.unpack("<QQQII", (tf + t)[-32:]) == (2, 3, 198, 1, 0x4B53345A)
    # 3. cat frame legacy skippable
    tl = sg.lg.build([sg.lg.literal_block(b"abcdef"), sg.lg.EMPTY, sg.lg.literal_block(b"ghi")])
    sk = g.members()["SK"]
    F = tf + tl + sk
    assert (len(tf), len(tl), len(sk)) == (46, 28, 18)
    t = st.table(F)
    assert len(t) == 40 + 24 * 4 + 16 * 7 == 248
    assert st.load(F + t) == (4, [(0, 46, 1), (46, 28, 4), (74, 18, 2 | 5 << 8), (92, 248, 0xC02)], 6,
                              [(7, 0), (19, 7), (28, 12), (50, 21), (61, 27), (66, 27), (74, 30)])
    # concat: the first negative item in item order, then the capacity
    assert st.concat([b"ab", b"", b"cde"]) == b"abcde" and st.concat([b"ab", -111, -5]) == -111
    assert st.concat([b"ab", b"cde"], cap=4) == sg.DST_TOO_SMALL and st.concat([], cap=0) == b""


def test_every_mutation_gets_its_code():
    muts = sg.mutations()
    assert len(muts) > 60 and len({b for _, b, _ in muts}) == len(muts)
    for name, buf, code in muts:
        sr, rows, idx_n, entries = st.load(buf)
        assert sr == code, (name, sr, code)
        assert idx_n == (len(entries) - 1 if sr > 0 else sg.INVALID_STATE), name
        assert st.rooms(buf) == ((sr, idx_n + 1) if sr > 0 else st.rooms(buf)), name
    assert [c for _, _, c in muts].count(5) == 5 and [c for _, _, c in muts].count(0) == 5
    F, R, E, T, n = sg.mutation_base()
    good = muts[0][1]
    assert st.load(good, mem_cap=4)[0] == sg.DST_TOO_SMALL == st.load(good, idx_cap=7)[0]
    assert st.load(good, mem_cap=5, idx_cap=8)[0] == 5
    # shape only: the moved position loads, and the range call is the judge
    moved = dict((nm, b) for nm, b, _ in muts)["entry_pos_moved_in_bound"]
    sr, rows, idx_n, entries = st.load(moved)
    assert ff.decompress_file_range(moved, rows, entries, idx_n, E[3][1], E[3][1] + 1)[0] == sg.INVALID_STATE
    assert ff.decompress_file_range(moved, rows, entries, idx_n, 0, 5)[0] == 5


def _cases():
    """(file bytes, the append's arguments) for the host check: every file with and without its table, every mutation"""
    out = []
    for name, F in sg.cpu_files() + sg.shape_files() + [(n, b) for n, b, _ in sg.refused_files()]:
        tab = st.table(F)
        out += [F] + ([F + tab, F + tab + st.table(F + tab)] if not isinstance(tab, int) else [])
    return out + [b for _, b, _ in sg.mutations()]


def _load_line(buf):
    sr, rows, idx_n, entries = st.load(buf)
    if sr <= 0:
        return "L %d %d :" % (sr, idx_n)
    return "L %d %d :%s ;%s" % (sr, idx_n, ",".join(" %d %d %d" % r for r in rows), ",".join(" %d %d" % e for e in entries))


def _append_args(buf, k):
    """-> (packed arguments, the expected line)"""
    rows = st.members(buf)
    idx_n, entries = ff.file_index(buf)
    T = st.table_bytes(len(rows) + 1, max(idx_n, 0))
    cap = len(buf) + T - (1 if k % 3 == 2 else 0)                      # every third case one byte short
    why = st.append_refusal(buf, cap=cap)
    last = rows[-1] if rows else (0, 0, 0)
    args = struct.pack("<qQQIqQQ", len(rows), last[0], last[1], last[2], idx_n, entries[idx_n][0] if idx_n >= 0 else 0, cap)
    return args, "A %d %d" % (why, T if why in (0, sg.DST_TOO_SMALL) else 0)


def test_shared_functions_on_the_host_under_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "no hipcc: the host build of the seek table functions cannot be checked"
    cases = _cases()
    exe, data = str(tmp_path / "seek_table_check"), str(tmp_path / "cases.bin")
    want = []
    with open(data, "wb") as fh:
        fh.write(struct.pack("<I", len(cases)))
        for k, b in enumerate(cases):
            args, line = _append_args(b, k)
            fh.write(struct.pack("<I", len(b)) + b + args)
            want += [_load_line(b), line]
    subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-Xarch_host",
                           "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "seek_table_check.cpp")], cwd=str(tmp_path))
    out = subprocess.run([exe, data], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and not out.stderr.strip(), out.stdout[-2000:] + out.stderr[-4000:]
    rows = out.stdout.splitlines()
    assert len(rows) == len(want) == 2 * len(cases)
    for k, (got, exp) in enumerate(zip(rows, want)):
        assert got == exp, (k // 2, got[:200], exp[:200])
    codes = {w.split()[1] for w in want if w.startswith("A")}
    assert codes >= {"0", "-5", "-111", "-112", "-114", "-116"}


def test_refusals_need_no_device(zl):
    L = zl.lib()
    buf = (C.c_uint8 * 128)()
    p = C.addressof(buf)
    assert L.zlz4f_seek_table_bound(0, 0) == 80 and L.zlz4f_seek_table_bound(3, 6) == 248
    assert L.zlz4f_seek_table_bound(0, (1 << 28) - 5) == 1 << 32 and L.zlz4f_seek_table_bound(0, (1 << 28) - 4) == 0
    assert L.zlz4f_seek_table_bound((1 << 64) - 1, 0) == 0 == L.zlz4f_seek_table_bound(1 << 62, 1 << 62)
    # host calls: an unknown flag bit, then a null pointer with a length
    assert L.zlz4f_seek_table(None, 16, None, 16, 2) == g.PARAMETER_INVALID
    assert L.zlz4f_seek_table(None, 16, p, 16, 1) == g.INVALID_STATE == L.zlz4f_seek_table(p, 16, None, 16, 0)
    assert L.zlz4f_decompress_file_range_ex(None, 16, 9, 4, None, 16, 2, 1) == g.PARAMETER_INVALID
    assert L.zlz4f_decompress_file_range_ex(p, 16, 0, 4, p, 16, 1, 2) == g.PARAMETER_INVALID
    assert L.zlz4f_decompress_file_range_ex(None, 16, 0, 4, p, 16, 1, 1) == g.INVALID_STATE
    assert L.zlz4f_decompress_file_range_ex(p, 16, 0, 4, None, 16, 1, 1) == g.INVALID_STATE
    assert L.zlz4f_decompress_file_range_ex(p, 16, 5, 4, p, 16, 1, 1) == g.INVALID_STATE
    assert L.zlz4f_decompress_file_range_ex(p, 16, 5, 4, p, 16, 1, 0) == g.INVALID_STATE       # range_flags 0: the plain call
    # batch calls: nothing to do, then null and misaligned arrays, all in front of the device check
    odd = p + 4
    assert L.zlz4f_batch_append_seek_table(*([None] * 5), 0, *([None] * 7)) == 0
    assert L.zlz4f_batch_append_seek_table(*([None] * 5), 1, *([None] * 7)) == g.INVALID_STATE
    assert L.zlz4f_batch_append_seek_table(p, p, p, p, p, 1, p, p, p, p, p, p, None) == g.INVALID_STATE
    assert L.zlz4f_batch_append_seek_table(p, p, p, odd, p, 1, p, p, p, p, p, p, p) == g.INVALID_STATE
    assert L.zlz4f_batch_load_seek_table(*([None] * 4), 0, None, None, *([None] * 6), 0, None) == g.INVALID_STATE   # no totals
    assert L.zlz4f_batch_load_seek_table(*([None] * 4), 1, None, p, *([None] * 6), 0, None) == g.INVALID_STATE
    assert L.zlz4f_batch_load_seek_table(None, p, p, p, 1, p, odd, *([None] * 6), 0, None) == g.INVALID_STATE
    assert L.zlz4f_batch_load_seek_table(None, p, p, p, 1, p, p, p, p, p, p, p, None, 4, p) == g.INVALID_STATE      # no idx_off
    assert L.zlz4f_batch_concat(*([None] * 5), 0, 0, *([None] * 5), 0) == 0
    assert L.zlz4f_batch_concat(*([None] * 5), 1, 0, *([None] * 5), 0) == g.INVALID_STATE
    assert L.zlz4f_batch_concat(p, p, p, p, p, 1, 1, p, p, p, p, None, 0) == g.INVALID_STATE       # no workspace
    assert L.zlz4f_batch_concat(p, p, p, p, p, 1, 1, p, p, odd, p, p, 256) == g.INVALID_STATE
    assert L.zlz4f_batch_concat_workspace(0) == 0 and L.zlz4f_batch_concat_workspace(33) == 512


def test_public_surface_names_the_new_calls(zl):
    def text(*p):
        return open(os.path.join(ROOT, *p)).read()

    header, mirror, zig = text("include", "zlz4_amd.h"), text("zig-lz4_amd", "csrc", "host", "zlz4.hpp"), text("zig-lz4_amd", "zig", "root.zig")
    for name in NAMES:
        assert name in header and name in zl.SYMBOLS and hasattr(zl.lib(), name), name
        assert name in zig and name in mirror and name in text("INTEGRATION.md"), name
    for name in PY_NAMES:
        assert hasattr(zl.lz4f, name), name
    for name in ("ZLZ4F_SEEK_TABLE_MAGICNUMBER", "0x184D2A5C", "0x4B53345A", "ZLZ4F_RANGE_SEEK_TABLE"):
        assert name in header, name
    for name in ("lz4f.compressFiles(", "lz4f.loadFileIndex(", "lz4f.appendSeekTables(", "lz4f.seekTable(", "0x184D2A5C", "Z4SK"):
        assert name in text("INTEGRATION.md"), name
    assert "4.4l" in text("DESIGN.md") and "compressFiles" in text("README.md")
    assert zl.lz4f.RANGE_SEEK_TABLE == 1 and zl.lz4f.SEEK_TABLE_MAGICNUMBER == st.MAGIC
