"""Streaming compression (lz4.Stream: loadDict / compressFastContinue / saveDict, reference src/lz4.zig:751-866): the
public surface and the two restatements (tools/pyref/zig_lz4_stream.py, tests/stream_ref.c), without a GPU."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "pyref"))
import datagen as dg  # noqa: E402
import streamgen  # noqa: E402
import zig_lz4_stream as zs  # noqa: E402

NEW = ("zlz4_stream_load_dict", "zlz4_stream_compress_fast_continue", "zlz4_batch_load_dict",
       "zlz4_batch_compress_fast_continue")
DICT_SIZES = (0, 1, 3, 4, 5, 13, 65535, 65536, 65537, 200000)


@pytest.fixture(scope="module")
def cref(tmp_path_factory):
    return streamgen.ref(tmp_path_factory.mktemp("streamref"))


def _kat():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "stream_kat.json")))["vectors"]


def _table(sparse):
    t = [0] * 4096
    for k, v in sparse.items():
        t[int(k)] = v
    return t


def _blocks(seed):
    rng = np.random.default_rng(seed)
    out = []
    for n in (13, 14, 40, 100, 300, 1000, 4096, 9000):
        for k, gen in enumerate((dg.text_bytes, dg.reptext_bytes, dg.mixed_bytes, dg.random_bytes)):
            out.append(bytes(gen(n, int(rng.integers(0, 1 << 30)))))
    out.append(b"a" * 500)
    out.append(bytes(range(256)) * 3)
    return out


def _tables(seed, n, L):
    """random tables of the kinds a stream can hold: positions of earlier blocks (any u32), values around L / ip"""
    rng = np.random.default_rng(seed)
    kinds = [np.zeros(4096, np.int64),
             rng.integers(0, 2 * max(L, 1) + 1, 4096),
             rng.integers(0, 1 << 32, 4096),
             np.where(rng.random(4096) < 0.5, rng.integers(0, max(L, 1), 4096), 0),
             np.full(4096, max(L - 1, 0)), np.full(4096, L), np.full(4096, L + 11)]
    return [[int(x) for x in kinds[i % len(kinds)]] for i in range(n)]


# ------------------------------------------------------------------ surface
def test_stream_symbols_declared_and_exported(zl):
    hdr = open(os.path.join(ROOT, "include", "zlz4_amd.h")).read()
    L = C.CDLL(zl.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in zl.SYMBOLS, name
    assert "#define ZLZ4_STREAM_TABLE_ENTRIES 4096u" in hdr


def test_root_zig_declares_stream(zl):
    txt = open(os.path.join(ROOT, "zig-lz4_amd", "zig", "root.zig")).read()
    assert re.search(r"^pub const Stream = struct \{", txt, re.M)
    for frag in ("hashTable: [LZ4_HASH_SIZE_U32]u32,", "dictionary: ?[]const u8,", "dictCtx: ?*const Stream,",
                 "currentOffset: u32,", "tableType: TableType,", "dictSize: u32,",
                 "pub fn create(allocator: std.mem.Allocator) Error!*Stream",
                 "pub fn destroy(self: *Stream) void", "pub fn init() Stream", "pub fn resetFast(self: *Stream) void",
                 "pub fn loadDict(self: *Stream, dict: []const u8) usize",
                 "pub fn compressFastContinue(self: *Stream, src: []const u8, dst: []u8, acceleration: u32) Error!usize",
                 "pub fn saveDict(self: *Stream, safeBuffer: []u8, maxDictSize: usize) usize",
                 "pub const Stream = root.Stream;", "pub const createStream = root.createStream;",
                 "pub const freeStream = root.freeStream;", "pub fn loadDictBatch(", "pub fn compressFastContinueBatch("):
        assert frag in txt, frag
    assert re.search(r"^pub fn createStream\(allocator: std\.mem\.Allocator\) Error!\*Stream", txt, re.M)
    assert re.search(r"^pub fn freeStream\(stream: \*Stream\) void", txt, re.M)
    # one root-level error set only (the façade must stay free of ambiguous `Error` references)
    assert len(re.findall(r"^pub const Error = error\{", txt, re.M)) == 1
    L = C.CDLL(zl.LIB_PATH)
    for fn in re.findall(r'^extern "c" fn (\w+)\(', txt, re.M):
        assert hasattr(L, fn), "root.zig binds %s, which the library does not export" % fn
    for name in NEW:
        assert re.search(r'^extern "c" fn %s\(' % name, txt, re.M), name


def test_python_stream_surface(zl):
    s = zl.createStream()
    assert s.hashTable.dtype == np.uint32 and s.hashTable.shape == (4096,)
    assert s.dictionary is None and s.currentOffset == 0 and s.dictSize == 0 and s.tableType == zl.Stream.byU32
    zl.freeStream(s)
    # host-only bookkeeping: saveDict without a dictionary, resetFast
    buf = bytearray(8)
    assert s.saveDict(buf, 8) == 0
    s.hashTable[5] = 9
    s.resetFast()
    assert not s.hashTable.any()


def test_batch_calls_with_no_blocks_need_no_device(zl):
    L = zl.lib()
    assert L.zlz4_batch_load_dict(None, None, None, None, None, None, 0) == 0
    assert L.zlz4_batch_compress_fast_continue(None, None, None, None, None, None, None, None, None, None, None, 0, 0, 1) == 0


def test_batch_table_arguments_are_checked_before_any_launch(zl):
    """misaligned tables (the kernel moves them in 16-byte vectors) and in-place indexing are refused on the host"""
    L = zl.lib()
    ok, bad = 0x10000, 0x10004
    one = (None, None, None, None, None, None)
    assert L.zlz4_batch_compress_fast_continue(None, *one, bad, None, None, None, 1, 16, 1) == -5
    assert L.zlz4_batch_compress_fast_continue(None, *one, ok, None, bad, None, 1, 16, 1) == -5
    assert L.zlz4_batch_compress_fast_continue(None, *one, ok, ok + 64, ok, None, 1, 16, 1) == -5
    assert L.zlz4_batch_compress_fast_continue(None, *one, None, None, None, None, 1, 16, 1) == -5
    assert L.zlz4_batch_load_dict(None, None, ok, ok, bad, ok, 1) == -5


def test_stream_calls_without_device(zl):
    """no silent CPU path: without a gfx950 device the compute steps fail loudly; the host-decided exits do not"""
    t = np.zeros(4096, np.uint32)
    L = zl.lib()
    big = 0x7E000001
    assert L.zlz4_stream_compress_fast_continue(t.ctypes.data, None, big, None, 0, 1) == -2      # :823
    assert L.zlz4_stream_compress_fast_continue(t.ctypes.data, None, 0, None, 0, 1) == 0         # :824
    assert L.zlz4_stream_compress_fast_continue(None, None, 5, None, 0, 1) == -5
    assert L.zlz4_stream_load_dict(t.ctypes.data, None, 3) == -5
    if zl.device_available():
        return
    with pytest.raises(zl.Lz4Error) as e:
        zl.Stream().loadDict(b"abcdefgh")
    assert e.value.name == "DeviceError"
    with pytest.raises(zl.Lz4Error) as e:
        zl.Stream().compressFastContinue(b"x" * 100)
    assert e.value.name == "DeviceError"


CPP = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "zlz4.hpp"
int main() {
    zlz4::Stream s;
    const unsigned char dict[] = "the quick brown fox jumps over the lazy dog";
    std::vector<unsigned char> src(300), out(400), save(8);
    for (size_t i = 0; i < src.size(); i++) src[i] = "the lazy fox "[i % 13];
    const long long n = s.loadDict(dict, sizeof dict - 1);
    zlz4::Result r = s.compressFastContinue(src.data(), src.size(), out.data(), out.size(), 1);
    zlz4::device::Blocks b{};
    zlz4::device::StreamTables t{};
    zlz4::Result q = zlz4::device::compressFastContinueBatch(nullptr, b, t, 0, 1);   // nblocks == 0
    zlz4::Result l = zlz4::device::loadDictBatch(nullptr, zlz4::device::DictBlocks{}, nullptr, nullptr, 0);
    if (!q.ok() || !l.ok()) return 1;
    if (zlz4_device_check() == 0) {
        if (n != (long long)(sizeof dict - 1) || !r.ok() || s.currentOffset != 300) return 2;
        if (s.saveDict(save.data(), save.size(), 100) != 8 || std::memcmp(save.data(), "lazy dog", 8)) return 3;
    } else {
        if (n != ZLZ4_ERR_DEVICE || r.ok() || r.error_name() != "DeviceError") return 4;
        if (s.saveDict(save.data(), save.size(), 100) != 0) return 5;
    }
    std::printf("stream mirror ok\n");
    return 0;
}
"""


def test_cpp_mirror_stream_calls_compile_link_and_run(zl, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = tmp_path / "sm.cpp"
    src.write_text(CPP)
    exe = str(tmp_path / "sm")
    libdir = os.path.dirname(zl.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, str(src), "-I", os.path.join(ROOT, "zig-lz4_amd", "csrc", "host"),
                           "-L", libdir, "-lzlz4_amd", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "stream mirror ok" in out.stdout, out.stdout + out.stderr


# ------------------------------------------------------------------ the restatements
def test_kat_hand_traced(cref):
    vs = _kat()
    assert len(vs) >= 2
    for v in vs:
        src = bytes.fromhex(v["src_hex"])
        seed = _table(v["seed"])
        want_out, want_t = bytes.fromhex(v["out_hex"]), _table(v["final"])
        r, o, t = zs.compress_fast_continue(seed, src, v["acceleration"])
        assert (r, o, t) == (v["result"], want_out, want_t), v["name"]
        r, o, t = cref.cont(seed, src, v["acceleration"])
        assert (r, o, list(t)) == (v["result"], want_out, want_t), v["name"]
    # the first vector is the point of the KAT: the seed gives a match that a fresh table misses
    assert vs[1]["seed"] == {} and vs[0]["src_hex"] == vs[1]["src_hex"] and vs[0]["out_hex"] != vs[1]["out_hex"]
    assert bytes.fromhex(vs[0]["out_hex"])[72:74] == b"\x3c\x00"         # offset 60: position 70 -> position 10


def test_zero_table_equals_oracle_compress_fast(oracle, cref):
    for i, b in enumerate(_blocks(1)):
        for a in (1, 2, 7, 64, 65537):
            want = oracle.compress_fast(b, a)
            r, o, _ = zs.compress_fast_continue([0] * 4096, b, a)
            assert o == want and r == len(want), (i, a)
            r, o, _ = cref.cont(np.zeros(4096, np.uint32), b, a)
            assert o == want and r == len(want), (i, a)


def test_restatements_agree_on_random_tables(cref):
    blocks = _blocks(2)
    for i, b in enumerate(blocks):
        L = max(len(b) - 12, 0)
        for j, t in enumerate(_tables(100 + i, 4, L)):
            for a in (1, 3):
                pr, po, pt = zs.compress_fast_continue(t, b, a)
                cr, co, ct = cref.cont(t, b, a)
                assert (pr, po) == (cr, co) and pt == [int(x) for x in ct], (i, j, a)


def test_outputs_round_trip_without_dictionary(oracle, cref):
    rng = np.random.default_rng(5)
    text = bytes(dg.text_bytes(300000, 11))
    t, _ = cref.load_dict(text[:65536])
    for k in range(40):
        n = int(rng.integers(13, 20000))
        o = int(rng.integers(65536, len(text) - n))
        b = text[o:o + n]
        r, c, t2 = cref.cont(t, b, 1)
        assert r == len(c) and oracle.decompress_safe(c, n) == b
        pr, pc, _ = zs.compress_fast_continue(list(t), b, 1)
        assert pc == c
        t = t2                                                       # a chained stream


def test_load_dict_edge_sizes(cref):
    text = bytes(dg.text_bytes(200000, 3))
    for n in DICT_SIZES:
        d = text[:n]
        pt, ps = zs.load_dict(d)
        ct, cs = cref.load_dict(d)
        assert ps == cs == min(n, 65536), n
        assert pt == [int(x) for x in ct], n
        if n <= 4:
            assert not any(pt), n                                    # 4 bytes or fewer hash nothing (:810-812)
    # last writer wins, offsets into the tail; position dictSize - 4 is not hashed (i < dictSize - MINMATCH)
    d = b"z" * 100000 + b"abcdabcd"
    pt, ps = zs.load_dict(d)
    h = lambda b4: ((int.from_bytes(b4, "little") * 2654435761) & 0xFFFFFFFF) >> 20
    assert ps == 65536 and pt[h(b"abcd")] == 65536 - 8 and pt[h(b"zzzz")] == 65536 - 8 - 4
    assert pt[h(b"dabc")] == 65536 - 8 + 3 and pt[h(b"bcda")] == 65536 - 8 + 1


def test_continue_statuses_leave_the_table(cref):
    t = list(np.random.default_rng(7).integers(0, 1 << 20, 4096))
    b = bytes(dg.text_bytes(5000, 9))
    full = len(zs.compress_fast_continue(t, b)[1])
    for src, cap, want in ((b, full - 1, -1), (b, 0, -1), (b"", 0, 0), (b"abc", 1, -1), (b"abc", 4, 4), (b"x" * 12, 13, 13)):
        r, o, t2 = zs.compress_fast_continue(t, src, 1, cap)
        cr, co, ct = cref.cont(t, src, 1, cap)
        assert r == cr == want and o == co and t2 == t and list(ct) == t, (len(src), cap)
    r, o, t2 = zs.compress_fast_continue(t, b, 1, full)
    assert r == full and t2 != t


def test_save_dict_quirks(zl):
    d = bytes(range(256)) * 300                                      # 76 800 bytes: only the last 64 KiB are kept
    assert zs.save_dict(None, 100, 100) == b""
    assert zs.save_dict(d[-65536:], 100, 0) == b""
    assert zs.save_dict(d[-65536:], 10, 100) == d[-10:]              # dictSize (100) > safeBuffer.len: the buffer's worth
    assert zs.save_dict(d[-65536:], 1000, 100) == d[-100:]
    assert zs.save_dict(d[-65536:], 1 << 20, 1 << 20) == d[-65536:]
    # the Python binding does the same bookkeeping without the device
    s = zl.Stream()
    s.dictionary = d[-65536:]
    s.dictSize = 65536
    for safe, mx in ((10, 100), (1000, 100), (1 << 17, 1 << 20), (5, 0)):
        buf = bytearray(b"\xee" * safe)
        k = s.saveDict(buf, mx)
        want = zs.save_dict(s.dictionary, safe, mx)
        assert k == len(want) and bytes(buf[:k]) == want
