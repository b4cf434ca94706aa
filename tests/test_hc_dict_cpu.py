"""The HC dictionary compressor (zlz4_compress_hc_using_dict): the public surface and the two
restatements (tools/pyref/zig_lz4_hc_dict.py, tests/hc_dict_ref.c), without a GPU."""
import ctypes as C
import hashlib
import json
import os
import re
import shutil
import struct
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "pyref"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import datagen as dg  # noqa: E402
import dictcgen as dc  # noqa: E402
import dictgen  # noqa: E402
import hcdictcgen as hg  # noqa: E402
import zig_lz4_dict as zd  # noqa: E402
import zig_lz4_hc_dict as zh  # noqa: E402

NEW = ("zlz4_compress_hc_using_dict", "zlz4_batch_compress_hc_using_dict_workspace", "zlz4_batch_compress_hc_using_dict")
GENS = (dg.text_bytes, dg.reptext_bytes, dg.mixed_bytes, dg.random_bytes)
LEVELS = (3, 4, 6, 8, 9)
DICT_LENS = (0, 1, 3, 4, 5, 100, 4096, 65535, 65536, 70000)
REC_LENS = (0, 1, 12, 13, 14, 37, 1000, 4096)


@pytest.fixture(scope="module")
def cref(tmp_path_factory):
    return hg.ref(tmp_path_factory.mktemp("hcdictcref"))


@pytest.fixture(scope="module")
def lz4lib():
    return dictgen.liblz4()


@pytest.fixture(scope="module")
def streams():
    """one stream per generator: a pair (D, n) is the D bytes in front of position 70000 and the n bytes after it"""
    return [bytes(g(70000 + 4096, 40 + k)) for k, g in enumerate(GENS)]


def _pair(s, D, n):
    return s[70000 - D:70000], s[70000:70000 + n]


def _py(r, d, level, cap=None):
    out = zh.compress_hc_using_dict(r, d, level, cap)
    return (out, b"") if isinstance(out, int) else (len(out), out)


def _check_stream(stream, r, d, lz4lib):
    """decodes to the record with both decoders; every match starts in the record, every offset is a 16-bit distance"""
    assert zd.decompress_safe_using_dict(stream, len(r), d) == (len(r), r)
    if lz4lib is not None:
        assert lz4lib(stream, len(r), d) == r
    D = min(len(d), 65536)
    for op, _, ml, off in hg.sequences(stream):
        assert 0 <= op and op + ml <= len(r) - 5 and 1 <= off <= 65535 and off <= op + D


# ------------------------------------------------------------------ surface
def test_symbols_declared_and_exported(zl):
    hdr = open(os.path.join(ROOT, "include", "zlz4_amd.h")).read()
    L = C.CDLL(zl.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in zl.SYMBOLS, name
    for name in ("compressHCUsingDict", "batch_compress_hc_using_dict_workspace", "batch_compress_hc_using_dict",
                 "compressBlocksHCUsingDict", "compressBlocksUsingDict"):
        assert callable(getattr(zl, name)), name


def test_root_zig_and_cpp_mirror_declare_the_call(zl):
    txt = open(os.path.join(ROOT, "zig-lz4_amd", "zig", "root.zig")).read()
    for name in NEW:
        assert re.search(r'^extern "c" fn %s\(' % name, txt, re.M), name
    for frag in ("pub fn compressHCUsingDict(src: []const u8, dst: []u8, dict: []const u8, compressionLevel: i32) Error!usize",
                 "pub const compressHCUsingDict = root.compressHCUsingDict;", "pub fn compressHCUsingDictBatch("):
        assert frag in txt, frag
    hpp = open(os.path.join(ROOT, "zig-lz4_amd", "csrc", "host", "zlz4.hpp")).read()
    assert "inline Result compressHCUsingDict(" in hpp and "inline Result compressHCUsingDictBatch(" in hpp


CPP = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "zlz4.hpp"
int main() {
    const unsigned char dict[] = "0123456789ABCDEF";
    const unsigned char src[] = "3456789ABCDEF";
    const unsigned char want[] = {0x04, 0x0d, 0x00, 0x50, 'B', 'C', 'D', 'E', 'F'};
    std::vector<unsigned char> out(64), back(64);
    zlz4::Result r = zlz4::compressHCUsingDict(src, sizeof src - 1, out.data(), out.size(), dict, sizeof dict - 1, 9);
    zlz4::Result e = zlz4::compressHCUsingDict(src, sizeof src - 1, out.data(), out.size(), nullptr, 4, 9);
    if (e.ok() || e.error_name() != "InvalidState") return 1;
    if (!zlz4::compressHCUsingDict(src, 0, out.data(), out.size(), dict, 16, 9).ok()) return 2;
    if (zlz4::compressHCUsingDict(src, sizeof src - 1, out.data(), out.size(), dict, 16, 2).error_name() != "Unsupported") return 8;
    if (zlz4::compressHCUsingDict(src, 0, out.data(), out.size(), dict, 16, 11).error_name() != "Unsupported") return 9;
    zlz4::device::Blocks b{};
    if (!zlz4::device::compressHCUsingDictBatch(nullptr, b, zlz4::device::DictBlocks{}, 0, 0, 9, nullptr, 0).ok()) return 3;
    b.nblocks = 1;
    if (zlz4::device::compressHCUsingDictBatch(nullptr, b, zlz4::device::DictBlocks{}, 0, 0, 9, nullptr, 0).error_name() != "InvalidState") return 4;
    if (zlz4::device::compressHCUsingDictWorkspace(1, 4096, 65536) < 13 * 69632) return 10;
    if (zlz4_device_check() == 0) {
        if (!r.ok() || r.value != sizeof want || std::memcmp(out.data(), want, sizeof want)) return 5;
        zlz4::Result d = zlz4::decompressSafeUsingDict(out.data(), r.value, back.data(), sizeof src - 1, dict, sizeof dict - 1);
        if (!d.ok() || d.value != sizeof src - 1 || std::memcmp(back.data(), src, sizeof src - 1)) return 6;
    } else {
        if (r.ok() || r.error_name() != "DeviceError") return 7;
    }
    std::printf("hc dict mirror ok\n");
    return 0;
}
"""


def test_cpp_mirror_compiles_links_and_runs(zl, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = tmp_path / "hm.cpp"
    src.write_text(CPP)
    exe = str(tmp_path / "hm")
    libdir = os.path.dirname(zl.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, str(src), "-I", os.path.join(ROOT, "zig-lz4_amd", "csrc", "host"),
                           "-L", libdir, "-lzlz4_amd", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "hc dict mirror ok" in out.stdout, "%d %s%s" % (out.returncode, out.stdout, out.stderr)


def test_calls_without_device(zl):
    """no silent CPU path: the host-decided exits answer, everything else is DeviceError without a gfx950 device"""
    L = zl.lib()
    f = L.zlz4_compress_hc_using_dict
    assert f(None, 5, None, 0, None, 3, 9) == -5                         # dict == NULL, dict_len > 0
    assert f(None, 5, None, 0, None, 3, 2) == -5                         # ... before the level
    for level in (2, 10, 11, 12, 13, 99):
        assert f(None, 5, None, 0, None, 0, level) == -8, level          # nothing is touched
        assert f(None, 0, None, 0, None, 0, level) == -8, level          # as the batch call: before the record is looked at
    assert f(None, 0x7E000001, None, 0, None, 0, 9) == -2                # :1442
    for level in (3, 9, 1, 0, -5):
        assert f(None, 0, None, 0, None, 0, level) == 0                  # :1443
    assert f(None, 5, None, 0, None, 0, 9) == -1                         # :1461
    b = L.zlz4_batch_compress_hc_using_dict
    assert b(*([None] * 11), 0, 0, 0, 9, None, 0) == 0                   # no blocks
    ok = 0x10000
    ws_bytes = L.zlz4_batch_compress_hc_using_dict_workspace(1, 16, 16)
    assert ws_bytes >= 32 * 7 and L.zlz4_batch_compress_hc_using_dict_workspace(1, 65536, 1) > L.zlz4_batch_compress_hc_using_dict_workspace(1, 65535, 1) * 3 // 2
    args = [None] + [ok] * 10
    tail = lambda level=9, ws=ok, wb=ws_bytes: (1, 16, 16, level, ws, wb)
    assert b(*([None] * 11), *tail()) == -5
    for k, v in ((10, ok + 4), (10, None), (1, None), (4, None), (7, None), (8, None), (9, None), (2, ok + 4), (6, ok + 2),
                 (3, ok + 2), (9, ok + 1)):
        a = list(args)
        a[k] = v
        assert b(*a, *tail()) == -5, k
    for level in (2, 10, 12, 40):
        assert b(*args, *tail(level=level)) == -8, level
    assert b(*args, *tail(ws=None)) == -5 and b(*args, *tail(ws=ok + 8)) == -5 and b(*args, *tail(wb=ws_bytes - 1)) == -5
    a = list(args)
    a[7] = None                                       # no dictionary arena is fine when max_dict_len == 0
    if zl.device_available():
        return
    assert b(*a, 1, 16, 0, 9, ok, ws_bytes) == zl.ERR_DEVICE
    assert b(*args, *tail()) == zl.ERR_DEVICE and b(*args, *tail(level=1)) == zl.ERR_DEVICE
    with pytest.raises(zl.Lz4Error) as e:
        zl.compressHCUsingDict(b"x" * 100, b"abcdefgh", 9)
    assert e.value.name == "DeviceError"
    with pytest.raises(zl.Lz4Error) as e:
        zl.compressHCUsingDict(b"x" * 100, b"abcdefgh", 10)
    assert e.value.name == "Unsupported"


# ------------------------------------------------------------------ the two restatements
def _caps(s, n):
    return sorted({max(c, 0) for c in (s, s - 1, 0, hg.bound(n), s // 2)})


def test_the_c_restatement_over_the_full_grid(cref, lz4lib, streams):
    """bytes, statuses and capacities; every stream decodes; the Python leg runs on the part of the grid it can afford"""
    for k, s in enumerate(streams):
        for D in DICT_LENS:
            for n in REC_LENS:
                d, r = _pair(s, D, n)
                for level in LEVELS:
                    size, out = cref.compress(r, d, level)
                    assert size == (0 if n == 0 else len(out)) and size <= hg.bound(n)
                    if n:
                        _check_stream(out, r, d, lz4lib)
                    for cap in _caps(size, n):
                        got = cref.compress(r, d, level, cap)
                        assert got == ((size, out) if cap >= size or n == 0 else (hg.OUTPUT_TOO_SMALL, b"")), (k, D, n, level, cap)
                    assert cref.compress(r, d, level, hg.bound(n))[0] != hg.OUTPUT_TOO_SMALL


def test_pyref_equals_the_c_restatement(cref, streams):
    """the Python leg: every length pair at levels 3 and 6 on two generators, level 9 and the capacities on the pairs that
    Python does in about a minute altogether"""
    for k, s in enumerate(streams):
        for D in DICT_LENS:
            for n in REC_LENS:
                d, r = _pair(s, D, n)
                levels = LEVELS if (D <= 4096 and n <= 1000) or (k == 0 and n in (13, 4096) and D in (65536, 70000)) else \
                    (3, 6) if k in (0, 2) and n <= 1000 else (3,) if n <= 37 else ()
                for level in levels:
                    want = cref.compress(r, d, level)
                    assert _py(r, d, level) == want, (k, D, n, level)
                    if n <= 37 or D <= 100:
                        for cap in _caps(want[0], n):
                            assert _py(r, d, level, cap) == cref.compress(r, d, level, cap), (k, D, n, level, cap)
    for level in (2, 10, 11, 12, 13):
        assert _py(b"x" * 20, b"abc", level) == cref.compress(b"x" * 20, b"abc", level) == (hg.UNSUPPORTED, b"")
        assert _py(b"", b"abc", level) == cref.compress(b"", b"abc", level) == (hg.UNSUPPORTED, b"")
    assert cref.compress(b"x" * 20, None, 9) == _py(b"x" * 20, None, 9)
    assert cref.L.hd_compress(None, 5, None, 0, None, 3, 2) == hg.INVALID_STATE


def test_empty_dictionary_equals_compress_hc(cref, oracle):
    """bytes and status of compressHC for levels 3..9 and for level 1 (which becomes 9), on the oracle tests' inputs"""
    import cases
    inputs = [b for _, b in cases.reference_test_inputs() + list(cases.kat_inputs().items()) + cases.seeded_cases()]
    inputs = [bytes(b) for b in inputs if len(b) <= 300000]
    for k, gen in enumerate(GENS):
        inputs += [bytes(gen(n, 60 + k)) for n in (1, 12, 13, 14, 100, 4096, 20000)]
    inputs += [b"", b"a" * 300, b"abcabcabcabcd", bytes(70000)]
    for src in inputs:
        for level in (1, 3, 4, 5, 6, 7, 8, 9):
            want = oracle.compress_hc(src, level)
            assert cref.compress(src, b"", level) == (len(want), want), (len(src), level)
            assert cref.compress(src, None, level) == (len(want), want)
            if len(src) <= 4096 and level in (1, 3, 6):
                assert _py(src, b"", level) == (len(want), want)
        if 13 <= len(src) <= 4096:
            s = len(oracle.compress_hc(src, 9))
            for cap in (s - 1, s // 2, 0):
                exp = oracle.compress_hc_expected(src, 9, cap)
                assert exp == hg.OUTPUT_TOO_SMALL and cref.compress(src, b"", 9, cap)[0] == exp


def test_the_dictionary_is_used(cref):
    """the six 4 KiB D-text records of DESIGN.md section 4.3c against the 65 536 bytes in front of them"""
    s = bytes(dg.text_bytes(65536 + 6 * 4096, 77))
    d = s[:65536]
    recs = [s[65536 + i * 4096:65536 + (i + 1) * 4096] for i in range(6)]
    fast = dc.ref(os.path.dirname(cref.L._name))
    total = {lv: sum(cref.compress(r, d, lv)[0] for r in recs) for lv in (3, 6, 9)}
    assert total == {3: 7835, 6: 6565, 9: 6304}
    assert {lv: sum(cref.compress(r, d[-61440:], lv)[0] for r in recs) for lv in (3, 6, 9)} == {3: 7862, 6: 6609, 9: 6347}
    without = sum(cref.compress(r, b"", 9)[0] for r in recs)
    fast_dict = sum(fast.compress(r, d)[0] for r in recs)
    assert (without, fast_dict) == (15556, 10658)
    assert total[9] < without and total[9] < fast_dict
    assert sum(_py(r, d, 3)[0] for r in recs[:2]) == sum(cref.compress(r, d, 3)[0] for r in recs[:2])
    d4 = d[-4096:]                                    # the 4 KiB in front of the records
    assert {lv: sum(cref.compress(r, d4, lv)[0] for r in recs) for lv in (3, 6, 9)} == {3: 12157, 6: 11628, 9: 11583}
    assert sum(fast.compress(r, d4)[0] for r in recs) == 13379


def test_crafted_cases_are_what_they_claim(cref, lz4lib):
    for name, d, r in hg.crafted():
        for level in (3, 4, 8, 9):
            size, out = cref.compress(r, d, level)
            assert _py(r, d, level) == (size, out), (name, level)
            _check_stream(out, r, d, lz4lib)
    by = {name: (d, r) for name, d, r in hg.crafted()}
    seqs = lambda name, level: hg.sequences(cref.compress(by[name][1], by[name][0], level)[1])
    assert seqs("thirteen_bytes", 9) == [(0, 0, 8, 250)] and cref.compress(by["thirteen_bytes"][1], by["thirteen_bytes"][0], 9)[0] == 9
    assert seqs("only_at_v_pos_0", 9) == [] and seqs("at_v_pos_1", 9) == [(30, 30, 4, 130)]
    assert seqs("offset_65535_only", 9) == [(19, 19, 60, 65535)] and seqs("offset_65536_none", 9) == []
    assert {op: ml for op, _, ml, _ in seqs("attempt_budget", 3)}[28] == 4
    assert {op: ml for op, _, ml, _ in seqs("attempt_budget", 4)}[28] == 23
    assert seqs("pattern_into_tail", 9)[1] == (301, 1, 350, 351) and seqs("pattern_into_tail", 8)[1] == (301, 1, 129, 130)


def test_known_answers(cref):
    import gen_hc_dict_kat as gk
    vectors = json.load(open(os.path.join(ROOT, "tests", "golden", "hc_dict_kat.json")))["vectors"]
    assert len(vectors) >= 30
    names = {v["name"] for v in vectors}
    assert {"thirteen_bytes", "v_pos_0", "v_pos_1", "attempt_budget_l3", "pattern_into_tail_l9"} <= names
    for v in vectors:
        if "gen" in v:
            d, src = gk.generated(v["gen"], v["seed"], v["dict_len"], v["n"])
        else:
            d, src = bytes.fromhex(v["dict"]), bytes.fromhex(v["src"])
        for got in (_py(src, d, v["level"], v["dst_cap"]), cref.compress(src, d, v["level"], v["dst_cap"])):
            assert got[0] == v["result"], v["name"]
            if "out" in v:
                assert got[1].hex() == v["out"], v["name"]
            else:
                assert hashlib.sha256(got[1]).hexdigest() == v["sha256"], v["name"]


def test_the_c_restatement_under_sanitizers(cref, tmp_path, streams):
    """tests/hc_dict_ref.c + its driver as a program built with -fsanitize=address,undefined: the crafted cases, the
    capacities around each size and the length grid's corners, every buffer a heap block of exactly its size"""
    cc = shutil.which("cc")
    exe = str(tmp_path / "hd_asan")
    build = subprocess.run([cc, "-O1", "-g", "-std=c11", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                            hg.SRC, os.path.join(ROOT, "tests", "hc_dict_ref_driver.c")], capture_output=True, text=True) if cc else None
    if build is None or build.returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime")
    cases = []
    for name, d, r in hg.crafted():
        for level in (3, 8, 9):
            s = cref.compress(r, d, level)[0]
            cases += [(level, cap, d, r) for cap in (hg.bound(len(r)), s, s - 1, s // 2, 0)]
    for D in (0, 1, 4, 65535, 65536, 70000):
        for n in (1, 12, 13, 14, 4096):
            d, r = _pair(streams[0], D, n)
            cases.append((9, hg.bound(n), d, r))
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        for level, cap, d, r in cases:
            f.write(struct.pack("<IIII", level, cap, len(d), len(r)) + d + r)
    run = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = run.stdout.split()
    assert len(lines) == 2 * len(cases)
    for k, (level, cap, d, r) in enumerate(cases):
        size, out = cref.compress(r, d, level, cap)
        h = 2166136261
        for b in out:
            h = ((h ^ b) * 16777619) & 0xFFFFFFFF
        assert (int(lines[2 * k]), lines[2 * k + 1]) == (size, "%08x" % h), k
