"""The dictionary compressor (zlz4_compress_fast_using_dict): the public surface and the two
restatements (tools/pyref/zig_lz4_dict_compress.py, tests/dict_compress_ref.c), without a GPU."""
import ctypes as C
import hashlib
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
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import datagen as dg  # noqa: E402
import dictcgen as dc  # noqa: E402
import dictgen  # noqa: E402
import zig_lz4_dict as zd  # noqa: E402
import zig_lz4_dict_compress as zc  # noqa: E402

NEW = ("zlz4_compress_fast_using_dict", "zlz4_batch_compress_fast_using_dict")
GENS = (dg.text_bytes, dg.reptext_bytes, dg.mixed_bytes, dg.random_bytes)


@pytest.fixture(scope="module")
def cref(tmp_path_factory):
    return dc.ref(tmp_path_factory.mktemp("dictcref"))


@pytest.fixture(scope="module")
def lz4lib():
    return dictgen.liblz4()


def _pairs():
    """(dictionary, record): the record continues the generator's stream after the dictionary, so that it has matches there"""
    out = []
    for k, gen in enumerate(GENS):
        for dl in (0, 100, 4096, 65536, 70000):
            s = bytes(gen(dl + 4096, 40 + k))
            for n in (12, 13, 37, 1000, 4096):
                out.append((s[:dl], s[dl:dl + n]))
    return out


def _decodes(stream, n, d, lz4lib):
    assert zd.decompress_safe_using_dict(stream, n, d)[0] == n
    if lz4lib is not None:                            # the optional cross-check
        return lz4lib(stream, n, d)
    return zd.decompress_safe_using_dict(stream, n, d)[1]


# ------------------------------------------------------------------ surface
def test_symbols_declared_and_exported(zl):
    hdr = open(os.path.join(ROOT, "include", "zlz4_amd.h")).read()
    L = C.CDLL(zl.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in zl.SYMBOLS, name
    for name in ("compressFastUsingDict", "batch_compress_fast_using_dict", "compressBlocksUsingDict"):
        assert callable(getattr(zl, name)), name


def test_root_zig_and_cpp_mirror_declare_the_call(zl):
    txt = open(os.path.join(ROOT, "zig-lz4_amd", "zig", "root.zig")).read()
    for name in NEW:
        assert re.search(r'^extern "c" fn %s\(' % name, txt, re.M), name
    for frag in ("pub fn compressFastUsingDict(src: []const u8, dst: []u8, dict: []const u8, acceleration: u32) Error!usize",
                 "pub const compressFastUsingDict = root.compressFastUsingDict;", "pub fn compressFastUsingDictBatch("):
        assert frag in txt, frag
    hpp = open(os.path.join(ROOT, "zig-lz4_amd", "csrc", "host", "zlz4.hpp")).read()
    assert "inline Result compressFastUsingDict(" in hpp and "inline Result compressFastUsingDictBatch(" in hpp


CPP = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "zlz4.hpp"
int main() {
    const unsigned char dict[] = "0123456789ABCDEF";
    const unsigned char src[] = "xy3456789qrstuvwxyz";
    const unsigned char want[] = {0x23, 'x', 'y', 0x0f, 0x00, 0xa0, 'q', 'r', 's', 't', 'u', 'v', 'w', 'x', 'y', 'z'};
    std::vector<unsigned char> out(64), back(64);
    zlz4::Result r = zlz4::compressFastUsingDict(src, sizeof src - 1, out.data(), out.size(), dict, sizeof dict - 1);
    zlz4::Result e = zlz4::compressFastUsingDict(src, sizeof src - 1, out.data(), out.size(), nullptr, 4);
    if (e.ok() || e.error_name() != "InvalidState") return 1;
    if (!zlz4::compressFastUsingDict(src, 0, out.data(), out.size(), dict, 16).ok()) return 2;
    zlz4::device::Blocks b{};
    if (!zlz4::device::compressFastUsingDictBatch(nullptr, b, zlz4::device::DictBlocks{}, nullptr, nullptr, 0, 0).ok()) return 3;
    b.nblocks = 1;
    if (zlz4::device::compressFastUsingDictBatch(nullptr, b, zlz4::device::DictBlocks{}, nullptr, nullptr, 0, 0).error_name() != "InvalidState") return 4;
    if (zlz4_device_check() == 0) {
        if (!r.ok() || r.value != sizeof want || std::memcmp(out.data(), want, sizeof want)) return 5;
        zlz4::Result d = zlz4::decompressSafeUsingDict(out.data(), r.value, back.data(), sizeof src - 1, dict, sizeof dict - 1);
        if (!d.ok() || d.value != sizeof src - 1 || std::memcmp(back.data(), src, sizeof src - 1)) return 6;
    } else {
        if (r.ok() || r.error_name() != "DeviceError") return 7;
    }
    std::printf("dict compress mirror ok\n");
    return 0;
}
"""


def test_cpp_mirror_compiles_links_and_runs(zl, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = tmp_path / "dm.cpp"
    src.write_text(CPP)
    exe = str(tmp_path / "dm")
    libdir = os.path.dirname(zl.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, str(src), "-I", os.path.join(ROOT, "zig-lz4_amd", "csrc", "host"),
                           "-L", libdir, "-lzlz4_amd", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "dict compress mirror ok" in out.stdout, "%d %s%s" % (out.returncode, out.stdout, out.stderr)


def test_calls_without_device(zl):
    """no silent CPU path: the host-decided exits answer, everything else is DeviceError without a gfx950 device"""
    L = zl.lib()
    assert L.zlz4_compress_fast_using_dict(None, 5, None, 0, None, 3, 1) == -5                   # dict == NULL, dict_len > 0
    assert L.zlz4_compress_fast_using_dict(None, 0x7E000001, None, 0, None, 0, 1) == -2          # :823
    assert L.zlz4_compress_fast_using_dict(None, 0, None, 0, None, 0, 1) == 0                    # :824
    assert L.zlz4_batch_compress_fast_using_dict(*([None] * 13), 0, 0, 0, 1) == 0                # no blocks
    ok, bad = 0x10000, 0x10004
    args = [None] + [ok] * 12
    assert L.zlz4_batch_compress_fast_using_dict(*([None] * 13), 1, 16, 16, 1) == -5
    for k, v in ((10, bad), (10, None), (1, None), (7, None), (8, None), (9, None), (12, None), (2, ok + 4), (6, ok + 2)):
        a = list(args)
        a[k] = v
        assert L.zlz4_batch_compress_fast_using_dict(*a, 1, 16, 16, 1) == -5, k
    a = list(args)
    a[7] = None                                       # no dictionary arena is fine when max_dict_len == 0
    if zl.device_available():
        return
    assert L.zlz4_batch_compress_fast_using_dict(*a, 1, 16, 0, 1) == zl.ERR_DEVICE
    assert L.zlz4_batch_compress_fast_using_dict(*args, 1, 16, 16, 1) == zl.ERR_DEVICE
    with pytest.raises(zl.Lz4Error) as e:
        zl.compressFastUsingDict(b"x" * 100, b"abcdefgh")
    assert e.value.name == "DeviceError"


# ------------------------------------------------------------------ the two restatements
def test_pyref_equals_the_c_restatement_and_decodes(cref, lz4lib):
    for d, r in _pairs():
        for accel in ((1, 8) if len(r) <= 1000 else (1,)):
            want = zc.compress_fast_using_dict(r, d, accel)
            assert cref.compress(r, d, accel) == want, (len(d), len(r), accel)
            assert want[0] <= dc.bound(len(r))
            assert _decodes(want[1], len(r), d, lz4lib) == r
            assert cref.compress(r, d, accel, cap=want[0]) == want
            assert cref.compress(r, d, accel, cap=want[0] - 1)[0] == -1
            if accel == 8 and len(r) <= 1000:
                assert zc.compress_fast_using_dict(r, d, accel, dst_cap=want[0]) == want
                assert zc.compress_fast_using_dict(r, d, accel, dst_cap=want[0] - 1)[0] == -1


def test_fuzzed_pairs(cref, lz4lib):
    rng = np.random.default_rng(5)
    for it in range(150):
        dl = int(rng.choice([0, int(rng.integers(1, 9)), int(rng.integers(9, 600)), int(rng.integers(65000, 66000))],
                            p=[0.1, 0.2, 0.6, 0.1]))
        n = int(rng.integers(0, 700))
        d = bytes(GENS[it % 4](dl, 900 + it))
        fresh = bytes(GENS[(it // 4) % 4](n + 1, 1900 + it))
        parts, left = [], n
        while left > 0:
            take = int(rng.integers(1, 60))
            s = int(rng.integers(0, max(1, len(d))))
            parts.append(d[s:s + take] if len(d) > 4 and rng.random() < 0.5 else fresh[left:left + take])
            left -= max(1, len(parts[-1]))
        r = b"".join(parts)[:n]
        accel = int(rng.choice([1, 1, 2, 8, 65, 65537]))
        want = zc.compress_fast_using_dict(r, d, accel)
        assert cref.compress(r, d, accel) == want, it
        if len(r):
            assert _decodes(want[1], len(r), d, lz4lib) == r
        cap = int(rng.integers(0, want[0] + 2))
        assert cref.compress(r, d, accel, cap=cap) == zc.compress_fast_using_dict(r, d, accel, dst_cap=cap), (it, cap)


def test_empty_dictionary_equals_compress_fast(cref, oracle):
    for k, gen in enumerate(GENS):
        for n in (13, 14, 100, 4096, 20000):
            src = bytes(gen(n, 60 + k))
            for accel in (1, 8, 65537):
                want = oracle.compress_fast(src, accel)
                assert zc.compress_fast_using_dict(src, b"", accel) == (len(want), want)
                assert cref.compress(src, b"", accel) == (len(want), want)
                # D == 0 with an all-zero table, whatever the dictionary argument's table would be
                assert cref.compress(src, b"", accel, table=np.zeros(4096, np.uint32)) == (len(want), want)


def test_garbage_tables_still_round_trip(cref, lz4lib):
    rng = np.random.default_rng(9)
    for k, (d, r) in enumerate(_pairs()):
        if len(r) < 13:
            continue
        D = min(len(d), 65536)
        t = (rng.integers(0, 1 << 32, 4096, dtype=np.uint64).astype(np.uint32) if k % 3 == 0 else
             rng.integers(0, D + len(r) + 20, 4096).astype(np.uint32) if k % 3 == 1 else
             np.clip(D - rng.integers(-4, 6, 4096), 0, None).astype(np.uint32))
        got = cref.compress(r, d, table=t)
        assert got == zc.compress_fast_using_dict(r, d, table=[int(x) for x in t])
        assert 0 < got[0] <= dc.bound(len(r))
        assert _decodes(got[1], len(r), d, lz4lib) == r


def test_known_answers(cref):
    import gen_dict_compress_kat as gk
    vectors = json.load(open(os.path.join(ROOT, "tests", "golden", "dict_compress_kat.json")))["vectors"]
    assert len(vectors) >= 30
    names = {v["name"] for v in vectors}
    assert {"empty_dict", "wholly_in_dict", "spans_dict_end", "first_byte_match", "dict_pos_0"} <= names
    for v in vectors:
        if "gen" in v:
            d, src = gk.generated(v["gen"], v["seed"], v["dict_len"], v["n"])
        else:
            d, src = bytes.fromhex(v["dict"]), bytes.fromhex(v["src"])
        for got in (zc.compress_fast_using_dict(src, d, v["acceleration"], v["dst_cap"]),
                    cref.compress(src, d, v["acceleration"], cap=v["dst_cap"])):
            assert got[0] == v["result"], v["name"]
            if "out" in v:
                assert got[1].hex() == v["out"], v["name"]
            else:
                assert hashlib.sha256(got[1]).hexdigest() == v["sha256"], v["name"]


def test_crafted_cases_are_what_they_claim(cref):
    by = {n: (d, r) for n, d, r in dc.crafted(cref)}

    def run(name):
        s = np.zeros(2, np.uint64)
        sz, out = cref.compress(by[name][1], by[name][0], stats=s)
        return sz, out, int(s[0]), int(s[1])
    plain = lambda name: cref.compress(by[name][1], b"")[0]
    sz, out, from_dict, total = run("equals_tail_4k")
    assert sz < 100 and from_dict > 4000               # one long match out of the dictionary
    sz, out, from_dict, total = run("offset_65535_only")
    assert b"\xff\xff" in out and from_dict == total == 60
    sz, out, from_dict, total = run("offset_65536_none")
    assert total == 0 and sz == plain("offset_65536_none")
    sz, out, from_dict, total = run("only_at_dict_pos_0")
    assert total == 0                                  # position 0 of V is never matchable
    assert run("at_dict_pos_1")[2:] == (4, 4)
    sz, out, from_dict, total = run("first_byte_starts_match")
    assert out[0] >> 4 == 0 and from_dict == 70
    assert run("match_ends_at_dict_end")[2:] == (40, 40)
    assert run("match_spans_dict_end")[2:] == (40, 80)
    sz, out, from_dict, total = run("period_from_dict")
    assert total == 3000 and 0 < from_dict < 10
    sz, out, from_dict, total = run("one_byte_dict_64k")
    assert from_dict > 0 and sz < plain("one_byte_dict_64k")


def test_dictionary_gains_ratio_on_text(cref):
    """4 KiB D-text records against a 64 KiB dictionary of the same text: strictly smaller than without"""
    s = bytes(dg.text_bytes(65536 + 6 * 4096, 3))
    d = s[:65536]
    recs = [s[65536 + i * 4096: 65536 + (i + 1) * 4096] for i in range(6)]
    with_dict = sum(cref.compress(r, d)[0] for r in recs)
    without = sum(cref.compress(r, b"")[0] for r in recs)
    assert with_dict < without
    assert with_dict == sum(zc.compress_fast_using_dict(r, d)[0] for r in recs)
