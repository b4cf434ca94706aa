"""Dictionary decoding (lz4.decompressSafeUsingDict / decompressSafePartialUsingDict, src/lz4.zig:960-969): the public
surface and the test infrastructure, without a GPU."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dictgen  # noqa: E402
import zig_lz4_dict as pd  # noqa: E402

NEW = ("zlz4_decompress_safe_using_dict", "zlz4_decompress_safe_partial_using_dict",
       "zlz4_batch_decompress_safe_using_dict")


def test_dict_symbols_declared_and_exported(zl):
    hdr = open(os.path.join(ROOT, "include", "zlz4_amd.h")).read()
    L = C.CDLL(zl.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in zl.SYMBOLS, name


def test_root_zig_declares_dict_functions(zl):
    txt = open(os.path.join(ROOT, "zig-lz4_amd", "zig", "root.zig")).read()
    assert re.search(r"^pub fn decompressSafeUsingDict\(src: \[\]const u8, dst: \[\]u8, dict: \[\]const u8\) Error!usize",
                     txt, re.M)
    assert re.search(r"^pub fn decompressSafePartialUsingDict\(src: \[\]const u8, dst: \[\]u8, targetOutputSize: usize, "
                     r"dict: \[\]const u8\) Error!usize", txt, re.M)
    assert "pub const decompressSafeUsingDict = root.decompressSafeUsingDict;" in txt
    assert "pub const decompressSafeUsingDictBatch = root.decompressSafeUsingDictBatch;" in txt
    L = C.CDLL(zl.LIB_PATH)
    for fn in re.findall(r'^extern "c" fn (\w+)\(', txt, re.M):
        assert hasattr(L, fn), "root.zig binds %s, which the library does not export" % fn
    for name in NEW:
        assert re.search(r'^extern "c" fn %s\(' % name, txt, re.M), name


def test_dict_calls_without_device_or_trivially(zl):
    # :97 / :98 / :99 are decided before any device work
    assert zl.decompressSafeUsingDict(b"", 10, b"abc") == b""
    assert zl.decompressSafeUsingDict(b"\x10a", 0, b"abc") == b""
    with pytest.raises(zl.Lz4Error) as e:
        zl.decompressSafePartialUsingDict(b"\x10a", 4, 5, b"abc")
    assert e.value.name == "OutputTooSmall"


CPP = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "zlz4.hpp"
int main() {
    const unsigned char dict[] = "0123456789abcdef";
    // literals "xy", then 8 bytes at offset 2 + 16 (the whole dictionary's first half), then 5 literals
    const unsigned char src[] = {0x24, 'x', 'y', 18, 0, 0x50, 'E', 'N', 'D', '!', '!'};
    std::vector<unsigned char> out(64);
    zlz4::Result r = zlz4::decompressSafeUsingDict(src, sizeof src, out.data(), out.size(), dict, 16);
    zlz4::Result p = zlz4::decompressSafePartialUsingDict(src, sizeof src, out.data(), out.size(), 0, dict, 16);
    zlz4::device::Blocks b{};
    zlz4::device::DictBlocks d{};
    zlz4::Result q = zlz4::device::decompressSafeUsingDictBatch(nullptr, b, d);   // nblocks == 0
    if (zlz4_device_check() == 0) {
        if (!r.ok() || r.value != 15 || std::memcmp(out.data(), "xy01234567END!!", 15)) return 1;
        if (p.ok() || p.error_name() != "OutputTooSmall") return 2;
        if (!q.ok()) return 3;
    } else {
        if (r.ok() || r.error_name() != "DeviceError") return 4;
        if (p.ok() || p.error_name() != "OutputTooSmall") return 5;   // target == 0: decided on the host
        if (q.ok() || q.error_name() != "DeviceError") return 6;
    }
    std::printf("dict mirror ok\n");
    return 0;
}
"""


def test_cpp_mirror_dict_calls_compile_link_and_run(zl, tmp_path):
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
    assert out.returncode == 0 and "dict mirror ok" in out.stdout, out.stdout + out.stderr


# ------------------------------------------------------------------ the Python restatement
def _status(o):
    return o if isinstance(o, int) else len(o)


def _fuzz_streams():
    """compressed fuzz inputs of tools/fuzz_parity.py, whole and damaged (truncated, flipped bytes)"""
    import fuzz_parity as fp
    from oracle import binding as ob
    rng = np.random.default_rng(2024)
    out = []
    for n in (13, 64, 200, 1000, 4096, 20000, 65536):
        for _ in range(3):
            b = fp.make_input(rng, n)
            c = ob.compress_default(b)
            out.append((c, len(b)))
            out.append((c[:int(rng.integers(0, len(c)))], len(b)))
            m = bytearray(c)
            for _ in range(int(rng.integers(1, 4))):
                m[int(rng.integers(0, len(m)))] = int(rng.integers(0, 256))
            out.append((bytes(m), len(b)))
            out.append((c, max(0, len(b) - int(rng.integers(1, 40)))))
    return out


def _golden_streams():
    d = json.load(open(os.path.join(ROOT, "tests", "golden", "kat_appendix_b.json")))
    out = []
    for v in d["vectors"]:
        if v.get("hex"):
            c = bytes.fromhex(v["hex"])
            out += [(c, 4096), (c, 3), (c[:-1], 4096)]
    return out


def test_pyref_empty_dict_equals_oracle_decompress_safe(oracle):
    streams = _fuzz_streams() + _golden_streams()
    assert len(streams) > 80
    for c, cap in streams:
        want = oracle.decompress_safe(c, cap)
        for dct in (b"", None):
            r, got = pd.decompress_safe_using_dict(c, cap, dct)
            assert r == _status(want), (len(c), cap, r, want if isinstance(want, int) else len(want))
            if r > 0:
                assert got == want
        # partial with target == cap is the same call
        assert pd.decompress_safe_partial_using_dict(c, cap, cap, b"")[0] == _status(want)


def test_pyref_crafted_cases_statuses():
    seen = {}
    for name, s, dct, cap, target in dictgen.crafted_cases():
        t = cap if target is None else target
        r, got = pd.decompress_generic(s, cap, t, dct)
        seen[name] = r
    assert seen["dl0_first"] == 28 and seen["dl0_beyond"] == -3 and seen["dl1_first"] == 10 + 4 + 14 and seen["dl1_beyond"] == -3
    assert seen["dl65536_off65535"] > 0 and seen["dl65535_off65535"] > 0
    assert seen["dl4_ots_over_corrupt"] == -1
    assert seen["dl200000_partial0"] == -1 and seen["dl200000_partial27"] == -1 and seen["dl200000_partial200"] > 0
    assert seen["dl200000_src0"] == 0 and seen["dl200000_cap0"] == 0


def test_encoder_streams_round_trip_through_pyref_and_liblz4(tmp_path):
    if shutil.which("cc") is None:
        pytest.skip("no cc")
    import datagen as dg
    enc = dictgen.encoder(tmp_path)
    lz = dictgen.liblz4()
    text = bytes(dg.text_bytes(400000, 77))
    cases = [(text[:65536], text[70000 + 4096 * k: 70000 + 4096 * (k + 1)]) for k in range(6)]
    cases += [(text[:200000], text[200000:265536]), (b"", text[:5000]), (b"abc", b"abcabcabcabcabcabcabcabc0123456789"),
              (b"xyzw" * 10, b"xyzw" * 50 + b"tail-literals")]
    tot = [0, 0, 0, 0]
    for dct, blk in cases:
        s, st = enc(dct, blk)
        tot = [a + b for a, b in zip(tot, st)]
        r, got = pd.decompress_safe_using_dict(s, len(blk), dct)
        assert r == len(blk) and got == blk
        if lz is not None:
            assert lz(s, len(blk), dct) == blk
        if dct:   # the stream really needs its dictionary
            assert pd.decompress_safe_using_dict(s, len(blk), b"")[0] < 0 or st[0] == 0
    assert tot[2] > 0 and tot[3] > 0, tot        # wholly-in-dict and spanning matches were produced


def test_pyref_equals_liblz4_on_crafted_and_damaged_streams(tmp_path):
    lz = dictgen.liblz4()
    if lz is None:
        pytest.skip("liblz4 not present")
    import datagen as dg
    rng = np.random.default_rng(5)
    enc = dictgen.encoder(tmp_path)
    text = bytes(dg.text_bytes(300000, 3))
    n_cmp = 0
    for name, s, dct, cap, target in dictgen.crafted_cases():
        if target is not None or not s or cap == 0:
            continue
        r, got = pd.decompress_safe_using_dict(s, cap, dct)
        want = lz(s, cap, dct)
        # liblz4 accepts any stream the reference accepts; where both decode, the bytes agree
        if r >= 0 and want is not None:
            assert got == want, name
            n_cmp += 1
    for k in range(20):
        dct, blk = text[:65536], text[65536 + 4096 * k: 65536 + 4096 * (k + 1)]
        s, _ = enc(dct, blk)
        m = bytearray(s)
        m[int(rng.integers(0, len(m)))] ^= 1 << int(rng.integers(0, 8))
        r, got = pd.decompress_safe_using_dict(bytes(m), len(blk), dct)
        want = lz(bytes(m), len(blk), dct)
        if r >= 0 and want is not None:
            assert got == want
            n_cmp += 1
    assert n_cmp > 20
