"""Decompressed-size queries (zlz4_decompressed_size, zlz4_batch_decompressed_size, zlz4_batch_plan_outputs,
zlz4f_*frame_decompressed_size): the public surface and the Python restatement tools/pyref/zig_lz4_sizes.py, without a
GPU.  The restatement is held against the oracle (blocks, frames) and against tools/pyref/zig_lz4_dict.py
(dictionaries); the GPU tests hold the kernels against the restatement."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "pyref"))
import sizegen  # noqa: E402
import zig_lz4_dict as pd  # noqa: E402
import zig_lz4_sizes as ps  # noqa: E402

NEW = ("zlz4_decompressed_size", "zlz4_batch_decompressed_size", "zlz4_batch_plan_outputs",
       "zlz4f_frame_decompressed_size", "zlz4f_batch_frame_decompressed_size_workspace",
       "zlz4f_batch_frame_decompressed_size")
OTS, CORRUPT = -1, -3


def _status(o):
    return o if isinstance(o, int) else len(o)


# ------------------------------------------------------------------ surface
def test_size_symbols_declared_exported_and_bound(zl):
    hdr = open(os.path.join(ROOT, "include", "zlz4_amd.h")).read()
    L = C.CDLL(zl.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in zl.SYMBOLS, name
    for fn in ("decompressedSize", "batch_decompressed_size", "batch_plan_outputs", "decompressBlocks"):
        assert callable(getattr(zl, fn)), fn
    for fn in ("frameDecompressedSize", "frameDecompressedSizeBatch", "frameDecompressedSizeBatchWorkspace"):
        assert callable(getattr(zl.lz4f, fn)), fn


def test_root_zig_and_cpp_mirror_declare_the_size_calls(zl):
    txt = open(os.path.join(ROOT, "zig-lz4_amd", "zig", "root.zig")).read()
    L = C.CDLL(zl.LIB_PATH)
    for name in NEW:
        assert re.search(r'^extern "c" fn %s\(' % name, txt, re.M), name
    for fn in re.findall(r'^extern "c" fn (\w+)\(', txt, re.M):
        assert hasattr(L, fn), "root.zig binds %s, which the library does not export" % fn
    for decl in ("pub fn decompressedSize(src: []const u8, dict_len: usize) Error!usize", "pub fn decompressedSizeBatch(",
                 "pub fn planOutputs(", "pub fn frameDecompressedSize(src: []const u8) Error!usize",
                 "pub fn frameDecompressedSizeBatch(", "pub fn frameDecompressedSizeBatchWorkspace("):
        assert decl in txt, decl
    hpp = open(os.path.join(ROOT, "zig-lz4_amd", "csrc", "host", "zlz4.hpp")).read()
    for name in NEW:
        assert name + "(" in hpp, name


def test_workspace_size_and_misuse_without_a_device(zl):
    L = zl.lib()
    ws = zl.lz4f.frameDecompressedSizeBatchWorkspace
    assert ws(0, 0) >= 0 and ws(10, 100) > ws(10, 10) > 0 and ws(100, 10) > ws(10, 10)
    assert ws(10, 100) < zl.lz4f.decompressFrameBatchWorkspace(10, 100)      # fewer tables than the decoder's
    # decided before any device work: empty batches, empty input, bad alignment values, null arrays
    assert L.zlz4_batch_decompressed_size(None, None, None, None, None, None, 0) == 0
    assert L.zlz4f_batch_frame_decompressed_size(None, None, None, None, None, 0, 0, None, 0) == 0
    assert zl.decompressedSize(b"") == 0 and zl.decompressedSize(b"", 7) == 0
    buf = (C.c_uint64 * 10)()
    p = (C.addressof(buf) + 15) & ~15                  # 16-byte aligned, 64 bytes behind it
    for align in (3, 6, 24, 8192, 4097, 0x80000000):
        assert L.zlz4_batch_plan_outputs(None, p, 1, align, p, p, p) == -5, align
    assert L.zlz4_batch_plan_outputs(None, p, 1, 16, p, p, None) == -5
    assert L.zlz4_batch_plan_outputs(None, None, 1, 16, p, p, p) == -5
    assert L.zlz4_batch_plan_outputs(None, p + 4, 1, 16, p, p, p) == -5      # misaligned 64-bit array
    assert L.zlz4_batch_decompressed_size(None, p, None, p, None, p, 1) == -5
    assert L.zlz4_batch_decompressed_size(None, p, p, p, None, p + 4, 1) == -5
    assert L.zlz4_batch_decompressed_size(None, p, p, p + 2, None, p, 1) == -5
    assert L.zlz4f_batch_frame_decompressed_size(None, p, p, p, p, 1, 0, None, 1 << 20) == -5
    assert L.zlz4f_batch_frame_decompressed_size(None, p, p, p, p, 1, 0, p + 8, 1 << 20) == -5   # not 16-byte aligned
    assert L.zlz4f_batch_frame_decompressed_size(None, p, p, p, p, 1, 4, p, ws(1, 4) - 1) == -5   # one byte short
    # header errors of a frame need no device
    for f, name in ((b"", "FrameHeaderIncomplete"), (b"\x04\x22\x4d\x18\x60\x40", "FrameHeaderIncomplete"),
                    (b"\x05\x22\x4d\x18\x60\x40\x82", "FrameTypeUnknown"), (b"\x04\x22\x4d\x18\x60\x40\x00", "HeaderChecksumInvalid")):
        with pytest.raises(zl.Lz4Error) as e:
            zl.lz4f.frameDecompressedSize(f)
        assert e.value.name == name, (f, e.value.name)


CPP = r"""
#include <cstdio>
#include "zlz4.hpp"
int main() {
    const unsigned char src[] = {0x24, 'x', 'y', 18, 0, 0x50, 'E', 'N', 'D', '!', '!'};   // 2 + 8 (dictionary) + 5
    zlz4::Result a = zlz4::decompressedSize(src, 0);
    zlz4::Result b = zlz4::decompressedSize(src, sizeof src, 16);
    zlz4::Result c = zlz4::decompressedSize(src, sizeof src, 15);
    zlz4::Result f = zlz4::lz4f::frameDecompressedSize(src, sizeof src);
    zlz4::device::Blocks bl{};
    zlz4::Result q = zlz4::device::decompressedSizeBatch(nullptr, bl, nullptr, nullptr);   // nblocks == 0
    zlz4::Result p = zlz4::device::planOutputs(nullptr, nullptr, 0, 3, nullptr, nullptr, nullptr);
    zlz4::lz4f::Frames fr{};
    zlz4::Result g = zlz4::lz4f::frameDecompressedSizeBatch(nullptr, fr, nullptr, 0, nullptr, 0);
    if (!a.ok() || a.value != 0) return 1;
    if (f.ok() || f.error_name() != "FrameTypeUnknown") return 2;
    if (!q.ok() || !g.ok()) return 3;
    if (p.ok() || p.error_name() != "InvalidState") return 4;
    if (zlz4::lz4f::frameDecompressedSizeBatchWorkspace(4, 16) == 0) return 5;
    if (zlz4_device_check() == 0) {
        if (!b.ok() || b.value != 15) return 6;
        if (c.ok() || c.error_name() != "CorruptedData") return 7;
    } else {
        if (b.ok() || b.error_name() != "DeviceError") return 8;
    }
    std::printf("size mirror ok\n");
    return 0;
}
"""


def test_cpp_mirror_size_calls_compile_link_and_run(zl, tmp_path):
    assert shutil.which("g++") is not None
    src = tmp_path / "sm.cpp"
    src.write_text(CPP)
    exe = str(tmp_path / "sm")
    libdir = os.path.dirname(zl.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, str(src), "-I", os.path.join(ROOT, "zig-lz4_amd", "csrc", "host"),
                           "-L", libdir, "-lzlz4_amd", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "size mirror ok" in out.stdout, out.stdout + out.stderr


# ------------------------------------------------------------------ blocks
@pytest.fixture(scope="module")
def streams(oracle):
    return sizegen.block_streams(oracle)


def test_pyref_block_size_equals_oracle_decompress_safe(oracle, streams):
    assert len(streams) > 1500
    seen = set()
    for name, c, plain in streams:
        want = _status(oracle.decompress_safe(c, sizegen.oracle_cap(c)))      # no case is skipped for its size
        got = ps.block_size(c)
        assert got == want, (name, len(c), got, want)
        if plain is not None:
            assert got == len(plain), (name, got, len(plain))
        seen.add(min(got, 0))
    assert seen == {0, CORRUPT}                      # OutputTooSmall needs more than 0xFFFFFFFF bytes: see the edge blocks


def test_block_size_is_the_smallest_capacity_that_decodes(oracle, streams):
    n = 0
    for name, c, plain in streams:
        if len(c) > 300000:
            continue
        s = ps.block_size(c)
        if s >= 1:
            assert _status(oracle.decompress_safe(c, s)) == s, name
            if s - 1 >= 1:
                assert oracle.decompress_safe(c, s - 1) == OTS, name
            n += 1
    assert n > 800


def test_edge_blocks_at_the_32_bit_limit():
    """built arithmetically (~17 MB each): exactly 0xFFFFFFFF bytes, one more, and a stream that ends inside its run"""
    a = sizegen.edge_block(0xFFFFFFFF)
    b = sizegen.edge_block(0x100000000)
    c = sizegen.edge_block(0xFFFFFFFF, end_inside=True)
    assert len(a) < 17 << 20 and a[:4] == b"\x1f\x41\x01\x00" and a[4] == 0xFF and a[-2] == 0xFF and a[-1] != 0xFF
    assert ps.block_size(a) == 0xFFFFFFFF
    assert ps.block_size(b) == OTS
    assert ps.block_size(c) == CORRUPT
    assert ps.block_size(sizegen.edge_block(1000)) == 1000 and ps.block_size(sizegen.edge_block(1000, True)) == CORRUPT


# ------------------------------------------------------------------ dictionaries
def test_pyref_dict_size_equals_dict_decoder_at_full_short_and_zero_length(tmp_path):
    recs = sizegen.dict_records(tmp_path)
    assert len(recs) > 150
    n_short = 0
    for name, c, dct in recs:
        cap = sizegen.oracle_cap(c)
        want = pd.decompress_safe_using_dict(c, cap, dct)[0]
        reach = []
        got = ps.block_size(c, len(dct), reach=reach)
        assert got == want, (name, got, want)
        # the query takes the dictionary's reachable length: anything past 64 KiB cannot matter
        assert ps.block_size(c, min(len(dct), 65536)) == want, name
        if got >= 0 and reach:
            # one byte short of the deepest reach: the match that reaches deepest fails :189-192
            short = max(reach) - 1
            assert ps.block_size(c, short) == CORRUPT, name
            assert pd.decompress_safe_using_dict(c, cap, dct[len(dct) - short:] if short else b"")[0] == CORRUPT, name
            assert ps.block_size(c, max(reach)) == got, name
            n_short += 1
        # length 0: an empty dictionary, which decodes like none at all
        z = pd.decompress_safe_using_dict(c, cap, b"")[0]
        assert ps.block_size(c, 0) == z and ps.block_size(c) == z, name
    assert n_short > 60


def test_dict_size_is_the_smallest_capacity_that_decodes(tmp_path):
    n = 0
    for name, c, dct in sizegen.dict_records(tmp_path):
        s = ps.block_size(c, len(dct))
        if s >= 1 and len(c) < 20000:
            assert pd.decompress_safe_using_dict(c, s, dct)[0] == s, name
            if s - 1 >= 1:
                assert pd.decompress_safe_using_dict(c, s - 1, dct)[0] == OTS, name
            n += 1
    assert n > 60


# ------------------------------------------------------------------ frames
def test_pyref_xxh32_equals_oracle(oracle):
    import datagen as dg
    for n in (0, 1, 3, 4, 15, 16, 17, 31, 32, 33, 1000, 65536):
        b = bytes(dg.random_bytes(n, 3 + n))
        assert ps.xxh32(b) == oracle.xxh32(b), n


def test_pyref_frame_size_equals_oracle_decompress_frame(oracle):
    frames = sizegen.frame_corpus(oracle)
    assert len(frames) > 600
    seen, n_exc = set(), 0
    for name, f, content in frames:
        got = ps.frame_size(f)
        want = _status(oracle.decompress_frame(f, 255 * len(f) + 64))
        if want == -118:
            # the stated exception: ContentChecksumInvalid needs the decoded bytes; the query reports the size, and the
            # oracle, given exactly that many bytes, still gets as far as the content checksum
            assert got >= 0, (name, got)
            assert oracle.decompress_frame(f, got) == -118, (name, got)
            n_exc += 1
        else:
            assert got == want, (name, len(f), got, want)
        if content is not None:
            assert got == len(content), (name, got, len(content))
        seen.add(min(want, 0))
    assert {0, -107, -112, -113, -114, -116, -117} <= seen, seen
    assert n_exc > 0


def test_frame_with_only_a_wrong_content_checksum_reports_its_size(oracle):
    import datagen as dg
    p = oracle.Prefs()
    p.content_checksum = 1
    p.block_checksum = 1
    for n in (0, 1, 70000, 200000):
        b = bytes(dg.text_bytes(n, 9)) if n else b""
        f = bytearray(oracle.compress_frame(b, p))
        assert ps.frame_size(bytes(f)) == n and _status(oracle.decompress_frame(bytes(f), n + 8)) == n
        f[-1] ^= 0x40
        assert oracle.decompress_frame(bytes(f), n + 8) == -118
        assert ps.frame_size(bytes(f)) == n
        assert ps.frame_size(bytes(f[:-1])) == -114 == oracle.decompress_frame(bytes(f[:-1]), n + 8)   # :626 missing word
