"""Legacy lz4 frames without a GPU (include/zlz4_amd.h; the model: tests/legacygen.py).

1. The constants: ZLZ4F_LEGACY_BLOCK_BOUND is zlz4_compress_bound(8 MiB) and liblz4's LZ4_compressBound(8 MiB).
2. The model's reader against a loop of liblz4's LZ4_decompress_safe over the model's blocks at a capacity of 8 MiB: bytes,
   the empty block behind a zero size word, a block of 8 MiB + 1 refused and taken with one byte more room.
3. zlz4f_legacy_compress_frame_bound against the model's arithmetic.
4. What the three host calls answer before the device check.
5. The shared walk of zig-lz4_amd/csrc/zlz4_frame_batch.hpp, compiled for the host (AddressSanitizer, UBSan) into
   tests/legacy_walk_check.cpp, against the model's walk over the crafted table and every prefix of two frames.
"""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import legacygen as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIB8 = 8 << 20


@pytest.fixture(scope="module")
def liblz4():
    lib = C.CDLL("liblz4.so.1")
    lib.LZ4_compressBound.restype = C.c_int
    lib.LZ4_compressBound.argtypes = [C.c_int]
    lib.LZ4_decompress_safe.restype = C.c_int
    lib.LZ4_decompress_safe.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_int]
    return lib


def lz4_decode(lib, block, cap):
    dst = C.create_string_buffer(max(1, cap))
    r = lib.LZ4_decompress_safe(bytes(block), dst, len(block), cap)
    return r if r < 0 else dst.raw[:r]


def test_constants(zl, liblz4):
    assert zl.lz4f.LEGACY_BLOCK_BOUND == g.BLOCK_BOUND == 8421520
    assert zl.compressBound(MIB8) == g.BLOCK_BOUND == liblz4.LZ4_compressBound(MIB8)
    assert zl.lz4f.LEGACY_BLOCK_SIZE == g.BLOCK_SIZE == MIB8 and zl.lz4f.LEGACY_MAGICNUMBER == g.MAGIC
    hdr = open(os.path.join(ROOT, "include", "zlz4_amd.h")).read()
    assert "#define ZLZ4F_LEGACY_BLOCK_BOUND 8421520u" in hdr and "#define ZLZ4F_LEGACY_MAGICNUMBER 0x184C2102u" in hdr
    # every lz4 magic is a size word above the bound: the walk ends in front of the next member
    assert min(g.MAGIC, g.MODERN_MAGIC, g.SKIP_MAGIC) > g.BLOCK_BOUND


def test_the_table_says_what_the_model_says():
    names = set()
    for c in g.table():
        r = g.read(c.buf)
        assert (r.result, r.consumed) == (c.result, c.consumed), c.name
        assert (r.content is None) == (c.result < 0) and c.name not in names
        names.add(c.name)
    results = {c.result for c in g.table()}
    assert {g.HEADER_INCOMPLETE, g.TYPE_UNKNOWN, g.SIZE_WRONG, g.FAILED, 0, MIB8} <= results


def test_model_reader_is_a_loop_of_liblz4(liblz4):
    for c in g.table():
        w = g.walk(c.buf)
        parts, failed = [], False
        for off, size in w.blocks:
            d = lz4_decode(liblz4, c.buf[off:off + size], MIB8)
            if isinstance(d, int):
                failed = True
                break
            parts.append(d)
        r = g.read(c.buf)
        if failed:
            assert r.result == g.FAILED, c.name
        elif w.verdict:
            assert r.result == w.verdict, c.name
        else:
            assert r.content == b"".join(parts), c.name
    # the writer's blocks too, at the fast level and two HC levels
    data = g.text(3 * 4096 + 5)
    for level in (0, 3, 9):
        f = g.write(data, 4096, level)
        assert b"".join(lz4_decode(liblz4, f[o:o + n], MIB8) for o, n in g.walk(f).blocks) == data == g.read(f).content
    # liblz4 fails the empty block that a zero size word stands for; the block calls here answer 0, so the walk flags it
    assert lz4_decode(liblz4, b"", MIB8) < 0
    assert g.read(g.build([b""])).result == g.FAILED
    assert lz4_decode(liblz4, g.EMPTY, MIB8) == b"" and lz4_decode(liblz4, g.CORRUPT, MIB8) < 0
    # a block of 8 MiB + 1 is refused at the format's capacity and decodes with one byte more
    over = g.zeros_block(MIB8 + 1)
    assert lz4_decode(liblz4, over, MIB8) < 0 and lz4_decode(liblz4, over, MIB8 + 1) == bytes(MIB8 + 1)
    assert lz4_decode(liblz4, g.zeros_block(MIB8), MIB8) == bytes(MIB8) == g.decode_block(g.zeros_block(MIB8))
    assert g.decode_block(over) is None


@pytest.mark.parametrize("bs", [1, 4096, MIB8])
def test_bound_arithmetic(zl, bs):
    for given in ((bs,) if bs != MIB8 else (bs, 0)):                   # 0 means 8 MiB
        p = zl.LegacyPrefs(given, 0)
        for n in (0, 1, bs - 1, bs, bs + 1, 3 * bs + 5):
            want = 4 + sum(4 + zl.compressBound(min(bs, n - p)) for p in range(0, n, bs))
            assert zl.lz4f.legacyCompressFrameBound(n, p) == want == g.bound(n, bs), (given, n)
    assert zl.lz4f.legacyCompressFrameBound(0) == 4 and zl.lz4f.legacyCompressFrameBound(MIB8 + 1) == 4 + 4 + g.BLOCK_BOUND + 4 + 17
    # a written frame never exceeds its bound; incompressible chunks grow towards it
    rnd = bytes(g.dg.random_bytes(3 * 4096 + 5, 3))
    assert len(rnd) + 4 + 4 * 4 < len(g.write(rnd, 4096)) <= g.bound(len(rnd), 4096)
    for bad in (MIB8 + 1, 0xFFFFFFFF):
        assert zl.lz4f.legacyCompressFrameBound(100, zl.LegacyPrefs(bad, 0)) == 0
        assert zl.lz4f.compressLegacyFrameBatchWorkspace(1, 1, zl.LegacyPrefs(bad, 0)) == 0


def test_workspace_sizes(zl):
    f = zl.lz4f
    q, d = f.legacyFrameDecompressedSizeBatchWorkspace, f.decompressLegacyFrameBatchWorkspace
    assert q(1, 0) == 256 and 0 < q(3, 100) < d(3, 100) and d(3, 100) < d(3, 101 + 64)
    fast, hc = zl.LegacyPrefs(4096, 0), zl.LegacyPrefs(4096, 9)
    w = f.compressLegacyFrameBatchWorkspace
    slot = (zl.compressBound(4096) + 15) // 16 * 16
    assert w(2, 10, fast) >= 10 * slot and w(2, 10, hc) >= w(2, 10, fast) + zl.batch_compress_hc_workspace(10, 4096)
    assert w(2, 10, None) >= 10 * g.BLOCK_BOUND


def test_host_calls_refuse_before_the_device_check(zl):
    """on a machine without a GPU these answers come as they stand; everything else there is DeviceError"""
    L = zl.lib()
    buf = (C.c_uint8 * 64)()
    a = C.addressof(buf)
    used = C.c_size_t(77)
    # a null pointer with a length
    assert L.zlz4f_compress_legacy_frame(None, 5, a, 64, None) == g.INVALID_STATE
    assert L.zlz4f_compress_legacy_frame(a, 5, None, 64, None) == g.INVALID_STATE
    assert L.zlz4f_decompress_legacy_frame(None, 5, a, 64, None) == g.INVALID_STATE
    assert L.zlz4f_decompress_legacy_frame(a, 5, None, 64, None) == g.INVALID_STATE
    assert L.zlz4f_legacy_frame_decompressed_size(None, 5, None) == g.INVALID_STATE
    # an invalid block size
    for bad in (MIB8 + 1, 1 << 31):
        with pytest.raises(zl.Lz4Error) as e:
            zl.lz4f.compressLegacyFrame(b"abc", zl.LegacyPrefs(bad, 0))
        assert e.value.code == g.MAX_BLOCK_SIZE_INVALID
    # step 1 of the read rules, with and without `consumed`
    for c in g.defects():
        if c.result not in (g.HEADER_INCOMPLETE, g.TYPE_UNKNOWN):
            continue
        s, n = zl._in(c.buf)
        for call in (lambda u: L.zlz4f_legacy_frame_decompressed_size(C.addressof(s), n, u),
                     lambda u: L.zlz4f_decompress_legacy_frame(C.addressof(s), n, a, 64, u)):
            used.value = 77
            assert call(C.byref(used)) == c.result and used.value == n, c.name
            assert call(None) == c.result, c.name
    assert L.zlz4f_legacy_frame_decompressed_size(None, 0, C.byref(used)) == g.HEADER_INCOMPLETE and used.value == 0
    if not zl.device_available():
        for call, arg in ((zl.lz4f.compressLegacyFrame, b"abc"), (zl.lz4f.decompressLegacyFrame, g.build([g.EMPTY])),
                          (zl.lz4f.legacyFrameDecompressedSize, g.build([g.EMPTY]))):
            with pytest.raises(zl.Lz4Error) as e:
                call(arg)
            assert e.value.name == "DeviceError"


def _prefixes(f):
    return [f[:k] for k in range(len(f) + 1)]


def test_shared_walk_on_the_host(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "no hipcc: the host build of the legacy walk cannot be checked"
    blocks, _ = g.small_blocks(70, 9)
    cases = [c.buf for c in g.table()]
    cases += _prefixes(g.build([g.literal_block(b"ab"), g.EMPTY, g.literal_block(b"cde")]) + g.le32(g.MAGIC) + b"\x10z")
    cases += _prefixes(g.build([g.CORRUPT, b"", g.EMPTY]))
    cases += [g.build(blocks), g.build(blocks) + g.skippable(), g.le32(g.BLOCK_BOUND) * 3]
    exe, data = str(tmp_path / "legacy_walk_check"), str(tmp_path / "cases.bin")
    with open(data, "wb") as f:
        f.write(len(cases).to_bytes(4, "little"))
        for b in cases:
            f.write(len(b).to_bytes(4, "little") + b)
    subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-Xarch_host",
                           "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "legacy_walk_check.cpp")], cwd=str(tmp_path))
    out = subprocess.run([exe, data], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and not out.stderr.strip(), out.stdout[-2000:] + out.stderr[-4000:]
    rows = out.stdout.splitlines()
    assert len(rows) == len(cases)
    for b, row in zip(cases, rows):
        w = g.walk(b)
        want = " ".join(["%d %d %d" % (w.verdict, len(w.blocks), w.consumed)] + ["%d:%d" % x for x in w.blocks])
        assert row == want, (b[:40], row[:200], want[:200])
    verdicts = {g.walk(b).verdict for b in cases}
    assert verdicts == {0, g.HEADER_INCOMPLETE, g.TYPE_UNKNOWN, g.SIZE_WRONG, g.FAILED}
