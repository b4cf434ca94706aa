"""Whole .lz4 files without a GPU (include/zlz4_amd.h; the model: tests/lz4filegen.py).

1. The model pinned by hand: positions, lengths, kinds, block counts and codes written out.
2. The new symbols, constants and Python signatures.
3. What the _ex host calls and zlz4f_batch_multiframe_split_ex refuse before the device check, in their order.
4. The shared member delimiter of zig-lz4_amd/csrc/zlz4_frame_batch.hpp, compiled for the host (AddressSanitizer, UBSan)
   into tests/member_walk_check.cpp, against the model for both split_flags values.
"""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import pytest

import legacygen as lg
import lz4filegen as g
import multiframegen as mg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = g.Member


def _parts():
    blocks, content = lg.small_blocks(3, 5)
    modern = lg.oracle.compress_frame(b"the next member")
    return blocks, lg.build(blocks), content, modern


def test_model_pinned_by_hand():
    blocks, f, content, modern = _parts()
    sk = mg.skippable(3, b"meta")
    magic = lg.le32(lg.MAGIC)
    assert (len(modern), len(sk)) == (7 + 4 + 15 + 4, 12), "header, one stored block, end mark; a skippable of 4 bytes"
    buf = f + modern + sk + magic
    a, b, c = len(f), len(f) + 30, len(f) + 42
    assert g.split(buf, True) == [M(0, a, 4, 0, 3, False), M(a, 30, 1, 0, 1, False), M(b, 12, 2, 3, 0, False),
                                  M(c, 4, 4, 0, 0, False)]
    assert g.split(buf, False) == mg.split(buf) == [M(0, len(buf), 1, 0, 0, True)]
    assert g.expected(buf, 0, True) == (len(content) + 15, content + b"the next member", [len(content), 15, None, 0])
    assert g.expected(buf, 0, False) == (mg.TYPE_UNKNOWN, None, [mg.TYPE_UNKNOWN])
    assert g.totals([buf, b"", modern], True) == [5, 2, 2, 3] and g.totals([buf, b"", modern], False) == [2, 1, 0, 0]
    # the magic alone: a member of no blocks and no content, first, in the middle, last and alone
    assert g.table(magic + modern + magic + magic) == [(0, 4, 4, 0), (4, 30, 1, 0), (34, 4, 4, 0), (38, 4, 4, 0)]
    assert g.expected(magic) == (0, b"", [0]) and g.expected(magic + magic) == (0, b"", [0, 0])
    # defects of the walk: the member reaches to the end and is the last one; the legacy reader names the code
    for tail, code in ((b"\x07", lg.SIZE_WRONG), (b"\x07\x00\x00", lg.SIZE_WRONG), (lg.le32(0) + modern, lg.FAILED),
                       (lg.le32(len(modern) + 1) + modern, lg.SIZE_WRONG)):
        bad = modern + f + tail
        assert g.split(bad) == [M(0, 30, 1, 0, 1, False), M(30, len(f + tail), 4, 0, 3, True)], tail[:4]
        assert g.expected(bad) == (code, None, [15, code])
    # a corrupt block is no defect of the walk: the block's code decides, the later frame still has its size
    bad = lg.build([blocks[0], lg.CORRUPT]) + modern
    n0 = len(lg.build([blocks[0], lg.CORRUPT]))
    assert g.split(bad) == [M(0, n0, 4, 0, 2, False), M(n0, 30, 1, 0, 1, False)]
    assert g.expected(bad) == (lg.FAILED, None, [lg.FAILED, 15])
    # a foreign word that is no magic ends the legacy member and starts a frame member that cannot be delimited
    for junk, code in ((b"xyz", mg.TYPE_UNKNOWN), (b"xy", mg.HEADER_INCOMPLETE)):
        bad = f + lg.le32(lg.BLOCK_BOUND + 1) + junk
        assert g.split(bad) == [M(0, a, 4, 0, 3, False), M(a, 4 + len(junk), 1, 0, 0, True)]
        assert g.expected(bad) == (code, None, [len(content), code])
    # a word of exactly the bound is a block's size word
    assert g.split(f + lg.le32(lg.BLOCK_BOUND) + b"x" * 40) == [M(0, a + 44, 4, 0, 3, True)]
    # other kinds around a legacy member
    cc = mg.pick("text1_bc1_cc1_cs1")[0]
    bad = mg.flip(cc.frame, len(cc.frame) - 1) + f
    assert g.expected(bad) == (mg.CONTENT_CHECKSUM, None, [mg.CONTENT_CHECKSUM, len(content)])
    assert g.expected(f + sk[:-1]) == (mg.SIZE_WRONG, None, [len(content), None])
    assert g.expected(f + sk[:6]) == (mg.HEADER_INCOMPLETE, None, [len(content), None])
    # without the flag the model is multiframegen's on everything above and on its own tables
    for buf in [buf, bad, magic, b""] + [c[1] for c in mg.defects()] + [c.buf for c in lg.table()]:
        assert g.split(buf, False) == mg.split(buf)
        assert g.expected(buf, 0, False) == mg.expected(buf, 0)


def test_symbols_constants_and_signatures(zl):
    L, f = zl.lib(), zl.lz4f
    for name in ("zlz4f_batch_multiframe_split_ex", "zlz4f_batch_multiframe_select", "zlz4f_multiframe_decompressed_size_ex",
                 "zlz4f_decompress_multiframe_ex"):
        assert name in zl.SYMBOLS and hasattr(L, name), name
    assert len(zl.SYMBOLS["zlz4f_batch_multiframe_split_ex"][1]) == len(zl.SYMBOLS["zlz4f_batch_multiframe_split"][1]) + 2
    assert len(zl.SYMBOLS["zlz4f_batch_multiframe_select"][1]) == 9
    assert (f.SPLIT_LEGACY, f.MEMBER_LEGACY) == (1, 4) == (g.SPLIT_LEGACY, g.LEGACY)
    hdr = open(os.path.join(ROOT, "include", "zlz4_amd.h")).read()
    assert "#define ZLZ4F_SPLIT_LEGACY  1u" in hdr and "#define ZLZ4F_MEMBER_LEGACY 4u" in hdr
    zig = open(os.path.join(ROOT, "zig-lz4_amd", "zig", "root.zig")).read()
    for name in ("zlz4f_batch_multiframe_split_ex", "zlz4f_batch_multiframe_select", "zlz4f_multiframe_decompressed_size_ex",
                 "zlz4f_decompress_multiframe_ex"):
        assert 'extern "c" fn %s(' % name in zig and name + "(" in hdr
    for fn in (f.splitMultiframes, f.multiframeMembers, f.decompressMultiframes, f.multiframeDecompressedSize,
               f.decompressMultiframe):
        p = inspect.signature(fn).parameters
        assert p["legacy"].default is False, fn.__name__
    assert list(inspect.signature(f.decompressFiles).parameters) == ["buffers", "align", "device"]
    assert list(inspect.signature(f.decompressFile).parameters) == ["src"]
    assert callable(f.multiframeSplitBatchEx) and callable(f.multiframeSelectBatch)


def test_refusals_come_before_the_device_check(zl):
    L = zl.lib()
    frame = mg.few()[1].frame
    src = (C.c_uint8 * len(frame)).from_buffer_copy(frame)
    dst = (C.c_uint8 * 64)()
    s, d, n = C.addressof(src), C.addressof(dst), len(frame)
    for bad in (2, 0x80000000, 3):
        # 1. an unknown decode_flags bit, 2. an unknown split_flags bit, 3. a null pointer with a length
        assert L.zlz4f_multiframe_decompressed_size_ex(s, n, bad, 1) == mg.PARAMETER_INVALID
        assert L.zlz4f_multiframe_decompressed_size_ex(s, n, 0, bad) == mg.PARAMETER_INVALID
        assert L.zlz4f_multiframe_decompressed_size_ex(None, 5, 1, bad) == mg.PARAMETER_INVALID
        assert L.zlz4f_decompress_multiframe_ex(s, n, d, 64, bad, 0) == mg.PARAMETER_INVALID
        assert L.zlz4f_decompress_multiframe_ex(s, n, d, 64, 1, bad) == mg.PARAMETER_INVALID
        assert L.zlz4f_decompress_multiframe_ex(None, 5, None, 5, 0, bad) == mg.PARAMETER_INVALID
        # the batch split: the flags before the null arrays
        assert L.zlz4f_batch_multiframe_split_ex(None, None, None, None, 3, None, None, None, None, None, None, None, None,
                                                 None, bad, None) == mg.PARAMETER_INVALID
    for sf in (0, 1):
        assert L.zlz4f_multiframe_decompressed_size_ex(None, 5, 0, sf) == mg.INVALID_STATE
        assert L.zlz4f_decompress_multiframe_ex(None, 5, d, 64, 1, sf) == mg.INVALID_STATE
        assert L.zlz4f_decompress_multiframe_ex(s, n, None, 64, 0, sf) == mg.INVALID_STATE
        assert L.zlz4f_batch_multiframe_split_ex(None, None, None, None, 3, None, None, None, None, None, None, None, None,
                                                 None, sf, None) == mg.INVALID_STATE
    assert L.zlz4f_batch_multiframe_select(None, None, None, None, None, None, None, 3, None) == mg.INVALID_STATE
    assert L.zlz4f_batch_multiframe_select(None, None, None, None, None, None, None, 0, None) == 0
    with pytest.raises(zl.Lz4Error) as e:
        zl.lz4f.decompressFiles([frame], device="cpu")
    assert e.value.name == "DeviceError"
    with pytest.raises(zl.Lz4Error):
        zl.lz4f.decompressMultiframes([frame], flags=2, device="cpu", legacy=True)
    if not zl.device_available():
        for call in (zl.lz4f.decompressFile, lambda b: zl.lz4f.multiframeDecompressedSize(b, legacy=True)):
            with pytest.raises(zl.Lz4Error) as e:
                call(frame)
            assert e.value.name == "DeviceError"


def _prefixes(f):
    return [f[:k] for k in range(len(f) + 1)]


def _row(buf, legacy):
    ms = g.split(buf, legacy)
    return " | ".join("%d %d %d %d %d" % (m.pos, m.len, m.kind | m.nibble << 8, m.nb, m.last) for m in ms) or "-"


def test_shared_member_delimiter_on_the_host(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "no hipcc: the host build of the member delimiter cannot be checked"
    blocks, f, content, modern = _parts()
    cases = _prefixes(f + modern + mg.skippable(3, b"meta") + lg.le32(lg.MAGIC))
    cases += [c[1] for c in mg.defects()] + [c.buf for c in lg.table()]
    cases += [f + lg.le32(lg.BLOCK_BOUND + 1) + b"xyz", f + lg.le32(lg.BLOCK_BOUND + 1), f + lg.le32(0x7FFFFFFF) + modern]
    exe, data = str(tmp_path / "member_walk_check"), str(tmp_path / "cases.bin")
    with open(data, "wb") as fh:
        fh.write(len(cases).to_bytes(4, "little"))
        for b in cases:
            fh.write(len(b).to_bytes(4, "little") + b)
    subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-Xarch_host",
                           "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "member_walk_check.cpp")], cwd=str(tmp_path))
    out = subprocess.run([exe, data], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and not out.stderr.strip(), out.stdout[-2000:] + out.stderr[-4000:]
    rows = out.stdout.splitlines()
    assert len(rows) == 2 * len(cases)
    kinds = set()
    for k, b in enumerate(cases):
        assert rows[2 * k] == _row(b, False), (k, b[:40], rows[2 * k][:200])
        assert rows[2 * k + 1] == _row(b, True), (k, b[:40], rows[2 * k + 1][:200])
        kinds |= {(m.kind, m.last) for m in g.split(b, True)}
    assert kinds == {(k, last) for k in (1, 4) for last in (False, True)} | {(2, False), (3, True)}
