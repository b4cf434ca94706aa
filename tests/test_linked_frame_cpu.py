"""Linked-block frames without a GPU: the CPU model tools/pyref/zig_lz4_linked_frame.py against liblz4 (committed fixtures,
and fresh frames where liblz4.so.1 loads), against the oracle for block 0, and against hand-made frames whose expected
results are stated with them (tests/linkedgen.py); the public surface of the new calls; the fixture file itself."""
import os
import sys

import pytest

import linkedgen as lg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "pyref"))
import zig_lz4_linked_frame as lf  # noqa: E402
import zig_lz4_sizes as zs  # noqa: E402

NEW = ("zlz4f_batch_decompress_frame_ex", "zlz4f_batch_decompress_frame_workspace_ex",
       "zlz4f_batch_frame_decompressed_size_ex", "zlz4f_batch_frame_decompressed_size_workspace_ex",
       "zlz4f_decompress_frame_device_ex", "zlz4f_decompress_frame_ex", "zlz4f_frame_decompressed_size_ex",
       "zlz4f_batch_compress_frame_workspace_ex")


@pytest.fixture(scope="module")
def fx():
    return lg.fixtures()


@pytest.fixture(scope="module")
def lz4f():
    return lg.liblz4f()


def test_fixture_file_is_what_the_generator_describes(fx):
    assert [f["name"] for f in fx] == [r["name"] for r in lg.RECIPES]
    assert [len(f["input"]) for f in fx] == [160000, 160000, 600000]
    for f, r in zip(fx, lg.RECIPES):
        assert f["recipe"] == r and len(f["frame"]) < 65536
        assert f["frame"][4] & 0x20 == 0                               # FLG declares linked blocks
        assert (f["frame"][4] >> 4) & 1 == r["block_checksum"] and (f["frame"][4] >> 2) & 1 == r["content_checksum"]
        assert (f["frame"][5] >> 4) & 7 == r["block_size_id"]
    assert os.path.getsize(lg.FIXTURES) < (1 << 20)


def test_model_decodes_liblz4_fixtures_and_the_reference_does_not(fx, oracle):
    for f in fx:
        n = len(f["input"])
        assert oracle.decompress_frame(f["frame"], n) == -116, f["name"]           # the reference: every block alone
        assert zs.frame_size(f["frame"]) == -116
        assert lf.decompress_frame_linked(f["frame"], n) == (n, f["input"]), f["name"]
        assert lf.frame_size_linked(f["frame"]) == n
        assert lf.decompress_frame_linked(f["frame"], n - 1)[0] == -116


def test_model_decodes_fresh_liblz4_frames(lz4f):
    if lz4f is None:
        pytest.skip("liblz4.so.1 does not load")
    import datagen as dg
    for data, bsid, bc, cc in ((lg.recipe_input(lg.RECIPES[0])[:150001], 4, 1, 0),
                               (bytes(dg.text_bytes(70000, 11)) * 2, 4, 0, 1),
                               (bytes(dg.mixed_bytes(300000, 3)), 5, 0, 0), (b"", 4, 0, 1), (b"x" * 70000, 4, 1, 1)):
        frame = lz4f.compress(data, bsid, bc, cc, linked=True)
        assert lf.decompress_frame_linked(frame, len(data)) == (len(data), data)
        assert lf.frame_size_linked(frame) == len(data)
        ind = lz4f.compress(data, bsid, bc, cc, linked=False)          # an independent frame: the reference's path
        assert ind[4] & 0x20 and lf.decompress_frame_linked(ind, len(data)) == (len(data), data)


def test_liblz4_decodes_the_models_linked_frames(lz4f, fx):
    if lz4f is None:
        pytest.skip("liblz4.so.1 does not load")
    import datagen as dg
    data = fx[0]["input"]
    frame = lf.compress_frame_linked(data)
    assert len(frame) == 20154                                         # (the independent frame of this input: 53 522)
    assert lz4f.decompress(frame, len(data)) == data
    rnd = bytes(dg.random_bytes(70000, 4))
    # 70 000 random bytes and a copy of the first 60 000: the copy lies 70 000 back, out of any block's reach, so both
    # blocks are stored; after 65 536 random bytes a copy from 1000 on lies 64 536 back: block 1 matches into stored block 0
    far, near = rnd + rnd[:60000], rnd[:65536] + rnd[1000:61000]
    for d, prefs in ((data, dict(block_checksum=1, content_checksum=1, content_size=len(data))), (far, dict()),
                     (near, dict()), (fx[2]["input"][:300000], dict(block_size_id=5)), (b"", dict(content_checksum=1)),
                     (data[:12], dict()), (data[:65537], dict(block_checksum=1))):
        frame = lf.compress_frame_linked(d, prefs)
        assert frame[4] & 0x20 == 0
        assert lz4f.decompress(frame, len(d)) == d
        assert lf.decompress_frame_linked(frame, len(d)) == (len(d), d)
    stored = lf.compress_frame_linked(near)
    assert int.from_bytes(stored[7:11], "little") == 0x80000000 | 65536          # block 0 is stored ...
    # ... and block 1 (60 000 bytes that are random but for block 0) is compressed all the same; the 4096-entry table of
    # loadDict keeps only some of the dictionary's positions, so the fast parse finds the copy in pieces
    assert int.from_bytes(stored[11 + 65536:15 + 65536], "little") < 55000


def test_block_0_of_a_model_frame_is_compress_default(oracle, fx):
    for data in (fx[0]["input"], fx[0]["input"][:30000], fx[2]["input"][:70000]):
        frame = lf.compress_frame_linked(data)
        n0 = int.from_bytes(frame[7:11], "little")
        assert frame[11:11 + n0] == oracle.compress_default(data[:65536])
    one = fx[0]["input"][:65536]                                       # a one-block frame is compressFrame's, FLG aside
    q = oracle.Prefs(); q.block_mode = 0
    assert lf.compress_frame_linked(one) == oracle.compress_frame(one, q)


def test_crafted_cases_give_the_stated_results():
    cases = lg.crafted_cases()
    assert len(cases) >= 7
    for name, frame, cap, want, want_bytes in cases:
        r, b = lf.decompress_frame_linked(frame, cap)
        assert r == want, name
        if want_bytes is not None:
            assert b == want_bytes, name
    by = {c[0]: c for c in cases}
    # the size query: capacity and content checksum play no part, everything else does
    assert lf.frame_size_linked(by["match_one_byte_before_the_frame"][1]) == -116
    assert lf.frame_size_linked(by["block_checksum_wrong_in_block_2"][1]) == -107
    assert lf.frame_size_linked(by["chain_truncated"][1]) == -114
    assert lf.frame_size_linked(by["capacity_one_short"][1]) == 409
    assert lf.frame_size_linked(by["content_checksum_wrong"][1]) == 409


def test_new_symbols_flags_and_workspaces(zl):
    L = zl.lib()
    for name in NEW:
        assert name in zl.SYMBOLS and hasattr(L, name), name
    assert zl.lz4f.DECODE_LINKED == 1 and zl.lz4f.BATCH_LINK_BLOCKS == 4
    p = zl.Prefs()
    for nf, mb in ((1, 0), (3, 7), (4096, 65536)):
        assert zl.lz4f.decompressFrameBatchWorkspace(nf, mb, 0) == L.zlz4f_batch_decompress_frame_workspace(nf, mb)
        assert zl.lz4f.frameDecompressedSizeBatchWorkspace(nf, mb, 0) == L.zlz4f_batch_frame_decompressed_size_workspace(nf, mb)
        assert zl.lz4f.compressFrameBatchWorkspace(nf, mb, p, 0) == L.zlz4f_batch_compress_frame_workspace(nf, mb, p)
        assert zl.lz4f.decompressFrameBatchWorkspace(nf, mb, 1) >= L.zlz4f_batch_decompress_frame_workspace(nf, mb) + 8 * nf
        assert zl.lz4f.frameDecompressedSizeBatchWorkspace(nf, mb, 1) >= \
            L.zlz4f_batch_frame_decompressed_size_workspace(nf, mb) + 8 * nf
        # one loadDict table (16 KiB) and a dictionary descriptor per table entry
        assert zl.lz4f.compressFrameBatchWorkspace(nf, mb, p, 4) >= L.zlz4f_batch_compress_frame_workspace(nf, mb, p) + mb * (16384 + 12)


def test_flag_errors_are_host_arithmetic(zl):
    """Refused before the device is looked at, so the codes are the same with and without a GPU."""
    L = zl.lib()
    none8 = (None,) * 8
    p = zl.Prefs(); p.block_mode = 1
    assert L.zlz4f_batch_compress_frame(*none8, 1, 1, p, 4, None, 0) == -104             # FLG would not say "linked"
    p = zl.Prefs(); p.compression_level = 9
    assert L.zlz4f_batch_compress_frame(*none8, 1, 1, p, 4, None, 0) == -8               # HC linking is not built
    assert L.zlz4f_batch_compress_frame(*none8, 1, 1, None, 8, None, 0) == -104
    assert L.zlz4f_batch_decompress_frame_ex(*none8, 1, 1, 2, None, 0) == -104
    assert L.zlz4f_batch_frame_decompressed_size_ex(None, None, None, None, None, 1, 1, 2, None, 0) == -104
    assert L.zlz4f_decompress_frame_ex(None, 0, None, 0, 6) == -104
    assert L.zlz4f_frame_decompressed_size_ex(None, 0, 2) == -104
    if not zl.device_available():
        assert L.zlz4f_batch_decompress_frame_ex(*none8, 4, 16, 1, None, 1 << 20) == -7
        fr = lg.fixtures()[0]["frame"]
        with pytest.raises(zl.Lz4Error) as e:
            zl.lz4f.decompressFrame(fr, 160000, zl.lz4f.DECODE_LINKED)
        assert e.value.name == "DeviceError"
