"""Linked-block frames at the HC levels 3..9 without a GPU: the CPU model tools/pyref/zig_lz4_linked_frame_hc.py against the
C restatement of the block compressor (tests/hc_dict_ref.c) block by block, against the stated frame sizes, against the
model's decoder and liblz4's; block 0 and one-block frames against the oracle; the public surface of the new calls (symbols,
refusals, the workspace condition); the fixture file itself."""
import hashlib
import json
import os
import sys

import pytest

import hcdictcgen as hg
import linkedgen as lg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "pyref"))
import zig_lz4_linked_frame as lf  # noqa: E402
import zig_lz4_linked_frame_hc as lh  # noqa: E402

NEW = ("zlz4f_batch_compress_frame_ex", "zlz4f_compress_frame_device_ex", "zlz4f_compress_frame_ex")
LEVELS = (3, 6, 9)
FIXTURES = os.path.join(ROOT, "tests", "golden", "linked_frames_hc.json")
SIZES = {"text160k_bs64k": {3: 17101, 6: 15840, 9: 15632}, "text600k_bs256k": {3: 18775, 6: 17560, 9: 17357}}


@pytest.fixture(scope="module")
def cref(tmp_path_factory):
    return hg.ref(tmp_path_factory.mktemp("hc_dict_ref"))


@pytest.fixture(scope="module")
def model_frames():
    """{(recipe name, level): (input, frame)}: the model's frames of the recipes, computed once"""
    out = {}
    for r in lg.RECIPES:
        data = lg.recipe_input(r)
        for level in LEVELS:
            out[r["name"], level] = (data, lh.compress_frame_linked_hc(data, level, r))
    return out


def test_model_equals_the_c_restatement_block_by_block(cref, model_frames):
    for r in lg.RECIPES:
        bs = lf.BLOCK_SIZES[r["block_size_id"]]
        for level in LEVELS:
            data, frame = model_frames[r["name"], level]
            blocks = lh.blocks_of(frame)
            assert len(blocks) == (len(data) + bs - 1) // bs and frame[4] & 0x20 == 0
            for k, (payload, stored) in enumerate(blocks):
                n, want = cref.compress(data[k * bs:(k + 1) * bs], data[max(0, k * bs - 65536):k * bs], level)
                assert n == len(want) and not stored and payload == want, (r["name"], level, k)


def test_model_frame_sizes_are_the_stated_ones(model_frames):
    for name, by_level in SIZES.items():
        for level, size in by_level.items():
            assert len(model_frames[name, level][1]) == size, (name, level)
    for level in LEVELS:                               # a 4-byte checksum per block and one for the content
        assert len(model_frames["text160k_bs64k_checksums", level][1]) == SIZES["text160k_bs64k"][level] + 3 * 4 + 4


def test_model_frames_decode_with_the_model_and_with_liblz4(model_frames):
    z = lg.liblz4f()
    for (name, level), (data, frame) in model_frames.items():
        assert lf.decompress_frame_linked(frame, len(data)) == (len(data), data), (name, level)
        assert lf.frame_size_linked(frame) == len(data)
        if z is not None:
            assert z.decompress(frame, len(data)) == data, (name, level)


def test_block_0_and_one_block_frames_are_compress_hc(oracle, model_frames):
    text = lg.recipe_input(lg.RECIPES[0])
    for level in LEVELS:
        data, frame = model_frames["text160k_bs64k", level]
        payload, stored = lh.blocks_of(frame)[0]
        assert not stored and payload == oracle.compress_hc(data[:65536], level)
        q = oracle.Prefs()
        q.block_mode, q.compression_level = 0, level
        for n in (0, 1, 12, 13, 65536):
            assert lh.compress_frame_linked_hc(text[:n], level) == oracle.compress_frame(text[:n], q), (level, n)


def test_stored_block_stays_the_dictionary(cref):
    import datagen as dg
    rnd = bytes(dg.random_bytes(65536, 4))
    data = rnd + rnd[1000:61000]                       # block 0 is stored, block 1 copies it from 64 536 back
    frame = lh.compress_frame_linked_hc(data, 9)
    blocks = lh.blocks_of(frame)
    assert blocks[0] == (rnd, True) and not blocks[1][1] and len(blocks[1][0]) < 300      # one match of 60 000 bytes: ~235 length bytes
    assert blocks[1][0] == cref.compress(data[65536:], rnd, 9)[1]
    assert lf.decompress_frame_linked(frame, len(data)) == (len(data), data)


def test_model_refuses_the_levels_the_dictionary_compressor_does(model_frames):
    for level in (2, 10, 11, 12, 13, 0, -3):
        assert lh.compress_frame_linked_hc(b"x" * 100, level) == -8
    data, frame = model_frames["text160k_bs64k", 9]
    assert lh.compress_frame_linked_hc(data, 1, lg.RECIPES[0]) == frame          # level 1 runs as 9


def test_new_symbols(zl):
    L = zl.lib()
    for name in NEW:
        assert name in zl.SYMBOLS and hasattr(L, name), name


def test_refusals_are_host_arithmetic(zl):
    """Refused before the device is looked at, so the codes are the same with and without a GPU."""
    L = zl.lib()
    none8 = (None,) * 8
    link = zl.lz4f.BATCH_LINK_BLOCKS

    def prefs(**kw):
        p = zl.Prefs()
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    # level 9 with the flag is accepted: without a workspace the answer is the device's or InvalidState, never Unsupported
    r = L.zlz4f_batch_compress_frame_ex(*none8, 1, 1, prefs(compression_level=9), link, None, 0)
    assert r == (-5 if zl.device_available() else -7)
    for level in (3, 1):
        assert L.zlz4f_batch_compress_frame_ex(*none8, 1, 1, prefs(compression_level=level), link, None, 0) == r
    for level in (2, 10, 12, 13):
        assert L.zlz4f_batch_compress_frame_ex(*none8, 1, 1, prefs(compression_level=level), link, None, 0) == -8
        assert L.zlz4f_compress_frame_ex(None, 0, None, 0, prefs(compression_level=level), link) == -8
        assert L.zlz4f_compress_frame_device_ex(None, None, 0, None, 0, prefs(compression_level=level), link) == -8
        assert L.zlz4f_batch_compress_frame_ex(*none8, 1, 1, prefs(compression_level=level), 0, None, 0) == r   # no flag
    assert L.zlz4f_batch_compress_frame_ex(*none8, 1, 1, prefs(block_mode=1, compression_level=9), link, None, 0) == -104
    assert L.zlz4f_batch_compress_frame_ex(*none8, 1, 1, prefs(block_mode=1, compression_level=10), link, None, 0) == -104
    assert L.zlz4f_batch_compress_frame_ex(*none8, 1, 1, prefs(content_size=5), 1, None, 0) == -104
    for bits in (2, 8, 4 | 2, 4 | 8):
        assert L.zlz4f_batch_compress_frame_ex(*none8, 1, 1, prefs(compression_level=9), bits, None, 0) == -104
        assert L.zlz4f_compress_frame_device_ex(None, None, 0, None, 0, None, bits) == -104
    assert L.zlz4f_compress_frame_ex(None, 0, None, 0, prefs(compression_level=9), 8) == -104
    assert L.zlz4f_compress_frame_ex(None, 0, None, 0, prefs(block_mode=1), link) == -104
    # the plain call keeps its answer
    assert L.zlz4f_batch_compress_frame(*none8, 1, 1, prefs(compression_level=9), link, None, 0) == -8
    if not zl.device_available():
        with pytest.raises(zl.Lz4Error) as e:
            zl.lz4f.compressFrame(b"abc" * 100, prefs(compression_level=9), flags=link)
        assert e.value.name == "DeviceError"


def test_workspace_holds_no_staged_copy_and_is_unchanged_elsewhere(zl):
    L = zl.lib()
    link = zl.lz4f.BATCH_LINK_BLOCKS
    m = 4
    fast, hc = zl.Prefs(), zl.Prefs()
    hc.compression_level = 9
    ws = L.zlz4f_batch_compress_frame_workspace_ex(1, m, hc, link)
    plain = L.zlz4f_batch_compress_frame_workspace(1, m, fast)
    staged = L.zlz4_batch_compress_hc_using_dict_workspace(m, 65536, 65536)
    assert staged > m * 131072 * 13                    # links, results and the staged tail ++ record per entry
    assert plain + m * 131072 * 12 < ws <= plain + staged - m * 65536
    for level in (3, 1):                               # one size for the levels 3..9
        hc.compression_level = level
        assert L.zlz4f_batch_compress_frame_workspace_ex(1, m, hc, link) == ws
    # every other combination: the expressions of test_linked_frame_cpu.py
    for nf, mb in ((1, 0), (3, 7), (4096, 65536)):
        assert L.zlz4f_batch_compress_frame_workspace_ex(nf, mb, fast, 0) == L.zlz4f_batch_compress_frame_workspace(nf, mb, fast)
        assert L.zlz4f_batch_compress_frame_workspace_ex(nf, mb, fast, link) >= \
            L.zlz4f_batch_compress_frame_workspace(nf, mb, fast) + mb * (16384 + 12)
        assert L.zlz4f_batch_compress_frame_workspace_ex(nf, mb, fast, link) < \
            L.zlz4f_batch_compress_frame_workspace(nf, mb, fast) + mb * (16384 + 20) + 4 * 256
        for level in (2, 9, 10):
            hc.compression_level = level
            assert L.zlz4f_batch_compress_frame_workspace_ex(nf, mb, hc, 0) == L.zlz4f_batch_compress_frame_workspace(nf, mb, hc)
            assert L.zlz4f_batch_compress_frame_workspace_ex(nf, mb, hc, 1) == L.zlz4f_batch_compress_frame_workspace(nf, mb, hc)


def test_fixture_file_is_what_the_generator_describes(model_frames):
    entries = json.load(open(FIXTURES))["frames"]
    assert [(e["name"], e["level"]) for e in entries] == [(r["name"], lv) for r in lg.RECIPES for lv in LEVELS]
    for e in entries:
        data, frame = model_frames[e["name"], e["level"]]
        assert e["recipe"] == [r for r in lg.RECIPES if r["name"] == e["name"]][0]
        assert hashlib.sha256(data).hexdigest() == e["input_sha256"]
        assert len(frame) == e["frame_len"] and hashlib.sha256(frame).hexdigest() == e["frame_sha256"], (e["name"], e["level"])
    assert os.path.getsize(FIXTURES) < (1 << 20)
