"""The CPU model of lz4f dictionary frames (tools/pyref/zig_lz4_dict_frame.py) held against liblz4's own dictionary frames
(tests/golden/dict_frames.json, and fresh ones where liblz4 loads), against liblz4's decoder, against the models it is
built from and against hand-made frames whose results follow from the contract (include/zlz4_amd.h).  No GPU."""
import os
import sys

import pytest

import datagen as dg
import dictframegen as dfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "pyref"))
import zig_lz4_dict_frame as df  # noqa: E402
import zig_lz4_linked_frame as lf  # noqa: E402


@pytest.fixture(scope="module")
def fx():
    return dfg.fixtures()


@pytest.fixture(scope="module")
def z():
    lib = dfg.liblz4fd()
    if lib is None:
        pytest.skip("no liblz4.so.1 with the dictionary frame calls")
    return lib


def test_fixtures_cover_what_the_contract_asks_for(fx):
    by = {f["name"]: f for f in fx}
    assert len(fx) == 5 and os.path.getsize(dfg.FIXTURES) <= 160 * 1024
    for f in fx:
        assert len(f["dict"]) > 65536                                  # only the tail counts
    big = [f for f in fx if len(f["input"]) == 150000]
    assert sorted((f["recipe"]["level"], f["recipe"]["linked"]) for f in big) == [(0, 0), (0, 1), (9, 0), (9, 1)]
    for f in big:
        assert bool(f["frame"][4] & 0x20) == (not f["recipe"]["linked"])
    c = by["l9_linked_checksums_dictid"]["frame"]
    assert c[4] & 0x10 and c[4] & 0x04 and c[4] & 0x01 and int.from_bytes(c[6:10], "little") == 0x1234ABCD
    assert len(by["l0_record_1000"]["input"]) == 1000


def test_model_decodes_the_fixtures_and_needs_the_dictionary(fx):
    for f in fx:
        n = len(f["input"])
        assert df.decompress_frame_using_dict(f["frame"], n, f["dict"]) == (n, f["input"]), f["name"]
        assert df.decompress_frame_using_dict(f["frame"], n, f["dict"][-65536:]) == (n, f["input"])    # T is what counts
        assert df.frame_size_using_dict(f["frame"], len(f["dict"])) == n
        assert df.decompress_frame_using_dict(f["frame"], n - 1, f["dict"])[0] == -116
        assert df.decompress_frame_using_dict(f["frame"], n, b"")[0] == -116
        assert df.frame_size_using_dict(f["frame"], 0) == -116
        assert lf.decompress_frame_linked(f["frame"], n)[0] == -116
        assert lf.frame_size_linked(f["frame"]) == -116


def test_later_linked_blocks_decode_with_the_output_alone(fx):
    """Block sizes are >= 64 KiB, so from block 1 on a linked frame's history is its own output: blocks 1 and 2 of
    liblz4's frame decode against the 64 KiB of input in front of them, without the dictionary."""
    f = [x for x in fx if x["name"] == "l0_linked"][0]
    from zig_lz4_dict import decompress_safe_using_dict
    frame, pos, out = f["frame"], 7, bytearray()
    k = 0
    while True:
        h = int.from_bytes(frame[pos:pos + 4], "little")
        pos += 4
        if h == 0:
            break
        body = frame[pos:pos + (h & 0x7FFFFFFF)]
        pos += len(body)
        if k >= 1 and not h & 0x80000000:
            r, got = decompress_safe_using_dict(body, 65536, f["input"][len(out) - 65536:len(out)])
            assert r == len(got) and got == f["input"][len(out):len(out) + r]
        out += f["input"][len(out):len(out) + 65536]
        k += 1
    assert k == 3


def test_fresh_liblz4_frames_decode_under_the_model(z):
    r = dfg.RECIPES[0]
    d, data = dfg.recipe_dict(r), dfg.recipe_input(r)
    for level in (0, 9):
        for linked in (True, False):
            for dct in (d, d[-1000:], d[-5:]):
                frame = z.compress(data, dct, level, linked, 4, 1, 1, 99)
                assert df.decompress_frame_using_dict(frame, len(data), dct) == (len(data), data)
                assert df.frame_size_using_dict(frame, len(dct)) == len(data)


def test_liblz4_decodes_the_models_frames(z):
    r = dfg.RECIPES[0]
    d = dfg.recipe_dict(r)
    text = bytes(dg.text_bytes(70000, 3))
    for data in (dfg.recipe_input(r), dfg.recipe_input(dfg.RECIPES[4]), text, b"", b"x"):
        for mode in (0, 1):
            for dct in (d, d[-1000:], b""):
                frame = df.compress_frame_using_dict(data, dct, dict(block_mode=mode, block_checksum=1, content_checksum=1,
                                                                     dict_id=5))
                assert bool(frame[4] & 0x20) == (mode == 1)
                assert z.decompress(frame, len(data), dct) == data
                assert df.decompress_frame_using_dict(frame, len(data), dct) == (len(data), data)


def test_frames_use_their_dictionary(fx):
    f = fx[0]
    plain = lf.compress_frame_linked(f["input"])
    for mode in (0, 1):
        frame = df.compress_frame_using_dict(f["input"], f["dict"], dict(block_mode=mode))
        assert len(frame) < len(plain) // 2
        assert df.decompress_frame_using_dict(frame, len(f["input"]), b"")[0] == -116


def test_empty_dictionary_gives_the_existing_frames(oracle):
    data = dfg.recipe_input(dfg.RECIPES[0])
    for item in (data, data[:65537], data[:1000], b"", b"a"):
        for kw in (dict(), dict(block_checksum=1, content_checksum=1, dict_id=3, content_size=77)):
            assert df.compress_frame_using_dict(item, b"", dict(kw, block_mode=0)) == lf.compress_frame_linked(item, kw)
            p = oracle.Prefs()
            p.block_mode = 1
            for k, v in kw.items():
                setattr(p, k, v)
            assert df.compress_frame_using_dict(item, None, dict(kw, block_mode=1)) == oracle.compress_frame(item, p)
    # and the decode is the linked decode
    for name, frame, cap, want, want_bytes in __import__("linkedgen").crafted_cases():
        r, out = df.decompress_frame_using_dict(frame, cap, b"")
        assert (r, out) == lf.decompress_frame_linked(frame, cap) and r == want, name
        assert df.frame_size_using_dict(frame, 0) == lf.frame_size_linked(frame)


def test_crafted_cases(z):
    for name, frame, dct, cap, want, want_bytes, valid in dfg.crafted_cases():
        r, out = df.decompress_frame_using_dict(frame, cap, dct)
        assert r == want and (want_bytes is None or out == want_bytes), name
        if valid:
            assert z.decompress(frame, cap, dct) == want_bytes, name
            assert df.frame_size_using_dict(frame, len(dct)) == want, name


def test_crafted_cases_model_only():
    """The same expectations where liblz4 does not load."""
    for name, frame, dct, cap, want, want_bytes, valid in dfg.crafted_cases():
        r, out = df.decompress_frame_using_dict(frame, cap, dct)
        assert r == want and (want_bytes is None or out == want_bytes), name
