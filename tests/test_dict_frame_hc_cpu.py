"""Dictionary frames at the HC levels 3..9 without a GPU: the CPU model
tools/pyref/zig_lz4_dict_frame_hc.py with the Python block compressor against the same model over the C restatement
(tests/hc_dict_ref.c), block by block against the block compressor, against the model's decoder and liblz4's, against the
frames without a dictionary, against the stated sizes and the fixture file; the public surface of the _ex calls (symbols,
the refusals that are host arithmetic, the workspace size)."""
import ctypes as C
import hashlib
import os
import re
import sys

import pytest

import dictcgen as dc
import dictframegen as dfg
import dictframehcgen as hcg
import hcdictcgen as hg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "pyref"))
import zig_lz4_dict_frame as df  # noqa: E402
import zig_lz4_dict_frame_hc as dh  # noqa: E402
import zig_lz4_linked_frame as lf  # noqa: E402
import zig_lz4_linked_frame_hc as lh  # noqa: E402

NEW = ("zlz4f_batch_compress_frame_using_dict_workspace_ex", "zlz4f_batch_compress_frame_using_dict_ex",
       "zlz4f_compress_frame_using_dict_ex")
KW = dict(block_checksum=1, content_checksum=1, dict_id=0x0D1C7)


@pytest.fixture(scope="module")
def cref(tmp_path_factory):
    return hg.ref(tmp_path_factory.mktemp("hc_dict_ref"))


@pytest.fixture(scope="module")
def frames(cref):
    """{(recipe name, level, block_mode): (dictionary, input, prefs, frame)}: the model over the C restatement, once"""
    by_c, out = hcg.model(cref), {}
    for name, level, mode in hcg.CASES:
        d, data = hcg.data_of(name)
        prefs = hcg.prefs_of(name, mode, **(KW if name == "three_blocks" else {}))
        out[name, level, mode] = (d, data, prefs, by_c(data, d, level, prefs))
    return out


def test_restatements_agree(cref, frames):
    """the Python block compressor on the records; the three-block input is the fixture file's business (its generator
    records a frame only where the Python model gave the same bytes)"""
    for (name, level, mode), (d, data, prefs, frame) in frames.items():
        assert isinstance(frame, bytes) and bool(frame[4] & 0x20) == (mode == 1)
        if name in hcg.SMALL:
            assert dh.compress_frame_using_dict_hc(data, d, level, prefs) == frame, (name, level, mode)
    # the big input's dictionary too: its first 3000 bytes against the whole tail
    d, data = hcg.data_of("three_blocks")
    assert dh.compress_frame_using_dict_hc(data[:3000], d, 9) == hcg.model(cref)(data[:3000], d, 9)


def test_round_trip_under_the_model_and_size_query(frames):
    for key, (d, data, prefs, frame) in frames.items():
        assert df.decompress_frame_using_dict(frame, len(data), d) == (len(data), data), key
        assert df.frame_size_using_dict(frame, len(d)) == len(data), key
        assert df.decompress_frame_using_dict(frame, len(data), b"")[0] == -116, key      # block 0 reaches into T


def test_round_trip_under_liblz4(frames):
    z = dfg.liblz4fd()
    if z is None:
        pytest.skip("no liblz4.so.1 with the dictionary frame calls")
    for key, (d, data, prefs, frame) in frames.items():
        assert z.decompress(frame, len(data), d) == data, key


def test_blocks_are_the_block_compressors(cref, frames):
    for (name, level, mode), (d, data, prefs, frame) in frames.items():
        bs = lf.BLOCK_SIZES[prefs["block_size_id"]]
        blocks = lh.blocks_of(frame)
        assert len(blocks) == (len(data) + bs - 1) // bs
        for k, (payload, stored) in enumerate(blocks):
            x = data[k * bs:(k + 1) * bs]
            d_k = d[-65536:] if mode == 1 or k == 0 else data[k * bs - 65536:k * bs]
            n, want = cref.compress(x, d_k, level)
            if stored:
                assert n >= len(x) and payload == x, (name, level, mode, k)
            else:
                assert n < len(x) and payload == want, (name, level, mode, k)
    # a frame of random bytes: the block is stored as it is
    import datagen as dg
    rnd = bytes(dg.random_bytes(5000, 3))
    d = hcg.data_of("record_1000")[0]
    frame = hcg.model(cref)(rnd, d, 9, dict(block_mode=1))
    assert lh.blocks_of(frame) == [(rnd, True)]
    assert df.decompress_frame_using_dict(frame, len(rnd), d) == (len(rnd), rnd)


def test_empty_dictionary_gives_the_frames_without_one(cref, oracle):
    by_c = hcg.model(cref)
    big = hcg.data_of("three_blocks")[1]
    for item in (big, big[:65537], big[:1000], b"", b"a", big[:13]):
        for level in hcg.LEVELS + (1,):
            for kw in (dict(block_size_id=4), dict(KW, block_size_id=4, content_size=77)):
                linked = lh.compress_frame_linked_hc(item, level, kw, hcg.c_block(cref))
                assert by_c(item, b"", level, dict(kw, block_mode=0)) == linked, (len(item), level)
                p = oracle.Prefs()
                p.block_mode, p.compression_level = 1, level
                for k, v in kw.items():
                    setattr(p, k, v)
                assert by_c(item, None, level, dict(kw, block_mode=1)) == oracle.compress_frame(item, p), (len(item), level)


def test_the_dictionary_is_used(cref):
    """the six 4 KiB records of DESIGN.md section 4.3c's table as six frames against their 64 KiB dictionary: the block
    payloads are the table's, the container adds a 7-byte header, a block header and the end mark per frame"""
    d, recs = hcg.table_records()
    by_c = hcg.model(cref)
    container = 6 * (7 + 4 + 4)
    want = {3: 7835, 6: 6565, 9: 6304}
    fast = sum(len(df.compress_frame_using_dict(r, d, dict(block_mode=1))) for r in recs)
    assert fast == 10658 + container
    for mode in (0, 1):
        for level, payload in want.items():
            fr = [by_c(r, d, level, dict(block_mode=mode)) for r in recs]
            assert sum(len(lh.blocks_of(f)[0][0]) for f in fr) == payload
            assert sum(len(f) for f in fr) == payload + container < fast
    fastc = dc.ref(os.path.dirname(cref.L._name))
    assert sum(fastc.compress(r, d)[0] for r in recs) == 10658


def test_refused_levels():
    d, data = hcg.data_of("record_1000")
    for level in (2, 10, 11, 12, 13, 0, -1):
        for mode in (0, 1):
            assert dh.compress_frame_using_dict_hc(data, d, level, dict(block_mode=mode)) == -8
    assert dh.compress_frame_using_dict_hc(data, d, 1) == dh.compress_frame_using_dict_hc(data, d, 9)   # 1 runs as 9


def test_fixture_file_is_what_the_generator_describes(frames):
    entries = hcg.fixtures()
    assert [(e["name"], e["level"], e["prefs"]["block_mode"]) for e in entries] == list(hcg.CASES)
    for e in entries:
        d, data, prefs, frame = frames[e["name"], e["level"], e["prefs"]["block_mode"]]
        assert e["recipe"] == hcg.recipe(e["name"]) and e["prefs"] == prefs
        assert hashlib.sha256(d).hexdigest() == e["dict_sha256"] and hashlib.sha256(data).hexdigest() == e["input_sha256"]
        assert len(frame) == e["frame_len"] and hashlib.sha256(frame).hexdigest() == e["frame_sha256"], \
            (e["name"], e["level"], prefs["block_mode"])
    assert os.path.getsize(hcg.FIXTURES) < (1 << 20)


# ------------------------------------------------------------------ the surface of the _ex calls
def _prefs(zl, **kw):
    p = zl.Prefs()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_symbols_declared_and_exported(zl):
    hdr = open(os.path.join(ROOT, "include", "zlz4_amd.h")).read()
    L = C.CDLL(zl.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(L, name) and name in zl.SYMBOLS, name
    for name in ("compressFrameUsingDictEx", "compressFrameUsingDictBatchWorkspaceEx", "compressFrameUsingDictBatchEx"):
        assert hasattr(zl.lz4f, name), name


def test_refusals_are_host_arithmetic(zl):
    """Refused before the device is looked at, so the codes are the same with and without a GPU."""
    L = zl.lib()
    batch, one = L.zlz4f_batch_compress_frame_using_dict_ex, L.zlz4f_compress_frame_using_dict_ex
    none8 = (None,) * 8

    def call(prefs, flags):
        return batch(*none8, 1, 1, prefs, flags, None, None, None, 1, None, 0, 65536, None, 0)
    accepted = call(_prefs(zl, compression_level=9), 0)                 # no arrays: the device's answer or InvalidState
    assert accepted == (-5 if zl.device_available() else -7)
    for level in (3, 6, 1, 0):
        assert call(_prefs(zl, compression_level=level), 0) == accepted
        assert call(_prefs(zl, compression_level=level, block_mode=1), 1) == accepted
    for level in (2, 10, 11, 12, 13):
        assert call(_prefs(zl, compression_level=level), 0) == -8
        assert one(None, 0, None, 0, _prefs(zl, compression_level=level), None, 0) == -8
    for bits in (2, 4, 8, 1 | 2):
        assert call(_prefs(zl, compression_level=9), bits) == -104
        assert call(_prefs(zl, compression_level=10), bits) == -104     # parameter errors come first
    assert call(_prefs(zl, compression_level=9, content_size=5), 1) == -104
    # the host call: null pointers and a short destination are decided before the device
    p9 = _prefs(zl, compression_level=9)
    assert one(None, 0, None, 0, p9, None, 5) == -5                     # dict NULL, dict_len > 0
    assert one(None, 3, None, 0, p9, None, 0) == -5
    buf = (C.c_uint8 * 64)()
    assert one(C.addressof(buf), 20, C.addressof(buf), 5, p9, None, 0) == -111     # DstMaxSizeTooSmall
    # the plain calls keep their answer
    assert L.zlz4f_batch_compress_frame_using_dict(*none8, 1, 1, p9, 0, None, None, None, 1, None, 0, 65536, None, 0) == -8
    assert L.zlz4f_compress_frame_using_dict(None, 0, None, 0, p9, None, 0) == -8


def test_workspace_size(zl):
    L = zl.lib()
    ex, plain = L.zlz4f_batch_compress_frame_using_dict_workspace_ex, L.zlz4f_batch_compress_frame_using_dict_workspace
    block_ws, linked_ws = L.zlz4_batch_compress_hc_using_dict_workspace, L.zlz4f_batch_compress_frame_workspace_ex
    nf, m = 5, 64                                                      # (64 entries: every per-entry array is whole 256s)
    up = lambda n: (n + 255) & ~255
    # every level the HC branch does not serve: the plain call's size
    for level in (0, -2, 2, 10, 12, 13):
        for mode in (0, 1):
            p = _prefs(zl, compression_level=level, block_mode=mode)
            for args in ((0, 3, 0, 65536), (1, 1, 4096, 100), (0, 2, 70000, 0)):
                assert ex(nf, m, p, *args) == plain(nf, m, p, *args)
    # frames, table, slots and launch A's 20 bytes of descriptors: the plain call's size without a dictionary table
    base = plain(nf, m, _prefs(zl, block_mode=1), 0, 0, 4096, 0)
    hc = _prefs(zl, compression_level=9)
    linked_scratch = linked_ws(1, m, hc, zl.lz4f.BATCH_LINK_BLOCKS) - linked_ws(1, m, _prefs(zl), 0) - 20 * m
    for level in (3, 9, 1):
        ind = _prefs(zl, compression_level=level, block_mode=1)
        lnk = _prefs(zl, compression_level=level, block_mode=0)
        # one launch: the block call's scratch on top; max_dict_len and max_src_len size it
        for src, dl in ((4096, 61440), (4096, 65536), (0, 65536), (0, 0), (1000, 5), (65536, 65536)):
            got = ex(nf, m, ind, 0, 3, src, dl)
            assert got == base + up(block_ws(m, src if src else 65536, dl)), (level, src, dl)
            if src:                                                    # a bounded record is one block: no launch B
                assert ex(nf, m, lnk, 0, 3, src, dl) == got
        assert ex(nf, m, ind, 0, 3, 4096, 61440) < ex(nf, m, ind, 0, 3, 4096, 65536)     # LDS links are smaller
        assert ex(nf, m, ind, 0, 7, 4096, 61440) == ex(nf, m, ind, 1, 1, 4096, 61440)   # flags, ndicts: no effect
        # two launches share ONE scratch region, the larger of the two; launch B adds 32 bytes per entry
        for src, dl in ((0, 65536), (0, 100), (70000, 0)):
            a = up(block_ws(m, 65536, dl))
            assert ex(nf, m, lnk, 0, 3, src, dl) == base + max(a, linked_scratch) + 32 * m, (level, src, dl)
        assert up(block_ws(m, 65536, 0)) < linked_scratch < up(block_ws(m, 65536, 65536))   # (both orders occur above)
