"""lz4f dictionary frames on the HIP path: zlz4f_batch_compress_frame_using_dict, zlz4f_batch_decompress_frame_using_dict,
zlz4f_batch_frame_decompressed_size_using_dict, zlz4f_batch_frame_dict_id and the single-frame host calls, byte for byte and
status for status against the CPU model tools/pyref/zig_lz4_dict_frame.py (itself held against liblz4 in
test_dict_frame_cpu.py) and against liblz4's own frames (tests/golden/dict_frames.json).  Every destination slot is fenced by
guard bytes.  Run on the GPU box: pytest -m gpu."""
import os
import sys

import numpy as np
import pytest

import datagen as dg
import dictframegen as dfg
import dictgen
import linkedgen as lg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "pyref"))
import zig_lz4_dict_frame as df  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5
DICT_LENS = (0, 4, 5, 1000, 65536, 100000)
# (frame length, dictionary number): every length of the contract, every dictionary length, long frames with and without
PAIRS = ((0, 3), (1, 1), (12, 2), (13, 0), (1000, 3), (1000, 5), (65536, 4), (65537, 5), (150000, 5), (150000, 0),
         (65537, 3), (1000, 1), (13, 4), (1000, 0))


def _prefs(P, **kw):
    p = P()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _stage(items, gpu):
    """Byte strings back to back at odd offsets (1 + a few bytes of gap) -> tensor, int64 offsets, int64 lengths."""
    import torch
    offs, pos = [], 1
    for b in items:
        offs.append(pos)
        pos += len(b) + 3
    buf = np.zeros(max(pos, 1), dtype=np.uint8)
    for o, b in zip(offs, items):
        if b:
            buf[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return (torch.from_numpy(buf).to(gpu), torch.tensor(offs, dtype=torch.int64, device=gpu),
            torch.tensor([len(b) for b in items], dtype=torch.int64, device=gpu))


def _stage_dicts(dicts, idx, gpu):
    import torch
    d, off, ln = _stage(dicts, gpu)
    t_idx = None if idx is None else torch.tensor(list(idx), dtype=torch.int32, device=gpu)
    return d, off, ln.to(torch.int32), t_idx


def _slots(caps, gpu):
    """Destination slots at odd offsets, each followed (and the first preceded) by GUARD bytes of FILL."""
    import torch
    offs, pos = [], GUARD + 1
    for c in caps:
        offs.append(pos)
        pos += c + GUARD
    d = torch.full((pos,), FILL, dtype=torch.uint8, device=gpu)
    return d, offs, torch.tensor(offs, dtype=torch.int64, device=gpu), torch.tensor(caps, dtype=torch.int64, device=gpu)


def _collect(d_dst, offs, caps, result):
    res = result.cpu().tolist()
    host = d_dst.cpu().numpy()
    outside = np.ones(len(host), dtype=bool)
    for o, c in zip(offs, caps):
        outside[o:o + c] = False
    assert (host[outside] == FILL).all(), "bytes outside the destination slots were written"
    raw = host.tobytes()
    return res, [raw[o:o + r] if r >= 0 else None for o, r in zip(offs, res)]


def _compress(zl, gpu, items, prefs, flags, dicts, idx, max_src_len=0, max_dict_len=65536, max_blocks=None):
    import torch
    caps = [zl.lz4f.compressFrameBound(len(b), prefs) for b in items]
    d_src, s_off, s_len = _stage(items, gpu)
    d_dict, k_off, k_len, t_idx = _stage_dicts(dicts, idx, gpu)
    d_dst, offs, t_off, t_cap = _slots(caps, gpu)
    result = torch.full((len(items),), -999, dtype=torch.int64, device=gpu)
    zl.lz4f.compressFrameUsingDictBatch(d_src, s_off, s_len, d_dst, t_off, t_cap, result, d_dict, k_off, k_len, t_idx, prefs,
                                        flags, max_blocks, max_src_len, max_dict_len)
    return _collect(d_dst, offs, caps, result)


def _decompress(zl, gpu, frames, caps, dicts, idx, max_blocks=None):
    import torch
    if max_blocks is None:
        max_blocks = sum(zl._chain_blocks(f) for f in frames)
    d_src, s_off, s_len = _stage(frames, gpu)
    d_dict, k_off, k_len, t_idx = _stage_dicts(dicts, idx, gpu)
    d_dst, offs, t_off, t_cap = _slots(caps, gpu)
    result = torch.full((len(frames),), -999, dtype=torch.int64, device=gpu)
    zl.lz4f.decompressFrameUsingDictBatch(d_src, s_off, s_len, d_dst, t_off, t_cap, result, d_dict, k_off, k_len, t_idx,
                                          max_blocks)
    return _collect(d_dst, offs, caps, result)


def _sizes(zl, gpu, frames, dicts, idx, max_blocks=None):
    import torch
    if max_blocks is None:
        max_blocks = sum(zl._chain_blocks(f) for f in frames)
    d_src, s_off, s_len = _stage(frames, gpu)
    k_len = torch.tensor([len(d) for d in dicts], dtype=torch.int32, device=gpu)
    t_idx = None if idx is None else torch.tensor(list(idx), dtype=torch.int32, device=gpu)
    size = torch.full((len(frames),), -999, dtype=torch.int64, device=gpu)
    zl.lz4f.frameDecompressedSizeUsingDictBatch(d_src, s_off, s_len, size, k_len, t_idx, max_blocks)
    return size.cpu().tolist()


def _check_against_model(zl, gpu, frames, caps, dicts, idx, max_blocks=None):
    """Decode and size query against the model -> the decode results."""
    pick = (lambda k: dicts[0]) if idx is None else (lambda k: dicts[idx[k]])
    res, outs = _decompress(zl, gpu, frames, caps, dicts, idx, max_blocks)
    sizes = _sizes(zl, gpu, frames, dicts, idx, max_blocks)
    bad = []
    for k, (f, c) in enumerate(zip(frames, caps)):
        want, want_bytes = df.decompress_frame_using_dict(f, c, pick(k))
        if res[k] != want or (want >= 0 and outs[k] != want_bytes):
            bad.append(("decode", k, res[k], want))
        want_size = df.frame_size_using_dict(f, len(pick(k)))
        if sizes[k] != want_size:
            bad.append(("size", k, sizes[k], want_size))
    assert not bad, (len(bad), bad[:8])
    return res


@pytest.fixture(scope="module")
def fx():
    return dfg.fixtures()


@pytest.fixture(scope="module")
def dicts():
    big = dfg.recipe_dict(dfg.RECIPES[0])
    return [big[len(big) - n:] for n in DICT_LENS]


def _item(d, n, seed):
    """n bytes that match the dictionary's tail (text of their own for a dictionary of a few bytes)."""
    base = d[-60000:] if len(d) >= 1000 else bytes(dg.text_bytes(60000, seed))
    b = bytearray((base * (n // len(base) + 1))[:n])
    for i in range(0, n, 1000 if n > 1000 else 100):
        b[i] ^= 0x55
    return bytes(b)


@pytest.fixture(scope="module")
def own(zl, gpu, dicts):
    """The frames of PAIRS compressed once per preference set: (kw, flags, items, idx, results, frames, model frames)."""
    out = []
    for kw, cs, pairs in ((dict(block_mode=0), False, PAIRS), (dict(block_mode=1), False, PAIRS),
                          (dict(block_mode=0, block_checksum=1, content_checksum=1, dict_id=9), True, PAIRS[:8]),
                          (dict(block_mode=1, block_checksum=1, content_checksum=1), True, PAIRS[:8])):
        items = [_item(dicts[k], n, 40 + j) for j, (n, k) in enumerate(pairs)]
        idx = [k for _, k in pairs]
        flags = zl.lz4f.BATCH_CONTENT_SIZE if cs else 0
        res, frames = _compress(zl, gpu, items, _prefs(zl.Prefs, **kw), flags, dicts, idx)
        model = [df.compress_frame_using_dict(b, dicts[k], dict(kw, content_size=len(b) if cs else 0))
                 for b, k in zip(items, idx)]
        out.append((kw, flags, items, idx, res, frames, model))
    return out


# ------------------------------------------------------------------ 1. liblz4's dictionary frames
def test_fixtures_decode_only_with_their_dictionary(zl, gpu, fx):
    import torch
    frames = [f["frame"] for f in fx]
    caps = [len(f["input"]) for f in fx]
    mb = sum(zl._chain_blocks(f) for f in frames)
    # the existing calls still fail on them: block 0 points in front of the frame
    d_src, s_off, s_len = _stage(frames, gpu)
    d_dst, offs, t_off, t_cap = _slots(caps, gpu)
    result = torch.full((len(frames),), -999, dtype=torch.int64, device=gpu)
    zl.lz4f.decompressFrameBatch(d_src, s_off, s_len, d_dst, t_off, t_cap, result, mb, flags=zl.lz4f.DECODE_LINKED)
    assert _collect(d_dst, offs, caps, result)[0] == [-116] * len(fx)
    dicts = [fx[0]["dict"]]                                            # one shared dictionary, NULL index
    assert all(f["dict"] == dicts[0] for f in fx)
    res, outs = _decompress(zl, gpu, frames, caps, dicts, None)
    assert res == caps and outs == [f["input"] for f in fx]
    assert _sizes(zl, gpu, frames, dicts, None) == caps
    res, _ = _decompress(zl, gpu, frames, [c - 1 for c in caps], dicts, None)
    assert res == [-116] * len(fx)
    assert _decompress(zl, gpu, frames, caps, [b""], None)[0] == [-116] * len(fx)
    assert _sizes(zl, gpu, frames, [b""], None) == [-116] * len(fx)
    _check_against_model(zl, gpu, frames, caps, dicts, None)
    for f in fx:
        assert zl.lz4f.decompressFrameUsingDict(f["frame"], len(f["input"]), f["dict"]) == f["input"]
        assert zl.lz4f.frameDecompressedSizeUsingDict(f["frame"], len(f["dict"])) == len(f["input"])
    with pytest.raises(zl.Lz4Error) as e:
        zl.lz4f.decompressFrameUsingDict(fx[0]["frame"], caps[0], b"")
    assert e.value.code == -116
    assert zl.lz4f.frameDictIDs(frames + [b"abc"]) == [f["recipe"]["dict_id"] for f in fx] + [-112]
    assert zl.lz4f.decompressFramesUsingDict(frames, dicts) == [f["input"] for f in fx]


# ------------------------------------------------------------------ 2. compress against the model
def test_compress_gives_the_models_bytes(own):
    for kw, flags, items, idx, res, frames, model in own:
        assert res == [len(m) for m in model], (kw, res)
        assert frames == model, kw


def test_own_frames_round_trip(zl, gpu, own, dicts):
    z = dfg.liblz4fd()
    for kw, flags, items, idx, res, frames, model in own:
        assert _check_against_model(zl, gpu, frames, [len(b) for b in items], dicts, idx) == [len(b) for b in items]
        got, outs = _decompress(zl, gpu, frames, [len(b) for b in items], dicts, idx)
        assert outs == items
        if z is not None:
            for f, b, k in zip(frames, items, idx):
                assert z.decompress(f, len(b), dicts[k]) == b


def test_block_0_is_the_dictionary_compressors_block(zl, own, dicts):
    for kw, flags, items, idx, res, frames, model in own[:2]:
        for f, b, k in zip(frames, items, idx):
            if not b:
                continue
            h = int.from_bytes(f[7:11], "little")
            x0 = b[:65536]
            want = zl.compressFastUsingDict(x0, dicts[k])
            if h & 0x80000000:
                assert len(want) >= len(x0) and f[11:11 + len(x0)] == x0
            else:
                assert f[11:11 + h] == want


def test_empty_dictionary_gives_the_existing_calls(zl, gpu, own):
    import torch
    for kw, flags, items, idx, res, frames, model in own:
        sel = [j for j, k in enumerate(idx) if k == 0]
        assert sel
        sub = [items[j] for j in sel]
        p = _prefs(zl.Prefs, **kw)
        old = flags | (zl.lz4f.BATCH_LINK_BLOCKS if kw["block_mode"] == 0 else 0)
        caps = [zl.lz4f.compressFrameBound(len(b), p) for b in sub]
        d_src, s_off, s_len = _stage(sub, gpu)
        d_dst, offs, t_off, t_cap = _slots(caps, gpu)
        result = torch.full((len(sub),), -999, dtype=torch.int64, device=gpu)
        zl.lz4f.compressFrameBatch(d_src, s_off, s_len, d_dst, t_off, t_cap, result, p, old)
        r, fr = _collect(d_dst, offs, caps, result)
        assert r == [res[j] for j in sel] and fr == [frames[j] for j in sel]
    # the single-frame host call, both block modes, with and without a dictionary
    data = items[4]
    for mode in (0, 1):
        p = _prefs(zl.Prefs, block_mode=mode)
        assert zl.lz4f.compressFrameUsingDict(data, b"", p) == df.compress_frame_using_dict(data, b"", dict(block_mode=mode))


def test_single_frame_host_calls(zl, own, dicts):
    kw, flags, items, idx, res, frames, model = own[0]
    for j in (4, 7, 8):
        p = _prefs(zl.Prefs, **kw)
        assert zl.lz4f.compressFrameUsingDict(items[j], dicts[idx[j]], p) == model[j]
        assert zl.lz4f.decompressFrameUsingDict(model[j], len(items[j]), dicts[idx[j]]) == items[j]
    with pytest.raises(zl.Lz4Error) as e:
        zl.lz4f.compressFrameUsingDict(items[4], dicts[3], _prefs(zl.Prefs, compression_level=9))
    assert e.value.code == -8
    assert zl.lib().zlz4f_compress_frame_using_dict(None, 0, None, 0, None, None, 5) == -5      # dict NULL, dict_len > 0
    assert zl.lib().zlz4f_decompress_frame_using_dict(None, 0, None, 0, None, 5) == -5


# ------------------------------------------------------------------ 3. crafted frames
def test_crafted_frames(zl, gpu):
    cases = dfg.crafted_cases()
    ds, idx = [], []
    for c in cases:
        if c[2] not in ds:
            ds.append(c[2])
        idx.append(ds.index(c[2]))
    frames, caps = [c[1] for c in cases], [c[3] for c in cases]
    res, outs = _decompress(zl, gpu, frames, caps, ds, idx)
    for k, (name, frame, dct, cap, want, want_bytes, valid) in enumerate(cases):
        assert res[k] == want and (want_bytes is None or outs[k] == want_bytes), (name, res[k], want)
    _check_against_model(zl, gpu, frames, caps, ds, idx)
    # every case alone as well: a batch of one through the host call
    for name, frame, dct, cap, want, want_bytes, valid in cases[:6]:
        r = zl.lib().zlz4f_frame_decompressed_size_using_dict(frame, len(frame), len(dct))
        assert r == df.frame_size_using_dict(frame, len(dct)), name


# ------------------------------------------------------------------ 4. a foreign frame of short blocks
def test_foreign_frame_of_short_blocks(zl, gpu, tmp_path):
    enc = dictgen.encoder(tmp_path)
    r = dict(dfg.RECIPES[0], input_len=100000, flip_every=333)
    T, text = dfg.recipe_dict(r)[-65536:], dfg.recipe_input(r)
    frames = []
    for mode in (0, 1):
        blocks, reach = [], []
        for pos in range(0, len(text), 1000):
            hist = (T + text[:pos])[-65536:] if mode == 0 else T
            s, st = enc(hist, text[pos:pos + 1000])
            blocks.append((s, False))
            reach.append(st[0])
        # most blocks copy most of their bytes from their history; block 0's history is T alone
        assert sum(1 for x in reach if x > 500) > 80 and all(x > 500 for x in reach[:5]), reach
        frames.append(lg.build_frame(blocks, block_checksum=True, content=text, block_mode=mode))
    assert _check_against_model(zl, gpu, frames, [len(text)] * 2, [T], None) == [len(text)] * 2
    assert _decompress(zl, gpu, frames, [len(text)] * 2, [T], None)[1] == [text, text]
    assert _decompress(zl, gpu, frames, [len(text)] * 2, [b""], None)[0] == [-116, -116]     # T is reached
    z = dfg.liblz4fd()
    if z is not None:
        assert z.decompress(frames[0], len(text), T) == text and z.decompress(frames[1], len(text), T) == text


# ------------------------------------------------------------------ 5. refusals and preconditions
def test_refusals_launch_nothing(zl, gpu, dicts):
    import torch
    items = [_item(dicts[3], 1000, 1), _item(dicts[3], 70000, 2)]
    p = _prefs(zl.Prefs)
    caps = [zl.lz4f.compressFrameBound(len(b), p) for b in items]
    d_src, s_off, s_len = _stage(items, gpu)
    d_dict, k_off, k_len, _ = _stage_dicts(dicts, None, gpu)
    d_dst, offs, t_off, t_cap = _slots(caps, gpu)
    result = torch.full((2,), -999, dtype=torch.int64, device=gpu)
    need = zl.lz4f.compressFrameUsingDictBatchWorkspace(2, 3, p, 0, len(dicts), 0, 65536)
    ws = torch.empty(need + 16, dtype=torch.uint8, device=gpu)

    def call(prefs, flags, w):
        with pytest.raises(zl.Lz4Error) as e:
            zl.lz4f.compressFrameUsingDictBatch(d_src, s_off, s_len, d_dst, t_off, t_cap, result, d_dict, k_off, k_len, None,
                                                prefs, flags, 3, 0, 65536, w)
        return e.value.code

    assert call(p, 2, ws) == -104
    assert call(p, zl.lz4f.BATCH_LINK_BLOCKS, ws) == -104
    assert call(_prefs(zl.Prefs, content_size=5), zl.lz4f.BATCH_CONTENT_SIZE, ws) == -104
    assert call(_prefs(zl.Prefs, compression_level=9), 0, ws) == -8
    assert call(_prefs(zl.Prefs, compression_level=9), 2, ws) == -104          # parameter errors come first
    assert call(p, 0, ws[:need - 1]) == -5
    assert call(p, 0, ws[1:need + 1]) == -5
    torch.cuda.synchronize()
    assert result.cpu().tolist() == [-999, -999]
    assert (d_dst.cpu().numpy() == FILL).all()
    # decode and size query: a workspace that is too small or misaligned
    frames = [df.compress_frame_using_dict(b, dicts[3]) for b in items]
    f_src, f_off, f_len = _stage(frames, gpu)
    o_dst, o_offs, o_off, o_cap = _slots([len(b) for b in items], gpu)
    need = zl.lz4f.decompressFrameUsingDictBatchWorkspace(2, 3)
    ws = torch.empty(need + 16, dtype=torch.uint8, device=gpu)
    for w in (ws[:need - 1], ws[1:need + 1]):
        with pytest.raises(zl.Lz4Error) as e:
            zl.lz4f.decompressFrameUsingDictBatch(f_src, f_off, f_len, o_dst, o_off, o_cap, result, d_dict, k_off, k_len, None,
                                                  3, w)
        assert e.value.code == -5
    need = zl.lz4f.frameDecompressedSizeUsingDictBatchWorkspace(2, 3)
    ws = torch.empty(need + 16, dtype=torch.uint8, device=gpu)
    for w in (ws[:need - 1], ws[1:need + 1]):
        with pytest.raises(zl.Lz4Error) as e:
            zl.lz4f.frameDecompressedSizeUsingDictBatch(f_src, f_off, f_len, result, k_len, None, 3, w)
        assert e.value.code == -5
    torch.cuda.synchronize()
    assert result.cpu().tolist() == [-999, -999] and (o_dst.cpu().numpy() == FILL).all()


def test_preconditions_fail_one_frame_only(zl, gpu, dicts):
    three = [dicts[3], dicts[5], dicts[1]]                             # ndicts = 3, mixed index
    idx = [0, 1, 2, 1, 0, 7]
    items = [_item(three[k % 3], n, 60 + j) for j, (n, k) in enumerate(zip((1000, 70000, 500, 2000, 1500, 800), idx))]
    for mode in (0, 1):
        kw = dict(block_mode=mode)
        p = _prefs(zl.Prefs, **kw)
        want = [df.compress_frame_using_dict(b, three[k], kw) if k < 3 else -5 for b, k in zip(items, idx)]
        # (a) an index out of range
        res, frames = _compress(zl, gpu, items, p, 0, three, idx)
        assert res == [len(w) if w != -5 else -5 for w in want] and frames[:5] == want[:5]
        # (b) max_src_len exceeded by frame 1 (70 000 > 2 000): with the bound every frame is one block
        res, frames = _compress(zl, gpu, items, p, 0, three, idx, max_src_len=2000)
        assert res[1] == -5 and res[5] == -5 and [frames[j] for j in (0, 2, 3, 4)] == [want[j] for j in (0, 2, 3, 4)]
        # (c) max_dict_len exceeded by dictionary 1 (T = 65 536 > 1 000)
        res, frames = _compress(zl, gpu, items, p, 0, three, idx, max_dict_len=1000)
        assert [res[j] for j in (1, 3, 5)] == [-5] * 3 and [frames[j] for j in (0, 2, 4)] == [want[j] for j in (0, 2, 4)]
        # (d) a block table that ends inside frame 1 (two blocks): that frame and no other... the later ones have no room
        res, frames = _compress(zl, gpu, items, p, 0, three, idx, max_blocks=2)
        assert res[0] == len(want[0]) and frames[0] == want[0] and res[1] == -5
        # decode: the same index and table preconditions
        good = [w for w in want if w != -5]
        caps = [len(b) for b in items[:5]]
        res, outs = _decompress(zl, gpu, good + [good[0]], caps + [caps[0]], three, idx)
        assert res == caps + [-5] and outs[:5] == items[:5]
        assert _sizes(zl, gpu, good + [good[0]], three, idx) == caps + [-5]
        res, outs = _decompress(zl, gpu, good, caps, three, idx[:5], max_blocks=2)
        assert res[0] == caps[0] and outs[0] == items[0] and res[1] == -5
        assert _sizes(zl, gpu, good, three, idx[:5], max_blocks=2)[:2] == [caps[0], -5]


# ------------------------------------------------------------------ 6. graph capture
def test_dictionary_batches_in_a_captured_graph(zl, gpu, dicts):
    import torch
    n = 24
    three = [dicts[3], dicts[5], dicts[0]]
    idx = [k % 3 for k in range(n)]
    items = [_item(three[k % 3], 1500 + 500 * (k % 5) + (140000 if k % 8 == 1 else 0), 100 + k) for k in range(n)]
    items2 = [bytes(dg.mixed_bytes(len(b), 700 + k)) for k, b in enumerate(items)]
    kw = dict(block_mode=0, block_checksum=1, content_checksum=1, dict_id=77)
    p = _prefs(zl.Prefs, **kw)
    caps = [zl.lz4f.compressFrameBound(len(b), p) for b in items]
    max_blocks = sum((len(b) + 65535) // 65536 for b in items)
    d_src, s_off, s_len = _stage(items, gpu)
    d_dict, k_off, k_len, t_idx = _stage_dicts(three, idx, gpu)
    d_frm, f_offs, t_foff, t_fcap = _slots(caps, gpu)
    d_out, o_offs, t_ooff, t_ocap = _slots([len(b) for b in items], gpu)
    cres, dres, qres, ires = (torch.zeros(n, dtype=torch.int64, device=gpu) for _ in range(4))
    cws = torch.empty(zl.lz4f.compressFrameUsingDictBatchWorkspace(n, max_blocks, p, 0, 3, 0, 65536), dtype=torch.uint8,
                      device=gpu)
    dws = torch.empty(zl.lz4f.decompressFrameUsingDictBatchWorkspace(n, max_blocks), dtype=torch.uint8, device=gpu)
    qws = torch.empty(zl.lz4f.frameDecompressedSizeUsingDictBatchWorkspace(n, max_blocks), dtype=torch.uint8, device=gpu)

    def run():
        zl.lz4f.compressFrameUsingDictBatch(d_src, s_off, s_len, d_frm, t_foff, t_fcap, cres, d_dict, k_off, k_len, t_idx, p,
                                            0, max_blocks, 0, 65536, cws)
        zl.lz4f.decompressFrameUsingDictBatch(d_frm, t_foff, cres, d_out, t_ooff, t_ocap, dres, d_dict, k_off, k_len, t_idx,
                                              max_blocks, dws)
        zl.lz4f.frameDecompressedSizeUsingDictBatch(d_frm, t_foff, cres, qres, k_len, t_idx, max_blocks, qws)
        zl.lz4f.frameDictIDBatch(d_frm, t_foff, cres, ires)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    for batch in (items2, items):
        d2, _, _ = _stage(batch, gpu)
        d_src.copy_(d2)
        for t in (cres, dres, qres, ires):
            t.fill_(-999)
        g.replay()
        torch.cuda.synchronize()
        c, d, q = cres.cpu().tolist(), dres.cpu().tolist(), qres.cpu().tolist()
        assert ires.cpu().tolist() == [77] * n
        frm = d_frm.cpu().numpy().tobytes()
        out = d_out.cpu().numpy().tobytes()
        for k, b in enumerate(batch):
            want = df.compress_frame_using_dict(b, three[idx[k]], kw)
            assert c[k] == len(want) and frm[f_offs[k]:f_offs[k] + c[k]] == want, k
            assert d[k] == len(b) == q[k] and out[o_offs[k]:o_offs[k] + d[k]] == b, k
