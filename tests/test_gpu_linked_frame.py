"""Linked-block frames on the HIP path: zlz4f_batch_decompress_frame_ex / zlz4f_batch_frame_decompressed_size_ex with
ZLZ4F_DECODE_LINKED and zlz4f_batch_compress_frame with ZLZ4F_BATCH_LINK_BLOCKS, byte for byte and status for status
against the CPU model tools/pyref/zig_lz4_linked_frame.py (itself held against liblz4 in test_linked_frame_cpu.py) and
against liblz4's own frames (tests/golden/linked_frames.json).  Every destination slot is fenced by guard bytes.
Run on the GPU box: pytest -m gpu."""
import os
import sys

import numpy as np
import pytest

import datagen as dg
import dictgen
import linkedgen as lg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "pyref"))
import zig_lz4_linked_frame as lf  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5


def _prefs(P, **kw):
    p = P()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _stage(items, gpu):
    """Sources back to back at odd offsets (1 + a few bytes of gap)."""
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


def _compress(zl, gpu, items, prefs, flags):
    import torch
    caps = [zl.lz4f.compressFrameBound(len(b), prefs) for b in items]
    d_src, s_off, s_len = _stage(items, gpu)
    d_dst, offs, t_off, t_cap = _slots(caps, gpu)
    result = torch.full((len(items),), -999, dtype=torch.int64, device=gpu)
    zl.lz4f.compressFrameBatch(d_src, s_off, s_len, d_dst, t_off, t_cap, result, prefs, flags)
    return _collect(d_dst, offs, caps, result)


def _decompress(zl, gpu, frames, caps, flags, max_blocks=None):
    import torch
    if max_blocks is None:
        max_blocks = sum(zl._chain_blocks(f) for f in frames)
    d_src, s_off, s_len = _stage(frames, gpu)
    d_dst, offs, t_off, t_cap = _slots(caps, gpu)
    result = torch.full((len(frames),), -999, dtype=torch.int64, device=gpu)
    zl.lz4f.decompressFrameBatch(d_src, s_off, s_len, d_dst, t_off, t_cap, result, max_blocks, flags=flags)
    return _collect(d_dst, offs, caps, result)


def _sizes(zl, gpu, frames, flags, max_blocks=None):
    import torch
    if max_blocks is None:
        max_blocks = sum(zl._chain_blocks(f) for f in frames)
    d_src, s_off, s_len = _stage(frames, gpu)
    size = torch.full((len(frames),), -999, dtype=torch.int64, device=gpu)
    zl.lz4f.frameDecompressedSizeBatch(d_src, s_off, s_len, size, max_blocks, flags=flags)
    return size.cpu().tolist()


def _check_against_model(zl, gpu, frames, caps, max_blocks=None, model=None):
    """Decode and size query with the flag against the model (computed once per frame and shared) -> the results."""
    L = zl.lz4f.DECODE_LINKED
    if model is None:
        model = [(lf.decompress_frame_linked(f, c), lf.frame_size_linked(f)) for f, c in zip(frames, caps)]
    res, outs = _decompress(zl, gpu, frames, caps, L, max_blocks)
    sizes = _sizes(zl, gpu, frames, L, max_blocks)
    bad = []
    for k, ((want, want_bytes), want_size) in enumerate(model):
        if res[k] != want or (want >= 0 and outs[k] != want_bytes):
            bad.append(("decode", k, res[k], want))
        if sizes[k] != want_size:
            bad.append(("size", k, sizes[k], want_size))
    assert not bad, (len(bad), bad[:8])
    return res, sizes


@pytest.fixture(scope="module")
def fx():
    return lg.fixtures()


def _text_items():
    text = lg.recipe_input(lg.RECIPES[2])                              # period 40 000: every block matches its history
    rnd = bytes(dg.random_bytes(70000, 4))
    items = [text[:n] for n in (0, 1, 12, 65536, 65537, 200000)]
    items.append(rnd + rnd[:60000])                # the copy lies 70 000 back: out of reach, both blocks stored
    items.append(rnd[:65536] + rnd[1000:61000])    # 64 536 back: block 1 matches into the stored block 0
    return items


@pytest.fixture(scope="module")
def own(zl, gpu):
    """The linked frames of _text_items under two preference sets, compressed once: (kw, flags, items, results, frames)."""
    out = []
    for kw, cs in ((dict(), False), (dict(block_checksum=1, content_checksum=1), True)):
        flags = zl.lz4f.BATCH_LINK_BLOCKS | (zl.lz4f.BATCH_CONTENT_SIZE if cs else 0)
        items = _text_items()
        res, frames = _compress(zl, gpu, items, _prefs(zl.Prefs, **kw), flags)
        out.append((kw, cs, items, res, frames))
    return out


# ------------------------------------------------------------------ 1. liblz4's linked frames
def test_fixtures_need_the_flag_and_decode_with_it(zl, gpu, fx):
    frames = [f["frame"] for f in fx]
    caps = [len(f["input"]) for f in fx]
    res, _ = _decompress(zl, gpu, frames, caps, 0)
    assert res == [-116] * len(fx)                                     # as today: every block on its own
    assert _sizes(zl, gpu, frames, 0) == [-116] * len(fx)
    res, outs = _decompress(zl, gpu, frames, caps, zl.lz4f.DECODE_LINKED)
    assert res == caps and outs == [f["input"] for f in fx]
    assert _sizes(zl, gpu, frames, zl.lz4f.DECODE_LINKED) == caps
    assert zl.lz4f.decompressFrames(frames, flags=zl.lz4f.DECODE_LINKED) == [f["input"] for f in fx]
    for f in fx[:2]:                                                   # the single-frame calls
        n = len(f["input"])
        with pytest.raises(zl.Lz4Error) as e:
            zl.lz4f.decompressFrame(f["frame"], n)
        assert e.value.code == -116
        assert zl.lz4f.decompressFrame(f["frame"], n, zl.lz4f.DECODE_LINKED) == f["input"]
        assert zl.lz4f.frameDecompressedSize(f["frame"], zl.lz4f.DECODE_LINKED) == n
        with pytest.raises(zl.Lz4Error) as e:
            zl.lz4f.decompressFrame(f["frame"], n - 1, zl.lz4f.DECODE_LINKED)
        assert e.value.code == -116


def test_single_frame_device_call_equals_the_batch_call(zl, gpu, fx):
    import torch
    f = fx[1]
    d_src = torch.from_numpy(np.frombuffer(f["frame"], dtype=np.uint8).copy()).to(gpu)
    d_dst = torch.full((len(f["input"]) + 5,), FILL, dtype=torch.uint8, device=gpu)
    r = zl.lz4f.decompressFrameDevice(d_src, len(f["frame"]), d_dst[:len(f["input"])], zl.lz4f.DECODE_LINKED)
    host = d_dst.cpu().numpy()
    assert r == len(f["input"]) and host[:r].tobytes() == f["input"] and (host[r:] == FILL).all()
    with pytest.raises(zl.Lz4Error) as e:
        zl.lz4f.decompressFrameDevice(d_src, len(f["frame"]), d_dst[:len(f["input"])])
    assert e.value.code == -116


# ------------------------------------------------------------------ 2. frames written with BATCH_LINK_BLOCKS
def test_linked_compress_equals_the_model_and_round_trips(zl, gpu, own):
    for kw, cs, items, res, frames in own:
        for k, b in enumerate(items):
            want = lf.compress_frame_linked(b, dict(kw, content_size=len(b) if cs else 0))
            assert res[k] == len(want) and frames[k] == want, (kw, k, len(b), res[k], len(want))
        got, outs = _decompress(zl, gpu, frames, [len(b) for b in items], zl.lz4f.DECODE_LINKED)
        assert got == [len(b) for b in items] and outs == items, kw
        assert _sizes(zl, gpu, frames, zl.lz4f.DECODE_LINKED) == [len(b) for b in items]
    # the multi-block frames are really linked: without the flag their later blocks do not decode
    kw, cs, items, res, frames = own[0]
    plain, _ = _decompress(zl, gpu, frames, [len(b) for b in items], 0)
    assert plain[:4] == [0, 1, 12, 65536] and plain[5] == -116 and plain[7] == -116
    assert int.from_bytes(frames[7][7:11], "little") == 0x80000000 | 65536           # stored block 0 of the "near" frame
    assert int.from_bytes(frames[7][11 + 65536:15 + 65536], "little") < 55000        # block 1 matched into it


def test_linked_compress_block_0_is_compress_default(zl, gpu, oracle, own):
    kw, cs, items, res, frames = own[0]
    for k in (3, 4, 5):
        n0 = int.from_bytes(frames[k][7:11], "little")
        assert frames[k][11:11 + n0] == oracle.compress_default(items[k][:65536])
    q = _prefs(oracle.Prefs, block_mode=0)
    for k in (0, 1, 2, 3):                                             # a one-block frame is compressFrame's
        assert frames[k] == oracle.compress_frame(items[k], q)


def test_linked_compress_refusals(zl, gpu):
    import torch
    L = zl.lib()
    items = [b"a" * 70000]
    d_src, s_off, s_len = _stage(items, gpu)
    d_dst, offs, t_off, t_cap = _slots([zl.lz4f.compressFrameBound(70000)], gpu)
    result = torch.full((1,), -999, dtype=torch.int64, device=gpu)
    big = torch.empty(zl.lz4f.compressFrameBatchWorkspace(1, 2, None, zl.lz4f.BATCH_LINK_BLOCKS), dtype=torch.uint8, device=gpu)

    def call(prefs, flags, ws, ws_bytes):
        return L.zlz4f_batch_compress_frame(None, d_src.data_ptr(), s_off.data_ptr(), s_len.data_ptr(), d_dst.data_ptr(),
                                            t_off.data_ptr(), t_cap.data_ptr(), result.data_ptr(), 1, 2, prefs, flags,
                                            ws.data_ptr(), ws_bytes)
    link = zl.lz4f.BATCH_LINK_BLOCKS
    assert call(_prefs(zl.Prefs, block_mode=1), link, big, big.numel()) == -104
    assert call(_prefs(zl.Prefs, compression_level=9), link, big, big.numel()) == -8
    old = L.zlz4f_batch_compress_frame_workspace(1, 2, None)
    assert old < big.numel() and call(None, link, big, old) == -5       # a workspace sized by the old function
    torch.cuda.synchronize()
    assert result.cpu().tolist() == [-999] and (d_dst.cpu().numpy() == FILL).all()   # nothing was launched
    assert call(None, link, big, big.numel()) == 0
    torch.cuda.synchronize()
    r = int(result.cpu()[0])
    assert d_dst.cpu().numpy()[offs[0]:offs[0] + r].tobytes() == lf.compress_frame_linked(items[0])


# ------------------------------------------------------------------ 3. many short blocks: the window slides
def test_foreign_frame_of_short_blocks_slides_the_window(zl, gpu, tmp_path):
    encode = dictgen.encoder(tmp_path)
    text = bytes(dg.text_bytes(20000, 17)) * 5                         # 100 000 bytes, every block matches far back
    blocks, dict_hits = [], 0
    for k in range(100):
        pos = k * 1000
        stream, st = encode(text[max(0, pos - 65536):pos], text[pos:pos + 1000])
        blocks.append((stream, False))
        dict_hits += st[0] > 0
    assert dict_hits > 90                                              # the blocks do reach into their history
    frames = [lg.build_frame(blocks), lg.build_frame(blocks, True, text)]
    res, sizes = _check_against_model(zl, gpu, frames, [len(text)] * 2)
    assert res == [len(text)] * 2
    assert _decompress(zl, gpu, frames, [len(text)] * 2, 0)[0] == [-116, -116]


# ------------------------------------------------------------------ 4. / 5. one mixed batch, decode and size query
def test_mixed_batch_with_the_flag_equals_the_model(zl, gpu, oracle, fx, own):
    text = lg.recipe_input(lg.RECIPES[0])
    frames, caps = [], []
    for kw in (dict(), dict(block_mode=1), dict(block_mode=1, block_checksum=1, content_checksum=1),
               dict(block_checksum=1, content_checksum=1)):
        for n in (0, 13, 65536, 150000):                               # this library's frames: independent blocks
            frames.append(oracle.compress_frame(text[:n], _prefs(oracle.Prefs, **kw)))
            caps.append(n)
    frames.append(oracle.compress_frame(text[:150000], _prefs(oracle.Prefs)))   # declared linked, one byte short
    caps.append(149999)
    frames.append(fx[1]["frame"])
    caps.append(len(fx[1]["input"]))
    frames += own[1][4][3:6]                                           # linked frames with checksums and content size
    caps += [len(b) for b in own[1][2][3:6]]
    crafted = lg.crafted_cases()
    for name, frame, cap, want, want_bytes in crafted:
        frames.append(frame)
        caps.append(cap)
    frames.append(b"\x04\x22\x4d\x18\x40\x40")                         # header incomplete
    caps.append(10)
    res, sizes = _check_against_model(zl, gpu, frames, caps)
    n0 = len(frames) - 1 - len(crafted)
    assert res[n0:n0 + len(crafted)] == [c[3] for c in crafted]        # (the results stated with the cases)
    # frames declared independent: bytes and status identical to the call without the flag
    plain, plain_outs = _decompress(zl, gpu, frames, caps, 0)
    flagged, flagged_outs = _decompress(zl, gpu, frames, caps, zl.lz4f.DECODE_LINKED)
    for k, f in enumerate(frames):
        if len(f) > 4 and f[4] & 0x20:
            assert plain[k] == flagged[k] and plain_outs[k] == flagged_outs[k], k
    # default-prefs frames of this library declare "linked" and hold independent blocks: the same bytes either way
    assert plain[:4] == flagged[:4] and plain_outs[:4] == flagged_outs[:4]


def test_frame_beyond_max_blocks_is_invalid_state_and_the_rest_stands(zl, gpu, fx, own):
    frames = [fx[0]["frame"], own[0][4][5], fx[1]["frame"], own[0][4][4]]            # 3, 4, 3, 2 blocks
    caps = [160000, 200000, 160000, 65537]
    assert [zl._chain_blocks(f) for f in frames] == [3, 4, 3, 2]
    L = zl.lz4f.DECODE_LINKED
    res, outs = _decompress(zl, gpu, frames, caps, L, max_blocks=9)
    assert res == [160000, 200000, -5, -5]
    assert outs[0] == fx[0]["input"] and outs[1] == own[0][2][5]
    assert _sizes(zl, gpu, frames, L, max_blocks=9) == [160000, 200000, -5, -5]
    res, outs = _decompress(zl, gpu, frames, caps, L, max_blocks=12)
    assert res == caps and outs[3] == own[0][2][4]


# ------------------------------------------------------------------ 6. graph capture
def test_linked_batches_in_a_captured_graph(zl, gpu):
    import torch
    n = 24
    text = lg.recipe_input(lg.RECIPES[2])
    items = [text[k * 3000: k * 3000 + 2000 + 500 * (k % 5) + (140000 if k % 8 == 0 else 0)] for k in range(n)]
    items2 = [bytes(dg.mixed_bytes(len(b), 700 + k)) for k, b in enumerate(items)]
    kw = dict(block_checksum=1, content_checksum=1)
    p = _prefs(zl.Prefs, **kw)
    link, dl = zl.lz4f.BATCH_LINK_BLOCKS, zl.lz4f.DECODE_LINKED
    caps = [zl.lz4f.compressFrameBound(len(b), p) for b in items]
    max_blocks = sum((len(b) + 65535) // 65536 for b in items)
    d_src, s_off, s_len = _stage(items, gpu)
    d_frm, f_offs, t_foff, t_fcap = _slots(caps, gpu)
    d_out, o_offs, t_ooff, t_ocap = _slots([len(b) for b in items], gpu)
    cres = torch.zeros(n, dtype=torch.int64, device=gpu)
    dres = torch.zeros(n, dtype=torch.int64, device=gpu)
    qres = torch.zeros(n, dtype=torch.int64, device=gpu)
    cws = torch.empty(zl.lz4f.compressFrameBatchWorkspace(n, max_blocks, p, link), dtype=torch.uint8, device=gpu)
    dws = torch.empty(zl.lz4f.decompressFrameBatchWorkspace(n, max_blocks, dl), dtype=torch.uint8, device=gpu)
    qws = torch.empty(zl.lz4f.frameDecompressedSizeBatchWorkspace(n, max_blocks, dl), dtype=torch.uint8, device=gpu)

    def run():
        zl.lz4f.compressFrameBatch(d_src, s_off, s_len, d_frm, t_foff, t_fcap, cres, p, link, max_blocks, cws)
        zl.lz4f.decompressFrameBatch(d_frm, t_foff, cres, d_out, t_ooff, t_ocap, dres, max_blocks, dws, flags=dl)
        zl.lz4f.frameDecompressedSizeBatch(d_frm, t_foff, cres, qres, max_blocks, qws, flags=dl)

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
        for t in (cres, dres, qres):
            t.fill_(-999)
        g.replay()
        torch.cuda.synchronize()
        c, d, q = cres.cpu().tolist(), dres.cpu().tolist(), qres.cpu().tolist()
        frm = d_frm.cpu().numpy().tobytes()
        out = d_out.cpu().numpy().tobytes()
        for k, b in enumerate(batch):
            want = lf.compress_frame_linked(b, kw)
            assert c[k] == len(want) and frm[f_offs[k]:f_offs[k] + c[k]] == want, k
            assert d[k] == len(b) == q[k] and out[o_offs[k]:o_offs[k] + d[k]] == b, k
