"""Batch frame calls on the HIP path vs the oracle, frame by frame: zlz4f_batch_compress_frame must give every frame the
bytes and status of oracle.compress_frame, zlz4f_batch_decompress_frame those of oracle.decompress_frame (which
restate src/lz4f.zig:354-446 and :541-638).  Every destination slot is fenced by guard bytes that must survive the call.
Run on the GPU box: pytest -m gpu."""
import numpy as np
import pytest

import cases
import datagen as dg

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5


def _prefs(P, **kw):
    p = P()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _pref_matrix():          # test_gpu_frame.py's matrix
    out = [dict()]
    for bsid in (0, 4, 5, 6, 7):
        out.append(dict(block_size_id=bsid, block_mode=1))
    out.append(dict(block_checksum=1))
    out.append(dict(content_checksum=1))
    out.append(dict(block_checksum=1, content_checksum=1, block_size_id=4, content_size=12345, dict_id=7))
    out.append(dict(compression_level=9))
    out.append(dict(compression_level=3, block_checksum=1))
    out.append(dict(compression_level=1, content_checksum=1))      # level 1 -> compressHC clamps to 9
    out.append(dict(compression_level=-5))                          # negative = fast
    out.append(dict(compression_level=2))                           # lz4mid
    out.append(dict(compression_level=12, block_checksum=1))        # lz4opt
    out.append(dict(compression_level=10))                          # lz4opt, targetLength 64
    return out


def _block_size(kw):
    return {5: 256 << 10, 6: 1 << 20, 7: 4 << 20}.get(kw.get("block_size_id", 0), 64 << 10)


def _mixed_items(seed=0):
    items = []
    for k, n in enumerate((0, 1, 12, 13, 4096, 65536, 65537, 300000)):
        items.append(bytes(dg.random_bytes(n, seed + 2 * k)))     # random: stored blocks
        items.append(bytes(dg.text_bytes(n, seed + 2 * k + 1)) if n else b"")
    return items


def _stage(items, gpu, odd=True):
    """Sources back to back at odd offsets (1 + a few bytes of gap)."""
    import torch
    offs, pos = [], 1
    for b in items:
        offs.append(pos)
        pos += len(b) + (3 if odd else 0)
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


def _compress(zl, gpu, items, prefs, flags=0, caps=None, max_blocks=None):
    import torch
    if caps is None:
        caps = [zl.lz4f.compressFrameBound(len(b), prefs) for b in items]
    d_src, s_off, s_len = _stage(items, gpu)
    d_dst, offs, t_off, t_cap = _slots(caps, gpu)
    result = torch.full((len(items),), -999, dtype=torch.int64, device=gpu)
    zl.lz4f.compressFrameBatch(d_src, s_off, s_len, d_dst, t_off, t_cap, result, prefs, flags, max_blocks)
    return _collect(d_dst, offs, caps, result)


def _decompress(zl, gpu, frames, caps, max_blocks=None):
    import torch
    if max_blocks is None:
        max_blocks = sum(zl._chain_blocks(f) for f in frames)
    d_src, s_off, s_len = _stage(frames, gpu)
    d_dst, offs, t_off, t_cap = _slots(caps, gpu)
    result = torch.full((len(frames),), -999, dtype=torch.int64, device=gpu)
    zl.lz4f.decompressFrameBatch(d_src, s_off, s_len, d_dst, t_off, t_cap, result, max_blocks)
    return _collect(d_dst, offs, caps, result)


def _check_decompress(zl, oracle, gpu, frames, caps, max_blocks=None):
    res, outs = _decompress(zl, gpu, frames, caps, max_blocks)
    bad = []
    for k, (f, cap) in enumerate(zip(frames, caps)):
        want = oracle.decompress_frame(f, cap)
        if isinstance(want, int):
            if res[k] != want:
                bad.append(("status", k, len(f), cap, res[k], want))
        elif res[k] != len(want) or outs[k] != want:
            bad.append(("bytes", k, len(f), cap, res[k], len(want)))
    assert not bad, (len(bad), bad[:6])
    return res


# ------------------------------------------------------------------ 1. compress parity over the preference matrix
@pytest.mark.parametrize("content_size_flag", [False, True])
def test_compress_batch_matches_compress_frame(zl, oracle, gpu, content_size_flag):
    items = _mixed_items()
    bad = []
    for kw in _pref_matrix():
        batch = [b for b in items if not (len(b) >= 300000 and kw.get("compression_level", 0) >= 10)]
        kw_dev = dict(kw)
        if content_size_flag:
            kw_dev["content_size"] = 0
        res, outs = _compress(zl, gpu, batch, _prefs(zl.Prefs, **kw_dev), zl.lz4f.BATCH_CONTENT_SIZE if content_size_flag else 0)
        for k, b in enumerate(batch):
            kw_ref = dict(kw, content_size=len(b)) if content_size_flag else kw
            want = oracle.compress_frame(b, _prefs(oracle.Prefs, **kw_ref))
            if res[k] != len(want) or outs[k] != want:
                bad.append((kw, len(b), res[k], len(want)))
    assert not bad, bad[:6]


def test_compress_batch_content_size_flag_needs_zero_content_size(zl, gpu):
    with pytest.raises(zl.Lz4Error) as e:
        _compress(zl, gpu, [b"abc"], _prefs(zl.Prefs, content_size=3), zl.lz4f.BATCH_CONTENT_SIZE)
    assert e.value.name == "ParameterInvalid"


# ------------------------------------------------------------------ 2. capacity and isolation
def test_compress_batch_short_destination_is_isolated(zl, oracle, gpu):
    items = [bytes(dg.text_bytes(n, 40 + n % 7)) for n in (5000, 70000, 12, 131072, 999, 65536)]
    for kw in (dict(), dict(block_checksum=1, content_checksum=1), dict(compression_level=9)):
        p = _prefs(zl.Prefs, **kw)
        caps = [zl.lz4f.compressFrameBound(len(b), p) for b in items]
        for victim in (0, 1, 3):
            c = list(caps)
            c[victim] -= 1
            res, outs = _compress(zl, gpu, items, p, caps=c)
            for k, b in enumerate(items):
                if k == victim:
                    assert res[k] == -111, (kw, victim, res)
                else:
                    want = oracle.compress_frame(b, _prefs(oracle.Prefs, **kw))
                    assert outs[k] == want, (kw, victim, k)


def test_compress_batch_max_blocks_one_short(zl, oracle, gpu):
    items = [bytes(dg.text_bytes(n, 60 + k)) for k, n in enumerate((70000, 100, 0, 200000, 65536, 0, 3000, 140000))]
    p = _prefs(zl.Prefs)
    nbs = [(len(b) + 65535) // 65536 for b in items]
    total = sum(nbs)
    for max_blocks in (total, total - 1, nbs[0] + nbs[1] + 1, 0):
        res, outs = _compress(zl, gpu, items, p, max_blocks=max_blocks)
        base = 0
        for k, b in enumerate(items):
            if nbs[k] and base + nbs[k] > max_blocks:
                assert res[k] == -5, (max_blocks, k, res)                  # ZLZ4_ERR_INVALID_STATE
            else:
                assert outs[k] == oracle.compress_frame(b), (max_blocks, k)
            base += nbs[k]


def test_decompress_batch_max_blocks_one_short(zl, oracle, gpu):
    p = oracle.Prefs()
    p.block_checksum = 1
    items = [bytes(dg.text_bytes(n, 80 + k)) for k, n in enumerate((70000, 100, 0, 200000, 3000, 140000))]
    frames = [oracle.compress_frame(b, p) for b in items]
    nbs = [zl._chain_blocks(f) for f in frames]
    assert nbs == [(len(b) + 65535) // 65536 for b in items]
    total = sum(nbs)
    for max_blocks in (total - 1, nbs[0] + 1):
        res, outs = _decompress(zl, gpu, frames, [len(b) for b in items], max_blocks)
        base = 0
        for k, b in enumerate(items):
            if nbs[k] and base + nbs[k] > max_blocks:
                assert res[k] == -5, (max_blocks, k, res)
            else:
                assert res[k] == len(b) and outs[k] == b, (max_blocks, k)
            base += nbs[k]


# ------------------------------------------------------------------ 3. decompress parity, every status
def _header(oracle, flg, bd, content_size=None):
    h = bytearray(b"\x04\x22\x4d\x18") + bytes([flg, bd])
    if content_size is not None:
        h += content_size.to_bytes(8, "little")
    h.append((oracle.xxh32(bytes(h[4:])) >> 8) & 0xFF)
    return bytes(h)


def _hand_frames(oracle):
    """Frames compressFrame never writes: short, empty and stored blocks (they take the exact path)."""
    t = bytes(dg.text_bytes(200000, 91))
    r = bytes(dg.random_bytes(5000, 92))
    out = []
    for bc in (0, 1):
        for cc in (0, 1):
            flg = 0x60 | (0x10 if bc else 0) | (0x04 if cc else 0)
            body, content = b"", b""

            def blk(data, stored=False):
                payload = data if stored else oracle.compress_default(data)
                hdr = (len(payload) | (0x80000000 if stored else 0)).to_bytes(4, "little")
                return hdr + payload + (oracle.xxh32(payload).to_bytes(4, "little") if bc else b"")
            for piece, stored in ((t[:1000], False), (b"", True), (r[:3000], True), (t[1000:66536], False),
                                  (t[70000:70013], False), (r, True), (t[100000:165536], True), (t[:17], False)):
                body += blk(piece, stored)
                content += piece
            tail = b"\0\0\0\0" + (oracle.xxh32(content).to_bytes(4, "little") if cc else b"")
            out.append((content, _header(oracle, flg, 0x40) + body + tail))
    # a frame whose blocks are all full-size but not the last one short: a stored block in the middle of the speculation
    p = oracle.Prefs()
    out.append((t, oracle.compress_frame(t, p)))
    return out


def _variants(f, rng):
    vs = [f[:k] for k in (0, 3, 6, 7, 8, 10, len(f) // 2, len(f) - 1, len(f) - 4, len(f) - 5) if 0 <= k <= len(f)]
    for _ in range(6):
        m = bytearray(f)
        if m:
            m[int(rng.integers(0, len(m)))] ^= 1 << int(rng.integers(0, 8))
        vs.append(bytes(m))
    vs.append(f + b"trailing garbage")
    return vs


def test_decompress_batch_matches_decompress_frame(zl, oracle, gpu):
    rng = np.random.default_rng(99)
    base = []
    ins = [b for _, b in cases.reference_test_inputs()][:10] + [bytes(dg.text_bytes(65537, 7)), bytes(dg.random_bytes(70000, 4)),
                                                               bytes(dg.mixed_bytes(200001, 5))]
    for kw in _pref_matrix():
        for b in ins:
            if len(b) > 100000 and kw.get("compression_level", 0) >= 10:
                continue
            base.append((b, oracle.compress_frame(b, _prefs(oracle.Prefs, **kw))))
    base += _hand_frames(oracle)
    frames, caps = [], []
    for k, (b, f) in enumerate(base):
        vs = _variants(f, rng) if k % 3 == 0 or k >= len(base) - 5 else [f]
        for v in vs:
            for cap in (len(b), max(0, len(b) - 1), len(b) // 2, 0):
                frames.append(v)
                caps.append(cap)
    frames.append(bytes([0x50, 0x2A, 0x4D, 0x18, 4, 0, 0, 0]) + b"skip")   # skippable frame: FrameTypeUnknown
    caps.append(100)
    assert len(frames) > 1000
    res = _check_decompress(zl, oracle, gpu, frames, caps)
    assert any(r >= 0 for r in res) and len({r for r in res if r < 0}) >= 6     # the batch really mixes outcomes


def test_decompress_batch_lz4_cli_style_frames(zl, oracle, gpu):
    """Frames with content size, dict id and every block size in one batch (what the lz4 CLI and compressFrame write)."""
    frames, caps, items = [], [], []
    for k, kw in enumerate((dict(block_size_id=4, content_size=1), dict(block_size_id=5, dict_id=9),
                            dict(block_size_id=6, block_checksum=1), dict(block_size_id=7, content_checksum=1))):
        b = bytes(dg.text_bytes(300000 + k, 70 + k))
        kw = dict(kw)
        if "content_size" in kw:
            kw["content_size"] = len(b)
        frames.append(oracle.compress_frame(b, _prefs(oracle.Prefs, **kw)))
        caps.append(len(b))
        items.append(b)
    _check_decompress(zl, oracle, gpu, frames, caps)


# ------------------------------------------------------------------ 4. many frames: the decoder's lane-copy build
@pytest.mark.parametrize("level", [0, 2, 9])
def test_round_trip_8192_text_frames(zl, oracle, gpu, level):
    text = bytes(dg.text_bytes(8192 * 600 + 8192, 123))
    items = [text[k * 600: k * 600 + 4096 + (k % 5) * 1000] for k in range(8192)]
    kw = dict(block_checksum=1, content_checksum=1, compression_level=level)
    p = _prefs(zl.Prefs, **kw)
    res, frames = _compress(zl, gpu, items, p, zl.lz4f.BATCH_CONTENT_SIZE)
    assert min(res) > 0
    for k in range(0, 8192, 257):
        assert frames[k] == oracle.compress_frame(items[k], _prefs(oracle.Prefs, content_size=len(items[k]), **kw)), k
    dres, outs = _decompress(zl, gpu, frames, [len(b) for b in items], max_blocks=8192)
    assert dres == [len(b) for b in items]
    assert outs == items


# ------------------------------------------------------------------ 5. graph capture
def test_batches_in_a_captured_graph(zl, oracle, gpu):
    import torch
    n = 300
    text = bytes(dg.text_bytes(n * 5000 + 70000, 31))
    items = [text[k * 5000: k * 5000 + 3000 + 300 * (k % 7) + (66000 if k % 50 == 0 else 0)] for k in range(n)]
    items2 = [bytes(dg.mixed_bytes(len(b), 500 + k)) for k, b in enumerate(items)]
    kw = dict(block_checksum=1, content_checksum=1)
    p = _prefs(zl.Prefs, **kw)
    caps = [zl.lz4f.compressFrameBound(len(b), p) for b in items]
    max_blocks = sum((len(b) + 65535) // 65536 for b in items)
    d_src, s_off, s_len = _stage(items, gpu)
    d_frm, f_offs, t_foff, t_fcap = _slots(caps, gpu)
    d_out, o_offs, t_ooff, t_ocap = _slots([len(b) for b in items], gpu)
    cres = torch.zeros(n, dtype=torch.int64, device=gpu)
    dres = torch.zeros(n, dtype=torch.int64, device=gpu)
    cws = torch.empty(zl.lz4f.compressFrameBatchWorkspace(n, max_blocks, p), dtype=torch.uint8, device=gpu)
    dws = torch.empty(zl.lz4f.decompressFrameBatchWorkspace(n, max_blocks), dtype=torch.uint8, device=gpu)

    def run():
        zl.lz4f.compressFrameBatch(d_src, s_off, s_len, d_frm, t_foff, t_fcap, cres, p, 0, max_blocks, cws)
        zl.lz4f.decompressFrameBatch(d_frm, t_foff, cres, d_out, t_ooff, t_ocap, dres, max_blocks, dws)

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
        cres.fill_(-999)
        dres.fill_(-999)
        g.replay()
        torch.cuda.synchronize()
        c = cres.cpu().tolist()
        d = dres.cpu().tolist()
        frm = d_frm.cpu().numpy().tobytes()
        out = d_out.cpu().numpy().tobytes()
        for k, b in enumerate(batch):
            want = oracle.compress_frame(b, _prefs(oracle.Prefs, **kw))
            assert c[k] == len(want) and frm[f_offs[k]:f_offs[k] + c[k]] == want, k
            assert d[k] == len(b) and out[o_offs[k]:o_offs[k] + d[k]] == b, k
