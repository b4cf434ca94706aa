"""lz4f dictionary frames at the HC levels 3..9 on the HIP path:
zlz4f_batch_compress_frame_using_dict_ex and zlz4f_compress_frame_using_dict_ex, byte for byte and status for status against
the CPU model tools/pyref/zig_lz4_dict_frame_hc.py over the C restatement of the block compressor (tests/hc_dict_ref.c; the
two are held against each other and against liblz4's decoder in test_dict_frame_hc_cpu.py).  Every destination slot is
fenced by guard bytes, every source and dictionary lies at an odd offset, every batch starts from a sentinel result.
Run on the GPU box: pytest -m gpu."""
import os
import sys

import numpy as np
import pytest

import datagen as dg
import dictframegen as dfg
import dictframehcgen as hcg
import hcdictcgen as hg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "pyref"))
import zig_lz4_dict_frame as df  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5
SENTINEL = -999
DICT_LENS = (0, 4, 5, 1000, 61440, 65536, 100000)                      # dictionary 7 ends in a run (fixture `dicts`)
# (frame length, dictionary number): every length of the contract, every dictionary length, long frames with and without
PAIRS = ((0, 3), (1, 1), (12, 2), (13, 0), (1000, 3), (1000, 6), (4096, 4), (4096, 5), (65536, 5), (65537, 6),
         (150000, 6), (150000, 0), (65537, 3), (1000, 1), (13, 5), (1000, 0), (4096, 0), (4096, 2))
SUBSET = (0, 3, 4, 6, 7, 9, 11)                                        # level 6
RANDOM, RUN = len(PAIRS), len(PAIRS) + 1                               # the two special frames behind PAIRS


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
        pos += len(b) + 2 + (len(b) & 1)                               # (every offset odd)
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
        pos += c + GUARD + (c & 1)
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
    for o, c, r in zip(offs, caps, res):                               # a frame without a result wrote nothing
        if r == -5:
            assert raw[o:o + c] == bytes([FILL]) * c, "a frame with InvalidState wrote into its slot"
    return res, [raw[o:o + r] if r >= 0 else None for o, r in zip(offs, res)]


def _compress(zl, gpu, items, prefs, flags, dicts, idx, max_src_len=0, max_dict_len=65536, max_blocks=None, caps=None,
              call=None):
    import torch
    if caps is None:
        caps = [zl.lz4f.compressFrameBound(len(b), prefs) for b in items]
    d_src, s_off, s_len = _stage(items, gpu)
    d_dict, k_off, k_len, t_idx = _stage_dicts(dicts, idx, gpu)
    d_dst, offs, t_off, t_cap = _slots(caps, gpu)
    result = torch.full((len(items),), SENTINEL, dtype=torch.int64, device=gpu)
    (call or zl.lz4f.compressFrameUsingDictBatchEx)(d_src, s_off, s_len, d_dst, t_off, t_cap, result, d_dict, k_off, k_len,
                                                    t_idx, prefs, flags, max_blocks, max_src_len, max_dict_len)
    return _collect(d_dst, offs, caps, result)


def _compress_plain(zl, gpu, items, prefs, flags):
    """zlz4f_batch_compress_frame(_ex): the frames without a dictionary"""
    import torch
    caps = [zl.lz4f.compressFrameBound(len(b), prefs) for b in items]
    d_src, s_off, s_len = _stage(items, gpu)
    d_dst, offs, t_off, t_cap = _slots(caps, gpu)
    result = torch.full((len(items),), SENTINEL, dtype=torch.int64, device=gpu)
    zl.lz4f.compressFrameBatch(d_src, s_off, s_len, d_dst, t_off, t_cap, result, prefs, flags)
    return _collect(d_dst, offs, caps, result)


def _decompress(zl, gpu, frames, caps, dicts, idx):
    import torch
    max_blocks = sum(zl._chain_blocks(f) for f in frames)
    d_src, s_off, s_len = _stage(frames, gpu)
    d_dict, k_off, k_len, t_idx = _stage_dicts(dicts, idx, gpu)
    d_dst, offs, t_off, t_cap = _slots(caps, gpu)
    result = torch.full((len(frames),), SENTINEL, dtype=torch.int64, device=gpu)
    zl.lz4f.decompressFrameUsingDictBatch(d_src, s_off, s_len, d_dst, t_off, t_cap, result, d_dict, k_off, k_len, t_idx,
                                          max_blocks)
    size = torch.full((len(frames),), SENTINEL, dtype=torch.int64, device=gpu)
    zl.lz4f.frameDecompressedSizeUsingDictBatch(d_src, s_off, s_len, size, k_len, t_idx, max_blocks)
    return _collect(d_dst, offs, caps, result) + (size.cpu().tolist(),)


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    """compress_frame_using_dict_hc over the C restatement, memoised: a frame is modelled once for all tests"""
    return hcg.model(hg.ref(tmp_path_factory.mktemp("hc_dict_ref")))


@pytest.fixture(scope="module")
def dicts():
    big = dfg.recipe_dict(dfg.RECIPES[0])
    return [big[len(big) - n:] for n in DICT_LENS] + [big[:1700] + b"z" * 300]


def _item(d, n, seed):
    """n bytes that match the dictionary's tail (text of their own for a dictionary of a few bytes)."""
    base = d[-60000:] if len(d) >= 1000 else bytes(dg.text_bytes(60000, seed))
    b = bytearray((base * (n // len(base) + 1))[:n])
    for i in range(0, n, 1000 if n > 1000 else 100):
        b[i] ^= 0x55
    return bytes(b)


@pytest.fixture(scope="module")
def batch(dicts):
    """-> (items, idx): PAIRS, then a frame of random bytes (its block is stored) and a frame that begins with 300 bytes
    of the last byte of its dictionary, which ends in 300 of them (level 9's pattern step walks down into T)"""
    items = [_item(dicts[k], n, 40 + j) for j, (n, k) in enumerate(PAIRS)]
    idx = [k for _, k in PAIRS]
    items += [bytes(dg.random_bytes(5000, 8)), b"z" * 300 + b"\xb0" + b"z" * 350 + bytes(dg.text_bytes(3000, 9))]
    idx += [3, 7]
    return items, idx


@pytest.fixture(scope="module")
def own(zl, gpu, dicts, batch, model):
    """The batch compressed once per preference set: (level, kw, items, idx, results, frames, model frames)."""
    all_items, all_idx = batch
    out = []
    cfgs = [(lv, dict(block_mode=m), False, None) for lv in (3, 9) for m in (0, 1)]
    cfgs += [(6, dict(block_mode=m), False, SUBSET + (RANDOM, RUN)) for m in (0, 1)]
    cfgs += [(9, dict(block_mode=0, block_checksum=1, content_checksum=1, dict_id=9), True, None),
             (3, dict(block_mode=1, block_checksum=1, content_checksum=1), True, SUBSET + (10, RANDOM))]
    for level, kw, cs, sel in cfgs:
        sel = range(len(all_items)) if sel is None else sel
        items, idx = [all_items[j] for j in sel], [all_idx[j] for j in sel]
        flags = zl.lz4f.BATCH_CONTENT_SIZE if cs else 0
        res, frames = _compress(zl, gpu, items, _prefs(zl.Prefs, compression_level=level, **kw), flags, dicts, idx)
        want = [model(b, dicts[k], level, dict(kw, content_size=len(b) if cs else 0)) for b, k in zip(items, idx)]
        out.append((level, kw, items, idx, res, frames, want))
    return out


# ------------------------------------------------------------------ 1. against the model
def test_compress_gives_the_models_bytes(own):
    for level, kw, items, idx, res, frames, want in own:
        assert res == [len(w) for w in want], (level, kw, res)
        assert frames == want, (level, kw)


def test_special_frames_are_what_they_claim(own, dicts, batch):
    import zig_lz4_linked_frame_hc as lh
    items, idx = batch
    level, kw, _, _, res, frames, want = own[1]                        # level 3, independent
    assert lh.blocks_of(frames[RANDOM]) == [(items[RANDOM], True)]
    for cfg in (own[2], own[3]):                                       # level 9: the pattern step's match starts in T
        payload, stored = lh.blocks_of(cfg[5][RUN])[0]
        assert not stored
        seqs = hg.sequences(payload)
        assert seqs[0] == (0, 0, 300, 1)                               # the record's first byte copies from the dictionary
        assert seqs[1] == (301, 1, 350, 351)                           # hcdictcgen.traced(): the pattern step, starts in T
    sizes = {cfg[0]: sum(r for r in cfg[4]) for cfg in own[:4] if cfg[1]["block_mode"] == 1}
    assert sizes[9] < sizes[3]


def test_own_frames_round_trip_on_the_device(zl, gpu, own, dicts):
    z = dfg.liblz4fd()
    for level, kw, items, idx, res, frames, want in own:
        lens = [len(b) for b in items]
        got, outs, sizes = _decompress(zl, gpu, frames, lens, dicts, idx)
        assert got == lens and outs == items and sizes == lens, (level, kw)
        if z is not None:
            for f, b, k in zip(frames, items, idx):
                assert z.decompress(f, len(b), dicts[k]) == b, (level, kw, len(b), k)


# ------------------------------------------------------------------ 2. the link width does not show
def test_link_width_does_not_change_the_bytes(zl, gpu, dicts, batch, model):
    all_items, all_idx = batch
    sel = [j for j, (b, k) in enumerate(zip(all_items, all_idx)) if len(b) <= 4096 and len(dicts[k]) <= 61440]
    assert {len(all_items[j]) for j in sel} >= {0, 1, 12, 13, 1000, 4096} and {all_idx[j] for j in sel} >= {0, 1, 2, 3, 4}
    items, idx = [all_items[j] for j in sel], [all_idx[j] for j in sel]
    for level in (3, 9):
        for mode in (0, 1):
            p = _prefs(zl.Prefs, compression_level=level, block_mode=mode)
            want = [model(b, dicts[k], level, dict(block_mode=mode)) for b, k in zip(items, idx)]
            lds = _compress(zl, gpu, items, p, 0, dicts, idx, max_src_len=4096, max_dict_len=61440)      # 65 536 in all
            hbm = _compress(zl, gpu, items, p, 0, dicts, idx)
            mid = _compress(zl, gpu, items, p, 0, dicts, idx, max_src_len=4097, max_dict_len=61440)      # one byte over
            assert lds == hbm == mid == ([len(w) for w in want], want), (level, mode)


# ------------------------------------------------------------------ 3. the calls this one must equal
def test_empty_dictionary_gives_the_existing_calls(zl, gpu, own, batch):
    items = [b for b, k in zip(*batch) if k == 0] + [batch[0][10]]     # and the three-block frame of dictionary 6
    for level in (3, 9):
        for mode in (0, 1):
            p = _prefs(zl.Prefs, compression_level=level, block_mode=mode)
            got = _compress(zl, gpu, items, p, 0, [b""], None)
            old = _compress_plain(zl, gpu, items, p, zl.lz4f.BATCH_LINK_BLOCKS if mode == 0 else 0)
            assert got == old and all(r > 0 for r in got[0]), (level, mode)
    for cfg in own[:4]:                                                # the frames of dictionary 0 in the mixed batch
        level, kw, all_items, idx, res, frames, want = cfg
        sel = [j for j, k in enumerate(idx) if k == 0]
        p = _prefs(zl.Prefs, compression_level=level, **kw)
        old = _compress_plain(zl, gpu, [all_items[j] for j in sel], p, zl.lz4f.BATCH_LINK_BLOCKS if kw["block_mode"] == 0 else 0)
        assert old == ([res[j] for j in sel], [frames[j] for j in sel]), (level, kw)


def test_fast_level_is_the_plain_call(zl, gpu, dicts, batch):
    items, idx = batch
    for mode in (0, 1):
        for level in (0, -3):
            p = _prefs(zl.Prefs, compression_level=level, block_mode=mode, block_checksum=mode)
            ex = _compress(zl, gpu, items, p, 0, dicts, idx)
            plain = _compress(zl, gpu, items, p, 0, dicts, idx, call=zl.lz4f.compressFrameUsingDictBatch)
            assert ex == plain and all(r > 0 for r in ex[0])
        want = [df.compress_frame_using_dict(b, dicts[k], dict(block_mode=mode, block_checksum=mode))
                for b, k in zip(items[:8], idx[:8])]
        assert ex[1][:8] == want
        args = (len(items), 40, _prefs(zl.Prefs, block_mode=mode), 0, len(dicts), 0, 65536)
        assert zl.lz4f.compressFrameUsingDictBatchWorkspaceEx(*args) == zl.lz4f.compressFrameUsingDictBatchWorkspace(*args)


# ------------------------------------------------------------------ 4. preconditions and refusals
def test_preconditions_fail_one_frame_only(zl, gpu, dicts, model):
    three = [dicts[3], dicts[6], dicts[1]]                             # ndicts = 3, mixed index
    idx = [0, 1, 2, 1, 0, 3]
    items = [_item(three[k % 3], n, 60 + j) for j, (n, k) in enumerate(zip((1000, 70000, 500, 2000, 1500, 800), idx))]
    for level, mode in ((9, 0), (3, 1), (9, 1)):
        kw = dict(block_mode=mode)
        p = _prefs(zl.Prefs, compression_level=level, **kw)
        want = [model(b, three[k], level, kw) if k < 3 else -5 for b, k in zip(items, idx)]
        # (a) an index out of range (d_dict_idx[f] = ndicts)
        res, frames = _compress(zl, gpu, items, p, 0, three, idx)
        assert res == [len(w) if w != -5 else -5 for w in want] and frames[:5] == want[:5], (level, mode)
        # (b) max_src_len exceeded by frame 1 (70 000 > 2 000): with the bound every frame is one block
        res, frames = _compress(zl, gpu, items, p, 0, three, idx, max_src_len=2000)
        assert res[1] == -5 and res[5] == -5 and [frames[j] for j in (0, 2, 3, 4)] == [want[j] for j in (0, 2, 3, 4)]
        # (c) max_dict_len exceeded by dictionary 1 (T = 65 536 > 1 000)
        res, frames = _compress(zl, gpu, items, p, 0, three, idx, max_dict_len=1000)
        assert [res[j] for j in (1, 3, 5)] == [-5] * 3 and [frames[j] for j in (0, 2, 4)] == [want[j] for j in (0, 2, 4)]
        # (d) a destination one byte below the bound: that frame alone
        caps = [zl.lz4f.compressFrameBound(len(b), p) for b in items]
        caps[3] -= 1
        res, frames = _compress(zl, gpu, items, p, 0, three, idx, caps=caps)
        assert res[3] == -111 and [frames[j] for j in (0, 1, 2, 4)] == [want[j] for j in (0, 1, 2, 4)]
        # (e) a block table one entry short: the last frame with a block has no room, the earlier ones are unaffected
        blocks = sum((len(b) + 65535) // 65536 for b in items[:5])
        res, frames = _compress(zl, gpu, items[:5], p, 0, three, idx[:5], max_blocks=blocks - 1)
        assert res[4] == -5 and frames[:4] == want[:4], (level, mode, res)


def test_refusals_launch_nothing(zl, gpu, dicts):
    import torch
    items = [_item(dicts[3], 1000, 1), _item(dicts[3], 70000, 2)]
    p9 = _prefs(zl.Prefs, compression_level=9)
    caps = [zl.lz4f.compressFrameBound(len(b), p9) for b in items]
    d_src, s_off, s_len = _stage(items, gpu)
    d_dict, k_off, k_len, _ = _stage_dicts(dicts, None, gpu)
    d_dst, offs, t_off, t_cap = _slots(caps, gpu)
    result = torch.full((2,), SENTINEL, dtype=torch.int64, device=gpu)
    need = zl.lz4f.compressFrameUsingDictBatchWorkspaceEx(2, 3, p9, 0, len(dicts), 0, 65536)
    assert need > zl.lz4f.compressFrameUsingDictBatchWorkspace(2, 3, p9, 0, len(dicts), 0, 65536)
    ws = torch.empty(need + 16, dtype=torch.uint8, device=gpu)

    def call(prefs, flags, w):
        with pytest.raises(zl.Lz4Error) as e:
            zl.lz4f.compressFrameUsingDictBatchEx(d_src, s_off, s_len, d_dst, t_off, t_cap, result, d_dict, k_off, k_len, None,
                                                  prefs, flags, 3, 0, 65536, w)
        return e.value.code

    for level in (2, 10, 11, 12):
        assert call(_prefs(zl.Prefs, compression_level=level), 0, ws) == -8
        assert call(_prefs(zl.Prefs, compression_level=level, block_mode=1), 0, ws) == -8
    assert call(p9, 2, ws) == -104                                     # parameter errors come first
    assert call(_prefs(zl.Prefs, compression_level=10), 2, ws) == -104
    assert call(p9, zl.lz4f.BATCH_LINK_BLOCKS, ws) == -104
    assert call(_prefs(zl.Prefs, compression_level=9, content_size=5), zl.lz4f.BATCH_CONTENT_SIZE, ws) == -104
    assert call(p9, 0, ws[:need - 1]) == -5
    assert call(p9, 0, ws[1:need + 1]) == -5
    torch.cuda.synchronize()
    assert result.cpu().tolist() == [SENTINEL, SENTINEL]
    assert (d_dst.cpu().numpy() == FILL).all()
    # and the same arguments with the workspace as asked for are served
    zl.lz4f.compressFrameUsingDictBatchEx(d_src, s_off, s_len, d_dst, t_off, t_cap, result, d_dict, k_off, k_len, None, p9, 0,
                                          3, 0, 65536, ws[:need])
    res, frames = _collect(d_dst, offs, caps, result)
    assert all(r > 0 for r in res)


# ------------------------------------------------------------------ 5. the host call and the list helper
def test_single_frame_host_call(zl, dicts, batch, model):
    items, idx = batch
    for j in (4, 10):                                                  # 1000 bytes, 150 000 bytes
        for level in (3, 9):
            for mode in (0, 1):
                p = _prefs(zl.Prefs, compression_level=level, block_mode=mode)
                want = model(items[j], dicts[idx[j]], level, dict(block_mode=mode))
                assert zl.lz4f.compressFrameUsingDictEx(items[j], dicts[idx[j]], p) == want, (j, level, mode)
    assert zl.lz4f.decompressFrameUsingDict(want, len(items[10]), dicts[idx[10]]) == items[10]
    p = _prefs(zl.Prefs, block_mode=1)
    assert zl.lz4f.compressFrameUsingDictEx(items[4], dicts[3], p) == zl.lz4f.compressFrameUsingDict(items[4], dicts[3], p)
    with pytest.raises(zl.Lz4Error) as e:
        zl.lz4f.compressFrameUsingDictEx(items[4], dicts[3], _prefs(zl.Prefs, compression_level=10))
    assert e.value.code == -8
    p9 = _prefs(zl.Prefs, compression_level=9)
    assert zl.lib().zlz4f_compress_frame_using_dict_ex(None, 0, None, 0, p9, None, 5) == -5     # dict NULL, dict_len > 0


def test_list_helper_takes_a_level(zl, dicts, batch, model):
    items, idx = batch
    sel = (4, 5, 9, 13, RUN)
    sub, sub_idx = [items[j] for j in sel], [idx[j] for j in sel]
    for mode in (0, 1):
        p = _prefs(zl.Prefs, compression_level=9, block_mode=mode)
        want = [model(b, dicts[k], 9, dict(block_mode=mode)) for b, k in zip(sub, sub_idx)]
        assert zl.lz4f.compressFramesUsingDict(sub, dicts, sub_idx, p) == want
        assert zl.lz4f.decompressFramesUsingDict(want, dicts, sub_idx) == sub
    fast = zl.lz4f.compressFramesUsingDict(sub, dicts, sub_idx, _prefs(zl.Prefs, block_mode=1))
    assert fast == [df.compress_frame_using_dict(b, dicts[k], dict(block_mode=1)) for b, k in zip(sub, sub_idx)]
