"""Linked-block frames at the HC levels 3..9 on the HIP path: zlz4f_batch_compress_frame_ex with ZLZ4F_BATCH_LINK_BLOCKS and
the single-frame _ex calls, byte for byte and status for status against the CPU model
tools/pyref/zig_lz4_linked_frame_hc.py composed from the C restatement of the block compressor (tests/hc_dict_ref.c; both
are held against each other, the oracle and liblz4 in test_linked_frame_hc_cpu.py), against the staged
zlz4_batch_compress_hc_using_dict, and back through zlz4f_batch_decompress_frame_ex(ZLZ4F_DECODE_LINKED) and liblz4.
Every destination slot is fenced by guard bytes.  Run on the GPU box: pytest -m gpu."""
import hashlib
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import datagen as dg
import gpu_harness as gh
import hcdictcgen as hg
import linkedgen as lg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "pyref"))
import zig_lz4_linked_frame as lf  # noqa: E402
import zig_lz4_linked_frame_hc as lh  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5
LEVELS = (3, 6, 9)
KW_SETS = ((dict(), False), (dict(block_checksum=1, content_checksum=1), True))


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


def _compress_ex(zl, gpu, items, prefs, flags, max_blocks=None, caps=None, fn="zlz4f_batch_compress_frame_ex"):
    """One call of the C entry `fn` -> (call status, results, frames, untouched): untouched[f] = frame f's slot still holds
    nothing but FILL."""
    import torch
    L = zl.lib()
    bs = zl.lz4f.BLOCK_SIZES[prefs.block_size_id]
    if caps is None:
        caps = [zl.lz4f.compressFrameBound(len(b), prefs) for b in items]
    if max_blocks is None:
        max_blocks = sum((len(b) + bs - 1) // bs for b in items)
    d_src, s_off, s_len = _stage(items, gpu)
    d_dst, offs, t_off, t_cap = _slots(caps, gpu)
    result = torch.full((len(items),), -999, dtype=torch.int64, device=gpu)
    ws = torch.empty(max(16, zl.lz4f.compressFrameBatchWorkspace(len(items), max_blocks, prefs, flags)), dtype=torch.uint8,
                     device=gpu)
    rc = getattr(L, fn)(None, d_src.data_ptr(), s_off.data_ptr(), s_len.data_ptr(), d_dst.data_ptr(), t_off.data_ptr(),
                        t_cap.data_ptr(), result.data_ptr(), len(items), max_blocks, prefs, flags, ws.data_ptr(), ws.numel())
    torch.cuda.synchronize()
    res, frames = _collect(d_dst, offs, caps, result)
    host = d_dst.cpu().numpy()
    return rc, res, frames, [bool((host[o:o + c] == FILL).all()) for o, c in zip(offs, caps)]


def _decompress(zl, gpu, frames, caps, flags):
    import torch
    max_blocks = sum(zl._chain_blocks(f) for f in frames)
    d_src, s_off, s_len = _stage(frames, gpu)
    d_dst, offs, t_off, t_cap = _slots(caps, gpu)
    result = torch.full((len(frames),), -999, dtype=torch.int64, device=gpu)
    zl.lz4f.decompressFrameBatch(d_src, s_off, s_len, d_dst, t_off, t_cap, result, max_blocks, flags=flags)
    return _collect(d_dst, offs, caps, result)


@pytest.fixture(scope="module")
def cref(tmp_path_factory):
    return hg.ref(tmp_path_factory.mktemp("hc_dict_ref"))


@pytest.fixture(scope="module")
def model(cref):
    """model(data, level, kw) -> the frame, composed from the C restatement per block"""
    def f(data, level, kw=None):
        return lh.compress_frame_linked_hc(data, level, kw, lambda b, d, lv: cref.compress(b, d, lv)[1])
    return f


@pytest.fixture(scope="module")
def hc_fixture():
    return {(e["name"], e["level"]): e for e in json.load(open(os.path.join(ROOT, "tests", "golden", "linked_frames_hc.json")))["frames"]}


def _items():
    text = lg.recipe_input(lg.RECIPES[0])              # period 40 000: every block matches the 64 KiB in front of it
    rnd = bytes(dg.random_bytes(65536, 4))
    items = [text[:n] for n in (0, 1, 12, 13, 65536, 65537, 65536 + 12, 65536 + 13)]
    items.append((text + text)[:131072 + 5000])        # block 2's tail begins inside block 0
    items.append(text)                                 # the recipe: 160 000 bytes
    items.append(rnd + rnd[1000:61000])                # block 0 random and stored, block 1 repeats it from 64 536 back
    return items


@pytest.fixture(scope="module")
def own(zl, gpu):
    """{(level, set index): (kw, content size from length, items, results, frames)}: one batch call each"""
    out = {}
    for level in LEVELS:
        for s, (kw, cs) in enumerate(KW_SETS):
            flags = zl.lz4f.BATCH_LINK_BLOCKS | (zl.lz4f.BATCH_CONTENT_SIZE if cs else 0)
            items = _items()
            rc, res, frames, _ = _compress_ex(zl, gpu, items, _prefs(zl.Prefs, compression_level=level, **kw), flags)
            assert rc == 0
            out[level, s] = (kw, cs, items, res, frames)
    return out


# ------------------------------------------------------------------ 1. the batch against the model
def test_batch_equals_the_model_and_the_fixture(own, model, hc_fixture):
    for (level, s), (kw, cs, items, res, frames) in own.items():
        for k, b in enumerate(items):
            want = model(b, level, dict(kw, content_size=len(b) if cs else 0))
            assert res[k] == len(want) and frames[k] == want, (level, kw, k, len(b), res[k], len(want))
        if s == 0:
            e = hc_fixture["text160k_bs64k", level]
            assert res[9] == e["frame_len"] and hashlib.sha256(frames[9]).hexdigest() == e["frame_sha256"]
        stored = lh.blocks_of(frames[10])
        assert stored[0][1] and not stored[1][1] and len(stored[1][0]) < 300     # one long match into the stored block


def test_frames_round_trip_and_are_really_linked(zl, gpu, oracle, own):
    z = lg.liblz4f()
    for (level, s), (kw, cs, items, res, frames) in own.items():
        caps = [len(b) for b in items]
        got, outs = _decompress(zl, gpu, frames, caps, zl.lz4f.DECODE_LINKED)
        assert got == caps and outs == items, (level, kw)
        if z is not None:
            for b, f in zip(items, frames):
                assert z.decompress(f, len(b)) == b, (level, kw, len(b))
        # without the flag every block is decoded alone (the reference's decoder): a block that matches into its history fails
        plain, _ = _decompress(zl, gpu, frames, caps, 0)
        ref = [oracle.decompress_frame(f, len(b)) for b, f in zip(items, frames)]
        assert plain == [r if isinstance(r, int) else len(r) for r in ref], (level, kw)
        assert plain[:5] == caps[:5] and plain[8:] == [-116, -116, -116], (level, kw, plain)


def test_block_0_is_compress_hc_and_one_block_frames_are_the_hc_frame(oracle, own):
    for level in LEVELS:
        kw, cs, items, res, frames = own[level, 0]
        q = _prefs(oracle.Prefs, block_mode=0, compression_level=level)
        for k in range(5):
            assert frames[k] == oracle.compress_frame(items[k], q), (level, k)
        for k in (5, 8, 9):
            assert lh.blocks_of(frames[k])[0][0] == oracle.compress_hc(items[k][:65536], level), (level, k)


def test_payloads_equal_the_staged_dictionary_call(zl, gpu, cref, own):
    """block k's payload is what zlz4_batch_compress_hc_using_dict returns for the same record and in-input dictionary"""
    for level in (3, 9):
        kw, cs, items, res, frames = own[level, 0]
        for k in (8, 10):
            data = items[k]
            records = [data[s:s + 65536] for s in range(0, len(data), 65536)]
            in_input = [(1 + max(0, j * 65536 - 65536), min(j * 65536, 65536)) for j in range(len(records))]
            got, want = hg.run_batch(zl, cref, records, [hg.bound(len(r)) for r in records], None, None, gpu, level,
                                     layout=gh.Packed(gaps=(0, 0)), in_input=in_input)
            hg.check(got, want, "staged")
            for j, ((payload, stored), (r, staged)) in enumerate(zip(lh.blocks_of(frames[k]), got)):
                assert (records[j] if stored else payload) == (records[j] if r >= len(records[j]) else staged), (level, k, j)


# ------------------------------------------------------------------ 2. larger blocks, rounds
def test_256k_blocks(zl, gpu, model, hc_fixture):
    r = lg.RECIPES[2]
    data = lg.recipe_input(r)                          # 600 000 bytes: blocks of 256 KiB with a 64 KiB tail in front
    p = _prefs(zl.Prefs, compression_level=9, block_size_id=5)
    rc, res, frames, _ = _compress_ex(zl, gpu, [data, data[:262144 + 13], data[:100]], p, zl.lz4f.BATCH_LINK_BLOCKS)
    assert rc == 0
    for b, n, f in zip((data, data[:262144 + 13], data[:100]), res, frames):
        want = model(b, 9, dict(block_size_id=5))
        assert n == len(want) and f == want, (len(b), n, len(want))
    e = hc_fixture[r["name"], 9]
    assert res[0] == e["frame_len"] == 17357 and hashlib.sha256(frames[0]).hexdigest() == e["frame_sha256"]
    got, outs = _decompress(zl, gpu, frames[:1], [len(data)], zl.lz4f.DECODE_LINKED)
    assert got == [len(data)] and outs[0] == data


def test_rounds_reuse_both_result_halves(zl, gpu, cref):
    """4 MiB blocks: a chunk holds on the order of a hundred entries, so a table of 2 * chunk + 7 entries runs in five
    rounds of half a chunk: both halves of the result area are reused after the event wait.  The one two-block frame lies
    across the boundary of rounds 2 and 3; all other entries are one-block frames of a few KiB."""
    import torch
    L = zl.lib()
    link = zl.lz4f.BATCH_LINK_BLOCKS
    level, bs = 4, 4 << 20
    p = _prefs(zl.Prefs, compression_level=level, block_size_id=7)
    fast = _prefs(zl.Prefs, block_size_id=7)

    def area(n):                                       # what the linked HC levels add to the fast level's table and slots
        return L.zlz4f_batch_compress_frame_workspace_ex(1, n, p, link) - L.zlz4f_batch_compress_frame_workspace(1, n, fast)
    per = area(1)                                      # links, results, visited bits and descriptors of one entry
    chunk = round(area(100000) / per)
    # the area grows by an entry's share up to `chunk` entries and by descriptors only beyond
    assert 50 < chunk < 200 and area(chunk) - area(chunk - 1) > per // 2 and area(chunk + 50) - area(chunk) < per // 2
    max_blocks = 2 * chunk + 7
    half = chunk // 2
    base = bytes(dg.text_bytes(50000, 21))
    big = bytearray((base * 86)[:bs + 70000])
    big[::997] = bytes(x ^ 0x55 for x in big[::997])
    big = bytes(big)
    items = [bytes(dg.text_bytes(2000 + 37 * (i % 50), 3000 + i)) for i in range(max_blocks - 2)]
    items.insert(3 * half - 1, big)                    # its blocks are entries 3 * half - 1 (round 2) and 3 * half (round 3)
    caps = [zl.lz4f.compressFrameBound(len(b), p) for b in items]
    d_src, s_off, s_len = _stage(items, gpu)
    d_dst, offs, t_off, t_cap = _slots(caps, gpu)
    result = torch.full((len(items),), -999, dtype=torch.int64, device=gpu)
    ws = torch.empty(zl.lz4f.compressFrameBatchWorkspace(len(items), max_blocks, p, link), dtype=torch.uint8, device=gpu)
    assert L.zlz4f_batch_compress_frame_ex(None, d_src.data_ptr(), s_off.data_ptr(), s_len.data_ptr(), d_dst.data_ptr(),
                                           t_off.data_ptr(), t_cap.data_ptr(), result.data_ptr(), len(items), max_blocks, p,
                                           link, ws.data_ptr(), ws.numel()) == 0
    torch.cuda.synchronize()
    res = result.cpu().tolist()
    guards = torch.cat([d_dst[:offs[0]]] + [d_dst[o + c:o + c + GUARD] for o, c in zip(offs, caps)])
    assert bool((guards == FILL).all()), "bytes outside the destination slots were written"
    bad = []
    for k, b in enumerate(items):
        want = lh.compress_frame_linked_hc(b, level, dict(block_size_id=7), lambda blk, d, lv: cref.compress(blk, d, lv)[1])
        got = d_dst[offs[k]:offs[k] + max(res[k], 0)].cpu().numpy().tobytes()
        if res[k] != len(want) or got != want:
            bad.append((k, len(b), res[k], len(want)))
    assert not bad, (len(bad), bad[:8])
    assert len(lh.blocks_of(d_dst[offs[3 * half - 1]:offs[3 * half - 1] + res[3 * half - 1]].cpu().numpy().tobytes())) == 2


# ------------------------------------------------------------------ 3. statuses
def test_max_blocks_too_small_and_a_short_destination(zl, gpu, model):
    text = lg.recipe_input(lg.RECIPES[0])
    items = [text[:70000], text[:65536], text[:140000], text[:5]]      # 2, 1, 3, 1 blocks
    p = _prefs(zl.Prefs, compression_level=9)
    link = zl.lz4f.BATCH_LINK_BLOCKS
    rc, res, frames, untouched = _compress_ex(zl, gpu, items, p, link, max_blocks=4)
    assert rc == 0 and res[2:] == [-5, -5] and untouched[2:] == [True, True]
    assert frames[0] == model(items[0], 9) and frames[1] == model(items[1], 9)
    caps = [zl.lz4f.compressFrameBound(len(b), p) for b in items]
    caps[1] -= 1
    rc, res, frames, untouched = _compress_ex(zl, gpu, items, p, link, caps=caps)
    assert rc == 0 and res[1] == -111
    for k in (0, 2, 3):
        assert frames[k] == model(items[k], 9), k


def test_plain_call_refuses_and_ex_is_the_plain_call_elsewhere(zl, gpu):
    text = lg.recipe_input(lg.RECIPES[0])
    items = [text[:n] for n in (0, 13, 65537, 150000)]
    link = zl.lz4f.BATCH_LINK_BLOCKS
    p9 = _prefs(zl.Prefs, compression_level=9)
    rc, res, frames, untouched = _compress_ex(zl, gpu, items, p9, link, fn="zlz4f_batch_compress_frame")
    assert rc == -8 and res == [-999] * 4 and all(untouched)           # nothing was launched
    for level in (2, 10):
        rc, res, frames, untouched = _compress_ex(zl, gpu, items, _prefs(zl.Prefs, compression_level=level), link)
        assert rc == -8 and res == [-999] * 4 and all(untouched)
    for prefs, flag_sets in ((_prefs(zl.Prefs), (0, 1, 4, 5)), (p9, (0, 1)), (_prefs(zl.Prefs, compression_level=2), (0,))):
        for flags in flag_sets:
            a = _compress_ex(zl, gpu, items, prefs, flags, fn="zlz4f_batch_compress_frame")
            b = _compress_ex(zl, gpu, items, prefs, flags)
            assert a[0] == b[0] == 0 and a[1] == b[1] and a[2] == b[2], (prefs.compression_level, flags)
    # a misaligned workspace
    import torch
    L = zl.lib()
    d_src, s_off, s_len = _stage(items, gpu)
    caps = [zl.lz4f.compressFrameBound(len(b), p9) for b in items]
    d_dst, offs, t_off, t_cap = _slots(caps, gpu)
    result = torch.full((4,), -999, dtype=torch.int64, device=gpu)
    n = zl.lz4f.compressFrameBatchWorkspace(4, 5, p9, link)
    ws = torch.empty(n + 16, dtype=torch.uint8, device=gpu)
    args = (None, d_src.data_ptr(), s_off.data_ptr(), s_len.data_ptr(), d_dst.data_ptr(), t_off.data_ptr(), t_cap.data_ptr(),
            result.data_ptr(), 4, 5, p9, link)
    assert L.zlz4f_batch_compress_frame_ex(*args, ws.data_ptr() + 4, n) == -5
    assert L.zlz4f_batch_compress_frame_ex(*args, ws.data_ptr(), n - 1) == -5
    assert L.zlz4f_batch_compress_frame_ex(*args, None, n) == -5
    torch.cuda.synchronize()
    assert result.cpu().tolist() == [-999] * 4 and bool((d_dst == FILL).all())


# ------------------------------------------------------------------ 4. single-frame calls, Python routing
def test_single_calls_equal_the_batch_frames(zl, gpu, own, model, hc_fixture):
    import torch
    link = zl.lz4f.BATCH_LINK_BLOCKS
    kw, cs, items, res, frames = own[9, 0]
    p9, p0 = _prefs(zl.Prefs, compression_level=9), _prefs(zl.Prefs)
    for k in (0, 3, 8, 10):
        assert zl.lz4f.compressFrame(items[k], p9, flags=link) == frames[k], k
    data = items[9]
    d_src = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(gpu)
    cap = zl.lz4f.compressFrameBound(len(data), p9)
    d_dst = torch.full((cap + 5,), FILL, dtype=torch.uint8, device=gpu)
    r = zl.lz4f.compressFrameDevice(d_src, d_dst[:cap], p9, flags=link)
    host = d_dst.cpu().numpy()
    assert r == res[9] and host[:r].tobytes() == frames[9] and (host[cap:] == FILL).all()
    with pytest.raises(zl.Lz4Error) as e:
        zl.lz4f.compressFrameDevice(d_src, d_dst[:cap - 1], p9, flags=link)
    assert e.value.code == -111
    # the checksum recipe, without a content size
    pc = _prefs(zl.Prefs, compression_level=6, block_checksum=1, content_checksum=1)
    f = zl.lz4f.compressFrame(data, pc, flags=link)
    ec = hc_fixture["text160k_bs64k_checksums", 6]
    assert len(f) == ec["frame_len"] and hashlib.sha256(f).hexdigest() == ec["frame_sha256"]
    # the fast level with the flag: the fast linked frame; content size from the length
    assert zl.lz4f.compressFrame(data, p0, flags=link) == lf.compress_frame_linked(data)
    assert zl.lz4f.compressFrame(data, p0, flags=link | zl.lz4f.BATCH_CONTENT_SIZE) == \
        lf.compress_frame_linked(data, dict(content_size=len(data)))
    assert zl.lz4f.compressFrameDevice(d_src, d_dst[:cap], p0, flags=link) == len(lf.compress_frame_linked(data))
    # flags 0: the call they are named after
    L = zl.lib()
    for p in (p0, p9, _prefs(zl.Prefs, compression_level=2, block_mode=1, content_checksum=1)):
        want = zl.lz4f.compressFrame(data, p)
        cap = zl.lz4f.compressFrameBound(len(data), p)
        src = (zl.C.c_uint8 * len(data)).from_buffer_copy(data)
        dst = (zl.C.c_uint8 * cap)()
        n = L.zlz4f_compress_frame_ex(zl.C.addressof(src), len(data), zl.C.addressof(dst), cap, p, 0)
        assert n == len(want) and bytes(dst[:n]) == want, p.compression_level
        assert L.zlz4f_compress_frame_ex(zl.C.addressof(src), len(data), zl.C.addressof(dst), cap - 1, p, 0) == -111
        dd = torch.full((cap,), FILL, dtype=torch.uint8, device=gpu)
        n = L.zlz4f_compress_frame_device_ex(None, d_src.data_ptr(), len(data), dd.data_ptr(), cap, p, 0)
        assert n == len(want) and dd.cpu().numpy()[:n].tobytes() == want, p.compression_level
    # the Python batch helpers route to the _ex entry
    assert zl.lz4f.compressFrames([items[8], items[3], items[10]], p9, link) == [frames[8], frames[3], frames[10]]
    assert zl.lz4f.compressFrames([data], p9) == [zl.lz4f.compressFrame(data, p9)]


# ------------------------------------------------------------------ 5. graph capture
def test_ex_batch_in_a_captured_graph(zl, gpu, model):
    import torch
    n = 12
    text = lg.recipe_input(lg.RECIPES[2])
    items = [text[k * 3000: k * 3000 + 2000 + 500 * (k % 5) + (140000 if k % 6 == 0 else 0)] for k in range(n)]
    items2 = [bytes(dg.mixed_bytes(len(b), 700 + k)) for k, b in enumerate(items)]
    kw = dict(block_checksum=1, content_checksum=1)
    p = _prefs(zl.Prefs, compression_level=5, **kw)
    link = zl.lz4f.BATCH_LINK_BLOCKS
    caps = [zl.lz4f.compressFrameBound(len(b), p) for b in items]
    max_blocks = sum((len(b) + 65535) // 65536 for b in items)
    d_src, s_off, s_len = _stage(items, gpu)
    d_frm, f_offs, t_foff, t_fcap = _slots(caps, gpu)
    cres = torch.zeros(n, dtype=torch.int64, device=gpu)
    cws = torch.empty(zl.lz4f.compressFrameBatchWorkspace(n, max_blocks, p, link), dtype=torch.uint8, device=gpu)

    def run():
        zl.lz4f.compressFrameBatch(d_src, s_off, s_len, d_frm, t_foff, t_fcap, cres, p, link, max_blocks, cws)

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
        g.replay()
        torch.cuda.synchronize()
        c = cres.cpu().tolist()
        frm = d_frm.cpu().numpy().tobytes()
        for k, b in enumerate(batch):
            want = model(b, 5, kw)
            assert c[k] == len(want) and frm[f_offs[k]:f_offs[k] + c[k]] == want, k


# ------------------------------------------------------------------ 6. the C++ mirror
def test_cpp_mirror_ex_calls(zl, gpu, model, tmp_path):
    """tests/host_mirror_linked_hc.cpp built with g++ against the shipped library: compressFrameEx, compressFrameDeviceEx
    and compressFrameBatchEx of zig-lz4_amd/csrc/host/zlz4.hpp write the model's frame."""
    if shutil.which("g++") is None:
        pytest.skip("no g++ on this box: the C++ mirror's new calls were NOT exercised")
    exe = str(tmp_path / "hml")
    libdir = os.path.dirname(zl.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "host_mirror_linked_hc.cpp"),
                           "-L", libdir, "-lzlz4_amd", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib"])
    data = lg.recipe_input(lg.RECIPES[0])[:150001]
    src = tmp_path / "in.bin"
    src.write_bytes(data)
    outs = [str(tmp_path / ("frame%d.out" % k)) for k in range(3)]
    run = subprocess.run([exe, str(src)] + outs, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "linked hc mirror ok" in run.stdout, run.stdout + run.stderr
    want = model(data, 9)
    for o in outs:
        assert open(o, "rb").read() == want, o
