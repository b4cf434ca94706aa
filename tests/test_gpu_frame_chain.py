"""Every consumer of the lz4f block chain on the GPU answers every case of tests/chaingen.py (all prefixes of tiny frames
with and without checksums, a zero-size stored block, a block word far past the input, bytes behind the frame).  The
expectations come from the Python models and chaingen.walk, never from another GPU call.  Destinations are fenced by guard
bytes (test_gpu_frame_batch._slots / _collect).  Run on the GPU box: pytest -m gpu."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import chaingen as g
import multiframegen as mg
import test_gpu_frame_batch as fb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "pyref"))
import zig_lz4_frame_prefix as fp  # noqa: E402
import zig_lz4_frame_range as fr  # noqa: E402
import zig_lz4_linked_frame as lf  # noqa: E402
import zig_lz4_sizes as zs  # noqa: E402

pytestmark = pytest.mark.gpu

CAP = 160                                             # above the 128 content bytes: never too small
ERR_DEVICE = -7


@functools.lru_cache(maxsize=None)
def _decoded(b):
    """(result, bytes) of the frame decoders for a destination of CAP bytes (independent blocks: both flags alike)"""
    return lf.decompress_frame_linked(b, CAP)


def _blocks(cs):
    return sum(g.walk(b)[1] for _, b in cs)


def _differ(cs, got, want):
    bad = [(name, a, w) for (name, _), a, w in zip(cs, got, want) if a != w]
    assert not bad, "%d of %d cases differ: %r" % (len(bad), len(cs), bad[:6])


@pytest.mark.parametrize("flags", [0, 1])
def test_batch_decompress_frame(zl, gpu, flags):
    import torch
    cs = g.cases()
    frames = [b for _, b in cs]
    d_src, s_off, s_len = fb._stage(frames, gpu)
    d_dst, offs, t_off, t_cap = fb._slots([CAP] * len(cs), gpu)
    result = torch.full((len(cs),), -999, dtype=torch.int64, device=gpu)
    zl.lz4f.decompressFrameBatch(d_src, s_off, s_len, d_dst, t_off, t_cap, result, _blocks(cs), flags=flags)
    res, outs = fb._collect(d_dst, offs, [CAP] * len(cs), result)
    got = [(r, o if r >= 0 else b"") for r, o in zip(res, outs)]
    _differ(cs, got, [_decoded(b) for b in frames])


@pytest.mark.parametrize("flags", [0, 1])
def test_batch_frame_decompressed_size(zl, gpu, flags):
    import torch
    cs = g.cases()
    frames = [b for _, b in cs]
    d_src, s_off, s_len = fb._stage(frames, gpu)
    size = torch.full((len(cs),), -999, dtype=torch.int64, device=gpu)
    zl.lz4f.frameDecompressedSizeBatch(d_src, s_off, s_len, size, _blocks(cs), flags=flags)
    model = lf.frame_size_linked if flags else zs.frame_size
    _differ(cs, size.cpu().tolist(), [model(b) for b in frames])


@pytest.mark.parametrize("n", [g.CONTENT_SIZE + 1, 70])
def test_batch_decompress_frame_prefix(zl, gpu, n):
    """n = 129: the whole chain is walked; n = 70: the cut falls inside the stored block"""
    import torch
    cs = g.cases()
    frames = [b for _, b in cs]
    d_src, s_off, s_len = fb._stage(frames, gpu)
    d_dst, offs, t_off, t_cap = fb._slots([n] * len(cs), gpu)
    result = torch.full((len(cs),), -999, dtype=torch.int64, device=gpu)
    zl.batch_decompress_frame_prefix(d_src, s_off, s_len, d_dst, t_off, t_cap, result)
    res, outs = fb._collect(d_dst, offs, [n] * len(cs), result)
    got = [(r, o if r > 0 else b"") for r, o in zip(res, outs)]
    want = [fp.decompress_frame_prefix(b, n) for b in frames]
    _differ(cs, got, [(r, d if r > 0 else b"") for r, d in want])


def test_batch_frame_index(zl, gpu):
    import torch
    cs = g.cases()
    frames = [b for _, b in cs]
    caps = [g.walk(b)[1] + 1 for b in frames]
    idx_off = np.cumsum([0] + [c + 1 for c in caps[:-1]]).astype(np.int64)          # one spare entry behind every frame
    fill = -7
    index = torch.full((int(idx_off[-1]) + caps[-1] + 1, 2), fill, dtype=torch.int64, device=gpu)
    idx_n = torch.full((len(cs),), -999, dtype=torch.int64, device=gpu)
    d_src, s_off, s_len = fb._stage(frames, gpu)
    zl.lz4f.frameIndexBatch(d_src, s_off, s_len, index, torch.from_numpy(idx_off).to(gpu),
                            torch.tensor(caps, dtype=torch.int64, device=gpu), idx_n, _blocks(cs))
    n, host = idx_n.cpu().tolist(), index.cpu().numpy()
    got = []
    for f in range(len(cs)):
        lo, used = int(idx_off[f]), (n[f] + 1 if n[f] >= 0 else 0)
        got.append((n[f], [tuple(int(x) for x in e) for e in host[lo:lo + used]]))
        assert (host[lo + used:lo + caps[f] + 1] == fill).all(), "%s: entries behind the result were written" % cs[f][0]
    _differ(cs, got, [fr.frame_index(b) for b in frames])


def test_batch_multiframe_split(zl, gpu):
    """every case as a buffer of its own: member count, positions, lengths and kinds, and the chain blocks of the members"""
    cs = g.cases()
    bufs = [b for _, b in cs]
    sp = zl.lz4f.splitMultiframes(bufs, gpu)
    rows, first = sp.member.cpu().tolist(), sp.item_first.cpu().tolist()
    got = [[(pos, ln, kb & 0xFF, (kb >> 8) & 15) for pos, ln, kb in rows[first[s]:first[s] + r]] if r >= 0 else r
           for s, r in enumerate(sp.results)]
    _differ(cs, got, [mg.table(b) for b in bufs])
    assert sp.nitems == sum(len(mg.split(b)) for b in bufs)
    assert sp.max_blocks == sum(m.nb for b in bufs for m in mg.split(b))


def test_decompress_frame_device_per_case(zl, gpu):
    """the single-frame walk (k_frame_walk): one call per case of the both-checksums variant and its mutations"""
    import torch
    cs = g.cases(bc=1, cc=1)
    assert 500 < len(cs) < 900
    frames = [b for _, b in cs]
    d_src, s_off, _ = fb._stage(frames, gpu)
    d_dst, offs, _, _ = fb._slots([CAP] * len(cs), gpu)
    src_off = s_off.cpu().tolist()
    fn, st = zl.lib().zlz4f_decompress_frame_device, zl._stream()
    res = []
    for k, b in enumerate(frames):
        res.append(fn(st, C.c_void_p(d_src.data_ptr() + src_off[k]), len(b), C.c_void_p(d_dst.data_ptr() + offs[k]), CAP))
    _, outs = fb._collect(d_dst, offs, [CAP] * len(cs), torch.tensor(res, dtype=torch.int64))
    got = [(r, o if r >= 0 else b"") for r, o in zip(res, outs)]
    _differ(cs, got, [_decoded(b) for b in frames])


def test_host_calls_size_and_range(zl, gpu):
    """zlz4f_frame_decompressed_size and zlz4f_decompress_frame_range(0, 2^40) size their table with a host walk of the
    chain: the plain variant and its zero-size stored block; no case may report a device error"""
    cs = g.cases(bc=0, cc=0, only=("bc0_cc0", "_zero_stored"))
    assert 200 < len(cs) < 400
    lib = zl.lib()
    sizes, ranges = [], []
    for _, b in cs:
        s, n = zl._in(b)
        sizes.append(lib.zlz4f_frame_decompressed_size(C.addressof(s), n))
        d = (C.c_uint8 * 4096)()
        r = lib.zlz4f_decompress_frame_range(C.addressof(s), n, 0, 1 << 40, C.addressof(d), 4096)
        ranges.append((r, bytes(d[:r]) if r > 0 else b""))
    assert ERR_DEVICE not in sizes and ERR_DEVICE not in [r for r, _ in ranges]
    _differ(cs, sizes, [zs.frame_size(b) for _, b in cs])
    _differ(cs, ranges, [fr.frame_range(b, 0, 1 << 40) for _, b in cs])
