"""Decompressed-size queries on the HIP path: zlz4_batch_decompressed_size / zlz4_batch_plan_outputs /
zlz4f_batch_frame_decompressed_size against the restatement tools/pyref/zig_lz4_sizes.py, the oracle and the decoders the
sizes are meant for.  Run on the GPU box: pytest -m gpu."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "pyref"))
import datagen as dg  # noqa: E402
import gpu_harness as gh  # noqa: E402
import sizegen  # noqa: E402
import zig_lz4_dict as pd  # noqa: E402
import zig_lz4_sizes as ps  # noqa: E402

pytestmark = pytest.mark.gpu

OTS, CORRUPT, INVALID = -1, -3, -5
FILL = 0xA5


def _u32(a, dev):
    import torch
    return torch.from_numpy(np.asarray(a, dtype=np.int64).astype(np.uint32).view(np.int32)).to(dev)


class Batch:
    """compressed blocks staged on the device in one of gpu_harness's layouts"""

    def __init__(self, items, dev, layout=None):
        import torch
        self.buf, offs, lens = gh._pack(items, layout=layout)
        self.n, self.dev = len(items), dev
        self.d_in = torch.from_numpy(self.buf).to(dev)
        self.in_off = torch.from_numpy(offs).to(dev)
        self.in_len = _u32(lens, dev)

    def sizes(self, zl, dict_lens=None):
        import torch
        size = torch.full((self.n,), -999, dtype=torch.int64, device=self.dev)
        zl.batch_decompressed_size(self.d_in, self.in_off, self.in_len, size,
                                   _u32(dict_lens, self.dev) if dict_lens is not None else None)
        torch.cuda.synchronize()
        assert (self.d_in.cpu().numpy() == self.buf).all(), "the input arena changed"
        return size


@pytest.fixture(scope="module")
def streams(oracle):
    """the CPU corpus, with a second round of damage so that the batch holds several thousand blocks"""
    base = sizegen.block_streams(oracle)
    rng = np.random.default_rng(5)
    extra = []
    for name, c, _ in base:
        if 0 < len(c) <= 20000:
            extra += [(name + "/x%d" % j, v, None) for j, v in enumerate(sizegen._damaged(c, rng)[:3])]
    return base + extra


@pytest.fixture(scope="module")
def expected(streams):
    return [ps.block_size(c) for _, c, _ in streams]


# ------------------------------------------------------------------ 1. block parity
@pytest.mark.parametrize("layout", [None, gh.Packed(seed=3, fill="cont"), gh.Packed(seed=4, fill="zero", gaps=(0, 0))],
                         ids=["aligned", "packed-cont", "packed-tight"])
def test_block_sizes_match_pyref_and_oracle(zl, oracle, gpu, streams, expected, layout):
    assert len(streams) > 3000
    items = [c for _, c, _ in streams]
    got = Batch(items, gpu, layout).sizes(zl).cpu().tolist()
    bad = [(streams[k][0], len(items[k]), got[k], expected[k]) for k in range(len(items)) if got[k] != expected[k]]
    assert not bad, (len(bad), bad[:8])
    assert sum(1 for e in expected if e == CORRUPT) > 300 and sum(1 for e in expected if e > 0) > 1500
    if layout is None:
        for k, c in enumerate(items):
            if len(c) <= 20000:                                   # where the oracle's buffer allows
                want = oracle.decompress_safe(c, sizegen.oracle_cap(c))
                assert got[k] == (want if isinstance(want, int) else len(want)), streams[k][0]


@pytest.mark.parametrize("layout", [None, gh.Packed(seed=8, fill="cont")], ids=["aligned", "packed"])
def test_block_sizes_with_dictionary_lengths(zl, gpu, streams, tmp_path, layout):
    """d_dict_len given: arbitrary lengths on the plain corpus, and the dictionary records at their full length, one
    byte short of their deepest reach and at length 0"""
    rng = np.random.default_rng(11)
    items, dls, names = [], [], []
    for name, c, _ in streams:
        items.append(c)
        dls.append(int(rng.choice((0, 1, 7, 4096, 65535, 65536, 65537, 200000, 0xFFFFFFFF))))
        names.append(name)
    for name, c, dct in sizegen.dict_records(tmp_path):
        reach = []
        full = ps.block_size(c, len(dct), reach=reach)
        for dl in [len(dct), 0] + ([max(reach) - 1, max(reach)] if full >= 0 and reach else []):
            items.append(c)
            dls.append(dl)
            names.append("%s@%d" % (name, dl))
    want = [ps.block_size(c, min(dl, 65536)) for c, dl in zip(items, dls)]
    got = Batch(items, gpu, layout).sizes(zl, dls).cpu().tolist()
    bad = [(names[k], dls[k], got[k], want[k]) for k in range(len(items)) if got[k] != want[k]]
    assert not bad, (len(bad), bad[:8])
    tail = want[len(streams):]
    assert sum(1 for w in tail if w == CORRUPT) > 60 and sum(1 for w in tail if w > 0) > 100


def test_single_call_equals_the_batch(zl, tmp_path):
    recs = sizegen.dict_records(tmp_path)[::9]
    for name, c, dct in recs:
        for dl in (None, len(dct)):
            want = ps.block_size(c, dl)
            try:
                got = zl.decompressedSize(c, dl or 0)
            except zl.Lz4Error as e:
                got = e.code
            assert got == want, (name, dl, got, want)


# ------------------------------------------------------------------ 2. the sizes are tight: size -> plan -> decode
@pytest.mark.parametrize("align", [0, 1, 64, 4096])
def test_plan_then_decode_round_trips_and_one_byte_less_fails(zl, oracle, gpu, streams, expected, align):
    import torch
    items = [c for _, c, _ in streams]
    n = len(items)
    bt = Batch(items, gpu)
    size = bt.sizes(zl)
    out_off = torch.full((n,), -1, dtype=torch.int64, device=gpu)
    out_cap = torch.full((n,), -1, dtype=torch.int32, device=gpu)
    total = torch.full((1,), -1, dtype=torch.int64, device=gpu)
    zl.batch_plan_outputs(size, out_off, out_cap, total, align)
    a = max(align, 1)
    slots = [(max(s, 0) + a - 1) // a * a for s in expected]
    offs = np.concatenate(([0], np.cumsum(slots)))
    assert out_off.cpu().tolist() == offs[:-1].tolist()
    assert out_cap.cpu().numpy().view(np.uint32).tolist() == [max(s, 0) for s in expected]
    assert int(total.item()) == int(offs[-1])
    tail = 256                                                     # guard bytes behind the last slot
    for less in (0, 1):
        caps = [max(max(s, 0) - less, 0) for s in expected]
        d_out = torch.full((int(offs[-1]) + tail,), FILL, dtype=torch.uint8, device=gpu)
        res = torch.full((n,), -999, dtype=torch.int64, device=gpu)
        zl.batch_decompress_safe(bt.d_in, bt.in_off, bt.in_len, d_out, out_off, _u32(caps, gpu) if less else out_cap, res)
        torch.cuda.synchronize()
        r = res.cpu().tolist()
        host = d_out.cpu().numpy()
        inside = np.zeros(len(host), dtype=bool)
        for k in range(n):
            inside[offs[k]:offs[k] + caps[k]] = True
        assert (host[~inside] == FILL).all(), "bytes between the slots were written (align %d, less %d)" % (align, less)
        for k, (name, c, plain) in enumerate(streams):
            s = expected[k]
            if less == 0:
                if s >= 1:
                    assert r[k] == s, (name, r[k], s)
                    want = plain if plain is not None else oracle.decompress_safe(c, s)
                    assert host[offs[k]:offs[k] + s].tobytes() == want, name
                else:
                    assert r[k] == 0, (name, r[k], s)              # capacity 0: src/lz4.zig:98
            elif s - 1 >= 1:
                assert r[k] == OTS, (name, r[k], s)


# ------------------------------------------------------------------ 3. the 32-bit edge
def test_blocks_at_the_32_bit_limit(zl, gpu):
    """~17 MB of input each, no output anywhere: exactly 0xFFFFFFFF bytes, one byte more, and a stream that ends inside
    its run of 0xFF; two small blocks ride along"""
    items = [sizegen.edge_block(0xFFFFFFFF), sizegen.edge_block(0x100000000), sizegen.edge_block(0xFFFFFFFF, end_inside=True),
             sizegen.edge_block(70000), sizegen.edge_block(0xFFFFFFFE)]
    want = [0xFFFFFFFF, OTS, CORRUPT, 70000, 0xFFFFFFFE]
    for layout in (None, gh.Packed(seed=1)):
        assert Batch(items, gpu, layout).sizes(zl).cpu().tolist() == want
    # the limit counts literals too: 0xFFFFFFFF - 3 from the match, then 3 / 4 literals
    base = sizegen.edge_block(0xFFFFFFFF - 3)
    assert Batch([base + b"\x30abc", base + b"\x40abcd"], gpu).sizes(zl).cpu().tolist() == [0xFFFFFFFF, OTS]


# ------------------------------------------------------------------ 4. frames
def _stage_frames(frames, gpu):
    import test_gpu_frame_batch as fb
    return fb._stage(frames, gpu)


def _frame_sizes(zl, gpu, frames, max_blocks=None, workspace=None):
    import torch
    d_src, s_off, s_len = _stage_frames(frames, gpu)
    if max_blocks is None:
        max_blocks = sum(zl._chain_blocks(f) for f in frames)
    size = torch.full((len(frames),), -999, dtype=torch.int64, device=gpu)
    zl.lz4f.frameDecompressedSizeBatch(d_src, s_off, s_len, size, max_blocks, workspace)
    torch.cuda.synchronize()
    return size.cpu().tolist()


def test_frame_sizes_match_the_batch_decoder_and_pyref(zl, oracle, gpu):
    import test_gpu_frame_batch as fb
    corpus = sizegen.frame_corpus(oracle)
    frames = [f for _, f, _ in corpus]
    assert len(frames) > 600
    room = []
    want = [ps.frame_size(f, room) for f in frames]
    got = _frame_sizes(zl, gpu, frames)
    bad = [(corpus[k][0], got[k], want[k]) for k in range(len(frames)) if got[k] != want[k]]
    assert not bad, (len(bad), bad[:8])
    # ample: room for every block in front of the frame's first error and 4 KiB more (the decoder's error order must not
    # meet a capacity error first); a size that is too small would show as an error of the decoder
    caps = [r + 4096 for r in room]
    res, outs = fb._decompress(zl, gpu, frames, caps)
    n_exc = 0
    for k, (name, f, content) in enumerate(corpus):
        if res[k] == -118:                                         # the documented exception
            assert got[k] >= 0, (name, got[k])
            n_exc += 1
        else:
            assert got[k] == res[k], (name, got[k], res[k])
        if content is not None:
            assert got[k] == len(content) and outs[k] == content, name
    assert n_exc > 0 and len({r for r in res if r < 0}) >= 6       # the batch mixes block sizes, flags and outcomes


def test_frame_single_call_equals_the_batch(zl, oracle, gpu):
    corpus = sizegen.frame_corpus(oracle)[::23]
    for name, f, _ in corpus:
        want = ps.frame_size(f)
        try:
            got = zl.lz4f.frameDecompressedSize(f)
        except zl.Lz4Error as e:
            got = e.code
        assert got == want, (name, got, want)


def test_frame_sizes_max_blocks_cuts_the_batch(zl, oracle, gpu):
    p = oracle.Prefs()
    p.block_checksum = 1
    items = [bytes(dg.text_bytes(n, 80 + k)) for k, n in enumerate((70000, 100, 0, 200000, 3000, 140000))]
    frames = [oracle.compress_frame(b, p) for b in items]
    nbs = [zl._chain_blocks(f) for f in frames]
    total = sum(nbs)
    for max_blocks in (total, total - 1, nbs[0] + 1, 0):
        got = _frame_sizes(zl, gpu, frames, max_blocks)
        base = 0
        for k, b in enumerate(items):
            if nbs[k] and base + nbs[k] > max_blocks:
                assert got[k] == INVALID, (max_blocks, k, got)
            else:
                assert got[k] == len(b), (max_blocks, k, got)
            base += nbs[k]


def test_frame_sizes_workspace_too_small_or_misaligned(zl, oracle, gpu):
    import torch
    frames = [oracle.compress_frame(bytes(dg.text_bytes(5000, k))) for k in range(4)]
    d_src, s_off, s_len = _stage_frames(frames, gpu)
    need = zl.lz4f.frameDecompressedSizeBatchWorkspace(4, 4)
    ws = torch.empty(need + 64, dtype=torch.uint8, device=gpu)
    assert ws.data_ptr() % 16 == 0
    size = torch.full((4,), -999, dtype=torch.int64, device=gpu)
    for bad in (ws[:need - 1], ws[8:], ws[1:]):
        with pytest.raises(zl.Lz4Error) as e:
            zl.lz4f.frameDecompressedSizeBatch(d_src, s_off, s_len, size, 4, bad)
        assert e.value.name == "InvalidState"
    for args in ((None, s_off, s_len, size), (d_src, None, s_len, size), (d_src, s_off, None, size)):     # null arguments
        assert zl.lib().zlz4f_batch_frame_decompressed_size(zl._stream(), *[zl._ptr(t) for t in args], 4, 4, zl._ptr(ws),
                                                            ws.numel()) == INVALID
    torch.cuda.synchronize()
    assert size.cpu().tolist() == [-999] * 4                       # nothing was launched
    zl.lz4f.frameDecompressedSizeBatch(d_src, s_off, s_len, size, 4, ws[16:])
    torch.cuda.synchronize()
    assert size.cpu().tolist() == [5000] * 4


def test_decompress_frames_without_caps(zl, oracle, gpu):
    corpus = [(n, f, c) for n, f, c in sizegen.frame_corpus(oracle) if c is not None][::3]
    frames = [f for _, f, _ in corpus] + [corpus[1][1][:-2], b"not a frame"]      # (half an end mark: FrameSizeWrong)
    outs = zl.lz4f.decompressFrames(frames, device=gpu)
    for (name, f, content), out in zip(corpus, outs):
        assert out == content, name
    assert outs[-1] == -113 and outs[-2] == -114
    # caps given: exactly as before
    caps = [len(c) for _, _, c in corpus]
    assert zl.lz4f.decompressFrames(frames[:len(corpus)], caps, device=gpu) == [c for _, _, c in corpus]


# ------------------------------------------------------------------ 5. the convenience call
def test_decompress_blocks_mixed_list(zl, oracle, gpu, streams, tmp_path):
    recs = sizegen.dict_records(tmp_path)
    plain_part = [(name, c, None) for name, c, _ in streams[::5] if len(c) <= 70000]
    mixed = plain_part + [(name, c, dct) for name, c, dct in recs]
    outs = zl.decompressBlocks([c for _, c, _ in mixed], [d for _, _, d in mixed], device=gpu)
    n_err = 0
    for (name, c, dct), out in zip(mixed, outs):
        if dct is None:
            want = oracle.decompress_safe(c, sizegen.oracle_cap(c))
        else:
            r, b = pd.decompress_safe_using_dict(c, sizegen.oracle_cap(c), dct)
            want = b if r >= 0 else r
        assert out == want, (name, out if isinstance(out, int) else len(out), want if isinstance(want, int) else len(want))
        n_err += isinstance(want, int)
    assert n_err > 20
    # without dictionaries
    outs = zl.decompressBlocks([c for _, c, _ in plain_part], device=gpu)
    for (name, c, _), out in zip(plain_part, outs):
        assert out == oracle.decompress_safe(c, sizegen.oracle_cap(c)), name
    assert zl.decompressBlocks([], device=gpu) == []


# ------------------------------------------------------------------ 6. graph capture
def test_size_plan_decode_in_a_captured_graph(zl, oracle, gpu):
    import torch
    n = 512
    text = bytes(dg.text_bytes(n * 3000 + 70000, 31))
    sets = []
    for seed in (0, 1):
        plain = [text[k * 3000 + 17 * seed: k * 3000 + 17 * seed + 2000 + 600 * ((k + seed) % 7) + (60000 if k % 100 == seed else 0)]
                 for k in range(n)]
        comp = [oracle.compress_default(b) for b in plain]
        comp[5 + seed] = comp[5 + seed][:-3]                       # a malformed member
        sets.append((plain, comp))
    slot = max(len(c) for _, cs in sets for c in cs) + 16
    arena = max(sum(len(b) for b in plain) for plain, _ in sets) + 64 * n + 4096

    def stage(comp):
        buf = np.zeros(n * slot, dtype=np.uint8)
        for k, c in enumerate(comp):
            buf[k * slot:k * slot + len(c)] = np.frombuffer(c, dtype=np.uint8)
        return torch.from_numpy(buf).to(gpu), _u32([len(c) for c in comp], gpu)

    d_in, in_len = stage(sets[0][1])
    in_off = torch.arange(n, dtype=torch.int64, device=gpu) * slot
    size = torch.zeros(n, dtype=torch.int64, device=gpu)
    out_off = torch.zeros(n, dtype=torch.int64, device=gpu)
    out_cap = torch.zeros(n, dtype=torch.int32, device=gpu)
    total = torch.zeros(1, dtype=torch.int64, device=gpu)
    res = torch.zeros(n, dtype=torch.int64, device=gpu)
    d_out = torch.full((arena,), FILL, dtype=torch.uint8, device=gpu)

    def run():
        zl.batch_decompressed_size(d_in, in_off, in_len, size)
        zl.batch_plan_outputs(size, out_off, out_cap, total, 64)
        zl.batch_decompress_safe(d_in, in_off, in_len, d_out, out_off, out_cap, res)

    def collect():
        torch.cuda.synchronize()
        return (size.cpu().tolist(), out_off.cpu().tolist(), out_cap.cpu().tolist(), int(total.item()), res.cpu().tolist(),
                d_out.cpu().numpy().tobytes())

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    eager = {0: collect()}
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    for which in (1, 0, 1):
        plain, comp = sets[which]
        d2, l2 = stage(comp)
        d_in.copy_(d2)
        in_len.copy_(l2)
        if which not in eager:                                     # the eager calls on the fresh inputs
            d_out.fill_(FILL)
            run()
            eager[which] = collect()
        for t in (size, out_off, res):
            t.fill_(-999)
        d_out.fill_(FILL)
        g.replay()
        got = collect()
        assert got == eager[which], which
        sz, off, cap, tot, r, out = got
        assert tot <= arena
        for k, b in enumerate(plain):
            if k == 5 + which:
                assert sz[k] == ps.block_size(comp[k]) < 0 and cap[k] == 0 and r[k] == 0
            else:
                assert sz[k] == len(b) == r[k] and out[off[k]:off[k] + sz[k]] == b, (which, k)
