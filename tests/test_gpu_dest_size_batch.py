"""Batch compressDestSize (zlz4_batch_compress_dest_size) on the HIP path vs the oracle, block by block: result and
consumed equal oracle.compress_dest_size, the slot's first `result` bytes equal compressDefault of the consumed prefix
and decode back to it, bytes [result, cap) of the slot and the guard bands behind it keep their fill.  Run on the GPU
box: pytest -m gpu."""
import numpy as np
import pytest

import datagen as dg
import dsz_blocks
import gpu_harness as gh

pytestmark = pytest.mark.gpu

FILL = 0xA5
DISTS = ("text", "reptext", "mixed", "random", "zero", "ramp")
LENGTHS = (0, 1, 12, 13, 14, 15, 100, 4096, 65536)


def _caps(zl, n):
    b = zl.compressBound(n)
    return [0, 1, 2, 5, 13, 14, 100, 4096, n // 4, n // 2, n, b - 1, b, b + 7]


class Batch:
    """one batch call's tensors: inputs packed by gpu_harness (aligned, or gh.Packed), output slots with guard bands"""

    def __init__(self, zl, items, caps, dev, layout=None, max_in=None):
        import torch
        self.zl, self.items, self.caps, self.layout = zl, items, [int(c) for c in caps], layout
        self.buf, offs, lens = gh._pack(items, layout=layout)
        self.out_offs, self.guard_ends, total = gh._out_slots(self.caps, layout)
        self.d_in = torch.from_numpy(self.buf).to(dev)
        self.d_out = torch.full((total,), FILL, dtype=torch.uint8, device=dev)
        self.in_off = torch.from_numpy(offs).to(dev)
        self.in_len = torch.from_numpy(lens.astype(np.uint32).view(np.int32)).to(dev)
        self.out_off = torch.from_numpy(self.out_offs).to(dev)
        self.out_cap = torch.from_numpy(np.asarray(self.caps, dtype=np.uint32).view(np.int32)).to(dev)
        self.res = torch.full((len(items),), -999, dtype=torch.int64, device=dev)
        self.consumed = torch.full((len(items),), -1, dtype=torch.int32, device=dev)
        self.max_in = int(lens.max()) if max_in is None else max_in
        self.ws = torch.empty(max(16, zl.batch_compress_dest_size_workspace(len(items), self.max_in)), dtype=torch.uint8,
                              device=dev)

    def call(self, ws=None):
        self.zl.batch_compress_dest_size(self.d_in, self.in_off, self.in_len, self.d_out, self.out_off, self.out_cap,
                                         self.res, self.consumed, self.max_in, self.ws if ws is None else ws)

    def collect(self):
        """-> [(result, consumed, slot bytes)], checking the fill behind every result and the untouched input"""
        import torch
        torch.cuda.synchronize()
        assert (self.d_in.cpu().numpy() == self.buf).all(), "the input arena changed"
        r = self.res.cpu().numpy()
        c = self.consumed.cpu().numpy().view(np.uint32)
        o = self.d_out.cpu().numpy()
        out = []
        for i, cap in enumerate(self.caps):
            n = int(r[i])
            o0 = int(self.out_offs[i])
            written = max(n, 0)
            assert (o[o0 + written: self.guard_ends[i]] == FILL).all(), "block %d wrote past its result" % i
            out.append((n, int(c[i]), bytes(o[o0: o0 + written])))
        if self.caps:
            assert (o[:int(self.out_offs[0])] == FILL).all(), "a block wrote before the first slot"
        return out


def _check(oracle, items, caps, got):
    for i, (b, cap, (r, c, out)) in enumerate(zip(items, caps, got)):
        want_r, want_c = oracle.compress_dest_size(b, cap)
        assert (r, c) == (want_r, want_c), (i, len(b), cap)
        assert out == oracle.compress_default(b[:c], cap=cap), (i, len(b), cap)
        if c:
            assert oracle.decompress_safe(out, c) == b[:c], (i, len(b), cap)


def _grid(zl):
    items, caps = [], []
    for k, dist in enumerate(DISTS):
        for n in LENGTHS:
            b = bytes(dg.make_blocks(dist, 1, n, seed=100 + k)[0]) if n else b""
            for cap in _caps(zl, n):
                items.append(b)
                caps.append(cap)
    return items, caps


@pytest.mark.parametrize("layout", [None, gh.Packed(seed=5, fill="cont")], ids=["aligned", "packed"])
def test_grid(zl, oracle, gpu, layout):
    items, caps = _grid(zl)
    bt = Batch(zl, items, caps, gpu, layout=layout)
    bt.call()
    _check(oracle, items, caps, bt.collect())


@pytest.mark.parametrize("dist", ["text", "reptext"])
def test_every_cap(zl, oracle, gpu, dist):
    """every cap 0..bound+1 of one 3000-byte block: where the non-monotone caps live"""
    b = bytes(dg.make_blocks(dist, 1, 3000, seed=11)[0])
    caps = list(range(zl.compressBound(len(b)) + 2))
    items = [b] * len(caps)
    bt = Batch(zl, items, caps, gpu)
    bt.call()
    _check(oracle, items, caps, bt.collect())


def test_edge_literal_runs_on_every_cap(zl, oracle, gpu):
    """first literal runs of 32 q (q + 1) + 2 bytes (and their neighbours), where the step after the attempt that found
    the match grows: every cap 0..bound+1 of each block, in one batch"""
    items, caps = [], []
    for lit in dsz_blocks.EDGE_RUNS:
        b = dsz_blocks.block_with_first_run(oracle.compress_default, lit)
        for cap in range(zl.compressBound(len(b)) + 2):
            items.append(b)
            caps.append(cap)
    bt = Batch(zl, items, caps, gpu)
    bt.call()
    _check(oracle, items, caps, bt.collect())


def test_large_blocks(zl, oracle, gpu):
    """blocks past 64 KiB take the u32-table instantiation of the full-length compression and wider checkpoints"""
    items, caps = [], []
    for n, dist, seed in ((200000, "text", 1), (200000, "reptext", 2), (1 << 20, "text", 3), (1 << 20, "mixed", 4)):
        b = bytes(dg.make_blocks(dist, 1, n, seed=seed)[0])
        for cap in (n // 4, n // 2):
            items.append(b)
            caps.append(cap)
    bt = Batch(zl, items, caps, gpu)
    bt.call()
    _check(oracle, items, caps, bt.collect())


def test_many_blocks(zl, oracle, gpu):
    n = 8192
    data = dg.make_blocks("text", n, 4096, seed=21)
    items = [bytes(r) for r in data]
    rng = np.random.default_rng(7)
    caps = [int(x) for x in rng.integers(0, zl.compressBound(4096) + 8, size=n)]
    bt = Batch(zl, items, caps, gpu)
    bt.call()
    _check(oracle, items, caps, bt.collect())


def test_over_long_block_beside_valid_neighbours(zl, oracle, gpu):
    a = bytes(dg.make_blocks("text", 1, 5000, seed=1)[0])
    long = bytes(dg.make_blocks("text", 1, 9000, seed=2)[0])
    c = bytes(dg.make_blocks("reptext", 1, 6000, seed=3)[0])
    items, caps = [a, long, c], [1200, 2000, 1500]
    bt = Batch(zl, items, caps, gpu, max_in=6000)
    bt.call()
    got = bt.collect()
    assert got[1] == (-5, 0, b"")                                  # InvalidState, consumed 0, slot untouched
    _check(oracle, [a, c], [1200, 1500], [got[0], got[2]])


def test_workspace_too_small_launches_nothing(zl, gpu):
    import torch
    items = [bytes(dg.make_blocks("text", 1, 4096, seed=s)[0]) for s in range(4)]
    bt = Batch(zl, items, [1000] * 4, gpu)
    need = zl.batch_compress_dest_size_workspace(4, bt.max_in)
    for ws in (bt.ws[:need - 1], None):
        with pytest.raises(zl.Lz4Error) as e:
            zl.batch_compress_dest_size(bt.d_in, bt.in_off, bt.in_len, bt.d_out, bt.out_off, bt.out_cap, bt.res,
                                        bt.consumed, bt.max_in, ws)
        assert e.value.name == "InvalidState"
    torch.cuda.synchronize()
    assert bt.res.cpu().tolist() == [-999] * 4
    assert (bt.d_out.cpu().numpy() == FILL).all()


def test_captured_graph(zl, oracle, gpu):
    import torch
    items = [bytes(r) for r in dg.make_blocks("text", 64, 8192, seed=41)]
    caps = [1000 + 97 * k for k in range(64)]
    bt = Batch(zl, items, caps, gpu)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        bt.call()
    torch.cuda.current_stream().wait_stream(s)
    first = bt.collect()
    _check(oracle, items, caps, first)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        bt.call()
    bt.res.fill_(-999)
    bt.consumed.fill_(-1)
    bt.d_out.fill_(FILL)
    g.replay()
    assert bt.collect() == first


def test_single_call_equals_the_batch(zl, gpu):
    items, caps = _grid(zl)
    bt = Batch(zl, items, caps, gpu)
    bt.call()
    for b, cap, (r, c, out) in zip(items, caps, bt.collect()):
        assert zl.compressDestSize(b, cap) == (out, c), (len(b), cap)
        assert len(out) == r


def test_helper(zl, oracle, gpu):
    items = [bytes(dg.make_blocks(d, 1, 20000, seed=9)[0]) for d in DISTS]
    caps = [4096] * len(items)
    got = zl.compressDestSizeBatch(items, caps, device=gpu)
    for b, cap, (out, c) in zip(items, caps, got):
        r, want_c = oracle.compress_dest_size(b, cap)
        assert (len(out), c) == (r, want_c) and out == oracle.compress_default(b[:c])


def test_single_call_edge_literal_runs(zl, oracle, gpu):
    """the single call goes through the same kernel: every cap of the crafted blocks against the oracle"""
    for lit in dsz_blocks.EDGE_RUNS:
        b = dsz_blocks.block_with_first_run(oracle.compress_default, lit)
        for cap in range(zl.compressBound(len(b)) + 2):
            r, c = oracle.compress_dest_size(b, cap)
            assert zl.compressDestSize(b, cap) == (oracle.compress_default(b[:c]), c), (lit, cap)
            assert len(oracle.compress_default(b[:c])) == r
