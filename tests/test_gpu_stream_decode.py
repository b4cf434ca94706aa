"""StreamDecode on the GPU (lz4.StreamDecode, src/lz4.zig:870-957): the single call and the whole-stream batch
(zlz4_batch_decompress_safe_continue) against tools/pyref/zig_lz4_stream_decode.py, replayed on the same device
addresses.  Every result, every successful slot and every final state is compared."""
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "pyref"))
import datagen as dg  # noqa: E402
import zig_lz4_stream_decode as psd  # noqa: E402
from stream_decode_harness import batch as _batch, ref_call as _ref_call  # noqa: E402

pytestmark = pytest.mark.gpu

def _pool(oracle, n, size, seed):
    blocks = []
    for i, d in enumerate(("text", "mixed", "zero", "random")):
        for b in dg.make_blocks(d, n // 4, size, seed=seed + i):
            blocks.append((bytes(b), oracle.compress_default(bytes(b))))
    return blocks


def test_single_call_reference_scenarios(zl, gpu, oracle):
    """test_streaming.zig:96-111 (two blocks through one StreamDecode) and test_dictionary.zig:38-75 (a dictionary
    pending, then plain), through zlz4_decompress_safe_continue on host buffers."""
    a = b"Hello streaming world! " * 20
    b = b"Second block of streaming data. " * 20
    sd = zl.StreamDecode.create()
    buf = np.zeros(4096, dtype=np.uint8)
    r1 = sd.decompressSafeContinue(oracle.compress_default(a), buf[:2048])
    assert bytes(buf[:r1]) == a and sd.prefixSize == r1 and sd.prefixEnd == buf.ctypes.data
    r2 = sd.decompressSafeContinue(oracle.compress_default(b), buf[2048:])
    assert bytes(buf[2048:2048 + r2]) == b and sd.prefixEnd == buf.ctypes.data + 2048
    zl.freeStreamDecode(sd)
    # a dictionary pending: the first call reads it, the second one does not
    dct = bytes(range(256)) * 64
    import dictgen
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        enc = dictgen.encoder(td)
        blk = dct[1000:3000] + b"tail"
        c, _ = enc(dct, blk)
    sd = zl.createStreamDecode()
    sd.setStreamDecode(bytearray(dct))
    out = np.zeros(8192, dtype=np.uint8)
    assert sd.decompressSafeContinue(c, out[:4096]) == len(blk) and bytes(out[:len(blk)]) == blk
    assert sd.extDictSize == 0 and sd.externalDict == 0
    with pytest.raises(zl.Lz4Error):                  # the dictionary is gone: the same block is corrupt now
        sd.decompressSafeContinue(c, out[4096:])
    # every single call equals the model on the same host addresses
    ref = psd.StreamDecode(sd.externalDict, sd.extDictSize, sd.prefixEnd, sd.prefixSize)
    for k, (src, cap, off) in enumerate([(oracle.compress_default(a), 600, 4096), (b"\x00", 10, 5000),
                                         (oracle.compress_default(b), 700, 100), (b"", 5, 7000)]):
        er, eb = ref.decompress_safe_continue(src, out.ctypes.data + off, cap)
        try:
            gr = sd.decompressSafeContinue(src, out[off:off + cap])
        except zl.Lz4Error as e:
            gr = e.code
        assert gr == er, k
        if er > 0:
            assert bytes(out[off:off + er]) == eb
        assert (sd.externalDict, sd.extDictSize, sd.prefixEnd, sd.prefixSize) == ref.state()


def _layout_runs(oracle, layout, nblk=6, size=3000, seed=1):
    data = [bytes(b) for b in dg.make_blocks("text", nblk, size, seed=seed)]
    comp = [oracle.compress_default(b) for b in data]
    cap = size
    if layout == "contiguous":
        offs = [i * cap for i in range(nblk)]
        total = nblk * cap
    elif layout == "double_up":
        offs = [(i % 2) * cap for i in range(nblk)]
        total = 2 * cap
    elif layout == "double_down":
        offs = [((i + 1) % 2) * cap for i in range(nblk)]
        total = 2 * cap
    else:                                             # ring of decoderRingBufferSize(size), through a wrap
        ring = psd.decoder_ring_buffer_size(size)
        offs, pos = [], 0
        for i in range(nblk):
            if pos + cap > ring:
                pos = 0
            offs.append(pos)
            pos += cap
        total = ring
        assert nblk >= ring // cap + 2
    return [[(comp[i], offs[i], cap) for i in range(nblk)]], total


@pytest.mark.parametrize("layout", ["contiguous", "double_up", "double_down", "ring"])
def test_buffer_layouts(zl, gpu, oracle, layout):
    """One stream through zlz4_decompress_safe_continue into a host buffer: contiguous, a double buffer in both orders,
    and a ring of decoderRingBufferSize bytes through a wrap (slots are reused, so these go through the single call)."""
    runs, total = _layout_runs(oracle, layout, nblk=24, size=4096)
    buf = np.zeros(total, dtype=np.uint8)
    sd, ref = zl.StreamDecode(), psd.StreamDecode()
    got = []
    for src, off, cap in runs[0]:
        er, eb = ref.decompress_safe_continue(src, buf.ctypes.data + off, cap)
        try:
            gr = sd.decompressSafeContinue(src, buf[off:off + cap])
        except zl.Lz4Error as e:
            gr = e.code
        assert gr == er
        if er > 0:
            assert bytes(buf[off:off + er]) == eb
        assert (sd.externalDict, sd.extDictSize, sd.prefixEnd, sd.prefixSize) == ref.state()
        got.append(gr)
    if layout == "contiguous":
        assert all(g > 0 for g in got)
    else:
        assert any(g == -3 for g in got), "the reference defect must show"


def _mixed_runs(oracle, pool, nruns, per_run, seed, dict_pool):
    rng = random.Random(seed)
    runs, dicts, pos = [], [], 0
    for s in range(nruns):
        kind = rng.random()
        calls, dct = [], None
        all_fail = kind < 0.05
        if 0.05 <= kind < 0.3:
            dct, dblocks = dict_pool[rng.randrange(len(dict_pool))]
        order = list(range(per_run))
        if rng.random() < 0.15:
            order.reverse()                           # slots placed downwards: the bound matters
        slots = []
        for j in range(per_run):
            raw, comp = pool[rng.randrange(len(pool))]
            cap = len(raw)
            u = rng.random()
            if all_fail:
                comp = comp[:-1] + b"\xff\xff" if len(comp) > 3 else b"\x1f"
            elif j == 0 and dct is not None:
                raw, comp = dblocks[rng.randrange(len(dblocks))]
                cap = len(raw)
            elif u < 0.04:
                comp = bytes([0x0F]) + comp[1:]       # corrupt token
            elif u < 0.08:
                cap = max(1, cap // 2)                # short capacity
            elif u < 0.11:
                comp = b""                            # zero result
            elif u < 0.13:
                cap = 0
            slots.append([comp, None, cap])
        for j in order:
            slots[j][1] = pos
            pos += max(slots[j][2], 1)
        runs.append([tuple(c) for c in slots])
        dicts.append(dct)
    return runs, dicts, pos


@pytest.fixture(scope="module")
def dict_pool(tmp_path_factory):
    import dictgen
    enc = dictgen.encoder(tmp_path_factory.mktemp("sdenc"))
    out = []
    for k in range(3):
        dct = bytes(b for b in dg.make_blocks("text", 1, 70000, seed=40 + k)[0])
        blocks = []
        for i in range(4):
            raw = dct[5000 + 900 * i:5000 + 900 * i + 700] + dct[60000 + 100 * i:60000 + 100 * i + 500]
            blocks.append((raw, enc(dct, raw)[0]))
        out.append((dct, blocks))
    return out


@pytest.mark.parametrize("nruns,per_run", [(4096, 16), (200, 16)])
def test_mixed_batch(zl, gpu, oracle, dict_pool, nruns, per_run):
    """About 4096 runs x 16 calls (lane-copy build) and 3200 calls (16-byte build): dictionary-first runs, plain runs,
    corrupt, short-capacity and zero-result calls at random positions, runs in which every call fails."""
    pool = _pool(oracle, 32, 1024, seed=7)
    runs, dicts, total = _mixed_runs(oracle, pool, nruns, per_run, seed=nruns, dict_pool=dict_pool)
    got, _ = _batch(zl, gpu, runs, total, dicts)
    assert sum(1 for g in got if g > 0) > len(got) // 2


def test_one_long_run(zl, gpu, oracle):
    """One run of 65 536 blocks, 1 % of them corrupt."""
    pool = _pool(oracle, 16, 512, seed=11)
    rng = random.Random(5)
    calls, pos = [], 0
    for j in range(65536):
        raw, comp = pool[rng.randrange(len(pool))]
        if rng.random() < 0.01:
            comp = bytes([0xF0]) + comp[1:]
        calls.append((comp, pos, len(raw)))
        pos += len(raw)
    got, _ = _batch(zl, gpu, [calls], pos)
    assert sum(1 for g in got if g < 0) > 100


def test_one_long_run_downwards(zl, gpu, oracle):
    """One run whose slots go downwards and whose calls alternate good and corrupt blocks: entry states depend on
    earlier results all the way (the serial walk)."""
    pool = _pool(oracle, 8, 512, seed=13)
    calls = []
    n = 3000
    for j in range(n):
        raw, comp = pool[j % len(pool)]
        if (j // 3) % 2:
            comp = bytes([0xF0]) + comp[1:]
        calls.append((comp, (n - 1 - j) * 512, 512))
    _batch(zl, gpu, [calls], n * 512)


def _chain_inputs(oracle, nstreams, steps, seed):
    pool = _pool(oracle, 16, 2048, seed=seed)
    rng = random.Random(seed)
    return [[pool[rng.randrange(len(pool))] for _ in range(nstreams)] for _ in range(steps)]


def _chain_tensors(gpu, step_blocks, nstreams, slot):
    import torch
    srcs = [c for _, c in step_blocks]
    offs = np.cumsum([0] + [len(s) for s in srcs])
    d_in = torch.from_numpy(np.frombuffer(b"".join(srcs), dtype=np.uint8).copy()).to(gpu)
    return (d_in, torch.tensor(offs[:-1], dtype=torch.int64, device=gpu),
            torch.tensor([len(s) for s in srcs], dtype=torch.int32, device=gpu))


@pytest.mark.parametrize("graph", [False, True])
def test_single_step_chain(zl, gpu, oracle, graph):
    """N one-call runs (run_start[s] = s) chained over 8 steps with the state kept on the device; the output of a step
    goes to the next slot of each stream's area.  With graph=True the 8 steps are captured once into a graph and
    replayed twice."""
    import torch
    ns, steps, slot = 512, 8, 2048
    inputs = _chain_inputs(oracle, ns, steps, seed=21)
    d_out = torch.zeros(ns * steps * slot, dtype=torch.uint8, device=gpu)
    base = d_out.data_ptr()
    staged = [_chain_tensors(gpu, inputs[t], ns, slot) for t in range(steps)]
    out_offs = [torch.tensor([(s * steps + t) * slot for s in range(ns)], dtype=torch.int64, device=gpu)
                for t in range(steps)]
    out_cap = torch.full((ns,), slot, dtype=torch.int32, device=gpu)
    run_start = torch.arange(ns + 1, dtype=torch.int32, device=gpu)
    state = torch.zeros((ns, 4), dtype=torch.int64, device=gpu)
    results = [torch.empty(ns, dtype=torch.int64, device=gpu) for _ in range(steps)]
    ws = torch.empty(zl.batch_decompress_safe_continue_workspace(ns, ns), dtype=torch.uint8, device=gpu)

    def run_all():
        for t in range(steps):
            d_in, in_off, in_len = staged[t]
            zl.batch_decompress_safe_continue(d_in, in_off, in_len, d_out, out_offs[t], out_cap, run_start, state,
                                              results[t], ws)

    def check(replays):
        refs = [psd.StreamDecode() for _ in range(ns)]
        for _ in range(replays):
            exp = [[_ref_call(refs[s], inputs[t][s][1], base + (s * steps + t) * slot, slot) for s in range(ns)]
                   for t in range(steps)]
        got = [r.cpu().tolist() for r in results]
        host = d_out.cpu().numpy().tobytes()
        fin = state.cpu().numpy().view(np.uint64)
        for s in range(ns):
            assert tuple(int(x) for x in fin[s]) == refs[s].state(), s
            for t in range(steps):
                assert got[t][s] == exp[t][s][0], (s, t)
                if exp[t][s][0] > 0:
                    o = (s * steps + t) * slot
                    assert host[o:o + exp[t][s][0]] == exp[t][s][1] == inputs[t][s][0]

    if not graph:
        run_all()
        torch.cuda.synchronize()
        check(1)
        return
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run_all()                                     # warm-up (and first pass of the state)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    state.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run_all()
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    check(2)


def test_invalid_and_empty_runs(zl, gpu, oracle):
    """A state holding a dictionary and a prefix: InvalidState for every call, state untouched; empty runs keep their
    state; a run that starts from a prefix above its slots."""
    pool = _pool(oracle, 4, 1024, seed=3)
    dct = bytes(range(256)) * 8
    runs = [[(pool[0][1], 0, 1024), (pool[1][1], 1024, 1024)], [], [(pool[2][1], 4096, 1024), (pool[3][1], 5120, 1024)]]
    states = [(0, len(dct), ("out", 8192), 10), None, (0, 0, ("out", 4096 + 100), 50)]
    got, fin = _batch(zl, gpu, runs, 16384, dicts=[dct, None, None], states=states)
    assert got[:2] == [-5, -5]
