"""The StreamDecode batch check shared by the GPU tests (tests/test_gpu_stream_decode.py,
tests/test_gpu_decoder_sequences.py): zlz4_batch_decompress_safe_continue on one batch, replayed call by call through
tools/pyref/zig_lz4_stream_decode.py on the same device addresses."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tools", "pyref") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools", "pyref"))
import zig_lz4_stream_decode as psd  # noqa: E402

_CACHE = {}


def ref_call(sd, src, dst, cap):
    """psd.StreamDecode.decompress_safe_continue with the decode memoised on (src, cap, kind)."""
    k = sd.kind(dst)
    key = (src, cap, k if k[0] != "dict" else ("dict", sd.dict_bytes[:sd.dict_len]))
    if k[0] in ("A", "dict", "bound") and key in _CACHE:
        r, out = _CACHE[key]
        if k[0] == "A":
            if r >= 0:
                sd.prefix, sd.prefix_len = dst, r
        elif r >= 0:
            sd.prefix, sd.prefix_len, sd.dict, sd.dict_len, sd.dict_bytes = dst, r, 0, 0, None
        return r, out
    r, out = sd.decompress_safe_continue(src, dst, cap)
    _CACHE[key] = (r, out)
    return r, out


def batch(zl, gpu, runs, out_bytes, dicts=None, states=None, fill=None):
    """runs: list of lists of (src, out_off, cap); dicts[s]: bytes or None; states[s]: (dict, dict_len, prefix,
    prefix_len) relative to the output buffer (prefix = ("out", off)) -- None = init.  Runs the batch once and checks
    everything against the reference replay.  Returns (results, final states).
    fill: the output buffer starts as this byte (else zeros), and every byte that no call may write must still hold it
    afterwards -- everything but the slots of failed calls and dst[0 .. result) of successful ones (slots must not
    overlap then)."""
    import torch
    calls = [c for r in runs for c in r]
    n, ns = len(calls), len(runs)
    srcs = [c[0] for c in calls]
    d_out = torch.full((max(1, out_bytes),), 0 if fill is None else fill, dtype=torch.uint8, device=gpu)
    base = d_out.data_ptr()
    offs = np.cumsum([0] + [len(s) for s in srcs])
    d_in = torch.from_numpy(np.frombuffer(b"".join(srcs) + b"\0", dtype=np.uint8).copy()).to(gpu)
    in_off = torch.tensor(offs[:-1], dtype=torch.int64, device=gpu)
    in_len = torch.tensor([len(s) for s in srcs], dtype=torch.int32, device=gpu)
    out_off = torch.tensor([c[1] for c in calls], dtype=torch.int64, device=gpu)
    out_cap = torch.tensor([c[2] for c in calls], dtype=torch.int32, device=gpu)
    rs = np.cumsum([0] + [len(r) for r in runs]).astype(np.int32)
    run_start = torch.from_numpy(rs).to(gpu)
    dicts = dicts or [None] * ns
    dall = b"".join(d or b"" for d in dicts) + b"\0"
    d_dict = torch.from_numpy(np.frombuffer(dall, dtype=np.uint8).copy()).to(gpu)
    doff = np.cumsum([0] + [len(d or b"") for d in dicts])
    st0, refs = np.zeros((ns, 4), dtype=np.uint64), []
    for s in range(ns):
        sd = psd.StreamDecode()
        if states and states[s] is not None:
            dct, dl, pre, pl = states[s]
            pre = base + pre[1] if isinstance(pre, tuple) else pre
            sd = psd.StreamDecode(0, dl, pre, pl)
            if dicts[s] is not None:
                sd.dict, sd.dict_bytes = d_dict.data_ptr() + int(doff[s]), dicts[s]
        elif dicts[s] is not None:
            sd.set_stream_decode(d_dict.data_ptr() + int(doff[s]), dicts[s])
        st0[s] = sd.state()
        refs.append(sd)
    state = torch.from_numpy(st0.view(np.int64).copy()).to(gpu)
    result = torch.full((max(1, n),), -99, dtype=torch.int64, device=gpu)
    ws = torch.empty(max(16, zl.batch_decompress_safe_continue_workspace(n, ns)), dtype=torch.uint8, device=gpu)
    zl.batch_decompress_safe_continue(d_in, in_off, in_len, d_out, out_off, out_cap, run_start, state, result[:n] if n else result[:0], ws)
    torch.cuda.synchronize()
    got = result[:n].cpu().tolist()
    host = d_out.cpu().numpy().tobytes()
    fin = state.cpu().numpy().view(np.uint64)
    may_write = np.zeros(max(1, out_bytes), dtype=bool)
    i = 0
    for s, r in enumerate(runs):
        for src, off, cap in r:
            er, eb = ref_call(refs[s], src, base + off, cap)
            assert got[i] == er, "run %d call %d: %d != %d" % (s, i - rs[s], got[i], er)
            if er > 0:
                assert host[off:off + er] == eb, "run %d call %d: bytes differ" % (s, i - rs[s])
            may_write[off:off + (er if er >= 0 else cap)] = True
            i += 1
        assert tuple(int(x) for x in fin[s]) == refs[s].state(), "run %d final state" % s
    if fill is not None:
        untouched = np.frombuffer(host, dtype=np.uint8)[~may_write]
        assert (untouched == fill).all(), "a call wrote outside dst[0 .. result) (%d bytes)" % int((untouched != fill).sum())
    return got, fin
