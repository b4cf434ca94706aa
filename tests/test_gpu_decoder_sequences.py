"""The block decoder on crafted sequence streams (tests/seqgen.py): streams no compressor of this project writes, each
family aimed at one branch of the batch path of k_decompress_safe (zig-lz4_amd/csrc/zlz4_decompress.hip) -- the cut
after the 16th short match, later copy phases up to their limit, the room-limited walk, self-overlap right after a
batch, the edge values of every length field, streams of 66..70 bytes, malformed sequences inside a window.

Every build the public calls choose runs: the lane-copy build with phases (one call of >= 6144 blocks), the
sequence-lane build (calls of fewer), the dictionary builds, the size pass of the frame decoder's exact plan and the
StreamDecode (kBound) builds.  Expected: the generator's own plaintext for valid streams, the reference restatements for
malformed ones.  On success the slot's bytes in [result, cap) must still hold the fill: the reference writes only
dst[0 .. result).  (tests/test_gpu_lane_decoder.py runs this file again under the tuning knobs.)"""
import os
import random
import sys

import numpy as np
import pytest

import gpu_harness as gh
import seqgen as sg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "pyref"))
import zig_lz4_dict as pdict  # noqa: E402
import zig_lz4_stream_decode as psd  # noqa: E402

pytestmark = pytest.mark.gpu
FILL = 0xA5
# the one-lane-per-block kernel (ZLZ4_DECOMP_LANE_MIN=1, tuning build) may copy up to 15 bytes past a literal run or a
# match, inside the capacity (its comment in zlz4_decompress.hip): only there is [result, cap) left unchecked
LANE_KERNEL = os.environ.get("ZLZ4_DECOMP_LANE_MIN") == "1"
LANE_COPY_MIN = 6144                                 # kLaneCopyMinBlocks


@pytest.fixture(scope="module")
def corpus():
    return sg.corpus()


def _expect(oracle, items):
    out = []
    for it in items:
        w = it.expected()
        if w is None:
            if it.dict_bytes is None:
                w = oracle.decompress_safe(it.src, it.cap)
            else:
                r, b = pdict.decompress_safe_using_dict(it.src, it.cap, it.dict_bytes)
                w = b if r >= 0 else r
        out.append(w)
    return out


def _decode(zl, gpu, items, layout=None):
    """one batch call (zlz4_batch_decompress_safe, or _using_dict when the items carry dictionaries) -> the results and
    the whole output arena, slots filled with FILL beforehand"""
    import torch
    buf, offs, lens = gh._pack([it.src for it in items], layout=layout)
    caps = np.array([it.cap for it in items], dtype=np.int64)
    out_offs, guard_ends, total = gh._out_slots(caps, layout)
    d_in = torch.from_numpy(buf).to(gpu)
    d_out = torch.full((total,), FILL, dtype=torch.uint8, device=gpu)
    res = torch.full((len(items),), -999, dtype=torch.int64, device=gpu)
    u32 = lambda a: torch.from_numpy(np.asarray(a).astype(np.uint32).view(np.int32)).to(gpu)
    args = (d_in, torch.from_numpy(offs).to(gpu), u32(lens), d_out, torch.from_numpy(out_offs).to(gpu), u32(caps))
    if items[0].dict_bytes is None:
        zl.batch_decompress_safe(*args, res)
    else:
        dicts = list({id(it.dict_bytes): it.dict_bytes for it in items}.values())
        index = {id(d): k for k, d in enumerate(dicts)}
        dbuf, doffs, dlens = gh._pack(dicts, layout=layout)
        idx = np.array([index[id(it.dict_bytes)] for it in items], dtype=np.int64)
        d_dict = torch.from_numpy(dbuf).to(gpu)
        zl.batch_decompress_safe_using_dict(*args, d_dict, torch.from_numpy(doffs[idx]).to(gpu), u32(dlens[idx]), res)
        torch.cuda.synchronize()
        assert (d_dict.cpu().numpy() == dbuf).all(), "the dictionary arena changed"
    torch.cuda.synchronize()
    assert (d_in.cpu().numpy() == buf).all(), "the input arena changed"
    return res.cpu().numpy(), d_out.cpu().numpy(), out_offs, guard_ends


def _check(items, want, got):
    r, o, out_offs, guard_ends = got
    bad = []
    for i, (it, w) in enumerate(zip(items, want)):
        n, s, cap = int(r[i]), int(out_offs[i]), it.cap
        if not (o[s + cap:guard_ends[i]] == FILL).all():
            bad.append("%d %s: wrote past its capacity" % (i, it.name))
        if isinstance(w, int):
            if n != w:
                bad.append("%d %s cap %d: status %d, expected %d" % (i, it.name, cap, n, w))
            continue
        if n != len(w) or o[s:s + n].tobytes() != w:
            bad.append("%d %s cap %d: result %d, expected %d bytes" % (i, it.name, cap, n, len(w)))
        elif not LANE_KERNEL and not (o[s + n:s + cap] == FILL).all():
            first = n + int(np.argmax(o[s + n:s + cap] != FILL))
            bad.append("%d %s: wrote [result, cap) at %d (result %d, cap %d)" % (i, it.name, first, n, cap))
    assert (o[:out_offs[0]] == FILL).all(), "a block wrote before the first slot"
    assert not bad, "%d/%d: %s" % (len(bad), len(items), "; ".join(bad[:8]))


# ------------------------------------------------------------------ the shipped library, every build of the plain call
def test_crafted_decompress_one_call_lane_copy_build(zl, oracle, gpu, corpus):
    """the whole corpus in ONE call: >= 6144 blocks, k_decompress_safe<true, true> (lane copy + phases)"""
    assert len(corpus) >= LANE_COPY_MIN
    _check(corpus, _expect(oracle, corpus), _decode(zl, gpu, corpus))


def test_crafted_decompress_sequence_lane_build(zl, oracle, gpu, corpus):
    """the same corpus in calls of fewer than 6144 blocks: k_decompress_safe<true, false> (16 bytes per sequence lane)"""
    want = _expect(oracle, corpus)
    step = 2900
    for k in range(0, len(corpus), step):
        _check(corpus[k:k + step], want[k:k + step], _decode(zl, gpu, corpus[k:k + step]))


def test_crafted_decompress_packed_layout(zl, oracle, gpu, corpus):
    """unaligned streams whose gaps continue the stream before them, odd output slots (gpu_harness.Packed)"""
    layout = gh.Packed(seed=9, fill="cont", gaps=(0, 5))
    _check(corpus, _expect(oracle, corpus), _decode(zl, gpu, corpus, layout))


# ------------------------------------------------------------------ the dictionary decoder
@pytest.mark.parametrize("nblocks", [300, 7000])
def test_crafted_decompress_using_dict(zl, gpu, nblocks):
    """matches into the dictionary's first byte, matches that end exactly at its end (and one byte before / after) and
    matches that span it, at 300 blocks (sequence-lane dict build) and 7000 (lane-copy dict build)"""
    items = sg.dict_corpus(seed=nblocks, count=nblocks)
    want = _expect(None, items)
    assert sum(1 for it in items if it.plain is None) >= nblocks // 20
    _check(items, want, _decode(zl, gpu, items))


# ------------------------------------------------------------------ frames: the exact plan and its size pass
def test_crafted_decompress_frames(zl, oracle, gpu, corpus):
    """crafted blocks wrapped into lz4f frames: every non-last block decodes short of the 64 KiB block size, so the
    frame decoder takes its exact plan and runs the size pass k_decompress_safe<false, false>"""
    from test_gpu_frame_batch import _header
    rng = random.Random(31)
    valid = [it for it in corpus if it.plain is not None and it.cap == len(it.plain) and len(it.plain) <= 65536]
    bad = [it for it in corpus if it.plain is None]
    frames, caps = [], []
    for k in range(700):
        cc = k % 2
        flg = 0x60 | (0x04 if cc else 0)
        body, content = b"", b""
        for j in range(rng.randint(2, 6)):
            it = bad[rng.randrange(len(bad))] if k % 10 == 9 and j == 1 else valid[rng.randrange(len(valid))]
            body += len(it.src).to_bytes(4, "little") + it.src
            content += it.plain or b""
        f = _header(oracle, flg, 0x40) + body + b"\0\0\0\0" + (oracle.xxh32(content).to_bytes(4, "little") if cc else b"")
        for cap in (len(content), len(content) - 1, len(content) + 40):
            frames.append(f)
            caps.append(max(0, cap))
    res = _decode_frames(zl, oracle, gpu, frames, caps)
    assert sum(1 for r in res if r > 0) > len(res) // 2 and any(r < 0 for r in res)


def _decode_frames(zl, oracle, gpu, frames, caps):
    """zlz4f_batch_decompress_frame on slots filled with test_gpu_frame_batch's FILL (its staging): status and bytes equal
    oracle.decompress_frame, nothing outside the slots changes, and on success [result, cap) keeps its fill"""
    import torch
    from test_gpu_frame_batch import FILL as SLOT_FILL, _slots, _stage
    d_src, s_off, s_len = _stage(frames, gpu)
    d_dst, offs, t_off, t_cap = _slots(caps, gpu)
    result = torch.full((len(frames),), -999, dtype=torch.int64, device=gpu)
    zl.lz4f.decompressFrameBatch(d_src, s_off, s_len, d_dst, t_off, t_cap, result,
                                 sum(zl._chain_blocks(f) for f in frames))
    res = result.cpu().tolist()
    host = d_dst.cpu().numpy()
    may_write = np.zeros(len(host), dtype=bool)
    bad = []
    for k, (f, cap, o, r) in enumerate(zip(frames, caps, offs, res)):
        want = oracle.decompress_frame(f, cap)
        if isinstance(want, int):
            may_write[o:o + cap] = True           # (dst after an error is unspecified)
            if r != want:
                bad.append("frame %d cap %d: status %d, expected %d" % (k, cap, r, want))
        elif r != len(want) or host[o:o + r].tobytes() != want:
            bad.append("frame %d cap %d: result %d, expected %d bytes" % (k, cap, r, len(want)))
        else:
            may_write[o:o + r] = True
    assert (host[~may_write] == SLOT_FILL).all(), "a frame wrote outside dst[0 .. result) or outside its slot"
    assert not bad, "%d/%d: %s" % (len(bad), len(frames), "; ".join(bad[:8]))
    return res


# ------------------------------------------------------------------ StreamDecode (kBound builds)
def _stream_runs(corpus, layout, nruns, per_run, seed):
    rng = random.Random(seed)
    pool = [it for it in corpus if it.plain is not None and it.cap == len(it.plain) and 1500 <= len(it.plain) <= 6000]
    bad = [it for it in corpus if it.plain is None][:40]
    templates = []
    for _ in range(24):
        t = []
        for j in range(per_run):
            it = bad[rng.randrange(len(bad))] if rng.random() < 0.05 else pool[rng.randrange(len(pool))]
            # every third slot has room to spare: [result, cap) must keep its fill
            t.append((it.src, len(it.plain) + (33 if j % 3 == 1 else 0) if it.plain else 4096))
        templates.append(t)
    ring = psd.decoder_ring_buffer_size(max(c for t in templates for _, c in t))
    runs, base = [], 0
    for s in range(nruns):
        t = templates[s % len(templates)]
        # a run starts 16 KiB in front of its ring's end and wraps once; the batch is checked after it has run, so no
        # slot may be used twice
        assert sum(c for _, c in t) + 16384 < ring
        calls, pos = [], ring - 16384 if layout == "ring" else 0
        for src, cap in t:
            if layout == "ring" and pos + cap > ring:
                pos = 0                               # the ring wraps
            calls.append((src, base + pos, cap))
            pos += cap
        runs.append(calls)
        base += (ring if layout == "ring" else pos) + 64     # (a guard band after every run's area)
    return runs, base


@pytest.mark.parametrize("layout", ["contiguous", "ring"])
def test_crafted_stream_decode_batch(zl, gpu, corpus, layout):
    """runs of crafted blocks through zlz4_batch_decompress_safe_continue, >= 6144 calls in the batch (lane-copy kBound
    build), against the pyref replay of the same calls on the same addresses; no byte outside dst[0 .. result) of a
    successful call (or the slot of a failed one) may change"""
    from stream_decode_harness import batch
    runs, total = _stream_runs(corpus, layout, nruns=400, per_run=16, seed=len(layout))
    assert sum(len(r) for r in runs) >= LANE_COPY_MIN
    got, _ = batch(zl, gpu, runs, total, fill=FILL)
    # (after the ring wraps, the reference rejects every match below the previous block: most calls fail there)
    assert sum(1 for g in got if g > 0) > len(got) // (2 if layout == "contiguous" else 4) and any(g < 0 for g in got)
