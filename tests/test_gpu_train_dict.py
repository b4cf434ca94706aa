"""Dictionary training on the device (zlz4_batch_train_dict / zlz4_train_dict) against the model
(tools/pyref/zig_lz4_train_dict.py) on the corpus of tests/traingen.py: every case alone, all cases of a parameter set as one
batch, and the batch in the Packed layout; the refusals per group; the host call; and the loop the feature exists for."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "pyref"))
import datagen as dg  # noqa: E402
import gpu_harness as gh  # noqa: E402
import traingen as tg  # noqa: E402
import zig_lz4_train_dict as zt  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = tg.corpus()
SETS = tg.by_params(CASES)
SET_IDS = ["d%d_k%d_f%d" % key for key in SETS]


def _i32(values):
    return torch.from_numpy(np.asarray(values, dtype=np.uint32).view(np.int32).copy())


def run_batch(zl, dev, groups, caps, d, k, f, layout=None, first=None, max_cap=None, ws_total=None):
    """groups: lists of samples; one call of the raw batch wrapper -> [(result, dictionary bytes)].  Checks that the input,
    the guard bands and every slot byte behind the dictionary stay as they were."""
    samples = [bytes(s) for g in groups for s in g]
    if first is None:
        first = [0]
        for g in groups:
            first.append(first[-1] + len(g))
    buf, offs, lens = gh._pack(samples, layout=layout)
    slots = [min(int(c), 70000) for c in caps]         # (a refused capacity needs no slot of its size)
    out_offs, guard_ends, total = gh._out_slots(slots, layout)
    d_src = torch.from_numpy(buf).to(dev)
    d_out = torch.full((total,), 0xA5, dtype=torch.uint8, device=dev)
    ng = len(caps)                                     # (`first` may describe more groups than `groups` lists)
    res = torch.full((ng,), -999, dtype=torch.int64, device=dev)
    if max_cap is None:
        max_cap = max(slots) if slots else 0
    nbytes = sum(len(s) for s in samples) if ws_total is None else ws_total
    ws = torch.empty(max(16, zl.batch_train_dict_workspace(ng, nbytes, max_cap, d, k, f)), dtype=torch.uint8, device=dev)
    zl.batch_train_dict(d_src, torch.from_numpy(offs).to(dev), _i32(lens).to(dev), _i32(first).to(dev), d_out,
                        torch.from_numpy(out_offs).to(dev), _i32(caps).to(dev), res, max_cap, ws, d, k, f)
    torch.cuda.synchronize()
    assert (d_src.cpu().numpy() == buf).all(), "the samples changed"
    r, o = res.cpu().numpy(), d_out.cpu().numpy()
    outs = []
    for i in range(ng):
        n = int(r[i])
        L = max(n, 0)
        assert L <= slots[i], "group %d: a dictionary longer than its capacity" % i
        assert (o[out_offs[i] + L: guard_ends[i]] == 0xA5).all(), "group %d wrote behind its dictionary" % i
        outs.append((n, bytes(o[out_offs[i]: out_offs[i] + L])))
    if ng:
        assert (o[:out_offs[0]] == 0xA5).all(), "a group wrote before the first slot"
    return outs


def want(case):
    m = tg.model(case)
    return (m, b"") if isinstance(m, int) else (len(m), m)


@pytest.mark.parametrize("key", list(SETS), ids=SET_IDS)
def test_every_case_alone_equals_the_model(zl, gpu, key):
    for c in SETS[key]:
        assert run_batch(zl, gpu, [c.samples], [c.C], *key) == [want(c)], c.name


@pytest.mark.parametrize("key", list(SETS), ids=SET_IDS)
def test_all_cases_as_one_batch(zl, gpu, key):
    """mixed capacities, groups with no samples and groups that finish many steps before others, in one call"""
    cs = SETS[key]
    got = run_batch(zl, gpu, [c.samples for c in cs], [c.C for c in cs], *key)
    for c, g in zip(cs, got):
        assert g == want(c), c.name


@pytest.mark.parametrize("key", list(SETS), ids=SET_IDS)
@pytest.mark.parametrize("fill", ["zero", "cont"])
def test_packed_layout(zl, gpu, key, fill):
    """unaligned sample offsets with gaps between them, dictionary slots at odd offsets between guard bands"""
    cs = SETS[key]
    got = run_batch(zl, gpu, [c.samples for c in cs], [c.C for c in cs], *key, layout=gh.Packed(seed=len(cs), fill=fill))
    for c, g in zip(cs, got):
        assert g == want(c), c.name


def test_refusals_per_group(zl, gpu):
    """a refused group gets InvalidState and writes nothing; its neighbours get the model's answer"""
    by = {c.name: c for c in CASES}
    ok1, ok2 = by["C100"], by["one_epoch"]
    good = [want(ok1), want(ok2)]
    # a capacity above 65536, and one above the call's max_dict_cap
    got = run_batch(zl, gpu, [ok1.samples, ok1.samples, ok2.samples], [ok1.C, 65537, ok2.C], 4, 16, 12, max_cap=65536)
    assert got == [good[0], (zt.INVALID_STATE, b""), good[1]]
    got = run_batch(zl, gpu, [ok1.samples, ok1.samples, ok2.samples], [ok1.C, 101, ok2.C], 4, 16, 12, max_cap=100)
    assert got == [good[0], (zt.INVALID_STATE, b""), good[1]]
    # runs of samples that are none: a start behind its end, an end behind the last sample
    n1, n2 = len(ok1.samples), len(ok2.samples)
    got = run_batch(zl, gpu, [ok1.samples, ok2.samples], [ok1.C, 64, ok2.C], 4, 16, 12, first=[0, n1, n1 - 1, n1 + n2])
    assert got[0] == good[0] and got[1] == (zt.INVALID_STATE, b"")
    got = run_batch(zl, gpu, [ok1.samples, ok2.samples], [ok1.C, ok2.C], 4, 16, 12, first=[0, n1, n1 + n2 + 1])
    assert got == [good[0], (zt.INVALID_STATE, b"")]
    # more sample bytes than the workspace was sized for: the groups that still fit are served
    S1 = sum(len(s) for s in ok1.samples)
    got = run_batch(zl, gpu, [ok1.samples, ok2.samples], [ok1.C, ok2.C], 4, 16, 12, ws_total=S1)
    assert got == [good[0], (zt.INVALID_STATE, b"")]
    # more than 2^27 bytes in a group: samples may overlap, so two views of 64 MiB + 1 bytes do
    half = (1 << 26) + 1
    d_src = torch.zeros(half, dtype=torch.uint8, device=gpu)
    d_src[:100] = torch.from_numpy(np.frombuffer(b"".join(ok2.samples), dtype=np.uint8).copy()).to(gpu)
    d_out = torch.full((256,), 0xA5, dtype=torch.uint8, device=gpu)
    res = torch.full((2,), -999, dtype=torch.int64, device=gpu)
    ws = torch.empty(zl.batch_train_dict_workspace(2, 4096, 64, 4, 16, 12), dtype=torch.uint8, device=gpu)
    zl.batch_train_dict(d_src, torch.tensor([0, 0, 0], dtype=torch.int64, device=gpu), _i32([half, half, 100]).to(gpu),
                        _i32([0, 2, 3]).to(gpu), d_out, torch.tensor([0, 128], dtype=torch.int64, device=gpu),
                        _i32([64, 64]).to(gpu), res, 64, ws, 4, 16, 12)
    assert res.cpu().tolist() == [zt.INVALID_STATE, good[1][0]]
    o = d_out.cpu().numpy()
    assert (o[:128] == 0xA5).all() and bytes(o[128:192]) == good[1][1] and (o[192:] == 0xA5).all()
    # the whole call: a bad d, k or f launches nothing
    for bad in ((5, 16, 12), (4, 15, 12), (4, 1025, 12), (4, 16, 9), (4, 16, 25)):
        assert zl.batch_train_dict_workspace(1, 100, 64, *bad) == 0
        res.fill_(-999)
        with pytest.raises(zl.Lz4Error) as e:
            zl.batch_train_dict(d_src, torch.tensor([0], dtype=torch.int64, device=gpu), _i32([100]).to(gpu),
                                _i32([0, 1]).to(gpu), d_out, torch.tensor([0], dtype=torch.int64, device=gpu),
                                _i32([64]).to(gpu), res[:1], 64, ws, *bad)
        assert e.value.name == "InvalidState"
        assert res.cpu().tolist() == [-999, -999] and (d_out.cpu().numpy()[:128] == 0xA5).all()


def test_host_call_equals_the_batch(zl, gpu):
    names = ("C100", "tiny_samples_d8", "nd_mod_E", "all_equal", "step_limit", "S4_d4", "S3_d4", "C0", "grid_d6_k64_C2500",
             "f10_collisions")
    cs = [c for c in CASES if c.name in names]
    assert len(cs) == len(names)
    for c in cs:
        host = zl.trainDict(c.samples, c.C, c.d, c.k, c.f)
        assert host == tg.model(c), c.name
        assert zl.trainDicts([c.samples], c.C, c.d, c.k, c.f, device=gpu) == [host], c.name
    grp = [c for c in cs if (c.d, c.k, c.f) == (4, 16, 12)]
    assert zl.trainDicts([c.samples for c in grp], [c.C for c in grp], 4, 16, 12, device=gpu) == [tg.model(c) for c in grp]
    with pytest.raises(zl.Lz4Error) as e:
        zl.trainDict([b"x" * 100], 65537, 4, 16, 12)
    assert e.value.name == "InvalidState"
    assert zl.trainDicts([[b"x" * 100]], 65537, 4, 16, 12, device=gpu) == [zt.INVALID_STATE]


@pytest.fixture(scope="module")
def dtext():
    """the D-text setup: 256 KiB of samples in 4 KiB records, 64 held-out 1 KiB records"""
    samples = bytes(dg.text_bytes(256 << 10, 11))
    held = bytes(dg.text_bytes(64 << 10, 12))
    return ([samples[i:i + 4096] for i in range(0, len(samples), 4096)], samples,
            [held[i:i + 1024] for i in range(0, len(held), 1024)])


def test_train_compress_decompress_loop(zl, gpu, dtext):
    """train on the device; the trained dictionary beats the last C bytes of the samples, which beat no dictionary, with the
    device's own fast and HC streams; the streams decode to the records"""
    recs, samples, held = dtext
    trained = zl.trainDicts([recs], 4096, 6, 64, 20, device=gpu)[0]
    assert trained == zt.train(recs, 4096, 6, 64, 20) and len(trained) == 4096
    naive = samples[-4096:]
    for compress in (lambda d: zl.compressBlocksUsingDict(held, [d], [0] * len(held), device=gpu),
                     lambda d: zl.compressBlocksHCUsingDict(held, [d], [0] * len(held), level=9, device=gpu)):
        total = {}
        for name, d in (("none", b""), ("naive", naive), ("trained", trained)):
            streams = compress(d)
            assert all(isinstance(s, bytes) for s in streams)
            assert zl.decompressBlocks(streams, [d] * len(held), device=gpu) == held
            total[name] = sum(len(s) for s in streams)
        print("sizes", total)
        assert total["trained"] < total["naive"] < total["none"], total


def test_trained_dictionary_in_lz4_files(zl, gpu, dtext):
    recs, _, held = dtext
    trained = zl.trainDict(recs, 16384, 6, 64, 20)
    assert len(trained) == 16384
    items = [b"".join(held[:20]), held[21], b""]
    files = zl.lz4f.compressFiles(items, frame_size=4096, device=gpu, dicts=[trained])
    assert all(isinstance(x, bytes) for x in files)
    assert zl.lz4f.decompressFilesUsingDict(files, [trained], device=gpu) == items
    plain = zl.lz4f.compressFiles(items, frame_size=4096, device=gpu)
    assert sum(map(len, files)) < sum(map(len, plain))
