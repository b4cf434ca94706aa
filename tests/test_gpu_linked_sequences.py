"""The crafted frame corpus of tests/linkedseqgen.py on the HIP path: the serial wave decoder (decode_block_wave behind
k_bfl_decode, zig-lz4_amd/csrc/zlz4_device.hpp and zlz4_frame_linked.hip) through the linked and the dictionary frame
calls, decode and size query, byte for byte against the generator's own plaintext and status for status against the CPU
models (held against each other and against liblz4 in tests/test_linked_sequence_corpus_cpu.py).  Every destination slot
is fenced by guard bytes (the helpers of test_gpu_linked_frame.py / test_gpu_dict_frame.py check them on every call,
failed frames included), and a failed slot's bytes are never read.  Run on the GPU box: pytest -m gpu."""
import pytest

import linkedseqgen as lsg
import test_gpu_dict_frame as td
import test_gpu_linked_frame as tl
from test_linked_sequence_corpus_cpu import pyref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def corpus():
    """[(item, ((result, bytes), size) of the CPU model)], computed once"""
    return [(it, pyref(it)) for it in lsg.corpus()]


def _dict_table(sel):
    """the distinct dictionaries of a selection (one arena) and each frame's index into them"""
    dicts, idx = [], []
    for it, _ in sel:
        k = next((j for j, d in enumerate(dicts) if d is it.dict_bytes), None)
        if k is None:
            k = len(dicts)
            dicts.append(it.dict_bytes)
        idx.append(k)
    return dicts, idx


def _judge(sel, res, outs, sizes):
    bad = []
    for k, (it, ((want, want_bytes), want_size)) in enumerate(sel):
        if res[k] != want or (want >= 0 and outs[k] != want_bytes):
            bad.append(("model", it.name, res[k], want))
        plain = it.expected()
        if plain is not None and (res[k] != len(plain) or outs[k] != plain):
            bad.append(("plaintext", it.name, res[k], len(plain)))
        if it.status is not None and res[k] != it.status:
            bad.append(("status", it.name, res[k], it.status))
        if sizes[k] != want_size:
            bad.append(("size", it.name, sizes[k], want_size))
    assert not bad, (len(bad), bad[:8])


def _run_linked(zl, gpu, sel):
    frames, caps = [it.frame for it, _ in sel], [it.cap for it, _ in sel]
    res, outs = tl._decompress(zl, gpu, frames, caps, zl.lz4f.DECODE_LINKED)
    sizes = tl._sizes(zl, gpu, frames, zl.lz4f.DECODE_LINKED)
    _judge(sel, res, outs, sizes)
    return res, outs


def _run_dict(zl, gpu, sel):
    frames, caps = [it.frame for it, _ in sel], [it.cap for it, _ in sel]
    dicts, idx = _dict_table(sel)
    res, outs = td._decompress(zl, gpu, frames, caps, dicts, idx)
    sizes = td._sizes(zl, gpu, frames, dicts, idx)
    _judge(sel, res, outs, sizes)
    return res, outs


def _linked(corpus):
    return [c for c in corpus if c[0].dict_bytes is None]


def _with_dict(corpus):
    return [c for c in corpus if c[0].dict_bytes is not None]


# ------------------------------------------------------------------ the whole corpus, one call each
def test_plain_linked_corpus_in_one_batch(zl, gpu, corpus):
    """every plain item in one decompressFrameBatch(DECODE_LINKED) and one frameDecompressedSizeBatch; the frames that
    declare independent blocks ride along, so k_bfl_mask and the parallel decode run in the same call"""
    sel = _linked(corpus)
    assert sum(it.family == "independent" for it, _ in sel) >= 4
    assert sum(it.family == "damaged" for it, _ in sel) > 50
    res, _ = _run_linked(zl, gpu, sel)
    assert sum(r >= 0 for r in res) > len(res) // 2 and sum(r < 0 for r in res) > 20


def test_dictionary_corpus_in_one_batch(zl, gpu, corpus):
    """every dictionary item, the multi-block frames (serial) and their one-block twins (parallel) in the same call, the
    dictionaries in one arena chosen by dict_idx; a twin's bytes are a prefix of its frame's"""
    sel = _with_dict(corpus)
    assert len(_dict_table(sel)[0]) >= 5
    res, outs = _run_dict(zl, gpu, sel)
    at = {it.name: k for k, (it, _) in enumerate(sel)}
    twins = 0
    for k, (it, _) in enumerate(sel):
        if it.twin_of is not None and res[k] >= 0 and res[at[it.twin_of]] >= 0:
            assert outs[at[it.twin_of]].startswith(outs[k]), it.name
            twins += 1
    assert twins > 250


def test_hist_pairs_give_the_statuses_the_generator_states(zl, gpu, corpus):
    """accepted = n, refused = -116, exactly at the history bound (this pins the model as well)"""
    hist = [c for c in corpus if c[0].family == "hist"]
    for it, ((want, _), _) in hist:
        assert it.status is not None and it.status == want, it.name
        assert it.status == (-116 if it.plain is None else len(it.plain)), it.name
    assert sum(it.status == -116 for it, _ in hist) >= 6 and sum(it.status >= 0 for it, _ in hist) >= 10
    res, _ = _run_linked(zl, gpu, _linked(hist))
    assert res == [it.status for it, _ in _linked(hist)]
    sel = _with_dict(hist)
    res, _ = _run_dict(zl, gpu, sel)
    assert res == [it.status for it, _ in sel]
    dicts, idx = _dict_table(sel)                                      # and through the dictionary file's own check
    assert td._check_against_model(zl, gpu, [it.frame for it, _ in sel], [it.cap for it, _ in sel], dicts, idx) == res


# ------------------------------------------------------------------ the batch shape: four frames per workgroup
@pytest.mark.parametrize("n", [1, 3, 5])
def test_calls_of_one_three_and_five_frames(zl, gpu, corpus, n):
    """k_bfl_decode runs four frames per workgroup: the same corpora in calls that fill part of one, and one and a part
    (the frames past 64 KiB have test_slide_frames_in_calls_of_their_own)"""
    sel = [c for c in _linked(corpus) if c[0].family != "slide"]
    for k in range(0, len(sel), n):
        part = sel[k:k + n]
        res, _ = tl._check_against_model(zl, gpu, [it.frame for it, _ in part], [it.cap for it, _ in part],
                                         model=[m for _, m in part])
        assert all(it.status is None or it.status == r for (it, _), r in zip(part, res))
    sel = [c for c in _with_dict(corpus) if c[0].family != "slide"]
    for k in range(0, len(sel), n):
        _run_dict(zl, gpu, sel[k:k + n])


def test_slide_frames_in_calls_of_their_own(zl, gpu, corpus):
    slide = [c for c in corpus if c[0].family == "slide"]
    assert len(slide) >= 4
    for c in slide:
        (_run_linked if c[0].dict_bytes is None else _run_dict)(zl, gpu, [c])


# ------------------------------------------------------------------ the single-frame host calls
def test_single_frame_calls(zl, corpus):
    """one valid base frame per family through decompressFrame / frameDecompressedSize(DECODE_LINKED) and through
    decompressFrameUsingDict / frameDecompressedSizeUsingDict, and one refused frame each"""
    L = zl.lz4f.DECODE_LINKED
    seen = set()
    for it, _ in corpus:
        key = (it.family, it.dict_bytes is None, it.plain is None)
        if it.seqs is None or key in seen or (it.plain is None and it.family != "hist"):
            continue
        seen.add(key)
        if it.plain is None:
            with pytest.raises(zl.Lz4Error) as e:
                if it.dict_bytes is None:
                    zl.lz4f.decompressFrame(it.frame, it.cap, L)
                else:
                    zl.lz4f.decompressFrameUsingDict(it.frame, it.cap, it.dict_bytes)
            assert e.value.code == -116, it.name
        elif it.dict_bytes is None:
            assert zl.lz4f.decompressFrame(it.frame, it.cap, L) == it.plain, it.name
            assert zl.lz4f.frameDecompressedSize(it.frame, L) == len(it.plain), it.name
        else:
            assert zl.lz4f.decompressFrameUsingDict(it.frame, it.cap, it.dict_bytes) == it.plain, it.name
            assert zl.lz4f.frameDecompressedSizeUsingDict(it.frame, len(it.dict_bytes)) == len(it.plain), it.name
    assert len(seen) >= 11, sorted(seen)
