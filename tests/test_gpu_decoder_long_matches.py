"""The block decoder on batched matches of more than 32 bytes (tests/longmatchgen.py): k_decompress_safe
(zig-lz4_amd/csrc/zlz4_decompress.hip) holds such a match in 16-byte pieces in the token's lane and the two lanes above
it (up to 96 bytes; longer ones keep a load -> store loop behind the pieces).

Cases: every length around a piece boundary (31 .. 97, 112, 273) at every window lane around a 16-lane row boundary
(0 .. 61), two long matches in neighbouring sequences, a long match beside matches the lane copy moves, in a second and a
third copy phase, with its source ending at / just before / one byte into the phase's first match, within the last
7100 bytes of the slot (the room-tested walk) and in its last 32; a damaged copy of every stream (one bit flipped, or
the end cut off).  A match of 19..273 bytes takes a 4-byte sequence, so the closest two long matches are four lanes
apart (t and t + 4; t, t + 3, t + 7 behind a 3-byte sequence) and lane 61 opens the next window.

Two batch sizes: >= 6144 blocks in one call (the lane-copy build) and calls of 64 (the sequence-lane build), through
decompress_safe, decompress_safe_using_dict (the source wholly in the dictionary, wholly in dst, across its end) and the
StreamDecode batch (kBound builds).  Bytes and status: oracle.decompress_safe; with a dictionary the generator's
plaintext, and the reference restatement (tools/pyref) for damaged streams; StreamDecode: the pyref replay."""
import random

import pytest

import longmatchgen as lg
from stream_decode_harness import batch
from test_gpu_decoder_sequences import FILL, LANE_COPY_MIN, _check, _decode, _expect

pytestmark = pytest.mark.gpu
SMALL = 64                                           # blocks per call of the sequence-lane build


@pytest.fixture(scope="module")
def corpus():
    return lg.corpus()


@pytest.fixture(scope="module")
def want(oracle, corpus):
    w = [oracle.decompress_safe(it.src, it.cap) for it in corpus]
    for it, x in zip(corpus, w):
        assert it.plain is None or x == it.expected(), "%s: the oracle and the generator disagree" % it.name
    assert sum(1 for it, x in zip(corpus, w) if it.plain is None and isinstance(x, int)) > 300
    assert sum(1 for it, x in zip(corpus, w) if it.plain is None and not isinstance(x, int)) > 300
    return w


@pytest.fixture(scope="module")
def dict_corpus():
    return lg.dict_corpus()


@pytest.fixture(scope="module")
def dict_want(dict_corpus):
    return _expect(None, dict_corpus)


def test_long_matches_lane_copy_build(zl, gpu, corpus, want):
    """the whole corpus in one call: k_decompress_safe<true, true>"""
    assert len(corpus) >= LANE_COPY_MIN
    _check(corpus, want, _decode(zl, gpu, corpus))


def test_long_matches_sequence_lane_build(zl, gpu, corpus, want):
    """the same corpus in calls of 64 blocks: k_decompress_safe<true, false>"""
    for k in range(0, len(corpus), SMALL):
        _check(corpus[k:k + SMALL], want[k:k + SMALL], _decode(zl, gpu, corpus[k:k + SMALL]))


def test_long_matches_using_dict_lane_copy_build(zl, gpu, dict_corpus, dict_want):
    assert len(dict_corpus) >= LANE_COPY_MIN
    _check(dict_corpus, dict_want, _decode(zl, gpu, dict_corpus))


def test_long_matches_using_dict_sequence_lane_build(zl, gpu, dict_corpus, dict_want):
    """every stream once at its roomy capacity and once at capacity n, and every damaged copy, in calls of 64 blocks"""
    pick = [k for k, it in enumerate(dict_corpus)
            if it.plain is None or it.cap in (len(it.plain), len(it.plain) + lg.ROOMY)]
    assert len(pick) >= 3 * len(lg.dict_streams(11))
    for j in range(0, len(pick), SMALL):
        items = [dict_corpus[k] for k in pick[j:j + SMALL]]
        _check(items, [dict_want[k] for k in pick[j:j + SMALL]], _decode(zl, gpu, items))


def _runs(corpus, nruns, per_run, seed):
    """runs of StreamDecode calls on one output buffer: a call's slot ends with its plaintext (the next call continues
    it), 33 bytes later, or lg.ROOMY bytes later (the walk without its room test); one call in 20 is a damaged stream"""
    rng = random.Random(seed)
    pool = [it for it in corpus if it.plain is not None and it.cap == len(it.plain)]
    bad = [it for it in corpus if it.plain is None][:60]
    templates = []
    for _ in range(24):
        t = []
        for j in range(per_run):
            it = bad[rng.randrange(len(bad))] if rng.random() < 0.05 else pool[rng.randrange(len(pool))]
            t.append((it.src, len(it.plain) + (0, 33, lg.ROOMY)[j % 3] if it.plain else 2048))
        templates.append(t)
    runs, base = [], 0
    for s in range(nruns):
        calls, pos = [], 0
        for src, cap in templates[s % len(templates)]:
            calls.append((src, base + pos, cap))
            pos += cap
        runs.append(calls)
        base += pos + 64                               # (a guard band after every run's area)
    return runs, base


@pytest.mark.parametrize("nruns", [400, 4])
def test_long_matches_stream_decode_batch(zl, gpu, corpus, nruns):
    """zlz4_batch_decompress_safe_continue on 6400 calls (lane-copy kBound builds) and on 64 (sequence-lane kBound builds)"""
    runs, total = _runs(corpus, nruns, 16, seed=5)
    assert (sum(len(r) for r in runs) >= LANE_COPY_MIN) == (nruns == 400)
    got, _ = batch(zl, gpu, runs, total, fill=FILL)
    assert sum(1 for g in got if g > 0) > len(got) // 2
