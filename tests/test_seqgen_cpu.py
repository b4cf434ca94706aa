"""CPU checks of the crafted sequence streams (tests/seqgen.py): the generator's plaintext is what the oracle and the
Python restatements of the reference decode, and the model of the wave decoder says the corpus reaches every branch
of the batch path that tests/test_gpu_decoder_sequences.py is there to test."""
import os
import sys

import pytest

import seqgen as sg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "pyref"))
import zig_lz4_dict as pdict  # noqa: E402
import zig_lz4_stream_decode as psd  # noqa: E402


@pytest.fixture(scope="module")
def corpus():
    return sg.corpus()


def _status(r):
    return r if isinstance(r, int) else len(r)


def test_corpus_is_deterministic_and_sized(corpus):
    again = sg.corpus()
    assert [(i.src, i.cap, i.plain) for i in again] == [(i.src, i.cap, i.plain) for i in corpus]
    assert len(corpus) >= 6144                       # one call of the GPU test reaches the lane-copy build
    assert sum(1 for i in corpus if i.plain is None) >= 100
    lens = [len(i.src) for i in corpus]
    assert min(lens) == 66 and max(lens) <= 8192
    assert {len(i.src) for i in corpus if i.name.startswith("exact_len")} == {66, 67, 68, 69, 70}


def test_oracle_decodes_the_generator_plaintext(corpus, oracle):
    bad = []
    for k, it in enumerate(corpus):
        got, want = oracle.decompress_safe(it.src, it.cap), it.expected()
        if want is None:
            assert isinstance(got, int) and got < 0, (k, it.name)     # every malformed stream is rejected
        elif got != want:
            bad.append((k, it.name, it.cap, _status(got), _status(want)))
    assert not bad, bad[:8]


def test_pyref_agrees_on_a_subset(corpus, oracle):
    """tools/pyref/zig_lz4_stream_decode.decompress_safe (pure Python: a few hundred streams) on bytes and status,
    malformed streams included"""
    sub = corpus[::23] + [i for i in corpus if i.plain is None][::3]
    assert len(sub) >= 300
    for it in sub:
        r, out = psd.decompress_safe(it.src, it.cap)
        want = oracle.decompress_safe(it.src, it.cap)
        assert r == _status(want), it.name
        if r >= 0:
            assert out == want == it.expected()


def test_dict_corpus_matches_the_dict_restatement():
    items = sg.dict_corpus()
    bad = 0
    for it in items:
        r, out = pdict.decompress_safe_using_dict(it.src, it.cap, it.dict_bytes)
        want = it.expected()
        if want is None:
            assert r < 0, it.name
        elif isinstance(want, int):
            bad += r != want
        else:
            bad += r != len(want) or out != want
    assert bad == 0
    assert sum(1 for i in items if i.plain is None) >= 20


def _totals(items, **kw):
    tot = sg.Counts()
    for it in items:
        r, c = sg.model(it.src, it.cap, **kw)
        tot.add(c)
    return tot


@pytest.fixture(scope="module")
def lane_totals(corpus):
    return _totals(corpus, lane_copy=True, phases=True)


@pytest.fixture(scope="module")
def seq_totals(corpus):
    return _totals(corpus, lane_copy=False, phases=False)


def test_model_result_equals_the_oracle(corpus, oracle):
    for it in corpus[::7]:
        want = _status(oracle.decompress_safe(it.src, it.cap))
        for kw in (dict(lane_copy=True, phases=True), dict(lane_copy=False, phases=False),
                   dict(lane_copy=True, phases=True, min_phase_tokens=1), dict(lane_copy=False, phases=False, write=False)):
            assert sg.model(it.src, it.cap, **kw)[0] == want, (it.name, kw)


def test_coverage_floors_lane_copy_with_phases(lane_totals):
    """The floors sit a little below what the committed corpus reaches (cap cuts 3867, batches with >= 3 phases 6748,
    phase-limit exits 2357, room-cut walks 428, streams ending with a match 1630): a generator change that loses a
    family fails here."""
    t = lane_totals
    assert t.cap_cuts >= 3400
    assert t.phases3 >= 6000
    assert t.phase_limit >= 2000
    assert t.room_cuts >= 350
    assert t.ends_with_match >= 1400
    assert t.later_phases >= 25000
    for ml in range(4, 41):
        assert t.ml_hist.get(ml, 0) >= 20, ml
    for lit in range(0, 17):
        assert t.lit_hist.get(lit, 0) >= 20, lit


def test_coverage_floors_sequence_lane(seq_totals):
    t = seq_totals
    assert t.cap_cuts == 0 and t.later_phases == 0 and t.phase_limit == 0
    assert t.batches >= 55000
    assert t.room_cuts >= 600
    assert t.single_seqs >= 40000
    for ml in range(4, 41):
        assert t.ml_hist.get(ml, 0) >= 20, ml
    for lit in range(0, 17):
        assert t.lit_hist.get(lit, 0) >= 20, lit


def test_model_on_hand_made_windows():
    """Fixed windows whose grouping is known by hand."""
    pre = bytes(range(200))
    head = sg.seq(pre, 100, 4)                       # single path: the literal run needs extension bytes
    # 21 sequences of 3 bytes (ml 4, sources in the preamble), then a 100-byte tail: the lane-copy build cuts the
    # phase after the 16th short match, and the 5 left form a second phase
    s = head + b"".join(sg.seq(b"", 150, 4) for _ in range(21)) + sg.seq(bytes(100))
    r, c = sg.model(s, 10000, lane_copy=True, phases=True)
    assert r == 200 + 4 + 21 * 4 + 100
    assert (c.batches, c.cap_cuts, c.later_phases, c.batch_seqs) == (1, 1, 1, 21)
    r, c = sg.model(s, 10000, lane_copy=False, phases=False)
    assert (c.batches, c.cap_cuts, c.later_phases, c.batch_seqs) == (1, 0, 0, 21)
    r, c = sg.model(s, 10000, lane_copy=True, phases=False)
    assert (c.batches, c.cap_cuts, c.later_phases, c.batch_seqs) == (2, 1, 0, 21)
    # every match reads the one before it: one token per phase, so three batches of six phases end at the phase limit
    # and a fourth takes the last three tokens
    s = head + sg.seq(b"", 150, 4) + b"".join(sg.seq(b"", 4, 4) for _ in range(20)) + sg.seq(bytes(100))
    r, c = sg.model(s, 10000, lane_copy=True, phases=True, min_phase_tokens=1)
    assert r == 200 + 4 + 21 * 4 + 100
    assert (c.batches, c.later_phases, c.phase_limit, c.batch_seqs) == (4, 17, 3, 21)
