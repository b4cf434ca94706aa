"""The crafted long-match corpus (tests/longmatchgen.py) against the model of the wave decoder's grouping
(tests/seqgen.py model()), no GPU: which sequences a batch or a phase takes must not depend on how long their matches
are, and the corpus must actually bring its long matches into batches -- the path tests/test_gpu_decoder_long_matches.py
is about."""
import pytest

import longmatchgen as lg
import seqgen as sg

GROUPING = ("batches", "batch_seqs", "later_phases", "single_seqs")


class _PerBatch(sg.Counts):
    """Counts that also notes, each time a batch begins, how many long matches the batches before it took"""

    def __init__(self):
        self._batches, self.marks = 0, []
        super().__init__()

    @property
    def batches(self):
        return self._batches

    @batches.setter
    def batches(self, v):
        if v > self._batches:
            self.marks.append(self.longs())
        self._batches = v

    def longs(self):
        return sum(n for ml, n in self.ml_hist.items() if ml > lg.LONG)


def _streams(shorten):
    out = [(name, s, p, 0) for name, s, p in lg.streams(shorten=shorten)]
    return out + [(name, s, p, min(len(d), 65536)) for name, s, p, d in lg.dict_streams(11, shorten=shorten)]


@pytest.mark.parametrize("lane_copy", [True, False])
def test_grouping_is_the_same_with_the_long_matches_made_short(lane_copy):
    """every stream and its twin (each match of 32 bytes or more replaced by one of 19..31 in the same 4-byte
    sequence): the same batches, batched sequences, later phases and single-path sequences"""
    bad = []
    for (name, s, p, dlen), (_, s2, p2, _) in zip(_streams(False), _streams(True)):
        r1, c1 = sg.model(s, len(p) + lg.ROOMY, lane_copy, lane_copy, dlen=dlen)
        r2, c2 = sg.model(s2, len(p2) + lg.ROOMY, lane_copy, lane_copy, dlen=dlen)
        assert (r1, r2) == (len(p), len(p2)), name
        k1, k2 = [getattr(c1, f) for f in GROUPING], [getattr(c2, f) for f in GROUPING]
        if k1 != k2:
            bad.append("%s: %s, twin %s" % (name, k1, k2))
    assert not bad, "%d: %s" % (len(bad), "; ".join(bad[:6]))


def test_the_corpus_reaches_the_long_path(monkeypatch):
    """more than 90 % of the batches the lane-copy build makes of the corpus's streams hold a match of more than 32
    bytes, and every length of MLS above 32 is among them"""
    monkeypatch.setattr(sg, "Counts", _PerBatch)
    batches = with_long = 0
    seen = set()
    for name, s, p in lg.streams():
        _, c = sg.model(s, len(p) + lg.ROOMY, True, True)
        marks = c.marks + [c.longs()]
        batches += c.batches
        with_long += sum(1 for a, b in zip(marks, marks[1:]) if b > a)
        seen.update(ml for ml in c.ml_hist if ml > lg.LONG)
    assert batches >= 500 and with_long > 0.9 * batches, (with_long, batches)
    assert seen >= {ml for ml in lg.MLS if ml > lg.LONG}, sorted(seen)
