"""The edge corpus (tests/edgegen.py) against the oracle, no GPU: every case is compressed with every setting
tests/test_gpu_edge_corpus.py uses, the stream is walked, and the parse inside the case's probe region must be the one
the construction predicts -- so that a GPU kernel that is off by one in the comparison a family is about cannot produce
the oracle's bytes.  `_expect()` derives each parse from the case's parameters (where the copies lie, how many attempts
the level has), never from the oracle's output; the values the issue lists are pinned literally on top.

Flips are checked as pairs: the accepted twin has the stated sequence, the refused twin has none from that source and
the stated sequences instead.  Where a setting cannot show a family's decision at all, `_expect()` returns None, and
UNWITNESSED names every such (setting, family): the witness test fails if the list is not exactly what is observed.
"""
import os
import sys
from collections import defaultdict

import pytest

import edgegen as eg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "pyref"))

SETTINGS = [("fast", a) for a in eg.ACCELS] + [("hc", l) for l in eg.HC_LEVELS]
BUDGET_ONLY = [("hc", 6), ("hc", 7)]                 # levels the GPU test does not run; the budget pairs exist for 3 .. 9
FAMILIES = ("far", "pattern_far", "early_exit", "budget", "pos0")

# What a setting cannot show, by name.  Acceleration 65537 probes positions 1, 2 and 65539 of a block and nothing
# else (the step is 65537 from the third probe on), and the table then holds positions 0 .. 2 only: a source 65535
# bytes before position 65539 is never in it, so no block of this size puts any of the five decisions on that
# schedule; those batches compare bytes only.  The fast compressor and level 2 (lz4mid) have no chain walk, so no
# attempt count, early exit or pattern step; levels 10 .. 12 are outside the budget pairs (3 .. 9).
UNWITNESSED = {
    ("fast", 65537): {"far", "pattern_far", "early_exit", "budget", "pos0"},
    ("fast", 1): {"pattern_far", "early_exit", "budget"},
    ("fast", 4): {"pattern_far", "early_exit", "budget"},
    ("hc", 2): {"pattern_far", "early_exit", "budget"},
    ("hc", 10): {"budget"},
    ("hc", 11): {"budget"},
    ("hc", 12): {"budget"},
}


def _compress(oracle, b, setting):
    kind, v = setting
    return oracle.compress_fast(b, v) if kind == "fast" else oracle.compress_hc(b, v)


@pytest.fixture(scope="module")
def parses(oracle):
    """{(case name, setting): (stream length, [(pos, offset, length)] inside the probe)}, computed once"""
    out = {}
    for fam, name, b, m in eg.cases():
        for s in SETTINGS + (BUDGET_ONLY if fam == "budget" else []):
            if s[0] == "fast" and not m["fast"]:
                continue
            c = _compress(oracle, b, s)
            out[(name, s)] = (len(c), eg.in_probe(eg.walk(c), m["probe"]))
    return out


def _walk_runs(p, run_end, lowest, period, nb):
    """The chain walk from the start p of a run over the earlier run that ends at run_end: the candidates are the
    earlier run's aligned positions, nearest first (length 4, then `period` more per step), down to `lowest`; it stops
    after nb attempts or at the first match longer than nb (:571, :613).  -> (offset, length) or None"""
    best, s, n = None, run_end - 4, 0
    while s >= lowest and n < nb:
        n += 1
        best = (p - s, run_end - s)
        if run_end - s > nb:
            break
        s -= period
    return best


def _expect_pattern(m, kind, v):
    if kind == "fast" or v == 2:
        return None
    p, gap, second, period = m["probe"][0], m["gap"], m["second"], len(m["pat"])
    run_end, lowest = p - gap, p - eg.MAX_DIST
    nb = eg.ATTEMPTS[v]
    if "reach" in m:                                 # 700 'a', `reach` of them in reach, then 500 'a'
        r = m["reach"]
        if v < 9:                                    # no pattern step: the walk leaves at nb + 1 bytes
            off, ml = _walk_runs(p, run_end, lowest, 1, nb)
            assert ml == nb + 1 and off == gap + nb + 1
        elif r >= second:                            # :653 the segment covers the run at p: placed at its end
            off, ml = gap + second, second
        elif v == 12:                                # the parser prefers one literal and the run on itself
            return "accept", [(p + 1, 1, second - 1)]
        else:                                        # :660 clamped to the lowest index
            off, ml = eg.MAX_DIST, r
        tail = [(p + ml, 1, second - ml)] if second - ml >= 4 else []
        return "accept", [(p, off, ml)] + tail
    own = [(p + period, period, second - period)]    # no earlier candidate: the run matches itself one period on
    if gap + 4 > eg.MAX_DIST:                        # the nearest earlier candidate is out of reach
        return "refuse", own
    if v >= 10 and period < 4:                       # the optimal parser prefers `period` literals and one long match
        return None
    off, ml = _walk_runs(p, run_end, lowest, period, nb)
    return "accept", [(p, off, ml), (p + ml, period, second - ml)]


def _expect(fam, m, setting):
    """-> (side, the sequences that start in the probe) as the construction predicts them, or None where the setting
    does not show the family's decision on this case"""
    kind, v = setting
    p = m["probe"][0]
    if fam == "far":
        if v == 65537 or (kind == "hc" and v == 2 and m["filler"] == "rnd"):   # lz4mid's tables lose X in the filler
            return None
        return ("accept", "far") if m["accept"] else ("refuse", [])
    if fam == "pattern_far":
        return _expect_pattern(m, kind, v)
    if fam == "early_exit":
        if kind != "hc" or v != m["level"]:
            return None
        e, old, new = m["e"], m["old"], m["new"]
        if m["accept"]:
            return "accept", [(p, p - old, e + 100)]
        return "refuse", [(p, p - new, e), (p + e, p - old, 100)]
    if fam == "budget":
        if kind != "hc" or v != m["level"]:
            return None
        if m["accept"]:
            return "accept", [(p, p - m["old"], 44)]
        return "refuse", [(p, 22, 4), (p + 4, p - m["old"], 40)]           # the nearest short occurrence, then the rest
    if fam == "pos0":
        if v == 65537:
            return None
        off = p - 1 if m["accept"] else p            # the distance between the two G (116, or 46 in the first window)
        if kind == "fast" and v == 1 and off == 116:  # the step is 2 there: (120, 116, 12) has source 4, not 0
            return ("accept", [(118, 116, 15)]) if m["accept"] else ("refuse", [(120, 116, 12)])
        return ("accept", [(p, off, 16)]) if m["accept"] else ("refuse", [(p + 1, off, 15)])   # source 1, not 0
    raise AssertionError(fam)


def _check_far(m, got):
    """one sequence with offset == d that starts at the copy or a byte into it and runs to the copy's end"""
    p, hi = m["probe"]
    return len(got) == 1 and got[0][1] == m["d"] and got[0][0] in (p, p + 1) and got[0][0] + got[0][2] == hi


def test_block_sizes():
    """far / pattern_far blocks are in HBM-link, 32-bit-table territory by their size; the others fit the LDS builds"""
    for fam, name, b, _ in eg.cases():
        if fam in ("far", "pattern_far"):
            assert len(b) > 65547, name
        else:
            assert 13 <= len(b) <= 65536, name
    assert len(eg.large()) + len(eg.small()) == len(eg.cases())
    assert 400 <= len(eg.cases()) <= 600 and max(len(c[2]) for c in eg.cases()) <= 67 * 1024


def test_parses_are_the_constructed_ones(parses):
    bad = []
    for fam, name, b, m in eg.cases():
        for s in SETTINGS + (BUDGET_ONLY if fam == "budget" else []):
            if (name, s) not in parses:
                continue
            want = _expect(fam, m, s)
            if want is None:
                continue
            got = parses[(name, s)][1]
            ok = _check_far(m, got) if want[1] == "far" else got == want[1]
            if not ok:
                bad.append("%s %s: %s, expected %s" % (name, s, got, want[1]))
    assert not bad, "%d: %s" % (len(bad), "; ".join(bad[:8]))


def test_flips_come_in_pairs(parses):
    """every case with a twin: wherever one side is witnessed, so is the other, on the other side"""
    by_name = {name: (fam, m) for fam, name, _, m in eg.cases()}
    pairs = 0
    for fam, name, _, m in eg.cases():
        if "twin" not in m:
            continue
        tfam, tm = by_name[m["twin"]]
        assert tfam == fam and tm["twin"] == name and tm["accept"] != m["accept"], name
        for s in SETTINGS + BUDGET_ONLY:
            a, b = _expect(fam, m, s), _expect(fam, tm, s)
            assert (a is None) == (b is None), (name, s)
            if a is not None and (name, s) in parses:
                assert {a[0], b[0]} == {"accept", "refuse"}, (name, s)
                assert parses[(name, s)][1] != parses[(m["twin"], s)][1], (name, s)
                pairs += 1
    assert pairs >= 900


def test_every_family_is_witnessed_or_named(parses):
    seen = defaultdict(set)
    for fam, name, _, m in eg.cases():
        for s in SETTINGS:
            want = _expect(fam, m, s)
            if want is not None and (name, s) in parses:
                seen[(s, fam)].add(want[0])
    for s in SETTINGS:
        missing = {fam for fam in FAMILIES if seen[(s, fam)] != {"accept", "refuse"}}
        assert missing == UNWITNESSED.get(s, set()), (s, sorted(missing))
    for level in range(3, 10):                       # the budget pairs, levels 6 and 7 included
        k = eg.BUDGET_K[level]
        assert parses[("budget/l%d/k%d" % (level, k), ("hc", level))][1][0][2] == 44
        assert parses[("budget/l%d/k%d" % (level, k + 1), ("hc", level))][1][0][2] == 4


def test_pinned_values(parses):
    """the figures of the corpus's description, literally"""
    def at(name, s):
        p = [c for c in eg.cases() if c[1] == name][0][3]["probe"][0]
        return [(q[0] - p, q[1], q[2]) for q in parses[(name, s)][1]]

    for s in SETTINGS:                               # far, k = 0, zero filler
        if s == ("fast", 65537):
            continue
        first = (1, 47) if s[0] == "fast" else (0, 48)
        for d in (65534, 65535):
            assert at("far/zero/k0/d%d" % d, s) == [(first[0], d, first[1])], (s, d)
        for d in (65536, 65537):
            assert at("far/zero/k0/d%d" % d, s) == [], (s, d)
        grow = parses[("far/zero/k0/d65536", s)][0] - parses[("far/zero/k0/d65535", s)][0]
        assert grow == (44 if s[0] == "fast" else 45), (s, grow)     # the 47 (48) matched bytes as literals, less token + offset
    for gap in range(65520, 65532):                  # pattern a, (300, 100): the clamped match, 15 .. 4 bytes
        for level in (5, 8, 9):
            assert at("pattern_far/a/300_100/gap%d" % gap, ("hc", level))[0] == (0, 65535, 65535 - gap)
        assert at("pattern_far/a/300_100/gap%d" % gap, ("hc", 12)) == [(1, 1, 99)]
        assert at("pattern_far/ab/300_100/gap%d" % gap, ("hc", 9))[0][1] == 65534 + gap % 2
        for level in (9, 12):
            assert at("pattern_far/abcd/300_100/gap%d" % gap, ("hc", level)) == \
                at("pattern_far/abcd/300_100/gap%d" % gap, ("hc", 8))
    for gap in range(65532, 65536):
        for level in (4, 9, 12):
            assert at("pattern_far/a/300_100/gap%d" % gap, ("hc", level)) == [(1, 1, 99)]
    for r, want in ((258, (0, 65535, 258)), (499, (0, 65535, 499)), (500, (0, 65535, 500)), (501, (0, 65534, 500))):
        for level in (9, 10, 11):                    # only the pattern step finds these; level 8 leaves at 129 bytes
            assert at("pattern_far/a/deep/reach%d" % r, ("hc", level))[0] == want
        assert at("pattern_far/a/deep/reach%d" % r, ("hc", 8))[0] == (0, 65535 - r + 129, 129)
    assert at("early_exit/l12/e16384/j0", ("hc", 12)) == [(0, 32941, 16484)]
    assert [q[2] for q in at("early_exit/l12/e16385/j0", ("hc", 12))] == [16385, 100]
    for k, l40, l44 in ((5, 3, 4), (9, 4, 8)):
        assert [q[2] for q in at("budget/l%d/k%d" % (l40, k), ("hc", l40))] == [4, 40]
        assert [q[2] for q in at("budget/l%d/k%d" % (l40, k), ("hc", l44))] == [44]


def test_pyref_gives_the_same_bytes(oracle):
    """the second restatement (tools/pyref) on every early_exit case up to level 11 at its own level, every budget and
    pos0 case at every setting, and one far pair: the expected bytes do not rest on one restatement"""
    import zig_lz4_pyref as pr

    def py(b, s):
        return pr.compress_fast(b, s[1]) if s[0] == "fast" else pr.compress_hc(b, s[1])

    n = 0
    for fam, name, b, m in eg.cases():
        if fam == "early_exit" and m["level"] <= 11:
            todo = [("hc", m["level"])]
        elif fam == "budget":
            todo = [("hc", m["level"]), ("hc", 2), ("fast", 1)]
        elif fam == "pos0":
            todo = SETTINGS
        elif name in ("far/zero/k0/d65535", "far/zero/k0/d65536"):
            todo = [("fast", 1)]
        else:
            continue
        for s in todo:
            assert py(b, s) == _compress(oracle, b, s), (name, s)
            n += 1
    assert n > 250
